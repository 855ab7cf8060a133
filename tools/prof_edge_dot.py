#!/usr/bin/env python3
"""Per-edge dot products (SDDMM): the kernel path (hip_ops.EDGE_DOT on) against the gather-multiply-reduce composition
(the switch off: `(A[rows] * B[cols]).sum(-1)` and stock autograd) in ONE process, each leg as a hipGraph replay:

    forward            out = edge_dot(A, A, rows, cols)
    backward atomic    d out / d A by mmrec_edge_dot_bwd_f32 (fp32 atomics into a zeroed table)
    backward dyn       d out / d A as two SpMMs over the DynGraph of the edges (fixed order)
    backward off       autograd's backward of the composition (zero-filled [n_edges, d] buffers + index_put scatters)
    spmm_vals bwd      dX and d vals of spmm_vals(dyn, X, vals): d vals by the kernel / by the composition

Shapes: GRCN at Amazon-Baby shape -- both directions of the synthetic Baby training interactions over the 26,495 nodes,
d = 64 -- and LATTICE's 7,050 x 10 kNN pairs, d = 64.  HIP events around windows of replays: median / min / max over five
windows after warm-up, windows of the two paths alternating.  A leg is "slower" when its median exceeds the composition's by
more than the composition's own min-max spread.  Results as JSON (default profiles/edge_dot_ab.json).

    python tools/prof_edge_dot.py [out.json]
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WINDOWS, REPLAYS = 5, 100


def captured(fn):
    import torch
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(5):
            fn()
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            fn()
    torch.cuda.current_stream().wait_stream(side)
    for _ in range(10):
        graph.replay()
    return graph


def window(graph):
    import torch
    a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(REPLAYS):
        graph.replay()
    e.record()
    torch.cuda.synchronize()
    return a.elapsed_time(e) / REPLAYS * 1e3


def shapes():
    import numpy as np
    from mmrec_amd.synth import shaped_edges
    nu, ni, eu, ei = shaped_edges("baby")
    src, dst = np.concatenate([eu, ei + nu]), np.concatenate([ei + nu, eu])
    rng = np.random.default_rng(0)
    knn_rows = np.repeat(np.arange(7050), 10)
    return (("grcn_baby", nu + ni, dst, src), ("lattice_knn", 7050, knn_rows, rng.integers(0, 7050, knn_rows.size)))


def one(name, n, rows_h, cols_h, d=64):
    import numpy as np
    import torch
    from mmrec_amd import hip_ops
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(0)
    rows, cols = torch.from_numpy(rows_h).to(dev), torch.from_numpy(cols_h).to(dev)
    ne = rows.numel()
    A = (torch.rand(n, d, device=dev, generator=gen) - 0.5).requires_grad_()
    g = torch.rand(ne, device=dev, generator=gen) - 0.5
    vals = (torch.rand(ne, device=dev, generator=gen) - 0.5).requires_grad_()
    dY = torch.rand(n, d, device=dev, generator=gen) - 0.5
    dyn = hip_ops.DynGraph(rows, cols, n, n)
    assert hip_ops.edge_dot_served(A, A, rows, cols)

    def with_switch(on, fn):
        def run():
            hip_ops.EDGE_DOT = on
            try:
                return fn()
            finally:
                hip_ops.EDGE_DOT = True
        return run

    def forward():
        with torch.no_grad():
            return hip_ops.edge_dot(A, A, rows, cols)

    def backward_of(on, use_dyn):
        hip_ops.EDGE_DOT = on
        out = hip_ops.edge_dot(A, A, rows, cols, dyn=dyn if use_dyn else None)
        hip_ops.EDGE_DOT = True
        return lambda: torch.autograd.grad(out, A, g, retain_graph=True)

    y = hip_ops.spmm_vals(dyn, A, vals)

    def vals_bwd():
        return torch.autograd.grad(y, (A, vals), dY, retain_graph=True)
    legs = (("forward", with_switch(True, forward), with_switch(False, forward)),
            ("backward_atomic", backward_of(True, False), backward_of(False, False)),
            ("backward_dyn", backward_of(True, True), backward_of(False, False)),
            ("spmm_vals_backward", with_switch(True, vals_bwd), with_switch(False, vals_bwd)))
    result = {"shape": name, "n_nodes": int(n), "n_edges": int(ne), "d": d, "max_edges_on_a_row": int(np.bincount(rows_h).max()),
              "windows": WINDOWS, "replays_per_window": REPLAYS, "legs": {}}
    for leg, on, off in legs:
        graphs = (("kernel", captured(on)), ("composition", captured(off)))
        per = {k: [] for k, _ in graphs}
        for _ in range(WINDOWS):
            for k, graph in graphs:
                per[k].append(window(graph))
        med = {k: float(np.median(v)) for k, v in per.items()}
        spread = max(per["composition"]) - min(per["composition"])
        entry = {k: {"median_us": med[k], "min_us": min(v), "max_us": max(v)} for k, v in per.items()}
        entry["kernel_minus_composition_us"] = med["kernel"] - med["composition"]
        entry["composition_spread_us"] = spread
        entry["verdict"] = "SLOWER than the spread allows" if med["kernel"] - med["composition"] > spread else "not slower"
        if leg == "forward":                # two rows of d floats read, two ids read, one float written per edge
            entry["kernel_logical_bytes_per_s"] = ne * (2 * d * 4 + 16 + 4) / (med["kernel"] * 1e-6)
        result["legs"][leg] = entry
        print("%-12s %-19s kernel %8.2f us [%.2f, %.2f]   composition %8.2f us [%.2f, %.2f]   %s" % (
            name, leg, med["kernel"], min(per["kernel"]), max(per["kernel"]), med["composition"], min(per["composition"]),
            max(per["composition"]), entry["verdict"]), flush=True)
        del graphs
    torch.cuda.empty_cache()
    return result


if __name__ == "__main__":
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "edge_dot_ab.json")
    results = [one(*s) for s in shapes()]
    with open(path, "w") as f:
        json.dump(results, f, indent=1)
    print("wrote", path)
