#!/usr/bin/env python3
"""Edge dropout inside the SpMM (hip_ops.spmm_edge_dropout / lightgcn_mean_edge_dropout: mmrec_edge_keep_bits +
mmrec_spmm_csr_masked_f32, dropped entries never gathered) against the composition it replaces (hip_ops.EDGE_DROPOUT off:
`spmm_vals` on (vals * keep) * scale per layer, stack().mean()) in ONE process, each leg as a hipGraph replay:

    layer_forward            Y = spmm_edge_dropout(eg, X, keep, scale)
    layer_forward_backward   the same + d / d X of sum(Y dY)
    mean2_forward_backward   lightgcn_mean_edge_dropout(eg, E0, 2, keep, scale) + d / d E0   (the encoder's dropout branch, L = 2)
    pack                     mmrec_edge_keep_bits alone, both orders in one launch (no composition twin)

at dropout rates 0.1, 0.5 and 0.9 (scale = 1 / (1 - rate)), d = 64, on the symmetric normalised [users; items] adjacency of the
synthetic Amazon-Baby-shaped graph and of the config-5 graph (1.5 M nodes, 20 M entries).  HIP events around windows of
replays: median / min / max over five windows after warm-up, windows of the two paths alternating.  A leg is "slower" when
its median exceeds the composition's by more than the composition's own min-max spread.  Results as JSON (default
profiles/edge_dropout_ab.json).

    python tools/prof_edge_dropout.py [out.json] [--shapes baby,c5]
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.prof_edge_dot import captured  # noqa: E402

WINDOWS = 5
RATES = (0.1, 0.5, 0.9)
REPLAYS = {"baby": 100, "c5": 10}


def window(graph, replays):
    import torch
    a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(replays):
        graph.replay()
    e.record()
    torch.cuda.synchronize()
    return a.elapsed_time(e) / replays * 1e3


def with_switch(on, fn):
    from mmrec_amd import hip_ops

    def run():
        hip_ops.EDGE_DROPOUT = on
        try:
            return fn()
        finally:
            hip_ops.EDGE_DROPOUT = True
    return run


def stats(v):
    import numpy as np
    return {"median_us": float(np.median(v)), "min_us": min(v), "max_us": max(v)}


def measure(name, leg, rate, fused, composed, replays, legs):
    graphs = (("fused", captured(fused)), ("composition", captured(composed)))
    per = {k: [] for k, _ in graphs}
    for _ in range(WINDOWS):
        for k, graph in graphs:
            per[k].append(window(graph, replays))
    entry = {k: stats(v) for k, v in per.items()}
    diff = entry["fused"]["median_us"] - entry["composition"]["median_us"]
    spread = max(per["composition"]) - min(per["composition"])
    entry["fused_minus_composition_us"], entry["composition_spread_us"] = diff, spread
    entry["verdict"] = "SLOWER than the spread allows" if diff > spread else "not slower"
    entry["faster_by_more_than_the_spread"] = bool(-diff > spread)
    legs[leg] = entry
    print("%-5s %-30s fused %9.2f us [%.2f, %.2f]   composition %9.2f us [%.2f, %.2f]   %s" % (
        name, "%s rate %.1f" % (leg, rate), entry["fused"]["median_us"], min(per["fused"]), max(per["fused"]), entry["composition"]["median_us"],
        min(per["composition"]), max(per["composition"]), entry["verdict"]), flush=True)


def one(name):
    import numpy as np
    import torch
    from mmrec_amd import hip_ops
    from mmrec_amd.synth import shaped_edges, sym_norm_coo
    dev = torch.device("cuda:0")
    nu, ni, eu, ei = shaped_edges(name)
    r, c, val = sym_norm_coo(eu, ei, nu, ni)
    n = nu + ni
    rows, cols = torch.from_numpy(np.ascontiguousarray(r, np.int64)).to(dev), torch.from_numpy(np.ascontiguousarray(c, np.int64)).to(dev)
    dyn = hip_ops.DynGraph(rows, cols, n, n)
    eg = hip_ops.EdgeDropoutGraph(dyn, torch.from_numpy(np.asarray(val, np.float32)).to(dev))
    gen = torch.Generator(device=dev).manual_seed(0)
    X = (torch.rand(n, 64, device=dev, generator=gen) - 0.5).requires_grad_()
    dY = torch.rand(n, 64, device=dev, generator=gen) - 0.5
    replays = REPLAYS.get(name, 20)
    result = {"shape": name, "n_nodes": int(n), "n_entries": int(rows.numel()), "d": 64, "long_row_threshold": dyn.fwd.long_row_threshold,
              "long_rows": dyn.fwd.n_long, "chunks": dyn.fwd.n_chunks, "windows": WINDOWS, "replays_per_window": replays,
              "rates": {}}
    assert hip_ops.edge_dropout_served(eg, X)
    for rate in RATES:
        keep = torch.rand(rows.numel(), device=dev, generator=gen) >= rate
        scale = 1.0 / (1.0 - rate)

        def layer_forward():
            with torch.no_grad():
                return hip_ops.spmm_edge_dropout(eg, X, keep, scale)

        def layer_forward_backward():
            return torch.autograd.grad(hip_ops.spmm_edge_dropout(eg, X, keep, scale), X, dY)

        def mean2_forward_backward():
            return torch.autograd.grad(hip_ops.lightgcn_mean_edge_dropout(eg, X, 2, keep, scale), X, dY)
        a, b = layer_forward(), with_switch(False, layer_forward)()
        assert torch.equal(a, b), "the fused layer differs from the zero-valued form"
        legs = {"kept_fraction": float(keep.float().mean())}
        for leg, fn in (("layer_forward", layer_forward), ("layer_forward_backward", layer_forward_backward),
                        ("mean2_forward_backward", mean2_forward_backward)):
            measure(name, leg, rate, with_switch(True, fn), with_switch(False, fn), replays, legs)
        pack = captured(lambda: hip_ops.edge_keep_bits(keep, dyn.perm, dyn.perm_t))
        legs["pack"] = stats([window(pack, replays) for _ in range(WINDOWS)])
        print("%-5s %-30s %9.2f us [%.2f, %.2f]" % (name, "pack rate %.1f" % rate, legs["pack"]["median_us"], legs["pack"]["min_us"],
                                                    legs["pack"]["max_us"]), flush=True)
        result["rates"]["%.1f" % rate] = legs
    del eg, dyn
    torch.cuda.empty_cache()
    return result


if __name__ == "__main__":
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    names = ("baby", "c5")
    if "--shapes" in sys.argv:
        names = tuple(sys.argv[sys.argv.index("--shapes") + 1].split(","))
        args = [a for a in args if a != ",".join(names)]
    path = args[0] if args else os.path.join(ROOT, "profiles", "edge_dropout_ab.json")
    results = [one(s) for s in names]
    with open(path, "w") as f:
        json.dump(results, f, indent=1)
    print("wrote", path)
