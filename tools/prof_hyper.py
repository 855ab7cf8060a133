#!/usr/bin/env python3
"""LGMRec's hypergraph message passing for one modality: the kernel path (hip_ops.HYPER on: hyper_assign + hyper_propagate,
csrc/hypergraph.hip) against the torch composition (the switch off: `hyper_assign_torch` + `hyper_layer_torch`, i.e. today's
softmax / dropout chain and three torch.mm per layer with stock autograd) in ONE process, each leg as a hipGraph replay:

    forward           P_i, P_u = assign(logits, noise, mask);  U', X' = propagate(P_i, P_u, E)            (no autograd)
    forward_backward  the same with autograd, then the gradients of <U', w_u> + <X', w_x> to both logits and E
    layer_forward     hyper_layer(P_i, P_u, E) alone: its achieved bytes / s against the algorithmic traffic
                      4 B x 64 x (2 I + U) (E read, X' and U' written) + 4 B x H x (I + U) (the assignments)

Sizes (I items, U users), H = 4, tau = 0.2, keep rate 0.5, one layer: Amazon-Baby 7,050 / 19,445, Amazon-Sports 18,357 /
35,598, and the 500,000 / 1,000,000 table of config 5.  `--hyper-num 64` takes the 64-hyperedge family (hyper64_assign +
hyper64_propagate, csrc/hypergraph64.hip) against the same composition; `--layers`, `--keep` and `--sizes` (names of the table
below, among them Amazon-Clothing's 23,033 / 39,387) set the rest: Clothing's setting is `--hyper-num 64 --layers 2 --keep 0.2`.  HIP events around windows of replays: median / min / max over five
windows after warm-up, windows of the two paths alternating.  A leg is "slower" when its median exceeds the composition's by more
than the composition's own min-max spread.  Peak memory: one eager forward + backward above the resident inputs.  Results as JSON
(default profiles/hyper_ab.json).

    python tools/prof_hyper.py [out.json] [--hyper-num H] [--layers L] [--keep Q] [--sizes baby,clothing,...]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WINDOWS = 5
SIZES = (("baby", 7050, 19445, 200), ("sports", 18357, 35598, 200), ("config5", 500000, 1000000, 20))
MORE_SIZES = (("clothing", 23033, 39387, 200),)      # by name only (--sizes)
H, TAU, KEEP, LAYERS, D = 4, 0.2, 0.5, 1, 64


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


def one(name, I, U, replays):
    import numpy as np
    import torch
    from mmrec_amd import hip_ops
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(I + U)
    r = lambda *s: torch.randn(*s, device=dev, generator=gen)            # noqa: E731
    a_i, a_u, E = r(I, H).requires_grad_(), r(U, H).requires_grad_(), (r(I, D) * 0.1).requires_grad_()
    g_i, g_u = (-torch.empty(n, H, device=dev).exponential_(generator=gen).log() for n in (I, U))
    m_i, m_u = (torch.bernoulli(torch.full((n, H), KEEP, device=dev), generator=gen) for n in (I, U))
    w_u, w_x = r(U, D), r(I, D)
    wide = H == hip_ops.HYPER64_H
    assign, propagate, layer, assign_served, layer_served = (
        (hip_ops.hyper64_assign, hip_ops.hyper64_propagate, hip_ops.hyper64_layer, hip_ops.hyper64_assign_served,
         hip_ops.hyper64_layer_served) if wide else
        (hip_ops.hyper_assign, hip_ops.hyper_propagate, hip_ops.hyper_layer, hip_ops.hyper_assign_served, hip_ops.hyper_layer_served))
    assert assign_served(a_i, g_i, m_i) and layer_served(a_i.detach(), a_u.detach(), E.detach())

    def with_switch(on, fn):
        def run():
            hip_ops.HYPER = on
            try:
                return fn()
            finally:
                hip_ops.HYPER = True
        return run

    def forward_value():
        P_i, P_u = assign(a_i, g_i, m_i, TAU, KEEP), assign(a_u, g_u, m_u, TAU, KEEP)
        return propagate(P_i, P_u, E, LAYERS)

    def forward():
        with torch.no_grad():
            return forward_value()

    def forward_backward():
        uo, xo = forward_value()
        return torch.autograd.grad((uo * w_u).sum() + (xo * w_x).sum(), (a_i, a_u, E))

    with torch.no_grad():
        P_i0, P_u0 = hip_ops.hyper_assign_torch(a_i, g_i, m_i, TAU, KEEP), hip_ops.hyper_assign_torch(a_u, g_u, m_u, TAU, KEEP)

    def layer_forward():
        with torch.no_grad():
            return layer(P_i0, P_u0, E)

    result = {"shape": name, "n_items": I, "n_users": U, "hyper_num": H, "layers": LAYERS, "keep_rate": KEEP, "windows": WINDOWS,
              "replays_per_window": replays, "legs": {}, "peak_mb_forward_backward": {}, "max_diff": {}}
    got = {}
    for k, on in (("kernel", True), ("composition", False)):
        run = with_switch(on, forward_backward)
        run()
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        out = run()
        torch.cuda.synchronize()
        result["peak_mb_forward_backward"][k] = (torch.cuda.max_memory_allocated() - base) / 2 ** 20
        got[k] = [t.clone() for t in with_switch(on, forward)()] + [t.clone() for t in out]
        del out
    for nm, a, b in zip(("U_out", "X_out", "d_logits_i", "d_logits_u", "d_E"), got["kernel"], got["composition"]):
        result["max_diff"][nm] = [float((a - b).abs().max()), float(b.abs().max())]
    del got
    traffic = 4 * D * (2 * I + U) + 4 * H * (I + U)
    for leg, fn in (("forward", forward), ("forward_backward", forward_backward), ("layer_forward", layer_forward)):
        graphs = (("kernel", captured(with_switch(True, fn))), ("composition", captured(with_switch(False, fn))))
        per = {k: [] for k, _ in graphs}
        for _ in range(WINDOWS):
            for k, graph in graphs:
                per[k].append(window(graph, replays))
        med = {k: float(np.median(v)) for k, v in per.items()}
        spread = max(per["composition"]) - min(per["composition"])
        entry = {k: {"median_us": med[k], "min_us": min(v), "max_us": max(v)} for k, v in per.items()}
        entry["kernel_minus_composition_us"] = med["kernel"] - med["composition"]
        entry["composition_spread_us"] = spread
        entry["verdict"] = "SLOWER than the spread allows" if med["kernel"] - med["composition"] > spread else "not slower"
        if leg == "layer_forward":
            entry["algorithmic_bytes"] = traffic
            entry["kernel_bytes_per_s"] = traffic / (med["kernel"] * 1e-6)
            entry["composition_bytes_per_s"] = traffic / (med["composition"] * 1e-6)
        result["legs"][leg] = entry
        print("%-8s %-17s kernel %9.2f us [%.2f, %.2f]   composition %9.2f us [%.2f, %.2f]   %s" % (
            name, leg, med["kernel"], min(per["kernel"]), max(per["kernel"]), med["composition"], min(per["composition"]),
            max(per["composition"]), entry["verdict"]), flush=True)
        del graphs
    print("%-8s peak MB of forward + backward: kernel %.2f  composition %.2f;  layer forward %.0f GB/s of algorithmic traffic" % (
        name, result["peak_mb_forward_backward"]["kernel"], result["peak_mb_forward_backward"]["composition"],
        result["legs"]["layer_forward"]["kernel_bytes_per_s"] / 1e9), flush=True)
    torch.cuda.empty_cache()
    return result


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("out", nargs="?", default=os.path.join(ROOT, "profiles", "hyper_ab.json"))
    ap.add_argument("--hyper-num", type=int, default=H)
    ap.add_argument("--layers", type=int, default=LAYERS)
    ap.add_argument("--keep", type=float, default=KEEP)
    ap.add_argument("--sizes", default=",".join(s[0] for s in SIZES))
    args = ap.parse_args()
    path, H, LAYERS, KEEP = args.out, args.hyper_num, args.layers, args.keep
    table = {s[0]: s for s in SIZES + MORE_SIZES}
    results = [one(*table[n]) for n in args.sizes.split(",")]
    with open(path, "w") as f:
        json.dump(results, f, indent=1)
    print("wrote", path)
