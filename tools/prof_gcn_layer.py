#!/usr/bin/env python3
"""One 64-wide layer of MMGCN's GCN.forward, the aggregation included: the kernel path (ONE spmm of x and hip_ops.gcn_layer,
csrc/gcn_layer.hip) against the composition (the loop body of GCN.forward with the `fused_layers` key off: the projection x Wc,
its spmm, the skip projection, `cat_leaky`, the 128 -> 64 projection and its leaky-ReLU, with stock autograd) in ONE process,
each leg as a hipGraph replay:

    forward           the layer's output from x                                                                   (no autograd)
    forward_backward  the same with autograd, then the gradients of <out, g> to x and the five parameters

Sizes (users + items): Amazon-Baby 26,495, Amazon-Sports 54,255, and 1,500,000, on a random bipartite mean-aggregation graph
(models/mmgcn.py `mean_aggregation_graph`) of three interactions per row.  HIP events around windows of replays: median / min /
max over five windows after warm-up, windows of the two paths alternating.  A leg is "faster" only when its median beats the
composition's by more than the composition's own min-max spread, "slower" when it exceeds it by more than that.  Peak memory:
one eager forward + backward above the resident inputs.
With `--trainer RUNS`: MMGCN through the Trainer on synthetic Baby-shaped data (tools/run_config.py `mmgcn`), RUNS runs with
`fused_layers` on and RUNS with it off, alternated.  Results as JSON (default profiles/gcn_layer_ab.json).

    python tools/prof_gcn_layer.py [out.json] [--trainer RUNS] [--sizes baby,sports,1.5M]
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from prof_hyper import captured, window  # noqa: E402

WINDOWS = 5
SIZES = (("baby", 26495, 50), ("sports", 54255, 50), ("1.5M", 1500000, 3))
D = 64


def mean_graph(n, device, seed):
    """a bipartite interaction graph over n = users + items rows, three interactions per row on average, as MMGCN builds it"""
    import numpy as np
    import scipy.sparse as sp
    from mmrec_amd.models.mmgcn import mean_aggregation_graph
    rng = np.random.default_rng(seed)
    nu = (7 * n) // 10
    ni = n - nu
    e = 3 * n
    inter = sp.coo_matrix((np.ones(e, np.float32), (rng.integers(0, nu, e), rng.integers(0, ni, e))), shape=(nu, ni))
    inter.sum_duplicates()
    return mean_aggregation_graph(inter.tocoo(), nu, ni, device)


def one(name, n, replays):
    import numpy as np
    import torch
    import torch.nn.functional as F
    from mmrec_amd import hip_ops
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(n)
    r = lambda *s: torch.randn(*s, device=dev, generator=gen)            # noqa: E731
    lin = lambda *s: ((torch.rand(*s, device=dev, generator=gen) - 0.5) * 0.25).requires_grad_()     # noqa: E731
    graph = mean_graph(n, dev, n)
    x = F.normalize(r(n, D)).requires_grad_()
    ident = r(n, D) * 0.1                                                # the id embedding: a plain tensor, never trained
    Wc, Wl, bl, Wg, bg = lin(D, D), lin(D, D), lin(D), lin(D, 2 * D), lin(D)
    params = [Wc, Wl, bl, Wg, bg]
    g = r(n, D)

    def kernel():
        return hip_ops.gcn_layer(hip_ops.spmm(graph, x), x, ident, Wc, Wl, bl, Wg, bg)

    def composition():                                                   # _Conv.forward and the loop body of GCN.forward
        h = hip_ops.spmm(graph, hip_ops.linear(x, Wc.t().contiguous(), None))
        return F.leaky_relu(hip_ops.linear(hip_ops.cat_leaky(h, hip_ops.linear(x, Wl, bl), ident), Wg, bg))

    with torch.no_grad():
        assert hip_ops.gcn_layer_served(hip_ops.spmm(graph, x), x, ident, Wc, Wl, bl, Wg, bg)
    paths = (("kernel", kernel), ("composition", composition))

    def forward(fn):
        def run():
            with torch.no_grad():
                return (fn(),)
        return run

    def forward_backward(fn):
        return lambda: torch.autograd.grad((fn() * g).sum(), [x] + params)

    result = {"shape": name, "n_rows": n, "nnz": int(graph.nnz), "rows_per_block": hip_ops.gcn_layer_rows_per_block(n),
              "windows": WINDOWS, "replays_per_window": replays, "legs": {}, "peak_mb_forward_backward": {}, "max_diff": {}}
    got = {}
    for k, fn in paths:
        run = forward_backward(fn)
        run()
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        out = run()
        torch.cuda.synchronize()
        result["peak_mb_forward_backward"][k] = (torch.cuda.max_memory_allocated() - base) / 2 ** 20
        got[k] = [t.clone() for t in forward(fn)()] + [t.clone() for t in out]
        del out
    names = ("out", "dx", "dWc", "dWl", "dbl", "dWg", "dbg")
    for nm, a, c in zip(names, got["kernel"], got["composition"]):
        result["max_diff"][nm] = [float((a - c).abs().max()), float(c.abs().max())]
    # a leaky-ReLU whose argument the two rounding orders put on either side of 0 moves one whole row of dx (and one term of every
    # weight gradient): the rows of dx that differ by more than 1e-5 of dx's range, and the largest difference in all other rows
    row_diff = (got["kernel"][1] - got["composition"][1]).abs().amax(dim=1)
    moved = row_diff > 1e-5 * got["composition"][1].abs().max()
    result["dx_rows_moved"] = int(moved.sum())
    result["dx_max_diff_other_rows"] = float(row_diff[~moved].max())
    print("%-7s dx: %d of %d rows differ by more than 1e-5 of its range %.3g; largest difference in the other rows %.3g" % (
        name, result["dx_rows_moved"], n, result["max_diff"]["dx"][1], result["dx_max_diff_other_rows"]), flush=True)
    del got
    for leg, wrap in (("forward", forward), ("forward_backward", forward_backward)):
        graphs = tuple((k, captured(wrap(fn))) for k, fn in paths)
        per = {k: [] for k, _ in graphs}
        for _ in range(WINDOWS):
            for k, gr in graphs:
                per[k].append(window(gr, replays))
        med = {k: float(np.median(v)) for k, v in per.items()}
        spread = max(per["composition"]) - min(per["composition"])
        entry = {k: {"median_us": med[k], "min_us": min(v), "max_us": max(v)} for k, v in per.items()}
        delta = med["kernel"] - med["composition"]
        entry["kernel_minus_composition_us"] = delta
        entry["composition_spread_us"] = spread
        entry["verdict"] = "FASTER than the spread" if -delta > spread else "SLOWER than the spread allows" if delta > spread else "no difference"
        result["legs"][leg] = entry
        print("%-7s %-17s kernel %9.2f us [%.2f, %.2f]   composition %9.2f us [%.2f, %.2f]   %s" % (
            name, leg, med["kernel"], min(per["kernel"]), max(per["kernel"]), med["composition"], min(per["composition"]),
            max(per["composition"]), entry["verdict"]), flush=True)
        del graphs
    print("%-7s peak MB of forward + backward: kernel %.2f  composition %.2f" % (
        name, result["peak_mb_forward_backward"]["kernel"], result["peak_mb_forward_backward"]["composition"]), flush=True)
    del graph
    torch.cuda.empty_cache()
    return result


def trainer(runs, epochs=3):
    """MMGCN through the Trainer at Baby size, the key on and off alternated -> {"on": [...], "off": [...]} ms per batch"""
    from run_config import run
    ms = {"on": [], "off": []}
    for i in range(2 * runs):
        on = i % 2 == 0
        ms["on" if on else "off"].append(run("mmgcn", dict(fused_layers=on), epochs, verbose=False)["ms_per_batch"])
        print("[mmgcn] run %d fused_layers %s: %.3f ms/batch" % (i // 2, on, ms["on" if on else "off"][-1]), flush=True)
    for k, v in ms.items():
        s = sorted(v)
        print("[mmgcn] fused_layers %-3s ms/batch median %.3f min %.3f max %.3f over %d runs" % (k, s[len(s) // 2], s[0], s[-1], len(s)),
              flush=True)
    return ms


if __name__ == "__main__":
    argv = sys.argv[1:]
    runs = 0
    if "--trainer" in argv:
        i = argv.index("--trainer")
        runs = int(argv[i + 1])
        del argv[i:i + 2]
    sizes = SIZES
    if "--sizes" in argv:                                                # e.g. --sizes baby,sports
        i = argv.index("--sizes")
        sizes = tuple(s for s in SIZES if s[0] in argv[i + 1].split(","))
        del argv[i:i + 2]
    path = argv[0] if argv else os.path.join(ROOT, "profiles", "gcn_layer_ab.json")
    results = {"ops": [one(*s) for s in sizes]}
    if runs:
        results["mmgcn_trainer_ms_per_batch_baby"] = trainer(runs)
    with open(path, "w") as f:
        json.dump(results, f, indent=1)
    print("wrote", path)
