#!/usr/bin/env python3
"""One MVGAE encoder's mean and log-variance heads, the aggregations included: the kernel path (ONE spmm and
hip_ops.encoder_heads, csrc/encoder_heads.hip) against the composition (the end of GCN.forward with the `fused_heads` key off:
per head a projection, an spmm, bias, row normalisation, dropout scale, leaky-ReLU, the output Linear and the skip Linear with
its leaky-ReLU, with stock autograd) in ONE process, each leg as a hipGraph replay:

    forward           mu, logvar of one encoder from x                                                          (no autograd)
    forward_backward  the same with autograd, then the gradients of <mu, g_0> + <logvar, g_1> to x and the twelve parameters

Both legs read the same pre-drawn dropout scales (mask / keep rate), so they compute the same function.  Sizes (users + items):
Amazon-Baby 26,495, Amazon-Sports 54,255, and 1,500,000, on a random bipartite mean graph with self loops of 7 entries per
row.  HIP events around windows of replays: median / min / max over five windows after warm-up, windows of the two paths
alternating.  A leg is "faster" only when its median beats the composition's by more than the composition's own min-max spread,
"slower" when it exceeds it by more than that.  Peak memory: one eager forward + backward above the resident inputs.
With `--trainer RUNS`: MVGAE through the Trainer on synthetic Baby-shaped data (tools/run_config.py `mvgae`), RUNS runs with
`fused_heads` on and RUNS with it off, alternated, without and with `fused_posterior`.  Results as JSON (default
profiles/encoder_heads_ab.json).

    python tools/prof_encoder_heads.py [out.json] [--trainer RUNS] [--sizes baby,sports,1.5M]
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
    """a bipartite interaction graph over n = users + items rows, three interactions per row on average, as MVGAE builds it"""
    import numpy as np
    import scipy.sparse as sp
    from mmrec_amd.models.mvgae import self_loop_mean_graph
    rng = np.random.default_rng(seed)
    nu = (7 * n) // 10
    ni = n - nu
    e = 3 * n
    inter = sp.coo_matrix((np.ones(e, np.float32), (rng.integers(0, nu, e), rng.integers(0, ni, e))), shape=(nu, ni))
    inter.sum_duplicates()
    return self_loop_mean_graph(inter.tocoo(), nu, ni, device)


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
    W, b, G, bg, L, bl = lin(2, D, D), lin(2, D), lin(2, D, D), lin(2, D), lin(2, D, D), lin(2, D)
    params = [W, b, G, bg, L, bl]
    scale = (torch.rand(2, n, D, device=dev, generator=gen) < 0.9).float() / 0.9
    g = r(2, n, D)

    def kernel():
        ax = hip_ops.spmm(graph, x)
        return hip_ops.encoder_heads(ax, x, W, b, G, bg, L, bl, scale)

    def composition():
        outs = []
        for h in range(2):                                               # BaseModel.forward and the two lines of GCN.forward
            xw = hip_ops.linear(x, W[h].t().contiguous(), None)
            conv = F.normalize(hip_ops.spmm(graph, xw) + b[h], p=2, dim=-1) * scale[h]
            outs.append(hip_ops.linear(F.leaky_relu(conv), G[h], bg[h]) + F.leaky_relu(hip_ops.linear(x, L[h], bl[h])))
        return torch.stack(outs)

    with torch.no_grad():
        assert hip_ops.encoder_heads_served(hip_ops.spmm(graph, x), x, W, b, G, bg, L, bl, scale)
    paths = (("kernel", kernel), ("composition", composition))

    def forward(fn):
        def run():
            with torch.no_grad():
                return (fn(),)
        return run

    def forward_backward(fn):
        return lambda: torch.autograd.grad((fn() * g).sum(), [x] + params)

    result = {"shape": name, "n_rows": n, "nnz": int(graph.nnz), "rows_per_block": hip_ops.encoder_heads_rows_per_block(n),
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
    names = ("out", "dx", "dW", "db", "dG", "dbg", "dL", "dbl")
    for nm, a, c in zip(names, got["kernel"], got["composition"]):
        result["max_diff"][nm] = [float((a - c).abs().max()), float(c.abs().max())]
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


def trainer(runs, posterior, epochs=3):
    """MVGAE through the Trainer at Baby size, the key on and off alternated -> {"on": [...], "off": [...]} ms per batch"""
    from run_config import run
    ms = {"on": [], "off": []}
    for i in range(2 * runs):
        on = i % 2 == 0
        ms["on" if on else "off"].append(run("mvgae", dict(fused_heads=on, fused_posterior=posterior), epochs,
                                             verbose=False)["ms_per_batch"])
        print("[mvgae] run %d fused_posterior %s fused_heads %s: %.3f ms/batch" % (i // 2, posterior, on, ms["on" if on else "off"][-1]),
              flush=True)
    for k, v in ms.items():
        s = sorted(v)
        print("[mvgae] fused_posterior %s fused_heads %-3s ms/batch median %.3f min %.3f max %.3f over %d runs" % (
            posterior, k, s[len(s) // 2], s[0], s[-1], len(s)), flush=True)
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
    path = argv[0] if argv else os.path.join(ROOT, "profiles", "encoder_heads_ab.json")
    results = {"ops": [one(*s) for s in sizes]}
    if runs:
        results["mvgae_trainer_ms_per_batch_baby"] = {"posterior_off": trainer(runs, False), "posterior_on": trainer(runs, True)}
    with open(path, "w") as f:
        json.dump(results, f, indent=1)
    print("wrote", path)
