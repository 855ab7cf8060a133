#!/usr/bin/env python3
"""DAMRS's symmetric KL term: `hip_ops.mutual_kl` (csrc/mutual_kl.hip) against the model's composition (`mutual_kl_torch`: two
GEMMs, sigmoids and eight products of logs over [users, items] blocks, stock autograd) on one MI355X, in ONE process:

    forward_backward  kl = fn(U, A, B), then the gradients to all three operands

EAGER (host launches included: DAMRS's step is not replayed), HIP events around windows of calls, median / min / max over five
windows after warm-up, windows of the two paths alternating.  m users x n items: 2,048 x 4,096 (every id of a shipped batch
distinct) and the expected numbers of distinct ids of a batch of 2,048 users and 4,096 items at Amazon-Sports size and at
500,000 items.  Peak memory: one forward + backward above the resident inputs.
With `--trainer RUNS`: DAMRS's Baby-size step through the Trainer (tools/run_config.py `damrs`) at four settings -- both keys
off, `fused_labels` only, `fused_kl` only, both on -- RUNS runs each, alternated, with the peak device memory of each run.
Results as JSON (default profiles/mutual_kl_ab.json).

    python tools/mutual_kl_ab.py [out.json] [--trainer RUNS]
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

WINDOWS = 5
CALLS = 20
BATCH = 2048


def distinct(population, draws):
    """expected number of distinct ids among `draws` uniform draws from `population`"""
    return int(round(population * (1.0 - (1.0 - 1.0 / population) ** draws)))


SIZES = (("batch", BATCH, 2 * BATCH),
         ("sports", distinct(35598, BATCH), distinct(18357, 2 * BATCH)),
         ("500K", distinct(1000000, BATCH), distinct(500000, 2 * BATCH)))
SETTINGS = (("off", {}), ("fused_labels", {"fused_labels": True}), ("fused_kl", {"fused_kl": True}),
            ("both", {"fused_labels": True, "fused_kl": True}))


def eager_window(fn, calls):
    import torch
    a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(calls):
        fn()
    e.record()
    torch.cuda.synchronize()
    return a.elapsed_time(e) / calls * 1e3


def one(name, m, n):
    import numpy as np
    import torch
    import torch.nn.functional as F
    from mmrec_amd import hip_ops
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(m + n)
    U = (0.1 * torch.randn(m, 64, device=dev, generator=gen)).requires_grad_()         # xavier-sized user rows
    A = F.normalize(torch.randn(n, 64, device=dev, generator=gen)).requires_grad_()
    B = F.normalize(torch.randn(n, 64, device=dev, generator=gen)).requires_grad_()
    assert hip_ops.mutual_kl_served(U, A, B)

    def leg(fn):
        def run():
            kl = fn(U, A, B)
            return (kl,) + torch.autograd.grad(kl, (U, A, B))
        return run
    fns = (("kernel", leg(hip_ops.mutual_kl)), ("composition", leg(hip_ops.mutual_kl_torch)))
    result = {"shape": name, "m": m, "n": n, "split_cols": [hip_ops.mutual_kl_split_cols(m, n, k) for k in range(3)],
              "windows": WINDOWS, "calls_per_window": CALLS, "peak_mb_forward_backward": {}, "max_diff": {}}
    got = {}
    for k, run in fns:
        run()
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        out = run()
        torch.cuda.synchronize()
        result["peak_mb_forward_backward"][k] = (torch.cuda.max_memory_allocated() - base) / 2 ** 20
        got[k] = [t.clone() for t in out]
        del out
    for nm, a, b in zip(("kl", "dU", "dA", "dB"), got["kernel"], got["composition"]):
        result["max_diff"][nm] = [float((a - b).abs().max()), float(b.abs().max())]
    del got
    for _, run in fns:
        for _ in range(5):
            run()
    per = {k: [] for k, _ in fns}
    for _ in range(WINDOWS):
        for k, run in fns:
            per[k].append(eager_window(run, CALLS))
    med = {k: float(np.median(v)) for k, v in per.items()}
    spread = max(per["composition"]) - min(per["composition"])
    delta = med["kernel"] - med["composition"]
    result["eager_forward_backward"] = {k: {"median_us": med[k], "min_us": min(v), "max_us": max(v)} for k, v in per.items()}
    result["kernel_minus_composition_us"] = delta
    result["composition_spread_us"] = spread
    result["verdict"] = "FASTER than the spread" if -delta > spread else "SLOWER than the spread allows" if delta > spread else "no difference"
    print("%-7s m %5d n %5d  kernel %9.2f us [%.2f, %.2f]   composition %9.2f us [%.2f, %.2f]   %s;  peak MB %.2f / %.2f" % (
        name, m, n, med["kernel"], min(per["kernel"]), max(per["kernel"]), med["composition"], min(per["composition"]),
        max(per["composition"]), result["verdict"], result["peak_mb_forward_backward"]["kernel"],
        result["peak_mb_forward_backward"]["composition"]), flush=True)
    torch.cuda.empty_cache()
    return result


def trainer(runs, epochs=3):
    """DAMRS through the Trainer at Baby size, the four settings alternated -> {setting: {"ms_per_batch": [...], "peak_mb": [...]}}"""
    import torch
    from run_config import run
    out = {k: {"ms_per_batch": [], "peak_mb": []} for k, _ in SETTINGS}
    for i in range(runs):
        for k, cd in SETTINGS:
            torch.cuda.synchronize()
            torch.cuda.empty_cache()
            torch.cuda.reset_peak_memory_stats()
            ms = run("damrs", dict(cd), epochs, verbose=False)["ms_per_batch"]
            out[k]["ms_per_batch"].append(ms)
            out[k]["peak_mb"].append(torch.cuda.max_memory_allocated() / 2 ** 20)
            print("[damrs] run %d %-12s %.3f ms/batch, peak %.1f MB" % (i, k, ms, out[k]["peak_mb"][-1]), flush=True)
    for k, v in out.items():
        s = sorted(v["ms_per_batch"])
        v["median_ms_per_batch"] = s[len(s) // 2]
        print("[damrs] %-12s ms/batch median %.3f min %.3f max %.3f over %d runs" % (k, s[len(s) // 2], s[0], s[-1], len(s)), flush=True)
    off, kl = out["off"]["median_ms_per_batch"], out["fused_kl"]["median_ms_per_batch"]
    out["kl_term_share_of_the_key_off_step"] = (off - kl) / off          # what taking the composition out removes, at most
    return out


if __name__ == "__main__":
    argv = sys.argv[1:]
    runs = 0
    if "--trainer" in argv:
        i = argv.index("--trainer")
        runs = int(argv[i + 1])
        del argv[i:i + 2]
    path = argv[0] if argv else os.path.join(ROOT, "profiles", "mutual_kl_ab.json")
    results = {"what": "hip_ops.mutual_kl against the composition, eager forward + backward, device-event us per call, one MI355X",
               "ops": [one(*s) for s in SIZES]}
    if runs:
        results["damrs_trainer_baby"] = trainer(runs)
    os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
    with open(path, "w") as f:
        json.dump(results, f, indent=1)
    print("wrote", path)
