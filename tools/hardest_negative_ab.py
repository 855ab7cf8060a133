#!/usr/bin/env python3
"""MVGAE's reconstruction term: the kernel path (hip_ops.HARDEST_NEGATIVE on: hardest_negative_loss, csrc/hardest_neg.hip) against
the torch composition (the switch off: `hardest_negative_loss_torch`, recon_loss's lines with stock autograd) in ONE process:

    forward_backward  loss = hardest_negative_loss(Z, users, pos, neg), then the gradient of <loss, w> to Z

L = 4 latents, B = 2,048 (the shipped train_batch_size), N (users + items): Amazon-Baby 26,495, Amazon-Sports 54,255, and
1,500,000; each leg EAGER (host launches included: MVGAE's step is not graph-capturable) and as a hipGraph replay.  HIP events
around windows of calls: median / min / max over five windows after warm-up, windows of the two paths alternating.  A leg is
"faster" only when its median beats the composition's by more than the composition's own min-max spread, "slower" when it
exceeds it by more than that.  Peak memory: one eager forward + backward above the resident inputs.
With `--trainer RUNS`: MVGAE through the Trainer on synthetic Baby-shaped data (tools/run_config.py `mvgae`), RUNS runs with
`fused_recon` on and RUNS with it off, alternated -- once with fused_posterior and fused_heads on, once with them off.
Results as JSON (default profiles/hardest_negative_ab.json).

    python tools/hardest_negative_ab.py [out.json] [--trainer RUNS] [--sizes baby,sports]
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from prof_hyper import captured, window  # noqa: E402

WINDOWS = 5
SIZES = (("baby", 26495, 50), ("sports", 54255, 50), ("1.5M", 1500000, 5))
L, B, D = 4, 2048, 64


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


def one(name, n, calls):
    import numpy as np
    import torch
    from mmrec_amd import hip_ops
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(n)
    Z = torch.randn(L, n, D, device=dev, generator=gen).requires_grad_()
    users, pos, neg = (torch.randint(0, n, (B,), device=dev, generator=gen) for _ in range(3))
    w = torch.tensor([1.0, 0.5, 2.0, 1.5], device=dev)
    assert hip_ops.hardest_negative_loss_served(Z, users, pos, neg)

    def with_switch(on):
        def run():
            hip_ops.HARDEST_NEGATIVE = on
            try:
                loss = hip_ops.hardest_negative_loss(Z, users, pos, neg)
                return loss, torch.autograd.grad((loss * w).sum(), Z)[0]
            finally:
                hip_ops.HARDEST_NEGATIVE = True
        return run

    result = {"shape": name, "n_rows": n, "L": L, "B": B, "split_cols": hip_ops.hardest_negative_split_cols(B, L),
              "windows": WINDOWS, "calls_per_window": calls, "legs": {}, "peak_mb_forward_backward": {}, "max_diff": {}}
    got = {}
    for k, on in (("kernel", True), ("composition", False)):
        run = with_switch(on)
        run()
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        out = run()
        torch.cuda.synchronize()
        result["peak_mb_forward_backward"][k] = (torch.cuda.max_memory_allocated() - base) / 2 ** 20
        got[k] = [t.clone() for t in out]
        del out
    for nm, a, b in zip(("loss", "dZ"), got["kernel"], got["composition"]):
        result["max_diff"][nm] = [float((a - b).abs().max()), float(b.abs().max())]
    del got
    for leg in ("eager", "graph"):
        fns = (("kernel", with_switch(True)), ("composition", with_switch(False)))
        if leg == "graph":
            fns = tuple((k, captured(fn)) for k, fn in fns)
        else:
            for _, fn in fns:
                for _ in range(5):
                    fn()
        per = {k: [] for k, _ in fns}
        for _ in range(WINDOWS):
            for k, fn in fns:
                per[k].append(window(fn, calls) if leg == "graph" else eager_window(fn, calls))
        med = {k: float(np.median(v)) for k, v in per.items()}
        spread = max(per["composition"]) - min(per["composition"])
        entry = {k: {"median_us": med[k], "min_us": min(v), "max_us": max(v)} for k, v in per.items()}
        delta = med["kernel"] - med["composition"]
        entry["kernel_minus_composition_us"] = delta
        entry["composition_spread_us"] = spread
        entry["verdict"] = "FASTER than the spread" if -delta > spread else "SLOWER than the spread allows" if delta > spread else "no difference"
        result["legs"][leg] = entry
        print("%-7s forward_backward %-5s kernel %9.2f us [%.2f, %.2f]   composition %9.2f us [%.2f, %.2f]   %s" % (
            name, leg, med["kernel"], min(per["kernel"]), max(per["kernel"]), med["composition"], min(per["composition"]),
            max(per["composition"]), entry["verdict"]), flush=True)
        del fns
    print("%-7s peak MB of forward + backward: kernel %.2f  composition %.2f" % (
        name, result["peak_mb_forward_backward"]["kernel"], result["peak_mb_forward_backward"]["composition"]), flush=True)
    torch.cuda.empty_cache()
    return result


def trainer(runs, others, epochs=3):
    """MVGAE through the Trainer at Baby size, `fused_recon` on and off alternated, the other two keys as given
    -> {"on": [...], "off": [...]} ms per batch"""
    from run_config import run
    ms = {"on": [], "off": []}
    for i in range(2 * runs):
        on = i % 2 == 0
        cd = dict(fused_recon=on, fused_posterior=others, fused_heads=others)
        ms["on" if on else "off"].append(run("mvgae", cd, epochs, verbose=False)["ms_per_batch"])
        print("[mvgae, other keys %s] run %d fused_recon %s: %.3f ms/batch" % (others, i // 2, on, ms["on" if on else "off"][-1]),
              flush=True)
    for k, v in ms.items():
        s = sorted(v)
        print("[mvgae, other keys %s] fused_recon %-3s ms/batch median %.3f min %.3f max %.3f over %d runs" % (
            others, k, s[len(s) // 2], s[0], s[-1], len(s)), flush=True)
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
    path = argv[0] if argv else os.path.join(ROOT, "profiles", "hardest_negative_ab.json")
    results = {"ops": [one(*s) for s in sizes]}
    if runs:
        results["mvgae_trainer_ms_per_batch_baby"] = {"other_keys_on": trainer(runs, True), "other_keys_off": trainer(runs, False)}
    with open(path, "w") as f:
        json.dump(results, f, indent=1)
    print("wrote", path)
