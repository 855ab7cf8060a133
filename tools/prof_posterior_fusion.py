#!/usr/bin/env python3
"""MVGAE's posterior tail: the kernel path (hip_ops.POSTERIOR_FUSION on: posterior_fusion, csrc/posterior.hip) against the torch
composition (the switch off: `posterior_fusion_torch`, i.e. the operations of MVGAE's product_of_experts, reparametrize and kl_loss
with stock autograd) in ONE process, each leg as a hipGraph replay:

    forward           Z, kl, score = posterior_fusion(mu_v, lv_v, mu_t, lv_t, mu_c, lv_c, noise)                (no autograd)
    forward_backward  the same with autograd, then the gradients of <Z, g> + <kl, w> to the six encoder outputs

Sizes (users + items): Amazon-Baby 26,495, Amazon-Sports 54,255, and 1,500,000.  HIP events around windows of replays: median /
min / max over five windows after warm-up, windows of the two paths alternating.  A leg is "faster" only when its median beats the
composition's by more than the composition's own min-max spread, "slower" when it exceeds it by more than that.  Peak memory: one
eager forward + backward above the resident inputs.  The bytes the kernels must move (forward: ten tables in, five out; backward:
fourteen in, six out) give the achieved bandwidth.
With `--trainer RUNS`: MVGAE through the Trainer on synthetic Baby-shaped data (tools/run_config.py `mvgae`), RUNS runs with
`fused_posterior` on and RUNS with it off, alternated.  Results as JSON (default profiles/posterior_fusion_ab.json).

    python tools/prof_posterior_fusion.py [out.json] [--trainer RUNS]
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from prof_hyper import captured, window  # noqa: E402

WINDOWS = 5
SIZES = (("baby", 26495, 100), ("sports", 54255, 100), ("1.5M", 1500000, 5))
D = 64
BYTES_FWD, BYTES_BWD = 15 * D * 4, 20 * D * 4    # per row


def one(name, n, replays):
    import numpy as np
    import torch
    from mmrec_amd import hip_ops
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(n)
    r = lambda *s: torch.randn(*s, device=dev, generator=gen)            # noqa: E731
    ops = [(r(n, D) * (0.5 if i % 2 == 0 else 2.0)).requires_grad_() for i in range(6)]     # means, then log-variances in +-8
    noise = [r(n, D) for _ in range(4)]
    g, w = r(4, n, D), torch.tensor([0.1, 0.1, 0.1, 0.1], device=dev)
    assert hip_ops.posterior_fusion_served(*ops, noise)

    def with_switch(on, fn):
        def run():
            hip_ops.POSTERIOR_FUSION = on
            try:
                return fn()
            finally:
                hip_ops.POSTERIOR_FUSION = True
        return run

    def forward():
        with torch.no_grad():
            return hip_ops.posterior_fusion(*ops, noise)

    def forward_backward():
        Z, kl, _ = hip_ops.posterior_fusion(*ops, noise)
        return torch.autograd.grad((Z * g).sum() + (kl * w).sum(), ops)

    result = {"shape": name, "n_rows": n, "rows_per_block": hip_ops.posterior_fusion_rows_per_block(n), "windows": WINDOWS,
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
    names = ("Z", "kl", "score", "d_mu_v", "d_lv_v", "d_mu_t", "d_lv_t", "d_mu_c", "d_lv_c")
    for nm, a, b in zip(names, got["kernel"], got["composition"]):
        result["max_diff"][nm] = [float((a - b).abs().max()), float(b.abs().max())]
    del got
    for leg, fn, nbytes in (("forward", forward, BYTES_FWD), ("forward_backward", forward_backward, BYTES_FWD + BYTES_BWD)):
        graphs = (("kernel", captured(with_switch(True, fn))), ("composition", captured(with_switch(False, fn))))
        per = {k: [] for k, _ in graphs}
        for _ in range(WINDOWS):
            for k, graph in graphs:
                per[k].append(window(graph, replays))
        med = {k: float(np.median(v)) for k, v in per.items()}
        spread = max(per["composition"]) - min(per["composition"])
        entry = {k: {"median_us": med[k], "min_us": min(v), "max_us": max(v)} for k, v in per.items()}
        delta = med["kernel"] - med["composition"]
        entry["kernel_minus_composition_us"] = delta
        entry["composition_spread_us"] = spread
        entry["verdict"] = "FASTER than the spread" if -delta > spread else "SLOWER than the spread allows" if delta > spread else "no difference"
        entry["kernel_gb_per_s"] = nbytes * n / (med["kernel"] * 1e-6) / 1e9
        result["legs"][leg] = entry
        print("%-7s %-17s kernel %9.2f us [%.2f, %.2f] (%.0f GB/s)   composition %9.2f us [%.2f, %.2f]   %s" % (
            name, leg, med["kernel"], min(per["kernel"]), max(per["kernel"]), entry["kernel_gb_per_s"], med["composition"],
            min(per["composition"]), max(per["composition"]), entry["verdict"]), flush=True)
        del graphs
    print("%-7s peak MB of forward + backward: kernel %.2f  composition %.2f" % (
        name, result["peak_mb_forward_backward"]["kernel"], result["peak_mb_forward_backward"]["composition"]), flush=True)
    torch.cuda.empty_cache()
    return result


def trainer(runs, epochs=3):
    """MVGAE through the Trainer at Baby size, the key on and off alternated -> {"on": [...], "off": [...]} ms per batch"""
    from run_config import run
    ms = {"on": [], "off": []}
    for i in range(2 * runs):
        on = i % 2 == 0
        ms["on" if on else "off"].append(run("mvgae", dict(fused_posterior=on), epochs, verbose=False)["ms_per_batch"])
        print("[mvgae] run %d fused_posterior %s: %.3f ms/batch" % (i // 2, on, ms["on" if on else "off"][-1]), flush=True)
    for k, v in ms.items():
        s = sorted(v)
        print("[mvgae] fused_posterior %-3s ms/batch median %.3f min %.3f max %.3f over %d runs" % (k, s[len(s) // 2], s[0], s[-1],
                                                                                                   len(s)), flush=True)
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
    path = argv[0] if argv else os.path.join(ROOT, "profiles", "posterior_fusion_ab.json")
    results = {"ops": [one(*s) for s in sizes]}
    if runs:
        results["mvgae_trainer_ms_per_batch_baby"] = trainer(runs)
    with open(path, "w") as f:
        json.dump(results, f, indent=1)
    print("wrote", path)
