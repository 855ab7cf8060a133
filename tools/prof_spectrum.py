#!/usr/bin/env python3
"""SMORE's spectrum step: the kernel path (hip_ops.SPECTRUM on: spectrum_fusion, csrc/spectrum.hip) against the torch composition
(the switch off: `spectrum_fusion_torch`, i.e. SMORE.spectrum_convolution's GEMMs and element-wise chains with stock autograd) in
ONE process, each leg as a hipGraph replay:

    forward           image_conv, text_conv, fusion_conv = spectrum_fusion(image, text, w_img, w_txt, w_fus)     (no autograd)
    forward_backward  the same with autograd, then the gradients of <image_conv, g1> + <text_conv, g2> + <fusion_conv, g3> to all
                      five operands

Sizes (items): Amazon-Baby 7,050, Amazon-Sports 18,357, and 500,000.  HIP events around windows of replays: median / min / max over
five windows after warm-up, windows of the two paths alternating.  A leg is "slower" when its median exceeds the composition's by
more than the composition's own min-max spread.  Peak memory: one eager forward + backward above the resident inputs.  The fp32
FMAs the kernels execute (20,480 per row forward, 28,672 backward, the packed 64 x 64 transforms) give the achieved FLOP / s.
With `--trainer RUNS`: SMORE through the Trainer on synthetic Baby-shaped data (tools/run_config.py `smore`), RUNS runs with
`fused_spectrum` on and RUNS with it off, alternated.  Results as JSON (default profiles/spectrum_ab.json).

    python tools/prof_spectrum.py [out.json] [--trainer RUNS]
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from prof_hyper import captured, window  # noqa: E402

WINDOWS = 5
SIZES = (("baby", 7050, 200), ("sports", 18357, 200), ("500k", 500000, 20))
D = 64
FMA_FWD, FMA_BWD = 5 * D * D, 7 * D * D        # per row: the packed [64, 64] transforms each call runs


def one(name, n, replays):
    import numpy as np
    import torch
    from mmrec_amd import hip_ops
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(n)
    r = lambda *s: torch.randn(*s, device=dev, generator=gen)            # noqa: E731
    x, y = (r(n, D) * 0.1).requires_grad_(), (r(n, D) * 0.1).requires_grad_()
    ws = [r(1, D // 2 + 1, 2).requires_grad_() for _ in range(3)]
    gs = [r(n, D) for _ in range(3)]
    assert hip_ops.spectrum_fusion_served(x, y, *ws)

    def with_switch(on, fn):
        def run():
            hip_ops.SPECTRUM = on
            try:
                return fn()
            finally:
                hip_ops.SPECTRUM = True
        return run

    def forward():
        with torch.no_grad():
            return hip_ops.spectrum_fusion(x, y, *ws)

    def forward_backward():
        outs = hip_ops.spectrum_fusion(x, y, *ws)
        return torch.autograd.grad(sum((o * g).sum() for o, g in zip(outs, gs)), [x, y] + ws)

    result = {"shape": name, "n_items": n, "rows_per_block": hip_ops.spectrum_rows_per_block(n), "windows": WINDOWS,
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
    names = ("image_conv", "text_conv", "fusion_conv", "d_image", "d_text", "d_w_img", "d_w_txt", "d_w_fus")
    for nm, a, b in zip(names, got["kernel"], got["composition"]):
        result["max_diff"][nm] = [float((a - b).abs().max()), float(b.abs().max())]
    del got
    for leg, fn, fma in (("forward", forward, FMA_FWD), ("forward_backward", forward_backward, FMA_FWD + FMA_BWD)):
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
        entry["kernel_fp32_tflops"] = 2.0 * fma * n / (med["kernel"] * 1e-6) / 1e12
        result["legs"][leg] = entry
        print("%-7s %-17s kernel %9.2f us [%.2f, %.2f] (%.2f TFLOP/s fp32)   composition %9.2f us [%.2f, %.2f]   %s" % (
            name, leg, med["kernel"], min(per["kernel"]), max(per["kernel"]), entry["kernel_fp32_tflops"], med["composition"],
            min(per["composition"]), max(per["composition"]), entry["verdict"]), flush=True)
        del graphs
    print("%-7s peak MB of forward + backward: kernel %.2f  composition %.2f" % (
        name, result["peak_mb_forward_backward"]["kernel"], result["peak_mb_forward_backward"]["composition"]), flush=True)
    torch.cuda.empty_cache()
    return result


def trainer(runs, epochs=3):
    """SMORE through the Trainer at Baby size, the key on and off alternated -> {"on": [...], "off": [...]} ms per batch"""
    from run_config import run
    ms = {"on": [], "off": []}
    for i in range(2 * runs):
        on = i % 2 == 0
        ms["on" if on else "off"].append(run("smore", dict(fused_spectrum=on), epochs, verbose=False)["ms_per_batch"])
        print("[smore] run %d fused_spectrum %s: %.3f ms/batch" % (i // 2, on, ms["on" if on else "off"][-1]), flush=True)
    for k, v in ms.items():
        s = sorted(v)
        print("[smore] fused_spectrum %-3s ms/batch median %.3f min %.3f max %.3f over %d runs" % (k, s[len(s) // 2], s[0], s[-1], len(s)),
              flush=True)
    return ms


if __name__ == "__main__":
    argv = sys.argv[1:]
    runs = 0
    if "--trainer" in argv:
        i = argv.index("--trainer")
        runs = int(argv[i + 1])
        del argv[i:i + 2]
    path = argv[0] if argv else os.path.join(ROOT, "profiles", "spectrum_ab.json")
    results = {"ops": [one(*s) for s in SIZES]}
    if runs:
        results["smore_trainer_ms_per_batch_baby"] = trainer(runs)
    with open(path, "w") as f:
        json.dump(results, f, indent=1)
    print("wrote", path)
