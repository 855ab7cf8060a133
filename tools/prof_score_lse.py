#!/usr/bin/env python3
"""`hip_ops.score_lse` against the torch composition `logsumexp(scale * Q @ K.T, 1)` on one MI355X, in one process:

    python tools/prof_score_lse.py [--reps 30] [--json out.json]

For every shape: device-event time of the forward and of forward + backward (versions alternated, `--reps` timed calls after
warm-up, median and spread), the peak memory of one forward + backward above the resident inputs, the largest difference of the
results, and for the fused op the achieved share of the 157.3 TFLOP/s fp32-MFMA rate: 2 B N d FLOP for the score sweep of the
forward, 3 sweeps + 2 gradient products = 10 B N d for forward + backward, over the call's time (a whole-call rate: launches and
the finish kernels are inside it).  The composition is skipped where its temporaries would not fit (`--skip-torch-above` bytes of
one B x N matrix)."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mmrec_amd import hip_ops  # noqa: E402

SHAPES = ((2048, 7050, 64), (2048, 19445, 64), (2048, 192403, 64), (2048, 2048, 128))
PEAK = 157.3e12


def timed(fn, reps):
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--json")
    ap.add_argument("--skip-torch-above", type=float, default=4e9)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing is measured")
    dev = torch.device("cuda:0")
    rows = []
    for B, N, d in SHAPES:
        gen = torch.Generator(device=dev).manual_seed(B + N)
        Q = torch.nn.functional.normalize(torch.randn(B, d, device=dev, generator=gen)).requires_grad_()
        K = torch.nn.functional.normalize(torch.randn(N, d, device=dev, generator=gen)).requires_grad_()
        scale = 5.0
        fns = {"fused": lambda: hip_ops.score_lse(Q, K, scale),
               "torch": lambda: torch.logsumexp(scale * (Q @ K.T), dim=1)}
        if B * N * 4 > args.skip_torch_above:
            del fns["torch"]

        def fwd_bwd(f):
            Q.grad = K.grad = None
            f().sum().backward()
        row = {"B": B, "N": N, "d": d}
        res = {}
        for name, f in fns.items():
            for _ in range(3):
                fwd_bwd(f)
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            fwd_bwd(f)
            torch.cuda.synchronize()
            row[name + "_peak_mb"] = (torch.cuda.max_memory_allocated() - base) / 2 ** 20
            with torch.no_grad():
                res[name] = (f().clone(), Q.grad.clone(), K.grad.clone())
        t = {(n, k): [] for n in fns for k in ("fwd", "fwd_bwd")}
        for _ in range(3):                                    # alternate the versions: three rounds of reps / 3
            for name, f in fns.items():
                with torch.no_grad():
                    t[(name, "fwd")] += timed(f, max(1, args.reps // 3))
                t[(name, "fwd_bwd")] += timed(lambda: fwd_bwd(f), max(1, args.reps // 3))
        for (name, k), v in t.items():
            row["%s_%s_ms" % (name, k)] = statistics.median(v)
            row["%s_%s_ms_min_max" % (name, k)] = [min(v), max(v)]
        row["fused_fwd_share_of_fp32_mfma"] = 2.0 * B * N * d / (row["fused_fwd_ms"] * 1e-3) / PEAK
        row["fused_fwd_bwd_share_of_fp32_mfma"] = 10.0 * B * N * d / (row["fused_fwd_bwd_ms"] * 1e-3) / PEAK
        if "torch" in res:
            row["max_diff"] = [float((a - b).abs().max()) for a, b in zip(res["fused"], res["torch"])]
        rows.append(row)
        print(json.dumps(row), flush=True)
        del Q, K, res
        torch.cuda.empty_cache()
    if args.json:
        with open(args.json, "w") as f:
            json.dump({"what": "hip_ops.score_lse against torch.logsumexp(scale * Q @ K.T, 1), device-event ms (median), one MI355X",
                       "reps": args.reps, "shapes": rows}, f, indent=1)


if __name__ == "__main__":
    main()
