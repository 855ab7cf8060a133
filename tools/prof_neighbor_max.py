#!/usr/bin/env python3
"""`hip_ops.neighbor_max` (mmrec_neighbor_max_f32 / _bwd_f32) on one MI355X, in one process:

    python tools/prof_neighbor_max.py [--reps 30] [--shapes baby c5] [--json profiles/r12_neighbor_max_op.json]

Graphs: both directions of the synthetic Amazon-Baby training interactions (19,445 + 7,050 nodes, 237,412 entries) and of the
20 M-nonzero benchmark graph (1,000,000 + 500,000 nodes), rows = the target node, d = 64.  For each, device-event times
(`--reps` timed calls after warm-up in three alternating rounds; median, min, max) of
    neighbor_max   forward, and forward + backward (autograd through the op)
    spmm_raw       the CSR SpMM on the SAME structure (dyn.fwd with unit values), and that plus the SpMM on dyn.bwd: the same
                   gathers of 256-byte rows; the max adds a 256-byte `arg` row per output row, and its backward gathers an
                   `arg` row next to each dY row
    torch          `hip_ops.neighbor_max_torch`, where its [n_edges, 64] temporaries fit (`--skip-torch-above` bytes of one)
and the peak memory of one forward + backward above the resident inputs.  The forwards' results are compared (arg equal, Y
bit-equal) where the composition runs."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mmrec_amd import hip_ops, synth  # noqa: E402


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


def one(name, reps, skip_torch_above):
    dev = torch.device("cuda:0")
    nu, ni, eu, ei = synth.shaped_edges(name, seed=0)
    n = nu + ni
    src, dst = np.concatenate([eu, ei + nu]), np.concatenate([ei + nu, eu])
    rows, cols = torch.from_numpy(dst).to(dev), torch.from_numpy(src).to(dev)
    ne = rows.numel()
    dyn = hip_ops.DynGraph(rows, cols, n, n)
    gen = torch.Generator(device=dev).manual_seed(0)
    X = (torch.rand(n, 64, device=dev, generator=gen) - 0.5).requires_grad_()
    dY = torch.rand(n, 64, device=dev, generator=gen) - 0.5
    dyn.fwd.vals = torch.ones(ne, device=dev)
    dyn.bwd.vals = torch.ones(ne, device=dev)
    out_f, out_b = torch.empty(n, 64, device=dev), torch.empty(n, 64, device=dev)
    assert hip_ops.neighbor_max_served(X, dyn)
    deg = np.bincount(dst, minlength=n)
    row = {"shape": name, "n_nodes": int(n), "n_entries": int(ne), "longest_row": int(deg.max()),
           "rows_beyond_group_max": int((deg > hip_ops.neighbor_max_group_max()).sum()), "group_max": hip_ops.neighbor_max_group_max()}

    def spmm_fwd():
        hip_ops.spmm_raw(dyn.fwd, X.detach(), Y=out_f)

    def spmm_fwd_bwd():
        hip_ops.spmm_raw(dyn.fwd, X.detach(), Y=out_f)
        hip_ops.spmm_raw(dyn.bwd, dY, Y=out_b)
    legs = {"neighbor_max": (lambda: hip_ops.neighbor_max(X.detach(), dyn),
                             lambda: torch.autograd.grad(hip_ops.neighbor_max(X, dyn)[0], X, dY)),
            "spmm_raw": (spmm_fwd, spmm_fwd_bwd)}
    if ne * 64 * 4 <= skip_torch_above:
        legs["torch"] = (lambda: hip_ops.neighbor_max_torch(X.detach(), rows, cols, n),
                         lambda: torch.autograd.grad(hip_ops.neighbor_max_torch(X, rows, cols, n)[0], X, dY))
    for k, (fwd, fwd_bwd) in legs.items():
        for _ in range(3):
            fwd_bwd()
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        fwd_bwd()
        torch.cuda.synchronize()
        row[k + "_peak_mb"] = (torch.cuda.max_memory_allocated() - base) / 2 ** 20
    if "torch" in legs:
        (y1, a1), (y2, a2) = legs["neighbor_max"][0](), legs["torch"][0]()
        row["same_arg_and_Y_bits_as_torch"] = bool(torch.equal(a1, a2) and torch.equal(y1.view(torch.int32), y2.view(torch.int32)))
    t = {(k, leg): [] for k in legs for leg in ("fwd", "fwd_bwd")}
    for _ in range(3):                                        # alternate the versions: three rounds of reps / 3
        for k, (fwd, fwd_bwd) in legs.items():
            t[(k, "fwd")] += timed(fwd, max(1, reps // 3))
            t[(k, "fwd_bwd")] += timed(fwd_bwd, max(1, reps // 3))
    for (k, leg), v in t.items():
        row["%s_%s_ms" % (k, leg)] = statistics.median(v)
        row["%s_%s_ms_min_max" % (k, leg)] = [min(v), max(v)]
    print(json.dumps(row), flush=True)
    del dyn, X, dY, out_f, out_b, legs
    torch.cuda.empty_cache()
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--shapes", nargs="+", default=["baby", "c5"])
    ap.add_argument("--json")
    ap.add_argument("--skip-torch-above", type=float, default=1e9)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing is measured")
    rows = [one(name, args.reps, args.skip_torch_above) for name in args.shapes]
    if args.json:
        with open(args.json, "w") as f:
            json.dump({"what": "hip_ops.neighbor_max against spmm_raw on the same structure and against neighbor_max_torch, "
                               "device-event ms (median, [min, max]), one MI355X, eager calls",
                       "reps": args.reps, "shapes": rows}, f, indent=1)


if __name__ == "__main__":
    main()
