#!/usr/bin/env python3
"""DAMRS's neighbour-discrimination term for three modalities, forward + backward: the `fused_labels` path (hip_ops.pseudo_labels
on csrc/tri_topk.hip, score_lse, edge_dot: DAMRS._neighbour_fused, no [b, I] block) against the key-off torch composition (three
cosine blocks, three softmaxes, the add / topk / scatter / topk chains and the exp blocks autograd keeps: DAMRS.calculate_loss's
lines) in ONE process, eager, on the same tables:

    b = 4,096 query rows against I = 7,050 (Amazon-Baby), 18,357 (Amazon-Sports) and 500,000 items, three [I, 64] tables

HIP events around windows of iterations: median / min / max over five windows after warm-up, windows of the two paths alternating.
A path is "slower" when its median exceeds the other's by more than the other's own min-max spread.  Peak memory: one forward +
backward above the resident inputs.  A path that cannot run (out of memory) is recorded with its error, not estimated.  The
labels of the two paths are compared (share of equal lists) and the two losses.
With `--trainer RUNS`: DAMRS through the Trainer on synthetic Baby-shaped data (tools/run_config.py `damrs`), RUNS runs with
`fused_labels` on and RUNS with it off, alternated.  Results as JSON (default profiles/pseudo_labels_ab.json).

    python tools/prof_pseudo_labels.py [out.json] [--trainer RUNS] [--sizes baby,sports,500k]
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

WINDOWS = 5
B = 4096
SIZES = {"baby": (7050, 10, 5), "sports": (18357, 5, 3), "500k": (500000, 2, 1)}     # items, iterations per window: fused, composition
D = 64


def composition(tables, i_id):
    """the key-off lines of DAMRS.calculate_loss for the neighbour term"""
    import torch
    import torch.nn.functional as F
    from mmrec_amd.models.damrs import DAMRS
    h_t, h_v, h_s = tables
    cos_t, cos_v, cos_s = (DAMRS._cosine_block(h[i_id], h) for h in (h_t, h_v, h_s))
    with torch.no_grad():
        p_t, p_v, p_s = (F.softmax(c, dim=1) for c in (cos_t, cos_v, cos_s))
        labels_s = DAMRS._pseudo_labels(p_t, p_v, p_s)
        labels_v = DAMRS._pseudo_labels(p_t, p_s, p_v)
        labels_t = DAMRS._pseudo_labels(p_v, p_s, p_t)
    return (DAMRS._neighbour_discrimination(*labels_s, cos_s) + DAMRS._neighbour_discrimination(*labels_v, cos_v)
            + DAMRS._neighbour_discrimination(*labels_t, cos_t)) / 3.0, (labels_t, labels_v, labels_s)


def window(fn, iters):
    import torch
    a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return a.elapsed_time(e) / iters


def one(name, n, it_fused, it_comp):
    import numpy as np
    import torch
    from mmrec_amd import hip_ops
    from mmrec_amd.models.damrs import DAMRS
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(n)
    # clustered rows, as propagated item embeddings are: near neighbours exist
    centres = torch.randn(max(2, n // 20), D, device=dev, generator=gen)
    tables = [(centres[torch.randint(0, centres.shape[0], (n,), device=dev, generator=gen)]
               + 0.3 * torch.randn(n, D, device=dev, generator=gen)).requires_grad_() for _ in range(3)]
    i_id = torch.sort(torch.randperm(n, device=dev, generator=gen)[:B]).values

    def fused():
        loss = DAMRS._neighbour_fused(None, i_id, tables)
        return loss, torch.autograd.grad(loss, tables)

    def comp():
        loss, _ = composition(tables, i_id)
        return loss, torch.autograd.grad(loss, tables)
    paths = {"fused": (fused, it_fused), "composition": (comp, it_comp)}
    result = {"shape": name, "n_items": n, "b": B, "windows": WINDOWS, "split_cols": hip_ops.tri_topk_split_cols(B, n), "paths": {}}
    alive = {}
    for k, (fn, iters) in paths.items():
        entry = {"iterations_per_window": iters}
        try:
            fn()
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            loss, grads = fn()
            torch.cuda.synchronize()
            entry["peak_mb_forward_backward"] = (torch.cuda.max_memory_allocated() - base) / 2 ** 20
            entry["loss"] = float(loss)
            entry["grad_abs_max"] = [float(g.abs().max()) for g in grads]
            del loss, grads
            alive[k] = (fn, iters)
        except torch.OutOfMemoryError as e:
            entry["error"] = "out of memory: " + str(e).split("\n")[0][:200]
            print("%-7s %-11s did not run: %s" % (name, k, entry["error"]), flush=True)
        torch.cuda.empty_cache()
        result["paths"][k] = entry
    if len(alive) == 2:
        with torch.no_grad():
            hn = [hip_ops.row_normalize(t.detach()) for t in tables]
            mm, single = hip_ops.pseudo_labels(hn, i_id)
            _, ref = composition([t.detach() for t in tables], i_id)
            same = [float((torch.sort(mm[m], dim=1).values == torch.sort(ref[m][0], dim=1).values).all(dim=1).float().mean())
                    for m in range(3)]
            same += [float((torch.sort(single[m], dim=1).values == torch.sort(ref[m][1], dim=1).values).all(dim=1).float().mean())
                     for m in range(3)]
            result["share_of_equal_lists_mm_then_single"] = same
            del hn, mm, single, ref
        torch.cuda.empty_cache()
    per = {k: [] for k in alive}
    for _ in range(WINDOWS):
        for k, (fn, iters) in alive.items():
            per[k].append(window(fn, iters))
    for k, v in per.items():
        result["paths"][k].update({"median_ms": float(np.median(v)), "min_ms": min(v), "max_ms": max(v)})
    if len(per) == 2:
        f, c = result["paths"]["fused"], result["paths"]["composition"]
        spread = c["max_ms"] - c["min_ms"]
        result["fused_minus_composition_ms"] = f["median_ms"] - c["median_ms"]
        result["verdict"] = "SLOWER than the spread allows" if f["median_ms"] - c["median_ms"] > spread else "not slower"
    for k in alive:
        p = result["paths"][k]
        print("%-7s %-11s %9.3f ms [%.3f, %.3f]  peak %.1f MB  loss %.6f" % (name, k, p["median_ms"], p["min_ms"], p["max_ms"],
                                                                             p["peak_mb_forward_backward"], p["loss"]), flush=True)
    if "verdict" in result:
        print("%-7s fused path: %s; equal lists (mm t, v, s; single t, v, s): %s" % (
            name, result["verdict"], " ".join("%.4f" % s for s in result["share_of_equal_lists_mm_then_single"])), flush=True)
    del tables
    torch.cuda.empty_cache()
    return result


def trainer(runs, epochs=3):
    """DAMRS through the Trainer at Baby size, the key on and off alternated -> {"on": [...], "off": [...]} ms per batch"""
    from run_config import run
    ms = {"on": [], "off": []}
    for i in range(2 * runs):
        on = i % 2 == 0
        ms["on" if on else "off"].append(run("damrs", dict(fused_labels=on), epochs, verbose=False)["ms_per_batch"])
        print("[damrs] run %d fused_labels %s: %.3f ms/batch" % (i // 2, on, ms["on" if on else "off"][-1]), flush=True)
    for k, v in ms.items():
        s = sorted(v)
        print("[damrs] fused_labels %-3s ms/batch median %.3f min %.3f max %.3f over %d runs" % (k, s[len(s) // 2], s[0], s[-1], len(s)),
              flush=True)
    return ms


if __name__ == "__main__":
    argv = sys.argv[1:]
    runs, sizes = 0, list(SIZES)
    if "--trainer" in argv:
        i = argv.index("--trainer")
        runs = int(argv[i + 1])
        del argv[i:i + 2]
    if "--sizes" in argv:
        i = argv.index("--sizes")
        sizes = [s for s in argv[i + 1].split(",") if s]
        del argv[i:i + 2]
    path = argv[0] if argv else os.path.join(ROOT, "profiles", "pseudo_labels_ab.json")
    results = {"ops": [one(s, *SIZES[s]) for s in sizes]}
    if runs:
        results["damrs_trainer_ms_per_batch_baby"] = trainer(runs)
    with open(path, "w") as f:
        json.dump(results, f, indent=1)
    print("wrote", path)
