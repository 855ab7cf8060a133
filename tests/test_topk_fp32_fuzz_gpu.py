"""Seeded differential fuzz of the fp32 implementations behind `mmrec_score_topk_f32` (csrc/topk.hip) through the RAW C ABI.

tests/test_topk_fuzz_gpu.py draws kd in {64, 128, 192, 384} with default flags: the fp16 filter, topk_wide.h and what is left
for the materialised block path.  This file draws the shapes the OTHER implementations serve, restates `topk_plan` in Python
(`topk_plan`, `path_label`, `workspace_bytes` below) and labels every case with the path it takes, so that a plan change that
moves cases off a path fails tests/test_topk_fp32_fuzz_cpu.py instead of quietly testing nothing:

    fused        kd % 32 != 0 (family 1) or nc > 2,097,152 (family 2): score_topk_kernel<false, 64>, transpose_pad_kernel on Q,
                 1 .. 16 candidate splits + merge_topk_kernel
    two_pass     kd == 64 and nc > 2,097,152 (family 2): score_groupmax_kernel, kth_largest_kernel, score_topk_kernel<true, 48>
    matgen       kd % 32 == 0, kd != 64, where neither the fp16 filter nor the wide path applies (family 3): gemm_nt + select
    mat64        kd == 64 below 4096 candidates, or with MMREC_TOPK_NO_FILTER (family 4): streaming GEMM + group maxima + select
    mat64_blocks the same in more than one query block (family 5: 2049 queries x 1,000,001 candidates, blocks of 1152 + 897)

and, on top: `hip_ops._score_topk_blocked` with a 96-query block (family 6) and the argument contract (family 7).

Checker: `check_lists` of tests/test_topk_fuzz_gpu.py, unchanged (near-tie rule 2e-6 |q| |c| on float64 scores, values, order,
tie order by lower id, no masked or duplicate id, a starved tail at exactly float32(-1e10)).  Inputs: that file's ingredients,
re-drawn here (common component, 2^+-40 query / 2^+-12 candidate row scales, outliers, zero queries, duplicated candidates and
queries, masks none / sparse / 16-40 per row / heavy users of 600 and 5,000 ids / best candidates masked / starved rows, scores
inside +-1e8).  Where the candidates are split, one user masks one split's WHOLE range and the first id of another split (the
per-split mask cursor starts mid-row there); on the block paths the same user masks one contiguous run (whole groups).

Every call has `out_idx`, `out_val` between guard elements and a workspace of EXACTLY `mmrec_topk_workspace_bytes` bytes between
guard bytes; every case runs twice and must give the same bits (no float atomics on these paths).  Cases above 2,097,152
candidates and the two-block case check a fixed subset of rows against float64 (stated at `check_rows`); all their rows take
part in the bit comparisons.

On one MI355X the 197 device tests take 20 s: 4.4 s, 3.3 s and 2.8 s for the two masked cases above 2,097,152 candidates and
the two-block case (host time: drawing and copying up to 1 GB of candidates, float64 scores of the checked rows), every other
case under 0.4 s.  Worst |val - s64| / (|q| |c|) per path against the checker's 2e-6: fused 5.8e-7, two-pass 1.6e-7, general
GEMM 1.1e-6 (kd = 512), streaming GEMM 4.7e-7, two blocks 1.6e-7.
"""
from collections import namedtuple

import numpy as np
import pytest
import torch

from tests.test_graph_build_fuzz_gpu import F32, I32, I64, Guarded, P, WS_GUARD, Workspace, _dev, _lib
from tests.test_topk_fuzz_gpu import WORK, check_lists

BAD_ARG, UNSUPPORTED = 10001, 10002
NO_FILTER = 1                                   # MMREC_TOPK_NO_FILTER
NC_FUSED = (2 << 20) + 1                        # from this many candidates on nothing is materialised
MASKED = np.float32(-1e10)

# ------------------------------------------------------------------------------------------------ topk_plan, restated
Plan = namedtuple("Plan", "n_tiles n_split tiles_per_wave two_pass n_groups materialise qb_rows max_s")
S_BYTES_MAX = 8192 << 20                        # MMREC_TOPK_S_MB
GEMM64_MAX_GROUPS = 384


def cdiv(a, b):
    return -(-a // b)


def al256(x):
    return (x + 255) & ~255


def pad_to(x, m):
    return cdiv(x, m) * m


def topk_plan(nq, nc, kd, k):
    n_tiles, qblocks = cdiv(nc, 32), cdiv(nq, 32)
    max_s = min(max(nc // (4 * k), 1), 16)
    if max_s * k > 512:
        max_s = 512 // k
    max_s = max(max_s, 1)
    s, best = 1, -1
    for c in range(1, max_s + 1):
        cost = cdiv(qblocks * c, 2048) * (cdiv(n_tiles, c) + 4)
        if best < 0 or cost < best:
            best, s = cost, c
    two_pass = kd == 64 and n_tiles >= 2 * k
    tiles_per_group = cdiv(n_tiles, 128) if two_pass else 1
    n_groups = cdiv(n_tiles, tiles_per_group)
    tiles_per_wave = cdiv(n_groups, s) * tiles_per_group
    n_split = cdiv(n_tiles, tiles_per_wave)
    materialise = kd % 32 == 0 and nc <= (2 << 20)
    qb_rows = 0
    if materialise:
        rows = max(S_BYTES_MAX // (pad_to(nc, 256) * 4) // 128 * 128, 128)
        qb_rows = min(nq, rows)
        qb_rows = min(pad_to(cdiv(nq, cdiv(nq, qb_rows)), 128), nq)
        two_pass, n_split = False, 1
    return Plan(n_tiles, n_split, tiles_per_wave, bool(two_pass), n_groups, bool(materialise), qb_rows, max_s)


def filter_applicable(nq, nc, kd, k):           # topk64_filter_applicable
    return kd in (64, 128) and k <= 128 and 4096 <= nc <= 1000000 and nq >= 1


def wide_applicable(nq, nc, kd, k):             # topk_wide_applicable
    return 128 < kd <= 4096 and kd % 32 == 0 and k <= 32 and nc >= 4096 and nq >= 1 and nc * kd >= 1 << 22


def filter_prepared_bytes(nc, kd):              # topk64_filter_prepared_bytes
    n_pad = pad_to(nc, 64)
    return 256 * 4 + al256(n_pad * 2 * kd) + (al256(n_pad * 4) + 2048 * 4 if nc >= 131072 else 0)


def filter_workspace_bytes(nq, nc, kd, k):      # topk64_filter_workspace_bytes over filter_plan
    n_stages, nq_pad = cdiv(nc, 64), pad_to(nq, 256)
    spr_of = lambda R: (cdiv(n_stages, R) + 3) & ~3
    best = min(cdiv(n_stages, spr_of(R)) * spr_of(R) for R in range(8, 17))
    for R in range(16, 7, -1):
        spr, reff = spr_of(R), cdiv(n_stages, spr_of(R))
        if reff * spr * 100 <= best * 106:
            break
    sparse = nc >= 32768
    wcap = 2 * (512 if nc >= 131072 else 256)
    bits = al256(nq * 4) + nq * wcap * 16 if sparse else nq * reff * spr * 8
    return (al256(nq_pad * 2 * kd) + filter_prepared_bytes(nc, kd) + al256(nq_pad * 4) + 256 + al256(nq * 32 * reff * 4) +
            3 * al256(nq * 4) + al256(bits) + al256(4096 * 128 * 8) + (al256(nq * 4) if sparse else 0))


def wide_extra_bytes(nc, kd, qb_rows):          # topk_wide_extra_bytes
    kdp = pad_to(kd, 64)
    return (256 + al256(nc * kdp * 2) + al256(qb_rows * kdp * 2) + al256(qb_rows * 64 * 8) + al256(qb_rows * 64 * 4) +
            2 * al256(qb_rows * 4) + al256(qb_rows * kd * 4))


def workspace_bytes(nq, nc, kd, k):
    """mmrec_topk_workspace_bytes: one formula per path (the block paths sized for the fp16 paths too: `flags` decides at launch)"""
    if nq <= 0 or nc <= 0 or k <= 0 or kd <= 0:
        return 0
    p = topk_plan(nq, nc, kd, k)
    kd_pad, ldc, ldq = pad_to(kd, 64), pad_to(nc, 256), pad_to(nq, 32)
    if p.materialise:
        b = (al256(kd_pad * ldc * 4) if kd == 64 else 0) + al256(p.qb_rows * ldc * 4) + al256(p.qb_rows * GEMM64_MAX_GROUPS * 4)
        f = filter_workspace_bytes(nq, nc, kd, k) if filter_applicable(nq, nc, kd, k) else 0
        w = wide_extra_bytes(nc, kd, p.qb_rows) if wide_applicable(nq, nc, kd, k) else 0
        return max(b, f) + w
    b = al256(kd_pad * ldc * 4)
    if kd != 64:
        b += al256(kd_pad * ldq * 4)
    if p.two_pass:
        b += al256(nq * p.n_groups * 4) + al256(nq * 4)
    if p.n_split > 1:
        b += 2 * al256(p.n_split * nq * k * 4)
    return b


def path_label(nq, nc, kd, k, flags):
    """which implementation score_topk_impl runs for this call"""
    p = topk_plan(nq, nc, kd, k)
    if not p.materialise:
        return "two_pass" if p.two_pass else "fused"
    if not flags & NO_FILTER and filter_applicable(nq, nc, kd, k):
        return "filter"
    if not flags & NO_FILTER and wide_applicable(nq, nc, kd, k):
        return "wide"
    if kd == 64:
        return "mat64" if p.qb_rows >= nq else "mat64_blocks"
    return "matgen"


PATHS = ("fused", "two_pass", "matgen", "mat64", "mat64_blocks")

# ------------------------------------------------------------------------------------------------ the cases
F1_KD = (4, 8, 20, 36, 40, 100, 132, 260)
F1_NQ = (1, 31, 32, 33, 64, 65, 100, 257)
F1_K = (1, 2, 31, 32, 33, 63, 64)
KINDS = ("none", "sparse", "perrow", "heavy", "best", "starved", "mix")
KIND_TAGS = {"none": {"none"}, "sparse": {"sparse"}, "perrow": {"sparse", "perrow"}, "heavy": {"sparse", "heavy"},
             "best": {"sparse", "bestmasked"}, "starved": {"sparse", "starved"},
             "mix": {"sparse", "perrow", "heavy", "bestmasked", "starved"}}
MASK_TAGS = ("none", "sparse", "perrow", "heavy", "bestmasked", "starved")
_NC_EDGES = (4096, 32768, 65536, 131072)


def _family1():
    out = []

    def add(nc, k, special=None, nq=None, kd=None, kind=None):
        j = len(out)
        out.append(dict(fam=1, nq=nq or F1_NQ[(j + j // 8) % 8], nc=nc, kd=kd or F1_KD[j % 8], k=k, flags=0,
                        kind=kind or KINDS[j % 7], special=special))

    for nc in (1, 31, 32, 33, 63, 64, 65):                      # one tile, a tile and a bit, two tiles and a bit; k = nc
        add(nc, min(nc, 64))
        add(nc, min(nc, F1_K[len(out) % 7]))
    for k in F1_K:                                              # where max_s = nc / 4k steps: 1 | 2 splits, 2 | 3 ... 15 | 16
        for mult in (4, 8, 64):
            for d in (-1, 0):
                if mult * k + d >= k:
                    add(mult * k + d, k)
    for S in range(1, 17):                                      # every split count, with the smallest nc that has it ...
        for k in (32, 10, 2):
            if S * k > 512:
                continue
            hit = [nc for nc in range(max(4 * k * S, k), 4 * k * S + 3000) if topk_plan(33, nc, 20, k).n_split == S]
            if hit:
                add(hit[0], k)
                add(hit[-1] + 7000 if topk_plan(33, hit[-1] + 7000, 20, k).n_split == S else hit[-1], k)   # ... and a larger one
                break
    add(5000, 10, kd=20)                                        # 16 splits of 10 tiles
    add(40000, 64, nq=65, kd=100, kind="mix")                   # S k = 8 x 64 = 512 merge slots
    add(39999, 32, nq=33, kd=8, kind="mix")                     # S k = 16 x 32 = 512
    add(12345, 1, nq=257, kd=4, kind="heavy")
    add(30011, 50, nq=100, kd=132, kind="starved")
    add(5000, 10, special="ascending", kd=20, nq=65, kind="none")       # > 64 survivors per lane in every split: compact
    add(20000, 64, special="ascending", kd=36, nq=33, kind="sparse")
    return out


def _family2():
    return [dict(fam=2, nq=33, nc=(2 << 20) + 4096 + 17, kd=64, k=50, flags=0, kind="mix", special="unmasked_too"),
            dict(fam=2, nq=33, nc=NC_FUSED, kd=128, k=64, flags=0, kind="mix", special=None),
            dict(fam=2, nq=33, nc=NC_FUSED, kd=4, k=1, flags=0, kind="none", special=None)]


def _family3():
    rows = [(32, 1, 5, 1, "none"), (32, 200, 33, 128, "heavy"), (96, 3000, 300, 65, "mix"), (160, 129, 64, 128, "starved"),
            (256, 4095, 257, 100, "best"), (512, 1000, 129, 64, "perrow"), (128, 4095, 500, 128, "mix"), (128, 130, 31, 65, "sparse"),
            (192, 4096, 200, 33, "mix"), (384, 5000, 150, 128, "heavy"), (192, 20000, 100, 65, "best"), (384, 11000, 64, 100, "starved"),
            (96, 2100, 1000, 10, "none"), (32, 3333, 1, 50, "sparse"), (160, 2049, 129, 1, "perrow")]
    return [dict(fam=3, nq=nq, nc=nc, kd=kd, k=k, flags=0, kind=kind, special=None) for kd, nc, nq, k, kind in rows]


def _family4():
    rows = [(4095, 0, 64, 300, "mix"), (4097, 1, 65, 257, "heavy"), (32767, 1, 1, 100, "mix"), (32769, 1, 128, 64, "heavy"),
            (65535, 1, 64, 50, "best"), (65537, 1, 65, 33, "starved"), (131071, 1, 128, 40, "mix"), (131073, 1, 1, 31, "perrow"),
            (100, 0, 65, 700, "sparse"), (2000, 0, 128, 1000, "none"), (4100, 1, 50, 1200, "none"), (7050, 1, 50, 600, "starved"),
            (4096, 1, 128, 129, "best"), (3000, 0, 1, 513, "perrow"), (65, 0, 65, 33, "starved")]
    return [dict(fam=4, nq=nq, nc=nc, kd=64, k=k, flags=flags, kind=kind, special=None) for nc, flags, k, nq, kind in rows]


def _family5():
    nc = 1_000_001                                              # just above what the fp16 filter accepts
    nq = S_BYTES_MAX // (pad_to(nc, 256) * 4) // 128 * 128 + 1  # one row more than a score block holds
    return [dict(fam=5, nq=nq, nc=nc, kd=64, k=50, flags=0, kind="mix", special="unmasked_too")]


def _random_cases():
    """seeded draws on top of the hand-placed edges: 40 fused, 12 general-GEMM and 12 streaming-GEMM cases"""
    rng = np.random.default_rng(20261)
    out = []
    pick_k = lambda ks, hi: int(rng.choice(ks)) if rng.random() < 0.6 else int(rng.integers(1, hi + 1))
    for _ in range(40):
        nc = int(np.exp(rng.uniform(0, np.log(40000))))
        nq = int(rng.choice(F1_NQ)) if rng.random() < 0.5 else int(rng.integers(1, min(600, int(4e6) // nc) + 1))
        out.append(dict(fam=1, nq=nq, nc=nc, kd=int(rng.choice(F1_KD)), k=min(nc, pick_k(F1_K, 64)), flags=0,
                        kind=str(rng.choice(KINDS)), special=None))
    for _ in range(12):
        if rng.random() < 0.7:
            kd, nc, k = int(rng.choice([32, 96, 128, 160, 256, 512])), int(rng.integers(1, 4096)), pick_k([1, 64, 65, 128], 128)
        else:
            kd, nc, k = int(rng.choice([192, 384])), int(rng.integers(4096, 30000)), int(rng.integers(33, 129))
        nq = int(rng.choice([1, 31, 127, 128, 129, 257])) if rng.random() < 0.5 else int(rng.integers(1, min(1000, int(4e6) // nc) + 1))
        out.append(dict(fam=3, nq=nq, nc=nc, kd=kd, k=min(nc, k), flags=0, kind=str(rng.choice(KINDS)), special=None))
    for _ in range(12):
        kind = int(rng.integers(0, 4))
        nc = (int(rng.integers(1, 4096)) if kind == 0 else int(rng.choice(_NC_EDGES)) + int(rng.integers(-70, 70)) if kind == 1
              else int(rng.integers(4096, 140000)))
        nq = int(rng.choice([1, 3, 4, 5, 127, 128, 129])) if rng.random() < 0.5 else int(rng.integers(1, min(1500, int(4e6) // nc) + 1))
        out.append(dict(fam=4, nq=nq, nc=nc, kd=64, k=min(nc, pick_k([1, 64, 65, 128], 128)), flags=0 if nc < 4096 else NO_FILTER,
                        kind=str(rng.choice(KINDS)), special=None))
    return out


CASES = _family1() + _family2() + _family3() + _family4() + _family5() + _random_cases()
N_CASES = len(CASES)
for _c in CASES:
    _c["path"] = path_label(_c["nq"], _c["nc"], _c["kd"], _c["k"], _c["flags"])
    assert _c["fam"] in (2, 5) or _c["nq"] * _c["nc"] <= WORK


def case_id(i):
    c = CASES[i]
    return "c%03d-f%d-%s-nq%d-nc%d-kd%d-k%d-%s" % (i, c["fam"], c["path"], c["nq"], c["nc"], c["kd"], c["k"], c["kind"])


def split_ranges(nq, nc, kd, k):
    """[c_begin, c_end) of every candidate split of the fused kernels"""
    p = topk_plan(nq, nc, kd, k)
    span = p.tiles_per_wave * 32
    return [(j * span, min((j + 1) * span, nc)) for j in range(p.n_split)]


def gen_case(i, small=False):
    """the tensors of case i; `small`: the same draw at a shape the torch-CPU stand-in ranks in milliseconds"""
    c = dict(CASES[i], index=i)
    rng = np.random.default_rng(7_000_003 * i + 29)
    if small:
        c["nc"] = min(c["nc"], 1500 + i % 7)
        c["nq"] = min(c["nq"], 40)
        c["k"] = min(c["k"], c["nc"])
    nq, nc, kd, k = c["nq"], c["nc"], c["kd"], c["k"]
    plan = topk_plan(nq, nc, kd, k)
    tags = []
    # ---- embeddings
    if c["special"] == "ascending":                             # scores rise with the candidate id: everything beats the threshold
        Q = np.zeros((nq, kd), np.float32)
        Q[:, 0] = 1.0
        C = np.zeros((nc, kd), np.float32)
        C[:, 0] = np.arange(nc, dtype=np.float32)
        tags.append("ascending")
    else:
        common = (rng.standard_normal(kd) * rng.choice([0.0, 0.05, 0.5])).astype(np.float32)
        Q = rng.standard_normal((nq, kd), dtype=np.float32) * np.float32(0.2) + common
        C = rng.standard_normal((nc, kd), dtype=np.float32) * np.float32(0.2) + common * np.float32(rng.choice([1.0, -1.0, 0.0]))
        if rng.random() < 0.5:
            Q *= np.exp2(rng.uniform(-40, 40, (nq, 1))).astype(np.float32)
            tags.append("qspread")
        if rng.random() < 0.3:
            C *= np.exp2(rng.uniform(-12, 12, (nc, 1)) * rng.choice([0.25, 1.0])).astype(np.float32)
            tags.append("cspread")
        if rng.random() < 0.3:
            rows = rng.choice(nc, max(1, min(nc, int(rng.choice([1, 8, 40, max(1, nc // 1000)])))), replace=False)
            C[rows] *= rng.uniform(5, 25, (rows.shape[0], 1)).astype(np.float32)
            tags.append("outliers")
        if rng.random() < 0.2 and nq > 2:
            Q[rng.choice(nq, max(1, nq // 50), replace=False)] = 0.0
            tags.append("zeroq")
        if rng.random() < 0.5 and nc > 4:                       # duplicated candidates: exact ties, across splits where there are any
            for _ in range(int(rng.integers(1, 4))):
                src = int(rng.integers(0, nc))
                C[rng.choice(nc, min(nc - 1, int(rng.choice([2, 30, 300, 1500]))), replace=False)] = C[src]
                if rng.random() < 0.5 and nq > 1:               # ... that ARE somebody's best candidates
                    Q[int(rng.integers(0, nq))] = C[src] * np.float32(rng.uniform(0.5, 2.0))
            tags.append("ties")
        if rng.random() < 0.2 and nq > 3:
            Q[rng.choice(nq, min(nq, 8), replace=False)] = Q[0]
            tags.append("dupq")
        bound = float(np.abs(Q).max()) * float(np.abs(C).max()) * kd
        if bound > 1e8:                                          # beyond the reference's mask sentinel its ranking is an artefact
            Q *= np.float32(np.exp2(-np.ceil(np.log2(bound / 1e8))))
    # ---- mask: the heavy, split-filling, starved and best-masked users are different queries where there are enough
    want = KIND_TAGS[c["kind"]]
    perm = rng.permutation(nq)
    r_600, r_5000, r_fill, r_starved = (int(perm[j % nq]) for j in range(4))
    r_best = np.sort(perm[4:4 + (2 if nq * nc > WORK else 16)]) if nq > 4 else np.sort(perm[:1])
    rows, cols = [np.zeros(0, np.int64)], [np.zeros(0, np.int64)]
    special_rows = []
    if "sparse" in want:
        rows.append(rng.integers(0, nq, nq)), cols.append(rng.integers(0, nc, nq))
    if "perrow" in want:
        n = min(nq * int(rng.integers(16, 41)), 400_000)
        rows.append(rng.integers(0, nq, n)), cols.append(rng.integers(0, nc, n))
    if "heavy" in want:
        for m, q in ((600, r_600), (5000, r_5000)):
            m = min(m, nc)
            rows.append(np.full(m, q)), cols.append(rng.choice(nc, m, replace=False))
        if plan.n_split > 1:            # one split's whole range, and the FIRST id of another split (the cursor's start), for one user
            rg = split_ranges(nq, nc, kd, k)
            j = int(rng.integers(0, len(rg)))
            j2 = (j + 1 + int(rng.integers(0, len(rg) - 1))) % len(rg) if len(rg) > 2 else 1 - j
            fill = np.arange(*rg[j]) if rg[j][1] - rg[j][0] <= 140_000 else np.arange(rg[j][0], rg[j][0] + 140_000)
            fill = np.concatenate([fill, [rg[j2][0]], rng.integers(0, nc, 100)])
            c["fill"] = (r_fill, rg[j], rg[j2][0])
        else:                           # block paths: one contiguous run (whole groups of the streaming GEMM's maxima)
            c0 = int(rng.integers(0, max(1, nc - 600)))
            fill = np.arange(c0, min(nc, c0 + 600))
        rows.append(np.full(fill.shape[0], r_fill)), cols.append(fill)
        special_rows += [r_600, r_5000, r_fill]
    if "bestmasked" in want:            # train positives score HIGH
        s = Q[r_best] @ C.T
        nb = min(nc, int(rng.choice([3, 20, 100])))
        best = np.argpartition(-s, nb - 1, axis=1)[:, :nb]
        rows.append(np.repeat(r_best, nb)), cols.append(best.reshape(-1))
        special_rows += r_best.tolist()
        del s
    if "starved" in want:               # fewer than k unmasked candidates for one query
        keep = int(rng.integers(0, k + 1))
        drop = rng.permutation(nc)[:nc - keep]
        rows.append(np.full(drop.shape[0], r_starved)), cols.append(drop)
        special_rows.append(r_starved)
        c["starved"] = (r_starved, keep)
    if want == {"none"}:
        mask = None
    else:
        key = np.unique(np.concatenate(rows).astype(np.int64) * nc + np.concatenate(cols).astype(np.int64))
        mask = np.stack([key // nc, key % nc])
        mask = mask[:, rng.permutation(mask.shape[1])]          # unsorted, as the loader hands it over
    # the rows compared with float64: all, or (more than WORK scores) rows 0, 31, 32, the last, the three around every block
    # seam, the heavy / split-filling / best-masked / starved rows and 16 random ones
    check_rows = None
    if nq * nc > WORK:
        seams = [q0 + d for q0 in range(plan.qb_rows, nq, plan.qb_rows) for d in (-1, 0, 1)] if plan.materialise else []
        extra = rng.integers(0, nq, 16).tolist() if nq > 64 else []
        check_rows = np.unique(np.array([r for r in [0, 31, 32, nq - 1] + seams + special_rows + extra if 0 <= r < nq], np.int64))
    c.update(Q=Q, C=C, mask=mask, tags=tags + sorted(want), check_rows=check_rows, plan=plan)
    return c


def describe(c):
    return "case %d (family %d, %s): nq %d nc %d kd %d k %d flags %d masked %d %s" % (
        c["index"], c["fam"], c["path"], c["nq"], c["nc"], c["kd"], c["k"], c["flags"],
        0 if c["mask"] is None else c["mask"].shape[1], "+".join(c["tags"]))


def local_mask_rows(mask, rows):
    """the [2, n] mask restricted to the ascending `rows`, row ids relative to the sample"""
    pos = np.searchsorted(rows, mask[0])
    hit = (pos < rows.shape[0]) & (rows[np.minimum(pos, rows.shape[0] - 1)] == mask[0])
    return np.stack([pos[hit], mask[1][hit]])


NO_MASK = np.zeros((2, 0), np.int64)


def float64_scores(Qt, Ct):
    if Ct.numel() <= 1 << 26:
        return Qt.double() @ Ct.double().t()
    q = Qt.double()
    return torch.cat([q @ Ct[a:a + (1 << 18)].double().t() for a in range(0, Ct.shape[0], 1 << 18)], dim=1)


def worst_value_error(idx, val, Qt, Ct, s64):
    """max |val - s64| / (|q| |c|) over the ranked, unmasked entries: what the checker holds to 2e-6"""
    qn, cn = Qt.double().norm(dim=1)[:, None], Ct.double().norm(dim=1)[idx]
    ok = (val != float(MASKED)) & (qn * cn > 0)
    err = (val.double() - torch.gather(s64, 1, idx)).abs() / (qn * cn).clamp_min(1e-300)
    return float(err[ok].max()) if bool(ok.any()) else 0.0


def check_case(c, run):
    """`run(c, mask)` -> (idx [nq, k] int64, val fp32) on the CPU, mask [2, n] or None.  Lists against float64 by `check_lists`;
    returns the lists and the worst relative value error."""
    Qt, Ct = torch.from_numpy(c["Q"]), torch.from_numpy(c["C"])
    rows = c["check_rows"]
    mask = NO_MASK if c["mask"] is None else c["mask"]
    idx, val = run(c, c["mask"])
    assert tuple(idx.shape) == (c["nq"], c["k"]) and tuple(val.shape) == (c["nq"], c["k"])
    if rows is not None:
        Qs, sel, mask = Qt[rows], (lambda t: t[rows]), local_mask_rows(mask, rows)
    else:
        Qs, sel = Qt, (lambda t: t)
    s64 = float64_scores(Qs, Ct)
    check_lists(describe(c), sel(idx), sel(val), Qs, Ct, mask, c["k"], s64)
    err = worst_value_error(sel(idx), sel(val), Qs, Ct, s64)
    if c["special"] == "unmasked_too" and c["mask"] is not None:
        ui, uv = run(c, None)
        check_lists(describe(c) + " (no mask)", sel(ui), sel(uv), Qs, Ct, NO_MASK, c["k"], s64)
    return idx, val, err


# ------------------------------------------------------------------------------------------------ GPU plumbing
class ExactWorkspace(Workspace):
    """tests/test_graph_build_fuzz_gpu.py's Workspace; only the guard bytes come back to the host (a workspace here has up to 5 GB)"""

    def check(self, name=""):
        front, back = self.buf[:WS_GUARD].cpu().numpy(), self.buf[WS_GUARD + self.n:].cpu().numpy()
        assert (front == 0xA5).all() and (back == 0xA5).all() and back.shape[0] == WS_GUARD, (name, "workspace guards overwritten", self.n)


def csr_on_device(mask, nq):
    from mmrec_amd import hip_ops
    if mask is None:
        return None, None
    rp, col = hip_ops.mask_to_csr(mask, nq, torch.device("cuda", 0))
    return rp, (col if col.numel() else torch.zeros(1, dtype=torch.int32, device=rp.device))


def run_raw(what, Qd, Cd, k, rp, col, flags, prepared=None):
    """one call of mmrec_score_topk_f32 (or _prepared_f32) with guarded outputs and an exact-size guarded workspace"""
    lib, s = _lib()
    (nq, kd), nc = Qd.shape, Cd.shape[0]
    nbytes = lib.mmrec_topk_workspace_bytes(nq, nc, kd, k)
    assert nbytes == workspace_bytes(nq, nc, kd, k), (what, nbytes, workspace_bytes(nq, nc, kd, k))
    ws, oi, ov = ExactWorkspace(nbytes), Guarded(nq * k, I64), Guarded(nq * k, F32)
    if prepared is None:
        rc = lib.mmrec_score_topk_f32(P(Qd), P(Cd), nq, nc, kd, P(rp), P(col), k, P(oi.view), P(ov.view), ws.ptr, flags, s)
    else:
        rc = lib.mmrec_score_topk_prepared_f32(P(Qd), P(Cd), P(prepared), nq, nc, kd, P(rp), P(col), k, P(oi.view), P(ov.view),
                                               ws.ptr, flags, s)
    assert rc == 0, (what, rc)
    torch.cuda.synchronize()
    ws.check(what)
    return torch.from_numpy(oi.get(what).reshape(nq, k)), torch.from_numpy(ov.get(what).reshape(nq, k))


def same_bits(a, b, what):
    assert torch.equal(a[0], b[0]), (what, "ids differ", torch.nonzero((a[0] != b[0]).any(1)).flatten()[:4].tolist())
    assert torch.equal(a[1].view(torch.int32), b[1].view(torch.int32)), (what, "values differ")


class DeviceRun:
    """`run` of check_case on the device through the raw ABI; keeps the operands for the follow-up calls"""

    def __init__(self, c):
        self.Qd, self.Cd = _dev(c["Q"]), _dev(c["C"])
        self.csr = {}

    def __call__(self, c, mask):
        key = mask is None
        if key not in self.csr:
            self.csr[key] = csr_on_device(mask, c["nq"])
        return run_raw(describe(c), self.Qd, self.Cd, c["k"], *self.csr[key], c["flags"])


GENERIC = [i for i in range(N_CASES) if CASES[i]["fam"] != 5]


@pytest.mark.gpu
@pytest.mark.parametrize("i", GENERIC, ids=case_id)
def test_fp32_path_case_vs_float64(i):
    c = gen_case(i)
    assert c["path"] in PATHS and c["path"] == path_label(c["nq"], c["nc"], c["kd"], c["k"], c["flags"])
    run = DeviceRun(c)
    idx, val, err = check_case(c, run)
    print("PATH %s worst |val - s64| / (|q| |c|) = %.3g (%s)" % (c["path"], err, describe(c)))
    same_bits(run(c, c["mask"]), (idx, val), describe(c) + " second run")
    lib, s = _lib()
    if c["fam"] == 4 and lib.mmrec_topk_prepared_bytes(c["nc"], c["kd"]) > 0:
        # flags 0: the prepared entry point equals the plain one bit for bit (include/mmrec_hip.h)
        rp, col = run.csr[c["mask"] is None]
        nb = lib.mmrec_topk_prepared_bytes(c["nc"], c["kd"])
        assert nb == filter_prepared_bytes(c["nc"], c["kd"])
        prep = ExactWorkspace(nb)
        assert lib.mmrec_topk_prepare_f32(P(run.Cd), c["nc"], c["kd"], prep.ptr, s) == 0
        plain = run_raw(describe(c) + " flags 0", run.Qd, run.Cd, c["k"], rp, col, 0)
        prepared = run_raw(describe(c) + " prepared", run.Qd, run.Cd, c["k"], rp, col, 0, prepared=prep.buf[WS_GUARD:])
        prep.check("prepared")
        same_bits(prepared, plain, describe(c) + " prepared against plain")


@pytest.mark.gpu
def test_two_query_blocks_equal_two_calls():
    """family 5: 2049 queries x 1,000,001 candidates of kd = 64 is walked in score blocks of 1152 and 897 queries (the `q0` loop):
    the checked rows (gen_case) against float64, and ALL rows bit for bit against two separate calls on the two blocks with the
    mask re-based"""
    i = next(j for j in range(N_CASES) if CASES[j]["fam"] == 5)
    c = gen_case(i)
    qb = c["plan"].qb_rows
    assert c["path"] == "mat64_blocks" and 0 < qb < c["nq"] <= 2 * qb
    assert all(q in c["check_rows"] for q in (0, qb - 1, qb, qb + 1, c["nq"] - 1))
    run = DeviceRun(c)
    idx, val, err = check_case(c, run)
    print("PATH %s worst |val - s64| / (|q| |c|) = %.3g (%s)" % (c["path"], err, describe(c)))
    same_bits(run(c, c["mask"]), (idx, val), describe(c) + " second run")
    rp, col = run.csr[False]
    rph = rp.cpu().numpy().astype(np.int64)
    for a, b in ((0, qb), (qb, c["nq"])):
        assert path_label(b - a, c["nc"], c["kd"], c["k"], 0) == "mat64"
        brp = (rp[a:b + 1] - int(rph[a])).contiguous()
        bcol = col[int(rph[a]):max(int(rph[b]), int(rph[a]) + 1)].contiguous()
        part = run_raw(describe(c) + " rows %d..%d alone" % (a, b), run.Qd[a:b], run.Cd, c["k"], brp, bcol, 0)
        same_bits(part, (idx[a:b], val[a:b]), describe(c) + " rows %d..%d alone" % (a, b))


# ------------------------------------------------------------------------------------------------ hip_ops._score_topk_blocked
BLOCK = 96


def blocked_masks(nq, nc, Q, C, rng):
    """none; rows without entries on both sides of every seam; all entries in the last block; a first block without any"""
    seams = list(range(BLOCK, nq, BLOCK))
    last0 = seams[-1]
    per = lambda rows, n: np.stack([np.repeat(rows, n), rng.integers(0, nc, rows.shape[0] * n)])
    best = lambda rows, n: np.stack([np.repeat(rows, n), np.argsort(-(Q[rows] @ C.T), axis=1)[:, :n].reshape(-1)])
    allq = np.arange(nq)
    away = allq[np.min(np.abs(allq[:, None] - np.array(seams)[None, :] + 0.5), axis=1) > 2]     # not within 2 rows of a seam
    out = {"none": None,
           "seamgaps": np.concatenate([per(away, 5), best(away[::7], 3)], axis=1),
           "lastonly": np.concatenate([per(allq[last0:], 40), best(allq[last0:], 20)], axis=1),
           "firstnone": np.concatenate([per(allq[BLOCK:], 5), best(allq[BLOCK::5], 10)], axis=1)}
    for name, m in out.items():
        if m is not None:
            key = np.unique(m[0].astype(np.int64) * nc + m[1])
            m = np.stack([key // nc, key % nc])
            out[name] = m[:, rng.permutation(m.shape[1])]
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("nq", (193, 289, 300))
def test_query_blocks_of_96_equal_the_unblocked_call(nq, monkeypatch):
    """family 6: with TOPK_QUERY_BLOCK = 96 these calls are walked in blocks whose last has 1, 1 and 12 rows; cold, warm (lists of a
    larger table read through permuted `hint_rows`; one list per query), with hint_update=False and with queue_counts: ids and
    values equal the unblocked call's bit for bit, which check_lists holds against float64"""
    from mmrec_amd import hip_ops
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(4100 + nq)
    nc, kd, k = 4100, 64, 20
    Q = (rng.standard_normal((nq, kd)) * 0.2 + 0.05).astype(np.float32) * np.exp2(rng.uniform(-20, 20, (nq, 1))).astype(np.float32)
    C = (rng.standard_normal((nc, kd)) * 0.2 + 0.05).astype(np.float32)
    C[rng.choice(nc, 300, replace=False)] = C[5]
    Q[nq - 1] = C[5] * np.float32(1.5)                           # the last block's last row ranks an exact tie
    Qt, Ct = torch.from_numpy(Q), torch.from_numpy(C)
    Qd, Cd = Qt.to(dev), Ct.to(dev)
    s64 = float64_scores(Qt, Ct)
    calls = []
    inner = hip_ops._score_topk_blocked
    for name, mask in blocked_masks(nq, nc, Q, C, rng).items():
        what = "nq %d mask %s" % (nq, name)
        rp, col = (None, None) if mask is None else hip_ops.mask_to_csr(mask, nq, dev)
        assert hip_ops.TOPK_QUERY_BLOCK == 65536
        ref = hip_ops.score_topk(Qd, Cd, k, rp, col, return_values=True)
        check_lists(what, ref[0].cpu(), ref[1].cpu(), Qt, Ct, NO_MASK if mask is None else mask, k, s64)
        with monkeypatch.context() as mp:
            mp.setattr(hip_ops, "TOPK_QUERY_BLOCK", BLOCK)
            mp.setattr(hip_ops, "_score_topk_blocked", lambda *a, **kw: (calls.append(what), inner(*a, **kw))[1])
            n0 = len(calls)
            same_bits(hip_ops.score_topk(Qd, Cd, k, rp, col, return_values=True), ref, what + " cold")
            assert torch.equal(hip_ops.score_topk(Qd, Cd, k, rp, col), ref[0])
            counts = torch.zeros(2, dtype=torch.int32, device=dev)
            # warm: a stale ranking stored in a table with more rows than queries, read through permuted hint_rows
            stale = torch.topk(torch.nan_to_num(Qt @ (Ct + 0.05 * torch.from_numpy(rng.standard_normal(C.shape).astype(np.float32))).t()),
                               k + 3, dim=1)[1].to(torch.int32)
            rows = torch.from_numpy(rng.permutation(nq + 7)[:nq].astype(np.int64))
            table = torch.full((nq + 7, k + 3), -1, dtype=torch.int32)
            table[rows] = stale
            td, rd = table.to(dev), rows.to(dev)
            same_bits(hip_ops.score_topk(Qd, Cd, k, rp, col, return_values=True, hint=td, hint_rows=rd, queue_counts=counts), ref,
                      what + " warm, hint_rows")
            assert torch.equal(td[rd][:, :k].long(), ref[0]), (what, "the rows do not hold the call's top-k")
            others = torch.ones(nq + 7, dtype=torch.bool)
            others[rows] = False
            assert bool((td.cpu()[others] == -1).all()), (what, "a row of no query was written")
            c1 = counts.clone()
            assert int(c1.min()) >= 0
            # one list per query, no rows: the first call's lists, then kept (hint_update=False)
            own = torch.full((nq, 64), -1, dtype=torch.int32, device=dev)
            own[:, :k] = ref[0].to(torch.int32)
            same_bits(hip_ops.score_topk(Qd, Cd, k, rp, col, return_values=True, hint=own, queue_counts=counts), ref, what + " warm")
            assert torch.equal(own[:, :k].long(), ref[0]) and bool((counts >= c1).all())
            kept, c2 = own.clone(), counts.clone()
            same_bits(hip_ops.score_topk(Qd, Cd, k, rp, col, return_values=True, hint=own, hint_update=False, queue_counts=counts),
                      ref, what + " warm, lists kept")
            assert torch.equal(own, kept) and bool((counts >= c2).all())
            cold = torch.full((nq, 64), -7, dtype=torch.int32, device=dev)
            assert torch.equal(hip_ops.score_topk(Qd, Cd, k, rp, col, hint=cold, hint_cold=True), ref[0])
            assert torch.equal(cold[:, :k].long(), ref[0]) and int(cold.min()) >= -1
            assert len(calls) - n0 == 6, (what, "the calls were not walked in blocks")


# ------------------------------------------------------------------------------------------------ the argument contract
@pytest.mark.gpu
def test_argument_contract_before_any_launch():
    """family 7: every refusal of score_topk_impl / the prepare entry points as include/mmrec_hip.h states it, in the order
    score_topk_impl checks; outputs pre-filled, workspace guarded: nothing is written"""
    lib, s = _lib()
    nq, nc, kd, k = 8, 200, 64, 10
    Q, C = _dev(np.ones((nq, 260), F32)), _dev(np.ones((nc, 260), F32))
    rp, col = _dev(np.zeros(nq + 1, I32)), _dev(np.zeros(4, I32))
    oi, ov = Guarded(nq * 128, I64), Guarded(nq * 128, F32)
    ws = ExactWorkspace(lib.mmrec_topk_workspace_bytes(nq, nc, 260, 64))

    def call(nq=nq, nc=nc, kd=kd, k=k, flags=0, rp=rp, col=col):
        return lib.mmrec_score_topk_f32(P(Q), P(C), nq, nc, kd, P(rp), P(col), k, P(oi.view), P(ov.view), ws.ptr, flags, s)

    for bad_kd in (1, 2, 3, 6, 62, 63, 65, 0, -4, -64):
        assert call(kd=bad_kd) == UNSUPPORTED, bad_kd
    for bad_k in (nc + 1, 0, -1, 129, 1000):
        assert call(k=bad_k) == BAD_ARG, bad_k
    assert call(nc=5, k=6) == BAD_ARG
    for flags in (2, 4, 3, 1 << 30, -2):
        assert call(flags=flags) == BAD_ARG, flags
    assert call(rp=None) == BAD_ARG                              # mask_col without mask_rowptr
    assert call(nq=0) == 0 and call(nq=0, rp=None, col=None) == 0
    for bad_kd in (4, 20, 36, 100, 132, 260):                    # k in (64, 128] off the 32-grid: the fused path ranks k <= 64
        for big_k in (65, 100, 128):
            assert call(kd=bad_kd, k=big_k) == UNSUPPORTED, (bad_kd, big_k)
    # ... and above 2,097,152 candidates: refused from the plan alone, before the table is read (none of that size is allocated)
    for wide_kd in (64, 128, 96):
        for big_k in (65, 128):
            assert call(nc=NC_FUSED, kd=wide_kd, k=big_k) == UNSUPPORTED, (wide_kd, big_k)
    assert path_label(nq, NC_FUSED - 1, 64, 65, NO_FILTER) == "mat64" and path_label(nq, NC_FUSED, 64, 64, 0) == "two_pass"
    # the candidate-side preparation: (nc, kd) the fp16 filter does not serve
    for unserved in ((4095, 64), (1_000_001, 64), (5000, 32), (5000, 192), (5000, 20), (0, 64), (-5, 128), (200, 128)):
        assert lib.mmrec_topk_prepared_bytes(*unserved) == 0, unserved
        if unserved[0] > 0:
            assert lib.mmrec_topk_prepare_f32(P(C), unserved[0], unserved[1], ws.ptr, s) == UNSUPPORTED, unserved
    assert lib.mmrec_topk_prepared_bytes(4096, 64) == filter_prepared_bytes(4096, 64) > 0
    assert lib.mmrec_topk_prepare_f32(None, 5000, 64, ws.ptr, s) == BAD_ARG and lib.mmrec_topk_prepare_f32(P(C), 5000, 64, None, s) == BAD_ARG
    assert lib.mmrec_score_topk_prepared_f32(P(Q), P(C), None, nq, nc, kd, P(rp), P(col), k, P(oi.view), P(ov.view), ws.ptr, 0, s) == BAD_ARG
    torch.cuda.synchronize()
    oi.untouched("argument contract"), ov.untouched("argument contract"), ws.check("argument contract")
