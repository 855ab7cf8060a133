"""Seeded differential fuzz of the two device kernels of csrc/evalsample.hip through the raw C ABI: `mmrec_topk_metrics_f64` (hit
matrix + per-user Recall / NDCG / Precision / MAP) and `mmrec_sample_negatives_i64` (one uniform negative per sample), each against
a numpy restatement written here from the text of include/mmrec_hip.h, never against another path of the project.

Metrics.  For user u with the sorted ground-truth row T (pos_len entries) and the k ranked ids, j = 0 .. k-1 in rank order:
    hit_j = id_j in T;  cum += hit_j;  dcg += hit_j ? discount[j] : 0;  sum_pre += (cum / (j + 1)) * hit_j
    cap = min(pos_len, k);  at a cut-off j + 1:   recall = cum / pos_len           ndcg = dcg / idcg_cum[min(j, cap - 1)]
                                                  precision = cum / (j + 1)        map  = sum_pre / min(j + 1, cap)
    and for a row without ground truth (cap = 0) ndcg = dcg / idcg_cum[k - 1], map = sum_pre / k, recall = 0 / 0 = NaN.
The reference is float64 numpy with the same sequential sums (a Python loop over the ranks, vectorised over the users); discount
and idcg_cum are inputs of the call, so both sides read the same doubles.  Why the comparison is BIT FOR BIT (hit matrix and all
four metrics at every cut-off, per user): every operation is one IEEE double add or divide of identical operands in identical
order; the kernel's only multiply is by 0.0 or 1.0, which is exact, so a contraction of `sum_pre + q * h` to an fma cannot change
a bit.  NaN (the recall of an empty row) is compared as NaN: the sign of 0 / 0 is not fixed by IEEE 754 (x86 gives the negative
quiet NaN, the GPU the positive one).  A mismatch names the expression that differs, nothing is loosened to a tolerance.
A `-1` id never hits (it is below every item id), an id repeated inside a ranking counts at both ranks (as `np.isin` does), a
repeated cut-off fills both of its slots.

Sampler.  mix64 = splitmix64's output function, G = 0x9E3779B97F4A7C15, all uint64 arithmetic mod 2^64:
    s = mix64(mix64(mix64(seed + G) + counter) + b);   draw t = 1, 2, ...: r = mix64(s + t G) >> 32, item = cand[(r n_cand) >> 32]
    redrawn while the item is in the user's sorted history, at most 4096 draws, the item of the last draw is returned.
Integer work: the device ids must equal the restatement's id for id, and next to that every output is a candidate and lies outside
the user's history wherever the restatement did not exhaust its 4096 draws.  The quality of the generator is tested on the
restatement alone, on the CPU: (a) for every seed of SEEDS and counters 0, 1, 7 the 4096 x 64 generator states of 4096 samples
are pairwise distinct -- the earlier seeding `seed ^ (counter C + b G)` fails that at seeds 0, 1, 2 and 2^64 - 1 (sample b + 1
repeats sample b one draw late; `test_parent_seeding_is_rejected` keeps that seeding as a planted error); (b) one user with 30 of 100 candidates in the
history, 200,000 samples: every allowed item's count within 6 sqrt(expected) of expected = 200,000 / 70 -- the bound of
tests/test_models_gpu.py::test_device_negative_sampler (a 6 sigma event of a binomial: 2e-9 per item).

Every output buffer (out_per_user, hit_out, out_neg) is pre-filled and carries GUARD sentinel elements on both sides, checked
after each call.  `draw_case(seed)` is deterministic in the seed; `test_cases_span_every_axis` asserts every axis value to occur;
`test_checker_rejects_planted_errors` shows that the restatement passes and each planted error fails on at least one drawn case.
One planted error of the issue's list cannot fail and the test says why: `cap = pos_len` without the min with k is the same
function, because cap enters only as min(j, cap - 1) and min(j + 1, cap) with j + 1 <= k (asserted: it passes every case).

On one MI355X the 67 device tests take 4.0 s (the slowest, the evaluator's, 0.6 s; a sampler case of 2^20 + 7 candidates 0.15 s);
the 5 CPU tests 5 s, 4 of them `test_cases_span_every_axis`, which draws every case and computes every reference.
"""
import ctypes

import numpy as np
import pytest
import torch

F64, U64, I64, I32 = np.float64, np.uint64, np.int64, np.int32
GUARD = 64
GUARD_VALUE = {np.dtype(F64): 12345.0, np.dtype(I64): 12345, np.dtype(np.uint8): 0xA5, np.dtype(I32): 12345}
FILL = {np.dtype(F64): -7.0, np.dtype(I64): -77, np.dtype(np.uint8): 9}
BAD_ARG = 10001
METRICS = ("recall: cum / pos_len", "ndcg: dcg / idcg_cum[held]", "precision: cum / (j + 1)", "map: sum_pre / min(j + 1, cap)")

# ---- metrics axes
M_USERS = (1, 255, 256, 257, 1000)
M_K = (1, 2, 5, 50, 128)
M_CUTS = ("one", "k", "all", "std", "repeat")
M_POS = ("0", "1", "k-1", "k", "k+1", "3k")
M_RANK = ("none", "sparse", "all", "first", "last", "pad", "dup")
N_METRIC = 25
METRIC_PLANTS = ("cap_no_min", "held_j", "map_div_j1", "recall_div_cap", "cutoff_late", "unsorted_truth")
EQUIVALENT_PLANTS = ("cap_no_min",)                         # the same function: see the module docstring

# ---- sampler axes
S_BATCH = (0, 1, 255, 256, 257, 5000)
S_NCAND = (1, 2, 3, 64, 1000, 2 ** 20 + 7)
SEEDS = (0, 1, 2, 999, 2 ** 63, 2 ** 64 - 1)
COUNTERS = (0, 1, 2 ** 32 + 5, 2 ** 64 - 1)
S_HIST = ("empty", "one", "noncand", "all_but_one", "full", "mixed")
N_SAMPLER = 36
SAMPLER_PLANTS = ("no_rejection", "modulo", "counter_ignored", "bound_4095")
MAX_DRAWS = 4096
G = U64(0x9E3779B97F4A7C15)
C_PARENT = U64(0xD1B54A32D192ED03)
MASK64 = 2 ** 64 - 1


# ------------------------------------------------------------------------------------------------ metrics: cases
class Case:
    def axes(self):
        keys = ("seed", "kind", "n_users", "k", "cuts", "hit_out", "batch", "n_cand", "rng_seed", "counter", "shuffled")
        return " ".join("%s=%s" % (k, getattr(self, k)) for k in keys if hasattr(self, k))


def cut_list(kind, k):
    if kind == "one":
        return (1,)
    if kind == "k":
        return (k,)
    if kind == "std" and k >= 50:
        return (5, 10, 20, 50)
    if kind == "repeat":                                    # ascending with a cut-off twice: only the raw ABI takes it
        return tuple(sorted((1, max(k // 2, 1), max(k // 2, 1), k)))
    return tuple(range(1, k + 1))


def _draw_metrics(c, i, rng):
    c.kind = "metrics"
    c.n_users = n = M_USERS[i % 5]
    c.k = k = M_K[(i + i // 5) % 5]
    c.cuts = M_CUTS[(2 * i + i // 5) % 5]
    if c.cuts == "std" and k < 50:
        c.cuts = "all"
    c.ks = cut_list(c.cuts, k)
    c.hit_out = i % 2 == 0
    c.n_items = ni = 4 * k + 16
    off = int(rng.integers(0, 42))
    c.pos_kind = [M_POS[((u + off) // 7) % 6] for u in range(n)]
    c.rank_kind = [M_RANK[(u + off) % 7] for u in range(n)]
    lens = {"0": 0, "1": 1, "k-1": k - 1, "k": k, "k+1": k + 1, "3k": 3 * k}
    truth, topk = [], np.empty((n, k), I64)
    for u in range(n):
        L = lens[c.pos_kind[u]]
        perm = rng.permutation(ni)
        T = perm[:L].copy()
        if L >= 1 and u % 3 == 0:                           # the smallest and the largest item id as ground truth
            T[0] = 0 if 0 not in T else T[0]
            if L >= 2 and ni - 1 not in T:
                T[1] = ni - 1
        T = np.unique(T)
        assert T.size == L
        N = np.setdiff1d(perm, T, assume_unique=True)       # keeps perm's (random) order
        Tp = rng.permutation(T)
        kind = c.rank_kind[u]
        row, ti, ni_ = np.empty(k, I64), 0, 0
        for j in range(k):
            if kind == "all":
                want = ti < L
            elif kind == "first":
                want = j == 0
            elif kind == "last":
                want = j == k - 1
            elif kind == "none":
                want = False
            else:
                want = rng.random() < 0.3
            if want and ti < L:
                row[j], ti = Tp[ti], ti + 1
            else:
                row[j], ni_ = N[ni_], ni_ + 1
        if kind == "pad":                                   # -1 padding at the tail (the whole row at k = 1)
            row[int(rng.integers(0, k)) if k > 1 else 0:] = -1
        if kind == "dup" and k >= 2 and L >= 1:             # one truth id at two ranks: both count
            row[0] = row[k - 1] = Tp[0]
        topk[u] = row
        truth.append(T.astype(I32))
    c.topk, c.truth = topk, truth
    c.pos_len = np.array([t.size for t in truth], I64)
    c.rowptr = np.concatenate([[0], np.cumsum(c.pos_len)]).astype(I32)
    c.col = np.concatenate(truth + [np.zeros(0, I32)]).astype(I32)
    c.discount = 1.0 / np.log2(np.arange(1, k + 1, dtype=F64) + 1)
    c.idcg = np.cumsum(c.discount)


# ------------------------------------------------------------------------------------------------ metrics: the restatement
def metrics_ref(c, plant=None):
    """hit [n, k] bool and out [n, 4, n_ks] float64 by the formulas of the header; `plant`: one planted error"""
    n, k = c.n_users, c.k
    pos_len = c.pos_len
    if plant == "unsorted_truth":                           # a binary search over a row that is not sorted
        hit = np.zeros((n, k), bool)
        for u in range(n):
            T = c.truth[u][::-1]
            if T.size:
                p = np.minimum(np.searchsorted(T, c.topk[u]), T.size - 1)
                hit[u] = T[p] == c.topk[u]
    else:
        stride = I64(c.n_items)
        keys = np.arange(n, dtype=I64)[:, None] * stride + c.topk
        tkeys = np.repeat(np.arange(n, dtype=I64), pos_len) * stride + c.col.astype(I64)
        hit = np.isin(keys, tkeys) & (c.topk >= 0)          # (u stride - 1 is the previous user's largest id, not "-1")
    cap = pos_len if plant == "cap_no_min" else np.minimum(pos_len, k)
    cum, dcg, sum_pre = np.zeros(n), np.zeros(n), np.zeros(n)
    curve = np.empty((n, 4, k))
    with np.errstate(invalid="ignore", divide="ignore"):
        for j in range(k):
            h = hit[:, j].astype(F64)
            cum = cum + h
            dcg = dcg + np.where(hit[:, j], c.discount[j], 0.0)
            sum_pre = sum_pre + (cum / F64(j + 1)) * h
            held = np.where(cap > 0, np.minimum(j, cap - 1), k - 1)
            div = np.where(cap > 0, np.minimum(j + 1, cap), k)
            if plant == "held_j":
                held = np.full(n, j)
            if plant == "map_div_j1":
                div = np.full(n, j + 1)
            curve[:, 0, j] = cum / (np.minimum(pos_len, k) if plant == "recall_div_cap" else pos_len).astype(F64)
            curve[:, 1, j] = dcg / c.idcg[held]
            curve[:, 2, j] = cum / F64(j + 1)
            curve[:, 3, j] = sum_pre / div.astype(F64)
    at = np.array([min(x, k - 1) if plant == "cutoff_late" else x - 1 for x in c.ks])
    return hit, np.ascontiguousarray(curve[:, :, at])


_MREF = {}


def metrics_reference(c):
    if c.seed not in _MREF:
        _MREF[c.seed] = metrics_ref(c)
    return _MREF[c.seed]


def same_doubles(got, ref):
    """bit for bit, a NaN equal to a NaN"""
    got, ref = np.ascontiguousarray(got, F64), np.ascontiguousarray(ref, F64)
    return (got.view(I64) == ref.view(I64)) | (np.isnan(got) & np.isnan(ref))


def check_metrics(c, hit, out):
    """hit: [n, k] (or None where the call passed NULL), out: [n, 4, n_ks]"""
    hit_ref, out_ref = metrics_reference(c)
    if hit is not None:
        bad = np.asarray(hit).astype(bool) != hit_ref
        assert set(np.unique(hit).tolist()) <= {0, 1} and not bad.any(), (c.axes(), "hit matrix", int(bad.sum()),
                                                                           "first at", tuple(np.argwhere(bad)[0]) if bad.any() else None)
    assert out.shape == out_ref.shape, (c.axes(), out.shape, out_ref.shape)
    ok = same_doubles(out, out_ref)
    if not ok.all():
        u, m, t = (int(x) for x in np.argwhere(~ok)[0])
        raise AssertionError((c.axes(), "bits differ in " + METRICS[m], int((~ok).sum()), "first at user %d cut-off %d" % (u, c.ks[t]),
                              "pos_len", int(c.pos_len[u]), "got", float(out[u, m, t]), "ref", float(out_ref[u, m, t])))
    empty = c.pos_len == 0                                  # the documented empty-row result, spelled out
    assert np.isnan(out[empty, 0]).all() and (out[empty, 1:] == 0.0).all(), (c.axes(), "empty ground-truth rows")


# ------------------------------------------------------------------------------------------------ sampler: cases
def _draw_sampler(c, i, rng):
    c.kind = "sampler"
    c.batch = S_BATCH[i % 6]
    c.n_cand = nc = S_NCAND[i // 6]
    c.rng_seed = SEEDS[(i + i // 6) % 6]
    c.counter = COUNTERS[(i + i // 6) % 4]
    c.shuffled = i % 2 == 1
    cand = 3 * np.arange(nc, dtype=I64) + 5 + rng.integers(0, 2, nc)      # sparse, 2 or 0 mod 3; the index is never the id
    non = 3 * np.arange(40, dtype=I64) + 7                                # 1 mod 3: never a candidate
    if c.shuffled:
        cand = rng.permutation(cand)
    c.cand = cand.astype(I32)
    hists, kinds = [], []
    for u in range(8):
        kind = ("empty", "one", "noncand", "all_but_one", "full", "mixed", "empty", "one")[u]
        if kind == "all_but_one" and nc > 64:
            kind = "mixed"
        if kind == "full" and nc > 1000:
            kind = "noncand"
        if kind == "one":
            h = cand[[int(rng.integers(0, nc))]]
        elif kind == "noncand":
            h = non[:int(rng.integers(1, 40))]
        elif kind == "all_but_one":
            h = np.delete(cand, int(rng.integers(0, nc)))
        elif kind == "full":
            h = cand
        elif kind == "mixed":
            h = np.concatenate([rng.permutation(cand)[:min(nc, 1000) * 3 // 10], non[:5]])
        else:
            h = np.zeros(0, I64)
        hists.append(np.unique(h).astype(I32))
        kinds.append(kind)
    c.hists, c.hist_kind = hists, kinds
    c.rowptr = np.concatenate([[0], np.cumsum([h.size for h in hists])]).astype(I32)
    c.col = np.concatenate(hists + [np.zeros(1, I32)]).astype(I32)        # (one spare entry: never an empty buffer)
    c.users = rng.integers(0, 8, c.batch).astype(I64)                     # 8 users: repeated in every batch beyond 8
    if c.batch >= 255:
        c.users[:8] = np.arange(8)
    c.full_user = np.array([np.isin(cand, h).all() for h in hists])


# ------------------------------------------------------------------------------------------------ sampler: the restatement
def mix64(z):
    with np.errstate(over="ignore"):
        z = (z ^ (z >> U64(30))) * U64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> U64(27))) * U64(0x94D049BB133111EB)
        return z ^ (z >> U64(31))


def first_state(seed, counter, b, seeding="mixed"):
    """the state of samples b (uint64 array) before their first draw"""
    seed, counter = np.full(1, seed & MASK64, U64), np.full(1, counter & MASK64, U64)
    b = np.asarray(b).astype(U64)
    with np.errstate(over="ignore"):
        if seeding == "parent":                             # the seeding this file's disjointness test was written against
            return seed ^ (counter * C_PARENT + b * G)
        return mix64(mix64(mix64(seed + G) + counter) + b)


def sampler_ref(c, plant=None, seeding="mixed"):
    """(ids int64 [batch], draws used [batch], exhausted [batch] bool)"""
    nb, nc = c.batch, c.n_cand
    stride = I64(2 ** 32)
    hkeys = np.repeat(np.arange(8, dtype=I64), np.diff(c.rowptr)) * stride + c.col[:c.rowptr[-1]].astype(I64)   # sorted
    s = np.broadcast_to(first_state(c.rng_seed, 0 if plant == "counter_ignored" else c.counter, np.arange(nb), seeding), (nb,)).copy()
    item = np.full(nb, c.cand[0], I64)
    draws = np.zeros(nb, I64)
    active = np.arange(nb)
    cand = c.cand.astype(I64)
    left = MAX_DRAWS - 1 if plant == "bound_4095" else MAX_DRAWS
    # the draws of a sample in rank order, a block of them at a time (8 single draws, then 8, 16, ... 2048: 4096 in all): the first
    # draw of the block that is outside the history ends the sample, a block without one ends on its last draw and goes on
    for block in [1] * 8 + [8 << i for i in range(9)]:
        block = min(block, left)
        if not active.size or block <= 0:
            break
        with np.errstate(over="ignore"):
            states = s[active, None] + np.arange(1, block + 1, dtype=U64)[None, :] * G
            r = mix64(states) >> U64(32)
            idx = r % U64(nc) if plant == "modulo" else (r * U64(nc)) >> U64(32)
            s[active] += U64(block) * G
        it = cand[idx.astype(I64)]
        if plant == "no_rejection" or not hkeys.size:
            free = np.ones(it.shape, bool)
        else:
            key = c.users[active, None] * stride + it
            free = hkeys[np.minimum(np.searchsorted(hkeys, key), hkeys.size - 1)] != key
        has = free.any(axis=1)
        last = np.where(has, free.argmax(axis=1), block - 1)
        item[active] = it[np.arange(active.size), last]
        draws[active] += last + 1
        active = active[~has]
        left -= block
    exhausted = np.zeros(nb, bool)
    exhausted[active] = True
    return item, draws, exhausted


_SREF = {}


def sampler_reference(c):
    if c.seed not in _SREF:
        _SREF[c.seed] = sampler_ref(c)
    return _SREF[c.seed]


def check_sampler(c, got):
    ref, _, exhausted = sampler_reference(c)
    got = np.asarray(got)
    assert got.shape == ref.shape and got.dtype == I64, (c.axes(), got.shape, got.dtype)
    assert np.isin(got, c.cand).all(), (c.axes(), "an output is no candidate")
    free = ~exhausted
    key = c.users[free] * I64(2 ** 32) + got[free]
    hkeys = np.repeat(np.arange(8, dtype=I64), np.diff(c.rowptr)) * I64(2 ** 32) + c.col[:c.rowptr[-1]].astype(I64)
    assert not np.isin(key, hkeys).any(), (c.axes(), "an output lies in its user's history")
    bad = got != ref
    assert not bad.any(), (c.axes(), "ids differ", int(bad.sum()), "first at", int(np.argmax(bad)), int(got[np.argmax(bad)]), int(ref[np.argmax(bad)]))
    assert (exhausted == c.full_user[c.users]).all(), (c.axes(), "exhausted exactly where the history holds every candidate")


def streams_disjoint(seeding):
    """[(seed, counter, number of repeated states)] over SEEDS x (0, 1, 7): 4096 samples, 64 draws each"""
    out = []
    with np.errstate(over="ignore"):
        steps = np.arange(1, 65, dtype=U64) * G
        for seed in SEEDS:
            for counter in (0, 1, 7):
                s0 = np.broadcast_to(first_state(seed, counter, np.arange(4096), seeding), (4096,))
                states = (s0[:, None] + steps[None, :]).ravel()
                out.append((seed, counter, states.size - np.unique(states).size))
    return out


_CASES = {}


def draw_case(seed):
    if seed in _CASES:
        return _CASES[seed]
    rng = np.random.default_rng(9100 + seed)
    c = Case()
    c.seed = seed
    if seed < N_METRIC:
        _draw_metrics(c, seed, rng)
    else:
        _draw_sampler(c, seed - N_METRIC, rng)
    _CASES[seed] = c
    return c


METRIC_SEEDS = tuple(range(N_METRIC))
SAMPLER_SEEDS = tuple(range(N_METRIC, N_METRIC + N_SAMPLER))
WRAPPER_SEED, EVALUATOR_SEED = 3, 8                         # 257 users, k = 50 / k = 128: asserted below


# ------------------------------------------------------------------------------------------------ CPU self-tests
def test_cases_span_every_axis():
    seen = {k: set() for k in ("n_users", "k", "cuts", "pos", "rank", "combo", "hit_out", "batch", "n_cand", "pair", "spair", "seed",
                               "counter", "hist", "shuffled")}
    for seed in METRIC_SEEDS:
        c = draw_case(seed)
        assert c.kind == "metrics" and c.axes() == draw_case(seed).axes()
        seen["n_users"].add(c.n_users), seen["k"].add(c.k), seen["cuts"].add(c.cuts), seen["hit_out"].add(c.hit_out)
        seen["pair"].add((c.n_users, c.k))
        seen["pos"] |= set(c.pos_kind)
        seen["rank"] |= set(c.rank_kind)
        seen["combo"] |= set(zip(c.pos_kind, c.rank_kind))
        assert all((np.diff(t) > 0).all() for t in c.truth) and (c.topk >= -1).all() and c.topk.max() < c.n_items
        assert list(c.ks) == sorted(c.ks) and 1 <= c.ks[0] and c.ks[-1] <= c.k
        if c.n_users >= 255:                                # the clamps active and inactive side by side in ONE launch
            assert set(c.pos_kind) == set(M_POS) and set(c.rank_kind) == set(M_RANK)
            assert any(t.size and t[0] == 0 for t in c.truth) and (c.k == 1 or any(t.size and t[-1] == c.n_items - 1 for t in c.truth))
            hit = metrics_reference(c)[0]
            kinds = np.array(c.rank_kind)
            assert not hit[kinds == "none"].any() and (c.topk[kinds == "pad"][:, -1] == -1).all()
            assert (hit[kinds == "all"].sum(1) == np.minimum(c.pos_len, c.k)[kinds == "all"]).all()
            f, l = hit[(kinds == "first") & (c.pos_len > 0)], hit[(kinds == "last") & (c.pos_len > 0)]
            assert f[:, 0].all() and not f[:, 1:].any() and l[:, -1].all() and not l[:, :-1].any()
            if c.k >= 2:
                d = (kinds == "dup") & (c.pos_len > 0)
                assert (c.topk[d][:, 0] == c.topk[d][:, -1]).all() and hit[d][:, 0].all() and hit[d][:, -1].all()
    assert seen["n_users"] == set(M_USERS) and seen["k"] == set(M_K) and seen["cuts"] == set(M_CUTS) and seen["hit_out"] == {True, False}
    assert len(seen["pair"]) == 25 and seen["pos"] == set(M_POS) and seen["rank"] == set(M_RANK) and len(seen["combo"]) == 42
    assert any(len(set(draw_case(s).ks)) < len(draw_case(s).ks) for s in METRIC_SEEDS)           # a repeated cut-off
    assert any(draw_case(s).ks == (5, 10, 20, 50) for s in METRIC_SEEDS)
    for s, k in ((WRAPPER_SEED, 50), (EVALUATOR_SEED, 128)):
        assert draw_case(s).n_users == 257 and draw_case(s).k == k
    for seed in SAMPLER_SEEDS:
        c = draw_case(seed)
        assert c.kind == "sampler" and c.axes() == draw_case(seed).axes()
        seen["batch"].add(c.batch), seen["n_cand"].add(c.n_cand), seen["seed"].add(c.rng_seed), seen["counter"].add(c.counter)
        seen["spair"].add((c.batch, c.n_cand)), seen["shuffled"].add(c.shuffled)
        seen["hist"] |= set(c.hist_kind)
        assert np.unique(c.cand).size == c.n_cand and not np.array_equal(np.sort(c.cand), np.arange(c.n_cand))
        assert all((np.diff(h) > 0).all() for h in c.hists)
        if c.batch > 8:
            assert np.unique(c.users).size < c.batch and set(c.users.tolist()) == set(range(8))
        for u, kind in enumerate(c.hist_kind):
            inside = np.isin(c.cand, c.hists[u]).sum()
            assert {"empty": inside == 0 and c.hists[u].size == 0, "one": inside == 1, "noncand": inside == 0 and c.hists[u].size > 0,
                    "all_but_one": inside == c.n_cand - 1, "full": inside == c.n_cand, "mixed": c.n_cand < 4 or 0 < inside < c.n_cand}[kind]
        _, draws, exhausted = sampler_reference(c)
        abo = np.isin(c.users, [u for u, kind in enumerate(c.hist_kind) if kind == "all_but_one" and not c.full_user[u]])
        assert (draws[abo] < MAX_DRAWS).all() and not exhausted[abo].any()       # the free one is found long before the bound
        assert (draws[exhausted] == MAX_DRAWS).all() and (exhausted == c.full_user[c.users]).all()
    assert seen["batch"] == set(S_BATCH) and seen["n_cand"] == set(S_NCAND) and seen["seed"] == set(SEEDS)
    assert seen["counter"] == set(COUNTERS) and seen["hist"] == set(S_HIST) and seen["shuffled"] == {True, False}
    assert len(seen["spair"]) == 36
    reached = [s for s in SAMPLER_SEEDS if sampler_reference(draw_case(s))[2].any()]
    assert any(draw_case(s).n_cand >= 64 for s in reached) and any(draw_case(s).n_cand == 1 for s in reached)


def test_checker_rejects_planted_errors():
    caught = {pl: [] for pl in METRIC_PLANTS + SAMPLER_PLANTS}
    for seed in METRIC_SEEDS:
        c = draw_case(seed)
        hit, out = metrics_ref(c)
        check_metrics(c, hit.astype(np.uint8), out)         # the restatement passes its own checker
        check_metrics(c, None, out)
        if c.n_users > 257:
            continue
        for pl in METRIC_PLANTS:
            try:
                check_metrics(c, *metrics_ref(c, pl))
            except AssertionError:
                caught[pl].append(seed)
    for seed in SAMPLER_SEEDS:
        c = draw_case(seed)
        check_sampler(c, sampler_reference(c)[0])
        for pl in SAMPLER_PLANTS if c.batch <= 257 else ():
            if pl == "bound_4095" and not sampler_reference(c)[2].any():
                continue
            try:
                check_sampler(c, sampler_ref(c, pl)[0])
            except AssertionError:
                caught[pl].append(seed)
    print({pl: len(s) for pl, s in caught.items()})
    for pl, seeds in caught.items():
        if pl in EQUIVALENT_PLANTS:
            # min(j, pos_len - 1) = min(j, min(pos_len, k) - 1) and min(j + 1, pos_len) = min(j + 1, min(pos_len, k)) for j + 1 <= k
            assert not seeds, (pl, "is the same function for j < k, yet a case tells them apart", seeds)
        else:
            assert seeds, (pl, "passes every case")


def test_sample_streams_are_disjoint():
    """(a) no two of the 4096 x 64 generator states coincide, for every seed and counters 0, 1, 7"""
    res = streams_disjoint("mixed")
    print("mixed :", [(hex(s), c, r) for s, c, r in res if r] or "no repeated state in %d (seed, counter) pairs" % len(res))
    assert all(r == 0 for _, _, r in res), res


def test_parent_seeding_is_rejected():
    """the seeding `seed ^ (counter C + b G)` aligns neighbouring samples' streams at seeds 0, 1, 2 and 2^64 - 1"""
    res = streams_disjoint("parent")
    print("parent:", [(hex(s), c, r) for s, c, r in res if r])
    bad = {s for s, _, r in res if r}
    assert bad >= {0, 1, 2, 2 ** 64 - 1}, bad
    c = draw_case(N_METRIC + 4 * 6 + 4)                     # and the ids follow: sample b + 1's first draw is b's second
    assert c.n_cand == 1000 and c.batch == 257
    c0 = Case()
    c0.__dict__.update(c.__dict__)
    c0.rng_seed, c0.counter = 0, 0
    with np.errstate(over="ignore"):
        s = first_state(0, 0, np.arange(257), "parent")
        assert (s[1:] == s[:-1] + G).all()
    old, draws, _ = sampler_ref(c0, seeding="parent")
    c0.users = np.zeros(c.batch, I64)                       # user 0 has no history: every sample keeps its first draw ...
    first = sampler_ref(c0, plant="no_rejection", seeding="parent")[0]
    b = np.flatnonzero(np.arange(c.batch) + draws - 1 < c.batch)
    assert (draws[b] > 1).sum() > 20 and (old[b] == first[b + draws[b] - 1]).all()      # ... and draw t of sample b is sample b + t - 1's first
    assert not np.array_equal(old, sampler_ref(draw_case(N_METRIC + 4 * 6 + 4))[0])


def test_reference_sampler_is_uniform():
    """(b) 30 of 100 candidates in the history, 200,000 samples of one user: every allowed item within 6 sqrt(expected)"""
    c = Case()
    rng = np.random.default_rng(5)
    c.batch, c.n_cand, c.rng_seed, c.counter = 200_000, 100, 999, 7
    c.cand = (7 * rng.permutation(100) + 3).astype(I32)
    hist = np.sort(c.cand[:30])
    c.rowptr = np.array([0, 30] + [30] * 7, I32)
    c.col = hist.astype(I32)
    c.users = np.zeros(c.batch, I64)
    ids, draws, exhausted = sampler_ref(c)
    assert not exhausted.any() and not np.isin(ids, hist).any()
    allowed = c.cand[30:]
    counts = np.array([(ids == a).sum() for a in allowed])
    expect = c.batch / allowed.size
    print("counts %d .. %d, expected %.0f +- %.0f; mean draws %.3f (1 / 0.7 = 1.429)" % (counts.min(), counts.max(), expect,
                                                                                          6 * np.sqrt(expect), draws.mean()))
    assert counts.sum() == c.batch and np.abs(counts - expect).max() < 6 * np.sqrt(expect)
    assert abs(draws.mean() - 1 / 0.7) < 0.01


# ------------------------------------------------------------------------------------------------ GPU plumbing
def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def P(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _lib():
    from mmrec_amd import _lib as L, hip_ops
    return L.load(), hip_ops._stream()


class Guarded:
    """an output of `n` elements pre-filled with FILL inside one tensor with GUARD sentinel elements on either side"""

    def __init__(self, shape, dtype):
        self.shape, self.n, self.dt = tuple(shape), int(np.prod(shape)), np.dtype(dtype)
        host = np.full(self.n + 2 * GUARD, GUARD_VALUE[self.dt], self.dt)
        host[GUARD:GUARD + self.n] = FILL[self.dt]
        self.buf = _dev(host)
        self.view = self.buf[GUARD:GUARD + self.n]

    def get(self, name=""):
        b = self.buf.cpu().numpy()
        g = GUARD_VALUE[self.dt]
        assert (b[:GUARD] == g).all() and (b[GUARD + self.n:] == g).all(), (name, "guard elements overwritten")
        return b[GUARD:GUARD + self.n].reshape(self.shape).copy()

    def untouched(self, name=""):
        assert (self.get(name) == FILL[self.dt]).all(), (name, "written although nothing may be launched")


def run_metrics(c, ks=None, hit_out=None):
    lib, s = _lib()
    ks = c.ks if ks is None else ks
    want_hit = c.hit_out if hit_out is None else hit_out
    out = Guarded((c.n_users, 4, len(ks)), F64)
    hit = Guarded((c.n_users, c.k), np.uint8) if want_hit else None
    args = [_dev(x) for x in (c.topk, c.rowptr, np.concatenate([c.col, np.zeros(1, I32)]), c.discount, c.idcg, np.array(ks, I32))]
    rc = lib.mmrec_topk_metrics_f64(P(args[0]), c.n_users, c.k, P(args[1]), P(args[2]), P(args[3]), P(args[4]), P(args[5]), len(ks),
                                    P(hit.view) if hit else None, P(out.view), s)
    assert rc == 0, (c.axes(), rc)
    torch.cuda.synchronize()
    return (hit.get(c.axes()) if hit else None), out.get(c.axes())


def run_sampler(c):
    lib, s = _lib()
    out = Guarded((c.batch,), I64)
    args = [_dev(x) for x in (c.users if c.batch else np.zeros(1, I64), c.rowptr, c.col, c.cand)]
    rc = lib.mmrec_sample_negatives_i64(P(args[0]), c.batch, P(args[1]), P(args[2]), P(args[3]), c.n_cand, c.rng_seed, c.counter,
                                        P(out.view), s)
    assert rc == 0, (c.axes(), rc)
    torch.cuda.synchronize()
    return out.get(c.axes())


# ------------------------------------------------------------------------------------------------ device tests
@pytest.mark.gpu
@pytest.mark.parametrize("seed", METRIC_SEEDS)
def test_topk_metrics_bit_for_bit(seed):
    c = draw_case(seed)
    hit, out = run_metrics(c)
    assert (hit is None) == (not c.hit_out)
    check_metrics(c, hit, out)


@pytest.mark.gpu
def test_topk_metrics_hit_out_does_not_change_the_numbers():
    c = draw_case(7)
    assert c.n_users >= 255
    a, b = run_metrics(c, hit_out=True), run_metrics(c, hit_out=False)
    assert b[0] is None and same_doubles(a[1], b[1]).all()
    check_metrics(c, a[0], a[1])


@pytest.mark.gpu
def test_topk_metrics_wrapper_means():
    """hip_ops.topk_metrics_per_user on a case with empty rows: per-user bits, hence the reference's means (NaN where it has NaN)"""
    from mmrec_amd import _lib as L, hip_ops
    c = draw_case(WRAPPER_SEED)
    ks = sorted(set(c.ks))
    rp, col, topk = _dev(c.rowptr), _dev(np.concatenate([c.col, np.zeros(1, I32)])), _dev(c.topk)
    out, hits = hip_ops.topk_metrics_per_user(topk, rp, col, ks, want_hits=True)
    hit_ref, _ = metrics_reference(c)
    c2 = Case()
    c2.__dict__.update(c.__dict__)
    c2.ks, c2.seed = tuple(ks), -1
    _, out_ref = metrics_ref(c2)
    got = out.cpu().numpy()
    assert np.array_equal(hits.cpu().numpy().astype(bool), hit_ref) and same_doubles(got, out_ref).all()
    assert same_doubles(got.sum(0) / c.n_users, out_ref.sum(0) / c.n_users).all() and np.isnan(got.sum(0)[0]).all()
    some = c.pos_len > 0                                    # the means over the users that have ground truth: numbers
    assert same_doubles(got[some].mean(0), out_ref[some].mean(0)).all() and np.isfinite(got[some]).all()
    for bad in ([0], [c.k + 1], [1, c.k + 1], [-1, 5]):
        with pytest.raises(L.MMRecHipError):
            hip_ops.topk_metrics_per_user(topk, rp, col, bad)


@pytest.mark.gpu
def test_evaluator_on_device_gives_the_reference_means():
    """TopKEvaluator.evaluate_device on the users of a drawn case that have ground truth: the reference's means, rounded as it rounds"""
    from mmrec_amd.utils.topk_evaluator import TopKEvaluator
    c = draw_case(EVALUATOR_SEED)
    keep = np.flatnonzero(c.pos_len > 0)
    assert 200 < keep.size < c.n_users
    c2 = Case()
    c2.__dict__.update(c.__dict__)
    c2.seed, c2.n_users, c2.topk, c2.truth, c2.pos_len = -1, keep.size, c.topk[keep], [c.truth[u] for u in keep], c.pos_len[keep]
    c2.col = np.concatenate(c2.truth).astype(I32)
    c2.ks = (5, 10, 20, 50, 128)
    _, out_ref = metrics_ref(c2)
    means = out_ref.sum(0) / keep.size
    assert (np.abs(means * 1e4 - np.round(means * 1e4) - 0.5) > 1e-6).all() and (np.abs(means * 1e4 - np.round(means * 1e4) + 0.5) > 1e-6).all()

    class Data:
        def get_eval_items(self):
            return c2.truth

        def get_eval_len_list(self):
            return c2.pos_len

    ev = TopKEvaluator({"metrics": ["Recall", "NDCG", "Precision", "MAP"], "topk": list(c2.ks), "save_recommended_topk": False})
    half = keep.size // 2
    res = ev.evaluate_device([_dev(c2.topk[:half]), _dev(c2.topk[half:])], Data())
    for m, name in enumerate(("recall", "ndcg", "precision", "map")):
        for t, kk in enumerate(c2.ks):
            assert res["%s@%d" % (name, kk)] == round(means[m, t], 4), (name, kk, res["%s@%d" % (name, kk)], means[m, t])


@pytest.mark.gpu
def test_topk_metrics_argument_checks():
    lib, s = _lib()
    c = draw_case(0)
    out, hit = Guarded((4, 4, 1), F64), Guarded((4, c.k), np.uint8)
    a = [_dev(x) for x in (np.zeros((4, c.k), I64), np.zeros(5, I32), np.zeros(1, I32), c.discount, c.idcg, np.array([1], I32))]

    def call(n=4, k=c.k, n_ks=1, null=()):
        p = [None if i in null else P(x) for i, x in enumerate(a)]
        return lib.mmrec_topk_metrics_f64(p[0], n, k, p[1], p[2], p[3], p[4], p[5], n_ks, P(hit.view), None if 6 in null else P(out.view), s)
    assert call(n=-1) == BAD_ARG and call(k=0) == BAD_ARG and call(k=-3) == BAD_ARG and call(n_ks=0) == BAD_ARG and call(n_ks=-1) == BAD_ARG
    assert call(n=0, null=range(7)) == 0
    for i in range(7):
        assert call(null=(i,)) == BAD_ARG, i
    torch.cuda.synchronize()
    out.untouched("metrics argument checks"), hit.untouched("metrics argument checks")


@pytest.mark.gpu
@pytest.mark.parametrize("seed", SAMPLER_SEEDS)
def test_sample_negatives_id_for_id(seed):
    c = draw_case(seed)
    got = run_sampler(c)
    check_sampler(c, got)
    if c.batch in (257, 5000):                              # reproducible, and the counter matters
        assert np.array_equal(run_sampler(c), got)
        c2 = Case()
        c2.__dict__.update(c.__dict__)
        c2.counter = (c.counter + 1) & MASK64
        assert c.n_cand < 64 or not np.array_equal(run_sampler(c2), got)


@pytest.mark.gpu
def test_sample_negatives_wrapper():
    """hip_ops.sample_negatives masks seed and counter to 64 bits and hands them over whole"""
    from mmrec_amd import hip_ops
    c = draw_case(N_METRIC + 4 * 6 + 4)
    assert c.batch == 257 and c.n_cand == 1000
    got = hip_ops.sample_negatives(_dev(c.users), _dev(c.rowptr), _dev(c.col), _dev(c.cand), c.rng_seed - 2 ** 64, c.counter + 2 ** 64)
    check_sampler(c, got.cpu().numpy())


@pytest.mark.gpu
def test_sample_negatives_argument_checks():
    lib, s = _lib()
    c = draw_case(N_METRIC + 8)
    out = Guarded((max(c.batch, 4),), I64)
    a = [_dev(x) for x in (np.zeros(4, I64), c.rowptr, c.col, c.cand)]

    def call(batch=4, n_cand=c.n_cand, null=()):
        p = [None if i in null else P(x) for i, x in enumerate(a)]
        return lib.mmrec_sample_negatives_i64(p[0], batch, p[1], p[2], p[3], n_cand, 1, 2, None if 4 in null else P(out.view), s)
    assert call(batch=-1) == BAD_ARG and call(n_cand=0) == BAD_ARG and call(n_cand=-5) == BAD_ARG and call(batch=0, n_cand=0) == BAD_ARG
    assert call(batch=0, null=range(5)) == 0
    for i in range(5):
        assert call(null=(i,)) == BAD_ARG, i
    torch.cuda.synchronize()
    out.untouched("sampler argument checks")
