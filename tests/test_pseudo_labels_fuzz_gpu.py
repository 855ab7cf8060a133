"""GPU: seeded differential fuzz of the tri-modal softmax top-k (csrc/tri_topk.hip, mmrec_tri_topk_f32) and of
mmrec_list_exclude_i32 through the raw C ABI, over guarded, sentinel-filled outputs and a sentinel-filled workspace, against
float64 numpy of the formulas as written here (`scores64`) on the same fp32 tables, never against another kernel.

    c_m[r, j] = <T_m[ids[r]], T_m[j]>,   p_m = exp(c_m - lse_m[r]),   S_t[r, j] = sum_m W[t][m] p_m[r, j],   W >= 0
    list t of row r: the k columns with the largest S_t[r, .], descending, ties by the lower column

The kernel is given the lse the library's own mmrec_score_lse_f32 computes (as hip_ops.pseudo_labels gives it); the reference
uses the float64 lse.

THE TOLERANCE eps[r], relative, of ONE score (derived, not picked; u = 2^-24):
    the logit          |c - c64| <= gamma(d + 2) A,  A = |T_m[ids[r]]| |T_m[j]| <= the largest row norm squared (unit rows: 1): the
                       fma chain of d = 64 products on the fp32 MFMA;
    the lse            F_m[r]: the forward bound of the log-sum-exp's own fuzz (tests/test_score_lse_fuzz_gpu.py `forward_bound`,
                       evaluated for Q = T_m[ids], K = T_m, scale 1);
    c - lse rounded    u |c - lse| <= u (A + |lse|);
    -> the exponent is off by e_m[r] = gamma(d + 2) A + F_m[r] + u (A + |lse_m[r]|), p_m by that relatively (first order);
    expf               E_EXP u relative (the constant of tests/test_edge_softmax_fuzz_gpu.py);
    the mix            three products and two additions of non-negative terms: 5 u relative at most, no cancellation.
    eps[r] = max_m e_m[r] + (E_EXP + 5) u                          (about 1e-5 on these cases; printed per case)
Two scores being compared are each off by eps, so every comparison below allows 2 eps[r].

THE RULE, per (row, list), with K64 the k-th largest float64 score of the row:
    every column with S64 > K64 (1 + 2 eps) is in the list; every listed column has S64 >= K64 (1 - 2 eps);
    no duplicates, every entry in [0, N); consecutive entries descend: S64[a] >= S64[b] (1 - 2 eps);
    out_val is within eps S64 of S64 (+ one denormal);
    EXACT where float64 is not needed: bit-identical table rows (planted duplicates) score the same bits, so of two duplicates the
    lower column is listed first and the higher never without the lower; a zero row of W scores 0.0 everywhere: the list is
    0 .. k-1; a row whose id is outside [0, N) holds -1 (values -inf) in all three lists.
A (row, list) pair NEEDS LENIENCY when its list is not the float64 ranking itself; at most 5 % of all pairs of the whole fuzz may
(`LENIENT_CAP`; counted over the cases, asserted by the last test of the file; tests/test_pseudo_labels_cpu.py confirms without a
GPU that the fp32 torch composition stays within the cap on these seeds, and holds the checker honest with planted errors)."""
import os

import numpy as np
import pytest
import torch

from tests.test_edge_softmax_fuzz_gpu import E_EXP, GUARD, SENTINEL
from tests.test_spmm_fuzz_gpu import U, _on, gamma

BS = (1, 31, 32, 33, 127, 128, 129, 300)
NS_FIXED = (16, 32, 63, 64, 65, 97, 700, 3000)
KS = (1, 10, 16)
IDS = ("null", "given", "repeats", "out_of_range")
WS = ("damrs", "random", "zero_row")
TABLES = ("random", "clustered", "duplicates")
CASES = 40
LENIENT_CAP = 0.05
D = 64
BAD = 10001
_TALLY = {}                                    # case -> (pairs, lenient pairs), filled by the GPU fuzz


def _lib():
    from mmrec_amd import _lib as L
    if not os.path.exists(L.LIB_PATH):
        from mmrec_amd.build import build
        build(verbose=False)
    return L.load()


def split_cols(B, N):
    return int(_lib().mmrec_tri_topk_split_cols(int(B), int(N)))


def min_split_n(B):
    """the smallest N at which the library's plan for B rows walks the columns in at least two splits"""
    for N in range(1, 1 << 16):
        s = split_cols(B, N)
        if s and -(-N // s) >= 2:
            return N
    raise AssertionError("no split below 65536 columns")


class Case:
    pass


def _unit(x):
    return x / np.maximum(np.linalg.norm(x, axis=1, keepdims=True), 1e-12)


def case(k):
    c = Case()
    c.seed = k
    c.B = BS[k % 8]
    ns = NS_FIXED + (min_split_n(c.B),)
    c.N = ns[(k + k // 8 + 2 * (k // 9)) % 9]
    c.k = KS[(k + k // 3) % 3]
    c.ids_mode = IDS[(k + k // 4) % 4]
    c.w_mode = WS[(k // 2) % 3]
    c.tables = TABLES[(k + k // 6) % 3]
    c.with_val = (k // 3) % 2 == 0
    if c.ids_mode == "null" and c.B > c.N:     # rows 0 .. B-1 must exist
        c.ids_mode = "repeats"
    rng = np.random.default_rng(7000 + k)
    B, N = c.B, c.N
    T = []
    for m in range(3):
        if c.tables == "clustered":            # a few dozen tight clusters: many near neighbours per row
            centres = rng.standard_normal((max(2, N // 12), D))
            x = centres[rng.integers(0, centres.shape[0], N)] + 0.15 * rng.standard_normal((N, D))
        else:
            x = rng.standard_normal((N, D))
        T.append(np.ascontiguousarray(_unit(x), np.float32))
    c.dup = np.arange(N)                       # dup[j]: the lowest column whose rows are bit-identical to column j's in all tables
    if c.tables == "duplicates":
        for _ in range(max(1, N // 8)):
            a, b = sorted(rng.integers(0, N, 2).tolist())
            if a != b and c.dup[a] == a and (c.dup == b).sum() == 1:      # b: a row of its own that nobody copies
                for m in range(3):
                    T[m][b] = T[m][a]
                c.dup[b] = a
    c.T = T
    if c.ids_mode == "null":
        c.ids = None
        c.rows = np.arange(B, dtype=np.int64)
    else:
        c.rows = (rng.permutation(N)[:B] if B <= N and c.ids_mode != "repeats" else rng.integers(0, N, B)).astype(np.int64)
        if c.ids_mode == "repeats" and B > 1:
            c.rows[rng.integers(0, B)] = c.rows[0]
            c.rows[B - 1] = c.rows[0]
        if c.tables == "duplicates" and (c.dup != np.arange(N)).any():      # a query that IS a duplicated row: ties at the top
            c.rows[0] = int(np.flatnonzero(c.dup != np.arange(N))[0])
        if c.ids_mode == "out_of_range":
            c.rows[rng.integers(0, B)] = (N, -1, N + 12345, -(1 << 40))[k % 4]
        c.ids = c.rows
    c.valid = (c.rows >= 0) & (c.rows < N)
    if c.w_mode == "damrs":
        W = np.ones((3, 3)) + np.eye(3)
    else:
        W = rng.uniform(0.0, 3.0, (3, 3))
        W[rng.integers(0, 3), rng.integers(0, 3)] = 0.0
        if c.w_mode == "zero_row":
            W[k % 3] = 0.0
    c.W = np.ascontiguousarray(W, np.float32)
    return c


def name_of(c):
    return "case %d (B %d N %d k %d ids %s W %s tables %s val %d)" % (c.seed, c.B, c.N, c.k, c.ids_mode, c.w_mode, c.tables,
                                                                      c.with_val)


# ------------------------------------------------------------------------------------------------ host reference
def safe_rows(c):
    return np.where(c.valid, c.rows, 0)


def lse64(c):
    """[3, B] float64 log-sum-exp of the rows' cosines"""
    out = []
    for T in c.T:
        x = T[safe_rows(c)].astype(np.float64) @ T.astype(np.float64).T
        M = x.max(axis=1)
        out.append(M + np.log(np.exp(x - M[:, None]).sum(axis=1)))
    return np.stack(out)


def scores64(c):
    """S [3, B, N] float64; bit-identical columns get bit-identical scores (whatever the BLAS does at its edges)"""
    l64 = lse64(c)
    p = []
    for m, T in enumerate(c.T):
        x = T[safe_rows(c)].astype(np.float64) @ T.astype(np.float64).T
        p.append(np.exp(x - l64[m][:, None]))
    W = c.W.astype(np.float64)
    S = np.stack([(W[t, 0] * p[0] + W[t, 1] * p[1]) + W[t, 2] * p[2] for t in range(3)])
    return S[:, :, c.dup]


def ranking64(S, k):
    """the float64 lists: score descending, ties by the lower column"""
    return np.argsort(-S, axis=-1, kind="stable")[..., :k]


def eps_rows(c):
    """eps[r] of the module docstring"""
    from tests.test_score_lse_fuzz_gpu import forward_bound
    A = max(float(np.linalg.norm(T.astype(np.float64), axis=1).max()) for T in c.T) ** 2
    l64 = lse64(c)
    e = np.zeros(c.B)
    for m, T in enumerate(c.T):
        q = Case()
        q.Q, q.K, q.B, q.N, q.d, q.scale = np.ascontiguousarray(T[safe_rows(c)]), T, c.B, c.N, D, 1.0
        F = forward_bound(q)[1]
        e = np.maximum(e, gamma(D + 2) * A + F + U * (A + np.abs(l64[m])))
    return e + (E_EXP + 5) * U


def check(c, idx, val=None, S=None, eps=None, name=""):
    """the rule of the module docstring for idx [3, B, k] (and val) -> the number of (row, list) pairs that needed leniency"""
    idx = np.asarray(idx).astype(np.int64)
    k, B, N = c.k, c.B, c.N
    assert idx.shape == (3, B, k), (name, idx.shape)
    S = scores64(c) if S is None else S
    eps = eps_rows(c) if eps is None else eps
    if val is not None:
        val = np.asarray(val, np.float64)
        assert val.shape == (3, B, k), (name, val.shape)
    want = ranking64(S, k)
    has_dup = bool((c.dup != np.arange(N)).any())
    lenient = 0
    for r in range(B):
        if not c.valid[r]:
            assert (idx[:, r] == -1).all(), (name, "row %d has no usable id: -1 expected" % r, idx[:, r].tolist())
            if val is not None:
                assert np.isneginf(val[:, r]).all(), (name, "row %d: -inf expected" % r)
            continue
        e2 = 2.0 * eps[r]
        for t in range(3):
            got, s = idx[t, r], S[t, r]
            tag = (name, "row %d list %d" % (r, t))
            assert ((got >= 0) & (got < N)).all(), tag + ("an entry outside [0, N)", got.tolist())
            assert len(set(got.tolist())) == k, tag + ("a duplicate entry", got.tolist())
            if not c.W[t].any():
                assert np.array_equal(got, np.arange(k)), tag + ("all scores are 0.0: the lowest columns, in order", got.tolist())
                continue
            kth = s[want[t, r, k - 1]]
            must = np.flatnonzero(s > kth * (1.0 + e2))
            missing = np.setdiff1d(must, got)
            assert missing.size == 0, tag + ("a column well above the k-th score is missing", missing[:4].tolist(),
                                             s[missing[:4]].tolist(), float(kth))
            low = got[s[got] < kth * (1.0 - e2)]
            assert low.size == 0, tag + ("a listed column is well below the k-th score", low[:4].tolist(), s[low[:4]].tolist(),
                                         float(kth))
            sg = s[got]
            asc = np.flatnonzero(sg[:-1] < sg[1:] * (1.0 - e2))
            assert asc.size == 0, tag + ("not in descending order", got.tolist())
            pos = {int(j): i for i, j in enumerate(got.tolist())}
            for j, i in pos.items() if has_dup else ():      # bit-identical rows: the lower column first, never the higher alone
                for o in np.flatnonzero(c.dup == c.dup[j]).tolist():
                    if o < j:
                        assert o in pos and pos[o] < i, tag + ("exact tie in the wrong order", o, j, got.tolist())
            if val is not None:
                bad = np.abs(val[t, r] - sg) > eps[r] * sg + 2.0 ** -149
                assert not bad.any(), tag + ("a value beyond the bound", val[t, r][bad][:3].tolist(), sg[bad][:3].tolist(),
                                             float(eps[r]))
            lenient += int(not np.array_equal(got, want[t, r]))
    return lenient


def torch_composition(c, lse=None):
    """the fp32 materialised fallback (hip_ops.tri_softmax_topk_torch) on the case, on the CPU, with the float64 lse rounded to
    fp32 unless one is given -> (idx, val) numpy"""
    from mmrec_amd import hip_ops
    lse = torch.from_numpy(lse64(c).astype(np.float32)) if lse is None else lse
    ids = None if c.ids is None else torch.from_numpy(c.ids)
    idx, val = hip_ops.tri_softmax_topk_torch([torch.from_numpy(T) for T in c.T], ids, lse, torch.from_numpy(c.W), c.k, True)
    return idx.numpy(), val.numpy()


# ------------------------------------------------------------------------------------------------ no GPU: the axes
def test_cases_span_every_axis():
    cs = [case(k) for k in range(CASES)]
    assert {c.B for c in cs} == set(BS)
    assert {c.N for c in cs} >= set(NS_FIXED)
    for B in BS:                                # the plan's first split point is on the axis of every B
        n2 = min_split_n(B)
        assert any(c.N == n2 for c in cs if c.B == B) or n2 in NS_FIXED, (B, n2)
        assert split_cols(B, n2) % 64 == 0 and split_cols(B, n2 - 1) >= n2 - 1
    assert any(c.N == min_split_n(c.B) for c in cs)
    assert any(-(-c.N // split_cols(c.B, c.N)) >= 2 and split_cols(c.B, c.N) > 64 for c in cs)      # splits of several tiles
    assert {c.k for c in cs} == set(KS) and {c.ids_mode for c in cs} == set(IDS) and {c.w_mode for c in cs} == set(WS)
    assert {c.tables for c in cs} == set(TABLES) and {c.with_val for c in cs} == {True, False}
    assert all(c.N >= c.k for c in cs) and any(c.N == c.k for c in cs)
    assert any(c.ids_mode == "repeats" and len(set(c.rows.tolist())) < c.B for c in cs)
    assert all((~c.valid).sum() == (c.ids_mode == "out_of_range") for c in cs)
    assert any(c.tables == "duplicates" and (c.dup != np.arange(c.N)).sum() >= 4 for c in cs)
    assert any(c.B > 128 and c.N >= 700 for c in cs)                                               # several row tiles x splits
    for c in cs:
        for T in c.T:
            assert float(np.abs(np.linalg.norm(T.astype(np.float64), axis=1) - 1.0).max()) < 1e-6


def test_eps_is_what_the_docstring_derives():
    """about 1e-5 on every case: the derivation, not a constant, and far from both 0 and the scores' spread"""
    worst = 0.0
    for k in range(0, CASES, 3):
        c = case(k)
        e = eps_rows(c)
        assert e.shape == (c.B,) and float(e.min()) >= (D + 2 + E_EXP + 5) * U
        worst = max(worst, float(e.max()))
    print("largest eps over the sampled cases: %.3e" % worst)
    assert worst <= 4e-5


# ------------------------------------------------------------------------------------------------ GPU: the raw C ABI, guarded
def _guarded(n, dtype):
    buf = torch.full((n + 2 * GUARD,), SENTINEL, dtype=torch.int32, device="cuda:0")
    return buf, buf[GUARD:GUARD + n].view(dtype)


def _guards_ok(buf, n, name):
    b = buf.cpu().numpy()
    assert (b[:GUARD] == SENTINEL).all() and (b[GUARD + n:] == SENTINEL).all(), (name, "wrote outside the output")
    assert not (b[GUARD:GUARD + n] == SENTINEL).any(), (name, "entries never written", int((b[GUARD:GUARD + n] == SENTINEL).sum()))


def device_lse(c, T):
    """[3, B] fp32 from the library's own log-sum-exp kernel, as hip_ops.pseudo_labels computes it"""
    from mmrec_amd import hip_ops
    rows = _on(safe_rows(c))
    return torch.stack([hip_ops.score_lse(t[rows].contiguous(), t, 1.0) for t in T]).contiguous()


def raw_tri(c, T, ids, lse, W, name="tri", with_val=None):
    from mmrec_amd import hip_ops
    p, lib = hip_ops._p, _lib()
    n = 3 * c.B * c.k
    with_val = c.with_val if with_val is None else with_val
    bi, idx = _guarded(n, torch.int32)
    bv, val = _guarded(n, torch.float32) if with_val else (None, None)
    nbytes = int(lib.mmrec_tri_topk_workspace_bytes(c.B, c.N, c.k))
    ws = torch.full((nbytes // 4 + 4,), SENTINEL, dtype=torch.int32, device="cuda:0")
    rc = lib.mmrec_tri_topk_f32(p(T[0]), p(T[1]), p(T[2]), c.N, p(ids), c.B, p(lse), p(W), c.k, p(idx), p(val), p(ws),
                                hip_ops._stream())
    assert rc == 0, (name, rc)
    torch.cuda.synchronize()
    _guards_ok(bi, n, name + " idx")
    if with_val:
        _guards_ok(bv, n, name + " val")
    assert (ws[nbytes // 4:] == SENTINEL).all(), (name, "wrote past the workspace")
    return idx.clone().view(3, c.B, c.k), (val.clone().view(3, c.B, c.k) if with_val else None)


def _device_case(c):
    T = [_on(t) for t in c.T]
    ids = None if c.ids is None else _on(c.ids)
    return T, ids, device_lse(c, T), _on(c.W)


@pytest.mark.gpu
@pytest.mark.parametrize("k", range(CASES))
def test_tri_topk_fuzz(k):
    c = case(k)
    name = name_of(c)
    T, ids, lse, W = _device_case(c)
    idx, val = raw_tri(c, T, ids, lse, W, name)
    eps = eps_rows(c)
    lenient = check(c, idx.cpu().numpy(), None if val is None else val.cpu().numpy(), eps=eps, name=name)
    pairs = 3 * int(c.valid.sum())
    _TALLY[k] = (pairs, lenient)
    print("%s: eps max %.3e, %d of %d pairs needed leniency" % (name, float(eps.max()), lenient, pairs))
    idx2, val2 = raw_tri(c, T, ids, lse, W, name)                      # the same call again: the same bits
    assert torch.equal(idx, idx2), name
    if val is not None:
        assert torch.equal(val.view(torch.int32), val2.view(torch.int32)), name


@pytest.mark.gpu
def test_leniency_stays_within_the_cap():
    """over the whole fuzz at most 5 % of the (row, list) pairs differ from the float64 ranking (cases this process has not run
    are run here, once)"""
    for k in range(CASES):
        if k not in _TALLY:
            c = case(k)
            T, ids, lse, W = _device_case(c)
            idx, _ = raw_tri(c, T, ids, lse, W, name_of(c), with_val=False)
            _TALLY[k] = (3 * int(c.valid.sum()), check(c, idx.cpu().numpy(), name=name_of(c)))
    pairs, lenient = (sum(v[i] for v in _TALLY.values()) for i in (0, 1))
    print("leniency: %d of %d pairs (%.3f %%)" % (lenient, pairs, 100.0 * lenient / pairs))
    assert lenient <= LENIENT_CAP * pairs, (lenient, pairs)


@pytest.mark.gpu
def test_a_captured_call_replays_the_same_lists():
    from mmrec_amd import hip_ops
    c = case(13)
    c.B, c.N = 129, 700
    c = _resized(c)
    T, ids, lse, W = _device_case(c)
    eager, _ = raw_tri(c, T, ids, lse, W, "eager", with_val=False)
    p, lib = hip_ops._p, _lib()
    idx = torch.full((3, c.B, c.k), -7, dtype=torch.int32, device="cuda:0")
    ws = torch.zeros(int(lib.mmrec_tri_topk_workspace_bytes(c.B, c.N, c.k)) // 4 + 4, dtype=torch.int32, device="cuda:0")
    ids_d = _on(c.rows)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        rc = lib.mmrec_tri_topk_f32(p(T[0]), p(T[1]), p(T[2]), c.N, p(ids_d), c.B, p(lse), p(W), c.k, p(idx), None, p(ws),
                                    hip_ops._stream())
    assert rc == 0
    idx.fill_(-7)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(idx, eager)


def _resized(c):
    """case 13's recipe at B = 129, N = 700 with given ids: several row tiles x several splits"""
    rng = np.random.default_rng(99)
    c.T = [np.ascontiguousarray(_unit(rng.standard_normal((c.N, D))), np.float32) for _ in range(3)]
    c.dup = np.arange(c.N)
    c.rows = rng.permutation(c.N)[:c.B].astype(np.int64)
    c.ids, c.ids_mode, c.valid = c.rows, "given", np.ones(c.B, bool)
    return c


@pytest.mark.gpu
def test_argument_errors_and_the_empty_batch():
    from mmrec_amd import hip_ops
    c = case(1)
    T, ids, lse, W = _device_case(c)
    p, lib = hip_ops._p, _lib()
    out = torch.full((3 * c.B * 16 + 8,), -7, dtype=torch.int32, device="cuda:0")
    ws = torch.zeros(1 << 16, dtype=torch.int32, device="cuda:0")

    def call(t0=T[0], t1=T[1], t2=T[2], N=c.N, B=c.B, l=lse, k=c.k):
        return lib.mmrec_tri_topk_f32(p(t0), p(t1), p(t2), N, p(ids), B, p(l), p(W), k, p(out), None, p(ws), hip_ops._stream())
    assert call(k=0) == BAD and call(k=17) == BAD and call(k=-1) == BAD
    assert call(N=c.k - 1) == BAD                                      # fewer columns than k
    assert call(t0=None) == BAD and call(t1=None) == BAD and call(t2=None) == BAD and call(l=None) == BAD
    assert call(B=-1) == BAD
    assert call(B=0) == 0                                              # nothing to do, nothing touched
    torch.cuda.synchronize()
    assert bool((out == -7).all())


@pytest.mark.gpu
@pytest.mark.parametrize("R,kc,ke,k", [(1, 20, 10, 10), (257, 20, 10, 10), (33, 7, 3, 4), (64, 5, 0, 5), (300, 32, 16, 16), (5, 9, 4, 1)])
def test_list_exclude_against_a_python_loop(R, kc, ke, k):
    from mmrec_amd import hip_ops
    p, lib = hip_ops._p, _lib()
    rng = np.random.default_rng(R + kc)
    cand = np.stack([rng.permutation(kc + 6)[:kc] for _ in range(R)]).astype(np.int32)
    excl = np.stack([rng.permutation(kc + 6)[:ke] for _ in range(R)]).astype(np.int32).reshape(R, ke)
    want = np.array([[x for x in cand[r].tolist() if x not in set(excl[r].tolist())][:k] for r in range(R)], np.int32)
    buf, out = _guarded(R * k, torch.int32)
    dc, de = _on(cand), (_on(excl) if ke else None)
    assert lib.mmrec_list_exclude_i32(p(dc), p(de), R, kc, ke, k, p(out), hip_ops._stream()) == 0
    torch.cuda.synchronize()
    _guards_ok(buf, R * k, "list_exclude")
    assert np.array_equal(out.view(R, k).cpu().numpy(), want)
    assert np.array_equal(hip_ops.list_exclude(dc, _on(excl), k).cpu().numpy(), want) if ke else True
    assert lib.mmrec_list_exclude_i32(p(dc), p(de), R, kc, ke, kc - ke + 1, p(out), hip_ops._stream()) == BAD    # kc - ke < k
    assert lib.mmrec_list_exclude_i32(p(dc), p(de), R, kc, ke, 0, p(out), hip_ops._stream()) == BAD
    assert lib.mmrec_list_exclude_i32(None, None, 0, kc, ke, k, None, hip_ops._stream()) == 0
