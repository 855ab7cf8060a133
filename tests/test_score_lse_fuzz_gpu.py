"""GPU: seeded differential fuzz of the contrastive log-sum-exp (csrc/score_lse.hip, mmrec_score_lse_f32 / _bwd_f32,
hip_ops.score_lse) against float64 numpy of the formulas as written here (`lse64`, `bwd64`), never against another kernel.  The
raw C ABI is called over guarded, sentinel-filled outputs and a sentinel-filled workspace.

    lse[i] = log sum_j exp(x_ij),  x = scale s,  s_ij = <Q[i], K[j]>;   p_ij = exp(x_ij - lse[i])
    dQ[i]  = scale g[i] sum_j p_ij K[j];   dK[j] = scale sum_i g[i] p_ij Q[i]

The kernel's plan (read from the library: `split_len`).  A score is an fma chain over k = 0 .. d-1 on the fp32 MFMA, then one
product with `scale`.  Forward: a lane walks the 32-column sub-tiles of its column split and keeps, for the 16 columns of a
sub-tile it holds (those with bit 2 of j % 32 equal to its half h), a running maximum m and a sum l of exp(x - m), rescaled by
exp(m_old - m_new) when the maximum rises (exp(0) = 1: no rounding while it stands); the two halves of a row are combined, then
the splits, each with one more rescale; lse = M + log L.  Backward: w = exp(x - lse) * (scale g) per pair, the products W K and
W^T Q as fma chains over the walked operand in order within a split, the splits added in order.

Two acceptance modes; each case uses one.
  exact  entries are multiples of 1/8 of magnitude <= 4, scale a power of two >= 16, g multiples of 1/8: every dot is exact.  A few
         TARGET columns (first, last, around the sub-tile, tile and split boundaries) hold 4 in a dimension of their own, every
         row of Q holds 4 in the dimension of its target j*(i), everything else is -1/8, 0 or 1/8: s(i, j*) >= 15 and every other
         score <= 1, so the maximal logit stands >= 14 scale >= 224 above the rest, exp of the difference is 0 in fp32 and
         lse[i] must EQUAL scale s(i, j*),  dQ[i] must EQUAL scale g[i] K[j*],  dK[j] must EQUAL scale sum_{i: j*(i) = j} g[i] Q[i]
         (multiples of 1/4 below 2^18: exact in any order).  A lost or doubled column, a wrong row or a wrong split cannot hide.
  float  normal inputs: rows normalised with scale 2, 5 or 10, or unnormalised with |scale s| up to a few hundred (finite only
         with the running maximum).  With u = 2^-24, A_ij = sum_k |Q_ik K_jk|, M_i = max_j x_ij:
           delta_ij = |scale| gamma(d) A_ij + u |x_ij|                         the logit: the chain and the product with scale
           rel_ij   = 2 u (M_i - x_ij + 2 max_j delta_ij) + (R_i + 1) (E_EXP + 1) u + gamma(n_fwd)
                      the roundings of x - m and of the m_old - m_new of every rescale (they telescope to at most M_i - x_ij
                      each), R_i rescales with the error of the device's exp (E_EXP u, tests/test_edge_softmax_fuzz_gpu.py) and
                      one product each, one more exp for the term itself, and the additions a term meets: 16 per sub-tile of
                      its split, the other half, the splits: n_fwd = 16 * (split_len / 32) + 1 + n_splits.
                      R_i = 2 + the largest number, over splits and halves, of sub-tiles whose maximum comes within
                      2 max_j delta_ij of the running maximum before it (counted on the float64 scores).
           |lse - ref|_i <= F_i = sum_j p_ij (delta_ij + rel_ij) + E_LOG u max(|log L_i|, 1) + u |lse_i| + 2 u
                      first order through log-sum-exp, the device's log (E_LOG: 4 x the worst error of fp32 log against float64
                      MEASURED ON THE CPU over these cases' own arguments L_i, `test_E_LOG_covers_these_cases`), the final
                      addition, two to spare.
         Gradients (the kernel is given ITS OWN lse, as the op gives it): p carries the logit's and the forward's error,
           relp_ij = delta_ij + F_i + u (|log p_ij| + E_EXP + 2)               x - lse rounded, exp, scale g and the product
           |dQ - ref|_ic <= |scale g_i| sum_j p_ij |K_jc| (relp_ij + gamma(n_q)) + n_q 2^-149,   n_q = split_len_1 + n_splits_1
           |dK - ref|_jc <= |scale| sum_i |g_i| p_ij |Q_ic| (relp_ij + gamma(n_k)) + n_k 2^-149,  n_k = split_len_2 + n_splits_2
`test_E_LOG_covers_these_cases`, `test_E_EXP_covers_these_cases` and `test_cases_span_every_axis` need no GPU; the checker's own
tests (an fp32 emulation of the plan passes, planted errors do not) are in tests/test_score_lse_cpu.py."""
import os

import numpy as np
import pytest
import torch

from tests.test_edge_softmax_fuzz_gpu import E_EXP, GUARD, SENTINEL
from tests.test_spmm_fuzz_gpu import U, _on, gamma

E_LOG = 5.0                                    # test_E_LOG_covers_these_cases: 4 x the measured 1.05, rounded up
BS = (0, 1, 31, 32, 33, 64, 65, 257)
NS_FIXED = (0, 1, 31, 32, 33, 63, 64, 65, 4097)
KINDS = ("exact", "norm2", "norm5", "norm10", "raw")
CASES = 40


def _lib():
    from mmrec_amd import _lib as L
    if not os.path.exists(L.LIB_PATH):
        from mmrec_amd.build import build
        build(verbose=False)
    return L.load()


def split_len(B, N, mode=0):
    """rows of the walked operand per split, from the library (mode 0 forward, 1 dQ sweep, 2 dK sweep)"""
    return int(_lib().mmrec_score_lse_split_cols(int(B), int(N), int(mode)))


def axis_N():
    s = split_len(257, 4097)                   # the one axis value whose splits hold more than one tile
    return NS_FIXED + (s - 1, s, s + 1)


class Case:
    pass


def case(k):
    ns = axis_N()
    c = Case()
    c.seed, c.B, c.N = k, BS[k % 8], ns[(5 * k + k // 8) % len(ns)]
    c.d = 64 if (k // 4) % 2 == 0 else 128
    c.kind = KINDS[(k + k // 5) % 5]
    if k in (7, 15):                           # the large table in both modes and both widths, on more than two row tiles
        c.B, c.N, c.kind = 257, 4097, ("exact", "raw")[k == 15]
    c.exact = c.kind == "exact"
    rng = np.random.default_rng(1000 + k)
    B, N, d = c.B, c.N, c.d
    if c.exact:
        c.scale = float(rng.choice([16.0, 32.0, 64.0]))
        s0 = split_len(B, N) if N else 0
        want = [0, N - 1, 31, 32, 33, 63, 64, s0 - 1, s0, s0 + 1, N - 2, 95, 96, N // 2]
        c.targets = sorted({t for t in want if 0 <= t < N})[:16]
        Q = rng.integers(-1, 2, (B, d)) / 8.0
        K = rng.integers(-1, 2, (N, d)) / 8.0
        nt = len(c.targets)
        Q[:, :nt] = 0.0
        K[:, :nt] = 0.0
        c.jstar = np.zeros(B, np.int64)
        if nt:
            pick = (np.arange(B) + rng.integers(0, nt)) % nt if B else np.zeros(0, np.int64)
            pick[rng.random(B) < 0.3] = rng.integers(0, nt)       # some targets shared by many rows
            c.jstar = np.asarray(c.targets, np.int64)[pick]
            for t, j in enumerate(c.targets):
                K[j, t] = 4.0
            Q[np.arange(B), pick] = 4.0
        c.g = (rng.integers(-16, 17, B) / 8.0).astype(np.float32)
    else:
        Q = rng.standard_normal((B, d))
        K = rng.standard_normal((N, d))
        if c.kind == "raw":                    # |scale s| up to a few hundred, rows shifted so that the maxima differ widely
            c.scale = float(rng.choice([1.0, 4.0, -2.0]))
            Q *= rng.uniform(0.5, 3.0, (B, 1))
            K *= rng.uniform(0.2, 2.5, (N, 1))
        else:
            c.scale = float(c.kind[4:])
            Q /= np.maximum(np.linalg.norm(Q, axis=1, keepdims=True), 1e-12)
            K /= np.maximum(np.linalg.norm(K, axis=1, keepdims=True), 1e-12)
        c.g = rng.standard_normal(B).astype(np.float32)
    c.Q, c.K = np.ascontiguousarray(Q, np.float32), np.ascontiguousarray(K, np.float32)
    return c


def float_cases():
    return [c for c in map(case, range(CASES)) if not c.exact]


# ------------------------------------------------------------------------------------------------ host references
def scores64(c):
    return np.float64(np.float32(c.scale)) * (c.Q.astype(np.float64) @ c.K.astype(np.float64).T)


def lse64(c, x=None):
    """-> (lse [B], M [B], L [B]) in float64; an empty table gives -inf"""
    x = scores64(c) if x is None else x
    if c.N == 0:
        return np.full(c.B, -np.inf), np.full(c.B, -np.inf), np.zeros(c.B)
    M = x.max(axis=1)
    L = np.exp(x - M[:, None]).sum(axis=1)
    return M + np.log(L), M, L


def bwd64(c, g=None):
    """-> (dQ, dK, p) in float64 from the float64 lse"""
    g = np.asarray(c.g if g is None else g, np.float64)
    s = np.float64(np.float32(c.scale))
    if c.N == 0 or c.B == 0:
        return np.zeros((c.B, c.d)), np.zeros((c.N, c.d)), np.zeros((c.B, c.N))
    x = scores64(c)
    p = np.exp(x - lse64(c, x)[0][:, None])
    return s * g[:, None] * (p @ c.K.astype(np.float64)), s * ((p * g[:, None]).T @ c.Q.astype(np.float64)), p


def _logit_delta(c, x):
    A = np.abs(c.Q.astype(np.float64)) @ np.abs(c.K.astype(np.float64)).T
    return abs(float(np.float32(c.scale))) * gamma(c.d) * A + U * np.abs(x)


def _rescales(c, x, slack):
    """R_i of the module docstring: 2 + the most sub-tile steps, over splits and halves, at which the running maximum may rise"""
    s0 = split_len(c.B, c.N)
    j = np.arange(c.N)
    worst = np.zeros(c.B, np.int64)
    for lo in range(0, c.N, s0):
        for h in (0, 1):
            run, cnt = np.full(c.B, -np.inf), np.zeros(c.B, np.int64)
            for t0 in range(lo, min(lo + s0, c.N), 32):
                cols = j[t0:t0 + 32]
                cols = cols[((cols % 32) >> 2) & 1 == h]
                if not cols.size:
                    continue
                tm = x[:, cols].max(axis=1)
                cnt += tm >= run - slack
                run = np.maximum(run, tm)
            worst = np.maximum(worst, cnt)
    return worst + 2


def forward_bound(c):
    """-> (ref lse, F) of the module docstring"""
    x = scores64(c)
    ref, M, L = lse64(c, x)
    if c.N == 0 or c.B == 0:
        return ref, np.zeros(c.B)
    delta = _logit_delta(c, x)
    dmax = delta.max(axis=1)
    s0 = split_len(c.B, c.N)
    n_fwd = 16 * (s0 // 32) + 1 + -(-c.N // s0)
    R = _rescales(c, x, 2 * dmax)
    rel = 2 * U * (M[:, None] - x + 2 * dmax[:, None]) + ((R + 1) * (E_EXP + 1) * U + gamma(n_fwd))[:, None]
    p = np.exp(x - ref[:, None])
    F = (p * (delta + rel)).sum(axis=1) + E_LOG * U * np.maximum(np.abs(np.log(L)), 1.0) + U * np.abs(ref) + 2 * U
    return ref, F


def backward_bounds(c):
    """-> (dQ ref, dQ bound, dK ref, dK bound) of the module docstring"""
    dq, dk, p = bwd64(c)
    if c.N == 0 or c.B == 0:
        return dq, np.zeros_like(dq), dk, np.zeros_like(dk)
    x = scores64(c)
    F = forward_bound(c)[1]
    with np.errstate(divide="ignore"):
        logp = np.where(p > 0, -np.log(np.maximum(p, 1e-300)), 0.0)
    relp = _logit_delta(c, x) + F[:, None] + U * (logp + E_EXP + 2)
    s1, s2 = split_len(c.B, c.N, 1), split_len(c.B, c.N, 2)
    n_q, n_k = s1 + -(-c.N // s1), s2 + -(-c.B // s2)
    s = abs(float(np.float32(c.scale)))
    g = np.abs(c.g.astype(np.float64))
    bq = s * g[:, None] * ((p * (relp + gamma(n_q))) @ np.abs(c.K.astype(np.float64))) + n_q * 2.0 ** -149
    bk = s * ((p * g[:, None] * (relp + gamma(n_k))).T @ np.abs(c.Q.astype(np.float64))) + n_k * 2.0 ** -149
    return dq, bq, dk, bk


def exact_expect(c):
    """-> (lse, dQ, dK) the exact mode's outputs must EQUAL (float64 of exactly representable numbers)"""
    s = float(c.scale)
    Q, K, g = c.Q.astype(np.float64), c.K.astype(np.float64), c.g.astype(np.float64)
    if c.N == 0:
        return np.full(c.B, -np.inf), np.zeros((c.B, c.d)), np.zeros((0, c.d))
    lse = s * (Q * K[c.jstar]).sum(axis=1)
    dK = np.zeros((c.N, c.d))
    np.add.at(dK, c.jstar, s * g[:, None] * Q)
    return lse, s * g[:, None] * K[c.jstar], dK


def _arr(got):
    return got.detach().cpu().double().numpy() if isinstance(got, torch.Tensor) else np.asarray(got, np.float64)


def _compare(got, ref, bound, exact, name):
    g = _arr(got)
    assert g.shape == ref.shape, (name, g.shape, ref.shape)
    if exact:
        bad = g != ref
        assert not bad.any(), (name, "exact mismatch", int(bad.sum()), "first at", np.argwhere(bad)[0].tolist(),
                               float(g[bad][0]), float(ref[bad][0]))
        return 0.0
    if not g.size:
        return 0.0
    assert np.isfinite(ref).all() and np.isfinite(g).all(), (name, "not finite", int((~np.isfinite(g)).sum()))
    err = np.abs(g - ref)
    viol = err > bound
    assert not viol.any(), (name, "beyond the bound", int(viol.sum()), "first at", np.argwhere(viol)[0].tolist(),
                            float(g[viol][0]), float(ref[viol][0]), float(bound[viol][0]))
    return float((err / bound).max(initial=0.0))


def check_fwd(got, c, name=""):
    """lse [B] against float64 in the case's mode; returns the float mode's worst err / bound"""
    if c.exact:
        return _compare(got, exact_expect(c)[0], None, True, name + " lse")
    if c.N == 0:
        g = _arr(got)
        assert g.shape == (c.B,) and np.all(np.isneginf(g)), (name, "an empty table gives -inf")
        return 0.0
    ref, F = forward_bound(c)
    return _compare(got, ref, F, False, name + " lse")


def check_bwd(dq, dk, c, name=""):
    if c.exact:
        _, eq, ek = exact_expect(c)
        return max(_compare(dq, eq, None, True, name + " dQ"), _compare(dk, ek, None, True, name + " dK"))
    rq, bq, rk, bk = backward_bounds(c)
    if c.N == 0 or c.B == 0:
        return max(_compare(dq, rq, None, True, name + " dQ"), _compare(dk, rk, None, True, name + " dK"))
    return max(_compare(dq, rq, bq, False, name + " dQ"), _compare(dk, rk, bk, False, name + " dK"))


# ------------------------------------------------------------------------------------------------ no GPU: the constants, the axes
def _log_args():
    for c in float_cases():
        if c.B and c.N:
            yield lse64(c)[2]


def test_E_LOG_covers_these_cases():
    """worst error of fp32 log (numpy, on the CPU) against float64 in units of u max(|log L|, 1) over the L_i of every float case"""
    worst = 0.0
    for L in _log_args():
        L32 = L.astype(np.float32)
        a, b = np.log(L32).astype(np.float64), np.log(L32.astype(np.float64))
        worst = max(worst, float((np.abs(a - b) / (U * np.maximum(np.abs(b), 1.0))).max(initial=0.0)))
    print("fp32 log against float64, worst error in units of u max(|log L|, 1): %.3f" % worst)
    assert 4.0 * worst <= E_LOG and (E_LOG == 4.0 or E_LOG <= 8.0 * worst), (worst, E_LOG)


def test_E_EXP_covers_these_cases():
    """the exp constant taken from the segment softmax's fuzz holds on these cases' arguments x - M too (same method)"""
    worst = 0.0
    for c in float_cases():
        if not (c.B and c.N):
            continue
        x = scores64(c)
        a = (x - x.max(axis=1, keepdims=True)).astype(np.float32)
        a = a[a > -87.0]
        e32, e64 = np.exp(a).astype(np.float64), np.exp(a.astype(np.float64))
        worst = max(worst, float((np.abs(e32 - e64) / (U * e64)).max(initial=0.0)))
    print("fp32 exp against float64 on these cases, worst error in units of u |value|: %.3f" % worst)
    assert 4.0 * worst <= E_EXP, (worst, E_EXP)


def test_cases_span_every_axis():
    cs = [case(k) for k in range(CASES)]
    ns = axis_N()
    s = split_len(257, 4097)
    assert s > 64 and s % 64 == 0 and len(set(ns)) == 12
    assert {c.B for c in cs} == set(BS) and {c.N for c in cs} == set(ns)
    assert {(c.d, c.exact) for c in cs} == {(64, True), (64, False), (128, True), (128, False)}
    assert {c.kind for c in cs} == set(KINDS)
    big = [c for c in cs if c.N == 4097 and c.B == 257]
    assert {c.exact for c in big} == {True, False} and all(split_len(c.B, c.N) == s for c in big)
    raw = [c for c in cs if c.kind == "raw" and c.B and c.N]
    assert max(float(np.abs(scores64(c)).max()) for c in raw) > 200.0          # fp32 exp overflows at 88.7
    for c in cs:
        if c.exact and c.B and c.N:
            x = scores64(c)
            top = np.sort(x, axis=1)
            assert np.array_equal(x.argmax(axis=1), c.jstar)
            assert c.N == 1 or float((top[:, -1] - top[:, -2]).min()) >= 128.0
            assert float(np.abs(c.Q).max()) <= 4 and np.array_equal(c.Q * 8, np.round(c.Q * 8))
            ref = lse64(c, x)[0]
            assert np.array_equal(ref.astype(np.float32).astype(np.float64), exact_expect(c)[0])      # the construction IS the formula
    ex = [c for c in cs if c.exact and c.N >= 66]
    assert any({0, c.N - 1, 31, 32, 63, 64} <= set(c.targets) for c in ex)
    e = next(c for c in ex if c.N == 4097)
    assert {s - 1, s} <= set(e.targets) and {s - 1, s} <= set(e.jstar.tolist())                       # maxima on a split boundary


def test_bound_is_sharp():
    """what the float mode's forward bound allows BEYOND the rounding of the logits themselves (sum_j p_ij delta_ij: the fp32 chain
    of d products, which no fp32 kernel avoids) stays below 3e-5 relative to max(|lse|, 1) in every case"""
    worst = 0.0
    for c in float_cases():
        if c.B and c.N:
            x = scores64(c)
            ref, F = forward_bound(c)
            own = (np.exp(x - ref[:, None]) * _logit_delta(c, x)).sum(axis=1)
            worst = max(worst, float(((F - own) / np.maximum(np.abs(ref), 1.0)).max()))
    print("forward bound beyond the logits' own rounding, worst relative to max(|lse|, 1): %.3e" % worst)
    assert worst <= 3e-5


# ------------------------------------------------------------------------------------------------ GPU: the raw C ABI, guarded
def _guarded(n):
    buf = torch.full((n + 2 * GUARD,), SENTINEL, dtype=torch.int32, device="cuda:0")
    return buf, buf[GUARD:GUARD + n].view(torch.float32)


def _guards_ok(buf, n, name):
    b = buf.cpu().numpy()
    assert (b[:GUARD] == SENTINEL).all() and (b[GUARD + n:] == SENTINEL).all(), (name, "wrote outside the output")
    assert not (b[GUARD:GUARD + n] == SENTINEL).any(), (name, "entries never written", int((b[GUARD:GUARD + n] == SENTINEL).sum()))


def _workspace(c):
    nbytes = int(_lib().mmrec_score_lse_workspace_bytes(c.B, c.N, c.d))
    return torch.full((nbytes // 4 + 4,), SENTINEL, dtype=torch.int32, device="cuda:0")      # a NaN wherever nothing was written


def raw_fwd(c, Q, K, name="fwd"):
    from mmrec_amd import hip_ops
    p, lib = hip_ops._p, _lib()
    buf, out = _guarded(c.B)
    ws = _workspace(c)
    rc = lib.mmrec_score_lse_f32(p(Q), p(K), c.B, c.N, c.d, c.scale, p(out), p(ws), hip_ops._stream())
    assert rc == 0, (name, rc)
    torch.cuda.synchronize()
    _guards_ok(buf, c.B, name)
    return out.clone()


def raw_bwd(c, Q, K, lse, g, name="bwd"):
    from mmrec_amd import hip_ops
    p, lib = hip_ops._p, _lib()
    bq, dq = _guarded(c.B * c.d)
    bk, dk = _guarded(c.N * c.d)
    ws = _workspace(c)
    rc = lib.mmrec_score_lse_bwd_f32(p(Q), p(K), c.B, c.N, c.d, c.scale, p(lse), p(g), p(dq), p(dk), p(ws), hip_ops._stream())
    assert rc == 0, (name, rc)
    torch.cuda.synchronize()
    _guards_ok(bq, c.B * c.d, name + " dQ")
    _guards_ok(bk, c.N * c.d, name + " dK")
    return dq.clone().view(c.B, c.d), dk.clone().view(c.N, c.d)


def _bits(t):
    return t.contiguous().view(torch.int32)


@pytest.mark.gpu
@pytest.mark.parametrize("k", range(CASES))
def test_score_lse_fuzz(k):
    c = case(k)
    name = "case %d (B %d N %d d %d %s scale %g)" % (k, c.B, c.N, c.d, c.kind, c.scale)
    Q, K, g = _on(c.Q), _on(c.K), _on(c.g)
    lse = raw_fwd(c, Q, K, name)
    w_f = check_fwd(lse, c, name)
    dq, dk = raw_bwd(c, Q, K, lse, g, name)
    w_b = check_bwd(dq, dk, c, name)
    print("%s: worst err / bound forward %.3f backward %.3f" % (name, w_f, w_b))
    # the same call again: the same bits, forward and both gradients
    lse2 = raw_fwd(c, Q, K, name)
    dq2, dk2 = raw_bwd(c, Q, K, lse2, g, name)
    assert torch.equal(_bits(lse), _bits(lse2)) and torch.equal(_bits(dq), _bits(dq2)) and torch.equal(_bits(dk), _bits(dk2)), name


@pytest.mark.gpu
@pytest.mark.parametrize("B,N", [(33, 0), (0, 65), (0, 0), (257, 0)])
def test_empty_operands(B, N):
    """an empty table: lse = -inf (torch.logsumexp's value) and zero gradients; an empty batch: nothing but a zeroed dK; in
    float mode too (the exact cases hold B = N = 0 only)"""
    c = case(1)
    rng = np.random.default_rng(B + N)
    c.B, c.N, c.exact = B, N, False
    c.Q, c.K = rng.standard_normal((B, c.d)).astype(np.float32), rng.standard_normal((N, c.d)).astype(np.float32)
    c.g = rng.standard_normal(B).astype(np.float32)
    Q, K, g = _on(c.Q), _on(c.K), _on(c.g)
    lse = raw_fwd(c, Q, K)
    assert check_fwd(lse, c) == 0.0
    assert lse.shape == (B,) and bool(torch.isneginf(lse).all())
    dq, dk = raw_bwd(c, Q, K, lse, g)
    assert check_bwd(dq, dk, c) == 0.0
    assert dq.shape == (B, c.d) and dk.shape == (N, c.d) and not bool(dq.any()) and not bool(dk.any())


@pytest.mark.gpu
@pytest.mark.parametrize("d", [64, 128])
def test_a_nan_row_of_q_leaves_every_other_row_alone(d):
    c = next(c for c in float_cases() if c.B == 257 and c.N == 4097)
    if c.d != d:
        rng = np.random.default_rng(5)
        c.d, c.Q, c.K = d, rng.standard_normal((c.B, d)).astype(np.float32), rng.standard_normal((c.N, d)).astype(np.float32)
    clean = raw_fwd(c, _on(c.Q), _on(c.K))
    for row in (0, 45, 128, 256):
        Qn = c.Q.copy()
        Qn[row, 7] = np.nan
        got = raw_fwd(c, _on(Qn), _on(c.K))
        keep = torch.ones(c.B, dtype=torch.bool, device=got.device)
        keep[row] = False
        assert torch.equal(_bits(got[keep]), _bits(clean[keep])), row
        assert not bool(torch.isfinite(got[row])), row
    assert bool(torch.isfinite(clean).all())


@pytest.mark.gpu
def test_no_b_by_n_matrix_is_ever_held():
    """B = 1024, N = 32768, d = 64, forward + backward through the op: the peak above the resident inputs stays below a quarter
    of ONE fp32 B x N matrix (33.5 MB; the gradients returned are 8.7 MB of it, a materialised matrix would be 134 MB)"""
    from mmrec_amd import hip_ops
    B, N, d = 1024, 32768, 64
    gen = torch.Generator(device="cuda:0").manual_seed(3)
    Q = torch.nn.functional.normalize(torch.randn(B, d, device="cuda:0", generator=gen)).requires_grad_()
    K = torch.nn.functional.normalize(torch.randn(N, d, device="cuda:0", generator=gen)).requires_grad_()
    assert hip_ops.score_lse_served(Q, K)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    lse = hip_ops.score_lse(Q, K, 5.0)
    lse.sum().backward()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    print("peak above the inputs: %.2f MB (limit %.2f MB)" % (peak / 2 ** 20, B * N / 2 ** 20))
    assert peak < B * N * 4 // 4, peak
    assert Q.grad.shape == (B, d) and K.grad.shape == (N, d)
    # and it is the formula: a float64 reference of a slice of the rows
    x = 5.0 * (Q.detach()[:8].double() @ K.detach().double().T)
    ref = torch.logsumexp(x, dim=1)
    assert float((lse.detach()[:8].double() - ref).abs().max()) <= 1e-5
    assert bool(torch.isfinite(Q.grad).all()) and bool(torch.isfinite(K.grad).all()) and float(K.grad.abs().max()) > 0


@pytest.mark.gpu
def test_forward_and_backward_replay_from_a_captured_graph():
    """B = 64, N = 200: forward + backward captured on one stream and replayed give the eager bits (no host synchronisation, no
    data-dependent launch shape)"""
    from mmrec_amd import hip_ops
    rng = np.random.default_rng(9)
    q0, k0 = rng.standard_normal((64, 64)).astype(np.float32) * 0.3, rng.standard_normal((200, 64)).astype(np.float32) * 0.3
    w = _on(rng.standard_normal(64).astype(np.float32))

    def step(Q, K):
        Q.grad = K.grad = None
        lse = hip_ops.score_lse(Q, K, 4.0)
        (lse * w).sum().backward()
        return lse.detach(), Q.grad, K.grad
    Q, K = _on(q0).requires_grad_(), _on(k0).requires_grad_()
    eager = [t.clone() for t in step(Q, K)]
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        held = step(Q, K)
    with torch.no_grad():                                   # other inputs in the same buffers, then the first ones again
        Q.copy_(_on(q0[::-1].copy())), K.copy_(_on(k0[::-1].copy()))
    graph.replay()
    torch.cuda.synchronize()
    other = [t.clone() for t in held]
    with torch.no_grad():
        Q.copy_(_on(q0)), K.copy_(_on(k0))
    graph.replay()
    torch.cuda.synchronize()
    for a, b, o in zip(eager, held, other):
        assert torch.equal(_bits(a), _bits(b))
        assert not torch.equal(_bits(a), _bits(o))          # the replay really computed
