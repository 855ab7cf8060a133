"""GPU: seeded differential fuzz of the fused edge attention (csrc/edge_attention.hip, mmrec_edge_attention_f32,
hip_ops.edge_attention) against float64 numpy of the three formulas as written here (`attention64`), never against another
kernel.  The raw C ABI is called over guarded, sentinel-filled outputs.

    s_p = <Q[r], KV[c_p]>     alpha_p = exp(s_p - m_r) / (sum_q exp(s_q - m_r) + eps),  m_r = max over row r     Y[r] = sum_p alpha_p KV[c_p]

The kernel's plan.  A 16-lane group walks its slots IN ORDER with an online softmax (m, den, acc[64]):
  score  4 roundings in a lane's chain + 4 in the butterfly: |s^ - s| <= delta = gamma(8) A + 8 * 2^-149, A = sum_i |Q_ri KV_ci|.
  group  one group per row (rows of <= group_max entries, and EVERY row when the call has no long-row list): a term of den / acc
         meets <= n = len additions; R = the number of times a new maximum rescaled the state.
  block  one workgroup per listed row: group g takes the slots 16 g ... 16 g + 15 of every 256: <= 16 ceil(len / 256) additions,
         then 16 fmas over the groups' states, each weighted by exp(m_g - m): n = 16 ceil(len / 256) + 16, R = the most
         rescales of one group + 1.
(`plan_of`).  R is bounded from the float64 scores: slot j can only rescale if s_j + delta_j > max_{i < j} (s_i - delta_i).
Two acceptance modes; each case uses one.
  exact  entries are multiples of 1/8 of magnitude <= 4, so every product (a multiple of 1/64) and every partial dot (below
         2^10) is exact.  In each row a power-of-two number k of scores share the maximum and all others lie at least 128 below:
         exp(-128) is 0 in fp32, so every weight is exactly 1 or 0 and the rescale at the maximum's arrival exactly 0, which
         wipes whatever was summed before it (`test_fp32_exp_is_exact_where_the_exact_mode_needs_it`).
         alpha must EQUAL 1/k or 0 (k + 1e-16 is k in fp32) and Y the float64 mean of the k rows (sums of <= 2^11 multiples of
         1/8 below 2^13: exact; the division by k too).
  float  normal tables, the scores' standard deviation 0.1 ... 30 per row, rows shifted by +-20; eps 1e-16, 1e-3, 0.5.
         With x = s - m, e = exp(x), u = 2^-24, E the device exp's error in u (the softmax fuzz's measured constant, checked
         on these cases' arguments by its method in `test_E_covers_these_cases`), dmax the row's largest delta:
             theta_q = u (|x_q| + delta_q + dmax + (R + 1) E + R) + gamma(n + 2)
         -- the subtractions s - m_now, m_now - m_next, ... of a term's chain telescope to |x| (widened by the score errors)
         seen through exp; (R + 1) exps; R rescale products; n additions, the eps and the division --
             a_q = expm1(delta_q + theta_q + 2 u)      b = sum_q e_q expm1(delta_q + theta_q) / den + (eps / den) expm1(dmax)
             rel_q = (1 + a_q) / (1 - b) - 1
         (alpha is invariant under a common shift of its row's scores, so the error of m itself only enters through eps).
             |alpha^ - alpha| <= alpha rel + 4 * 2^-126
             |Y^ - Y|_c       <= sum_q (alpha_q rel_q + 4 * 2^-126) |KV[c_q]_c|
Non-finite: a row whose scores hold a NaN, a +inf or nothing but -inf is NaN in every alpha and in Y[r]; a -inf next to a
finite maximum weighs exactly 0 -- float64's pattern, which the checker asks for value for value (NaN / not NaN).

Gradients through hip_ops.edge_attention (`grad_bound`): the backward is g = edge_dot(dY, KV) + dA, ds = segment softmax
backward(alpha^, g), dQ = SpMM(ds) KV, dKV = SpMM^T(alpha^) dY + SpMM^T(ds) Q; its bound is those ops' own (gamma(8) on the dots:
tests/test_edge_dot_fuzz_gpu.py; gamma(n + 2) alpha (|g| + sum alpha |g|) with the softmax's plan_n: tests/test_edge_softmax_
fuzz_gpu.py; gamma(plan_depth) on the SpMMs: tests/test_spmm_fuzz_gpu.py) carried forward to first order together with the
forward's alpha rel, times 1 + 2^-10 for the products of two such errors.

The tests without the gpu mark hold the bound honest: an fp32 numpy emulation of the plan and the torch composition pass the
checker, each planted error is rejected."""
import ctypes
import os

import numpy as np
import pytest
import scipy.sparse as sp
import torch

from tests.test_edge_softmax_fuzz_gpu import E_EXP, GUARD, SENTINEL, TINY
from tests.test_edge_softmax_fuzz_gpu import plan_n as softmax_plan_n
from tests.test_spmm_fuzz_gpu import U, _on, gamma, plan_depth

D = 64
LAYOUTS = ("lens", "hub3000", "one_row", "many", "dups")
CASES = 4 * len(LAYOUTS)
EPS = (1e-16, 1e-3, 0.5)
SCORE_N = 8


def group_max():
    from mmrec_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        from mmrec_amd.build import build
        build(verbose=False)
    return int(_lib.load().mmrec_edge_attention_group_max())


def axis_lens():
    gm = group_max()
    return (0, 1, 2, 15, 16, 17, 63, 64, 65, gm - 1, gm, gm + 1, 1025)


# ------------------------------------------------------------------------------------------------ host references
class Ref:
    pass


def attention64(Q, KV, seg, cols, n_rows, eps, *, drop=None, eps_each=False):
    """float64 of the three formulas over the edges (seg[e], cols[e]) -> Ref(s, A, x, e, den, alpha, Y).  The keywords plant
    errors: `drop` edges left out of their row's sums, `eps_each` eps added once per entry."""
    r = Ref()
    q, k = Q.astype(np.float64)[seg], KV.astype(np.float64)[cols]
    with np.errstate(invalid="ignore", over="ignore"):
        r.s, r.A = (q * k).sum(1), (np.abs(q) * np.abs(k)).sum(1)
        m = np.full(n_rows, -np.inf)
        np.maximum.at(m, seg, r.s)
        r.x = r.s - m[seg]
        r.e = np.exp(r.x)
        w = r.e.copy()
        if drop is not None:
            w[drop] = 0.0
        cnt = np.bincount(seg, minlength=n_rows)
        r.den = np.bincount(seg, weights=w, minlength=n_rows) + float(np.float32(eps)) * (cnt if eps_each else 1.0)
        r.alpha = r.e / r.den[seg]
        r.Y = _rows_sum(w / r.den[seg], seg, cols, n_rows, KV)
    return r


def _rows_sum(w, seg, cols, n_rows, KV):
    """sum_e w_e KV[cols[e]] into row seg[e] (float64; duplicates are separate terms; an explicit 0 * inf is NaN)"""
    mat = sp.csr_matrix((np.asarray(w, np.float64), (seg, cols)), shape=(n_rows, KV.shape[0]))
    with np.errstate(invalid="ignore", over="ignore"):
        return np.asarray(mat @ KV.astype(np.float64))


def _records(s, d):
    """upper bound of the rescales of an in-order walk over scores s known to within d (module docstring)"""
    if s.size == 0:
        return 0
    with np.errstate(invalid="ignore"):
        before = np.concatenate([[-np.inf], np.fmax.accumulate(s - d)[:-1]])
        return int((s + d > before).sum())


def plan_of(rowptr, order, ref, with_list, score_n=SCORE_N, composition=False):
    """per row (n, R) of the module docstring; `order` = COO position of CSR slot j.  composition: the three torch ops (a
    serial sum per row, no rescales)."""
    lens = np.diff(rowptr.astype(np.int64))
    n, R = lens.copy(), np.zeros(lens.size, np.int64)
    if composition:
        return n, R
    delta = gamma(score_n) * ref.A + score_n * 2.0 ** -149
    s_csr, d_csr = ref.s[order], delta[order]
    gm = group_max()
    for r in np.flatnonzero(lens):
        a, b = int(rowptr[r]), int(rowptr[r + 1])
        if with_list and lens[r] > gm:
            g = (np.arange(b - a) // 16) % 16
            R[r] = 1 + max(_records(s_csr[a:b][g == k], d_csr[a:b][g == k]) for k in range(16))
            n[r] = 16 * -(-lens[r] // 256) + 16
        else:
            R[r] = _records(s_csr[a:b], d_csr[a:b])
    return n, R


def forward_rel(c, ref, n, R, score_n=SCORE_N):
    """the float mode's relative bound per edge (module docstring)"""
    seg = c.seg
    with np.errstate(invalid="ignore", over="ignore"):
        delta = gamma(score_n) * ref.A + score_n * 2.0 ** -149
        dmax = np.zeros(c.n_rows)
        np.maximum.at(dmax, seg, np.where(np.isfinite(delta), delta, 0.0))
        live = ref.e > 0
        theta = U * (np.abs(ref.x) + delta + dmax[seg] + (R[seg] + 1) * E_EXP + R[seg]) + gamma(n[seg] + 2)
        a = np.where(live, np.expm1(delta + theta + 2 * U), 0.0)
        t = np.where(live, ref.e * np.expm1(delta + theta), 0.0)
        b = np.bincount(seg, weights=t, minlength=c.n_rows) / ref.den + float(np.float32(c.eps)) / ref.den * np.expm1(dmax)
        return (1.0 + a) / (1.0 - b[seg]) - 1.0


def _arr(got):
    return got.detach().cpu().double().numpy() if isinstance(got, torch.Tensor) else np.asarray(got, np.float64)


def check(alpha, Y, c, n=None, R=None, name="", ref=None, score_n=SCORE_N, skip=None):
    """alpha [n_edges], Y [n_rows, 64] against float64 in the case's mode; the float mode's worst err / bound.  skip: edges
    whose alpha is not looked at (absent edges)."""
    al, y = _arr(alpha), _arr(Y)
    assert al.shape == (c.ne,) and y.shape == (c.n_rows, D), (name, al.shape, y.shape)
    keep = np.ones(c.ne, bool) if skip is None else ~skip
    if c.exact:
        bad = (al != c.expect_alpha) & keep
        assert not bad.any(), (name, "alpha: exact mismatch", int(bad.sum()), "first at", int(np.argmax(bad)),
                               float(al[np.argmax(bad)]), float(c.expect_alpha[np.argmax(bad)]))
        bad = y != c.expect_Y
        assert not bad.any(), (name, "Y: exact mismatch", int(bad.sum()), "first at row", int(np.argmax(bad.any(1))))
        return 0.0
    ref = ref if ref is not None else c.ref
    rel = forward_rel(c, ref, n, R, score_n)
    nan = np.isnan(ref.alpha)
    assert np.isfinite(ref.alpha[~nan]).all()
    assert np.array_equal(np.isnan(al)[keep], nan[keep]), (name, "alpha: NaN pattern", int((np.isnan(al) != nan)[keep].sum()))
    with np.errstate(invalid="ignore"):
        tol_a = np.where(nan, 0.0, ref.alpha * rel + TINY)
        err = np.where(nan | ~keep, 0.0, np.abs(al - ref.alpha))
    viol = err > tol_a
    assert not viol.any(), (name, "alpha beyond the bound", int(viol.sum()), "first at", int(np.argmax(viol)),
                            float(al[np.argmax(viol)]), float(ref.alpha[np.argmax(viol)]), float(rel[np.argmax(viol)]))
    worst = float((err[~nan] / tol_a[~nan]).max(initial=0.0))
    ynan = np.isnan(ref.Y)
    assert np.array_equal(np.isnan(y), ynan), (name, "Y: NaN pattern", int((np.isnan(y) != ynan).sum()))
    with np.errstate(invalid="ignore", over="ignore"):
        tol_y = _rows_sum(tol_a, c.seg, c.cols, c.n_rows, np.abs(c.KV)) + 2.0 ** -140
        fin = ~ynan & np.isfinite(tol_y)                              # (a NaN of float64: the pattern was the check)
        err_y = np.where(fin, np.abs(y - ref.Y), 0.0)
        tol_y = np.where(fin, tol_y, 1.0)
    viol = err_y > tol_y
    assert not viol.any(), (name, "Y beyond the bound", int(viol.sum()), "first at row", int(np.argmax(viol.any(1))),
                            float(err_y[viol].max()), float(tol_y[viol].min()))
    return max(worst, float((err_y / tol_y).max(initial=0.0)))


# ------------------------------------------------------------------------------------------------ cases
class Case:
    pass


def _row_lens(layout, rng, k):
    al = axis_lens()
    small = lambda n: rng.integers(0, 40, n)                          # noqa: E731
    if layout == "lens":                                              # every length of the axis, empty rows first and last
        return np.concatenate([[0, 0], rng.permutation(al), [0]])
    if layout == "hub3000":
        return np.concatenate([small(30), [3000], small(30)])
    if layout == "one_row":
        return np.array([(2, 17, group_max(), 1025)[k % 4]])
    if layout == "many":                                              # several workgroups of short rows, a few long ones
        lens = rng.geometric(0.1, 3000) - 1
        lens[rng.integers(0, 3000, 4)] = group_max() + rng.integers(1, 300, 4)
        return lens
    return np.concatenate([small(60), [group_max() + 5], [0, 0], small(60)])      # "dups": three source rows for everything


def _finish(c, rng, lens, n_kv):
    lens = np.asarray(lens, np.int64)
    c.lens, c.n_rows, c.ne, c.n_kv = lens, lens.size, int(lens.sum()), n_kv
    c.rowptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    rid = np.repeat(np.arange(c.n_rows), lens)                        # row of CSR slot j
    if c.shuffled:                                                    # slot j lives at COO position perm[j]
        c.perm = rng.permutation(c.ne).astype(np.int64)
        c.seg = np.empty(c.ne, np.int64)
        c.seg[c.perm] = rid
    else:
        c.perm, c.seg = None, rid
    c.order = c.perm if c.shuffled else np.arange(c.ne)


def draw_case(seed):
    rng = np.random.default_rng(7700 + seed)
    c = Case()
    c.seed = seed
    c.layout = LAYOUTS[seed % len(LAYOUTS)]
    c.exact = (seed // len(LAYOUTS)) % 2 == 0
    c.shuffled = (seed // (2 * len(LAYOUTS))) % 2 == 1
    c.eps = 1e-16 if c.exact else EPS[(seed % 7) % len(EPS)]
    n_kv = 3 if c.layout == "dups" else int(rng.integers(40, 400))
    _finish(c, rng, _row_lens(c.layout, rng, seed), n_kv + (n_kv if c.exact else 0))
    ne = c.ne
    if c.exact:
        # columns 0-7: Q = 4, KV = +4 in the "top" source rows [0, n_kv) and -4 in the "low" ones [n_kv, 2 n_kv): +-128;
        # columns 8-35: Q random in [-1, 1], the top rows share ONE pattern (equal scores), the low rows are random in [-2, 2]
        # (|dot| <= 56 each: a low score is >= 256 - 112 = 144 below the top); columns 36-63: Q = 0, KV random in [-4, 4]
        Q = np.zeros((c.n_rows, D))
        Q[:, :8] = 4.0
        Q[:, 8:36] = rng.integers(-8, 9, (c.n_rows, 28)) / 8.0
        KV = rng.integers(-32, 33, (2 * n_kv, D)) / 8.0
        KV[:n_kv, :8], KV[n_kv:, :8] = 4.0, -4.0
        KV[:n_kv, 8:36] = rng.integers(-16, 17, 28) / 8.0
        KV[n_kv:, 8:36] = rng.integers(-16, 17, (n_kv, 28)) / 8.0
        cols = n_kv + rng.integers(0, n_kv, ne)
        c.expect_alpha = np.zeros(ne)
        for r in np.flatnonzero(c.lens):
            where = c.order[c.rowptr[r]:c.rowptr[r + 1]]
            k = 1 << int(rng.integers(0, int(np.log2(where.size)) + 1))
            top = rng.choice(where, size=k, replace=False)
            cols[top] = rng.integers(0, n_kv, k)
            c.expect_alpha[top] = 1.0 / k
        c.Q, c.KV, c.cols = Q.astype(np.float32), KV.astype(np.float32), cols
        c.expect_Y = _rows_sum(c.expect_alpha, c.seg, c.cols, c.n_rows, c.KV)
    else:
        std = rng.choice([0.1, 1.0, 5.0, 30.0], c.n_rows)
        shift = rng.choice([0.0, 20.0, -20.0], c.n_rows)
        KV = rng.standard_normal((n_kv, D))
        KV[:, D - 1] = 1.0
        Q = rng.standard_normal((c.n_rows, D)) * (std / 8.0)[:, None]
        Q[:, D - 1] = shift
        c.Q, c.KV, c.cols = Q.astype(np.float32), KV.astype(np.float32), rng.integers(0, n_kv, ne)
    c.colidx = c.cols[c.order].astype(np.int32)
    c.ref = attention64(c.Q, c.KV, c.seg, c.cols, c.n_rows, c.eps)
    return c


_CASES = {}


def case(seed):
    """the cases (and their float64 reference) are drawn once and shared; nothing changes them"""
    if seed not in _CASES:
        _CASES[seed] = draw_case(seed)
    return _CASES[seed]


def float_cases():
    return [case(s) for s in range(CASES) if not case(s).exact]


# ------------------------------------------------------------------------------------------------ CPU: the checker and the cases
def _torch_composition(c):
    """the three ops in fp32 torch on the CPU: per-edge dots, the scatter / gather softmax, index_add"""
    from mmrec_amd import hip_ops
    Q, KV, seg, cols = torch.from_numpy(c.Q), torch.from_numpy(c.KV), torch.from_numpy(c.seg), torch.from_numpy(c.cols)
    alpha = hip_ops.segment_softmax_torch((Q[seg] * KV[cols]).sum(-1), seg, c.n_rows, c.eps)
    Y = torch.zeros(c.n_rows, D).index_add_(0, seg, alpha.unsqueeze(1) * KV[cols])
    return alpha.numpy(), Y.numpy()


def _f32(x):
    return np.asarray(x, np.float32)


def _fma(a, b, acc):
    return _f32(np.float64(a) * np.float64(b) + np.float64(acc))


def emulate(c, with_list, *, no_rescale_row=None, drop_group=None):
    """the kernel's plan in fp32 numpy: lane chains and butterfly for the scores, the in-order online softmax per group, the
    16-state combine of a listed row.  The keywords plant errors: the rescale after a new maximum left out in one row; one
    group's state of the listed rows dropped from the combine."""
    Q, KV, gm, eps = c.Q, c.KV, group_max(), np.float32(c.eps)
    alpha, Y = np.zeros(c.ne, np.float32), np.zeros((c.n_rows, D), np.float32)
    rid = np.repeat(np.arange(c.n_rows), c.lens)
    q, k = Q[rid].reshape(-1, 16, 4), KV[c.colidx].reshape(-1, 16, 4)
    lane = _f32(q[:, :, 3] * k[:, :, 3])
    for i in (2, 1, 0):
        lane = _fma(q[:, :, i], k[:, :, i], lane)
    for m in (8, 4, 2, 1):
        lane = _f32(lane + lane[:, np.arange(16) ^ m])
    s = lane[:, 0]

    def walk(slots, rescale=True):
        m, den, acc = np.float32(-np.inf), np.float32(0), np.zeros(D, np.float32)
        with np.errstate(invalid="ignore", over="ignore"):
            for j in slots:
                if s[j] > m:
                    if rescale:
                        sc = np.exp(_f32(m - s[j]))
                        den, acc = _f32(den * sc), _f32(acc * sc)
                    m = s[j]
                e = np.float32(0) if s[j] == -np.inf else np.exp(_f32(s[j] - m))
                den, acc = _f32(den + e), _fma(e, KV[c.colidx[j]], acc)
        return m, den, acc
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        for r in np.flatnonzero(c.lens):
            a, b = int(c.rowptr[r]), int(c.rowptr[r + 1])
            if with_list and b - a > gm:
                st = [walk([j for j in range(a, b) if ((j - a) // 16) % 16 == g]) for g in range(16)]
                m = np.float32(max(x[0] for x in st))
                den, acc = np.float32(0), np.zeros(D, np.float32)
                for g, (mg, dg, ag) in enumerate(st):
                    if g == drop_group:
                        continue
                    w = np.float32(1) if mg == m else np.exp(_f32(mg - m))
                    den, acc = _fma(dg, w, den), _fma(ag, w, acc)
            else:
                m, den, acc = walk(range(a, b), rescale=r != no_rescale_row)
            dn = np.float32(np.nan) if m == -np.inf else _f32(den + eps)
            Y[r] = _f32(acc / dn)
            alpha[c.order[a:b]] = _f32(np.exp(_f32(s[a:b] - m)) / dn)
    return alpha, Y


def test_draw_case_is_deterministic():
    a, b = draw_case(7), draw_case(7)
    assert np.array_equal(a.Q, b.Q) and np.array_equal(a.KV, b.KV) and np.array_equal(a.seg, b.seg) and np.array_equal(a.cols, b.cols)


def test_cases_span_every_axis():
    gm = group_max()
    seen = {"lens": set(), "combo": set(), "eps": set(), "one_row": set()}
    for s in range(CASES):
        c = case(s)
        seen["lens"].update(int(x) for x in c.lens)
        seen["combo"].add((c.layout, c.exact, c.shuffled))
        if not c.exact:
            seen["eps"].add(c.eps)
        if c.n_rows == 1:
            seen["one_row"].add(c.ne)
        assert c.n_rows <= 4200 and c.seg.size == c.ne and np.array_equal(np.bincount(c.seg, minlength=c.n_rows), c.lens)
        assert np.array_equal(c.seg[c.order], np.repeat(np.arange(c.n_rows), c.lens))
        if c.shuffled and c.ne > 50:
            assert (np.diff(c.seg) < 0).any()                         # the COO order is not the CSR order
        if c.ne > 100:                                                # duplicate edges
            assert np.unique(c.seg * (1 << 20) + c.cols).size < c.ne
        if c.exact:
            assert (np.abs(c.Q) <= 4).all() and (np.abs(c.KV) <= 4).all() and (c.Q * 8 == np.round(c.Q * 8)).all()
            assert (c.KV * 8 == np.round(c.KV * 8)).all()
            r = c.ref                                                 # the construction IS the formulas
            top = r.x == 0
            assert (r.x[~top] <= -128).all() and np.array_equal(top, c.expect_alpha > 0)
            assert np.array_equal(r.alpha.astype(np.float32).astype(np.float64), c.expect_alpha)
            assert np.abs(r.Y - c.expect_Y).max(initial=0.0) <= 1e-12
            k = np.bincount(c.seg, weights=top, minlength=c.n_rows)[c.lens > 0]
            assert (k == 2.0 ** np.round(np.log2(k))).all()
    assert set(axis_lens()) | {3000} <= seen["lens"], sorted(seen["lens"])
    assert seen["combo"] == {(l, e, p) for l in LAYOUTS for e in (True, False) for p in (True, False)}
    assert seen["eps"] == set(EPS) and len(seen["one_row"]) >= 3
    assert any(case(s).n_rows > 2500 for s in range(CASES)) and any(case(s).n_kv == 3 for s in range(CASES))
    assert gm >= 64


def test_fp32_exp_is_exact_where_the_exact_mode_needs_it():
    """a score minus its row's maximum is 0 or at most -128 in an exact case, and fp32 exp gives exactly 1 and exactly 0 there.
    What the online walk sums BEFORE the row's maximum arrives (low scores against a low running maximum) is not exact, but
    finite, and is multiplied by exp(<= -128) = 0 when the maximum arrives (or by that weight in a listed row's combine); after
    it, every factor is exp(0) or exp(<= -128).  The torch composition passes the exact mode."""
    assert np.exp(np.float32(0)) == 1 and np.exp(np.float32(-128)) == 0 and torch.exp(torch.tensor(-128.0)).item() == 0
    for c in (case(s) for s in range(CASES) if case(s).exact):
        args = _f32(np.unique(c.ref.x))
        out = np.exp(args)
        assert ((out == 1) | (out == 0)).all() and ((args == 0) == (out == 1)).all()
        if c.lens.max(initial=0) <= 1100:
            check(*_torch_composition(c), c, name="torch composition, exact, seed %d" % c.seed)


def test_E_covers_these_cases():
    """the softmax fuzz's method on this file's arguments: fp32 exp (numpy, CPU) against float64 over x = s - m of every float
    case, results that are normal numbers; E_EXP must be at least four times the worst error (in u |value|)"""
    worst = 0.0
    for c in float_cases():
        x = _f32(c.ref.x)
        x = x[np.isfinite(x) & (x > -87.0)]
        a, b = np.exp(x).astype(np.float64), np.exp(x.astype(np.float64))
        worst = max(worst, float((np.abs(a - b) / (U * b)).max(initial=0.0)))
    print("fp32 exp against float64 on the attention cases, worst error in u |value|: %.3f" % worst)
    assert 4.0 * worst <= E_EXP, (worst, E_EXP)


def _small_float_cases():
    return [c for c in float_cases() if c.layout in ("lens", "dups", "one_row")]


def test_plan_emulation_passes_the_checker():
    ran, worst = 0, 0.0
    for c in _small_float_cases():
        for with_list in (True, False):
            n, R = plan_of(c.rowptr, c.order, c.ref, with_list)
            worst = max(worst, check(*emulate(c, with_list), c, n, R, "emulation seed %d list %s" % (c.seed, with_list)))
            ran += 1
    print("fp32 emulation of the plan: %d runs, worst err / bound %.3f" % (ran, worst))
    assert ran >= 6 and worst <= 1.0
    c = next(case(s) for s in range(CASES) if case(s).exact and case(s).layout == "lens" and case(s).shuffled)
    for with_list in (True, False):
        check(*emulate(c, with_list), c, name="emulation, exact")


def test_torch_composition_passes_the_checker():
    """dots summed over 64 products (65 roundings at most), a serial sum per row, no rescales"""
    ran, worst = 0, 0.0
    for c in float_cases():
        if c.lens.max(initial=0) > 1100:
            continue
        n, R = plan_of(c.rowptr, c.order, c.ref, True, composition=True)
        worst = max(worst, check(*_torch_composition(c), c, n, R, "torch composition seed %d" % c.seed, score_n=65))
        ran += 1
    print("torch composition: %d cases, worst err / bound %.3f" % (ran, worst))
    assert ran >= 4


def test_checker_rejects_planted_errors():
    c = next(c for c in float_cases() if c.layout == "lens" and c.shuffled)
    assert c.eps >= 1e-3
    n, R = plan_of(c.rowptr, c.order, c.ref, True)
    ref = c.ref
    f32 = lambda r: (r.alpha.astype(np.float32), r.Y.astype(np.float32))      # noqa: E731
    assert check(*f32(ref), c, n, R, "clean") <= 1.0
    rows = [int(r) for r in np.flatnonzero((c.lens >= 15) & (c.lens <= 65))]
    # an edge dropped from its row's sums (one that carries a thousandth of them or more)
    q = next(int(q) for r in rows for q in np.flatnonzero(c.seg == r) if 1e-3 <= ref.alpha[q] <= 0.5)
    with pytest.raises(AssertionError):
        check(*f32(attention64(c.Q, c.KV, c.seg, c.cols, c.n_rows, c.eps, drop=[q])), c, n, R)
    # that edge counted in the neighbouring row
    seg2 = c.seg.copy()
    seg2[q] = c.seg[q] + 1 if c.lens[c.seg[q] + 1] else c.seg[q] - 1
    bad = attention64(c.Q, c.KV, seg2, c.cols, c.n_rows, c.eps)
    with pytest.raises(AssertionError):
        check(*f32(bad), c, n, R)
    # alpha left in CSR order (Y right)
    with pytest.raises(AssertionError):
        check(ref.alpha[c.order].astype(np.float32), ref.Y.astype(np.float32), c, n, R)
    # eps added per entry
    with pytest.raises(AssertionError):
        check(*f32(attention64(c.Q, c.KV, c.seg, c.cols, c.n_rows, c.eps, eps_each=True)), c, n, R)
    # the rescale after a new maximum left out, in a row whose first slot is not its maximum
    r = next(r for r in rows if ref.x[c.order[c.rowptr[r]]] < -1.0)
    with pytest.raises(AssertionError):
        check(*emulate(c, True, no_rescale_row=r), c, n, R)
    # a listed row's partial state (one group of 16) dropped from the combine
    assert (c.lens > group_max()).any()
    with pytest.raises(AssertionError):
        check(*emulate(c, True, drop_group=5), c, n, R)
    # exact mode: an edge moved to the neighbouring row, and alpha in CSR order
    c = next(case(s) for s in range(CASES) if case(s).exact and case(s).layout == "lens" and case(s).shuffled)
    check(c.expect_alpha.astype(np.float32), c.expect_Y.astype(np.float32), c, name="clean exact")
    r = int(np.flatnonzero(c.lens >= 16)[0])
    q = int(np.flatnonzero((c.seg == r) & (c.expect_alpha > 0))[0])
    seg2 = c.seg.copy()
    seg2[q] = r - 1 if c.lens[r - 1] else r + 1
    with pytest.raises(AssertionError):
        check(*f32(attention64(c.Q, c.KV, seg2, c.cols, c.n_rows, c.eps)), c)
    with pytest.raises(AssertionError):
        check(c.expect_alpha[c.order].astype(np.float32), c.expect_Y.astype(np.float32), c)


# ------------------------------------------------------------------------------------------------ GPU: the raw C ABI, guarded
class _Dev:
    """a case's arrays on the device + the long-row list the wrapper would build"""

    def __init__(self, c, colidx=None, perm=None):
        from mmrec_amd import hip_ops
        self.rowptr, self.colidx = _on(c.rowptr), _on(c.colidx if colidx is None else colidx)
        perm = c.perm if perm is None else perm
        self.perm = None if perm is None else _on(perm)
        self.Q, self.KV = _on(c.Q), _on(c.KV)
        lr = hip_ops.segment_long_rows(c.rowptr)
        self.long_rows, self.n_long = (_on(lr), lr.size) if lr.size else (None, 0)


def _guarded(n):
    buf = torch.full((n + 2 * GUARD,), SENTINEL, dtype=torch.int32, device="cuda:0")
    return buf, buf[GUARD:GUARD + n].view(torch.float32)


def _guards_ok(buf, n, name, unwritten=None):
    """nothing outside the output was written; inside it exactly the entries of `unwritten` (a mask, default none) still hold
    the sentinel"""
    b = buf.cpu().numpy()
    assert (b[:GUARD] == SENTINEL).all() and (b[GUARD + n:] == SENTINEL).all(), (name, "wrote outside the output")
    left = b[GUARD:GUARD + n] == SENTINEL
    want = np.zeros(n, bool) if unwritten is None else unwritten
    assert np.array_equal(left, want), (name, "never written", int((left & ~want).sum()), "written, must not be", int((~left & want).sum()))


def raw(c, dev, with_list, name="raw", unwritten=None, n_kv=None):
    from mmrec_amd import hip_ops
    p, lib = hip_ops._p, hip_ops._lib.load()
    abuf, alpha = _guarded(c.ne)
    ybuf, y = _guarded(c.n_rows * D)
    rc = lib.mmrec_edge_attention_f32(p(dev.rowptr), c.n_rows, p(dev.colidx), p(dev.perm), p(dev.long_rows) if with_list else None,
                                      dev.n_long if with_list else 0, p(dev.Q), c.n_rows, p(dev.KV), c.n_kv if n_kv is None else n_kv,
                                      D, c.ne, c.eps, ctypes.c_void_p(y.data_ptr()), ctypes.c_void_p(alpha.data_ptr()),
                                      hip_ops._stream())
    assert rc == 0, (name, rc)
    torch.cuda.synchronize()
    _guards_ok(abuf, c.ne, name + " alpha", unwritten)
    _guards_ok(ybuf, c.n_rows * D, name + " Y")                        # EVERY row of Y is written, empty ones too
    return alpha, y.view(c.n_rows, D)


def _wrapper_graph(c):
    from mmrec_amd import hip_ops
    return hip_ops.DynGraph(_on(c.seg.astype(np.int64)), _on(c.cols.astype(np.int64)), c.n_rows, c.n_kv)


@pytest.mark.gpu
@pytest.mark.parametrize("seed", range(CASES))
def test_edge_attention_fuzz(seed):
    from mmrec_amd import hip_ops
    c = case(seed)
    dev = _Dev(c)
    assert (dev.n_long > 0) == bool((c.lens > group_max()).any())
    worst = 0.0
    for with_list in (True, False):                                   # without the list every row goes through the group kernel
        n, R = (None, None) if c.exact else plan_of(c.rowptr, c.order, c.ref, with_list)
        tag = "seed %d %s" % (seed, "list" if with_list else "n_long = 0")
        alpha, y = raw(c, dev, with_list, tag)
        worst = max(worst, check(alpha, y, c, n, R, tag))
        empty = c.lens == 0
        assert not y.cpu().numpy()[empty].any(), (tag, "an empty row of Y is not zero")
    dyn = _wrapper_graph(c)                                           # through the wrapper: its own (stable) CSR order
    Q, KV = _on(c.Q), _on(c.KV)
    assert hip_ops.edge_attention_served(Q, KV, dyn)
    y, alpha = hip_ops.edge_attention(Q, KV, dyn, eps=c.eps)
    torch.cuda.synchronize()
    order = np.argsort(c.seg, kind="stable")
    assert np.array_equal(order, dyn.perm.cpu().numpy())
    n, R = (None, None) if c.exact else plan_of(c.rowptr, order, c.ref, True)
    worst = max(worst, check(alpha, y, c, n, R, "wrapper seed %d" % seed))
    print("edge_attention fuzz seed %d: %s %s %s rows %d edges %d longest %d eps %g worst err / bound %.3f" % (
        seed, c.layout, "exact" if c.exact else "float", "shuffled" if c.shuffled else "csr order", c.n_rows, c.ne,
        int(c.lens.max(initial=0)), c.eps, worst))


# ------------------------------------------------------------------------------------------------ GPU: targeted tests
def _nonfinite_case():
    """source rows 0, 1, 2 hold -inf, +inf and NaN in column 0, which only the DESIGNATED rows (Q[r, 0] = 1; 0 elsewhere, and
    those rows never name the three) multiply: a designated row gets the non-finite score wherever it names one of them --
    early, late, beyond the first 16 slots, in a group row, a listed row and a hub -- and rows of nothing but -inf; finite rows
    in between"""
    gm = group_max()
    rng = np.random.default_rng(98)
    NEG, POS, NAN = 0, 1, 2
    spec = [(2, {1: NEG}), (2, {0: NEG, 1: NEG}), (2, {0: POS}), (2, {1: NAN}), (1, {0: NAN}), (1, {0: NEG}), (1, {0: POS}), (1, {}),
            (17, {16: NAN}), (100, {70: POS}), (100, {0: NEG, 3: NEG}), (gm, {gm - 1: NAN}), (gm + 1, {gm: NAN}), (gm + 1, {5: POS}),
            (gm + 40, {0: NEG, 100: NEG}), (3000, {2999: NAN}), (3000, {1500: POS}), (1500, {7: NEG, 800: NEG}),
            (300, {i: NEG for i in range(300)}), (64, {i: NEG for i in range(64)}), (2000, {}), (30, {}), (0, {})]
    c = Case()
    c.exact, c.eps, c.seed, c.shuffled, c.layout = False, 1e-16, -1, True, "nonfinite"
    _finish(c, rng, [n for n, _ in spec], 60)
    KV = rng.standard_normal((c.n_kv, D))
    KV[:3, 0] = (-np.inf, np.inf, np.nan)
    Q = rng.standard_normal((c.n_rows, D)) * 0.3
    Q[:, 0] = 0.0
    colidx = rng.integers(3, c.n_kv, c.ne)
    for r, (n, special) in enumerate(spec):
        if special:
            Q[r, 0] = 1.0
        for at, which in special.items():
            colidx[c.rowptr[r] + at] = which
    c.Q, c.KV, c.colidx = Q.astype(np.float32), KV.astype(np.float32), colidx.astype(np.int32)
    c.cols = np.empty(c.ne, np.int64)
    c.cols[c.order] = colidx
    c.ref = attention64(c.Q, c.KV, c.seg, c.cols, c.n_rows, c.eps)
    c.poisoned = np.array([any(w != NEG for w in sp_.values()) or (n > 0 and len(sp_) == n) for n, sp_ in spec])
    return c


def test_nonfinite_case_follows_the_rule_in_float64():
    """(CPU) the float64 formulas give exactly the rule the checker then asks of the kernel"""
    c = _nonfinite_case()
    ref = c.ref
    assert c.poisoned.sum() >= 12 and (~c.poisoned).sum() >= 8
    for r in range(c.n_rows):
        e = c.seg == r
        if c.poisoned[r]:
            assert np.isnan(ref.alpha[e]).all() and np.isnan(ref.Y[r]).all(), r
        else:
            assert np.isfinite(ref.alpha[e]).all() and (ref.alpha[e][ref.s[e] == -np.inf] == 0).all(), r
            assert np.isfinite(ref.Y[r, 1:]).all(), r                 # (column 0: 0 * -inf where a -inf source row is named)
            assert c.lens[r] == 0 or abs(ref.alpha[e].sum() - 1) < 1e-12
    assert int((ref.alpha == 0).sum()) >= 7
    for with_list in (True, False):                                   # and the plan's fp32 emulation follows it
        check(*emulate(c, with_list), c, *plan_of(c.rowptr, c.order, c.ref, with_list), "non-finite emulation")


@pytest.mark.gpu
def test_non_finite_rows_value_for_value():
    c = _nonfinite_case()
    dev = _Dev(c)
    assert dev.n_long >= 6
    for with_list in (True, False):
        n, R = plan_of(c.rowptr, c.order, c.ref, with_list)
        alpha, y = raw(c, dev, with_list, "non-finite list %s" % with_list)
        check(alpha, y, c, n, R, "non-finite list %s" % with_list)
        a = alpha.cpu().numpy()
        assert (a[(c.ref.s == -np.inf) & ~c.poisoned[c.seg]] == 0).all()     # -inf next to a finite maximum: exactly 0
        assert np.isnan(y.cpu().numpy()[c.poisoned]).all()


@pytest.mark.gpu
def test_out_of_range_ids_are_absent_edges():
    """a colidx outside [0, n_kv) (-1, n_kv, far beyond) or a perm entry outside [0, n_edges) is an absent edge: the result is
    that of the graph without it, its alpha keeps the sentinel, nothing outside the outputs is written; a row left with absent
    edges only is a row of zeros"""
    base = next(c for c in float_cases() if c.layout == "lens" and c.shuffled)
    rng = np.random.default_rng(3)
    absent = rng.random(base.ne) < 0.1                                # by CSR slot
    gone = int(np.flatnonzero(base.lens == 2)[0])
    absent[base.rowptr[gone]:base.rowptr[gone + 1]] = True            # a whole row
    for what in ("colidx", "perm"):
        colidx, perm = base.colidx.copy(), base.perm.copy()
        bad = np.flatnonzero(absent)
        if what == "colidx":
            colidx[bad] = rng.choice([-1, base.n_kv, base.n_kv + 12345, -(1 << 31), (1 << 31) - 1], bad.size)
        else:
            perm[bad] = rng.choice([-1, base.ne, base.ne + 12345, -(1 << 40), 1 << 40], bad.size)
        c = Case()
        c.__dict__.update(base.__dict__)
        keep = np.ones(base.ne, bool)
        keep[base.order[bad]] = False                                 # by COO position
        # float64 of the graph WITHOUT those edges, spread back over all positions (an absent edge: score -inf, weight 0)
        sub = attention64(base.Q, base.KV, base.seg[keep], base.cols[keep], base.n_rows, base.eps)
        ref = Ref()
        for k, fill in (("s", -np.inf), ("A", 0.0), ("x", -np.inf), ("e", 0.0), ("alpha", 0.0)):
            full = np.full(base.ne, fill)
            full[keep] = getattr(sub, k)
            setattr(ref, k, full)
        ref.den, ref.Y = sub.den, sub.Y
        dev = _Dev(c, colidx=colidx, perm=perm)
        assert not np.bincount(base.seg[keep], minlength=base.n_rows)[gone]
        for with_list in (True, False):
            n, R = plan_of(c.rowptr, c.order, ref, with_list)
            # the absent edges' positions keep the sentinel: the edge's own (bad colidx) or the one no slot maps to (bad perm)
            alpha, y = raw(c, dev, with_list, "bad %s list %s" % (what, with_list), unwritten=~keep)
            check(alpha, y, c, n, R, "bad %s list %s" % (what, with_list), ref=ref, skip=~keep)
            assert not y.cpu().numpy()[gone].any()


@pytest.mark.gpu
def test_two_runs_give_identical_bits():
    from mmrec_amd import hip_ops
    c = next(c for c in float_cases() if c.layout == "hub3000" and c.shuffled)
    dev = _Dev(c)
    for with_list in (True, False):
        a, b = raw(c, dev, with_list), raw(c, dev, with_list)
        for x, y in zip(a, b):
            assert torch.equal(x.view(torch.int32), y.view(torch.int32)), with_list
    dyn = _wrapper_graph(c)
    Q, KV = _on(c.Q), _on(c.KV)
    a, b = hip_ops.edge_attention(Q, KV, dyn), hip_ops.edge_attention(Q, KV, dyn)
    for x, y in zip(a, b):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32))


def test_argument_errors():
    """(no launch: runs without a GPU) the stated codes, in the stated order"""
    from mmrec_amd import _lib
    group_max()
    f = _lib.load().mmrec_edge_attention_f32
    one = np.zeros(4, np.int32).ctypes.data_as(_lib._P)

    def call(rowptr=one, n_rows=3, colidx=one, long_rows=None, n_long=0, Q=one, n_q=3, KV=one, n_kv=5, d=64, ne=5, Y=one, alpha=one):
        return f(rowptr, n_rows, colidx, None, long_rows, n_long, Q, n_q, KV, n_kv, d, ne, 1e-16, Y, alpha, None)
    for d in (0, 8, 32, 63, 65, 128):
        assert call(d=d) == 10002                                     # d == 64 only
    for kw in ({"n_rows": -1}, {"ne": -1}, {"n_long": -1}, {"n_q": -1}, {"n_kv": -1}):
        assert call(**kw) == 10001
    none = dict(rowptr=None, colidx=None, Q=None, KV=None, Y=None, alpha=None)
    assert call(n_rows=0, **none) == 0 and call(ne=0, **none) == 0    # nothing to launch: pointers may be NULL
    assert call(ne=2 ** 31) == 10002 and call(n_kv=2 ** 31) == 10002
    assert call(n_q=2) == 10001                                       # fewer rows of Q than rows
    for k in none:
        assert call(**{k: None}) == 10001, k
    assert call(n_long=2) == 10001                                    # a long-row count without a list


# ------------------------------------------------------------------------------------------------ GPU: gradients through hip_ops
def _grad_case(same):
    """a square graph (so that Q may be KV): short rows, empty rows, one row beyond the group maximum; float tables"""
    rng = np.random.default_rng(55 + same)
    c = Case()
    c.exact, c.eps, c.seed, c.shuffled, c.layout = False, 1e-16, -2, True, "grad"
    n = 400
    lens = rng.integers(0, 30, n)
    lens[7], lens[200], lens[0], lens[-1] = group_max() + 50, 70, 0, 0
    _finish(c, rng, lens, n)
    c.cols = rng.integers(0, n, c.ne)
    c.colidx = c.cols[c.order].astype(np.int32)
    c.KV = (rng.standard_normal((n, D)) * 0.4).astype(np.float32)
    c.Q = c.KV if same else (rng.standard_normal((n, D)) * 0.4).astype(np.float32)
    c.dY = rng.standard_normal((n, D)).astype(np.float32)
    c.dA = rng.standard_normal(c.ne).astype(np.float32)
    c.ref = attention64(c.Q, c.KV, c.seg, c.cols, c.n_rows, c.eps)
    return c


def grads64(c, use_y, use_a, same):
    """float64 autograd of the three formulas (torch, CPU) -> (dQ, dKV), or their sum when Q is KV"""
    seg, cols = torch.from_numpy(c.seg), torch.from_numpy(c.cols)
    Q = torch.from_numpy(c.Q).double().requires_grad_()
    KV = Q if same else torch.from_numpy(c.KV).double().requires_grad_()
    s = (Q[seg] * KV[cols]).sum(-1)
    m = torch.full((c.n_rows,), -np.inf, dtype=torch.float64).scatter_reduce(0, seg, s.detach(), "amax")
    e = (s - m[seg]).exp()
    alpha = e / (torch.zeros(c.n_rows, dtype=torch.float64).index_add_(0, seg, e)[seg] + float(np.float32(c.eps)))
    Y = torch.zeros(c.n_rows, D, dtype=torch.float64).index_add_(0, seg, alpha.unsqueeze(1) * KV[cols])
    out = 0.0
    if use_y:
        out = out + (Y * torch.from_numpy(c.dY).double()).sum()
    if use_a:
        out = out + (alpha * torch.from_numpy(c.dA).double()).sum()
    out.backward()
    return (Q.grad.numpy(),) if same else (Q.grad.numpy(), KV.grad.numpy())


def grad_bound(c, use_y, use_a, same, thr_fwd, thr_bwd):
    """the composed first-order bound of the module docstring -> (tol dQ, tol dKV) or their sum"""
    seg, cols, nr = c.seg, c.cols, c.n_rows
    ref = c.ref
    order = np.argsort(seg, kind="stable")
    rel = forward_rel(c, ref, *plan_of(c.rowptr, order, ref, True))
    al = ref.alpha
    Q, KV, dY = np.abs(c.Q).astype(np.float64), np.abs(c.KV).astype(np.float64), np.abs(c.dY).astype(np.float64)
    g = np.zeros(c.ne)
    dg = np.zeros(c.ne)
    if use_y:
        g = (c.dY.astype(np.float64)[seg] * c.KV.astype(np.float64)[cols]).sum(1)
        dg = gamma(8) * (dY[seg] * KV[cols]).sum(1)
    if use_a:
        g = g + c.dA
        dg = dg + U * np.abs(g)
    mag = np.bincount(seg, weights=al * np.abs(g), minlength=nr)
    dot = np.bincount(seg, weights=al * g, minlength=nr)
    ds = al * (g - dot[seg])
    ns = softmax_plan_n(c.lens, True)[seg] + 2
    dds = (gamma(ns) * al * (np.abs(g) + mag[seg])                                           # the softmax backward's own
           + al * (dg + np.bincount(seg, weights=al * dg, minlength=nr)[seg])               # g's error
           + al * rel * np.abs(g - dot[seg]) + al * np.bincount(seg, weights=al * rel * np.abs(g), minlength=nr)[seg])   # alpha's
    dep_f = plan_depth(c.lens, thr_fwd) + 3
    dep_b = plan_depth(np.bincount(cols, minlength=c.n_kv), thr_bwd) + 3
    tq = gamma(dep_f)[:, None] * _rows_sum(np.abs(ds), seg, cols, nr, KV) + _rows_sum(dds, seg, cols, nr, KV)
    tk = gamma(dep_b)[:, None] * _rows_sum(np.abs(ds), cols, seg, c.n_kv, Q) + _rows_sum(dds, cols, seg, c.n_kv, Q)
    if use_y:
        tk = tk + gamma(dep_b)[:, None] * _rows_sum(al, cols, seg, c.n_kv, dY) + _rows_sum(al * rel, cols, seg, c.n_kv, dY)
    floor = 2.0 ** -120                                               # gradual underflow of a few thousand terms
    slack = 1.0 + 2.0 ** -10
    return (slack * (tq + tk) + floor,) if same else (slack * tq + floor, slack * tk + floor)


@pytest.mark.gpu
@pytest.mark.parametrize("same", [False, True], ids=["distinct", "Q_is_KV"])
@pytest.mark.parametrize("use", ["Y", "alpha", "both"])
def test_gradients_through_hip_ops_vs_float64(same, use):
    from mmrec_amd import hip_ops
    c = _grad_case(int(same))
    use_y, use_a = use in ("Y", "both"), use in ("alpha", "both")
    dyn = _wrapper_graph(c)
    Q = _on(c.Q).requires_grad_()
    KV = Q if same else _on(c.KV).requires_grad_()
    assert hip_ops.edge_attention_served(Q, KV, dyn)
    y, alpha = hip_ops.edge_attention(Q, KV, dyn, eps=c.eps)
    out = 0.0
    if use_y:
        out = out + (y * _on(c.dY)).sum()
    if use_a:
        out = out + (alpha * _on(c.dA)).sum()
    out.backward()
    torch.cuda.synchronize()
    got = (Q.grad,) if same else (Q.grad, KV.grad)
    want = grads64(c, use_y, use_a, same)
    tol = grad_bound(c, use_y, use_a, same, dyn.fwd.long_row_threshold, dyn.bwd.long_row_threshold)
    worst = 0.0
    for nm, a, b, t in zip(("dQ", "dKV"), got, want, tol):
        a = a.cpu().double().numpy()
        assert np.isfinite(a).all() and float(np.abs(b).max()) > 0
        err = np.abs(a - b)
        assert (err <= t).all(), (nm, use, same, int((err > t).sum()), float((err / t).max()))
        assert float(np.median(t[np.abs(b) > 0] / np.abs(b)[np.abs(b) > 0])) < 1e-3, nm      # the bound is not vacuous
        worst = max(worst, float((err / t).max()))
    print("edge_attention gradients %s %s: worst err / bound %.3f" % ("Q is KV" if same else "distinct", use, worst))
    # needs_input_grad: a table that asks for no gradient gets none
    if not same:
        Q2, KV2 = _on(c.Q).requires_grad_(), _on(c.KV)
        y2, _ = hip_ops.edge_attention(Q2, KV2, dyn, eps=c.eps)
        (y2 * _on(c.dY)).sum().backward()
        assert KV2.grad is None and torch.equal(y2, y)
        if use == "Y":
            assert torch.equal(Q2.grad, Q.grad)


@pytest.mark.gpu
def test_switch_off_takes_the_three_ops(monkeypatch):
    from mmrec_amd import _lib, hip_ops
    c = _grad_case(0)
    dyn = _wrapper_graph(c)
    lib = _lib.load()
    calls = []
    for fn in ("mmrec_edge_attention_f32", "mmrec_edge_dot_f32", "mmrec_segment_softmax_f32"):
        monkeypatch.setattr(lib, fn, lambda *a, _real=getattr(lib, fn), _fn=fn: calls.append(_fn) or _real(*a))
    Q, KV = _on(c.Q), _on(c.KV)
    y_on, a_on = hip_ops.edge_attention(Q, KV, dyn)
    assert calls == ["mmrec_edge_attention_f32"]
    monkeypatch.setattr(hip_ops, "EDGE_ATTENTION", False)
    assert not hip_ops.edge_attention_served(Q, KV, dyn)
    y_off, a_off = hip_ops.edge_attention(Q, KV, dyn)
    assert calls == ["mmrec_edge_attention_f32", "mmrec_edge_dot_f32", "mmrec_segment_softmax_f32"]
    want_a = hip_ops.edge_softmax(hip_ops.edge_dot(Q, KV, dyn.rows, dyn.cols, dyn=dyn), dyn)
    assert torch.equal(a_off, want_a) and torch.equal(y_off, hip_ops.spmm_vals(dyn, KV, want_a))       # today's bits
    np.testing.assert_allclose(a_on.cpu().numpy(), a_off.cpu().numpy(), rtol=1e-4, atol=1e-7)
    np.testing.assert_allclose(y_on.cpu().numpy(), y_off.cpu().numpy(), rtol=1e-4, atol=1e-6)
