"""GPU: seeded differential fuzz of the segment softmax over a graph's edges (csrc/edge_softmax.hip, mmrec_segment_softmax_f32 /
_bwd_f32, hip_ops.edge_softmax) against float64 numpy of the two formulas as written here (`softmax64`, `softmax_bwd64`), never
against another form of the kernel.  The raw C ABI is called over guarded outputs.

The kernels' plan.  Lanes stride over a row's entries, each adds its own entries in one chain, then the lanes are reduced:
  group  16 lanes per row: a term meets at most ceil(len / 16) roundings in its lane's chain and 4 in the butterfly:
         n = ceil(len / 16) + 4.  Serves rows of <= group_max entries, and EVERY row when the call has no long-row list.
  block  one 256-thread workgroup per listed row: ceil(len / 256) in the chain, 6 in the wave butterfly, 2 over the four wave
         partials: n = ceil(len / 256) + 8.
(`plan_n`).  Two acceptance modes; each case uses one.
  exact  in every row a power-of-two number k of entries share the maximum, a multiple of 1/8; all others are -inf.  The
         output must EQUAL 1/k and 0 (k + 1e-16 is k in fp32).  Backward: alpha = 2^-j, j <= 4, g a multiple of 1/8 of magnitude
         <= 1: every product is a multiple of 2^-7, every partial sum stays below 2^16 (rows of <= 40,000 entries), g - sum and
         its product with 2^-j are exact: ds must EQUAL float64.  A lost entry, a wrong segment or a wrong perm cannot hide.
  float  normal scores, standard deviation 0.1 ... 30 per row, rows shifted by +-100, some -inf entries; eps 1e-16, 1e-3, 0.5.
         Forward, per element:  |got - ref| <= ref * rel + 4 * 2^-126,
             rel = u (|x_e| + E) + sum_q e_q u (|x_q| + E) / den + gamma(n) + 4 u,     x = s - m, e = exp(x), u = 2^-24:
         u |x| is the rounding of s - m seen through exp, E u the error of the device's exp (E = 4 x the worst error of fp32 exp
         against float64 MEASURED ON THE CPU over these cases' own arguments, `test_E_is_four_times_the_measured_worst`), the
         sum is the same two errors carried into the denominator, gamma(n) its summation, 4 u the addition of eps, the division
         and two to spare; 4 * 2^-126 covers results at and below the smallest normal number.
         Backward, per element: |got - ref| <= gamma(n + 2) alpha_e (|g_e| + sum_q alpha_q |g_q|) + (n + 2) 2^-149  (n for the
         sum, 2 for the subtraction and the product; the last term is gradual underflow).
Non-finite: a row that holds a NaN, a +inf or nothing but -inf is NaN in every entry, every other row is unaffected, a -inf next
to a finite maximum is exactly 0 -- which is what the float64 formulas give, so the checker asks for float64's NaN pattern.

`test_E_...`, `test_bound_is_sharp`, `test_torch_composition_passes_the_checker`, `test_checker_rejects_planted_errors` and
`test_cases_span_every_axis` need no GPU."""
import ctypes
import os

import numpy as np
import pytest
import torch

from tests.test_spmm_fuzz_gpu import U, _on, gamma

CASES = 28
LAYOUTS = ("lens", "hub3000", "hub40000", "one_row", "tiny", "many", "runs")
EPS = (1e-16, 1e-3, 0.5)
E_EXP = 14.0                                  # test_E_is_four_times_the_measured_worst
TINY = 4 * 2.0 ** -126
SENTINEL = 0x7FC12345                          # a NaN no arithmetic produces: "never written"
GUARD = 64


def group_max():
    from mmrec_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        from mmrec_amd.build import build
        build(verbose=False)
    return int(_lib.load().mmrec_segment_softmax_group_max())


def axis_lens():
    gm = group_max()
    return (0, 1, 2, 15, 16, 17, 63, 64, 65, gm - 1, gm, gm + 1, 1025)


def plan_n(lens, with_list):
    """per row: the roundings a term of the row's sum meets (module docstring)"""
    lens = np.asarray(lens, np.int64)
    grp, blk = -(-lens // 16) + 4, -(-lens // 256) + 8
    return np.where((lens > group_max()) & with_list, blk, grp)


# ------------------------------------------------------------------------------------------------ host references
def softmax64(score, seg, n_rows, eps, *, drop=None, no_max=False, eps_each=False):
    """float64 of  out[e] = exp(s[e] - m) / (sum_q exp(s[q] - m) + eps)  over the edges sharing seg[e]; -> (out, x, e, den).
    The keywords plant errors (test_checker_rejects_planted_errors): `drop` an edge left out of its row's sum, `no_max` the
    maximum not subtracted -- in fp32's range, as a kernel would --, `eps_each` eps added once per entry."""
    s = np.asarray(score, np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        m = np.full(n_rows, -np.inf)
        np.maximum.at(m, seg, s)
        x = s - (0.0 if no_max else m[seg])
        e = np.exp(x)
        if no_max:
            e = e.astype(np.float32).astype(np.float64)
        w = e.copy()
        if drop is not None:
            w[drop] = 0.0
        den = np.bincount(seg, weights=w, minlength=n_rows)
        den = den + float(np.float32(eps)) * (np.bincount(seg, minlength=n_rows) if eps_each else 1.0)
        out = e / den[seg]
    return out, x, e, den


def softmax_bwd64(alpha, g, seg, n_rows):
    """float64 of  ds[e] = alpha[e] (g[e] - sum_q alpha[q] g[q]); -> (ds, M) with M = alpha_e (|g_e| + sum_q alpha_q |g_q|)"""
    a, g = np.asarray(alpha, np.float64), np.asarray(g, np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        dot = np.bincount(seg, weights=a * g, minlength=n_rows)
        mag = np.bincount(seg, weights=np.abs(a * g), minlength=n_rows)
        return a * (g - dot[seg]), np.abs(a) * (np.abs(g) + mag[seg])


def forward_rel(c, n):
    """the float mode's relative bound per element (module docstring); n per row"""
    out, x, e, den = softmax64(c.score, c.seg, c.n_rows, c.eps)
    with np.errstate(invalid="ignore", over="ignore"):
        t = np.where(e > 0, e * U * (np.abs(x) + E_EXP), 0.0)
        carried = np.bincount(c.seg, weights=t, minlength=c.n_rows) / den
        rel = np.where(e > 0, U * (np.abs(x) + E_EXP), 0.0) + carried[c.seg] + gamma(n)[c.seg] + 4 * U
    return out, rel


def _arr(got):
    return got.detach().cpu().double().numpy() if isinstance(got, torch.Tensor) else np.asarray(got, np.float64)


def check_fwd(got, c, n, name=""):
    """got [n_edges] against float64 in the case's mode; returns the float mode's worst err / bound"""
    g = _arr(got)
    assert g.shape == (c.ne,), (name, g.shape)
    if c.exact:
        bad = g != c.expect
        assert not bad.any(), (name, "exact mismatch", int(bad.sum()), "first at", int(np.argmax(bad)),
                               float(g[np.argmax(bad)]), float(c.expect[np.argmax(bad)]))
        return 0.0
    ref, rel = forward_rel(c, n)
    nan = np.isnan(ref)
    assert np.isfinite(ref[~nan]).all()
    assert np.array_equal(np.isnan(g), nan), (name, "NaN pattern", int((np.isnan(g) != nan).sum()))
    with np.errstate(invalid="ignore"):
        err, tol = np.where(nan, 0.0, np.abs(g - ref)), np.where(nan, 1.0, ref * rel + TINY)
    viol = err > tol
    assert not viol.any(), (name, "beyond the bound", int(viol.sum()), "first at", int(np.argmax(viol)),
                            float(g[np.argmax(viol)]), float(ref[np.argmax(viol)]), float(rel[np.argmax(viol)]))
    return float((err / tol).max(initial=0.0))


def check_bwd(got, alpha, g, c, n, name=""):
    """ds [n_edges] against float64 of the backward formula on the fp32 alpha and g given; worst err / bound in float mode"""
    d = _arr(got)
    assert d.shape == (c.ne,), (name, d.shape)
    ref, M = softmax_bwd64(alpha, g, c.seg, c.n_rows)
    nan = np.isnan(ref)
    assert np.array_equal(np.isnan(d), nan), (name, "NaN pattern", int((np.isnan(d) != nan).sum()))
    if c.exact:
        bad = ~nan & (d != ref)
        assert not bad.any(), (name, "exact mismatch", int(bad.sum()), "first at", int(np.argmax(bad)),
                               float(d[np.argmax(bad)]), float(ref[np.argmax(bad)]))
        return 0.0
    nn = n[c.seg] + 2
    with np.errstate(invalid="ignore"):
        err, tol = np.where(nan, 0.0, np.abs(d - ref)), np.where(nan, 1.0, gamma(nn) * M + nn * 2.0 ** -149)
    viol = err > tol
    assert not viol.any(), (name, "beyond the bound", int(viol.sum()), "first at", int(np.argmax(viol)),
                            float(d[np.argmax(viol)]), float(ref[np.argmax(viol)]), float(tol[np.argmax(viol)]))
    return float((err / tol).max(initial=0.0))


# ------------------------------------------------------------------------------------------------ cases
class Case:
    pass


def _row_lens(layout, rng, k):
    al = axis_lens()
    small = lambda n: rng.integers(0, 40, n)
    if layout == "lens":                                              # every length of the axis, empty rows first and last
        return np.concatenate([[0, 0], rng.permutation(al), [0]])
    if layout == "hub3000":
        return np.concatenate([small(30), [3000], small(30)])
    if layout == "hub40000":
        return np.concatenate([small(20), [40000], small(20), [group_max() + 1]])
    if layout == "one_row":
        return np.array([al[1:][k % (len(al) - 1)]])
    if layout == "tiny":                                              # n_edges 0 and 1
        return np.array([0, 0, 0]) if k % 2 == 0 else np.array([0, 1, 0, 0])
    if layout == "many":                                              # several workgroups of short rows, a few long ones
        lens = rng.geometric(0.08, 3000) - 1
        lens[rng.integers(0, 3000, 5)] = group_max() + rng.integers(1, 400, 5)
        return lens
    lens = small(200)                                                 # "runs": runs of empty rows between the others
    for a in rng.integers(0, 190, 8):
        lens[a:a + int(rng.integers(2, 10))] = 0
    lens[0], lens[-1], lens[100] = 0, 0, group_max() + 1
    return lens


def draw_case(seed):
    rng = np.random.default_rng(7300 + seed)
    c = Case()
    c.seed = seed
    c.layout = LAYOUTS[seed % len(LAYOUTS)]
    c.exact = (seed // len(LAYOUTS)) % 2 == 0
    c.shuffled = (seed // (2 * len(LAYOUTS))) % 2 == 1                # perm: NULL (CSR order) or a shuffled COO order
    c.eps = 1e-16 if c.exact else EPS[seed % len(EPS)]
    lens = np.asarray(_row_lens(c.layout, rng, seed // len(LAYOUTS)), np.int64)
    c.lens, c.n_rows, c.ne = lens, lens.size, int(lens.sum())
    c.rowptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    rid = np.repeat(np.arange(c.n_rows), lens)                        # row of CSR slot j
    if c.shuffled:                                                    # slot j lives at COO position perm[j]
        c.perm = rng.permutation(c.ne).astype(np.int64)
        c.seg = np.empty(c.ne, np.int64)
        c.seg[c.perm] = rid
    else:
        c.perm, c.seg = None, rid
    ne = c.ne
    if c.exact:
        score = np.full(ne, -np.inf, np.float32)
        c.expect = np.zeros(ne)
        for r in np.flatnonzero(lens):
            where = c.perm[c.rowptr[r]:c.rowptr[r + 1]] if c.shuffled else np.arange(c.rowptr[r], c.rowptr[r + 1])
            k = 1 << int(rng.integers(0, int(np.log2(where.size)) + 1))
            top = rng.choice(where, size=k, replace=False)
            score[top] = rng.integers(-32, 33) / 8.0
            c.expect[top] = 1.0 / k
        c.score = score
        c.alpha = (2.0 ** -rng.integers(0, 5, ne)).astype(np.float32)
        c.g = (rng.integers(-8, 9, ne) / 8.0).astype(np.float32)
    else:
        std = rng.choice([0.1, 1.0, 5.0, 30.0], c.n_rows)
        shift = rng.choice([0.0, 100.0, -100.0], c.n_rows)
        score = rng.standard_normal(ne) * std[c.seg] + shift[c.seg]
        score[rng.random(ne) < 0.03] = -np.inf
        c.score = score.astype(np.float32)
        ref = softmax64(c.score, c.seg, c.n_rows, c.eps)[0]
        c.alpha = np.where(np.isnan(ref), 0.5, ref).astype(np.float32)     # (a row of nothing but -inf: any alpha will do)
        g = rng.standard_normal(ne)
        g[rng.random(ne) < 0.05] = 0.0
        c.g = g.astype(np.float32)
    return c


_CASES = {}


def case(seed):
    """the cases are drawn once and shared; nothing changes them"""
    if seed not in _CASES:
        _CASES[seed] = draw_case(seed)
    return _CASES[seed]


def float_cases():
    return [case(s) for s in range(CASES) if not case(s).exact]


# ------------------------------------------------------------------------------------------------ CPU: the checker and the cases
def _torch_composition(c):
    from mmrec_amd import hip_ops
    return hip_ops.segment_softmax_torch(torch.from_numpy(c.score), torch.from_numpy(c.seg), c.n_rows, c.eps).numpy()


def test_draw_case_is_deterministic():
    a, b = draw_case(8), draw_case(8)
    assert np.array_equal(a.score, b.score, equal_nan=True) and np.array_equal(a.seg, b.seg) and np.array_equal(a.g, b.g)


def test_cases_span_every_axis():
    gm = group_max()
    seen = {k: set() for k in ("lens", "combo", "eps", "hub", "tiny", "one_row")}
    for s in range(CASES):
        c = case(s)
        seen["lens"].update(int(x) for x in c.lens)
        seen["combo"].add((c.layout, c.exact, c.shuffled))
        if not c.exact:
            seen["eps"].add(c.eps)
        if c.lens.max(initial=0) >= 3000:
            seen["hub"].add((int(c.lens.max()), c.exact, c.shuffled))
        if c.layout == "tiny":
            seen["tiny"].add(c.ne)
        if c.n_rows == 1:
            seen["one_row"].add(c.ne)
        assert c.seg.size == c.ne and c.rowptr[-1] == c.ne and np.array_equal(np.bincount(c.seg, minlength=c.n_rows), c.lens)
        if c.shuffled and c.ne > 50:
            assert (np.diff(c.seg) < 0).any()                         # the COO order is not the CSR order
        if c.exact:                                                   # the construction IS the formula, rounded to fp32
            ref = softmax64(c.score, c.seg, c.n_rows, c.eps)[0]
            assert np.array_equal(ref.astype(np.float32).astype(np.float64), c.expect)
            assert np.array_equal(_torch_composition(c).astype(np.float64), c.expect)        # and the composition equals it
    assert set(axis_lens()) | {3000, 40000} <= seen["lens"], sorted(seen["lens"])
    assert seen["combo"] == {(l, e, p) for l in LAYOUTS for e in (True, False) for p in (True, False)}
    assert seen["eps"] == set(EPS) and seen["tiny"] == {0, 1} and len(seen["one_row"]) >= 4
    assert {(h, e, p) for h in (3000, 40000) for e in (True, False) for p in (True, False)} <= seen["hub"]
    c = case(0)                                                       # empty rows first, last and in runs
    assert c.lens[0] == 0 and c.lens[-1] == 0 and c.lens[1] == 0
    r = case(LAYOUTS.index("runs")).lens
    assert r[0] == 0 and r[-1] == 0 and ((r[:-1] == 0) & (r[1:] == 0)).sum() >= 8 and r.max() == gm + 1


def measure_E():
    """worst error of fp32 exp (numpy, on the CPU) against float64, in units of u |value|, over the arguments s - m of every
    float case whose result is a normal number"""
    worst = 0.0
    for c in float_cases():
        if not c.ne:
            continue
        m = np.full(c.n_rows, -np.inf, np.float32)
        np.maximum.at(m, c.seg, c.score)
        with np.errstate(invalid="ignore"):
            x = (c.score - m[c.seg]).astype(np.float32)
        x = x[np.isfinite(x) & (x > -87.0)]
        a, b = np.exp(x).astype(np.float64), np.exp(x.astype(np.float64))
        worst = max(worst, float((np.abs(a - b) / (U * b)).max(initial=0.0)))
    return worst


def test_E_is_four_times_the_measured_worst():
    worst = measure_E()
    print("fp32 exp against float64, worst error in units of u |value|: %.3f" % worst)
    assert 4.0 * worst <= E_EXP and (E_EXP == 4.0 or E_EXP <= 8.0 * worst), (worst, E_EXP)


def test_bound_is_sharp():
    """at least 90 % of the outputs above 1e-30 have a relative bound <= 1e-4 (the plan with the long-row list: the one the
    wrapper runs); scores have a standard deviation of at most 30"""
    n_all = n_sharp = 0
    for c in float_cases():
        if not c.ne:
            continue
        ref, rel = forward_rel(c, plan_n(c.lens, True))
        big = ~np.isnan(ref) & (ref > 1e-30)
        n_all += int(big.sum())
        n_sharp += int((rel[big] <= 1e-4).sum())
    print("outputs above 1e-30: %d, with rel <= 1e-4: %d (%.1f %%)" % (n_all, n_sharp, 100.0 * n_sharp / n_all))
    assert n_all > 50000 and n_sharp >= 0.9 * n_all


def test_torch_composition_passes_the_checker():
    """the fp32 torch composition (serial index_add_: n = the row's entry count) on every float case whose longest row is at
    most 1,024 entries"""
    ran, worst = 0, 0.0
    for c in float_cases():
        if c.lens.max(initial=0) > 1024:
            continue
        worst = max(worst, check_fwd(_torch_composition(c), c, c.lens, name="torch composition seed %d" % c.seed))
        ran += 1
    print("torch composition: %d cases, worst err / bound %.3f" % (ran, worst))
    assert ran >= 4


def test_checker_rejects_planted_errors():
    c = next(c for c in float_cases() if c.layout == "many" and c.shuffled and c.eps >= 1e-3)
    n = plan_n(c.lens, True)
    clean, x, e, den = softmax64(c.score, c.seg, c.n_rows, c.eps)
    assert check_fwd(clean.astype(np.float32), c, n, "clean") <= 1.0
    rows = [r for r in np.flatnonzero(c.lens >= 20) if np.isfinite(den[r])]
    # one entry dropped from a sum (one that carries a thousandth of it or more)
    q = next(q for q in np.flatnonzero(c.seg == rows[0]) if e[q] >= 1e-3 * den[rows[0]])
    bad = softmax64(c.score, c.seg, c.n_rows, c.eps, drop=q)[0]
    with pytest.raises(AssertionError):
        check_fwd(bad.astype(np.float32), c, n)
    # one entry sent to the neighbouring row
    seg2 = c.seg.copy()
    seg2[q] = rows[0] + 1 if rows[0] + 1 < c.n_rows else rows[0] - 1
    bad = softmax64(c.score, seg2, c.n_rows, c.eps)[0]
    with pytest.raises(AssertionError):
        check_fwd(bad.astype(np.float32), c, n)
    # the maximum not subtracted, on a row whose scores exceed 89: fp32 exp overflows
    r = next(r for r in rows if c.score[c.seg == r].max() > 89)
    bad = softmax64(c.score, c.seg, c.n_rows, c.eps, no_max=True)[0]
    assert not np.isfinite(bad[c.seg == r]).all()
    with pytest.raises(AssertionError):
        check_fwd(bad.astype(np.float32), c, n)
    # perm ignored: CSR slot j taken for COO position j
    bad = softmax64(c.score, np.sort(c.seg), c.n_rows, c.eps)[0]
    with pytest.raises(AssertionError):
        check_fwd(bad.astype(np.float32), c, n)
    # eps added per entry
    bad = softmax64(c.score, c.seg, c.n_rows, c.eps, eps_each=True)[0]
    with pytest.raises(AssertionError):
        check_fwd(bad.astype(np.float32), c, n)
    # backward: clean passes, an entry dropped from the sum or a sum of the neighbouring row does not
    ds, M = softmax_bwd64(c.alpha, c.g, c.seg, c.n_rows)
    assert check_bwd(ds.astype(np.float32), c.alpha, c.g, c, n, "clean bwd") <= 1.0
    q = next(q for q in np.flatnonzero(c.seg == rows[0]) if abs(c.alpha[q] * c.g[q]) >= 1e-3)
    g2 = c.g.copy()
    g2[q] = 0.0
    bad = softmax_bwd64(c.alpha, g2, c.seg, c.n_rows)[0]
    bad[q] = ds[q]
    with pytest.raises(AssertionError):
        check_bwd(bad.astype(np.float32), c.alpha, c.g, c, n)
    with pytest.raises(AssertionError):
        check_bwd(softmax_bwd64(c.alpha, c.g, seg2, c.n_rows)[0].astype(np.float32), c.alpha, c.g, c, n)
    # exact mode: one entry moved to the neighbouring row, and perm ignored
    c = next(case(s) for s in range(CASES) if case(s).exact and case(s).layout == "lens" and case(s).shuffled)
    assert check_fwd(c.expect.astype(np.float32), c, None, "clean exact") == 0.0
    r = int(np.flatnonzero(c.lens >= 16)[0])
    q = int(np.flatnonzero((c.seg == r) & (c.expect > 0))[0])
    seg2 = c.seg.copy()
    seg2[q] = r - 1
    with pytest.raises(AssertionError):
        check_fwd(softmax64(c.score, seg2, c.n_rows, c.eps)[0].astype(np.float32), c, None)
    with pytest.raises(AssertionError):
        check_fwd(softmax64(c.score, np.sort(c.seg), c.n_rows, c.eps)[0].astype(np.float32), c, None)


# ------------------------------------------------------------------------------------------------ GPU: the raw C ABI, guarded
class _Dev:
    """a case's arrays on the device + the long-row list the wrapper would build"""

    def __init__(self, c):
        from mmrec_amd import hip_ops
        self.rowptr = _on(c.rowptr)
        self.perm = None if c.perm is None else _on(c.perm)
        lr = hip_ops.segment_long_rows(c.rowptr)
        self.long_rows, self.n_long = (_on(lr), lr.size) if lr.size else (None, 0)


def _guarded(ne):
    buf = torch.full((ne + 2 * GUARD,), SENTINEL, dtype=torch.int32, device="cuda:0")
    return buf, buf[GUARD:GUARD + ne].view(torch.float32)


def _guards_ok(buf, ne, name):
    b = buf.cpu().numpy()
    assert (b[:GUARD] == SENTINEL).all() and (b[GUARD + ne:] == SENTINEL).all(), (name, "wrote outside the output")
    assert not (b[GUARD:GUARD + ne] == SENTINEL).any(), (name, "entries never written", int((b[GUARD:GUARD + ne] == SENTINEL).sum()))


def raw_fwd(c, dev, score, with_list, name="fwd"):
    from mmrec_amd import hip_ops
    p, lib = hip_ops._p, hip_ops._lib.load()
    buf, out = _guarded(c.ne)
    rc = lib.mmrec_segment_softmax_f32(p(dev.rowptr), c.n_rows, p(dev.perm), p(dev.long_rows) if with_list else None,
                                       dev.n_long if with_list else 0, p(score) if c.ne else None, c.ne, c.eps,
                                       ctypes.c_void_p(out.data_ptr()) if c.ne else None, hip_ops._stream())
    assert rc == 0, (name, rc)
    torch.cuda.synchronize()
    _guards_ok(buf, c.ne, name)
    return out


def raw_bwd(c, dev, alpha, g, with_list, name="bwd"):
    from mmrec_amd import hip_ops
    p, lib = hip_ops._p, hip_ops._lib.load()
    buf, ds = _guarded(c.ne)
    rc = lib.mmrec_segment_softmax_bwd_f32(p(dev.rowptr), c.n_rows, p(dev.perm), p(dev.long_rows) if with_list else None,
                                           dev.n_long if with_list else 0, p(alpha) if c.ne else None,
                                           p(g) if c.ne else None, c.ne, ctypes.c_void_p(ds.data_ptr()) if c.ne else None,
                                           hip_ops._stream())
    assert rc == 0, (name, rc)
    torch.cuda.synchronize()
    _guards_ok(buf, c.ne, name)
    return ds


def _wrapper_graph(c, by, rng):
    """a DynGraph whose `by` side is the case's segments (the other side: random ids)"""
    from mmrec_amd import hip_ops
    other_n = 37
    other = _on(rng.integers(0, other_n, c.ne).astype(np.int64))
    seg = _on(c.seg.astype(np.int64))
    if by == "row":
        return hip_ops.DynGraph(seg, other, c.n_rows, other_n)
    return hip_ops.DynGraph(other, seg, other_n, c.n_rows)


@pytest.mark.gpu
@pytest.mark.parametrize("seed", range(CASES))
def test_edge_softmax_fuzz(seed):
    from mmrec_amd import hip_ops
    c = case(seed)
    dev = _Dev(c)
    score, alpha, g = _on(c.score), _on(c.alpha), _on(c.g)
    assert (dev.n_long > 0) == bool((c.lens > group_max()).any())
    worst = 0.0
    for with_list in (True, False):                                   # the same graph with the list and with n_long = 0
        n = plan_n(c.lens, with_list)
        tag = "seed %d %s" % (seed, "list" if with_list else "n_long = 0")
        out = raw_fwd(c, dev, score, with_list, "fwd " + tag)
        worst = max(worst, check_fwd(out, c, n, "fwd " + tag))
        ds = raw_bwd(c, dev, alpha, g, with_list, "bwd " + tag)
        worst = max(worst, check_bwd(ds, c.alpha, c.g, c, n, "bwd " + tag))
    if c.ne:                                                          # through the wrapper, segments on either side
        rng = np.random.default_rng(seed)
        for by in ("row", "col"):
            dyn = _wrapper_graph(c, by, rng)
            s = _on(c.score).requires_grad_()
            assert hip_ops.edge_softmax_served(s, dyn)
            out = hip_ops.edge_softmax(s, dyn, by=by, eps=c.eps)
            n = plan_n(c.lens, True)
            worst = max(worst, check_fwd(out, c, n, "wrapper %s seed %d" % (by, seed)))
            out.backward(g)
            torch.cuda.synchronize()
            # the wrapper's backward reads ITS forward: float64 of the formula on that alpha.  Exact mode: alpha is 1/k >= 2^-15
            # and sums to 1 per row, so the products (multiples of 2^-18) and every partial sum (<= 1) are still exact
            worst = max(worst, check_bwd(s.grad, out.detach().cpu().numpy(), c.g, c, n, "wrapper bwd %s seed %d" % (by, seed)))
    print("edge_softmax fuzz seed %d: %s %s %s rows %d edges %d longest %d eps %g worst err / bound %.3f" % (
        seed, c.layout, "exact" if c.exact else "float", "shuffled" if c.shuffled else "csr order", c.n_rows, c.ne,
        int(c.lens.max(initial=0)), c.eps, worst))


# ------------------------------------------------------------------------------------------------ GPU: targeted tests
def _nonfinite_case():
    """the rule's rows -- [0, 1 | -inf, -inf | inf, 2 | nan, 3 | 1, -200] -- and their like in every kind of row: the NaN / inf
    in a lane's registers and beyond them, in a group row, a long row and a hub; finite rows in between"""
    gm = group_max()
    rng = np.random.default_rng(99)
    inf, nan = np.inf, np.nan
    rows = [[0, 1], [-inf, -inf], [inf, 2], [nan, 3], [1, -200], [nan], [-inf], [inf], [3.5]]

    def normal(n):
        return list(rng.standard_normal(n) * 3)
    for n, at, v in ((17, 16, nan), (100, 70, inf), (100, 3, -inf), (gm, gm - 1, nan), (gm + 1, gm, nan), (gm + 1, 5, inf),
                     (gm + 40, 100, -inf), (3000, 2999, nan), (3000, 1500, inf), (1500, 7, -inf), (300, None, -inf),
                     (64, None, -inf), (2000, None, None), (30, None, None)):
        r = normal(n)                                                 # v None: a finite row
        if v is not None and at is None:
            r = [v] * n                                               # nothing but -inf
        elif v is not None:
            r[at] = v
        rows.append(r)
    c = Case()
    c.exact, c.eps, c.seed = False, 1e-16, -1
    c.lens = np.array([len(r) for r in rows], np.int64)
    c.n_rows, c.ne = c.lens.size, int(c.lens.sum())
    c.rowptr = np.concatenate([[0], np.cumsum(c.lens)]).astype(np.int32)
    rid = np.repeat(np.arange(c.n_rows), c.lens)
    c.perm = rng.permutation(c.ne).astype(np.int64)
    c.seg = np.empty(c.ne, np.int64)
    c.seg[c.perm] = rid
    c.score = np.empty(c.ne, np.float32)
    c.score[c.perm] = np.concatenate(rows).astype(np.float32)
    c.g = rng.standard_normal(c.ne).astype(np.float32)
    return c


def test_nonfinite_case_follows_the_rule_in_float64():
    """(CPU) the float64 formulas give exactly the rule the checker then asks of the kernel"""
    c = _nonfinite_case()
    ref = softmax64(c.score, c.seg, c.n_rows, c.eps)[0]
    with np.errstate(invalid="ignore"):
        for r in range(c.n_rows):
            s, o = c.score[c.seg == r], ref[c.seg == r]
            poisoned = np.isnan(s).any() or (s == np.inf).any() or (s == -np.inf).all()
            assert np.isnan(o).all() if poisoned else np.isfinite(o).all(), r
            if not poisoned:
                assert (o[s == -np.inf] == 0).all() and abs(o.sum() - 1) < 1e-12
    first = ref[c.perm[:10]]                                          # the rule's own five rows (fp32 rounds exp(-201) to 0)
    assert np.isfinite(first[:2]).all() and np.isnan(first[2:8]).all() and first[8] == 1.0 and 0 < first[9] < 1e-80
    assert int(np.isnan(ref).sum()) > 4000 and int((ref == 0).sum()) >= 3


@pytest.mark.gpu
def test_non_finite_rows_value_for_value():
    c = _nonfinite_case()
    dev = _Dev(c)
    assert dev.n_long >= 6
    score, g = _on(c.score), _on(c.g)
    for with_list in (True, False):
        n = plan_n(c.lens, with_list)
        out = raw_fwd(c, dev, score, with_list, "non-finite fwd")
        check_fwd(out, c, n, "non-finite fwd list %s" % with_list)
        o = out.cpu().numpy()
        assert (o[c.score == -np.inf][~np.isnan(o[c.score == -np.inf])] == 0).all()       # -inf next to a finite maximum: exactly 0
        ds = raw_bwd(c, dev, out.clone(), g, with_list, "non-finite bwd")                 # the forward's alpha, NaN rows and all
        check_bwd(ds, o, c.g, c, n, "non-finite bwd list %s" % with_list)
        d = ds.cpu().numpy()
        assert np.array_equal(np.isnan(d), np.isnan(o)) and (d[o == 0] == 0).all()


@pytest.mark.gpu
def test_hub_repeats_bit_for_bit():
    """forward and backward on the 40,000-entry hub case, run twice: the same bits (and through the wrapper)"""
    from mmrec_amd import hip_ops
    c = next(case(s) for s in range(CASES) if case(s).layout == "hub40000" and not case(s).exact and case(s).shuffled)
    dev = _Dev(c)
    score, g = _on(c.score), _on(c.g)
    for with_list in (True, False):
        outs = [raw_fwd(c, dev, score, with_list) for _ in range(2)]
        assert torch.equal(outs[0].view(torch.int32), outs[1].view(torch.int32)), with_list
        dss = [raw_bwd(c, dev, outs[0], g, with_list) for _ in range(2)]
        assert torch.equal(dss[0].view(torch.int32), dss[1].view(torch.int32)), with_list
    dyn = _wrapper_graph(c, "row", np.random.default_rng(0))
    runs = []
    for _ in range(2):
        s = _on(c.score).requires_grad_()
        out = hip_ops.edge_softmax(s, dyn)
        out.backward(g)
        torch.cuda.synchronize()
        runs.append((out.detach(), s.grad))
    for a, b in zip(*runs):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    assert float(runs[0][1].abs().max()) > 0


@pytest.mark.gpu
def test_forward_and_backward_are_capturable():
    """forward + backward recorded with torch.cuda.graph and replayed twice after the scores change: the eager bits"""
    from mmrec_amd import hip_ops
    c = next(case(s) for s in range(CASES) if case(s).layout == "many" and not case(s).exact and case(s).shuffled)
    dyn = _wrapper_graph(c, "row", np.random.default_rng(0))
    rng = np.random.default_rng(4)
    other = (rng.standard_normal(c.ne) * 4).astype(np.float32)
    g = _on(c.g)
    hip_ops.edge_softmax(_on(c.score), dyn)                           # (the long-row list is built outside the capture)
    torch.cuda.synchronize()

    def step(s):
        out = hip_ops.edge_softmax(s, dyn)
        (ds,) = torch.autograd.grad(out, s, g)
        return out, ds
    eager = []
    for sc in (c.score, other):
        out, ds = step(_on(sc).requires_grad_())
        eager.append((out.detach().clone(), ds.clone()))
    torch.cuda.synchronize()
    static_s = _on(c.score).requires_grad_()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        static = step(static_s)
    for sc, want in ((other, eager[1]), (c.score, eager[0]), (other, eager[1])):
        with torch.no_grad():
            static_s.copy_(_on(sc))
        for t in static:
            t.detach().zero_()
        graph.replay()
        graph.replay()
        torch.cuda.synchronize()
        for a, b in zip(want, static):
            assert torch.equal(a.view(torch.int32), b.detach().view(torch.int32))
    assert not torch.equal(eager[0][0], eager[1][0])


@pytest.mark.gpu
def test_switch_off_takes_the_composition(monkeypatch):
    from mmrec_amd import _lib, hip_ops
    c = next(case(s) for s in range(CASES) if case(s).layout == "runs" and not case(s).exact and case(s).shuffled)
    dyn = _wrapper_graph(c, "row", np.random.default_rng(0))
    lib = _lib.load()
    calls = []
    for fn in ("mmrec_segment_softmax_f32", "mmrec_segment_softmax_bwd_f32"):
        monkeypatch.setattr(lib, fn, lambda *a, _real=getattr(lib, fn), _fn=fn: calls.append(_fn) or _real(*a))
    g = _on(c.g)
    s_on = _on(c.score).requires_grad_()
    on = hip_ops.edge_softmax(s_on, dyn, eps=c.eps)
    on.backward(g)
    assert calls == ["mmrec_segment_softmax_f32", "mmrec_segment_softmax_bwd_f32"]
    monkeypatch.setattr(hip_ops, "EDGE_SOFTMAX", False)
    s_off = _on(c.score).requires_grad_()
    assert not hip_ops.edge_softmax_served(s_off, dyn)
    off = hip_ops.edge_softmax(s_off, dyn, eps=c.eps)
    off.backward(g)
    torch.cuda.synchronize()
    assert len(calls) == 2                                            # the library was not called again
    n = plan_n(c.lens, True)
    check_fwd(on, c, n, "switch on")
    check_fwd(off, c, c.lens, "switch off")                           # the composition: n = the row's entry count
    ok = ~np.isnan(on.detach().cpu().numpy())
    np.testing.assert_allclose(off.detach().cpu().numpy()[ok], on.detach().cpu().numpy()[ok], rtol=1e-4, atol=1e-30)
    np.testing.assert_allclose(s_off.grad.cpu().numpy()[ok], s_on.grad.cpu().numpy()[ok], rtol=1e-3, atol=1e-6)
