"""GPU: seeded differential fuzz of the SpMM family (csrc/spmm.hip, csrc/spmm_narrow.hip) against float64 results computed on
the host (scipy / torch CPU), never against another form of the same kernels: mmrec_spmm_csr_f32 at every width it is built
for (slices of 8 / 16 / 32 columns, DCH = 1 ... 6), in both row-per-group regimes (one row per 16-lane group up to 2^18 rows,
four above), over every kind of long-row plan (single- and multi-chunk rows, the last-arriver finish and the two-launch
finish), with every epilogue input; the listed-row pull and push kernels; the LayerGCN layer; and the autograd wrappers on
top (`spmm` with its width padding, `lightgcn_mean`, `layergcn_sum`, `spmm_vals`).

Two acceptance modes; each case uses one.
  exact  X, vals, Z, acc_in and upstream gradients are multiples of 1/16 (vals: 1/8) of magnitude <= 1, the coefficients
         alpha / beta / acc_scale / g_scale powers of two.  Every value any summation order can form is then a multiple of
         1 / GRID = 2^-9 below 2^14 in magnitude -- an exact fp32 number -- and the output must EQUAL the float64 result (as
         numbers: +0 == -0), whatever the row length, plan or order.  The generator asserts the grid on an upper bound of every
         intermediate, `check` again on the actual largest one (sum |terms| + |acc_in| + the epilogue's magnitude).  A dropped,
         doubled or misplaced nonzero, a wrong chunk boundary or a lost group of a 16-way tree cannot hide.  The push kernel's
         fp32 atomics are exact too.
  float  normal values, scaled rows and columns, exact zeros, explicit zero values in the CSR, an occasional inf / NaN row of
         X.  An element passes if |got - ref64| <= gamma(n) M + n 2^-149, M the same expression on absolute values
         (|alpha| sum |a_k x_k| + |beta Z|, + |acc_in|, times |acc_scale|), n the number of roundings a term meets on its way
         to the output under the kernels' plan (`plan_depth`: a short row's fma chain is its length; a long row's term meets
         <= 32 fmas in its group, 15 adds over the groups, ceil(chunks / 16) + 15 adds over the chunks) + 4 for the epilogue;
         gamma(n) = n u / (1 - n u), u = 2^-24: the bound of any fp32 evaluation of a sum of products in which no term meets
         more than n roundings (Higham, Accuracy and Stability of Numerical Algorithms, sec. 3.1; 2^-149 per rounding covers
         underflow).  Float cases keep sequential chains <= 1024 nonzeros (gamma < 6.2e-5: a 1e-4 relative error is caught
         everywhere); longer chains are exact cases.  Non-finite outputs must be float64's, value for value (NaN, +inf, -inf:
         with finite terms this small, which one a sum gives does not depend on the order).

`test_checker_rejects_planted_errors` and `test_cases_span_every_axis` (no GPU) show that the checker passes an fp32 SpMM and
rejects each planted error, and that the cases cover every width, threshold, degree, shape and epilogue."""
import contextlib

import numpy as np
import pytest
import scipy.sparse as sp
import torch

CASES = 120
SLICES = (8, 16, 32)
RAW_WIDTHS = SLICES + (64, 128, 192, 256, 320, 384)        # through spmm_raw: the slices and DCH = 1 ... 6
PAD_WIDTHS = (40, 100, 200, 300)                            # through hip_ops.spmm: zero-padded to 64 / 128 / 256 / 320
WIDTHS = RAW_WIDTHS + PAD_WIDTHS
THRESHOLDS = (0, 1, 8, 16, 32, 256, 511, 512, 513, 4096, None)
EPILOGUES = ("Y", "YZ", "YZacc", "acc", "alias", "beta_noZ")
SHAPES = ("tiny", "nnz0", "tall", "wide", "xrows", "square")
SPECIAL_DEGREES = (0, 1, 512, 513, 1024, 1025, 5000, 8200)  # + threshold - 1, threshold, threshold + 1; 8200: 17 chunks
BIG_ROWS = (1 << 18) + 37                                   # just above the row count where the kernels go to 4 rows per group
BIG_SEEDS = (105, 107, 109, 111)                            # d = 16, 64, 192, 320 (seed % 13)
EXACT_COEF = (1.0, -2.0, 0.5, 0.25, -0.25)
FLOAT_COEF = EXACT_COEF + (1.0 / 3.0, -0.7)
CHUNK = 512
U = 2.0 ** -24
GRID = 512.0
FLT_MAX = float(np.finfo(np.float32).max)


# ------------------------------------------------------------------------------------------------ host references
def csr(rowptr, cols, vals, shape):
    """scipy CSR in exactly this entry order (the (data, indices, indptr) form keeps duplicates: nothing is summed)"""
    return sp.csr_matrix((np.asarray(vals, np.float64), np.asarray(cols, np.int64), np.asarray(rowptr, np.int64)), shape=shape)


def rows_of(rowptr, cols, vals, rows):
    """(rowptr, cols, vals) of A[rows], listed rows in order, duplicates kept"""
    rows = np.asarray(rows, np.int64)
    s, e = rowptr[rows], rowptr[rows + 1]
    deg = e - s
    rp = np.zeros(rows.size + 1, np.int64)
    np.cumsum(deg, out=rp[1:])
    take = np.repeat(s - rp[:-1], deg) + np.arange(rp[-1])
    return rp, cols[take], vals[take]


def scatter_matrix(rows, n_rows):
    """P [n_rows, len(rows)] with P[rows[i], i] = 1: P @ G adds G[i] into row rows[i]"""
    rows = np.asarray(rows, np.int64)
    return sp.csc_matrix((np.ones(rows.size), rows, np.arange(rows.size + 1)), shape=(n_rows, rows.size))


def absolute(mat):
    """|mat| entry by entry (scipy's abs() sums duplicate entries first -- in place -- and so would shrink sum |a_k x_k| and turn
    0 * inf + 1 * inf into 1 * inf)"""
    out = mat.copy()
    out.data = np.abs(out.data)
    return out


def plan_depth(deg, thr):
    """per row: the most roundings a term meets under the kernels' plan, the epilogue's four included (module docstring)"""
    deg = np.asarray(deg, np.int64)
    nch = -(-deg // CHUNK)
    chunked = 32 + 15 + np.where(nch > 1, -(-nch // 16) + 15, 0)
    return np.where(deg > thr, chunked, deg) + 4


def gamma(n):
    n = np.asarray(n, np.float64)
    return n * U / (1.0 - n * U)


def _block(t, n, c0, c1):
    if isinstance(t, torch.Tensor):
        return t[:n, c0:c1].detach().cpu().double().numpy()
    return np.asarray(t[:n, c0:c1], dtype=np.float64)


def check(got, terms, *, Z=None, beta=1.0, acc_in=None, acc_scale=None, exact, depth=None, name=""):
    """got[:n] against  acc_scale * (acc_in + sum_t coef_t * M_t @ X_t + beta * Z)  (terms = [(coef, scipy matrix [n, k],
    dense [>= k, d])]; acc_scale None: no acc form) in the mode's sense (module docstring); the float64 work runs in column
    blocks of a few MB.  Returns the float mode's worst err / M (0 in exact mode)."""
    n, d = terms[0][1].shape[0], terms[0][2].shape[1]
    assert got.shape[0] >= n and got.shape[1] == d, (name, tuple(got.shape), n, d)
    if not exact:
        tol = gamma(depth)[:, None]
        floor = np.asarray(depth, np.float64)[:, None] * 2.0 ** -149
    step = max(1, (1 << 21) // max(n, 1))
    worst = 0.0
    for c0 in range(0, d, step):
        c1 = min(d, c0 + step)
        with np.errstate(invalid="ignore", over="ignore"):
            ref, T, M = (np.zeros((n, c1 - c0)) for _ in range(3))
            for coef, mat, X in terms:
                Xb = np.asarray(X[:mat.shape[1], c0:c1], dtype=np.float64)
                t = np.asarray(absolute(mat) @ np.abs(Xb))
                ref += coef * np.asarray(mat @ Xb)
                T += t
                M += abs(coef) * t
            if Z is not None:
                Zb = _block(Z, n, c0, c1)
                ref += beta * Zb
                M += abs(beta) * np.abs(Zb)
            peak = T + M
            if acc_scale is not None:
                Ab = _block(acc_in, n, c0, c1)
                peak += np.abs(Ab)
                ref = acc_scale * (Ab + ref)
                M = abs(acc_scale) * (np.abs(Ab) + M)
        g = _block(got, n, c0, c1)
        if exact:
            assert np.isfinite(ref).all() and (peak * GRID < 2.0 ** 23).all(), (name, "case outside the exact grid")
            bad = g != ref
            if bad.any():
                r, col = np.argwhere(bad)[0]
                raise AssertionError((name, "exact mismatch", int(bad.sum()), "first at", (int(r), int(c0 + col)),
                                      float(g[r, col]), float(ref[r, col])))
            continue
        ref32 = np.where(np.abs(ref) > FLT_MAX, np.copysign(np.inf, ref), ref)
        fin = np.isfinite(ref32)
        assert np.array_equal(np.isfinite(g), fin), (name, "non-finite pattern", int((np.isfinite(g) != fin).sum()))
        same = (g == ref32) | (np.isnan(g) & np.isnan(ref32))
        if not same[~fin].all():
            r, col = np.argwhere(~fin & ~same)[0]
            raise AssertionError((name, "non-finite values differ", int((~fin & ~same).sum()), "first at",
                                  (int(r), int(c0 + col)), float(g[r, col]), float(ref32[r, col])))
        with np.errstate(invalid="ignore"):
            err = np.where(fin, np.abs(g - ref32), 0.0)
            viol = fin & (err > tol * M + floor)
        if viol.any():
            r, col = np.argwhere(viol)[0]
            raise AssertionError((name, "beyond gamma(n) M", int(viol.sum()), "first at", (int(r), int(c0 + col)),
                                  float(err[r, col]), float(M[r, col]), int(np.asarray(depth)[r])))
        pos = fin & (M > 0)
        if pos.any():
            worst = max(worst, float((err[pos] / M[pos]).max()))
    return worst


# ------------------------------------------------------------------------------------------------ cases
def _grid(rng, shape, k=16):
    """multiples of 1/16 in [-k/16, k/16]"""
    return (rng.integers(-k, k + 1, shape) / 16.0).astype(np.float32)


def _on(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


class Case:
    pass


def _degrees(rng, c):
    n_rows, thr = c.n_rows, c.thr_eff
    c.tail = [int(x) for x in np.minimum((rng.pareto(1.1, 3) + 1) * 40, 3000)]     # a power-law tail
    if c.shape == "nnz0":
        return np.zeros(n_rows, np.int64)
    deg = rng.geometric(0.5 if c.big else 0.15, n_rows) - 1
    deg[rng.random(n_rows) < 0.2] = 0                                 # empty rows
    special = [k for k in SPECIAL_DEGREES + (thr - 1, thr, thr + 1) + tuple(c.tail) if k >= 0]
    rng.shuffle(special)
    # rows placed first, last and in between
    order = np.concatenate([[0, n_rows - 1], 1 + rng.permutation(max(n_rows - 2, 0))]) if n_rows > 1 else np.zeros(1, np.int64)
    for r, k in zip(order, special):
        deg[r] = k
    if not c.exact:
        deg[(deg <= thr) & (deg > 1024)] = 1024                       # float mode: sequential chains <= 1024 nonzeros
    return deg.astype(np.int64)


def draw_case(seed):
    from mmrec_amd.hip_ops import default_long_row_threshold
    rng = np.random.default_rng(7000 + seed)
    c = Case()
    c.seed = seed
    c.d = WIDTHS[seed % len(WIDTHS)]
    c.thr = THRESHOLDS[seed % len(THRESHOLDS)]
    c.exact = seed % 3 != 2
    c.epi = EPILOGUES[(seed // 3) % len(EPILOGUES)]
    c.big = seed in BIG_SEEDS
    c.shape = "big" if c.big else SHAPES[(seed // len(WIDTHS)) % len(SHAPES)]
    if c.big:
        c.epi = "Y"                                                   # (the epilogue paths run at every width elsewhere)
    c.n_rows, c.n_cols = {"tiny": lambda: (int(rng.integers(1, 51)), int(rng.integers(8, 51))),
                          "nnz0": lambda: (int(rng.integers(1, 300)), int(rng.integers(1, 300))),
                          "tall": lambda: (2000, 300), "wide": lambda: (300, 4000), "xrows": lambda: (800, 800),
                          "square": lambda: (1500, 1500), "big": lambda: (BIG_ROWS, 3000)}[c.shape]()
    n_rows, n_cols, d = c.n_rows, c.n_cols, c.d
    c.x_rows = n_cols + (int(rng.integers(1, 50)) if c.shape == "xrows" else 0)
    c.thr_eff = default_long_row_threshold(n_cols) if c.thr is None else c.thr
    c.deg = _degrees(rng, c)
    c.rowptr = np.zeros(n_rows + 1, np.int64)
    np.cumsum(c.deg, out=c.rowptr[1:])
    nnz = int(c.rowptr[-1])
    c.rows = np.repeat(np.arange(n_rows), c.deg)
    c.cols = rng.integers(0, n_cols, nnz)
    c.alpha, c.beta, c.acc_scale = (float(rng.choice(EXACT_COEF if c.exact else FLOAT_COEF)) for _ in range(3))
    if c.epi == "beta_noZ":
        c.beta = -2.0                                                 # given, and must be ignored: Z is NULL
    want_z = c.epi in ("YZ", "YZacc") or (d in PAD_WIDTHS and c.epi == "alias")
    want_acc = d in RAW_WIDTHS and c.epi in ("YZacc", "acc", "alias")
    c.alias_y = bool(rng.integers(0, 2))
    if c.exact:
        c.vals = (rng.integers(-8, 9, nnz) / 8.0).astype(np.float32)
        c.X = _grid(rng, (c.x_rows, d))
        c.Z = _grid(rng, (n_rows, d)) if want_z else None
        c.acc_in = _grid(rng, (n_rows, d)) if want_acc else None
        c.G = _grid(rng, (n_rows, d)) if d in PAD_WIDTHS else None
        # the exact grid on an upper bound of every intermediate (|X|, |Z|, |acc_in|, |G| <= 1): the forward rows and, for the
        # autograd widths, the rows of A^T
        vsum = np.bincount(c.rows, weights=np.abs(c.vals), minlength=n_rows)
        assert ((1 + abs(c.alpha)) * vsum.max(initial=0) + abs(c.beta) + 1) * GRID < 2.0 ** 23, (seed, "outside the grid")
        if c.G is not None:
            csum = np.bincount(c.cols, weights=np.abs(c.vals), minlength=n_cols)
            assert (2 * csum.max(initial=0) + 1) * GRID < 2.0 ** 23, (seed, "backward outside the grid")
    else:
        vals = rng.standard_normal(nnz) * np.repeat(10.0 ** rng.uniform(-3, 3, n_rows), c.deg)
        vals[rng.random(nnz) < 0.05] = 0.0                            # explicit zero values
        c.vals = vals.astype(np.float32)
        X = rng.standard_normal((c.x_rows, d))
        for i in rng.choice(c.x_rows, size=min(c.x_rows, 4), replace=False):
            X[i] *= 10.0 ** rng.uniform(-8, 8)
        for j in rng.choice(d, size=min(d, 4), replace=False):
            X[:, j] *= 10.0 ** rng.uniform(-4, 4)
        X[rng.random(X.shape) < 0.2] = 0.0
        c.inf_row = (seed // 3) % 4 == 1
        if c.inf_row:                                                 # an inf / NaN row
            X[int(rng.integers(0, c.x_rows)), rng.random(d) < 0.5] = rng.choice([np.inf, -np.inf, np.nan])
        c.X = X.astype(np.float32)
        c.Z = rng.standard_normal((n_rows, d)).astype(np.float32) if want_z else None
        c.acc_in = rng.standard_normal((n_rows, d)).astype(np.float32) if want_acc else None
        c.G = rng.standard_normal((n_rows, d)).astype(np.float32) if d in PAD_WIDTHS else None
        assert not ((c.deg <= c.thr_eff) & (c.deg > 1024)).any()
    c.A = csr(c.rowptr, c.cols, c.vals, (n_rows, n_cols))
    return c


# ------------------------------------------------------------------------------------------------ CPU: the checker and the cases
def _fp32_spmm(c, vals=None, cols=None, with_z=True):
    """an fp32 SpMM of the case on the host.  Exact cases: torch's fp32 CSR product and an fp32 epilogue (any order gives the
    exact result); float cases: the float64 result rounded to fp32 (the best any fp32 kernel can give)"""
    vals = c.vals if vals is None else vals
    cols = c.cols if cols is None else cols
    z = c.Z if (with_z and c.Z is not None) else None
    if c.exact:
        A = torch.sparse_csr_tensor(torch.from_numpy(c.rowptr), torch.from_numpy(np.asarray(cols, np.int64)),
                                    torch.from_numpy(np.asarray(vals, np.float32)), size=(c.n_rows, c.n_cols))
        y = np.float32(c.alpha) * (A @ torch.from_numpy(c.X[:c.n_cols])).numpy()
        return y + np.float32(c.beta) * z if z is not None else y
    with np.errstate(invalid="ignore", over="ignore"):
        y = c.alpha * np.asarray(csr(c.rowptr, cols, vals, (c.n_rows, c.n_cols)) @ c.X[:c.n_cols].astype(np.float64))
        if z is not None:
            y = y + c.beta * z
        return y.astype(np.float32)


def _find(cond):
    for s in range(CASES):
        if s not in BIG_SEEDS:
            c = draw_case(s)
            if cond(c):
                return c
    raise AssertionError("no such case")


def test_checker_rejects_planted_errors():
    # exact mode: a case with a >= 5000-nonzero row and a Z term
    c = _find(lambda c: c.exact and c.Z is not None and c.d in RAW_WIDTHS and c.deg.max() >= 5000)
    terms, kw = [(c.alpha, c.A, c.X)], dict(Z=c.Z, beta=c.beta, exact=True)
    good = _fp32_spmm(c)
    check(good, terms, **kw, name="clean")
    long_row = int(np.argmax(c.deg))
    s, e = c.rowptr[long_row], c.rowptr[long_row + 1]
    cand = s + np.flatnonzero((c.vals[s:e] != 0) & np.abs(c.X[c.cols[s:e]]).any(1))
    k = int(cand[cand.size // 2])
    vals = c.vals.copy()
    vals[k] = 0.0                                                     # a dropped nonzero in a >= 5000-nonzero row
    with pytest.raises(AssertionError):
        check(_fp32_spmm(c, vals=vals), terms, **kw)
    cols = c.cols.copy()
    cols[k] = int(np.flatnonzero((c.X[:c.n_cols] != c.X[c.cols[k]]).any(1))[0])      # a wrong column id
    with pytest.raises(AssertionError):
        check(_fp32_spmm(c, cols=cols), terms, **kw)
    stale = good.copy()
    r = int(np.flatnonzero((good != c.Z).any(1))[-1])
    stale[r] = c.Z[r]                                                 # a row left at its previous content
    with pytest.raises(AssertionError):
        check(stale, terms, **kw)
    stale[r] = np.nan                                                 # ... or at a NaN sentinel
    with pytest.raises(AssertionError):
        check(stale, terms, **kw)
    with pytest.raises(AssertionError):                               # a missing beta * Z term
        check(_fp32_spmm(c, with_z=False), terms, **kw)
    # float mode: a case with an inf / NaN row of X that reaches the output
    c = _find(lambda c: not c.exact and c.Z is not None and c.inf_row and not np.isfinite(_fp32_spmm(c)).all())
    terms, depth = [(c.alpha, c.A, c.X)], plan_depth(c.deg, c.thr_eff)
    kw = dict(Z=c.Z, beta=c.beta, exact=False, depth=depth)
    good = _fp32_spmm(c)
    assert check(good, terms, **kw, name="clean float") <= 1.01 * U
    with np.errstate(invalid="ignore", over="ignore"):
        ref = c.alpha * np.asarray(c.A @ c.X[:c.n_cols].astype(np.float64)) + c.beta * c.Z
        M = abs(c.alpha) * np.asarray(absolute(c.A) @ np.abs(c.X[:c.n_cols].astype(np.float64))) + abs(c.beta) * np.abs(c.Z)
        share = np.where(np.isfinite(ref) & (M > 0), np.abs(ref) / M, 0)
    r, col = np.unravel_index(np.argmax(share), share.shape)
    assert share[r, col] > 0.7
    bad = good.copy()
    bad[r, col] = np.float32(ref[r, col] * (1 + 1e-4))                # a 1e-4 relative error
    with pytest.raises(AssertionError):
        check(bad, terms, **kw)
    bad = good.copy()
    bad[r, col] = np.inf                                              # a wrong non-finite pattern: inf where float64 is finite
    with pytest.raises(AssertionError):
        check(bad, terms, **kw)
    bad = good.copy()
    bad[~np.isfinite(good)] = 0.0                                     # ... finite where float64 is not
    with pytest.raises(AssertionError):
        check(bad, terms, **kw)
    bad = good.copy()
    bad[np.isnan(good)], bad[np.isposinf(good)], bad[np.isneginf(good)] = np.inf, -np.inf, np.nan      # ... the wrong one
    with pytest.raises(AssertionError):
        check(bad, terms, **kw)
    with pytest.raises(AssertionError):                               # a missing beta * Z term
        check(_fp32_spmm(c, with_z=False), terms, **kw)


def test_cases_span_every_axis():
    """every width, threshold, epilogue, shape and special degree appears; exact and float cases at every width and with every
    epilogue; rows placed first and last; the big cases above 2^18 rows; multi-chunk rows (so both long-row finishes) at every
    width that is not a slice"""
    seen = {k: set() for k in ("d", "thr", "epi", "shape", "mode", "deg", "multi", "inf")}
    ends, tail = False, 0
    for s in range(CASES):
        c = draw_case(s)
        seen["d"].add(c.d), seen["thr"].add(c.thr), seen["epi"].add(c.epi), seen["shape"].add(c.shape)
        seen["mode"].add((c.d, c.exact)), seen["mode"].add((c.epi, c.exact))
        t = c.thr_eff
        for k, nm in [(k, k) for k in SPECIAL_DEGREES] + [(t - 1, "t-1"), (t, "t"), (t + 1, "t+1")]:
            if (c.deg == k).any():
                seen["deg"].add(nm)
        ends |= bool(c.n_rows > 2 and c.deg[0] > t and c.deg[-1] > t)
        tail = max(tail, max(c.tail))
        if c.d not in SLICES and ((c.deg > t) & (c.deg > CHUNK)).any():
            seen["multi"].add(c.d)
        if not c.exact and c.inf_row:
            seen["inf"].add(c.epi)
        assert c.big == (c.n_rows > (1 << 18))
    assert seen["d"] == set(WIDTHS) and seen["thr"] == set(THRESHOLDS) and seen["epi"] == set(EPILOGUES)
    assert seen["shape"] == set(SHAPES) | {"big"}
    assert seen["mode"] == {(x, e) for x in WIDTHS + EPILOGUES for e in (True, False)}
    assert seen["deg"] == set(SPECIAL_DEGREES) | {"t-1", "t", "t+1"}
    assert ends and tail > 1025 and len(seen["inf"]) >= 3
    assert seen["multi"] == {x for x in WIDTHS if x not in SLICES}
    assert {WIDTHS[s % len(WIDTHS)] for s in BIG_SEEDS} == {16, 64, 192, 320}


# ------------------------------------------------------------------------------------------------ GPU: the fuzz
@contextlib.contextmanager
def _tickets(on, *graphs):
    """on = False: tickets withheld, multi-chunk rows are finished by the second launch"""
    saved = [g.long_tickets for g in graphs]
    if not on:
        for g in graphs:
            g.long_tickets = None
    try:
        yield
    finally:
        for g, t in zip(graphs, saved):
            g.long_tickets = t


def _tickets_zero(*graphs):
    torch.cuda.synchronize()
    for g in graphs:
        if g.long_tickets is not None:
            assert int(g.long_tickets.abs().sum()) == 0, "tickets left non-zero"


def _raw(c, g):
    from mmrec_amd import hip_ops
    nan = lambda: torch.full((c.n_rows, c.d), float("nan"), device="cuda:0")      # noqa: E731
    Y = Z = acc_in = acc = None
    if c.epi in ("Y", "YZ", "YZacc", "beta_noZ") or (c.epi == "alias" and c.alias_y):
        Y = nan()
    if c.epi in ("YZ", "YZacc"):
        Z = _on(c.Z)
    if c.epi in ("YZacc", "acc"):
        acc_in, acc = _on(c.acc_in), nan()
    if c.epi == "alias":
        acc = acc_in = _on(c.acc_in)
    hip_ops.spmm_raw(g, _on(c.X), Y=Y, Z=Z, acc_in=acc_in, acc_out=acc, alpha=c.alpha, beta=c.beta, acc_scale=c.acc_scale)
    torch.cuda.synchronize()
    terms, depth = [(c.alpha, c.A, c.X)], plan_depth(c.deg, c.thr_eff)
    z = c.Z if Z is not None else None
    worst = 0.0
    if Y is not None:
        worst = check(Y, terms, Z=z, beta=c.beta, exact=c.exact, depth=depth, name="Y seed %d" % c.seed)
    if acc is not None:
        worst = max(worst, check(acc, terms, Z=z, beta=c.beta, acc_in=c.acc_in, acc_scale=c.acc_scale, exact=c.exact,
                                 depth=depth, name="acc seed %d" % c.seed))
    return worst


def _autograd(c, g):
    """hip_ops.spmm at a width the kernels do not have (zero-padded), forward and backward (A^T dY through g.transpose())"""
    from mmrec_amd import hip_ops
    X = _on(c.X).requires_grad_()
    Z = _on(c.Z).requires_grad_() if c.Z is not None else None
    out = hip_ops.spmm(g, X, Z)
    assert tuple(out.shape) == (c.n_rows, c.d)
    worst = check(out.detach(), [(1.0, c.A, c.X)], Z=c.Z, exact=c.exact, depth=plan_depth(c.deg, c.thr_eff),
                  name="spmm seed %d" % c.seed)
    out.backward(_on(c.G))
    torch.cuda.synchronize()
    col_deg = np.bincount(c.cols, minlength=c.n_cols)
    worst = max(worst, check(X.grad, [(1.0, c.A.T, c.G)], exact=c.exact, depth=plan_depth(col_deg, c.thr_eff),
                             name="dX seed %d" % c.seed))
    assert bool((X.grad[c.n_cols:] == 0).all())                       # rows of X beyond the graph's columns: no gradient
    if Z is not None:
        assert torch.equal(Z.grad, _on(c.G))
    return worst


@pytest.mark.gpu
@pytest.mark.parametrize("seed", range(CASES))
def test_spmm_fuzz(seed):
    from mmrec_amd import hip_ops
    c = draw_case(seed)
    g = hip_ops.CsrGraph.from_coo_host(np.stack([c.rows, c.cols]), c.vals, c.n_rows, c.n_cols, torch.device("cuda:0"),
                                       long_row_threshold=c.thr)
    assert g.long_row_threshold == c.thr_eff
    graphs = (g, g.transpose()) if c.d in PAD_WIDTHS else (g,)
    forms = (True, False) if c.d not in SLICES and any(h.n_chunks > h.n_long for h in graphs) else (True,)
    worst = 0.0
    for tickets in forms:                                             # both long-row finishes, each against float64
        with _tickets(tickets, *graphs):
            worst = max(worst, _raw(c, g) if c.d in RAW_WIDTHS else _autograd(c, g))
        _tickets_zero(*graphs)
    print("spmm fuzz seed %d: d %d thr %s %s %s %s rows %d nnz %d forms %d worst err/M %.3e" % (
        seed, c.d, c.thr, "exact" if c.exact else "float", c.epi, c.shape, c.n_rows, int(c.rowptr[-1]), len(forms), worst))


# ------------------------------------------------------------------------------------------------ GPU: targeted tests
def _graph(rng, deg, n_cols, vk=8, **kw):
    """CsrGraph + host arrays of a graph with these row degrees, vals multiples of 1/8 in [-vk/8, vk/8], columns uniform"""
    from mmrec_amd import hip_ops
    deg = np.asarray(deg, np.int64)
    rowptr = np.zeros(deg.size + 1, np.int64)
    np.cumsum(deg, out=rowptr[1:])
    rows = np.repeat(np.arange(deg.size), deg)
    cols = rng.integers(0, n_cols, rows.size)
    vals = (rng.integers(-vk, vk + 1, rows.size) / 8.0).astype(np.float32)
    g = hip_ops.CsrGraph.from_coo_host(np.stack([rows, cols]), vals, deg.size, n_cols, torch.device("cuda:0"), **kw)
    return g, rowptr, cols, vals


@pytest.mark.gpu
@pytest.mark.parametrize("d,multi", [(8, False), (16, False), (32, False), (64, False), (64, True)])
def test_listed_rows_pull_and_push_vs_float64(d, multi):
    """spmm_rows_raw on both ABI paths (rows_f32: no multi-chunk row in the graph; rows_any_f32: d = 64 with such rows) with Z
    absent, full and compact, duplicated rows, empty rows; spmm_push_rows_raw into accumulating dX and dZ, separate and
    aliased -- exact mode"""
    from mmrec_amd import hip_ops
    rng = np.random.default_rng(d + 1000 * multi)
    n = 3000
    deg = rng.integers(0, 40, n)
    single = {5: 33, 6: 200, 7: 512, n - 1: 100}                      # long rows of one chunk (threshold 32)
    several = {0: 2000, 10: 513, 11: 1024, 12: 1025, 13: 5000}        # rows of 2 ... 10 chunks
    deg[[1, 2]] = 0
    for r, k in list(single.items()) + (list(several.items()) if multi else []):
        deg[r] = k
    g, rowptr, cols, vals = _graph(rng, deg, n, long_row_threshold=32)
    assert (g.n_chunks > g.n_long) == multi and hip_ops.rows_servable(g, d)
    X, Z = _grid(rng, (n, d)), _grid(rng, (n, d))
    rows = np.concatenate([list(single), list(several) if multi else [3], [1, 2, 5, 5, 7, 0, n - 1, 13, 13],
                           rng.integers(0, n, 500)]).astype(np.int64)
    Ar = csr(*rows_of(rowptr, cols, vals, rows), (rows.size, n))
    Zc = _grid(rng, (rows.size, d))
    for zname, Zt, zref, compact in (("none", None, None, False), ("full", _on(Z), Z[rows], False), ("compact", _on(Zc), Zc, True)):
        got = hip_ops.spmm_rows_raw(g, _on(X), _on(rows), Z=Zt, z_compact=compact)
        check(got, [(1.0, Ar, X)], Z=zref, exact=True, name="rows d %d Z %s" % (d, zname))
    G = _grid(rng, (rows.size, d))
    D0, E0 = _grid(rng, (n, d)), _grid(rng, (n, d))
    P = scatter_matrix(rows, n)
    for scale in (1.0, -0.25):
        dX, dZ = _on(D0), _on(E0)
        hip_ops.spmm_push_rows_raw(g, _on(G), _on(rows), dX=dX, dZ=dZ, scale=scale)
        torch.cuda.synchronize()
        check(dX, [(scale, Ar.T, G)], acc_in=D0, acc_scale=1.0, exact=True, name="push dX")
        check(dZ, [(scale, P, G)], acc_in=E0, acc_scale=1.0, exact=True, name="push dZ")
        both = _on(D0)
        hip_ops.spmm_push_rows_raw(g, _on(G), _on(rows), dX=both, dZ=both, scale=scale)
        torch.cuda.synchronize()
        check(both, [(scale, Ar.T, G), (scale, P, G)], acc_in=D0, acc_scale=1.0, exact=True, name="push aliased")


@pytest.mark.gpu
@pytest.mark.parametrize("extra", [0, 1])
def test_listed_row_at_the_lds_limit(extra):
    """a listed row of exactly 480 x 512 nonzeros is served by the row-list kernel; one of 480 x 512 + 1 is not
    (spmm_rows_raw refuses it on the host, hip_ops.spmm_rows takes the full launch) -- both equal float64"""
    from mmrec_amd import _lib, hip_ops
    rng = np.random.default_rng(480 + extra)
    n = 1000
    deg = rng.integers(0, 20, n)
    deg[3], deg[4] = 480 * CHUNK + extra, 1300
    g, rowptr, cols, vals = _graph(rng, deg, n, vk=1, long_row_threshold=None)      # vals in {-1/8, 0, 1/8}
    assert g.max_row_chunks == 480 + extra and hip_ops.rows_servable(g, 64) == (extra == 0)
    X = _grid(rng, (n, 64), k=2)                                      # |x| <= 1/8: the 245,760-term row stays on the grid
    rows = np.array([3, 4, 0, 3, n - 1, 17, 4], np.int64)
    Ar = csr(*rows_of(rowptr, cols, vals, rows), (rows.size, n))
    check(hip_ops.spmm_rows(g, _on(X), _on(rows)), [(1.0, Ar, X)], exact=True, name="spmm_rows extra %d" % extra)
    if extra == 0:
        check(hip_ops.spmm_rows_raw(g, _on(X), _on(rows)), [(1.0, Ar, X)], exact=True, name="spmm_rows_raw")
    else:
        with pytest.raises(_lib.MMRecHipError):
            hip_ops.spmm_rows_raw(g, _on(X), _on(rows))


@pytest.mark.gpu
def test_listed_row_beyond_max_row_chunks_is_nan():
    """mmrec_spmm_rows_any_f32 with max_row_chunks below a listed row's chunk count: that row is written as quiet NaN (not
    left at what the buffer held); every other listed row is still the float64 result"""
    from mmrec_amd import _lib, hip_ops
    rng = np.random.default_rng(3)
    n = 500
    deg = rng.integers(0, 30, n)
    deg[7], deg[8], deg[9] = 1400, 900, 300                           # 3 chunks, 2 chunks, 1 chunk (threshold 32)
    g, rowptr, cols, vals = _graph(rng, deg, n, long_row_threshold=32)
    assert g.max_row_chunks == 3
    X = _grid(rng, (n, 64))
    rows = np.array([7, 8, 9, 0, 7, n - 1, 8], np.int64)
    Xt, rt = _on(X), _on(rows)
    Y = torch.full((rows.size, 64), 12345.0, device="cuda:0")
    p = hip_ops._p
    rc = _lib.load().mmrec_spmm_rows_any_f32(p(g.rowptr), p(g.colidx), p(g.vals), p(Xt), None, 0, p(rt), rows.size, 64,
                                             g.long_row_threshold, 2, p(Y), hip_ops._stream())
    assert rc == 0
    torch.cuda.synchronize()
    loud = rows == 7
    assert bool(torch.isnan(Y[_on(loud)]).all())
    keep = np.flatnonzero(~loud)
    Ar = csr(*rows_of(rowptr, cols, vals, rows[keep]), (keep.size, n))
    check(Y[_on(keep)], [(1.0, Ar, X)], exact=True, name="rows beside the loud one")


@pytest.mark.gpu
@pytest.mark.parametrize("tickets", [True, False])
@pytest.mark.parametrize("acc", ["sum", "first", "none"])
def test_layergcn_layer_vs_float64(tickets, acc):
    """mmrec_spmm_csr_f32_layergcn on the exact grid: y exactly A x; w = dot / (max(|y|, 1e-8) max(|ego|, 1e-8)) within 64 u
    (its fp32 evaluation: 8 roundings in the dot and in each sum of squares, a square root per norm, a product, a quotient:
    < 25 u relative to sum |y_i ego_i| / (|y| |ego|) <= 1); scaled = w y within 66 u |y|; acc = acc_in + scaled within
    67 u (|y| + |acc_in|); empty rows and zero ego rows give w = 0 exactly"""
    from mmrec_amd import _lib, hip_ops
    rng = np.random.default_rng(17)
    n = 2500
    deg = rng.integers(0, 30, n)
    deg[[3, 4, 5]] = 0                                                 # empty rows
    deg[10], deg[11], deg[12], deg[n - 1] = 2000, 513, 300, 1025
    g, rowptr, cols, vals = _graph(rng, deg, n, long_row_threshold=32)
    assert g.n_chunks > g.n_long
    A = csr(rowptr, cols, vals, (n, n))
    X, ego, A0 = _grid(rng, (n, 64)), _grid(rng, (n, 64)), _grid(rng, (n, 64))
    ego[[3, 20, 21, 10]] = 0.0                                         # zero ego rows (3: also empty; 10: four chunks)
    nan = lambda: torch.full((n, 64), float("nan"), device="cuda:0")   # noqa: E731
    Y, scaled, acc_out = nan(), nan(), (nan() if acc != "none" else None)
    w = torch.full((n,), float("nan"), device="cuda:0")
    acc_in = _on(A0) if acc == "sum" else None
    Xt, egot, p = _on(X), _on(ego), hip_ops._p
    with _tickets(tickets, g):
        rc = _lib.load().mmrec_spmm_csr_f32_layergcn(
            p(g.rowptr), p(g.colidx), p(g.vals), p(Xt), p(Y), p(egot), p(scaled), p(w), p(acc_in), p(acc_out), n, 64,
            g.long_row_threshold, p(g.long_rows), p(g.long_chunk_ptr), g.n_long, g.n_chunks, p(g.partials_for(64)),
            p(g.long_tickets), hip_ops._stream())
        assert rc == 0
        _tickets_zero(g)
    check(Y, [(1.0, A, X)], exact=True, name="layergcn y")
    y64, e64 = np.asarray(A @ X.astype(np.float64)), ego.astype(np.float64)
    w64 = (y64 * e64).sum(1) / (np.maximum(np.linalg.norm(y64, axis=1), 1e-8) * np.maximum(np.linalg.norm(e64, axis=1), 1e-8))
    wg = w.cpu().double().numpy()
    assert np.all(np.abs(wg - w64) <= 64 * U), float(np.abs(wg - w64).max())
    zero = (np.abs(y64).sum(1) == 0) | (np.abs(e64).sum(1) == 0)
    assert zero[[3, 4, 5, 10, 20, 21]].all() and np.all(wg[zero] == 0)
    s64 = w64[:, None] * y64
    sg = scaled.cpu().double().numpy()
    assert np.all(np.abs(sg - s64) <= 66 * U * np.abs(y64)), float(np.abs(sg - s64).max())
    if acc_out is not None:
        a0 = A0.astype(np.float64) if acc == "sum" else 0.0
        ag = acc_out.cpu().double().numpy()
        assert np.all(np.abs(ag - (a0 + s64)) <= 67 * U * (np.abs(y64) + np.abs(a0))), float(np.abs(ag - a0 - s64).max())


def _square_graph(rng, n, n_edges, hubs, isolated, symmetric=True, signed=True):
    """a square graph: random edges plus hub rows (several chunks at threshold 32), no edge at the isolated nodes (empty rows);
    symmetric: every edge mirrored with the same value.  |v| in [1/64, 1/8], of either sign (signed) or positive"""
    from mmrec_amd import hip_ops
    i = np.concatenate([rng.integers(0, n, n_edges)] + [np.full(k, h) for h, k in hubs.items()])
    j = np.concatenate([rng.integers(0, n, n_edges)] + [rng.integers(0, n, k) for k in hubs.values()])
    keep = ~(np.isin(i, isolated) | np.isin(j, isolated))
    i, j = i[keep], j[keep]
    v = (rng.uniform(1 / 64, 1 / 8, i.size) * (rng.choice([-1.0, 1.0], i.size) if signed else 1.0)).astype(np.float32)
    if symmetric:
        i, j, v = np.concatenate([i, j]), np.concatenate([j, i]), np.concatenate([v, v])
    order = np.argsort(i, kind="stable")
    i, j, v = i[order], j[order], v[order]
    rowptr = np.zeros(n + 1, np.int64)
    np.cumsum(np.bincount(i, minlength=n), out=rowptr[1:])
    g = hip_ops.CsrGraph.from_coo_host(np.stack([i, j]), v, n, n, torch.device("cuda:0"), symmetric=symmetric,
                                       long_row_threshold=32)
    return g, csr(rowptr, j, v, (n, n))


@pytest.mark.gpu
@pytest.mark.parametrize("symmetric", [True, False])
@pytest.mark.parametrize("L", [0, 1, 2, 3, 4])
def test_lightgcn_mean_vs_float64(symmetric, L):
    """lightgcn_mean forward s sum_l A^l E0 and backward s sum_l (A^T)^l dOut (s = 1 / (L + 1); non-symmetric: through
    transpose()) against float64, within gamma(N) of the same sums on absolute values: N = L x (the plan's deepest row,
    epilogue included) + 2 (the rounded s)"""
    from mmrec_amd import hip_ops
    rng = np.random.default_rng(40 + L + 10 * symmetric)
    n = 1200
    g, A = _square_graph(rng, n, 9000, {0: 1300, 600: 700, n - 1: 520}, [5, 6, 7], symmetric)
    assert g.n_chunks > g.n_long and A[[5, 6, 7]].nnz == 0
    E0 = rng.standard_normal((n, 64)).astype(np.float32)
    dOut = rng.standard_normal((n, 64)).astype(np.float32)
    E = _on(E0).requires_grad_()
    out = hip_ops.lightgcn_mean(g, E, L)
    out.backward(_on(dOut))
    torch.cuda.synchronize()
    s = 1.0 / (L + 1)
    for name, M, deg, V, got in (("forward", A, np.diff(A.indptr), E0, out.detach()),
                                 ("backward", A.T, np.bincount(A.indices, minlength=n), dOut, E.grad)):
        ref = cur = V.astype(np.float64)
        mag = cabs = np.abs(ref)
        for _ in range(L):
            cur, cabs = np.asarray(M @ cur), np.asarray(absolute(M) @ cabs)
            ref, mag = ref + cur, mag + cabs
        ref, mag = s * ref, s * mag
        N = L * int(plan_depth(deg, g.long_row_threshold).max()) + 2
        err = np.abs(got.cpu().double().numpy() - ref)
        ratio = float((err / np.maximum(mag, 1e-300)).max())
        print("lightgcn_mean L %d %s %s: worst err / M %.3e, bound gamma(%d) = %.3e" % (
            L, "symmetric" if symmetric else "directed", name, ratio, N, gamma(N)))
        assert np.all(err <= gamma(N) * mag + N * 2.0 ** -149), (name, ratio, N)


def _layergcn64(A, E0, L):
    """layergcn.py:125-138 in float64 torch autograd (each norm clamped at 1e-8; their subgradient at 0 is 0), and the sum over
    the layers of A |E_{l-1}| (A >= 0): the magnitude of the products the cosines re-weight"""
    cur, acc, mag = E0, torch.zeros_like(E0), torch.zeros_like(E0)
    ng = torch.linalg.vector_norm(E0, dim=1).clamp_min(1e-8)
    for _ in range(L):
        mag = mag + torch.sparse.mm(A, cur.detach().abs())
        y = torch.sparse.mm(A, cur)
        w = (y * E0).sum(1) / (torch.linalg.vector_norm(y, dim=1).clamp_min(1e-8) * ng)
        cur = w[:, None] * y
        acc = acc + cur
    return acc, mag


@pytest.mark.gpu
@pytest.mark.parametrize("L", [1, 2, 3, 4])
def test_layergcn_sum_vs_float64_autograd(L):
    """layergcn_sum forward and backward against float64 torch autograd of the same formula, on a symmetric graph with empty
    rows (y = 0: the clamped norm), zero ego rows and multi-chunk rows, positive values as the normalised adjacency has.  Each
    row is held to 1e-4 (the project's fp32 tolerance) of a norm: the forward to that of the products it re-weights (a cosine
    near 0 has an absolute error of a few u, not a relative one), the gradient to its own"""
    from mmrec_amd import hip_ops
    rng = np.random.default_rng(70 + L)
    n = 1500
    g, A = _square_graph(rng, n, 12000, {0: 1400, 900: 600}, [3, 4, n - 1], signed=False)
    assert g.n_chunks > g.n_long and A[[3, 4, n - 1]].nnz == 0
    E0 = (rng.standard_normal((n, 64)) * 0.1).astype(np.float32)
    E0[[5, 6, 4]] = 0.0                                                # zero ego rows (4: also an empty row)
    dSum = rng.standard_normal((n, 64)).astype(np.float32)
    E = _on(E0).requires_grad_()
    out = hip_ops.layergcn_sum(g, E, L)
    out.backward(_on(dSum))
    torch.cuda.synchronize()
    coo = A.tocoo()
    A64 = torch.sparse_coo_tensor(torch.from_numpy(np.stack([coo.row, coo.col]).astype(np.int64)), torch.from_numpy(coo.data),
                                  (n, n)).coalesce()
    E64 = torch.from_numpy(E0.astype(np.float64)).requires_grad_()
    ref, mag = _layergcn64(A64, E64, L)
    ref.backward(torch.from_numpy(dSum.astype(np.float64)))
    for name, got, want, scale in (("forward", out.detach(), ref.detach(), mag), ("dE0", E.grad, E64.grad, E64.grad)):
        got, want = got.cpu().double().numpy(), want.numpy()
        row = np.linalg.norm(scale.numpy(), axis=1, keepdims=True)
        err = np.abs(got - want)
        ratio = float((err / np.maximum(row, 1e-300)).max())
        print("layergcn_sum L %d %s: worst err / row norm %.3e" % (L, name, ratio))
        assert np.all(err <= 1e-4 * row), (name, ratio)


@pytest.mark.gpu
@pytest.mark.parametrize("d", [64, 192, 40])
def test_spmm_autograd_vs_float64(d):
    """hip_ops.spmm with Z on a rectangular graph, X with more rows than the graph has columns: out = A X + Z, dX = A^T dY on
    the first n_cols rows and exactly 0 below, dZ = dY -- exact mode, both long-row finishes"""
    from mmrec_amd import hip_ops
    rng = np.random.default_rng(d)
    n_rows, n_cols, x_rows = 700, 500, 530
    deg = rng.integers(0, 30, n_rows)
    deg[[0, 350, n_rows - 1]] = [1500, 0, 600]
    g, rowptr, cols, vals = _graph(rng, deg, n_cols, long_row_threshold=16)
    gt = g.transpose()
    A = csr(rowptr, cols, vals, (n_rows, n_cols))
    X, Z, dY = _grid(rng, (x_rows, d)), _grid(rng, (n_rows, d)), _grid(rng, (n_rows, d))
    for tickets in (True, False):
        with _tickets(tickets, g, gt):
            Xt, Zt = _on(X).requires_grad_(), _on(Z).requires_grad_()
            out = hip_ops.spmm(g, Xt, Zt)
            out.backward(_on(dY))
            _tickets_zero(g, gt)
        check(out.detach(), [(1.0, A, X)], Z=Z, exact=True, name="spmm d %d" % d)
        check(Xt.grad, [(1.0, A.T, dY)], exact=True, name="dX d %d" % d)
        assert bool((Xt.grad[n_cols:] == 0).all()) and torch.equal(Zt.grad, _on(dY))


@pytest.mark.gpu
def test_spmm_vals_vs_float64():
    """hip_ops.spmm_vals (the learned item graph of LATTICE / GRCN): forward A(vals) X, dX = A^T dY and d vals_e =
    <dY[row_e], X[col_e]> on an unsorted COO with duplicate entries and multi-chunk rows -- exact mode"""
    from mmrec_amd import hip_ops
    rng = np.random.default_rng(5)
    n_rows, n_cols = 600, 400
    deg = rng.integers(0, 25, n_rows)
    deg[[1, 2, n_rows - 1]] = [1100, 0, 300]
    r = np.repeat(np.arange(n_rows), deg)
    c = rng.integers(0, n_cols, r.size)
    c[deg[0] + 1:deg[0] + 20] = c[deg[0]]                              # duplicate entries in row 1
    perm = rng.permutation(r.size)
    r, c = r[perm], c[perm]
    v = (rng.integers(-8, 9, r.size) / 8.0).astype(np.float32)
    X, dY = _grid(rng, (n_cols, 64)), _grid(rng, (n_rows, 64))
    dyn = hip_ops.DynGraph(_on(r), _on(c), n_rows, n_cols, long_row_threshold=32)
    Xt, vt = _on(X).requires_grad_(), _on(v).requires_grad_()
    out = hip_ops.spmm_vals(dyn, Xt, vt)
    out.backward(_on(dY))
    torch.cuda.synchronize()
    order = np.argsort(r, kind="stable")
    rowptr = np.zeros(n_rows + 1, np.int64)
    np.cumsum(np.bincount(r, minlength=n_rows), out=rowptr[1:])
    A = csr(rowptr, c[order], v[order], (n_rows, n_cols))
    check(out.detach(), [(1.0, A, X)], exact=True, name="spmm_vals")
    check(Xt.grad, [(1.0, A.T, dY)], exact=True, name="spmm_vals dX")
    dv = (dY.astype(np.float64)[r] * X.astype(np.float64)[c]).sum(1)
    assert np.array_equal(vt.grad.cpu().double().numpy(), dv)


@pytest.mark.gpu
def test_misuse_is_rejected_before_any_launch():
    """Y == X, acc_out == X, acc_out without acc_in, widths 24 and 448, X with fewer rows than n_cols: MMRecHipError from the
    host, nothing written, tickets left at zero"""
    from mmrec_amd import _lib, hip_ops
    rng = np.random.default_rng(9)
    n = 300
    deg = rng.integers(0, 20, n)
    deg[4] = 1200
    g, *_ = _graph(rng, deg, n, long_row_threshold=32)
    X = _on(_grid(rng, (n, 64)))
    X0 = X.clone()
    Y = torch.full((n, 64), 7.0, device="cuda:0")
    A0 = torch.zeros(n, 64, device="cuda:0")
    calls = [lambda: hip_ops.spmm_raw(g, X, Y=X),
             lambda: hip_ops.spmm_raw(g, X, acc_in=A0, acc_out=X),
             lambda: hip_ops.spmm_raw(g, X, Y=Y, acc_in=A0, acc_out=X),
             lambda: hip_ops.spmm_raw(g, X, Y=Y, acc_out=A0),
             lambda: hip_ops.spmm_raw(g, X[:, :24].contiguous(), Y=Y[:, :24].contiguous()),
             lambda: hip_ops.spmm_raw(g, torch.zeros(n, 448, device="cuda:0"), Y=torch.zeros(n, 448, device="cuda:0")),
             lambda: hip_ops.spmm_raw(g, X[:n - 1].contiguous(), Y=Y)]
    for i, call in enumerate(calls):
        with pytest.raises(_lib.MMRecHipError):
            call()
        torch.cuda.synchronize()
        assert torch.equal(X, X0) and bool((Y == 7.0).all()) and bool((A0 == 0).all()), i
    _tickets_zero(g)
    p = hip_ops._p                                                     # the library itself refuses acc_out == X
    rc = _lib.load().mmrec_spmm_csr_f32(p(g.rowptr), p(g.colidx), p(g.vals), p(X), None, None, p(A0), p(X), n, 64, 1.0, 0.0, 1.0,
                                        g.long_row_threshold, p(g.long_rows), p(g.long_chunk_ptr), g.n_long, g.n_chunks,
                                        p(g.partials_for(64)), p(g.long_tickets), hip_ops._stream())
    assert rc == 10001                                                 # MMREC_ERR_BAD_ARG
    torch.cuda.synchronize()
    assert torch.equal(X, X0)
