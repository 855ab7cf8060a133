"""Seeded differential fuzz of the kernels that turn a batch into a loss and a gradient -- csrc/bpr.hip (BPR single / sliced /
multi-term, cosine single / multi-term, gather_sqnorm, rows_reg, the position-ordered scatter), csrc/layer_ew.hip
(row_normalize, cat_leaky) and csrc/infonce.hip -- against float64 numpy written here from the formulas of
include/mmrec_hip.h, never against another form of the same kernels.  The C ABI is called with raw pointers (guarded outputs,
workspaces of exactly *_workspace_bytes(), pre-filled gradient tables, NULL arguments), the autograd wrappers of
mmrec_amd/hip_ops.py on top, with `set_deterministic` off and on.

Two acceptance modes (the SpMM fuzz's):
  exact  sums of products only.  Tables are multiples of 1/16 of magnitude <= 1, per-sample coefficients multiples of 1/4 of
         magnitude <= 2 supplied BY THE TEST, scalars +-1, +-2, 1/2 or 0: every value any order of summation can form is a
         multiple of 2^-10 (2^-4 for a table entry, 2^-2 for the coefficient, 2^-3 for three scalars, 2^-3 for the pre-fill)
         and `table` asserts sum |terms| < 2^14 per element (sums of squares: integers k^2 / 256 with sum k^2 < 2^24), so
         every partial sum is an exact fp32 number and the output must EQUAL float64.  fp32 atomics on such values are exact in
         any order: a contribution of a duplicated id that is lost, doubled, given the wrong sign or sent to the wrong row
         cannot hide.  (The multi-term cosine backward divides by batch[t]: its tables are exact where every batch[t] is a
         power of two and are held to gamma(n) M otherwise.)  cat_leaky is exact for ANY finite input: one rounding per fp32
         operation (the product with the slope; `+ R` is a second operation, as in the torch ops it replaces), so the result is
         the float64 result rounded to fp32 after each operation, bit for bit, -0.0 included (float64 holds the 24 x 24-bit
         product exactly, and a sum of two fp32 numbers rounded through float64 is the correctly rounded fp32 sum).
  float  per element |got - ref64| <= tol, tol the sum of
         1. gamma(n) M + n 2^-149 for the sums of products that feed it (gamma(n) = n u / (1 - n u), u = 2^-24, M the same sum
            on absolute values, Higham sec. 3.1), n from the kernel's plan: a dot of d floats is d / 64 f4_dots of 4 fmas per
            lane and 4 levels of row16_sum (`ndot`), plus one for a difference of two dots; reduce_sum_kernel /
            nce_reduce_kernel: ceil(n / 256) strided adds, 8 LDS levels, the scale (`nsum_plain`); the multi-term finishes:
            the block's 16-way serial sum, ceil(blocks / 256) strided adds, wave_sum's 6 levels, 2 adds over the waves, 2 for
            the epilogue (`nsum_blocks`); a scatter row: its number of occurrences + the products of the chain + the pre-fill;
            InfoNCE: per logit as many fmas as a row has non-zero entries (at most 64), per row sum 4 ceil(tiles / 4) adds, 4
            levels and 4 splits, per gradient column ceil(tiles / 4) tiles of 64 fmas (`nce_chain`) or its non-zero count;
         2. that error through the scalar function: max |f(x +- dx) - f(x)| + dx^2 (f smooth with |f''| <= 1 on the scale of 1:
            the endpoint differences bound the first-order term, dx^2 the remainder; |l'| <= 1, |c'| <= 1/4 for BPR), the
            quotient rule for cs / (cx cx), 1 / max(norm, eps), log(ttl);
         3. E u |value| for expf / log1pf / logf / sqrtf / division on the device.  E is MEASURED ON THE CPU, never taken from
            the kernels: the fp32 numpy evaluation of the same formulas at the fp32-rounded float64 arguments of every float
            case against float64, worst error in units of u |value|, times 4, not below 4
            (`test_E_is_four_times_the_measured_worst`).  Measured worst: BPR logsig loss / coef 4.8, the gamma variant's
            sigmoid 3.3, sqrt and division 1.0, InfoNCE's exp and log(exp) 3.5 -> E_BPR = 20, E_SIG = 14, E_DIV = 4, E_NCE = 14.  The
            gamma variant forms 1 - s and 1e-10 + s from the rounded sigmoid: its l and coef carry E_SIG u s through those
            two expressions (an absolute u near s = 1, as the fp32 reference formula has it);
         4. FLOOR = 4 x 2^-126 (x 1e10 for the gamma variant's coef, whose divisor can be 1e-10) for values float64 resolves and
            fp32 flushes: expf under- / overflow at |x| > 87.
         Non-finite outputs must be float64's, value for value, and appear only where float64 has them.
         Sharpness (`test_tolerances_stay_sharp`, CPU): scalars tol <= 1e-5 |ref| where |ref| > 1e-3; gradient tables: >= 90 %
         of the non-zero elements tol <= 1e-4 |ref|.  Float cases therefore keep <= 1024 occurrences of one id (gamma(1024)
         = 6.1e-5; longer chains are exact cases), rows of one sign per dot (no cancellation inside a dot product) and, for the
         gamma variant, mostly negative scores (its coef has an absolute error u).  InfoNCE multiplies a logit's error by 1 / tau (50 at tau = 0.02), and E >= 4 on
         the two normalisations alone is 16 u: its cases with tau < 0.5 or more than 1024 rows therefore use nearly orthogonal
         rows (eight non-zero entries, one of them dominant, the two views' dominant columns in different halves), so that
         sum |v1 v2| of a logit is a few per cent, an fma chain has eight live terms and a gradient column's chain its
         non-zero count -- `ev_infonce` bounds each logit by ITS sum |v1 v2|, not by 1; the dense cases are tau = 0.5 and 1.

`draw_case(seed)` is deterministic in the seed; `test_cases_span_every_axis` asserts every axis value to occur;
`test_checker_rejects_planted_errors` shows that an fp32 restatement passes and each planted error fails, on the CPU.
"""
import ctypes

import numpy as np
import pytest
import torch

F32, F64 = np.float32, np.float64
U = 2.0 ** -24
TINY = 2.0 ** -149
FLOOR = 4 * 2.0 ** -126
E_BPR, E_SIG, E_DIV, E_NCE = 20.0, 14.0, 4.0, 14.0            # test_E_is_four_times_the_measured_worst
EPS_BPR = float(F32(1e-10))
EPS_COS = float(F32(1e-8))
EPS_NRM = float(F32(1e-12))

OPS = ("bpr", "bpr_dots", "bpr_multi", "cosine", "cosine_multi", "gather", "rows_reg", "scatter", "row_normalize", "cat_leaky",
       "infonce")
PER_OP = 14
CASES = PER_OP * len(OPS)                                   # 154
BATCHES = (0, 1, 15, 16, 17, 255, 256, 257, 2048, 4096, 4097, 8193)
WHOLE_TABLE = 39400                                         # >= 39,387: BM3's whole-table EmbLoss term
NCE_BATCHES = (1, 63, 64, 65, 255, 257, 333, 2048, 4097)
WIDE = (64, 128, 192, 256, 384)
SLICES = (8, 16, 32)
EW_WIDTHS = (4, 12, 20, 100, 4096) + WIDE
TAUS = (0.02, 0.07, 0.2, 0.5, 1.0)
PATTERNS = ("perm", "one", "zipf")
MAX_TERMS = {"bpr_multi": 4, "cosine_multi": 8, "rows_reg": 6}
EXACT_SCALARS = (1.0, -2.0, 0.5, 0.0, -1.0, 2.0)
FLOAT_SCALARS = (1.0, -0.7, 1.0 / 3.0, 0.0, 2.5, -1.0)
FLOAT_ONLY = ("row_normalize", "infonce")
GUARD = 64
GUARD_VALUE = 12345.0


def gamma(n):
    n = np.asarray(n, F64)
    return n * U / (1.0 - n * U)


def ndot(d):
    return 4 * -(-d // 64) + 4


def nsum_plain(n):
    return -(-max(n, 1) // 256) + 8 + 1


def nsum_blocks(batch):
    blocks = -(-max(batch, 1) // 16)
    return 16 + -(-blocks // 256) + 6 + 2 + 2


def nce_chain(B):
    tiles = -(-B // 64)
    return 64 * -(-tiles // 4) + 3


def rnd(a, dt):
    """one fp32 rounding in the restatement (dt = F32); nothing in the reference"""
    a = np.asarray(a, F64)
    if dt is F32:
        with np.errstate(over="ignore", invalid="ignore", under="ignore"):
            return a.astype(F32).astype(F64)
    return a


def fn(f, dt, *xs):
    """f on dt arrays (fp32 numpy in the restatement: the stand-in for the device's math functions), results as float64"""
    with np.errstate(all="ignore"):
        out = f(*[np.asarray(x, F64).astype(dt) for x in xs])
    return tuple(np.asarray(o, F64) for o in out) if isinstance(out, tuple) else np.asarray(out, F64)


# ------------------------------------------------------------------------------------------------ checks
def check_exact(got, ref, name):
    got, ref = np.asarray(got, F64), np.asarray(ref, F64)
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    assert np.isfinite(ref).all(), (name, "exact reference not finite")
    bad = got != ref
    if bad.any():
        i = tuple(int(x) for x in np.argwhere(bad)[0])
        raise AssertionError((name, "exact mismatch", int(bad.sum()), "first at", i, float(got[i]), float(ref[i])))
    return 0.0


def check_float(got, ref, tol, name):
    """|got - ref| <= tol where ref is finite, the same non-finite values elsewhere; returns the worst err / tol"""
    got, ref = np.asarray(got, F64), np.asarray(ref, F64)
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    tol = np.broadcast_to(np.asarray(tol, F64), ref.shape)
    fmax = float(np.finfo(F32).max)
    with np.errstate(invalid="ignore"):
        ref = np.where(np.abs(ref) > fmax, np.copysign(np.inf, ref), ref)
    fin = np.isfinite(ref)
    if not np.array_equal(np.isfinite(got), fin):
        i = tuple(int(x) for x in np.argwhere(np.isfinite(got) != fin)[0])
        raise AssertionError((name, "non-finite pattern", int((np.isfinite(got) != fin).sum()), "first at", i, float(got[i]),
                              float(ref[i])))
    same = (got == ref) | (np.isnan(got) & np.isnan(ref))
    if not same[~fin].all():
        raise AssertionError((name, "non-finite values differ", int((~fin & ~same).sum())))
    with np.errstate(invalid="ignore"):
        err = np.where(fin, np.abs(got - ref), 0.0)
        t = np.where(fin, tol, 1.0)
    assert not np.isnan(t).any() and (t >= 0).all(), (name, "tolerance undefined")
    viol = err > t
    if viol.any():
        i = tuple(int(x) for x in np.argwhere(viol)[0])
        raise AssertionError((name, "beyond tol", int(viol.sum()), "first at", i, "got", float(got[i]), "ref", float(ref[i]),
                              "err", float(err[i]), "tol", float(t[i])))
    pos = fin & (t > 0)
    return float((err[pos] / t[pos]).max()) if pos.any() else 0.0


def check(got, ref, tol, exact, name):
    return check_exact(got, ref, name) if exact else check_float(got, ref, tol, name)


def sharp_scalar(ref, tol, name, factor=1.0):
    ref, tol = float(ref), float(tol)
    if np.isfinite(ref) and abs(ref) > 1e-3:
        assert tol <= 1e-5 * factor * abs(ref), (name, "scalar tolerance not sharp", tol / abs(ref))


def sharp_table(ref, tol, name, factor=1.0, share=0.9):
    with np.errstate(invalid="ignore"):
        nz = np.isfinite(ref) & (ref != 0)
        if nz.any():
            ok = tol[nz] <= 1e-4 * factor * np.abs(ref[nz])
            assert ok.mean() >= share, (name, "table tolerance not sharp", float(ok.mean()))


def _on_grid(total_abs, quantum, name):
    assert np.all(np.asarray(total_abs, F64) / quantum < 2.0 ** 24), (name, "outside the exact grid")


# ------------------------------------------------------------------------------------------------ scalar functions
def bpr_scalar(x, variant):
    """(l, c) in the dtype of x, in the kernels' algebraic form"""
    dt = x.dtype.type
    one = dt(1)
    if variant == 0:
        return np.maximum(-x, dt(0)) + np.log1p(np.exp(-np.abs(x))), -one / (one + np.exp(x))
    s = one / (one + np.exp(-x))
    eps = dt(EPS_BPR)
    return -np.log(eps + s), -(s * (one - s)) / (eps + s)


def bpr_eval(x, dx, variant, dt):
    """l, c at the scores x (float64 value, bound dx) and their tolerances"""
    l, c = fn(lambda v: bpr_scalar(v, variant), dt, rnd(x, dt))
    if dt is F32:
        return l, c, None, None
    with np.errstate(all="ignore"):
        lp, cp = bpr_scalar(x + dx, variant)
        lm, cm = bpr_scalar(x - dx, variant)
        tl = np.maximum(np.abs(lp - l), np.abs(lm - l)) + dx * dx
        tc = np.maximum(np.abs(cp - c), np.abs(cm - c)) + dx * dx
        if variant == 0:
            tl, tc = tl + E_BPR * U * np.abs(l) + FLOOR, tc + E_BPR * U * np.abs(c) + FLOOR
        else:
            s = 1.0 / (1.0 + np.exp(-x))
            ds = E_SIG * U * s
            tl = tl + ds / (EPS_BPR + s) + E_SIG * U * np.abs(l) + FLOOR
            tc = tc + (ds * (1 - s) + s * (ds + U * (1 - s))) / (EPS_BPR + s) + np.abs(c) * (ds + U * (EPS_BPR + s)) / (EPS_BPR + s) \
                + E_SIG * U * np.abs(c) + FLOOR * 1e10
    return l, c, tl, tc


def dots(A, ia, B, ib):
    a = A.astype(F64) if ia is None else A[ia].astype(F64)
    b = B.astype(F64) if ib is None else B[ib].astype(F64)
    with np.errstate(invalid="ignore", over="ignore"):
        return (a * b).sum(1), (np.abs(a) * np.abs(b)).sum(1)


def total(vals, tols, n, scale, dt, drop=None):
    """scale * sum(vals) as a fixed-order fp32 tree of depth n; drop: indices a planted error leaves out"""
    vals = np.asarray(vals, F64)
    keep = np.ones(vals.size, bool)
    if drop is not None:
        keep[drop] = False
    with np.errstate(invalid="ignore", over="ignore"):
        s = float(vals[keep].astype(dt).sum(dtype=dt)) if vals.size else 0.0
        out = rnd(scale * s, dt)
        tol = None if tols is None else abs(scale) * (np.sum(tols) + gamma(n) * np.sum(np.abs(vals))) + n * TINY
    return float(out), tol


def table(n_rows, d, pre, contribs, chain, dt, plant=None, grid=False, name=""):
    """pre + sum over contribs (ids, coef [B], rows [B, d], tolc [B] or None) of coef[b] rows[b] into row ids[b]; float64 with
    its tolerance, or the fp32 restatement (np.add.at in fp32: one order of the atomics) with a planted error"""
    if dt is F32:
        out = np.zeros((n_rows, d), F32) if plant == "store_prefill" else pre.astype(F32).copy()
        for ids, coef, rows, _ in contribs:
            with np.errstate(all="ignore"):
                v = coef.astype(F32)[:, None] * rows.astype(F32)
            if plant == "store_dup":                   # a store where an atomic add belongs: the last occurrence wins
                out[ids] = pre.astype(F32)[ids] + v
            else:
                np.add.at(out, ids, v)
        return out.astype(F64), None
    ref = pre.astype(F64).copy()
    M, T, cnt = np.abs(ref), np.zeros((n_rows, d)), np.zeros(n_rows)
    with np.errstate(invalid="ignore", over="ignore"):
        for ids, coef, rows, tolc in contribs:
            if ids.size == 0:
                continue
            v = coef[:, None] * rows
            np.add.at(ref, ids, v)
            np.add.at(M, ids, np.abs(v))
            np.add.at(cnt, ids, 1)
            if tolc is not None:
                np.add.at(T, ids, tolc[:, None] * np.abs(rows))
        n = cnt + chain + 1
        tol = gamma(n)[:, None] * M + n[:, None] * TINY + T
    if grid:
        _on_grid(M, 2.0 ** -10, name)
    return ref, tol


# ------------------------------------------------------------------------------------------------ cases
class Case:
    zero_pre = False

    def axes(self):
        keys = ("seed", "op", "exact", "batch", "d", "pattern", "n_terms", "variant", "mode", "tau", "eps", "g", "scale", "nonfinite",
                "null")
        return " ".join("%s=%s" % (k, getattr(self, k)) for k in keys if hasattr(self, k))


def _grid(rng, shape, k=16):
    return (rng.integers(-k, k + 1, shape) / 16.0).astype(F32)


def _coefgrid(rng, n):
    return (rng.integers(-8, 9, n) / 4.0).astype(F32)


def _rows(rng, n, d, lo=-1.0, hi=0.85, sign=None):
    """float-mode rows: entries of one sign per row (5 % flipped) and magnitude in [0.05, 3] / sqrt(0.64 d) times a row scale
    10^U(lo, hi): a dot of two such rows is about the product of their scales and hardly cancels"""
    a = np.clip(np.abs(rng.standard_normal((n, d))), 0.05, 3.0) / np.sqrt(0.64 * d)
    a[rng.random((n, d)) < 0.05] *= -1.0
    s = rng.choice([-1.0, 1.0], (n, 1)) if sign is None else sign
    return (a * s * 10.0 ** rng.uniform(lo, hi, (n, 1))).astype(F32)


def _ids(rng, pattern, batch, n_rows, seed, cap=None):
    """ids of one pattern; rows 1 and n_rows - 2 are never named; the first and the last row are (pattern "one": one of them)"""
    if batch == 0:
        return np.zeros(0, np.int64)
    if pattern == "one":
        return np.full(batch, n_rows - 1 if seed % 2 else 0, np.int64)
    free = np.setdiff1d(np.arange(n_rows), [0, 1, n_rows - 2, n_rows - 1])
    if pattern == "perm":
        assert free.size + 2 >= batch
        ids = np.concatenate([[0, n_rows - 1], rng.permutation(free)])[:batch]
    else:
        hot = rng.permutation(free)
        ids = hot[(rng.zipf(1.3, batch) - 1) % hot.size]
        if cap is not None:                                  # float mode: at most `cap` occurrences of an id
            order = np.argsort(ids, kind="stable")
            rank = np.arange(batch) - np.searchsorted(ids[order], ids[order])
            over = order[rank >= cap]
            ids[over] = hot[-1 - (np.arange(over.size) % max(hot.size // 2, 1))]
        ids[0], ids[-1] = 0, n_rows - 1
    return rng.permutation(ids).astype(np.int64)


def _n_rows(pattern, batch):
    return batch + 8 if pattern == "perm" else max(12, batch // 3 + 8)


def _share(k, n_terms):
    """term -> table: a table named by two or three terms where (k + t) % 3 == 0"""
    share = [0] * n_terms
    for t in range(1, n_terms):
        share[t] = share[t - 1] if (k + t) % 3 == 0 else share[t - 1] + 1
    return share


def _renorm(row, norm):
    return (row.astype(F64) * (norm / max(np.linalg.norm(row.astype(F64)), 1e-300))).astype(F32)


def draw_case(seed):
    rng = np.random.default_rng(9000 + seed)
    c = Case()
    c.seed, oi, k = seed, seed % len(OPS), seed // len(OPS)
    c.op = op = OPS[oi]
    sliced = op in ("bpr_dots", "scatter")
    c.exact = op == "cat_leaky" or (op not in FLOAT_ONLY and (k + oi + (k // 8 if sliced else 0)) % 2 == 0)
    c.batch = BATCHES[k] if k < 12 else (8193, 4097)[k - 12]
    c.pattern = PATTERNS[(k + oi) % 3] if k < 12 else ("one", "zipf")[k - 12]
    if k == 12:
        c.exact = op not in FLOAT_ONLY                      # the 8193-long chain of one id: exact
    if not c.exact and c.pattern == "one" and c.batch > 1024:
        c.pattern = "zipf"                                  # float chains <= 1024 (module docstring)
    cap = None if c.exact else (160 if op in MAX_TERMS else 512)      # occurrences of an id per list: <= 1024 per table row
    c.d = (SLICES + WIDE)[k % 8] if sliced else WIDE[k % 5]
    sc = EXACT_SCALARS if c.exact else FLOAT_SCALARS
    c.g, c.scale = float(sc[k % 6]), float(sc[(k + 2) % 6]) or 1.0
    c.nonfinite = (not c.exact) and k % 7 == 3 and op in ("bpr", "bpr_multi", "gather", "scatter")
    c.nonfinite_named = c.nonfinite and (seed // 2) % 2 == 0
    B, d = c.batch, c.d
    c.n_rows = n = _n_rows(c.pattern, B)
    heavy = c.exact and B > 2048 and c.pattern != "perm"
    tab = (lambda rows, **kw: _grid(rng, (rows, d), 4 if heavy else 16)) if c.exact else (lambda rows, **kw: _rows(rng, rows, d, **kw))
    ids = lambda: _ids(rng, c.pattern, B, n, seed, cap)      # noqa: E731

    def poison(T, named):
        """one inf and one NaN row at ids the batch names / does not name"""
        pool = np.unique(named) if c.nonfinite_named and named.size else np.array([1, T.shape[0] - 2])
        if c.nonfinite and pool.size >= 2:
            T[pool[0], ::2], T[pool[-1], 1::3] = np.inf, np.nan
        return T

    if op in ("bpr", "bpr_dots", "bpr_multi"):
        c.variant = (k // 2 + oi) % 2 if op != "bpr_dots" else k % 2
        c.n_terms = 1 + k % MAX_TERMS["bpr_multi"] if op == "bpr_multi" else 1
        c.users, c.U = ids(), tab(n, sign=1.0)
        if not c.exact:
            c.U[rng.choice(n, 2)] = 0.0
        c.share = _share(k, c.n_terms)
        c.pos = [ids() for _ in range(c.n_terms)]
        c.neg = [_ids(rng, c.pattern, B, n, seed + 1, cap) for _ in range(c.n_terms)]      # (pattern "one": the other end row)
        c.I = []
        for j in range(max(c.share) + 1):
            T = tab(n)
            if not c.exact and c.variant == 1:              # gamma variant: mostly negative scores
                sgn = np.ones((n, 1))
                for t in range(c.n_terms):
                    if c.share[t] == j and B:
                        sgn[c.pos[t]] = np.where(rng.random((B, 1)) < 0.95, -1.0, 1.0)
                T = np.abs(T) * sgn.astype(F32)
                T[rng.random(T.shape) < 0.03] *= -1
            c.I.append(poison(T, c.pos[0]))
        c.same_pn = op != "bpr_multi" and k % 2 == 0          # P and N the same table (and dP == dN)
        if op != "bpr_multi" and not c.same_pn:
            c.I.append(tab(n))
        if not c.exact:                                      # columns scaled over many decades, dots unchanged
            cs = np.ones(d, F32)
            cs[rng.choice(d, min(4, d), replace=False)] = (10.0 ** rng.uniform(-3, 3, min(4, d))).astype(F32)
            c.U = c.U * cs
            c.I = [T / cs for T in c.I]
        c.w = [float(sc[(k + 1 + t) % 6]) for t in range(c.n_terms)]
        if not c.exact:
            c.w = [abs(w) + 0.25 for w in c.w]               # (a scalar whose terms do not cancel)
        c.coef = [_coefgrid(rng, B) // (2 if heavy else 1) for _ in range(c.n_terms)] if c.exact else None
        c.null = ("none", "dU", "dI", "losses")[k % 4] if op == "bpr_multi" else ("none", "dU")[k % 5 == 4]
    elif op in ("cosine", "cosine_multi"):
        c.n_terms = 1 + k % MAX_TERMS["cosine_multi"] if op == "cosine_multi" else 1
        c.batches = [B] + [(0, 37, B // 2 + 1, 300)[(k + t) % 4] for t in range(1, c.n_terms)]
        if op == "cosine_multi" and k == 12:
            c.batches[0], c.pattern = WHOLE_TABLE, "perm"
        c.share = _share(k, c.n_terms)
        c.X, c.Y, c.ix, c.iy = [], [], [], []
        ysign = 1.0 if k % 2 else -1.0
        for t in range(c.n_terms):
            bt = c.batches[t]
            whole = (k + t) % 3 == 1 or bt == WHOLE_TABLE    # ix NULL: row b
            shared = t > 0 and c.share[t] == c.share[t - 1]
            gmax = max(b for b, j in zip(c.batches, c.share) if j == c.share[t])      # the largest term naming this table
            nx = c.X[-1].shape[0] if shared else max(bt if whole else 0, _n_rows(c.pattern, gmax) if gmax > bt or not whole else 0, 1)
            if shared and whole and nx < bt:
                whole = False
            if not shared:
                X = tab(nx, lo=-3.0, hi=3.0, sign=1.0)
                if not c.exact and nx >= 12:
                    X[3] = 0.0                               # an exact zero row
                    X[4], X[5] = _renorm(X[4], 0.4e-8), _renorm(X[5], 2.5e-8)      # clearly below / above the clamp
                c.X.append(X)
            if whole:
                xi = None
            elif nx >= 12:
                xi = _ids(rng, c.pattern if (c.pattern != "perm" or bt <= nx - 4) else "zipf", bt, nx, seed, cap)
            else:
                xi = rng.integers(0, nx, bt)
            if xi is not None and not c.exact and nx >= 12 and bt > 8 and c.pattern != "one":
                xi[1:4] = [3, 4, 5]
            ywhole = (k + t) % 2 == 0
            ny = max(bt if ywhole else _n_rows("zipf", bt), 1)
            Yt = tab(ny, lo=-3.0, hi=3.0, sign=ysign)
            if not c.exact and ny >= 12:
                Yt[2] = 0.0
                Yt[6] = _renorm(Yt[6], 0.4e-8)
            c.Y.append(Yt)
            c.ix.append(xi)
            c.iy.append(None if ywhole else rng.integers(0, ny, bt))
        c.w = [float(sc[(k + 1 + t) % 6]) for t in range(c.n_terms)]
        if not c.exact:
            c.w = [abs(w) + 0.25 for w in c.w]
        c.coef = [np.stack([_coefgrid(rng, bt), _coefgrid(rng, bt)], 1) // (2 if heavy else 1) for bt in c.batches] if c.exact else None
        c.null = ("none", "dX")[k % 2] if c.n_terms > 1 else "none"
    elif op in ("gather", "rows_reg"):
        c.mode = (k // 2) % 2 if op == "rows_reg" else 0
        c.n_terms = 1 + k % MAX_TERMS["rows_reg"] if op == "rows_reg" else 1
        c.batches = [B] + [(0, 37, B // 2 + 1, 300)[(k + t) % 4] for t in range(1, c.n_terms)]
        if op == "rows_reg" and k == 12:
            c.batches[0], c.pattern = WHOLE_TABLE, "perm"
        c.share = _share(k, c.n_terms)
        size = max(c.batches) * d                            # exact: sum k^2 < 2^24 over the largest term (entries k / 16)
        kk = 16 if size <= 2 ** 12 else (2 if size <= 2 ** 21 else 1)
        c.E, c.ids = [], []
        for t in range(c.n_terms):
            bt = c.batches[t]
            whole = op == "rows_reg" and ((k + t) % 3 == 1 or bt == WHOLE_TABLE)
            shared = t > 0 and c.share[t] == c.share[t - 1]
            gmax = max(b for b, j in zip(c.batches, c.share) if j == c.share[t])      # the largest term naming this table
            ne = c.E[-1].shape[0] if shared else max(bt if whole else 0, _n_rows(c.pattern, gmax) if gmax > bt or not whole else 0, 1)
            if shared and whole and ne != bt:
                whole = False
            if not shared:
                T = _grid(rng, (ne, d), kk) if c.exact else _rows(rng, ne, d, lo=-2.0, hi=2.0)
                if op == "rows_reg" and (k + t) % 5 == 4:
                    T[:] = 0.0                               # an all-zero term (mode 1: coef 0, not NaN)
                c.E.append(T)
            if whole:
                c.ids.append(None)
            elif ne >= 12:
                c.ids.append(_ids(rng, c.pattern if (c.pattern != "perm" or bt <= ne - 4) else "zipf", bt, ne, seed, cap))
            else:
                c.ids.append(rng.integers(0, ne, bt))
        if op == "gather":
            c.E[0] = poison(c.E[0], c.ids[0])
        c.coef = [float(x) or 0.5 for x in _coefgrid(rng, c.n_terms)] if c.exact else None
    elif op == "scatter":
        c.ids = ids()
        if B > 4:
            c.ids[rng.choice(B, max(B // 10, 1), replace=False)] = -1
        c.rows = tab(max(B, 1), sign=1.0)[:B]
        if c.nonfinite and B > 4:                            # named: rows that reach the table; not named: rows whose id is -1
            at = np.flatnonzero(c.ids >= 0 if c.nonfinite_named else c.ids < 0)
            c.rows[at[0], ::2], c.rows[at[-1], 1::3] = np.inf, np.nan
    elif op == "row_normalize":
        c.d = d = EW_WIDTHS[k % len(EW_WIDTHS)]
        c.eps = (1e-12, 1e-5)[k % 2]
        c.n = B if d < 4096 else min(B, 300)
        X = _rows(rng, max(c.n, 1), d, lo=-4.0, hi=4.0)[:c.n]
        if c.n >= 8:
            X[1] = 0.0
            for r, f in ((2, 0.4), (3, 2.5), (4, 0.01), (5, 4.0)):
                X[r] = _renorm(X[r], f * c.eps)
        c.X, c.G = X, _rows(rng, max(c.n, 1), d, lo=-2.0, hi=2.0)[:c.n]
    elif op == "cat_leaky":
        c.wa, c.wb = EW_WIDTHS[k % len(EW_WIDTHS)], EW_WIDTHS[(k + 3) % len(EW_WIDTHS)]
        c.n = B if max(c.wa, c.wb) < 4096 else min(B, 200)
        c.slope = (0.01, 0.2, -0.5, 0.0, 1.0 / 3.0)[k % 5]
        mk = lambda w: (rng.standard_normal((c.n, w)) * 10.0 ** rng.uniform(-6, 6, (c.n, 1))).astype(F32)      # noqa: E731
        c.A, c.B, c.dOut = mk(c.wa), mk(c.wb), mk(c.wa + c.wb)
        c.R = mk(c.wb) if k % 3 else None
        for T in (c.A, c.B):
            if T.size:
                T.flat[rng.choice(T.size, max(T.size // 20, 1))] = F32(0.0)
                T.flat[rng.choice(T.size, max(T.size // 20, 1))] = F32(-0.0)
        c.null = ("none", "dA", "dB", "dR")[k % 4]
    elif op == "infonce":
        c.batch = B = NCE_BATCHES[k % len(NCE_BATCHES)]
        c.d, c.tau = 64, TAUS[k % len(TAUS)]
        c.pattern = PATTERNS[k % 3]
        c.n_rows = n = _n_rows(c.pattern, B)
        c.ids = _ids(rng, c.pattern, B, n, seed, 256)
        c.E1 = _rows(rng, n, 64, lo=-3.0, hi=3.0, sign=1.0)
        c.E2 = (0.5 * _rows(rng, n, 64, lo=0.0, hi=0.0, sign=1.0) + 0.5 * c.E1 / np.linalg.norm(c.E1, axis=1, keepdims=True)).astype(F32)
        c.E2 *= (10.0 ** rng.uniform(-3, 3, (n, 1))).astype(F32)
        c.sparse = c.tau < 0.5 or B > 1024
        if c.sparse:                                         # 8 non-zero entries per row: one of the row's size in a column of the
            for T, half in ((c.E1, 0), (c.E2, 32)):          # view's own half, seven 30 times smaller anywhere -- nearly orthogonal
                nr = np.linalg.norm(T.astype(F64), axis=1)   # rows: small logits, short chains (magnitudes are chosen, module docstring)
                keep = np.argsort(rng.random((n, 64)), axis=1)[:, :7]
                mask = np.zeros((n, 64), bool)
                np.put_along_axis(mask, keep, True, axis=1)
                T[~mask] = 0.0
                T *= F32(1.0 / 30.0)
                T[np.arange(n), half + rng.integers(0, 32, n)] = nr.astype(F32)
        if B >= 8 and c.pattern != "one":
            named = np.unique(c.ids)
            z, lo_, hi_ = named[0], named[len(named) // 2], named[-1]
            c.E1[z] = 0.0
            c.E1[lo_], c.E2[hi_] = _renorm(c.E1[lo_], 0.4e-12), _renorm(c.E2[hi_], 4e-12)      # below the clamp / above it
            c.below = int(lo_)
        c.null = ("none", "dE1", "dE2")[k % 3]
    return c


# ------------------------------------------------------------------------------------------------ the ops in float64 (and fp32)
def ev_bpr_fwd(c, t, dt, plant=None, from_dots=None):
    """per term: x, l, c and the loss with tolerances"""
    B, d = c.batch, c.d
    P = c.I[c.share[t]]
    N = P if (c.op == "bpr_multi" or c.same_pn) else c.I[-1]
    if from_dots is None:
        p, Mp = dots(c.U, c.users, P, c.pos[t])
        q, Mq = dots(c.U, c.users, N, c.neg[t])
        with np.errstate(invalid="ignore", over="ignore"):
            x = rnd(rnd(p, dt) - rnd(q, dt), dt)
            dx = gamma(ndot(d) + 1) * (Mp + Mq) + TINY * 8
    else:
        with np.errstate(invalid="ignore", over="ignore"):
            x = rnd(from_dots[:B].astype(F64) - from_dots[B:].astype(F64), dt)
            dx = U * np.abs(x) + TINY
    l, cf, tl, tc = bpr_eval(x, dx, c.variant, dt)
    n = nsum_blocks(B) if c.op == "bpr_multi" else nsum_plain(B)
    drop = None
    if plant == "last_block" and B:
        drop = np.arange(16 * ((B - 1) // 16), B)
    if plant == "beyond_256" and B > 4096:
        drop = np.arange(4096, B)
    scale = c.scale * {"scale_twice": c.scale, "scale_never": 1.0 / c.scale}.get(plant, 1.0)
    loss, tloss = total(l, tl, n, scale, dt, drop)
    return dict(x=x, l=l, coef=cf, tcoef=tc, loss=loss, tloss=tloss, P=P, N=N)


def ev_cos_fwd(c, t, dt, plant=None):
    X, Y, ix, iy, B = c.X[c.share[t]], c.Y[t], c.ix[t], c.iy[t], c.batches[t]
    d = c.d
    if ix is None:
        X = X[:B]
    if iy is None:
        Y = Y[:B]
    xy, Mxy = dots(X, ix, Y, iy)
    xx, _ = dots(X, ix, X, ix)
    yy, _ = dots(Y, iy, Y, iy)
    xy, xx, yy = rnd(xy, dt), rnd(xx, dt), rnd(yy, dt)
    nx, ny = fn(np.sqrt, dt, xx), fn(np.sqrt, dt, yy)
    cx, cy = np.maximum(nx, EPS_COS), np.maximum(ny, EPS_COS)
    with np.errstate(all="ignore"):
        inv = rnd(1.0 / rnd(cx * cy, dt), dt)
        cs = rnd(xy * inv, dt)
        cyv = np.where(nx > EPS_COS, rnd(cs / rnd(cx * cx, dt), dt), 0.0)
        if plant == "coef_y_on_clamped":
            cyv = rnd(cs / rnd(cx * cx, dt), dt)
    coef = np.stack([inv, cyv], 1)
    tcoef = tcs = None
    if dt is F64:
        gd = gamma(ndot(d))
        rx = np.where(nx > EPS_COS, gd / 2 + (E_DIV + 1) * U, 0.0)       # relative error of max(norm, 1e-8)
        ry = np.where(ny > EPS_COS, gd / 2 + (E_DIV + 1) * U, 0.0)
        tinv = np.abs(inv) * (rx + ry + (E_DIV + 2) * U)
        tcs = gd * Mxy * np.abs(inv) + np.abs(xy) * tinv + U * np.abs(cs) + TINY
        tcy = np.where(nx > EPS_COS, tcs / (cx * cx) + np.abs(cyv) * (2 * rx + (E_DIV + 2) * U), 0.0)
        tcoef = np.stack([tinv + TINY, tcy + TINY], 1)
    return dict(cs=cs, tcs=tcs, coef=coef, tcoef=tcoef, Xg=X if ix is None else X[ix], Yg=Y if iy is None else Y[iy])


def ev_sq(c, t, dt):
    """S_t = sum_b ||E[ids[b]]||^2: per-row squares and their sum's tolerance"""
    E, ids, B = c.E[c.share[t]], c.ids[t], c.batches[t]
    Eg = E[:B] if ids is None else E[ids]
    sq, _ = dots(Eg, None, Eg, None)
    sq = rnd(sq, dt)
    n = nsum_blocks(B) if c.op == "rows_reg" else nsum_plain(B)
    with np.errstate(invalid="ignore", over="ignore"):
        S, tS = total(sq, gamma(ndot(c.d)) * sq, n, 1.0, dt)
    return Eg, S, tS


def ev_normalize(X, eps, dt):
    """Y, inv (signed: negative where the clamp is active), norms"""
    X64 = X.astype(F64)
    ss = rnd((X64 * X64).sum(1), dt)
    nrm = fn(np.sqrt, dt, ss)
    with np.errstate(all="ignore"):
        r = rnd(1.0 / np.maximum(nrm, eps), dt)
        Y = rnd(X64 * r[:, None], dt)
    return Y, np.where(nrm > eps, r, -r), nrm


def ev_normalize_bwd(Y, G, inv, dt, plant=None):
    """dX = |inv| (G - Y (Y . G)) (clamp active: |inv| G) from GIVEN fp32 Y, G, inv, with its tolerance"""
    Y, G, inv = Y.astype(F64), G.astype(F64), inv.astype(F64)
    proj = inv > 0 if plant != "project_clamped" else np.ones(inv.shape, bool)
    with np.errstate(all="ignore"):
        yg = np.where(proj, rnd((Y * G).sum(1), dt), 0.0)
        dX = rnd(np.abs(inv)[:, None] * rnd(G - rnd(Y * yg[:, None], dt), dt), dt)
        M = np.abs(inv)[:, None] * (np.abs(G) + np.abs(Y) * (np.abs(Y) * np.abs(G)).sum(1)[:, None] * proj[:, None])
    return dX, gamma(ndot(Y.shape[1]) + 4) * M + 8 * TINY


def ev_cat_leaky(c):
    """bit-exact reference: float64 products are exact, every fp32 operation is one rounding of a float64 result"""
    s = F64(F32(c.slope))
    with np.errstate(all="ignore"):
        leaky = lambda a: np.where(a > 0, a, (a.astype(F64) * s).astype(F32)).astype(F32)      # noqa: E731
        right = leaky(c.B) if c.R is None else (leaky(c.B).astype(F64) + c.R.astype(F64)).astype(F32)
        out = np.concatenate([leaky(c.A), right], 1)
        grad = lambda a, g: np.where(a > 0, g, (g.astype(F64) * s).astype(F32)).astype(F32)      # noqa: E731
        dA, dB = grad(c.A, c.dOut[:, :c.wa]), grad(c.B, c.dOut[:, c.wa:])
    return out, dA, dB, c.dOut[:, c.wa:].copy()


def ev_infonce(c, dt, plant=None, block=512):
    """loss, per-sample gradient rows [B, 64] of both views (before the scatter) and their tolerances, row-blocked float64.
    A logit's error is (gamma(m + 1) + 2 rv + 2 u) sum_k |v1_k v2_k| / tau with m the largest number of non-zero entries of a
    row (an fma whose product is exactly 0 rounds nothing), rv the relative error of a normalised row; log ttl_i carries the
    p-weighted mean of its logits' errors; a gradient column k is a chain of at most min(nnz of that column, nce_chain) fmas"""
    B, g = c.batch, c.g
    X1, X2 = c.E1[c.ids], c.E2[c.ids]
    V1, inv1, _ = ev_normalize(X1, EPS_NRM, dt)
    V2, inv2, _ = ev_normalize(X2, EPS_NRM, dt)
    itau = float(F32(1.0) / F32(c.tau))
    m = int(max((X1 != 0).sum(1).max(), (X2 != 0).sum(1).max(), 1))
    rv = gamma(min(m, 8)) / 2 + (2 * E_DIV + 2) * U                  # relative error of a normalised row
    kdot = (gamma(m + 1) + 2 * rv + 2 * U) * itau                    # x sum |v1 v2|: the error of a logit
    tiles = -(-B // 64)
    ttl_chain = 4 * -(-tiles // 4) + 8
    lossi, d1, d2 = np.zeros(B), np.zeros((B, 64)), np.zeros((B, 64))
    tli = np.zeros(B)
    M1, M2, T1, T2 = (np.zeros((B, 64)) for _ in range(4))
    gs = F64(F32(g)) * itau / B
    A1, A2 = np.abs(V1), np.abs(V2)
    for b0 in range(0, B, block):
        sl = slice(b0, min(B, b0 + block))
        rr, cc = np.arange(sl.stop - b0), np.arange(b0, sl.stop)
        S = rnd(V1[sl] @ V2.T, dt) * itau
        e = fn(np.exp, dt, S)
        ttl = rnd(e.sum(1), dt)
        lossi[sl] = fn(lambda a, t_: -np.log(np.exp(a) / t_), dt, S[rr, cc], ttl)
        p = e / ttl[:, None]
        G = p.copy()
        if plant != "no_diagonal":
            G[rr, cc] -= 1.0
        G = rnd(gs * G, dt)
        d1[sl] = rnd(G @ V2, dt)
        d2 += G.T @ V1[sl]
        if dt is F64:
            DS = kdot * (A1[sl] @ A2.T)
            avg = (p * DS).sum(1)                                    # the error of log ttl_i
            tli[sl] = DS[rr, cc] + avg + gamma(ttl_chain) + (2 * E_NCE + 2) * U * (1.0 + np.abs(lossi[sl]))
            TG = np.abs(gs) * p * (DS + avg[:, None] + gamma(ttl_chain) + (2 * E_NCE + 4) * U)
            M1[sl], T1[sl] = np.abs(G) @ A2, TG @ A2
            M2 += np.abs(G).T @ A1[sl]
            T2 += TG.T @ A1[sl]
    d2 = rnd(d2, dt)
    loss, _ = total(lossi, None, nsum_plain(B), 1.0 / B, dt)
    out = dict(loss=loss, tloss=None)
    t1 = t2 = None
    if dt is F64:
        out["tloss"] = float(np.sum(tli) / B + gamma(nsum_plain(B)) * np.sum(np.abs(lossi)) / B)
        n1 = np.minimum((V2 != 0).sum(0), nce_chain(B)) + 7          # per gradient column: fmas with a non-zero product
        n2 = np.minimum((V1 != 0).sum(0), nce_chain(B)) + 7
        t1 = T1 + (gamma(n1)[None, :] + rv) * M1
        t2 = T2 + (gamma(n2)[None, :] + rv) * M2
    rows = []
    for V, inv, dv, tv in ((V1, inv1, d1, t1), (V2, inv2, d2, t2)):
        proj = inv > 0 if plant != "project_clamped" else np.ones(B, bool)
        with np.errstate(all="ignore"):
            vd = np.where(proj, rnd((V * dv).sum(1), dt), 0.0)
            r = rnd((dv - V * vd[:, None]) * np.abs(inv)[:, None], dt)
            tol = None
            if dt is F64:
                a, absV = np.abs(inv)[:, None], np.abs(V)
                tol = a * (tv + absV * ((absV * tv).sum(1) * proj)[:, None]) \
                    + (gamma(12) + 3 * rv) * a * (np.abs(dv) + absV * ((absV * np.abs(dv)).sum(1) * proj)[:, None]) + 8 * TINY
        rows.append((r, tol))
    out["rows"] = rows
    return out


def _prefill(c, name, n_rows, d):
    """what a gradient table holds before the launch: zeros, or non-zero grid values (exact) / normal values (float)"""
    if c.zero_pre:
        return np.zeros((n_rows, d), F32)
    rng = np.random.default_rng([c.seed, sum(map(ord, name))])
    if c.exact:
        return ((rng.integers(1, 9, (n_rows, d)) / 8.0) * rng.choice([-1.0, 1.0], (n_rows, d))).astype(F32)
    return (rng.standard_normal((n_rows, d)) * 1e-3).astype(F32)


def evaluate(c, dt=F64, plant=None):
    """every output of the case's op: name -> (value, tol, kind), kind in {"scalar", "vector", "table"}; dt = F32: the fp32
    restatement (values only), optionally with a planted error.  Fills c.pre (the tables' pre-fill) and c.exact_tables."""
    op, d, ex = c.op, c.d, c.exact
    out = {}
    c.pre = {}
    c.exact_tables = ex
    pre = lambda name, rows, w=d: c.pre.setdefault(name, _prefill(c, name, rows, w))      # noqa: E731
    tb = lambda nm, nr, lst, chain: table(nr, d, pre(nm, nr), lst, chain, dt, plant, c.exact_tables, nm + " " + c.axes()) + ("table",)      # noqa: E731
    if op in ("bpr", "bpr_dots", "bpr_multi"):
        nu = c.U.shape[0]
        fw = []
        for t in range(c.n_terms):
            fd = None
            if op == "bpr_dots":
                P = c.I[0]
                N = P if c.same_pn else c.I[-1]
                p, Mp = dots(c.U, c.users, P, c.pos[0])
                q, Mq = dots(c.U, c.users, N, c.neg[0])
                dd = np.concatenate([p, q])
                with np.errstate(invalid="ignore"):
                    out["dots"] = (rnd(dd, dt), gamma(ndot(d)) * np.concatenate([Mp, Mq]) + 8 * TINY, "vector")
                if ex:
                    _on_grid(np.concatenate([Mp, Mq]), 2.0 ** -8, c.axes())
                with np.errstate(over="ignore", invalid="ignore"):
                    fd = dd.astype(F32)                      # the dots the test hands to loss_from_dots
                c.given_dots = fd
            f = ev_bpr_fwd(c, t, dt, plant, fd)
            fw.append(f)
            out["coef%d" % t] = (f["coef"], f["tcoef"], "vector")
            out["loss%d" % t] = (f["loss"], f["tloss"], "scalar")
        if op == "bpr_multi":
            w = list(c.w)
            if plant == "wrong_weight" and c.n_terms > 1:
                w = w[1:] + w[:1]
            tot = rnd(sum(rnd(F64(F32(w[t])) * fw[t]["loss"], dt) for t in range(c.n_terms)), dt)
            ttot = None if dt is F32 else sum(abs(w[t]) * (fw[t]["tloss"] + 3 * U * abs(fw[t]["loss"])) for t in range(c.n_terms)) + TINY
            out["total"] = (float(tot), ttot, "scalar")
        # backward: test-supplied grid coef (exact) or the forward's own (float: its tolerance carried)
        gsc = F64(F32(c.g)) * F64(F32(c.scale))
        cu, ci = [], {}
        for t in range(c.n_terms):
            f = fw[t]
            wt = F64(F32(c.w[t])) if op == "bpr_multi" else 1.0
            cf = c.coef[t].astype(F64) if ex else f["coef"]
            tc = None if (ex or dt is F32) else np.abs(gsc * wt) * f["tcoef"]
            cc = gsc * wt * cf
            Pg, Ng, Ug = f["P"][c.pos[t]].astype(F64), f["N"][c.neg[t]].astype(F64), c.U[c.users].astype(F64)
            with np.errstate(invalid="ignore", over="ignore"):
                cu.append((c.users, cc, Pg - Ng, tc))
            jp = c.share[t]
            jn = jp if (op == "bpr_multi" or c.same_pn) else len(c.I) - 1
            ci.setdefault(jp, []).append((c.pos[t], cc, Ug, tc))
            ci.setdefault(jn, []).append((c.neg[t], cc if plant == "dN_sign" else -cc, Ug, tc))
        out["dU"] = tb("dU", nu, cu, 5)
        for j, lst in ci.items():
            out["dI%d" % j] = tb("dI%d" % j, c.I[j].shape[0], lst, 5)
    elif op in ("cosine", "cosine_multi"):
        fw = [ev_cos_fwd(c, t, dt, plant) for t in range(c.n_terms)]
        if op == "cosine_multi":
            c.exact_tables = ex and all(b & (b - 1) == 0 for b in c.batches)
        gq = F64(F32(c.g))
        terms, tterms, contribs = [], [], {}
        for t, f in enumerate(fw):
            bt = c.batches[t]
            if op == "cosine":
                scale = c.scale * (c.scale if plant == "scale_twice" else 1.0)
                val, tol = total(f["cs"], f["tcs"], nsum_plain(bt), scale, dt,
                                 np.arange(16 * ((bt - 1) // 16), bt) if plant == "last_block" and bt else None)
                out["out"] = (val, tol, "scalar")
                fac = gq * F64(F32(c.scale))
            else:
                mean_scale = 1.0 / max(bt, 1)
                if plant == "scale_twice":
                    mean_scale *= mean_scale
                val, tol = total(f["cs"], f["tcs"], nsum_blocks(bt), mean_scale, dt)
                terms.append(float(rnd(F64(F32(c.w[t])) * val, dt)))
                tterms.append(None if dt is F32 else abs(c.w[t]) * (tol + 3 * U * abs(val)))
                fac = float(rnd(rnd(gq * F64(F32(c.w[t])), dt) / max(bt, 1), dt))
            out["coef%d" % t] = (f["coef"], f["tcoef"], "vector")
            cf = c.coef[t].astype(F64) if ex else f["coef"]
            tcf = None if (ex or dt is F32) else f["tcoef"]
            ids = np.arange(bt) if c.ix[t] is None else c.ix[t]
            with np.errstate(invalid="ignore", over="ignore"):
                lst = contribs.setdefault(c.share[t], [])
                lst.append((ids, fac * cf[:, 0], f["Yg"].astype(F64), None if tcf is None else abs(fac) * tcf[:, 0]))
                lst.append((ids, -fac * cf[:, 1], f["Xg"].astype(F64), None if tcf is None else abs(fac) * tcf[:, 1]))
        if op == "cosine_multi":
            out["out"] = (float(rnd(sum(terms), dt)),
                          None if dt is F32 else sum(tterms) + gamma(c.n_terms) * sum(abs(x) for x in terms) + TINY, "scalar")
        for j, lst in contribs.items():
            out["dX%d" % j] = tb("dX%d" % j, c.X[j].shape[0], lst, 6)
    elif op in ("gather", "rows_reg"):
        parts, tparts, contribs = [], [], {}
        gq, sc32 = F64(F32(c.g)), F64(F32(c.scale))
        coefs, tcoefs = [], []
        for t in range(c.n_terms):
            Eg, S, tS = ev_sq(c, t, dt)
            if ex:
                _on_grid((Eg.astype(F64) ** 2).sum(), 2.0 ** -8, c.axes())
            if op == "gather" or c.mode == 0:
                parts.append(S), tparts.append(tS)
                kc, tk = 2.0 * sc32, 0.0
            else:
                nrm = float(fn(np.sqrt, dt, S))
                parts.append(nrm), tparts.append(None if dt is F32 else (0.5 * tS / nrm if nrm > 0 else 0.0) + E_DIV * U * nrm)
                with np.errstate(all="ignore"):
                    kc = float(rnd(sc32 / nrm, dt)) if S > 0 else 0.0
                    if plant == "zero_term_coef" and not S > 0:
                        kc = float("nan")
                tk = 0.0 if (dt is F32 or not S > 0) else abs(kc) * (0.5 * tS / S + (E_DIV + 1) * U)
            coefs.append(kc), tcoefs.append(tk)
            if op == "gather":
                kk, tkk = (c.coef[0] if ex else gq), 0.0          # gather_scale_add: the test's device scalar
            else:
                kk = float(rnd(gq * (c.coef[t] if ex else kc), dt))
                tkk = 0.0 if ex else abs(gq) * tk
            ids = np.arange(c.batches[t]) if c.ids[t] is None else c.ids[t]
            contribs.setdefault(c.share[t], []).append((ids, np.full(ids.size, float(kk)), Eg.astype(F64),
                                                        None if dt is F32 else np.full(ids.size, float(tkk))))
        if op == "gather":
            out["out"] = (parts[0], tparts[0], "scalar")
        else:
            tot = rnd(sc32 * rnd(sum(parts), dt), dt)
            out["out"] = (float(tot), None if dt is F32 else abs(sc32) * (sum(tparts) + gamma(c.n_terms + 1) * sum(abs(p) for p in parts))
                          + TINY, "scalar")
            out["coef"] = (np.array(coefs), np.array(tcoefs) + TINY, "vector")
        for j, lst in contribs.items():
            out["dE%d" % j] = tb("dE%d" % j, c.E[j].shape[0], lst, 3)
    elif op == "scatter":
        keep = c.ids >= 0
        out["out"] = tb("out", c.n_rows, [(c.ids[keep], np.ones(int(keep.sum())), c.rows[keep].astype(F64), None)], 1)
    elif op == "row_normalize":
        eps = float(F32(c.eps))
        Y, inv, nrm = ev_normalize(c.X, eps, dt)
        rr = np.where(nrm > eps, gamma(ndot(d)) / 2 + (2 * E_DIV + 1) * U, (E_DIV + 1) * U)
        out["Y"] = (Y, None if dt is F32 else (rr + U)[:, None] * np.abs(Y) + TINY, "vector")
        out["inv"] = (inv, None if dt is F32 else rr * np.abs(inv), "vector")
    elif op == "infonce":
        r = ev_infonce(c, dt, plant)
        out["loss"] = (r["loss"], r["tloss"], "scalar")
        for nm, (rows, tol) in zip(("dE1", "dE2"), r["rows"]):
            p0 = pre(nm, c.n_rows, 64)
            if dt is F32:
                o = np.zeros((c.n_rows, 64), F32) if plant == "store_prefill" else p0.copy()
                np.add.at(o, c.ids, rows.astype(F32))
                out[nm] = (o.astype(F64), None, "table")
            else:
                ref, T, cnt = p0.astype(F64).copy(), np.zeros((c.n_rows, 64)), np.zeros(c.n_rows)
                M = np.abs(ref)
                np.add.at(ref, c.ids, rows), np.add.at(M, c.ids, np.abs(rows)), np.add.at(T, c.ids, tol), np.add.at(cnt, c.ids, 1)
                out[nm] = (ref, gamma(cnt + 1)[:, None] * M + T, "table")
    return out


def _compare(c, ref, got, names=None):
    """every output of `got` (name -> (value, ...)) against `ref`; returns the worst err / tol"""
    worst = 0.0
    for nm, (val, tol, kind) in ref.items():
        if (names is not None and nm not in names) or nm not in got:
            continue
        exact = (kind == "table" and c.exact_tables) or (c.exact and (
            nm == "dots" or (nm == "out" and c.op == "gather") or (nm in ("out", "coef") and c.op == "rows_reg" and c.mode == 0)))
        worst = max(worst, check(got[nm][0], val, tol, exact, "%s [%s]" % (nm, c.axes())))
    return worst


# ------------------------------------------------------------------------------------------------ CPU: the checker and the cases
def _find(cond):
    for s in range(CASES):
        c = draw_case(s)
        if cond(c):
            return c
    raise AssertionError("no such case")


def _rejects(c, ref, plant=None, mutate=None, names=None):
    got = evaluate(c, F32, plant)
    if mutate is not None:
        mutate(got)
    with pytest.raises(AssertionError):
        _compare(c, ref, got, names)


def measure_E():
    """worst error, in units of u |value|, of the fp32 numpy evaluation of each function group at the fp32-rounded float64
    arguments of every float case (values below 2^-100 excluded: FLOOR is theirs)"""
    worst = {"bpr": 0.0, "sig": 0.0, "div": 0.0, "nce": 0.0}

    def units(v32, v64):
        with np.errstate(all="ignore"):
            ok = np.isfinite(v64) & (np.abs(v64) > 2.0 ** -100)
            return float((np.abs(v32 - v64)[ok] / (U * np.abs(v64[ok]))).max()) if ok.any() else 0.0

    for s in range(CASES):
        c = draw_case(s)
        if c.exact:
            continue
        with np.errstate(all="ignore"):
            if c.op in ("bpr", "bpr_dots", "bpr_multi"):
                for t in range(c.n_terms):
                    x = ev_bpr_fwd(c, t, F64)["x"]
                    x = x[np.isfinite(x)].astype(F32)
                    if c.variant == 0:
                        for a, b in zip(bpr_scalar(x, 0), bpr_scalar(x.astype(F64), 0)):
                            worst["bpr"] = max(worst["bpr"], units(a.astype(F64), b))
                    else:
                        worst["sig"] = max(worst["sig"], units((F32(1) / (F32(1) + np.exp(-x))).astype(F64),
                                                               1.0 / (1.0 + np.exp(-x.astype(F64)))))
            elif c.op in ("row_normalize", "cosine", "cosine_multi"):
                X = c.X if c.op == "row_normalize" else c.X[0]
                ss = (X.astype(F64) ** 2).sum(1).astype(F32)
                ss = ss[ss > 0]
                worst["div"] = max(worst["div"], units(np.sqrt(ss).astype(F64), np.sqrt(ss.astype(F64))),
                                   units((F32(1) / np.sqrt(ss)).astype(F64), 1.0 / np.sqrt(ss).astype(F64)))
            elif c.op == "infonce":
                a = np.random.default_rng(s).uniform(-1.0, 1.0, 4096).astype(F32) * F32(1.0 / c.tau)
                worst["nce"] = max(worst["nce"], units(np.exp(a).astype(F64), np.exp(a.astype(F64))),
                                   units(np.log(np.exp(a)).astype(F64), np.log(np.exp(a).astype(F64))))
    return worst


def test_E_is_four_times_the_measured_worst():
    worst = measure_E()
    print("measured worst error in units of u |value|:", worst)
    for key, E in (("bpr", E_BPR), ("sig", E_SIG), ("div", E_DIV), ("nce", E_NCE)):
        assert E >= 4.0 and 4.0 * worst[key] <= E, (key, worst[key], E)
        assert E == 4.0 or E <= 8.0 * worst[key], (key, "E above twice what the rule gives", worst[key], E)


def test_checker_rejects_planted_errors():
    """the fp32 numpy restatement of each op passes the checker on every case; each planted error is rejected"""
    for s in range(CASES):
        c = draw_case(s)
        if c.op != "cat_leaky":
            _compare(c, evaluate(c), evaluate(c, F32))
    # reductions: the last partial block of 16 missing; partial blocks beyond the 256th missing; 1 / B twice or not at all
    c = _find(lambda c: c.op == "bpr" and not c.exact and c.batch == 4097 and not c.nonfinite)
    ref = evaluate(c)
    for plant in ("scale_twice", "scale_never"):
        if c.scale != 1.0:
            _rejects(c, ref, plant, names=("loss0",))
    for batch, plant in ((255, "last_block"), (257, "last_block"), (8193, "beyond_256")):
        c2 = _find(lambda c: c.op in ("bpr", "bpr_multi", "bpr_dots") and not c.exact and c.batch == batch and not c.nonfinite)
        _rejects(c2, evaluate(c2), plant, names=("loss0",))
    _rejects(c, ref, mutate=lambda g: g.__setitem__("loss0", (g["loss0"][0] * (1 + 1e-4),)), names=("loss0",))   # 1e-4 of a loss

    def one_coef(g):                                          # a 1e-4 relative error in one coef of a 4097-sample batch
        v = g["coef0"][0].copy()
        i = int(np.argmax(np.abs(v)))
        v[i] *= 1 + 1e-4
        g["coef0"] = (v,)
    _rejects(c, ref, mutate=one_coef, names=("coef0",))
    c = _find(lambda c: c.op == "cosine" and not c.exact and c.batch >= 255 and c.ix[0] is not None and c.pattern != "one")
    ref = evaluate(c)
    _rejects(c, ref, "last_block", names=("out",))
    _rejects(c, ref, "coef_y_on_clamped", names=("coef0",))   # the cosine coef.y not zeroed on a clamped row
    c = _find(lambda c: c.op == "cosine_multi" and not c.exact and c.n_terms >= 2 and c.batches[0] > 16)
    _rejects(c, evaluate(c), "scale_twice", names=("out",))
    # a term's weight applied to the wrong term
    c = _find(lambda c: c.op == "bpr_multi" and not c.exact and c.n_terms >= 2 and c.batch > 16 and len(set(c.w)) > 1 and not c.nonfinite and c.pattern != "one")
    _rejects(c, evaluate(c), "wrong_weight", names=("total",))
    # scatters, exact mode: dN with dP's sign; the second occurrence of a duplicated id lost; a store where += belongs
    c = _find(lambda c: c.op == "bpr" and c.exact and c.pattern != "perm" and 255 <= c.batch <= 4097 and c.g != 0)
    ref = evaluate(c)
    for plant in ("dN_sign", "store_dup", "store_prefill"):
        _rejects(c, ref, plant)
    for op in ("cosine", "gather", "rows_reg", "scatter", "bpr_multi", "cosine_multi"):
        c = _find(lambda c: c.op == op and c.exact and c.pattern != "perm" and 255 <= c.batch <= 4097 and (c.g != 0 or op == "scatter"))
        ref = evaluate(c)
        _rejects(c, ref, "store_dup")
        _rejects(c, ref, "store_prefill")
    # rows_reg mode 1: coef NaN for an all-zero term
    c = _find(lambda c: c.op == "rows_reg" and not c.exact and c.mode == 1 and any(
        not np.any(c.E[c.share[t]][:c.batches[t]] if c.ids[t] is None else c.E[c.share[t]][c.ids[t]]) for t in range(c.n_terms)))
    _rejects(c, evaluate(c), "zero_term_coef", names=("coef",))
    # the projected form of the normalisation backward on a clamped, non-zero row: row_normalize and InfoNCE
    c = _find(lambda c: c.op == "row_normalize" and c.n >= 255 and c.d >= 64)
    Y, inv, _ = ev_normalize(c.X, float(F32(c.eps)), F32)
    ref, tol = ev_normalize_bwd(Y.astype(F32), c.G, inv.astype(F32), F64)
    check_float(ev_normalize_bwd(Y.astype(F32), c.G, inv.astype(F32), F32)[0], ref, tol, "row_normalize_bwd restated")
    with pytest.raises(AssertionError):
        check_float(ev_normalize_bwd(Y.astype(F32), c.G, inv.astype(F32), F32, "project_clamped")[0], ref, tol, "planted")
    c = _find(lambda c: c.op == "infonce" and 255 <= c.batch <= 333 and c.g != 0 and hasattr(c, "below"))
    ref = evaluate(c)
    _rejects(c, ref, "project_clamped")
    _rejects(c, ref, "no_diagonal")                           # the [i = j] term missing from g_ij
    _rejects(c, ref, "store_prefill")
    # a wrong non-finite pattern
    c = _find(lambda c: c.op == "bpr" and c.nonfinite_named and c.batch >= 16)
    ref = evaluate(c)
    assert not np.isfinite(ref["coef0"][0]).all()

    def finite_where_nan(g):
        v = g["coef0"][0].copy()
        v[~np.isfinite(v)] = 0.0
        g["coef0"] = (v,)
    _rejects(c, ref, mutate=finite_where_nan, names=("coef0",))

    def nan_where_finite(g):
        v = g["dU"][0].copy()
        v[tuple(np.argwhere(np.isfinite(v))[0])] = np.nan
        g["dU"] = (v,)
    _rejects(c, ref, mutate=nan_where_finite, names=("dU",))


def test_tolerances_stay_sharp():
    """the two sharpness conditions of the module docstring, for EVERY float case, from the float64 side alone (tables: the
    run on a zero-filled buffer)"""
    for s in range(CASES):
        c = draw_case(s)
        if c.exact:
            continue
        c.zero_pre = True
        for nm, (val, tol, kind) in evaluate(c).items():
            if kind == "scalar":
                sharp_scalar(val, tol, "%s [%s]" % (nm, c.axes()))
            elif kind == "table" and c.g != 0 and not (c.op == "infonce" and c.pattern == "one"):
                sharp_table(val, tol, "%s [%s]" % (nm, c.axes()))      # (InfoNCE on one id: identical rows, gradient exactly 0)


def _id_lists(c):
    """(id list drawn by `_ids`, rows of its table) of the case's main batch"""
    if c.op in ("bpr", "bpr_dots", "bpr_multi"):
        return [(i, c.n_rows) for i in [c.users] + c.pos + c.neg]
    if c.op in ("cosine", "cosine_multi"):
        return [(c.ix[0], c.X[0].shape[0])] if c.ix[0] is not None and c.batches[0] <= c.X[0].shape[0] - 4 else []
    if c.op in ("gather", "rows_reg"):
        return [(c.ids[0], c.E[0].shape[0])] if c.ids[0] is not None and c.batches[0] <= c.E[0].shape[0] - 4 else []
    if c.op == "scatter":
        return []                                            # (ids overwritten with -1 at random positions)
    if c.op == "infonce":
        return [(c.ids, c.n_rows)]
    return []


def test_cases_span_every_axis():
    seen = {k: set() for k in ("batch", "d", "terms", "pattern", "tau", "eps", "nce_batch", "null", "g", "variant", "mode",
                               "ids_null", "zero_len", "shared", "same_pn", "nonfinite", "whole", "ew", "minus1", "iy_null", "same_pn_mode",
                               "scale_sign", "w_sign", "below", "ends", "clamp_rows")}
    for s in range(CASES):
        c = draw_case(s)
        assert draw_case(s).axes() == c.axes()
        if c.op == "infonce":
            seen["nce_batch"].add(c.batch), seen["tau"].add(c.tau)
        elif c.op in ("row_normalize", "cat_leaky"):
            seen["ew"].update((c.d,) if c.op == "row_normalize" else (c.wa, c.wb))
            if c.op == "row_normalize":
                seen["eps"].add(c.eps)
        else:
            seen["batch"].add((c.batch, c.exact)), seen["d"].add((c.d, c.exact)), seen["pattern"].add((c.pattern, c.exact))
        seen["g"].add(float(np.sign(c.g)) if c.g in (0.0, 1.0) or c.g < 0 else 2.0)
        if c.op in MAX_TERMS:
            seen["terms"].add((c.op, c.n_terms))
            seen["shared"].add(len(set(c.share)) < c.n_terms)
            if c.op != "bpr_multi":
                seen["zero_len"].add(0 in c.batches), seen["whole"].add(max(c.batches) >= 39387)
                seen["ids_null"].update(i is None for i in (c.ids if c.op == "rows_reg" else c.ix))
        if hasattr(c, "null"):
            seen["null"].add((c.op, c.null))
        if hasattr(c, "variant"):
            seen["variant"].add((c.variant, c.exact))
        if c.op == "rows_reg":
            seen["mode"].add((c.mode, c.exact))
        if hasattr(c, "same_pn") and c.op != "bpr_multi":
            seen["same_pn"].add(c.same_pn)
        if c.nonfinite:
            seen["nonfinite"].add(c.nonfinite_named)
        if c.op == "scatter":
            seen["minus1"].add(bool((c.ids < 0).any()))
        seen["scale_sign"].add(float(np.sign(c.scale)))
        seen["w_sign"].update(float(np.sign(w)) for w in getattr(c, "w", []))
        if c.op in ("cosine", "cosine_multi"):
            seen["iy_null"].update(i is None for i in c.iy)
            if not c.exact:                                  # an exact zero row, a row below and a row above the 1e-8 clamp
                n0 = np.linalg.norm(c.X[0].astype(F64), axis=1)
                seen["clamp_rows"].add(c.X[0].shape[0] < 12 or (n0[3] == 0 and 0 < n0[4] <= EPS_COS / 2 and 2 * EPS_COS <= n0[5] < 4 * EPS_COS))
        if c.op == "row_normalize" and c.n >= 8:
            n0 = np.linalg.norm(c.X.astype(F64), axis=1)
            seen["clamp_rows"].add(bool(n0[1] == 0 and 0 < n0[2] <= c.eps / 2 and n0[3] >= 2 * c.eps and 0 < n0[4] <= c.eps / 2))
            assert ((n0 == 0) | (n0 <= c.eps / 2) | (n0 >= 2 * c.eps)).all(), "a row between clamp / 2 and 2 clamp"
        if c.op == "infonce" and c.batch >= 8 and c.pattern != "one":
            n1 = np.linalg.norm(c.E1[c.below].astype(F64))
            seen["below"].add(bool(0 < n1 <= EPS_NRM / 2 and c.below in c.ids))
        if c.op in ("bpr", "bpr_dots"):
            seen["same_pn_mode"].add((c.same_pn, c.exact))
        # the first and the last row of the table named (pattern "one": one of them), rows 1 and n - 2 never
        for lst, rows in _id_lists(c):
            if lst.size >= 2 and rows >= 12:
                hit = {0, rows - 1} & set(lst.tolist())
                seen["ends"].add(len(hit) == (1 if c.pattern == "one" else 2) and not ({1, rows - 2} & set(lst.tolist())))
    both = lambda vals: {(v, e) for v in vals for e in (True, False)}      # noqa: E731
    assert seen["iy_null"] == {True, False} and seen["same_pn_mode"] == both((True, False))
    assert seen["scale_sign"] == {-1.0, 1.0} and seen["w_sign"] >= {-1.0, 0.0, 1.0}
    assert seen["below"] == {True} and seen["ends"] == {True} and seen["clamp_rows"] == {True}
    assert seen["batch"] >= both(BATCHES), sorted(both(BATCHES) - seen["batch"])
    assert seen["d"] >= both(WIDE + SLICES), sorted(both(WIDE + SLICES) - seen["d"])
    assert seen["pattern"] >= both(PATTERNS)
    assert seen["terms"] == {(op, n) for op, m in MAX_TERMS.items() for n in range(1, m + 1)}
    assert seen["tau"] == set(TAUS) and seen["nce_batch"] == set(NCE_BATCHES) and seen["eps"] == {1e-12, 1e-5}
    assert seen["ew"] >= set(EW_WIDTHS)
    assert seen["g"] == {0.0, 1.0, -1.0, 2.0}
    assert seen["null"] >= {("bpr_multi", x) for x in ("none", "dU", "dI", "losses")} | {("cosine_multi", "dX")} | {
        ("infonce", x) for x in ("none", "dE1", "dE2")} | {("cat_leaky", x) for x in ("none", "dA", "dB", "dR")}
    assert seen["variant"] == both((0, 1)) and seen["mode"] == both((0, 1))
    for key in ("shared", "zero_len", "ids_null", "same_pn", "nonfinite", "whole", "minus1"):
        assert seen[key] == {True, False}, key


def test_workspace_size_functions_cover_the_kernels_layout():
    """the library's own size functions (host code, no launch) are never below what the kernels index: n_terms x ceil(batch / 16)
    partial sums for the multi-term ops (mmrec_rows_reg_workspace_bytes divides without parentheses: still enough), one float
    per sample for the single-term ones (the GPU cases show the same with a guard behind exactly these sizes)"""
    from mmrec_amd import _lib as L
    lib = L.load()
    for mb in (0, 1, 15, 16, 17, 255, 4097, 8193, 39400):
        assert lib.mmrec_bpr_workspace_bytes(mb) >= 4 * mb and lib.mmrec_cosine_workspace_bytes(mb) >= 4 * mb
        for n in range(1, 9):
            need = n * ((mb + 15) // 16) * 4
            if n <= 6:
                assert lib.mmrec_rows_reg_workspace_bytes(n, mb) >= need
            if n <= 4:
                assert lib.mmrec_bpr_multi_workspace_bytes(n, mb) >= need
            assert lib.mmrec_cosine_multi_workspace_bytes(n, mb) >= need


# ------------------------------------------------------------------------------------------------ GPU plumbing
def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def P(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def PA(ts):
    return (ctypes.c_void_p * len(ts))(*[None if t is None else t.data_ptr() for t in ts])


class Guarded:
    """an output array inside one tensor with GUARD floats on either side, handed over by offset pointer"""

    def __init__(self, n, fill=float("nan")):
        self.n = n
        self.buf = torch.full((n + 2 * GUARD,), GUARD_VALUE, device="cuda:0")
        self.view = self.buf[GUARD:GUARD + n]
        self.view.fill_(fill)

    def get(self, name):
        b = self.buf.cpu().numpy()
        assert (b[:GUARD] == GUARD_VALUE).all() and (b[GUARD + self.n:] == GUARD_VALUE).all(), (name, "guard floats overwritten")
        return b[GUARD:GUARD + self.n].copy()


class Workspace:
    """exactly nbytes, followed by a guard that must stay intact"""

    def __init__(self, nbytes):
        self.nbytes = int(nbytes)
        self.buf = torch.full((self.nbytes + 256,), 0xA5, dtype=torch.uint8, device="cuda:0")
        self.p = ctypes.c_void_p(self.buf.data_ptr())

    def ok(self, name):
        assert bool((self.buf[self.nbytes:] == 0xA5).all()), (name, "workspace overrun", self.nbytes)


class Table:
    """a pre-filled gradient table with two guard rows before and after"""

    def __init__(self, pre):
        self.pre = pre
        n, d = pre.shape
        self.buf = torch.full((n + 4, d), GUARD_VALUE, device="cuda:0")
        self.view = self.buf[2:2 + n]
        self.view.copy_(_dev(pre))

    def get(self, name, named):
        b = self.buf.cpu().numpy()
        assert (b[:2] == GUARD_VALUE).all() and (b[-2:] == GUARD_VALUE).all(), (name, "rows outside the table written")
        got = b[2:-2].copy()
        un = np.setdiff1d(np.arange(got.shape[0]), named)
        assert np.array_equal(got[un].view(np.int32), self.pre[un].view(np.int32)), (name, "a row the batch does not name changed")
        return got


def _lib():
    from mmrec_amd import _lib as L, hip_ops
    return L.load(), hip_ops._stream()


def _ok(rc, what):
    assert rc == 0, (what, rc)


def _named(lst):
    return np.unique(np.concatenate([np.asarray(i, np.int64) for i in lst] + [np.zeros(0, np.int64)]))


NONE = np.zeros(0, np.int64)


def run_gpu(c, ref):
    """the case through the C ABI; name -> (value,) for every output the case asks for (NULL outputs are left out)"""
    lib, s = _lib()
    op, B, d = c.op, c.batch, c.d
    got, tag = {}, c.axes()
    gdev = _dev(np.array([c.g], F32))
    if op in ("bpr", "bpr_dots"):
        U_, I = _dev(c.U), [_dev(T) for T in c.I]
        Pt, Nt = I[0], (I[0] if c.same_pn else I[-1])
        users, pos, neg = _dev(c.users), _dev(c.pos[0]), _dev(c.neg[0])
        loss, coef = Guarded(1), Guarded(max(B, 1))
        ws = Workspace(lib.mmrec_bpr_workspace_bytes(B))
        if op == "bpr":
            _ok(lib.mmrec_bpr_fwd_f32(P(U_), P(Pt), P(Nt), P(users), P(pos), P(neg), B, d, c.variant, c.scale, P(loss.view), P(coef.view),
                                      ws.p, s), "bpr_fwd")
        else:
            dts = Guarded(max(2 * B, 1))
            _ok(lib.mmrec_bpr_dots_f32(P(U_), P(Pt), P(Nt), P(users), P(pos), P(neg), B, d, P(dts.view), s), "bpr_dots")
            got["dots"] = (dts.get("dots")[:2 * B],)
            given = _dev(c.given_dots) if B else None
            _ok(lib.mmrec_bpr_loss_from_dots_f32(P(given), B, c.variant, c.scale, P(loss.view), P(coef.view), ws.p, s), "from_dots")
        got["loss0"], got["coef0"] = (loss.get("loss")[0],), (coef.get("coef")[:B],)
        ws.ok(tag)
        cf = _dev(c.coef[0]) if (c.exact and B) else coef.view
        want_u = c.null != "dU"
        dU = Table(c.pre["dU"])
        jn = 0 if c.same_pn else len(I) - 1
        dI = {j: Table(c.pre["dI%d" % j]) for j in {0, jn}}
        _ok(lib.mmrec_bpr_bwd_f32(P(U_), P(Pt), P(Nt), P(users), P(pos), P(neg), B, d, P(cf), P(gdev), c.scale,
                                  P(dU.view) if want_u else None, P(dI[0].view), P(dI[jn].view), s), "bpr_bwd")
        torch.cuda.synchronize()
        if want_u:
            got["dU"] = (dU.get("dU", c.users),)
        else:
            dU.get("dU", NONE)                                # NULL: nothing of it written
        for j in dI:
            got["dI%d" % j] = (dI[j].get("dI", _named(([c.pos[0]] if j == 0 else []) + ([c.neg[0]] if j == jn else []))),)
    elif op == "bpr_multi":
        n = c.n_terms
        U_, I = _dev(c.U), [_dev(T) for T in c.I]
        users, pos, neg = _dev(c.users), [_dev(x) for x in c.pos], [_dev(x) for x in c.neg]
        tabs = [I[c.share[t]] for t in range(n)]
        w = (ctypes.c_float * n)(*c.w)
        tot, losses, coef = Guarded(1), Guarded(n), Guarded(max(n * B, 1))
        ws = Workspace(lib.mmrec_bpr_multi_workspace_bytes(n, B))
        _ok(lib.mmrec_bpr_multi_fwd_f32(P(U_), P(users), PA(tabs), PA(pos), PA(neg), w, n, B, d, c.variant, c.scale, P(tot.view),
                                        None if c.null == "losses" else P(losses.view), P(coef.view), ws.p, s), "bpr_multi_fwd")
        got["total"] = (tot.get("total")[0],)
        lv, cv = losses.get("losses"), coef.get("coef")
        ws.ok(tag)
        for t in range(n):
            got["coef%d" % t] = (cv[t * B:(t + 1) * B],)
            if c.null != "losses":
                got["loss%d" % t] = (lv[t],)
        if c.null == "losses":
            assert np.isnan(lv).all(), "losses NULL, yet written"
        # fused == per-term: the per-term call against float64 too, and the two against each other
        w1 = Workspace(lib.mmrec_bpr_workspace_bytes(B))
        for t in range(n):
            l1, c1 = Guarded(1), Guarded(max(B, 1))
            _ok(lib.mmrec_bpr_fwd_f32(P(U_), P(tabs[t]), P(tabs[t]), P(users), P(pos[t]), P(neg[t]), B, d, c.variant, c.scale,
                                      P(l1.view), P(c1.view), w1.p, s), "bpr_fwd per term")
            per = c1.get("coef per term")[:B]
            check_float(per, ref["coef%d" % t][0], ref["coef%d" % t][1], "per-term coef%d [%s]" % (t, tag))
            check_float(per, cv[t * B:(t + 1) * B].astype(F64), 2 * ref["coef%d" % t][1], "fused vs per-term coef%d [%s]" % (t, tag))
            check_float(l1.get("loss per term")[0], ref["loss%d" % t][0], ref["loss%d" % t][1], "per-term loss%d [%s]" % (t, tag))
        cf = _dev(np.concatenate(c.coef)) if (c.exact and B) else coef.view
        dU = Table(c.pre["dU"])
        skip = 0 if c.null == "dI" else -1                    # one dI[t] NULL: every term of table share[0]
        dI = {j: Table(c.pre["dI%d" % j]) for j in set(c.share)}
        ptrs = [None if c.share[t] == skip else dI[c.share[t]].view for t in range(n)]
        _ok(lib.mmrec_bpr_multi_bwd_f32(P(U_), P(users), PA(tabs), PA(pos), PA(neg), w, n, B, d, P(cf), P(gdev), c.scale,
                                        None if c.null == "dU" else P(dU.view), PA(ptrs), s), "bpr_multi_bwd")
        torch.cuda.synchronize()
        if c.null != "dU":
            got["dU"] = (dU.get("dU", c.users),)
        else:
            dU.get("dU", NONE)
        for j in dI:
            if j == skip:
                dI[j].get("dI", NONE)
            else:
                got["dI%d" % j] = (dI[j].get("dI", _named([x for t in range(n) if c.share[t] == j for x in (c.pos[t], c.neg[t])])),)
    elif op in ("cosine", "cosine_multi"):
        n = c.n_terms
        Xs, Ys = [_dev(T) for T in c.X], [_dev(T) for T in c.Y]
        X = [Xs[c.share[t]] for t in range(n)]
        ix = [None if i is None else _dev(i) for i in c.ix]
        iy = [None if i is None else _dev(i) for i in c.iy]
        mb = max(c.batches)
        out = Guarded(1)
        dX = {j: Table(c.pre["dX%d" % j]) for j in set(c.share)}
        skip = -1
        if op == "cosine":
            coef = Guarded(2 * max(B, 1))
            ws = Workspace(lib.mmrec_cosine_workspace_bytes(B))
            _ok(lib.mmrec_cosine_fwd_f32(P(X[0]), P(ix[0]), P(Ys[0]), P(iy[0]), B, d, c.scale, P(out.view), P(coef.view), ws.p, s), "cosine_fwd")
            got["coef0"] = (coef.get("coef")[:2 * B].reshape(B, 2),)
            cf = _dev(c.coef[0]) if (c.exact and B) else coef.view
            _ok(lib.mmrec_cosine_bwd_f32(P(X[0]), P(ix[0]), P(Ys[0]), P(iy[0]), B, d, P(cf), P(gdev), c.scale, P(dX[0].view), s), "cosine_bwd")
        else:
            w = (ctypes.c_float * n)(*c.w)
            bt = (ctypes.c_int32 * n)(*c.batches)
            coef = Guarded(2 * n * max(mb, 1))
            ws = Workspace(lib.mmrec_cosine_multi_workspace_bytes(n, mb))
            _ok(lib.mmrec_cosine_multi_fwd_f32(PA(X), PA(ix), PA(Ys), PA(iy), w, bt, n, d, P(out.view), P(coef.view), ws.p, s), "cosine_multi_fwd")
            cv = coef.get("coef").reshape(n, max(mb, 1), 2)
            for t in range(n):
                got["coef%d" % t] = (cv[t, :c.batches[t]],)
            if c.exact:
                host = np.zeros((n, max(mb, 1), 2), F32)
                for t in range(n):
                    host[t, :c.batches[t]] = c.coef[t]
                cf = _dev(host)
            else:
                cf = coef.view
            skip = 0 if c.null == "dX" else -1
            ptrs = [None if c.share[t] == skip else dX[c.share[t]].view for t in range(n)]
            _ok(lib.mmrec_cosine_multi_bwd_f32(PA(X), PA(ix), PA(Ys), PA(iy), w, bt, n, d, P(cf), P(gdev), PA(ptrs), s), "cosine_multi_bwd")
        torch.cuda.synchronize()
        got["out"] = (out.get("out")[0],)
        ws.ok(tag)
        if op == "cosine_multi":                              # fused == per-term: mmrec_cosine_fwd_f32's coef, each against float64
            for t in range(n):
                bt_, c1, o1 = c.batches[t], Guarded(2 * max(c.batches[t], 1)), Guarded(1)
                w1 = Workspace(lib.mmrec_cosine_workspace_bytes(bt_))
                _ok(lib.mmrec_cosine_fwd_f32(P(X[t]), P(ix[t]), P(Ys[t]), P(iy[t]), bt_, d, 1.0, P(o1.view), P(c1.view), w1.p, s), "cosine_fwd per term")
                per = c1.get("coef per term")[:2 * bt_].reshape(bt_, 2)
                check_float(per, ref["coef%d" % t][0], ref["coef%d" % t][1], "per-term coef%d [%s]" % (t, tag))
                check_float(per, got["coef%d" % t][0].astype(F64), 2 * ref["coef%d" % t][1], "fused vs per-term coef%d [%s]" % (t, tag))
        for j in dX:
            if j == skip:
                dX[j].get("dX", NONE)
            else:
                got["dX%d" % j] = (dX[j].get("dX", _named([np.arange(c.batches[t]) if c.ix[t] is None else c.ix[t]
                                                           for t in range(n) if c.share[t] == j])),)
    elif op == "gather":
        E, ids = _dev(c.E[0]), _dev(c.ids[0])
        out = Guarded(1)
        ws = Workspace(4 * B)
        _ok(lib.mmrec_gather_sqnorm_fwd_f32(P(E), P(ids), B, d, P(out.view), ws.p, s), "gather_sqnorm")
        got["out"] = (out.get("out")[0],)
        ws.ok(tag)
        dE = Table(c.pre["dE0"])
        kdev = _dev(np.array([c.coef[0] if c.exact else c.g], F32))
        _ok(lib.mmrec_gather_scale_add_bwd_f32(P(E), P(ids), B, d, P(kdev), P(dE.view), s), "gather_scale_add")
        torch.cuda.synchronize()
        got["dE0"] = (dE.get("dE", c.ids[0]),)
    elif op == "rows_reg":
        n = c.n_terms
        Es = [_dev(T) for T in c.E]
        E = [Es[c.share[t]] for t in range(n)]
        ids = [None if i is None else _dev(i) for i in c.ids]
        bt = (ctypes.c_int32 * n)(*c.batches)
        out, coef = Guarded(1), Guarded(n)
        ws = Workspace(lib.mmrec_rows_reg_workspace_bytes(n, max(c.batches)))
        _ok(lib.mmrec_rows_reg_fwd_f32(PA(E), PA(ids), bt, n, d, c.mode, c.scale, P(out.view), P(coef.view), ws.p, s), "rows_reg_fwd")
        got["out"], got["coef"] = (out.get("out")[0],), (coef.get("coef"),)
        ws.ok(tag)
        if c.mode == 0 and not c.nonfinite:                   # fused == per-term: sum_t gather_sqnorm (terms with ids), against float64
            parts = []
            for t in range(n):
                if ids[t] is not None:
                    o1, w1 = Guarded(1), Workspace(4 * c.batches[t])
                    _ok(lib.mmrec_gather_sqnorm_fwd_f32(P(E[t]), P(ids[t]), c.batches[t], d, P(o1.view), w1.p, s), "gather_sqnorm per term")
                    parts.append(float(o1.get("per term")[0]))
            if len(parts) == n:
                check(c.scale * sum(parts), ref["out"][0], 2 * ref["out"][1], c.exact, "per-term sum vs float64 [%s]" % tag)
        cf = _dev(np.array(c.coef, F32)) if c.exact else coef.view
        dE = {j: Table(c.pre["dE%d" % j]) for j in set(c.share)}
        _ok(lib.mmrec_rows_reg_bwd_f32(PA(E), PA(ids), bt, n, d, P(cf), P(gdev), PA([dE[c.share[t]].view for t in range(n)]), s), "rows_reg_bwd")
        torch.cuda.synchronize()
        for j in dE:
            got["dE%d" % j] = (dE[j].get("dE", _named([np.arange(c.batches[t]) if c.ids[t] is None else c.ids[t]
                                                       for t in range(n) if c.share[t] == j])),)
    elif op == "scatter":
        ids, rows = _dev(c.ids), _dev(c.rows)
        order = torch.sort(ids, stable=True)[1] if B else ids
        out = Table(c.pre["out"])
        _ok(lib.mmrec_scatter_add_rows_sorted_f32(P(order), P(ids), P(rows), B, d, P(out.view), s), "scatter_add_rows_sorted")
        torch.cuda.synchronize()
        got["out"] = (out.get("out", c.ids[c.ids >= 0]),)
    elif op == "row_normalize":
        n = c.n
        X, G = _dev(c.X), _dev(c.G)
        Y, inv, dX = Guarded(max(n * d, 1)), Guarded(max(n, 1)), Guarded(max(n * d, 1))
        _ok(lib.mmrec_row_normalize_fwd_f32(P(X), n, d, c.eps, P(Y.view), P(inv.view), s), "row_normalize_fwd")
        _ok(lib.mmrec_row_normalize_bwd_f32(P(Y.view), P(G), P(inv.view), n, d, P(dX.view), s), "row_normalize_bwd")
        torch.cuda.synchronize()
        Yv, iv = Y.get("Y")[:n * d].reshape(n, d), inv.get("inv")[:n]
        got["Y"], got["inv"] = (Yv,), (iv,)
        r, tol = ev_normalize_bwd(Yv, c.G, iv, F64)           # the backward on the forward's own fp32 outputs
        got["_bwd"] = check_float(dX.get("dX")[:n * d].reshape(n, d), r, tol, "row_normalize_bwd [%s]" % tag)
    elif op == "cat_leaky":
        n, wa, wb = c.n, c.wa, c.wb
        A, Bm, dOut = _dev(c.A), _dev(c.B), _dev(c.dOut)
        R = None if c.R is None else _dev(c.R)
        out, dA, dB, dR = Guarded(max(n * (wa + wb), 1)), Guarded(max(n * wa, 1)), Guarded(max(n * wb, 1)), Guarded(max(n * wb, 1))
        _ok(lib.mmrec_cat_leaky_fwd_f32(P(A), P(Bm), P(R), n, wa, wb, c.slope, P(out.view), s), "cat_leaky_fwd")
        _ok(lib.mmrec_cat_leaky_bwd_f32(P(A), P(Bm), P(dOut), n, wa, wb, c.slope, None if c.null == "dA" else P(dA.view),
                                        None if c.null == "dB" else P(dB.view), None if c.null == "dR" else P(dR.view), s), "cat_leaky_bwd")
        torch.cuda.synchronize()
        ro, ra, rb, rr = ev_cat_leaky(c)
        bits = lambda a: np.ascontiguousarray(a, F32).view(np.int32).ravel()      # noqa: E731
        assert np.array_equal(bits(out.get("out")[:n * (wa + wb)]), bits(ro)), ("cat_leaky out bits", tag)
        for nm, gd, rf in (("dA", dA, ra), ("dB", dB, rb), ("dR", dR, rr)):
            v = gd.get(nm)
            if c.null == nm:
                assert np.isnan(v).all(), (nm, "NULL, yet written")
            else:
                assert np.array_equal(bits(v[:rf.size]), bits(rf)), ("cat_leaky bits", nm, tag)
    elif op == "infonce":
        E1, E2, ids = _dev(c.E1), _dev(c.E2), _dev(c.ids)
        loss = Guarded(1)
        ws = Workspace(lib.mmrec_infonce_workspace_bytes(B))
        _ok(lib.mmrec_infonce_fwd_f32(P(E1), P(E2), P(ids), B, 64, c.tau, P(loss.view), ws.p, s), "infonce_fwd")
        d1, d2 = Table(c.pre["dE1"]), Table(c.pre["dE2"])
        _ok(lib.mmrec_infonce_bwd_f32(P(ids), B, 64, c.tau, P(gdev), None if c.null == "dE1" else P(d1.view),
                                      None if c.null == "dE2" else P(d2.view), ws.p, s), "infonce_bwd")
        torch.cuda.synchronize()
        got["loss"] = (loss.get("loss")[0],)
        ws.ok(tag)
        for nm, tb in (("dE1", d1), ("dE2", d2)):
            if c.null == nm:
                tb.get(nm, NONE)
            else:
                got[nm] = (tb.get(nm, c.ids),)
    return got


@pytest.mark.gpu
@pytest.mark.parametrize("seed", range(CASES))
def test_loss_fuzz(seed):
    """every case twice through the C ABI: gradient tables zero-filled, then pre-filled (the accumulation contract: the second
    reference is the first plus the pre-fill); outputs behind guards, workspaces of exactly the reported size, rows the batch
    does not name bit-identical afterwards"""
    c = draw_case(seed)
    worst = 0.0
    for zero in (True, False):
        c.zero_pre = zero
        ref = evaluate(c)
        got = run_gpu(c, ref)
        worst = max(worst, _compare(c, ref, got), got.get("_bwd", 0.0))
        if c.op in ("row_normalize", "cat_leaky"):
            break                                            # no accumulating output
    print("loss fuzz %s: worst err / tol %.3f" % (c.axes(), worst))


# ------------------------------------------------------------------------------------------------ GPU: the autograd wrappers
WRAPPER_OPS = ("bpr", "bpr_multi", "cosine", "cosine_multi", "gather", "rows_reg", "infonce", "scatter")
WRAPPER_SEEDS = [s for s in range(CASES) if OPS[s % len(OPS)] in WRAPPER_OPS and (s // len(OPS)) in (4, 5, 7, 9, 13)]


def _wrapper(c, hip_ops):
    """the case through its autograd wrapper: forward value(s) and the gradients of the tables, as evaluate() names them"""
    op, got = c.op, {}
    g = torch.tensor(c.g, device="cuda:0")
    leaf = lambda a: _dev(a).requires_grad_()                # noqa: E731
    dv = lambda i: None if i is None else _dev(i)            # noqa: E731
    if op in ("bpr", "bpr_multi"):
        U_, I = leaf(c.U), [leaf(T) for T in c.I]
        users = _dev(c.users)
        terms = [(I[c.share[t]], _dev(c.pos[t]), _dev(c.neg[t])) for t in range(c.n_terms)]
        if op == "bpr":
            loss = hip_ops.bpr_loss(U_, I[0], users, terms[0][1], terms[0][2], c.variant, "mean")
            got["loss0"] = (float(loss),)
        else:
            loss = hip_ops.bpr_weighted_total(U_, users, terms, c.w, c.variant, "mean")
            got["total"] = (float(loss),)
            each = hip_ops.bpr_losses_shared_users(U_.detach(), users, [(T.detach(), p, q) for T, p, q in terms], c.variant, "mean")
            for t, l in enumerate(each):
                got["loss%d" % t] = (float(l),)
        loss.backward(g)
        got["dU"] = (U_.grad.cpu().numpy(),)
        for j, T in enumerate(I):
            got["dI%d" % j] = (T.grad.cpu().numpy(),)
    elif op in ("cosine", "cosine_multi"):
        X = [leaf(T) for T in c.X]
        terms = [(X[c.share[t]], dv(c.ix[t]), _dev(c.Y[t])[:c.batches[t]] if c.iy[t] is None else _dev(c.Y[t]), dv(c.iy[t]), c.w[t])
                 for t in range(c.n_terms)]
        out = hip_ops.cosine_mean(*terms[0][:4]) if op == "cosine" else hip_ops.cosine_means(terms)
        got["out"] = (float(out),)
        out.backward(g)
        for j, T in enumerate(X):
            got["dX%d" % j] = (T.grad.cpu().numpy(),)
    elif op in ("gather", "rows_reg"):
        E = [leaf(T) for T in c.E]
        terms = [(E[c.share[t]], dv(c.ids[t])) for t in range(c.n_terms)]
        out = hip_ops.gather_sqnorm(*terms[0]) if op == "gather" else hip_ops.rows_reg(terms, c.mode, c.scale)
        got["out"] = (float(out),)
        out.backward(g if op == "rows_reg" else g / 2)       # gather_sqnorm's backward factor is 2 g; evaluate() takes g
        for j, T in enumerate(E):
            got["dE%d" % j] = (T.grad.cpu().numpy(),)
    elif op == "infonce":
        E1, E2 = leaf(c.E1), leaf(c.E2)
        loss = hip_ops.infonce(E1, E2, _dev(c.ids), c.tau)
        got["loss"] = (float(loss),)
        loss.backward(g)
        got["dE1"], got["dE2"] = (E1.grad.cpu().numpy(),), (E2.grad.cpu().numpy(),)
    elif op == "scatter":
        out = _dev(c.pre["out"]).clone()
        hip_ops.scatter_add_rows(_dev(c.ids), _dev(c.rows), out)
        got["out"] = (out.cpu().numpy(),)
    return got


@pytest.mark.gpu
@pytest.mark.parametrize("seed", WRAPPER_SEEDS)
def test_wrappers_vs_float64(seed):
    """the autograd wrappers (scale = 1 / B or 1 as they set it; an operand without an index has one row per sample) with
    set_deterministic off and on: every value against float64; forward scalars bit-identical across two runs in both settings,
    gradients bit-identical across two runs in deterministic mode"""
    from mmrec_amd import hip_ops
    c = draw_case(seed)
    if c.op in ("bpr", "bpr_multi", "cosine"):
        c.scale = 1.0 / max(c.batch, 1)                      # the wrappers' `mean`
    if c.op == "bpr" and not c.same_pn:
        c.same_pn, c.I = True, c.I[:1]                       # the wrapper takes one item table
    if c.op in ("cosine", "cosine_multi"):
        for t in range(c.n_terms):
            if c.ix[t] is None and c.X[c.share[t]].shape[0] != c.batches[t]:
                c.ix[t] = np.arange(c.batches[t])
    if c.op == "rows_reg":
        for t in range(c.n_terms):                           # ids None means the WHOLE table to the wrapper
            if c.ids[t] is None and c.E[c.share[t]].shape[0] != c.batches[t]:
                c.ids[t] = np.arange(c.batches[t])
    _check_wrappers(c, hip_ops)


@pytest.mark.gpu
@pytest.mark.parametrize("op", ["rows_reg", "cosine_means"])
@pytest.mark.parametrize("layout", ["prefix_first", "base_first", "overlap", "detached_alias"])
def test_tables_that_share_storage(op, layout):
    """two terms whose tables share memory without being the same table -- (T[:k], ids) + (T, None), (T, None) + (T[:k], ids),
    two overlapping row ranges with different base pointers, a detached alias -- against float64: the gradient of T is the sum
    over the live terms, nothing is written outside it"""
    from mmrec_amd import hip_ops
    rng = np.random.default_rng(len(op) + len(layout))
    n, k, d = 300, 100, 64
    T0 = rng.standard_normal((n + 2, d)).astype(F32)
    big = _dev(T0).requires_grad_()
    T = big[1:n + 1]                                         # a view: the rows before and after it must get no gradient
    ids = rng.integers(0, k, 77)
    a, b = (T[:k], ids), (T, None)
    if layout == "base_first":
        a, b = b, a
    elif layout == "overlap":
        a, b = (T[:200], None), (T[150:], None)
    elif layout == "detached_alias":
        a, b = (T, None), (T.detach(), None)
    Y0 = rng.standard_normal((n, d)).astype(F32)
    T64 = torch.from_numpy(T0.astype(F64)).requires_grad_()
    V = T64[1:n + 1]

    def as64(x):                                             # the same view of the float64 table
        off = (x.data_ptr() - T.data_ptr()) // (4 * d)
        v = V[off:off + x.shape[0]]
        return v if x.requires_grad else v.detach()

    if op == "rows_reg":
        out = hip_ops.rows_reg([(x, None if i is None else _dev(i)) for x, i in (a, b)], 1, 0.5)
        ref = 0.5 * sum(torch.sqrt(((as64(x) if i is None else as64(x)[torch.from_numpy(i)]) ** 2).sum()) for x, i in (a, b))
    else:
        Yd = _dev(Y0)
        out = hip_ops.cosine_means([(x, None if i is None else _dev(i), Yd[:x.shape[0]] if i is None else Yd,
                                     None if i is None else _dev(i), w) for (x, i), w in zip((a, b), (1.0, -0.5))])
        Y64 = torch.from_numpy(Y0.astype(F64))
        ref = 0.0
        for (x, i), w in zip((a, b), (1.0, -0.5)):
            xs = as64(x) if i is None else as64(x)[torch.from_numpy(i)]
            ys = Y64[:x.shape[0]] if i is None else Y64[torch.from_numpy(i)]
            ref = ref + w * torch.nn.functional.cosine_similarity(xs, ys, dim=1, eps=1e-8).mean()
    (1.5 * out).backward()
    (1.5 * ref).backward()
    torch.cuda.synchronize()
    assert abs(float(out) - float(ref)) <= 1e-5 * abs(float(ref)) + 1e-7
    got, want = big.grad.cpu().double().numpy(), T64.grad.numpy()
    assert (got[0] == 0).all() and (got[-1] == 0).all()
    assert np.all(np.abs(got - want) <= 1e-5 * np.abs(want) + 1e-9), float(np.abs(got - want).max())


@pytest.mark.gpu
def test_misuse_is_rejected_before_any_launch():
    """unsupported widths, negative batch, n_terms 0 and maximum + 1, NULL required pointers with batch > 0, bad variant / mode,
    tau <= 0, InfoNCE batch == 0: an error code from the host, nothing written"""
    lib, s = _lib()
    B, d, n = 32, 64, 50
    rng = np.random.default_rng(1)
    T = _dev(rng.standard_normal((n, d)).astype(F32))
    T0 = T.clone()
    ids = _dev(rng.integers(0, n, B))
    out = torch.full((4096,), 7.0, device="cuda:0")
    ws = torch.zeros(1 << 20, dtype=torch.uint8, device="cuda:0")
    g = torch.ones(1, device="cuda:0")
    o, w_, t, i = P(out), P(ws), P(T), P(ids)
    one = lambda x: PA([x])                                   # noqa: E731
    wf = (ctypes.c_float * 1)(1.0)
    b1, bneg = (ctypes.c_int32 * 1)(B), (ctypes.c_int32 * 1)(-1)
    many = lambda k: (PA([T] * k), PA([ids] * k), (ctypes.c_float * k)(*[1.0] * k), (ctypes.c_int32 * k)(*[B] * k))      # noqa: E731
    calls = [
        lambda: lib.mmrec_bpr_fwd_f32(t, t, t, i, i, i, B, 48, 0, 1.0, o, o, w_, s),
        lambda: lib.mmrec_bpr_fwd_f32(t, t, t, i, i, i, -1, d, 0, 1.0, o, o, w_, s),
        lambda: lib.mmrec_bpr_fwd_f32(t, t, t, i, i, i, B, d, 2, 1.0, o, o, w_, s),
        lambda: lib.mmrec_bpr_fwd_f32(None, t, t, i, i, i, B, d, 0, 1.0, o, o, w_, s),
        lambda: lib.mmrec_bpr_fwd_f32(t, t, t, i, i, i, B, d, 0, 1.0, None, o, w_, s),
        lambda: lib.mmrec_bpr_bwd_f32(t, t, t, i, i, i, B, 24, o, P(g), 1.0, o, o, o, s),
        lambda: lib.mmrec_bpr_bwd_f32(t, t, t, i, i, i, B, d, None, P(g), 1.0, o, o, o, s),
        lambda: lib.mmrec_bpr_dots_f32(t, t, t, i, i, i, B, 12, o, s),
        lambda: lib.mmrec_bpr_dots_f32(t, t, t, i, i, i, B, d, None, s),
        lambda: lib.mmrec_bpr_loss_from_dots_f32(o, B, 3, 1.0, o, o, w_, s),
        lambda: lib.mmrec_bpr_loss_from_dots_f32(None, B, 0, 1.0, o, o, w_, s),
        lambda: lib.mmrec_bpr_multi_fwd_f32(t, i, one(T), one(ids), one(ids), wf, 0, B, d, 0, 1.0, o, o, o, w_, s),
        lambda: lib.mmrec_bpr_multi_fwd_f32(t, i, many(5)[0], many(5)[1], many(5)[1], many(5)[2], 5, B, d, 0, 1.0, o, o, o, w_, s),
        lambda: lib.mmrec_bpr_multi_fwd_f32(t, i, one(None), one(ids), one(ids), wf, 1, B, d, 0, 1.0, o, o, o, w_, s),
        lambda: lib.mmrec_bpr_multi_bwd_f32(t, i, one(T), one(ids), one(ids), wf, 1, B, 32, o, P(g), 1.0, o, one(out), s),
        lambda: lib.mmrec_cosine_fwd_f32(t, i, t, i, B, 32, 1.0, o, o, w_, s),
        lambda: lib.mmrec_cosine_fwd_f32(t, i, None, i, B, d, 1.0, o, o, w_, s),
        lambda: lib.mmrec_cosine_bwd_f32(t, i, t, i, -2, d, o, P(g), 1.0, o, s),
        lambda: lib.mmrec_cosine_multi_fwd_f32(many(9)[0], many(9)[1], many(9)[0], many(9)[1], many(9)[2], many(9)[3], 9, d, o, o, w_, s),
        lambda: lib.mmrec_cosine_multi_fwd_f32(one(T), one(ids), one(T), one(ids), wf, bneg, 1, d, o, o, w_, s),
        lambda: lib.mmrec_cosine_multi_bwd_f32(one(T), one(ids), one(T), one(ids), wf, b1, 1, d, o, P(g), None, s),
        lambda: lib.mmrec_gather_sqnorm_fwd_f32(t, i, B, 100, o, w_, s),
        lambda: lib.mmrec_gather_sqnorm_fwd_f32(t, None, B, d, o, w_, s),
        lambda: lib.mmrec_gather_scale_add_bwd_f32(t, i, B, d, P(g), None, s),
        lambda: lib.mmrec_rows_reg_fwd_f32(one(T), one(ids), b1, 1, d, 2, 1.0, o, o, w_, s),
        lambda: lib.mmrec_rows_reg_fwd_f32(many(7)[0], many(7)[1], many(7)[3], 7, d, 0, 1.0, o, o, w_, s),
        lambda: lib.mmrec_rows_reg_fwd_f32(one(T), one(ids), b1, 0, d, 0, 1.0, o, o, w_, s),
        lambda: lib.mmrec_rows_reg_bwd_f32(one(T), one(ids), b1, 1, d, o, P(g), one(None), s),
        lambda: lib.mmrec_scatter_add_rows_sorted_f32(i, i, t, B, 48, o, s),
        lambda: lib.mmrec_scatter_add_rows_sorted_f32(None, i, t, B, d, o, s),
        lambda: lib.mmrec_row_normalize_fwd_f32(t, n, 6, 1e-12, o, o, s),
        lambda: lib.mmrec_row_normalize_fwd_f32(t, -1, d, 1e-12, o, o, s),
        lambda: lib.mmrec_row_normalize_bwd_f32(t, t, None, n, d, o, s),
        lambda: lib.mmrec_cat_leaky_fwd_f32(t, t, None, n, 6, 64, 0.1, o, s),
        lambda: lib.mmrec_cat_leaky_bwd_f32(t, t, None, n, 32, 32, 0.1, o, o, o, s),
        lambda: lib.mmrec_infonce_fwd_f32(t, t, i, 0, 64, 0.2, o, w_, s),
        lambda: lib.mmrec_infonce_fwd_f32(t, t, i, B, 128, 0.2, o, w_, s),
        lambda: lib.mmrec_infonce_fwd_f32(t, t, i, B, 64, 0.0, o, w_, s),
        lambda: lib.mmrec_infonce_fwd_f32(t, t, i, B, 64, -1.0, o, w_, s),
        lambda: lib.mmrec_infonce_bwd_f32(i, B, 64, 0.2, None, o, o, w_, s),
        lambda: lib.mmrec_infonce_bwd_f32(i, 0, 64, 0.2, P(g), o, o, w_, s),
    ]
    for k, call in enumerate(calls):
        rc = call()
        assert rc in (10001, 10002), (k, rc)
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and torch.equal(T, T0) and int(ws.sum()) == 0


# ------------------------------------------------------------------------------------------------ GPU: the elementwise wrappers
def _check_wrappers(c, hip_ops):
    """c through its wrapper with set_deterministic off and on: values against float64, forward scalars repeatable in both
    settings, gradients bit-identical across two runs in deterministic mode"""
    c.exact, c.coef = False, None                            # the wrappers run on their own forward coefficients
    c.zero_pre = c.op != "scatter"
    ref = evaluate(c)
    c.exact_tables = False
    before = hip_ops.DETERMINISTIC
    try:
        for det in (False, True):
            hip_ops.set_deterministic(det)
            a, b = _wrapper(c, hip_ops), _wrapper(c, hip_ops)
            worst = _compare(c, ref, a)
            for nm, (val, tol, kind) in ref.items():
                if nm in a and (kind == "scalar" or det):
                    assert np.array_equal(np.asarray(a[nm][0]), np.asarray(b[nm][0]), equal_nan=True), (nm, "not repeatable", det, c.axes())
            print("wrappers %s det %s: worst err / tol %.3f" % (c.axes(), det, worst))
    finally:
        hip_ops.set_deterministic(before)


@pytest.mark.gpu
@pytest.mark.parametrize("op", ["bpr", "bpr_multi", "cosine", "gather", "rows_reg", "infonce", "scatter"])
def test_deterministic_wrappers_on_a_one_id_batch(op):
    """a batch in which EVERY sample names the same row (users one id, positives one id, negatives another): the worst
    contention of the atomics; in deterministic mode two runs give the same bits, and both settings meet float64"""
    from mmrec_amd import hip_ops
    c = _find(lambda c: c.op == op and c.batch in (255, 256, 257, 333) and not c.nonfinite and not (op == "bpr" and not c.same_pn))
    one = lambda ids, row: None if ids is None else np.full(ids.size, row, np.int64)      # noqa: E731
    if op in ("bpr", "bpr_multi"):
        c.scale = 1.0 / c.batch
        c.users, c.pos, c.neg = one(c.users, 2), [one(i, 3) for i in c.pos], [one(i, c.n_rows - 1) for i in c.neg]
        lists = [c.users] + c.pos + c.neg
    elif op == "cosine":
        c.scale = 1.0 / c.batch
        if c.ix[0] is None:
            c.ix[0] = np.arange(c.batch)
        c.ix = [one(c.ix[0], 7)]
        lists = c.ix
    elif op in ("gather", "rows_reg"):
        c.ids = [one(i, 0) for i in c.ids]
        lists = [i for i in c.ids if i is not None]
    else:
        c.ids = one(c.ids, c.n_rows - 1)
        lists = [c.ids]
    assert all(np.unique(i).size == 1 for i in lists if i.size) and max(i.size for i in lists) >= 255      # the pattern this test is about
    c.pattern = "one"
    _check_wrappers(c, hip_ops)


@pytest.mark.gpu
@pytest.mark.parametrize("seed", [s for s in range(CASES) if OPS[s % len(OPS)] in ("row_normalize", "cat_leaky") and s // len(OPS) in (2, 5, 6, 9)])
def test_elementwise_wrappers_vs_float64(seed):
    """hip_ops.row_normalize and hip_ops.cat_leaky, forward and backward through autograd, set_deterministic off and on:
    row_normalize against float64 (the backward through the forward's own Y; its 1 / max(norm, eps) carries the forward's
    relative error rr), cat_leaky bit for bit"""
    from mmrec_amd import hip_ops
    c = draw_case(seed)
    before = hip_ops.DETERMINISTIC
    try:
        for det in (False, True):
            hip_ops.set_deterministic(det)
            if c.op == "row_normalize":
                if c.n == 0:
                    continue
                X = _dev(c.X).requires_grad_()
                Y = hip_ops.row_normalize(X, c.eps)
                Y.backward(_dev(c.G))
                ref = evaluate(c)
                Yv = Y.detach().cpu().numpy()
                check_float(Yv, ref["Y"][0], ref["Y"][1], "row_normalize wrapper Y [%s]" % c.axes())
                inv64, tinv = ref["inv"][0], ref["inv"][1]
                r, tol = ev_normalize_bwd(Yv, c.G, inv64.astype(F32), F64)
                rel = (tinv / np.abs(inv64) + U)[:, None]
                tol = tol + rel * (np.abs(r) + tol / gamma(ndot(c.d) + 4))
                check_float(X.grad.cpu().numpy(), r, tol, "row_normalize wrapper dX [%s]" % c.axes())
            else:
                A, B = _dev(c.A).requires_grad_(), _dev(c.B).requires_grad_()
                R = None if c.R is None else _dev(c.R).requires_grad_()
                out = hip_ops.cat_leaky(A, B, R, c.slope)
                if c.n:
                    out.backward(_dev(c.dOut))
                ro, ra, rb, rr = ev_cat_leaky(c)
                bits = lambda a: np.ascontiguousarray(a, F32).view(np.int32).ravel()      # noqa: E731
                assert np.array_equal(bits(out.detach().cpu().numpy()), bits(ro)), ("cat_leaky wrapper", c.axes())
                if c.n:
                    for t, rf in ((A, ra), (B, rb)) + (((R, rr),) if R is not None else ()):
                        assert np.array_equal(bits(t.grad.cpu().numpy()), bits(rf)), ("cat_leaky wrapper grad", c.axes())
    finally:
        hip_ops.set_deterministic(before)


# ------------------------------------------------------------------------------------------------ GPU: capture
def _family(c):
    """static device buffers of the case and launch(): zero the gradient tables, forward, backward -- C ABI calls only, on
    the current stream; load(c): new table contents into the static inputs; read(): name -> (value,)"""
    from mmrec_amd import hip_ops
    lib = _lib()[0]
    op, B, d = c.op, c.batch, c.d
    g = _dev(np.array([c.g], F32))
    S = lambda: hip_ops._stream()                            # noqa: E731
    if op == "bpr":
        U_, I0 = _dev(c.U), _dev(c.I[0])
        N0 = I0 if c.same_pn else _dev(c.I[-1])
        users, pos, neg = _dev(c.users), _dev(c.pos[0]), _dev(c.neg[0])
        loss, coef = torch.zeros(1, device="cuda:0"), torch.zeros(B, device="cuda:0")
        ws = torch.zeros(max(lib.mmrec_bpr_workspace_bytes(B), 16), dtype=torch.uint8, device="cuda:0")
        dU, dI = torch.zeros_like(U_), torch.zeros_like(I0)
        dN = dI if c.same_pn else torch.zeros_like(N0)

        def launch():
            dU.zero_(), dI.zero_(), dN.zero_()
            _ok(lib.mmrec_bpr_fwd_f32(P(U_), P(I0), P(N0), P(users), P(pos), P(neg), B, d, c.variant, c.scale, P(loss), P(coef), P(ws), S()), "fwd")
            _ok(lib.mmrec_bpr_bwd_f32(P(U_), P(I0), P(N0), P(users), P(pos), P(neg), B, d, P(coef), P(g), c.scale, P(dU), P(dI), P(dN), S()), "bwd")
        load = lambda c: (U_.copy_(_dev(c.U)), I0.copy_(_dev(c.I[0])), N0.copy_(_dev(c.I[-1])))      # noqa: E731
        read = lambda: {"loss0": (loss.item(),), "coef0": (coef.cpu().numpy(),), "dU": (dU.cpu().numpy(),), "dI0": (dI.cpu().numpy(),),      # noqa: E731
                        "dI%d" % (len(c.I) - 1): (dN.cpu().numpy(),)}
    elif op == "cosine":
        X, Y = _dev(c.X[0]), _dev(c.Y[0])
        ix, iy = (None if i is None else _dev(i) for i in (c.ix[0], c.iy[0]))
        out, coef = torch.zeros(1, device="cuda:0"), torch.zeros(B, 2, device="cuda:0")
        ws = torch.zeros(max(lib.mmrec_cosine_workspace_bytes(B), 16), dtype=torch.uint8, device="cuda:0")
        dX = torch.zeros_like(X)

        def launch():
            dX.zero_()
            _ok(lib.mmrec_cosine_fwd_f32(P(X), P(ix), P(Y), P(iy), B, d, c.scale, P(out), P(coef), P(ws), S()), "fwd")
            _ok(lib.mmrec_cosine_bwd_f32(P(X), P(ix), P(Y), P(iy), B, d, P(coef), P(g), c.scale, P(dX), S()), "bwd")
        load = lambda c: (X.copy_(_dev(c.X[0])), Y.copy_(_dev(c.Y[0])))      # noqa: E731
        read = lambda: {"out": (out.item(),), "coef0": (coef.cpu().numpy(),), "dX0": (dX.cpu().numpy(),)}      # noqa: E731
    elif op == "rows_reg":
        n = c.n_terms
        Es = [_dev(T) for T in c.E]
        ids = [None if i is None else _dev(i) for i in c.ids]
        EA, IA, bt = PA([Es[c.share[t]] for t in range(n)]), PA(ids), (ctypes.c_int32 * n)(*c.batches)
        out, coef = torch.zeros(1, device="cuda:0"), torch.zeros(n, device="cuda:0")
        ws = torch.zeros(lib.mmrec_rows_reg_workspace_bytes(n, max(c.batches)), dtype=torch.uint8, device="cuda:0")
        dE = [torch.zeros_like(T) for T in Es]
        DA = PA([dE[c.share[t]] for t in range(n)])

        def launch():
            for t_ in dE:
                t_.zero_()
            _ok(lib.mmrec_rows_reg_fwd_f32(EA, IA, bt, n, d, c.mode, c.scale, P(out), P(coef), P(ws), S()), "fwd")
            _ok(lib.mmrec_rows_reg_bwd_f32(EA, IA, bt, n, d, P(coef), P(g), DA, S()), "bwd")
        load = lambda c: [t_.copy_(_dev(T)) for t_, T in zip(Es, c.E)]      # noqa: E731
        read = lambda: dict({"out": (out.item(),), "coef": (coef.cpu().numpy(),)},      # noqa: E731
                            **{"dE%d" % j: (t_.cpu().numpy(),) for j, t_ in enumerate(dE)})
    elif op == "infonce":
        E1, E2, ids = _dev(c.E1), _dev(c.E2), _dev(c.ids)
        loss = torch.zeros(1, device="cuda:0")
        ws = torch.zeros(lib.mmrec_infonce_workspace_bytes(B), dtype=torch.uint8, device="cuda:0")
        d1, d2 = torch.zeros_like(E1), torch.zeros_like(E2)

        def launch():
            d1.zero_(), d2.zero_()
            _ok(lib.mmrec_infonce_fwd_f32(P(E1), P(E2), P(ids), B, 64, c.tau, P(loss), P(ws), S()), "fwd")
            _ok(lib.mmrec_infonce_bwd_f32(P(ids), B, 64, c.tau, P(g), P(d1), P(d2), P(ws), S()), "bwd")
        load = lambda c: (E1.copy_(_dev(c.E1)), E2.copy_(_dev(c.E2)))      # noqa: E731
        read = lambda: {"loss": (loss.item(),), "dE1": (d1.cpu().numpy(),), "dE2": (d2.cpu().numpy(),)}      # noqa: E731
    elif op == "scatter":
        ids, rows = _dev(c.ids), _dev(c.rows)
        order = torch.sort(ids, stable=True)[1]
        out = torch.zeros(c.n_rows, d, device="cuda:0")

        def launch():
            out.zero_()
            _ok(lib.mmrec_scatter_add_rows_sorted_f32(P(order), P(ids), P(rows), B, d, P(out), S()), "scatter")
        load = lambda c: rows.copy_(_dev(c.rows))           # noqa: E731
        read = lambda: {"out": (out.cpu().numpy(),)}         # noqa: E731
    elif op == "row_normalize":
        n = c.n
        X, G = _dev(c.X), _dev(c.G)
        Y, inv, dX = torch.zeros_like(X), torch.zeros(n, device="cuda:0"), torch.zeros_like(X)

        def launch():
            _ok(lib.mmrec_row_normalize_fwd_f32(P(X), n, d, c.eps, P(Y), P(inv), S()), "fwd")
            _ok(lib.mmrec_row_normalize_bwd_f32(P(Y), P(G), P(inv), n, d, P(dX), S()), "bwd")
        load = lambda c: (X.copy_(_dev(c.X)), G.copy_(_dev(c.G)))      # noqa: E731

        def read():
            Yv, iv = Y.cpu().numpy(), inv.cpu().numpy()
            r, tol = ev_normalize_bwd(Yv, c.G, iv, F64)
            check_float(dX.cpu().numpy(), r, tol, "captured row_normalize_bwd")
            return {"Y": (Yv,), "inv": (iv,)}
    return launch, load, read


@pytest.mark.gpu
@pytest.mark.parametrize("op", ["bpr", "cosine", "rows_reg", "infonce", "scatter", "row_normalize"])
def test_forward_and_backward_replay_as_a_captured_graph(op):
    """one case per family: forward and backward through the C ABI captured with torch.cuda.graph on a side stream as a single
    chain, replayed twice with new table contents, each replay against float64 -- no allocation, no synchronisation, no state
    kept between calls"""
    c = _find(lambda c: c.op == op and not c.exact and not c.nonfinite and 255 <= c.batch <= 2048
              and (op != "cosine" or c.ix[0] is not None))
    c.zero_pre = True
    launch, load, read = _family(c)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        launch()                                             # (code objects loaded before the capture)
    side.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        launch()
    for replay in range(3):
        if replay:                                           # new table contents: every table's rows rotated
            for nm in ("U", "X", "G", "rows", "E1", "E2", "I", "E", "Y"):
                v = getattr(c, nm, None)
                if isinstance(v, np.ndarray):
                    setattr(c, nm, np.roll(v, replay, axis=0).copy())
                elif isinstance(v, list):
                    setattr(c, nm, [np.roll(T, replay, axis=0).copy() for T in v])
            load(c)
        graph.replay()
        torch.cuda.synchronize()
        ref = evaluate(c)
        worst = _compare(c, ref, read())
        print("captured %s replay %d: worst err / tol %.3f" % (c.axes(), replay, worst))


# ------------------------------------------------------------------------------------------------ GPU: offsets beyond 4 GiB
BIG_ROWS = (1 << 24) + 16                                    # x 64 floats: 2^32 + 4096 bytes


def _big_rows(rows):
    """rows of the big table on the host: T[r, c] = ((7 r + 3 c) mod 33 - 16) / 16"""
    r = np.asarray(rows, np.int64)[:, None]
    return (((7 * r + 3 * np.arange(64)) % 33 - 16) / 16.0).astype(F32)


@pytest.mark.gpu
def test_rows_beyond_four_gib():
    """a table of 2^24 + 16 rows of 64 floats (just over 2^32 bytes), filled on the device by the formula `_big_rows` restates,
    named in its first and its last 16 rows: bpr_fwd / bwd, gather_sqnorm / gather_scale_add, rows_reg with ids, all three
    backwards accumulating into one gradient table of the same size (exact mode: grid values), then row_normalize over all
    rows with its int64 n.  Named rows against float64, a strided sample and both ends of the rest for untouched bits"""
    free = torch.cuda.mem_get_info()[0]
    if free < 24 << 30:
        pytest.skip("needs 24 GiB of free device memory, the device reports %.1f GiB" % (free / 2 ** 30))
    lib, s = _lib()
    T = torch.empty(BIG_ROWS, 64, device="cuda:0")
    col = 3 * torch.arange(64, device="cuda:0")
    for r0 in range(0, BIG_ROWS, 1 << 21):
        r = torch.arange(r0, min(BIG_ROWS, r0 + (1 << 21)), device="cuda:0")[:, None]
        T[r0:r0 + r.shape[0]] = (((7 * r + col) % 33 - 16).float() / 16.0)
    G = torch.full((BIG_ROWS, 64), 0.25, device="cuda:0")
    rng = np.random.default_rng(4)
    ends = np.concatenate([np.arange(16), np.arange(BIG_ROWS - 16, BIG_ROWS)])
    named = np.setdiff1d(ends, [1, BIG_ROWS - 2])            # rows 1 and BIG_ROWS - 2 stay unnamed
    B = 300
    compact = {int(r): i for i, r in enumerate(named)}
    c = Case()
    c.seed, c.op, c.exact, c.batch, c.d, c.pattern, c.n_terms, c.variant = 0, "bpr", True, B, 64, "zipf", 1, 0
    c.g, c.scale, c.nonfinite, c.same_pn, c.share, c.null, c.zero_pre = 0.5, 1.0, False, True, [0], "none", True
    big = {k: rng.choice(named, B) for k in ("users", "pos", "neg", "gather", "reg")}
    for k in big:
        big[k][:2] = [0, BIG_ROWS - 1]
    loc = lambda ids: np.array([compact[int(r)] for r in ids], np.int64)      # noqa: E731
    c.U = _big_rows(named)
    c.I = [c.U]
    c.users, c.pos, c.neg, c.coef = loc(big["users"]), [loc(big["pos"])], [loc(big["neg"])], [_coefgrid(rng, B)]
    ref = evaluate(c)
    dev = {k: _dev(v) for k, v in big.items()}
    loss, coef = Guarded(1), Guarded(B)
    ws = Workspace(lib.mmrec_bpr_workspace_bytes(B))
    gdev, cf = _dev(np.array([c.g], F32)), _dev(c.coef[0])
    _ok(lib.mmrec_bpr_fwd_f32(P(T), P(T), P(T), P(dev["users"]), P(dev["pos"]), P(dev["neg"]), B, 64, 0, 1.0, P(loss.view), P(coef.view),
                              ws.p, s), "bpr_fwd")
    _ok(lib.mmrec_bpr_bwd_f32(P(T), P(T), P(T), P(dev["users"]), P(dev["pos"]), P(dev["neg"]), B, 64, P(cf), P(gdev), 1.0, P(G), P(G), P(G), s),
        "bpr_bwd")
    check_float(loss.get("loss")[0], ref["loss0"][0], ref["loss0"][1], "big bpr loss")
    check_float(coef.get("coef"), ref["coef0"][0], ref["coef0"][1], "big bpr coef")
    want = 0.25 + ref["dU"][0] + ref["dI0"][0]
    # gather_sqnorm / gather_scale_add and rows_reg (one term with ids, mode 0) on the same rows
    rows64 = c.U.astype(F64)
    for key, k_coef in (("gather", 0.5), ("reg", None)):
        ids_c = loc(big[key])
        S = float((rows64[ids_c] ** 2).sum())
        out = Guarded(1)
        if key == "gather":
            w2 = Workspace(4 * B)
            _ok(lib.mmrec_gather_sqnorm_fwd_f32(P(T), P(dev[key]), B, 64, P(out.view), w2.p, s), "gather_sqnorm")
            kd = _dev(np.array([k_coef], F32))
            _ok(lib.mmrec_gather_scale_add_bwd_f32(P(T), P(dev[key]), B, 64, P(kd), P(G), s), "gather_scale_add")
            assert out.get("out")[0] == S
            factor = k_coef
        else:
            w2, kc = Workspace(lib.mmrec_rows_reg_workspace_bytes(1, B)), Guarded(1)
            bt = (ctypes.c_int32 * 1)(B)
            _ok(lib.mmrec_rows_reg_fwd_f32(PA([T]), PA([dev[key]]), bt, 1, 64, 0, 2.0, P(out.view), P(kc.view), w2.p, s), "rows_reg_fwd")
            _ok(lib.mmrec_rows_reg_bwd_f32(PA([T]), PA([dev[key]]), bt, 1, 64, P(kc.view), P(gdev), PA([G]), s), "rows_reg_bwd")
            assert out.get("out")[0] == 2.0 * S and kc.get("coef")[0] == 4.0
            factor = 4.0 * c.g
        w2.ok(key)
        np.add.at(want, ids_c, factor * rows64[ids_c])
    torch.cuda.synchronize()
    _on_grid(np.abs(want) + 64, 2.0 ** -10, "big table")
    check_exact(G[_dev(named)].cpu().numpy(), want, "big gradient rows")
    quiet = np.setdiff1d(np.concatenate([np.arange(0, BIG_ROWS, 65537), np.arange(64), np.arange(BIG_ROWS - 64, BIG_ROWS)]), named)
    assert bool((G[_dev(quiet)] == 0.25).all()), "a row the batch does not name changed"
    # row_normalize over every row (n is int64), the backward into the gradient table
    Y = torch.empty_like(T)
    inv = torch.empty(BIG_ROWS, device="cuda:0")
    _ok(lib.mmrec_row_normalize_fwd_f32(P(T), BIG_ROWS, 64, 1e-12, P(Y), P(inv), s), "row_normalize_fwd")
    _ok(lib.mmrec_row_normalize_bwd_f32(P(Y), P(T), P(inv), BIG_ROWS, 64, P(G), s), "row_normalize_bwd")
    torch.cuda.synchronize()
    look = np.unique(np.concatenate([quiet, named]))
    Xs = _big_rows(look)
    Yr, invr, nrm = ev_normalize(Xs, EPS_NRM, F64)
    rr = gamma(ndot(64)) / 2 + (2 * E_DIV + 1) * U
    Yv, iv = Y[_dev(look)].cpu().numpy(), inv[_dev(look)].cpu().numpy()
    check_float(Yv, Yr, (rr + U) * np.abs(Yr) + TINY, "big row_normalize Y")
    check_float(iv, invr, rr * np.abs(invr), "big row_normalize inv")
    r, tol = ev_normalize_bwd(Yv, Xs, iv, F64)
    check_float(G[_dev(look)].cpu().numpy(), r, tol, "big row_normalize dX")
