"""GPU: seeded differential fuzz of LGMRec's hypergraph kernels (csrc/hypergraph.hip: mmrec_hyper_assign_fwd_f32 / _bwd_f32,
mmrec_hyper_layer_fwd_f32 / _bwd_f32; hip_ops.hyper_assign / hyper_layer / hyper_propagate) against float64 numpy of the formulas
as written here (`assign64`, `assign_bwd64`, `layer64`, `layer_bwd64`), never against another kernel.  The raw C ABI is called
over guarded, sentinel-filled outputs and a sentinel-filled workspace; EVERY CALL is checked against float64 of the fp32 arrays
that call was given (a later call's input is an earlier call's output: the chain of L layers is checked link by link).

    x = (a + g) / tau;  p = softmax(x, dim=1);  P = p * m / q  (no mask: P = p)            s = dP * m / q;  d a = p (s - <p, s>) / tau
    lat = P_i^T X;  X' = P_i lat;  U' = P_u lat
    dlat = P_u^T dU + P_i^T dX;  dP_u = dU lat^T;  dP_i = dX lat^T + X dlat^T;  dX = P_i dlat

The kernels' plan, read from the library (R = mmrec_hyper_rows_per_block(n)): a reduction over rows is cut into blocks of R rows;
inside a block four waves take R / 4 consecutive rows each, as an fma chain in row order; the four are added in order (3
additions), wave k of the finish adds the blocks k, k + 16, ... in order (ceil(blocks / 16) additions), the sixteen sums are added
in order (15).  A term of a reduced sum therefore meets at most
    n_red(n_a, n_b) = max(R_a, R_b) / 4 + 3 + ceil((blocks_a + blocks_b) / 16) + 15
roundings (the forward reduces one side, dlat both).  A row of an output is P[r][0] lat[0] and one fma per further hyperedge (H
roundings).  A dot product of the backward is, per lane, an fma chain over its 4 columns of dX then its 4 of X (8), then a 4-step
butterfly over the row's 16 lanes: 12 roundings.

Two acceptance modes; each case uses one.
  exact  every row's (a + g) holds one exact 0 (its hot hyperedge) and the rest <= -200 tau, so exp of the rest is 0 in fp32 and p
         is exactly one-hot; q is a power of two; E, dU, dX are multiples of 1/8 of magnitude <= 1/4 chosen so that every sum of
         magnitudes stays below 2^24 quanta (`exact_grid_ok`, asserted without a GPU): every sum is exact in any order.  lat, U',
         X', dlat (through dX and dP), dP must EQUAL the closed forms -- sums over the kept rows assigned to each hyperedge
         (`closed_*`, written with np.add.at over the hot index, not as matrix products) -- and d a must be exactly 0 (s_h - s_h at
         the hot entry, p = 0 elsewhere).  Hyperedge 0 holds only the rows on block and wave boundaries (first, last, 15 / 16,
         63 / 64, R - 1 / R ...), the last hyperedge holds no row at all (H >= 3).
  float  random logits, a quarter of the rows with a spread of several hundred (finite only with the row maximum subtracted).
         With u = 2^-24, gamma(n) = n u / (1 - n u), everything first order with a factor 1 + 2^-10 for the higher orders:
           assignment   x as computed is off by 2 u |x| (a sum, a quotient); the argument x_h - max by
                        eta_h = u (2 |x_h| + 2 max|x| + (max x - x_h)); the device's exp by E_EXP u
                        (tests/test_edge_softmax_fuzz_gpu.py); so e_h carries rho_h = eta_h + E_EXP u, the sum of H terms
                        sum_k p_k rho_k + gamma(H), the quotient u, the mask and 1 / q 2 u:
                          |P - ref| <= P_ref (rho_h + sum_k p_k rho_k + gamma(H) + 3 u) + 2^-125      (the last: underflow)
           its backward |d a - ref|_h <= (p_h / tau) (3 u |s_h| + gamma(H + 2) sum_k |p_k s_k|) + 3 u |ref| + 2^-125
           layer        every term of an output is a product of fp32 inputs that meets n roundings: |out - ref| <= gamma(n) MAG
                        with MAG the same formula over magnitudes:   lat: n_red, |P_i|^T |X|;   X', U': n_red + H,
                        |P| (|P_i|^T |X|);   dlat: n_red(I, U), MAG_dlat = |P_i|^T |dX| + |P_u|^T |dU|;   dX: n_red + H,
                        |P_i| MAG_dlat;   dP_u: 12, |dU| |lat|^T;   dP_i: gamma(12) |dX| |lat|^T + gamma(12 + n_red) |X| MAG_dlat^T
                        (the backward is given lat as an fp32 input).  Each plus n 2^-149 for results below the normal range.
The worst err / bound per family is printed by every case and recorded in EXPERIMENTS.md section 4.
`test_cases_span_every_axis`, `test_exact_cases_are_on_the_grid` and `test_E_EXP_covers_these_cases` need no GPU; the checker's own
tests (an fp32 emulation of the plan passes, planted errors do not) are in tests/test_hyper_cpu.py."""
import os

import numpy as np
import pytest
import torch

from tests.test_edge_softmax_fuzz_gpu import E_EXP, GUARD, SENTINEL
from tests.test_spmm_fuzz_gpu import U, _on, gamma

D = 64
HS = (1, 2, 3, 4, 7, 8)
BIG = 20011                                    # 313 blocks: the finish adds many partials
CASES = 40
SLACK = 1.0 + 2.0 ** -10
FLOOR = 2.0 ** -125
TINY = 2.0 ** -149
BAD_ARG, UNSUPPORTED = 10001, 10002


def _lib():
    from mmrec_amd import _lib as L
    if not os.path.exists(L.LIB_PATH):
        from mmrec_amd.build import build
        build(verbose=False)
    return L.load()


def rows_per_block(n):
    return int(_lib().mmrec_hyper_rows_per_block(int(n)))


def blocks(n):
    return -(-n // rows_per_block(n)) if n > 0 else 0


def n_red(n_a, n_b=0):
    """the roundings a term of a reduction over the rows of one side (forward) or of both (dlat) meets"""
    r = max(rows_per_block(n_a) if n_a else 0, rows_per_block(n_b) if n_b else 0)
    return r // 4 + 3 + -(-(blocks(n_a) + blocks(n_b)) // 16) + 15


def axis_n():
    r = rows_per_block(1)
    return tuple(sorted({0, 1, 2, 15, 16, 17, 63, 64, 65, r - 1, r, r + 1, 2 * r + 1}))


def boundary_rows(n):
    r = rows_per_block(max(n, 1))
    want = {0, n - 1, 15, 16, 31, 32, 63, 64, r - 1, r, 2 * r - 1, 2 * r, n - 2, (n // r) * r - 1, (n // r) * r}
    return np.array(sorted(x for x in want if 0 <= x < n), np.int64)


class Case:
    pass


def _side(c, rng, n):
    """one side's logits, noise, mask, hot index (exact) and the gradient dP its backward is given"""
    H = c.H
    s = Case()
    s.n = n
    if c.exact:
        hot = np.zeros(n, np.int64)
        if H == 2:
            hot[:] = 1
        elif H >= 3:
            hot = rng.integers(1, H - 1, n)                               # hyperedge H - 1 holds no row
        if H >= 2:
            hot[boundary_rows(n)] = 0                                     # hyperedge 0: the rows on block and wave boundaries only
        g = rng.integers(-8, 9, (n, H)) / 4.0
        drop = c.tau * (210.0 + rng.integers(0, 100, (n, H)))
        a = -g - drop
        a[np.arange(n), hot] = -g[np.arange(n), hot]
        s.hot = hot
        s.dP = rng.integers(-8, 9, (n, H)) / 8.0
    else:
        a = rng.standard_normal((n, H)) * 2.0
        wide = rng.random(n) < 0.25
        a[wide] *= 150.0                                                  # a spread of several hundred inside a row
        g = -np.log(rng.exponential(1.0, (n, H)))
        s.dP = rng.standard_normal((n, H))
    s.a, s.g, s.dP = (np.ascontiguousarray(x, np.float32) for x in (a, g, s.dP))
    s.m = None
    if c.masked:
        m = (rng.random((n, H)) < 0.6).astype(np.float32)
        if n > 2:
            m[rng.integers(0, n, max(1, n // 16))] = 0.0                  # rows whose mask is all zero
        s.m = m
    return s


def case(k):
    ns = axis_n()
    c = Case()
    c.k = k
    c.I, c.U = ns[k % len(ns)], ns[(3 * k + k // len(ns) + 5) % len(ns)]
    c.H = HS[(k + k // 6) % 6]
    c.L = 1 + (k // 8) % 2
    c.masked = (k // 3) % 2 == 0
    c.tau = (0.2, 1.0)[(k // 5) % 2]
    c.exact = (k + k // 4) % 2 == 0
    c.q = (0.5, 0.25)[(k // 7) % 2]
    if k in (9, 27):
        c.q, c.masked = 0.4, True                                         # an inexact 1 / q: float mode only
    if k == 5:
        c.I, c.U = BIG, 2 * rows_per_block(1) + 1                         # the large table in both modes
    if k == 11:
        c.I, c.U = BIG, BIG
    if c.exact and c.L == 2 and max(c.I, c.U) > 65:
        c.L = 1                                                           # two exact layers stay on the grid up to 65 rows
    c.amp = 2
    if c.exact and (c.L == 2 or max(c.I, c.U) > 1000):
        c.q, c.amp = 0.5, 1
    c.in_null, c.out_null = k % 4, (k // 4) % 8                           # bit 0: dU NULL, bit 1: dX NULL; bits: dP_i, dP_u, dX_prev NULL
    rng = np.random.default_rng(4000 + k)
    c.i, c.u = _side(c, rng, c.I), _side(c, rng, c.U)
    if c.exact:
        E, dU, dX = (rng.integers(-c.amp, c.amp + 1, (n, D)) / 8.0 for n in (c.I, c.U, c.I))
    else:
        E, dU, dX = rng.standard_normal((c.I, D)) * 0.3, rng.standard_normal((c.U, D)), rng.standard_normal((c.I, D))
    c.E, c.dU, c.dX = (np.ascontiguousarray(x, np.float32) for x in (E, dU, dX))
    return c


def name_of(c):
    return "case %d (I %d U %d H %d L %d %s%s tau %g q %g nulls in %d out %d)" % (
        c.k, c.I, c.U, c.H, c.L, "exact" if c.exact else "float", " masked" if c.masked else "", c.tau, c.q, c.in_null, c.out_null)


def float_cases():
    return [c for c in map(case, range(CASES)) if not c.exact]


# ------------------------------------------------------------------------------------------------ host references (float64)
def f64(x):
    return None if x is None else np.asarray(x, np.float64)


def _x64(a, g, tau):
    return (f64(a) + f64(g)) / np.float64(np.float32(tau))


def assign64(a, g, m, tau, q):
    """-> (P, p) in float64"""
    x = _x64(a, g, tau)
    if x.shape[0] == 0:
        return x.copy(), x.copy()
    e = np.exp(x - x.max(axis=1, keepdims=True))
    p = e / e.sum(axis=1, keepdims=True)
    return (p if m is None else p * f64(m) / np.float64(np.float32(q))), p


def assign_bwd64(p, m, dP, tau, q):
    p, dP = f64(p), f64(dP)
    s = dP if m is None else dP * f64(m) / np.float64(np.float32(q))
    return p * (s - (p * s).sum(axis=1, keepdims=True)) / np.float64(np.float32(tau)), s


def layer64(P_i, P_u, X):
    P_i, P_u, X = f64(P_i), f64(P_u), f64(X)
    lat = P_i.T @ X
    return lat, P_i @ lat, (None if P_u is None else P_u @ lat)


def layer_bwd64(P_i, P_u, X, lat, dU, dX):
    """-> (dP_i, dP_u, dX_prev, dlat); a None gradient is zeros"""
    P_i, P_u, X, lat = f64(P_i), f64(P_u), f64(X), f64(lat)
    dU = np.zeros((P_u.shape[0], D)) if dU is None else f64(dU)
    dX = np.zeros((P_i.shape[0], D)) if dX is None else f64(dX)
    dlat = P_u.T @ dU + P_i.T @ dX
    return dX @ lat.T + X @ dlat.T, dU @ lat.T, P_i @ dlat, dlat


# ------------------------------------------------------------------------------------------------ the float mode's bounds
def assign_bound(a, g, m, tau, q):
    """-> (P ref, bound on P, p ref, bound on p) of the module docstring"""
    P, p = assign64(a, g, m, tau, q)
    if p.shape[0] == 0:
        return P, P.copy(), p, p.copy()
    x = _x64(a, g, tau)
    xmax = np.abs(x).max(axis=1, keepdims=True)
    eta = U * (2 * np.abs(x) + 2 * xmax + (x.max(axis=1, keepdims=True) - x))
    rho = eta + E_EXP * U
    rel = rho + (p * rho).sum(axis=1, keepdims=True) + gamma(a.shape[1]) + 3 * U
    return P, SLACK * rel * np.abs(P) + FLOOR, p, SLACK * rel * p + FLOOR


def assign_bwd_bound(p, m, dP, tau, q):
    ref, s = assign_bwd64(p, m, dP, tau, q)
    H = np.asarray(p).shape[1]
    t = np.float64(np.float32(tau))
    b = (f64(p) / t) * (3 * U * np.abs(s) + gamma(H + 2) * (f64(p) * np.abs(s)).sum(axis=1, keepdims=True)) + 3 * U * np.abs(ref)
    return ref, SLACK * b + FLOOR


def layer_bounds(P_i, P_u, X):
    """-> {name: (ref, bound)} for lat, X_out, U_out"""
    lat, xo, uo = layer64(P_i, P_u, X)
    I, H = np.asarray(P_i).shape
    n = n_red(I)
    mag = np.abs(f64(P_i)).T @ np.abs(f64(X))
    out = {"lat": (lat, SLACK * gamma(n) * mag + n * TINY),
           "X_out": (xo, SLACK * gamma(n + H) * (np.abs(f64(P_i)) @ mag) + (n + H) * TINY)}
    if P_u is not None:
        out["U_out"] = (uo, SLACK * gamma(n + H) * (np.abs(f64(P_u)) @ mag) + (n + H) * TINY)
    return out


def layer_bwd_bounds(P_i, P_u, X, lat, dU, dX):
    """-> {name: (ref, bound)} for dP_i, dP_u, dX_prev"""
    dpi, dpu, dxp, _ = layer_bwd64(P_i, P_u, X, lat, dU, dX)
    I, H = np.asarray(P_i).shape
    Un = np.asarray(P_u).shape[0]
    n = n_red(I if dX is not None else 0, Un if dU is not None else 0)
    aU = np.zeros((Un, D)) if dU is None else np.abs(f64(dU))
    aX = np.zeros((I, D)) if dX is None else np.abs(f64(dX))
    mag = np.abs(f64(P_i)).T @ aX + np.abs(f64(P_u)).T @ aU
    al = np.abs(f64(lat))
    return {"dP_i": (dpi, SLACK * (gamma(12) * (aX @ al.T) + gamma(12 + n) * (np.abs(f64(X)) @ mag.T)) + (12 + n) * TINY),
            "dP_u": (dpu, SLACK * gamma(12) * (aU @ al.T) + 12 * TINY),
            "dX_prev": (dxp, SLACK * gamma(n + H) * (np.abs(f64(P_i)) @ mag) + (n + H) * TINY)}


# ------------------------------------------------------------------------------------------------ the exact mode's closed forms
def closed_weights(c, s):
    """-> w [n]: the one nonzero of a row of P, at s.hot: 1 / q where the hot entry is kept, 0 where it is dropped, 1 without a mask"""
    if s.m is None:
        return np.ones(s.n)
    return f64(s.m)[np.arange(s.n), s.hot] / c.q


def closed_P(c, s):
    P = np.zeros((s.n, c.H))
    P[np.arange(s.n), s.hot] = closed_weights(c, s)
    return P


def closed_layer(c, X, want_u=True):
    """sums over the kept rows assigned to each hyperedge -> (lat, X_out, U_out)"""
    wi, wu = closed_weights(c, c.i), closed_weights(c, c.u)
    lat = np.zeros((c.H, D))
    np.add.at(lat, c.i.hot, wi[:, None] * f64(X))
    return lat, wi[:, None] * lat[c.i.hot], (wu[:, None] * lat[c.u.hot] if want_u else None)


def closed_layer_bwd(c, X, lat, dU, dX):
    """-> (dP_i, dP_u, dX_prev, dlat)"""
    wi, wu = closed_weights(c, c.i), closed_weights(c, c.u)
    dlat = np.zeros((c.H, D))
    if dU is not None:
        np.add.at(dlat, c.u.hot, wu[:, None] * f64(dU))
    if dX is not None:
        np.add.at(dlat, c.i.hot, wi[:, None] * f64(dX))
    X = f64(X)
    dpi = np.stack([(X * dlat[h]).sum(axis=1) + (0.0 if dX is None else (f64(dX) * lat[h]).sum(axis=1)) for h in range(c.H)], axis=1)
    dpu = np.stack([np.zeros(c.U) if dU is None else (f64(dU) * lat[h]).sum(axis=1) for h in range(c.H)], axis=1)
    return dpi.reshape(c.I, c.H), dpu.reshape(c.U, c.H), wi[:, None] * dlat[c.i.hot], dlat


def exact_chain(c):
    """the whole exact case in closed form -> lists per layer of (X_prev, lat, X_out, U_out) and of (dP_i, dP_u, dX_prev, dU, dX)"""
    fwd, X = [], f64(c.E)
    for l in range(c.L):
        lat, xo, uo = closed_layer(c, X, l == c.L - 1)
        fwd.append((X, lat, xo, uo))
        X = xo
    dU = None if c.in_null & 1 else f64(c.dU)
    dX = None if c.in_null & 2 else f64(c.dX)
    bwd = []
    for l in reversed(range(c.L)):
        Xp, lat = fwd[l][0], fwd[l][1]
        dpi, dpu, dxp, dlat = closed_layer_bwd(c, Xp, lat, dU, dX)
        bwd.append((dpi, dpu, dxp, dU, dX, dlat))
        dU, dX = None, dxp
    return fwd, bwd


def exact_grid_ok(c):
    """every sum of an exact case -- in ANY order -- is exactly representable: the sum of its terms' magnitudes, in units of the
    quantum of its terms, stays below 2^24.  Checked on the magnitudes' chain (all weights and values replaced by |.|)."""
    a_E, a_dU, a_dX = np.abs(f64(c.E)), np.abs(f64(c.dU)), np.abs(f64(c.dX))
    ok, X, quantum = True, a_E, 1.0 / 8
    lats = []
    for l in range(c.L):
        lat, xo, uo = closed_layer(c, X, True)                            # weights are >= 0: the closed form over |X| IS the magnitude sum
        for t in (lat, xo, uo):
            ok &= bool(t.size == 0 or t.max() / quantum < 2.0 ** 24)
        lats.append((X, lat))
        X = xo
    dU, dX = a_dU, a_dX
    for l in reversed(range(c.L)):
        Xp, lat = lats[l]
        dpi, dpu, dxp, dlat = closed_layer_bwd(c, Xp, lat, dU, dX)
        for t, qn in ((dlat, quantum), (dxp, quantum), (dpi, quantum * quantum), (dpu, quantum * quantum)):
            ok &= bool(t.size == 0 or t.max() / qn < 2.0 ** 24)
        dU, dX = None, dxp
    return ok


# ------------------------------------------------------------------------------------------------ comparison
def _arr(got):
    return got.detach().cpu().double().numpy() if isinstance(got, torch.Tensor) else np.asarray(got, np.float64)


def compare(got, ref, bound, name):
    """bound None: EQUAL.  Returns the worst err / bound (0 in exact mode)."""
    g = _arr(got)
    assert g.shape == ref.shape, (name, g.shape, ref.shape)
    if not g.size:
        return 0.0
    if bound is None:
        bad = g != ref
        assert not bad.any(), (name, "exact mismatch", int(bad.sum()), "first at", np.argwhere(bad)[0].tolist(),
                               float(g[bad][0]), float(ref[bad][0]))
        return 0.0
    assert np.isfinite(ref).all() and np.isfinite(g).all(), (name, "not finite", int((~np.isfinite(g)).sum()))
    err = np.abs(g - ref)
    viol = err > bound
    assert not viol.any(), (name, "beyond the bound", int(viol.sum()), "first at", np.argwhere(viol)[0].tolist(),
                            float(g[viol][0]), float(ref[viol][0]), float(bound[viol][0]))
    return float((err / bound).max(initial=0.0))


def check_assign(c, s, P, p, name):
    if c.exact:
        onehot = np.zeros((s.n, c.H))
        onehot[np.arange(s.n), s.hot] = 1.0
        w = compare(P, closed_P(c, s), None, name + " P")
        return w if p is None else max(w, compare(p, onehot, None, name + " p"))
    ref, b, pref, pb = assign_bound(s.a, s.g, s.m, c.tau, c.q)
    w = compare(P, ref, b, name + " P")
    return w if p is None else max(w, compare(p, pref, pb, name + " p"))


def check_assign_bwd(c, s, p_in, da, name):
    if c.exact:
        return compare(da, np.zeros((s.n, c.H)), None, name + " d a")
    ref, b = assign_bwd_bound(p_in, s.m, s.dP, c.tau, c.q)
    return compare(da, ref, b, name + " d a")


def check_layer(c, P_i, P_u, X, got, closed, name):
    """got: {name: array}; closed: (lat, X_out, U_out) of the exact mode"""
    if c.exact:
        refs = dict(zip(("lat", "X_out", "U_out"), closed))
        return max([compare(v, refs[k], None, name + " " + k) for k, v in got.items()] + [0.0])
    bounds = layer_bounds(P_i, P_u if "U_out" in got else None, X)
    return max([compare(v, *bounds[k], name + " " + k) for k, v in got.items()] + [0.0])


def check_layer_bwd(c, P_i, P_u, X, lat, dU, dX, got, closed, name):
    if c.exact:
        refs = dict(zip(("dP_i", "dP_u", "dX_prev"), closed))
        return max([compare(v, refs[k], None, name + " " + k) for k, v in got.items()] + [0.0])
    bounds = layer_bwd_bounds(P_i, P_u, X, lat, dU, dX)
    return max([compare(v, *bounds[k], name + " " + k) for k, v in got.items()] + [0.0])


# ------------------------------------------------------------------------------------------------ no GPU: the constant, the axes
def test_E_EXP_covers_these_cases():
    """the exp constant taken from the segment softmax's fuzz holds on these cases' arguments x - max too (same method)"""
    worst = 0.0
    for c in float_cases():
        for s in (c.i, c.u):
            if not s.n:
                continue
            x = _x64(s.a, s.g, c.tau)
            a = (x - x.max(axis=1, keepdims=True)).astype(np.float32)
            a = a[a > -87.0]
            e32, e64 = np.exp(a).astype(np.float64), np.exp(a.astype(np.float64))
            worst = max(worst, float((np.abs(e32 - e64) / (U * e64)).max(initial=0.0)))
    print("fp32 exp against float64 on these cases, worst error in units of u |value|: %.3f" % worst)
    assert 4.0 * worst <= E_EXP, (worst, E_EXP)


def test_cases_span_every_axis():
    cs = [case(k) for k in range(CASES)]
    ns = axis_n()
    r = rows_per_block(1)
    assert r % 64 == 0 and r == rows_per_block(BIG) and {0, 1, 2, 63, 64, 65, r - 1, r, r + 1, 2 * r + 1} <= set(ns)
    assert set(ns) <= {c.I for c in cs} and set(ns) <= {c.U for c in cs}
    for mode in (True, False):
        m = [c for c in cs if c.exact == mode]
        assert {c.H for c in m} == set(HS) and {c.L for c in m} == {1, 2} and {c.masked for c in m} == {True, False}, mode
        assert {c.tau for c in m} == {0.2, 1.0} and {0.5, 0.25} <= {c.q for c in m if c.masked}, mode
        assert {c.in_null for c in m} == set(range(4)) and {c.out_null for c in m} == set(range(8)), mode
        big = [c for c in m if c.I == BIG]
        assert len(big) == 1 and blocks(BIG) > 16 * 16                    # every wave of the finish adds many partials
    assert any(c.U == BIG for c in cs)
    assert all(c.q in (0.5, 0.25) for c in cs if c.exact) and any(c.q == 0.4 and c.masked for c in cs if not c.exact)
    assert {(c.in_null, c.out_null) for c in cs} == {(a, b) for a in range(4) for b in range(8)}      # every NULL combination
    for L in (1, 2):
        assert {c.in_null for c in cs if c.L == L} == set(range(4))
    wide = [float((_x64(s.a, s.g, c.tau).max(axis=1) - _x64(s.a, s.g, c.tau).min(axis=1)).max())
            for c in cs if not c.exact for s in (c.i, c.u) if s.n > 8 and c.H > 1]
    assert max(wide) > 200.0 and sum(w > 200.0 for w in wide) > len(wide) // 2      # fp32 exp overflows at 88.7: finite only with the maximum subtracted
    for c in cs:
        if not c.exact:
            continue
        for s in (c.i, c.u):
            x = (s.a.astype(np.float32) + s.g.astype(np.float32)).astype(np.float64)                  # the kernel's own sum
            assert np.array_equal(x[np.arange(s.n), s.hot], np.zeros(s.n))
            if s.n and c.H > 1:
                assert float(x[~np.eye(c.H, dtype=bool)[s.hot]].max()) <= -200.0 * c.tau
            if c.H >= 3 and s.n:
                assert not (s.hot == c.H - 1).any()                      # a hyperedge with no rows
            if c.H >= 2 and s.n:
                assert set(np.flatnonzero(s.hot == 0)) == set(boundary_rows(s.n))
            if s.m is not None and s.n > 2:
                assert (s.m.sum(axis=1) == 0).any() and (s.m[np.arange(s.n), s.hot] == 0).any()       # dropped rows
            P, p = assign64(s.a, s.g, s.m, c.tau, c.q)
            assert np.array_equal(P.astype(np.float32).astype(np.float64), closed_P(c, s))            # the construction IS the formula
    e = next(c for c in cs if c.exact and c.I == BIG)
    assert {r - 1, r, BIG - 1} <= set(np.flatnonzero(e.i.hot == 0))


def test_exact_cases_are_on_the_grid():
    for k in range(CASES):
        c = case(k)
        if c.exact:
            assert exact_grid_ok(c), name_of(c)
            for t in (c.E, c.dU, c.dX):
                assert np.array_equal(t * 8, np.round(t * 8)) and float(np.abs(t).max(initial=0)) <= 0.25
            fwd, bwd = exact_chain(c)                                     # the closed forms ARE the formulas (float64 is exact here)
            P_i, P_u = closed_P(c, c.i), closed_P(c, c.u)
            X = f64(c.E)
            for (Xp, lat, xo, uo) in fwd:
                r_lat, r_x, r_u = layer64(P_i, P_u, Xp)
                assert np.array_equal(lat, r_lat) and np.array_equal(xo, r_x) and (uo is None or np.array_equal(uo, r_u))
            for (dpi, dpu, dxp, dU, dX, dlat), (Xp, lat, _, _) in zip(bwd, reversed(fwd)):
                r = layer_bwd64(P_i, P_u, Xp, lat, dU, dX)
                assert all(np.array_equal(a, b) for a, b in zip((dpi, dpu, dxp, dlat), r))


# ------------------------------------------------------------------------------------------------ GPU: the raw C ABI, guarded
def _guarded(n):
    buf = torch.full((n + 2 * GUARD,), SENTINEL, dtype=torch.int32, device="cuda:0")
    return buf, buf[GUARD:GUARD + n].view(torch.float32)


def _guards_ok(buf, n, name):
    b = buf.cpu().numpy()
    assert (b[:GUARD] == SENTINEL).all() and (b[GUARD + n:] == SENTINEL).all(), (name, "wrote outside the output")
    assert not (b[GUARD:GUARD + n] == SENTINEL).any(), (name, "entries never written", int((b[GUARD:GUARD + n] == SENTINEL).sum()))


def _workspace(I, Un, H):
    nbytes = int(_lib().mmrec_hyper_workspace_bytes(I, Un, H))
    assert nbytes > 0
    return torch.full((nbytes // 4 + GUARD,), SENTINEL, dtype=torch.int32, device="cuda:0"), nbytes // 4


def _workspace_ok(ws, n, name):
    assert bool((ws[n:] == SENTINEL).all()), (name, "wrote beyond the workspace")


def _outs(shapes):
    """{name: shape or None} -> ({name: (buffer, view)}, {name: pointer or None})"""
    from mmrec_amd import hip_ops
    held = {k: _guarded(int(np.prod(s))) for k, s in shapes.items() if s is not None}
    return held, {k: (hip_ops._p(held[k][1]) if k in held else None) for k in shapes}


def _collect(held, shapes, name):
    torch.cuda.synchronize()
    out = {}
    for k, (buf, view) in held.items():
        _guards_ok(buf, view.numel(), name + " " + k)
        out[k] = view.clone().view(*shapes[k])
    return out


def raw_assign(c, s, name):
    from mmrec_amd import hip_ops
    p_, lib = hip_ops._p, _lib()
    a, g, m = _on(s.a), _on(s.g), (None if s.m is None else _on(s.m))
    shapes = {"P": (s.n, c.H), "p": (s.n, c.H) if s.m is not None else None}
    held, ptr = _outs(shapes)
    rc = lib.mmrec_hyper_assign_fwd_f32(p_(a), p_(g), p_(m), s.n, c.H, c.tau, c.q, ptr["P"], ptr["p"], hip_ops._stream())
    assert rc == 0, (name, rc)
    out = _collect(held, shapes, name)
    return out["P"], out.get("p")


def raw_assign_bwd(c, s, p_in, name):
    from mmrec_amd import hip_ops
    p_, lib = hip_ops._p, _lib()
    m, dP = (None if s.m is None else _on(s.m)), _on(s.dP)
    shapes = {"da": (s.n, c.H)}
    held, ptr = _outs(shapes)
    rc = lib.mmrec_hyper_assign_bwd_f32(p_(p_in), p_(m), p_(dP), s.n, c.H, c.tau, c.q, ptr["da"], hip_ops._stream())
    assert rc == 0, (name, rc)
    return _collect(held, shapes, name)["da"]


def raw_layer(c, P_i, P_u, X, want_u, name):
    from mmrec_amd import hip_ops
    p_, lib = hip_ops._p, _lib()
    shapes = {"lat": (c.H, D), "X_out": (c.I, D), "U_out": (c.U, D) if want_u else None}
    held, ptr = _outs(shapes)
    ws, n_ws = _workspace(c.I, c.U, c.H)
    rc = lib.mmrec_hyper_layer_fwd_f32(p_(P_i), p_(P_u) if want_u else None, p_(X), c.I, c.U, c.H, D, ptr["U_out"], ptr["X_out"],
                                       ptr["lat"], p_(ws), hip_ops._stream())
    assert rc == 0, (name, rc)
    out = _collect(held, shapes, name)
    _workspace_ok(ws, n_ws, name)
    return out


def raw_layer_bwd(c, P_i, P_u, X, lat, dU, dX, out_null, name):
    from mmrec_amd import hip_ops
    p_, lib = hip_ops._p, _lib()
    shapes = {"dP_i": None if out_null & 1 else (c.I, c.H), "dP_u": None if out_null & 2 else (c.U, c.H),
              "dX_prev": None if out_null & 4 else (c.I, D)}
    held, ptr = _outs(shapes)
    ws, n_ws = _workspace(c.I, c.U, c.H)
    rc = lib.mmrec_hyper_layer_bwd_f32(p_(P_i), p_(P_u), p_(X), p_(lat), p_(dU), p_(dX), c.I, c.U, c.H, D, ptr["dP_i"], ptr["dP_u"],
                                       ptr["dX_prev"], p_(ws), hip_ops._stream())
    assert rc == 0, (name, rc)
    out = _collect(held, shapes, name)
    _workspace_ok(ws, n_ws, name)
    return out


def _bits(t):
    return t.contiguous().view(torch.int32)


def run_case(c, check=True):
    """every call of the case through the raw ABI -> (all outputs in call order, worst err / bound per family)"""
    name = name_of(c)
    outs, worst = [], {"assign": 0.0, "assign_bwd": 0.0, "layer": 0.0, "layer_bwd": 0.0}
    Ps = []
    for tag, s in (("i", c.i), ("u", c.u)):
        P, p = raw_assign(c, s, name + " assign " + tag)
        p_in = P if p is None else p
        da = raw_assign_bwd(c, s, p_in, name + " assign bwd " + tag)
        outs += [P, da] + ([] if p is None else [p])
        Ps.append(P)
        if check:
            worst["assign"] = max(worst["assign"], check_assign(c, s, P, p, name + " " + tag))
            worst["assign_bwd"] = max(worst["assign_bwd"], check_assign_bwd(c, s, p_in.cpu().numpy(), da, name + " " + tag))
    P_i, P_u = Ps
    closed_f, closed_b = exact_chain(c) if (c.exact and check) else (None, None)
    X, kept = _on(c.E), []
    for l in range(c.L):
        want_u = l == c.L - 1
        got = raw_layer(c, P_i, P_u, X, want_u, name + " layer %d" % l)
        outs += list(got.values())
        if check:
            worst["layer"] = max(worst["layer"], check_layer(c, P_i.cpu().numpy(), P_u.cpu().numpy(), X.cpu().numpy(), got,
                                                             closed_f[l][1:] if c.exact else None, name + " layer %d" % l))
        kept.append((X, got["lat"]))
        X = got["X_out"]
    dU = None if c.in_null & 1 else _on(c.dU)
    dX = None if c.in_null & 2 else _on(c.dX)
    for j, l in enumerate(reversed(range(c.L))):
        Xp, lat = kept[l]
        out_null = c.out_null if l == 0 else 0                            # an inner link of the chain needs its dX_prev
        got = raw_layer_bwd(c, P_i, P_u, Xp, lat, dU, dX, out_null, name + " layer bwd %d" % l)
        outs += list(got.values())
        if check:
            n = lambda t: None if t is None else t.cpu().numpy()          # noqa: E731
            worst["layer_bwd"] = max(worst["layer_bwd"], check_layer_bwd(
                c, n(P_i), n(P_u), n(Xp), n(lat), n(dU), n(dX), got, closed_b[j][:3] if c.exact else None, name + " layer bwd %d" % l))
        dU, dX = None, got.get("dX_prev")
    return outs, worst


@pytest.mark.gpu
@pytest.mark.parametrize("k", range(CASES))
def test_hyper_fuzz(k):
    c = case(k)
    outs, worst = run_case(c)
    print("%s: worst err / bound %s" % (name_of(c), " ".join("%s %.3f" % kv for kv in sorted(worst.items()))))
    again, _ = run_case(c, check=False)                                   # the same calls again: the same bits, both directions
    assert len(outs) == len(again) and all(torch.equal(_bits(a), _bits(b)) for a, b in zip(outs, again)), name_of(c)


@pytest.mark.gpu
def test_unserved_shapes_are_refused_by_the_library_and_served_by_torch_bit_for_bit():
    """H = 9, a non-contiguous E, width 32: the C ABI says UNSUPPORTED where it can see the shape, the wrappers take `*_torch`"""
    from mmrec_amd import hip_ops
    lib = _lib()
    assert lib.mmrec_hyper_layer_fwd_f32(None, None, None, 5, 5, 9, 64, None, None, None, None, None) == UNSUPPORTED
    assert lib.mmrec_hyper_layer_fwd_f32(None, None, None, 5, 5, 4, 32, None, None, None, None, None) == UNSUPPORTED
    assert lib.mmrec_hyper_assign_fwd_f32(None, None, None, 5, 9, 1.0, 1.0, None, None, None) == UNSUPPORTED
    gen = torch.Generator(device="cuda:0").manual_seed(11)
    r = lambda *s: torch.randn(*s, device="cuda:0", generator=gen)        # noqa: E731
    I, Un = 70, 45
    for H, width, strided in ((9, 64, False), (4, 128, True), (4, 32, False)):
        a_i, g_i, a_u, g_u, E = r(I, H), r(I, H), r(Un, H), r(Un, H), r(I, width)
        m_i = (torch.rand(I, H, device="cuda:0", generator=gen) < 0.5).float()
        runs = []
        for fused in (True, False):
            # the assignment is unserved for H = 9 only: elsewhere both runs are given the torch composition's P
            assign = hip_ops.hyper_assign if (fused and H > 8) else hip_ops.hyper_assign_torch
            la, lu, e = a_i.clone().requires_grad_(), a_u.clone().requires_grad_(), E.clone().requires_grad_()
            ev = e[:, ::2] if strided else e                              # a non-contiguous [I, 64] view of a wider table
            assert H <= 8 or not hip_ops.hyper_assign_served(la, g_i, m_i)
            P_i, P_u = assign(la, g_i, m_i, 0.2, 0.5), assign(lu, g_u, None, 0.2, 0.5)
            assert not hip_ops.hyper_layer_served(P_i, P_u, ev)
            uo, xo = hip_ops.hyper_propagate(P_i, P_u, ev, 2) if fused else _propagate_torch(P_i, P_u, ev, 2)
            one_u, one_x = hip_ops.hyper_layer(P_i, P_u, ev) if fused else hip_ops.hyper_layer_torch(P_i, P_u, ev)
            (uo.sum() + (xo * xo).sum() + (one_u * one_x[:Un].flip(0)).sum()).backward()
            runs.append((uo.detach(), xo.detach(), one_u.detach(), la.grad, lu.grad, e.grad))
        for a, b in zip(*runs):
            assert torch.equal(_bits(a), _bits(b))
        assert float(runs[0][3].abs().max()) > 0


def _propagate_torch(P_i, P_u, X, L):
    from mmrec_amd import hip_ops
    for _ in range(L):
        uo, X = hip_ops.hyper_layer_torch(P_i, P_u, X)
    return uo, X


# ------------------------------------------------------------------------------------------------ GPU: the wrappers
def _wrapper_inputs(I, Un, H, seed, masked):
    rng = np.random.default_rng(seed)
    t = lambda *s: rng.standard_normal(s).astype(np.float32)             # noqa: E731
    d = {"a_i": t(I, H) * 2, "a_u": t(Un, H) * 2, "E": t(I, D) * 0.3, "w_u": t(Un, D), "w_x": t(I, D),
         "g_i": -np.log(rng.exponential(1.0, (I, H))).astype(np.float32), "g_u": -np.log(rng.exponential(1.0, (Un, H))).astype(np.float32)}
    d["m_i"] = (rng.random((I, H)) < 0.5).astype(np.float32) if masked else None
    d["m_u"] = (rng.random((Un, H)) < 0.5).astype(np.float32) if masked else None
    return d


def _wrapper_run(d, L, tau, q, dtype, device, fused):
    """loss = <U_L, w_u> + <X_L, w_x> through assign + propagate -> (U_L, X_L, d a_i, d a_u, d E, P_i, P_u)"""
    from mmrec_amd import hip_ops
    T = lambda x, grad=False: None if x is None else torch.from_numpy(x).to(device=device, dtype=dtype).requires_grad_(grad)   # noqa: E731
    a_i, a_u, E = T(d["a_i"], True), T(d["a_u"], True), T(d["E"], True)
    assign = hip_ops.hyper_assign if fused else hip_ops.hyper_assign_torch
    P_i = assign(a_i, T(d["g_i"]), T(d["m_i"]), tau, q)
    P_u = assign(a_u, T(d["g_u"]), T(d["m_u"]), tau, q)
    if fused:
        assert hip_ops.hyper_layer_served(P_i, P_u, E)
        uo, xo = hip_ops.hyper_propagate(P_i, P_u, E, L)
    else:
        uo, xo = _propagate_torch(P_i, P_u, E, L)
    ((uo * T(d["w_u"])).sum() + (xo * T(d["w_x"])).sum()).backward()
    return [t.detach() for t in (uo, xo, a_i.grad, a_u.grad, E.grad, P_i, P_u)]


def wrapper_bounds(d, L, tau, q, ref):
    """A first-order bound for the whole chain, from the per-call bounds of the module docstring: every term of an output is a
    product of inputs, of entries of P (each with a relative error of at most kappa u, the worst of `assign_bound` over the
    entries that are not dropped -- 2 L of them in a term of the forward, one more in the backward, through the softmax's
    Jacobian) and of roundings: L (n_red + H) in the forward, L (n_red_b + 12 + H) more in the backward, H + 8 in the
    assignment's.  So |got - ref| <= gamma(K) MAG with MAG the same chain over magnitudes (every subtraction an addition),
    evaluated in float64 from the reference's P.  Logits here are moderate (|x| of a few tens), so kappa is a few hundred."""
    I, H = d["a_i"].shape
    Un = d["a_u"].shape[0]
    kappa = 0.0
    for a, g, m in ((d["a_i"], d["g_i"], d["m_i"]), (d["a_u"], d["g_u"], d["m_u"])):
        P, b, p, pb = assign_bound(a, g, m, tau, q)
        kappa = max(kappa, float(((pb - FLOOR) / np.maximum(p, 1e-300)).max()) / U)
    k_f = 2 * L * kappa + L * (n_red(I) + H)
    k_b = k_f + kappa + L * (n_red(I, Un) + 12 + H) + H + 8
    P_i, P_u = np.abs(f64(ref[5].cpu().numpy())), np.abs(f64(ref[6].cpu().numpy()))
    t64 = np.float64(np.float32(tau))
    X, fwd = np.abs(f64(d["E"])), []
    for l in range(L):
        lat = P_i.T @ X
        fwd.append((X, lat))
        X = P_i @ lat
    mag_u, mag_x = P_u @ fwd[-1][1], X
    dU, dX = np.abs(f64(d["w_u"])), np.abs(f64(d["w_x"]))
    dPi, dPu = np.zeros_like(P_i), np.zeros_like(P_u)
    for l in reversed(range(L)):
        Xp, lat = fwd[l]
        dlat = P_i.T @ dX + (P_u.T @ dU if l == L - 1 else 0.0)
        dPi += dX @ lat.T + Xp @ dlat.T
        if l == L - 1:
            dPu += dU @ lat.T
        dX = P_i @ dlat
    out = [gamma(k_f) * mag_u, gamma(k_f) * mag_x]
    for dP, a, g, m in ((dPi, d["a_i"], d["g_i"], d["m_i"]), (dPu, d["a_u"], d["g_u"], d["m_u"])):
        p = assign64(a, g, m, tau, q)[1]
        s = dP if m is None else dP * f64(m) / np.float64(np.float32(q))
        out.append(gamma(k_b) * p * (s + (p * s).sum(axis=1, keepdims=True)) / t64)
    out.append(gamma(k_b) * dX)
    return [SLACK * b + FLOOR for b in out]


@pytest.mark.gpu
@pytest.mark.parametrize("L,H,masked,I,Un", [(1, 4, True, 129, 70), (2, 4, True, 65, 200), (2, 8, False, 300, 33), (1, 3, False, 1, 64)])
def test_wrappers_autograd_against_float64_autograd_of_the_torch_composition(L, H, masked, I, Un):
    from mmrec_amd import hip_ops
    d = _wrapper_inputs(I, Un, H, 100 * L + H, masked)
    calls = {"fwd": 0, "bwd": 0}
    lib = _lib()
    real_f, real_b = lib.mmrec_hyper_layer_fwd_f32, lib.mmrec_hyper_layer_bwd_f32
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(lib, "mmrec_hyper_layer_fwd_f32", lambda *a: calls.__setitem__("fwd", calls["fwd"] + 1) or real_f(*a))
        mp.setattr(lib, "mmrec_hyper_layer_bwd_f32", lambda *a: calls.__setitem__("bwd", calls["bwd"] + 1) or real_b(*a))
        got = _wrapper_run(d, L, 0.2, 0.5, torch.float32, "cuda:0", True)
        torch.cuda.synchronize()
    assert calls == {"fwd": L, "bwd": L}, calls                          # the kernels were really taken
    ref = _wrapper_run(d, L, 0.2, 0.5, torch.float64, "cpu", False)
    bounds = wrapper_bounds(d, L, 0.2, 0.5, ref)
    names = ("U_L", "X_L", "d a_i", "d a_u", "d E")
    worst = {n: compare(g, r.numpy(), b, n) for n, g, r, b in zip(names, got, ref, bounds)}
    print("wrappers L %d H %d: worst err / bound %s" % (L, H, " ".join("%s %.3f" % kv for kv in worst.items())))
    assert float(got[2].abs().max()) > 0 and float(got[4].abs().max()) > 0
    # the switch off: the torch composition, bit for bit
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(hip_ops, "HYPER", False)
        off = _wrapper_run(d, L, 0.2, 0.5, torch.float32, "cuda:0", False)
        T = lambda x: None if x is None else _on(x)                       # noqa: E731
        assert not hip_ops.hyper_assign_served(T(d["a_i"]), T(d["g_i"]), T(d["m_i"]))
        P_off = hip_ops.hyper_assign(T(d["a_i"]), T(d["g_i"]), T(d["m_i"]), 0.2, 0.5)
    assert torch.equal(_bits(P_off), _bits(off[5]))


@pytest.mark.gpu
def test_forward_and_backward_replay_from_a_captured_graph():
    """assignment + two layers, forward + backward, captured on one stream and replayed: the eager bits (no host synchronisation,
    no allocation inside the library, no data-dependent launch shape)"""
    from mmrec_amd import hip_ops
    d = _wrapper_inputs(150, 90, 4, 7, True)
    T = lambda x: _on(x)                                                  # noqa: E731
    a_i, a_u, E = T(d["a_i"]).requires_grad_(), T(d["a_u"]).requires_grad_(), T(d["E"]).requires_grad_()
    g_i, g_u, m_i, m_u, w_u, w_x = (T(d[k]) for k in ("g_i", "g_u", "m_i", "m_u", "w_u", "w_x"))

    def step():
        a_i.grad = a_u.grad = E.grad = None
        P_i, P_u = hip_ops.hyper_assign(a_i, g_i, m_i, 0.2, 0.5), hip_ops.hyper_assign(a_u, g_u, m_u, 0.2, 0.5)
        uo, xo = hip_ops.hyper_propagate(P_i, P_u, E, 2)
        ((uo * w_u).sum() + (xo * w_x).sum()).backward()
        return uo.detach(), xo.detach(), a_i.grad, a_u.grad, E.grad
    eager = [t.clone() for t in step()]
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        held = step()
    with torch.no_grad():                                                 # other inputs in the same buffers, then the first ones again
        E.copy_(T(d["E"][::-1].copy())), a_i.copy_(T(d["a_i"][::-1].copy()))
    graph.replay()
    torch.cuda.synchronize()
    other = [t.clone() for t in held]
    with torch.no_grad():
        E.copy_(T(d["E"])), a_i.copy_(T(d["a_i"]))
    graph.replay()
    torch.cuda.synchronize()
    for a, b, o in zip(eager, held, other):
        assert torch.equal(_bits(a), _bits(b))
        assert not torch.equal(_bits(a), _bits(o))                        # the replay really computed
