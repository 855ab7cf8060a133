"""GPU: seeded differential fuzz of LGMRec's hypergraph kernels at 64 hyperedges (csrc/hypergraph64.hip: mmrec_hyper64_assign_fwd_f32
/ _bwd_f32, mmrec_hyper64_layer_fwd_f32 / _bwd_f32; hip_ops.hyper64_assign / hyper64_layer / hyper64_propagate) against float64
numpy of the formulas as tests/test_hyper_fuzz_gpu.py writes them (`assign64`, `assign_bwd64`, `layer64`, `layer_bwd64`, imported),
never against another kernel.  The raw C ABI is called over guarded, sentinel-filled outputs and a sentinel-filled workspace of
exactly the reported size; EVERY CALL is checked against float64 of the fp32 arrays that call was given (the chain of L layers is
checked link by link).

The kernels' plan, read from the library (R = mmrec_hyper64_rows_per_block(n): 64 up to 16,384 rows, then 64 ceil(n / 16,384)): a
reduction over rows is cut into blocks of R rows, each ONE fma chain in row order (R roundings); the finish adds the blocks
quarter, quarter + 4, ... in order and then the four quarters in order (ceil(blocks / 4) + 3).  A term of a reduced sum meets at most
    n_red(n_a, n_b) = max(R_a, R_b) + ceil((blocks_a + blocks_b) / 4) + 3
roundings (the forward reduces the item side alone, dlat both sides).  A row of X', U', dX_prev is one chain of 64 fmas from 0.
dP_u[r][h] is one chain of 64 fmas over dU[r] lat[h].  dP_i[r][h] is ONE chain of 128 fmas from 0 -- the 64 of dX[r] lat[h], then
the 64 of X[r] dlat[h] -- so a term of the first product meets 128 roundings and one of the second 64 besides dlat's own
(counted from hyper64_rows_bwd_kernel: t64_stage_nt on the dX tile, then t64_stage_nt on the X tile onto the same accumulators).

Two acceptance modes, those of tests/test_hyper_fuzz_gpu.py; each case uses one.
  exact  one-hot assignments (one exact 0 per row, the rest <= -200 tau), q a power of two, data on a 1/8 grid sized so that every
         sum stays below 2^24 quanta (`exact_grid_ok`, asserted without a GPU): every output must EQUAL the closed forms written
         with np.add.at, d a must be exactly 0.  Hyperedge 0 holds only the rows on tile and block boundaries, hyperedge 63 none.
  float  first-order bounds, u = 2^-24, gamma(n) = n u / (1 - n u), times 1 + 2^-10:
           assignment and its backward: the bounds of tests/test_hyper_fuzz_gpu.py with H = 64 (they do not depend on the order of
                        the row's sum; the kernel's 7 additions of the sum and 8 roundings of the dot product are below the
                        gamma(64) and gamma(66) those bounds grant)
           lat          gamma(n_red(I)) |P_i|^T |X|
           X', U'       gamma(n_red(I) + 64) |P| (|P_i|^T |X|)
           dX_prev      gamma(n_red(I, U) + 64) |P_i| MAG_dlat,   MAG_dlat = |P_i|^T |dX| + |P_u|^T |dU|
           dP_u         gamma(64) |dU| |lat|^T
           dP_i         gamma(128) |dX| |lat|^T + gamma(64 + n_red(I, U)) |X| MAG_dlat^T
         each plus n 2^-149 for results below the normal range (n the count inside gamma).
The worst err / bound per family is printed by every case and recorded in EXPERIMENTS.md section 4.
`test_cases_span_every_axis` and `test_exact_cases_are_on_the_grid` need no GPU; the checker's own tests (an fp32 emulation of the
plan passes, planted errors do not) are in tests/test_hyper64_cpu.py."""
import numpy as np
import pytest
import torch

import tests.test_hyper_fuzz_gpu as Z
from tests.test_edge_softmax_fuzz_gpu import E_EXP, GUARD, SENTINEL   # noqa: F401  (E_EXP: inside Z.assign_bound)
from tests.test_spmm_fuzz_gpu import U, _on, gamma                    # noqa: F401

D = H = 64
CASES = 32
BIG = 16385                                    # just past where R grows from 64: R = 128, 129 blocks (129 = 1 mod 4)
MID = 6521                                     # 102 blocks of 64 rows (102 = 2 mod 4); with BIG's 129: 231 = 3 mod 4
FINISH_STRIDE = 4
MAX_BLOCKS = 256                               # blocks of a side: the cap of csrc/tile64.h's fuser plan
SLACK, TINY = Z.SLACK, Z.TINY
f64 = Z.f64


def _lib():
    return Z._lib()


def rows_per_block(n):
    return int(_lib().mmrec_hyper64_rows_per_block(int(n)))


def blocks(n):
    return -(-n // rows_per_block(n)) if n > 0 else 0


def n_red(n_a, n_b=0):
    """the roundings a term of a reduction over the rows of one side (forward) or of both (dlat) meets"""
    r = max(rows_per_block(n_a) if n_a else 0, rows_per_block(n_b) if n_b else 0)
    return r + -(-(blocks(n_a) + blocks(n_b)) // FINISH_STRIDE) + 3


def axis_n():
    r = rows_per_block(1)
    return tuple(sorted({0, 1, 2, 15, 16, 17, 63, 64, 65, r - 1, r, r + 1, 2 * r + 1}))


def boundary_rows(n):
    r = rows_per_block(max(n, 1))
    want = {0, n - 1, n - 2, 15, 16, 63, 64, 65, 127, 128, r - 1, r, 2 * r - 1, 2 * r, (n // r) * r - 1, (n // r) * r,
            (n // 64) * 64 - 1, (n // 64) * 64}
    return np.array(sorted(x for x in want if 0 <= x < n), np.int64)


def _side(c, rng, n):
    """one side's logits, noise, mask, hot index (exact) and the gradient dP its backward is given"""
    s = Z.Case()
    s.n = n
    if c.exact:
        hot = rng.integers(1, H - 1, n)                                   # hyperedge 63 holds no row
        hot[boundary_rows(n)] = 0                                         # hyperedge 0: the rows on tile and block boundaries only
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
        m = (rng.random((n, H)) < c.q).astype(np.float32)
        if n > 2:
            m[rng.integers(0, n, max(1, n // 16))] = 0.0                  # rows whose mask is all zero
        s.m = m
    return s


def case(k):
    ns = axis_n()
    c = Z.Case()
    c.k, c.H = k, H
    c.I, c.U = ns[k % len(ns)], ns[(3 * k + k // len(ns) + 5) % len(ns)]
    c.L = 1 + (k // 8) % 2
    c.masked = (k // 3) % 2 == 0
    c.tau = (0.2, 1.0)[(k // 5) % 2]
    c.exact = (k + k // 4) % 2 == 0
    c.q = (0.5, 0.25)[(k // 7) % 2] if c.exact else (0.5, 0.25, 0.2)[(k // 7) % 3]      # 1 / 0.2 is inexact: float mode only
    if k == 5:
        c.I, c.U = BIG, 2 * rows_per_block(1) + 1                         # the large table in both modes
    if k == 12:
        c.I, c.U = BIG, MID
    if c.exact and c.L == 2 and max(c.I, c.U) > 65:
        c.L = 1                                                           # two exact layers stay on the grid up to 65 rows
    c.amp = 2
    if c.exact and (c.L == 2 or max(c.I, c.U) > 1000):
        c.q, c.amp = 0.5, 1
    c.in_null, c.out_null = k % 4, (k // 4) % 8                           # bit 0: dU NULL, bit 1: dX NULL; bits: dP_i, dP_u, dX_prev NULL
    rng = np.random.default_rng(6400 + k)
    c.i, c.u = _side(c, rng, c.I), _side(c, rng, c.U)
    if c.exact:
        E, dU, dX = (rng.integers(-c.amp, c.amp + 1, (n, D)) / 8.0 for n in (c.I, c.U, c.I))
    else:
        E, dU, dX = rng.standard_normal((c.I, D)) * 0.3, rng.standard_normal((c.U, D)), rng.standard_normal((c.I, D))
    c.E, c.dU, c.dX = (np.ascontiguousarray(x, np.float32) for x in (E, dU, dX))
    return c


name_of = Z.name_of


# ------------------------------------------------------------------------------------------------ the float mode's layer bounds
def layer_bounds(P_i, P_u, X):
    """-> {name: (ref, bound)} for lat, X_out, U_out"""
    lat, xo, uo = Z.layer64(P_i, P_u, X)
    n = n_red(np.asarray(P_i).shape[0])
    mag = np.abs(f64(P_i)).T @ np.abs(f64(X))
    out = {"lat": (lat, SLACK * gamma(n) * mag + n * TINY),
           "X_out": (xo, SLACK * gamma(n + H) * (np.abs(f64(P_i)) @ mag) + (n + H) * TINY)}
    if P_u is not None:
        out["U_out"] = (uo, SLACK * gamma(n + H) * (np.abs(f64(P_u)) @ mag) + (n + H) * TINY)
    return out


def layer_bwd_bounds(P_i, P_u, X, lat, dU, dX):
    """-> {name: (ref, bound)} for dP_i, dP_u, dX_prev"""
    dpi, dpu, dxp, _ = Z.layer_bwd64(P_i, P_u, X, lat, dU, dX)
    I, Un = np.asarray(P_i).shape[0], np.asarray(P_u).shape[0]
    n = n_red(I if dX is not None else 0, Un if dU is not None else 0)
    aU = np.zeros((Un, D)) if dU is None else np.abs(f64(dU))
    aX = np.zeros((I, D)) if dX is None else np.abs(f64(dX))
    mag = np.abs(f64(P_i)).T @ aX + np.abs(f64(P_u)).T @ aU
    al = np.abs(f64(lat))
    return {"dP_i": (dpi, SLACK * (gamma(2 * D) * (aX @ al.T) + gamma(D + n) * (np.abs(f64(X)) @ mag.T)) + (2 * D + n) * TINY),
            "dP_u": (dpu, SLACK * gamma(D) * (aU @ al.T) + D * TINY),
            "dX_prev": (dxp, SLACK * gamma(n + H) * (np.abs(f64(P_i)) @ mag) + (n + H) * TINY)}


def check_layer(c, P_i, P_u, X, got, closed, name):
    """got: {name: array}; closed: (lat, X_out, U_out) of the exact mode"""
    if c.exact:
        refs = dict(zip(("lat", "X_out", "U_out"), closed))
        return max([Z.compare(v, refs[k], None, name + " " + k) for k, v in got.items()] + [0.0])
    bounds = layer_bounds(P_i, P_u if "U_out" in got else None, X)
    return max([Z.compare(v, *bounds[k], name + " " + k) for k, v in got.items()] + [0.0])


def check_layer_bwd(c, P_i, P_u, X, lat, dU, dX, got, closed, name):
    if c.exact:
        refs = dict(zip(("dP_i", "dP_u", "dX_prev"), closed))
        return max([Z.compare(v, refs[k], None, name + " " + k) for k, v in got.items()] + [0.0])
    bounds = layer_bwd_bounds(P_i, P_u, X, lat, dU, dX)
    return max([Z.compare(v, *bounds[k], name + " " + k) for k, v in got.items()] + [0.0])


# ------------------------------------------------------------------------------------------------ no GPU: the axes, the grid
def test_cases_span_every_axis():
    cs = [case(k) for k in range(CASES)]
    ns = axis_n()
    r = rows_per_block(1)
    assert r == 64 and rows_per_block(BIG - 1) == 64 and rows_per_block(BIG) == 128          # BIG: just past where R grows
    assert {0, 1, 2, 15, 16, 17, 63, 64, 65, r - 1, r, r + 1, 2 * r + 1} == set(ns)
    assert set(ns) <= {c.I for c in cs} and set(ns) <= {c.U for c in cs}
    assert blocks(BIG) % FINISH_STRIDE and blocks(MID) % FINISH_STRIDE and (blocks(BIG) + blocks(MID)) % FINISH_STRIDE
    for mode in (True, False):
        m = [c for c in cs if c.exact == mode]
        assert {c.L for c in m} == {1, 2} and {c.masked for c in m} == {True, False}, mode
        assert {c.tau for c in m} == {0.2, 1.0} and {0.5, 0.25} <= {c.q for c in m if c.masked}, mode
        assert {c.in_null for c in m} == set(range(4)) and {c.out_null for c in m} == set(range(8)), mode
        assert len([c for c in m if c.I == BIG]) == 1, mode                # the large table in both modes
    assert any(c.U == MID and c.I == BIG and not c.in_null for c in cs)    # dlat over 231 blocks of both plans
    assert all(c.q in (0.5, 0.25) for c in cs if c.exact) and any(c.q == 0.2 and c.masked for c in cs if not c.exact)
    assert {c.q for c in cs} == {0.5, 0.25, 0.2}
    assert {(c.in_null, c.out_null) for c in cs} == {(a, b) for a in range(4) for b in range(8)}      # every NULL combination
    for L in (1, 2):
        assert {c.in_null for c in cs if c.L == L} == set(range(4))       # (L = 2: the inner layers ask for no user rows)
    wide = [float((Z._x64(s.a, s.g, c.tau).max(axis=1) - Z._x64(s.a, s.g, c.tau).min(axis=1)).max())
            for c in cs if not c.exact for s in (c.i, c.u) if s.n > 8]
    assert max(wide) > 200.0 and sum(w > 200.0 for w in wide) > len(wide) // 2      # finite only with the maximum subtracted
    for c in cs:
        if not c.exact:
            continue
        for s in (c.i, c.u):
            x = (s.a.astype(np.float32) + s.g.astype(np.float32)).astype(np.float64)                  # the kernel's own sum
            assert np.array_equal(x[np.arange(s.n), s.hot], np.zeros(s.n))
            if s.n:
                assert float(x[~np.eye(H, dtype=bool)[s.hot]].max()) <= -200.0 * c.tau
                assert not (s.hot == H - 1).any()                         # a hyperedge with no rows
                assert set(np.flatnonzero(s.hot == 0)) == set(boundary_rows(s.n))
            if s.m is not None and s.n > 2:
                assert (s.m.sum(axis=1) == 0).any() and (s.m[np.arange(s.n), s.hot] == 0).any()       # dropped rows
            P, p = Z.assign64(s.a, s.g, s.m, c.tau, c.q)
            assert np.array_equal(P.astype(np.float32).astype(np.float64), Z.closed_P(c, s))          # the construction IS the formula
    e = next(c for c in cs if c.exact and c.I == BIG)
    assert {63, 64, 127, 128, BIG - 1} <= set(np.flatnonzero(e.i.hot == 0))


def test_exact_cases_are_on_the_grid():
    for k in range(CASES):
        c = case(k)
        if c.exact:
            assert Z.exact_grid_ok(c), name_of(c)
            for t in (c.E, c.dU, c.dX):
                assert np.array_equal(t * 8, np.round(t * 8)) and float(np.abs(t).max(initial=0)) <= 0.25
            fwd, bwd = Z.exact_chain(c)                                   # the closed forms ARE the formulas (float64 is exact here)
            P_i, P_u = Z.closed_P(c, c.i), Z.closed_P(c, c.u)
            for (Xp, lat, xo, uo) in fwd:
                r_lat, r_x, r_u = Z.layer64(P_i, P_u, Xp)
                assert np.array_equal(lat, r_lat) and np.array_equal(xo, r_x) and (uo is None or np.array_equal(uo, r_u))
            for (dpi, dpu, dxp, dU, dX, dlat), (Xp, lat, _, _) in zip(bwd, reversed(fwd)):
                r = Z.layer_bwd64(P_i, P_u, Xp, lat, dU, dX)
                assert all(np.array_equal(a, b) for a, b in zip((dpi, dpu, dxp, dlat), r))


# ------------------------------------------------------------------------------------------------ GPU: the raw C ABI, guarded
def _workspace(I, Un):
    nbytes = int(_lib().mmrec_hyper64_workspace_bytes(I, Un))
    assert nbytes > 0 and nbytes % 16 == 0
    return torch.full((nbytes // 4 + GUARD,), SENTINEL, dtype=torch.int32, device="cuda:0"), nbytes // 4


def raw_assign(c, s, name):
    from mmrec_amd import hip_ops
    p_, lib = hip_ops._p, _lib()
    a, g, m = _on(s.a), _on(s.g), (None if s.m is None else _on(s.m))
    shapes = {"P": (s.n, H), "p": (s.n, H) if s.m is not None else None}
    held, ptr = Z._outs(shapes)
    rc = lib.mmrec_hyper64_assign_fwd_f32(p_(a), p_(g), p_(m), s.n, c.tau, c.q, ptr["P"], ptr["p"], hip_ops._stream())
    assert rc == 0, (name, rc)
    out = Z._collect(held, shapes, name)
    return out["P"], out.get("p")


def raw_assign_bwd(c, s, p_in, dP, name):
    from mmrec_amd import hip_ops
    p_, lib = hip_ops._p, _lib()
    m = None if s.m is None else _on(s.m)
    shapes = {"da": (s.n, H)}
    held, ptr = Z._outs(shapes)
    rc = lib.mmrec_hyper64_assign_bwd_f32(p_(p_in), p_(m), p_(dP), s.n, c.tau, c.q, ptr["da"], hip_ops._stream())
    assert rc == 0, (name, rc)
    return Z._collect(held, shapes, name)["da"]


def raw_layer(I, Un, P_i, P_u, X, want_u, name):
    from mmrec_amd import hip_ops
    p_, lib = hip_ops._p, _lib()
    shapes = {"lat": (H, D), "X_out": (I, D), "U_out": (Un, D) if want_u else None}
    held, ptr = Z._outs(shapes)
    ws, n_ws = _workspace(I, Un)
    rc = lib.mmrec_hyper64_layer_fwd_f32(p_(P_i), p_(P_u) if want_u else None, p_(X), I, Un, ptr["U_out"], ptr["X_out"], ptr["lat"],
                                         p_(ws), hip_ops._stream())
    assert rc == 0, (name, rc)
    out = Z._collect(held, shapes, name)
    Z._workspace_ok(ws, n_ws, name)
    return out


def raw_layer_bwd(I, Un, P_i, P_u, X, lat, dU, dX, out_null, name):
    from mmrec_amd import hip_ops
    p_, lib = hip_ops._p, _lib()
    shapes = {"dP_i": None if out_null & 1 else (I, H), "dP_u": None if out_null & 2 else (Un, H),
              "dX_prev": None if out_null & 4 else (I, D)}
    held, ptr = Z._outs(shapes)
    ws, n_ws = _workspace(I, Un)
    rc = lib.mmrec_hyper64_layer_bwd_f32(p_(P_i), p_(P_u), p_(X), p_(lat), p_(dU), p_(dX), I, Un, ptr["dP_i"], ptr["dP_u"],
                                         ptr["dX_prev"], p_(ws), hip_ops._stream())
    assert rc == 0, (name, rc)
    out = Z._collect(held, shapes, name)
    Z._workspace_ok(ws, n_ws, name)
    return out


def run_case(c, check=True):
    """every call of the case through the raw ABI -> (all outputs in call order, worst err / bound per family)"""
    name = name_of(c)
    outs, worst = [], {"assign": 0.0, "assign_bwd": 0.0, "layer": 0.0, "layer_bwd": 0.0}
    Ps = []
    for tag, s in (("i", c.i), ("u", c.u)):
        P, p = raw_assign(c, s, name + " assign " + tag)
        p_in = P if p is None else p
        da = raw_assign_bwd(c, s, p_in, _on(s.dP), name + " assign bwd " + tag)
        outs += [P, da] + ([] if p is None else [p])
        Ps.append(P)
        if check:
            worst["assign"] = max(worst["assign"], Z.check_assign(c, s, P, p, name + " " + tag))
            worst["assign_bwd"] = max(worst["assign_bwd"], Z.check_assign_bwd(c, s, p_in.cpu().numpy(), da, name + " " + tag))
    P_i, P_u = Ps
    closed_f, closed_b = Z.exact_chain(c) if (c.exact and check) else (None, None)
    X, kept = _on(c.E), []
    for l in range(c.L):
        want_u = l == c.L - 1
        got = raw_layer(c.I, c.U, P_i, P_u, X, want_u, name + " layer %d" % l)
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
        got = raw_layer_bwd(c.I, c.U, P_i, P_u, Xp, lat, dU, dX, out_null, name + " layer bwd %d" % l)
        outs += list(got.values())
        if check:
            n = lambda t: None if t is None else t.cpu().numpy()          # noqa: E731
            worst["layer_bwd"] = max(worst["layer_bwd"], check_layer_bwd(
                c, n(P_i), n(P_u), n(Xp), n(lat), n(dU), n(dX), got, closed_b[j][:3] if c.exact else None, name + " layer bwd %d" % l))
        dU, dX = None, got.get("dX_prev")
    return outs, worst


def _bits(t):
    return t.contiguous().view(torch.int32)


@pytest.mark.gpu
@pytest.mark.parametrize("k", range(CASES))
def test_hyper64_fuzz(k):
    c = case(k)
    outs, worst = run_case(c)
    print("%s: worst err / bound %s" % (name_of(c), " ".join("%s %.3f" % kv for kv in sorted(worst.items()))))
    again, _ = run_case(c, check=False)                                   # the same calls again: the same bits, both directions
    assert len(outs) == len(again) and all(torch.equal(_bits(a), _bits(b)) for a, b in zip(outs, again)), name_of(c)


@pytest.mark.gpu
@pytest.mark.parametrize("L,masked,I,Un", [(1, True, 129, 70), (2, True, 65, 200), (2, False, 300, 33)])
def test_wrappers_through_autograd_equal_the_chained_raw_calls_bit_for_bit(L, masked, I, Un):
    """hyper64_assign + hyper64_propagate, loss = <U_L, w_u> + <X_L, w_x>: the kernels are really taken (counted), and every result
    and gradient has the bits of the raw calls chained by hand (the inner layers without user rows, the two uses of P_i added)"""
    from mmrec_amd import hip_ops
    lib = _lib()
    d = Z._wrapper_inputs(I, Un, H, 640 + L, masked)
    c = Z.Case()
    c.tau, c.q = 0.2, 0.2
    T = lambda x: None if x is None else _on(x)                           # noqa: E731
    a_i, a_u, E = T(d["a_i"]).requires_grad_(), T(d["a_u"]).requires_grad_(), T(d["E"]).requires_grad_()
    calls = []
    with pytest.MonkeyPatch.context() as mp:
        for fn in ("mmrec_hyper64_assign_fwd_f32", "mmrec_hyper64_assign_bwd_f32", "mmrec_hyper64_layer_fwd_f32",
                   "mmrec_hyper64_layer_bwd_f32"):
            mp.setattr(lib, fn, lambda *a, _real=getattr(lib, fn), _fn=fn: calls.append(_fn[14:-4]) or _real(*a))
        assert hip_ops.hyper64_assign_served(a_i, T(d["g_i"]), T(d["m_i"]))
        P_i = hip_ops.hyper64_assign(a_i, T(d["g_i"]), T(d["m_i"]), c.tau, c.q)
        P_u = hip_ops.hyper64_assign(a_u, T(d["g_u"]), T(d["m_u"]), c.tau, c.q)
        assert hip_ops.hyper64_layer_served(P_i, P_u, E)
        uo, xo = hip_ops.hyper64_propagate(P_i, P_u, E, L)
        P_i.retain_grad(), P_u.retain_grad()
        ((uo * T(d["w_u"])).sum() + (xo * T(d["w_x"])).sum()).backward()
        torch.cuda.synchronize()
    assert sorted(calls) == sorted(["assign_fwd"] * 2 + ["assign_bwd"] * 2 + ["layer_fwd"] * L + ["layer_bwd"] * L), calls
    sides = []
    for n, a, g, m in ((I, "a_i", "g_i", "m_i"), (Un, "a_u", "g_u", "m_u")):
        s = Z.Case()
        s.n, s.a, s.g, s.m = n, d[a], d[g], d[m]
        sides.append((s,) + raw_assign(c, s, "raw assign " + a))
    rP_i, rP_u = sides[0][1], sides[1][1]
    X, kept = T(d["E"]), []
    for l in range(L):
        got = raw_layer(I, Un, rP_i, rP_u, X, l == L - 1, "raw layer %d" % l)
        kept.append((X, got["lat"]))
        X, rU = got["X_out"], got.get("U_out")
    dU, dX, dP_i = T(d["w_u"]), T(d["w_x"]), None
    for l in reversed(range(L)):
        Xp, lat = kept[l]
        g = raw_layer_bwd(I, Un, rP_i, rP_u, Xp, lat, dU, dX, 0 if l == L - 1 else 2, "raw layer bwd %d" % l)
        dP_i = g["dP_i"] if dP_i is None else dP_i + g["dP_i"]
        if l == L - 1:
            dP_u = g["dP_u"]
        dU, dX = None, g["dX_prev"]
    da = [raw_assign_bwd(c, s, P if p is None else p, dP, "raw assign bwd") for (s, P, p), dP in zip(sides, (dP_i, dP_u))]
    for name, a, b in (("P_i", P_i, rP_i), ("P_u", P_u, rP_u), ("U_L", uo, rU), ("X_L", xo, X),
                       ("dP_i", P_i.grad, dP_i), ("dP_u", P_u.grad, dP_u), ("dE", E.grad, dX), ("da_i", a_i.grad, da[0]),
                       ("da_u", a_u.grad, da[1])):
        assert torch.equal(_bits(a.detach()), _bits(b)), name
    assert float(a_i.grad.abs().max()) > 0 and float(E.grad.abs().max()) > 0



@pytest.mark.gpu
def test_forward_and_backward_replay_from_a_captured_graph():
    """assignment + two layers, forward + backward, captured on one stream and replayed: the eager bits (no host synchronisation,
    no allocation inside the library, no data-dependent launch shape)"""
    from mmrec_amd import hip_ops
    d = Z._wrapper_inputs(150, 90, H, 64, True)
    a_i, a_u, E = _on(d["a_i"]).requires_grad_(), _on(d["a_u"]).requires_grad_(), _on(d["E"]).requires_grad_()
    g_i, g_u, m_i, m_u, w_u, w_x = (_on(d[k]) for k in ("g_i", "g_u", "m_i", "m_u", "w_u", "w_x"))

    def step():
        a_i.grad = a_u.grad = E.grad = None
        P_i, P_u = hip_ops.hyper64_assign(a_i, g_i, m_i, 0.2, 0.5), hip_ops.hyper64_assign(a_u, g_u, m_u, 0.2, 0.5)
        uo, xo = hip_ops.hyper64_propagate(P_i, P_u, E, 2)
        ((uo * w_u).sum() + (xo * w_x).sum()).backward()
        return uo.detach(), xo.detach(), a_i.grad, a_u.grad, E.grad
    assert hip_ops.hyper64_assign_served(a_i, g_i, m_i)
    eager = [t.clone() for t in step()]
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        held = step()
    with torch.no_grad():                                                 # other inputs in the same buffers, then the first ones again
        E.copy_(_on(d["E"][::-1].copy())), a_i.copy_(_on(d["a_i"][::-1].copy()))
    graph.replay()
    torch.cuda.synchronize()
    other = [t.clone() for t in held]
    with torch.no_grad():
        E.copy_(_on(d["E"])), a_i.copy_(_on(d["a_i"]))
    graph.replay()
    torch.cuda.synchronize()
    for a, b, o in zip(eager, held, other):
        assert torch.equal(_bits(a), _bits(b))
        assert not torch.equal(_bits(a), _bits(o))                        # the replay really computed
