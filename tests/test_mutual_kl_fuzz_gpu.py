"""GPU: seeded differential fuzz of DAMRS's symmetric KL kernels (csrc/mutual_kl.hip, mmrec_mutual_kl_f32 / _bwd_f32,
hip_ops.mutual_kl) against float64 numpy of the formulas as written here (`ref64`), never against another kernel.  The raw C ABI
is called over guarded, sentinel-filled outputs and a sentinel-filled workspace.

    a = <U[r], A[i]>, b = <U[r], B[i]>, p = sigmoid(a), q = sigmoid(b),  J = (p - q)(a - b)  (= KL(p || q) + KL(q || p))
    out = scale sum_ri J;   ga = g scale [s'(a)(a - b) + (p - q)],  gb = -g scale [s'(b)(a - b) + (p - q)],  s'(x) = p (1 - p)
    dU = Ga A + Gb B,  dA = Ga^T U,  dB = Gb^T U

The kernels' plan (read from the library: `split_len`).  A logit is an fma chain over k = 0 .. 63 on the fp32 MFMA.  Forward: a
lane adds the J of its pairs in the order it meets them, 16 per 32-row sub-tile of its split; the 64 lanes of a wave by a
butterfly, the four waves in order, one partial per workgroup; one workgroup adds the partials (thread t the partials t, t + 256,
..., the butterfly, the four waves) and multiplies by scale.  Backward: the coefficients per pair, the products as fma chains
over the walked side in order within a split, the splits added in order.

Two modes; each case uses one.
  sparse  entries are multiples of 1/8 (every logit exact) and B == A bit for bit except at a few TARGET item rows: the first and
          last rows and the rows around the sub-tile, tile and split boundaries.  Off target a == b in the same bits, so J and both
          coefficients are exactly 0: every off-target row of dA and dB must EQUAL 0 and the sum must match float64 of the target
          pairs alone within the float bound.  A lost or doubled column cannot hide.
  float   rows of A and B normalised, |U[r]| from 0.05 to 8; the kind "tie" has B = A + 1e-3 noise (J of order 1e-7 a pair, all
          cancellation).  Bounds are absolute and first order, u = 2^-24:
            da = gamma(64) sum_k |U_rk A_ik|, db likewise                                      the chains
            e_pa = s'(a) da + E_SIG u                                                          the sigmoid: its argument, itself
                   E_SIG = E_EXP + 2: the device's exp (tests/test_edge_softmax_fuzz_gpu.py), the addition 1 + e and the
                   division; confirmed as 4 x the worst error of fp32 sigmoid against float64 measured on the CPU over these
                   cases' own logits (`test_E_SIG_covers_these_cases`)
            T = |a - b| (e_pa + e_pb + u |p - q|) + |p - q| (da + db + u |a - b|) + u |J|      a pair's J
            |out - ref| <= scale (sum T + gamma(n_acc) sum |J|) + 2 u |ref|                    n_acc: the additions a term meets,
                   16 (split_len / 32) + 10 in its workgroup, ceil(P / 256) + 10 in the finish, P partials
            e_ga = |g scale| [|a - b| (|1 - 2 p| e_pa + 2 u) + s'(a) (da + db + u |a - b|) + e_pa + e_pb
                              + 4 u (|s'(a) (a - b)| + |p - q|)],  e_gb likewise with b, q
            |dU - ref|_rc <= sum_i (e_ga |A_ic| + e_gb |B_ic|) + gamma(n_u) sum_i (|ga A_ic| + |gb B_ic|) + n_u 2^-149
                   n_u = 2 split_len_1 + n_splits_1;  dA, dB the same over r with n_a = split_len_2 + n_splits_2
`test_E_SIG_covers_these_cases`, `test_cases_span_every_axis` and `test_a_dropped_column_exceeds_the_bound_tenfold` need no GPU;
the checker's own tests (an fp32 emulation of the plan passes, planted errors do not) are in tests/test_mutual_kl_cpu.py."""
import functools
import gc
import os

import numpy as np
import pytest
import torch

from tests.test_edge_softmax_fuzz_gpu import E_EXP, GUARD, SENTINEL
from tests.test_spmm_fuzz_gpu import U, gamma

E_SIG = E_EXP + 2.0                            # test_E_SIG_covers_these_cases
D = 64
MS = (1, 31, 32, 33, 127, 128, 129, 257)
NS_FIXED = (1, 31, 32, 33, 63, 64, 65, 129, 4097)
KINDS = ("sparse", "float", "tie")
CASES = 40


def _lib():
    from mmrec_amd import _lib as L
    if not os.path.exists(L.LIB_PATH):
        from mmrec_amd.build import build
        build(verbose=False)
    return L.load()


def split_len(m, n, mode=0):
    """rows of the walked side per split, from the library (mode 0 forward, 1 dU sweep, 2 dA / dB sweep)"""
    return int(_lib().mmrec_mutual_kl_split_cols(int(m), int(n), int(mode)))


@functools.lru_cache(maxsize=None)
def n_split():
    """the smallest n below 4,097 at which the dU sweep over 257 rows has three or more splits, each of more than one tile, and
    a LAST SPLIT OF ONE COLUMN (the forward's one-tile splits then end in one column too)"""
    for n in range(130, 4097):
        s = split_len(257, n, 1)
        if s > 64 and n % s == 1 and n // s >= 2:
            return n
    raise AssertionError("no n with a last split of one column")


def axis_n():
    return NS_FIXED + (n_split(),)


class Case:
    pass


@functools.lru_cache(maxsize=None)
def case(k):
    ns = axis_n()
    c = Case()
    c.seed, c.m, c.n = k, MS[k % 8], ns[(3 * k + k // 8) % len(ns)]
    c.kind = KINDS[(k + k // 6) % 3]
    if k in (7, 15, 23, 31):                    # the large shapes in both modes, on more than two row tiles
        c.m, c.n, c.kind = 257, (4097, n_split())[k in (23, 31)], ("sparse", "float")[k in (15, 31)]
    c.sparse = c.kind == "sparse"
    rng = np.random.default_rng(4000 + k)
    m, n = c.m, c.n
    c.scale = float(np.float32(1.0 / (float(m) * float(n))))
    if c.sparse:
        s0, s1 = split_len(m, n, 0), split_len(m, n, 1)
        want = [0, n - 1, 31, 32, 33, 63, 64, 65, s0 - 1, s0, s0 + 1, s1 - 1, s1, s1 + 1, n - 2, n // 2, 95, 96]
        c.targets = sorted({t for t in want if 0 <= t < n})
        Um = rng.integers(-8, 9, (m, D)) / 8.0
        A = rng.integers(-4, 5, (n, D)) / 8.0
        B = A.copy()
        B[c.targets] = rng.integers(-4, 5, (len(c.targets), D)) / 8.0
        c.g = float(rng.choice([1.0, -0.5, 2.25]))
    else:
        unit = lambda x: x / np.maximum(np.linalg.norm(x, axis=1, keepdims=True), 1e-12)      # noqa: E731
        Um = unit(rng.standard_normal((m, D))) * np.exp(rng.uniform(np.log(0.05), np.log(8.0), (m, 1)))
        A = unit(rng.standard_normal((n, D)))
        B = A + 1e-3 * rng.standard_normal((n, D)) if c.kind == "tie" else unit(rng.standard_normal((n, D)))
        c.targets = None
        c.g = float(rng.choice([1.0, 0.37, -1.6]))
    c.U, c.A, c.B = (np.ascontiguousarray(x, np.float32) for x in (Um, A, B))
    return c


def float_cases():
    return [c for c in map(case, range(CASES)) if not c.sparse]


# ------------------------------------------------------------------------------------------------ host references
def sigmoid64(x):
    e = np.exp(-np.abs(x))
    return np.where(x >= 0, 1.0, e) / (1.0 + e)


class Ref:
    pass


def ref64(c):
    """float64 of the formulas on the fp32 arrays of the case -> Ref(a, b, p, q, J, out, ga, gb, dU, dA, dB)"""
    r = Ref()
    U64, A64, B64 = c.U.astype(np.float64), c.A.astype(np.float64), c.B.astype(np.float64)
    with np.errstate(invalid="ignore"):
        r.a, r.b = U64 @ A64.T, U64 @ B64.T
        r.p, r.q = sigmoid64(r.a), sigmoid64(r.b)
        r.J = (r.p - r.q) * (r.a - r.b)
        s = float(c.scale)
        r.out = s * r.J.sum()
        gs = float(np.float32(c.g)) * s
        r.ga = gs * (r.p * (1 - r.p) * (r.a - r.b) + (r.p - r.q))
        r.gb = -gs * (r.q * (1 - r.q) * (r.a - r.b) + (r.p - r.q))
        r.dU, r.dA, r.dB = r.ga @ A64 + r.gb @ B64, r.ga.T @ U64, r.gb.T @ U64
    return r


def bounds_of(c):
    """-> (Ref, forward bound, dU bound, dA bound, dB bound) of the module docstring"""
    r = ref64(c)
    m, n = c.m, c.n
    aU, aA, aB = (np.abs(x.astype(np.float64)) for x in (c.U, c.A, c.B))
    da, db = gamma(D) * (aU @ aA.T), gamma(D) * (aU @ aB.T)
    spa, spb = r.p * (1 - r.p), r.q * (1 - r.q)
    e_pa, e_pb = spa * da + E_SIG * U, spb * db + E_SIG * U
    d, pq = np.abs(r.a - r.b), np.abs(r.p - r.q)
    T = d * (e_pa + e_pb + U * pq) + pq * (da + db + U * d) + U * np.abs(r.J)
    s0 = split_len(m, n, 0)
    parts = -(-m // 128) * -(-n // s0)
    n_acc = 16 * (s0 // 32) + 10 + -(-parts // 256) + 10
    s = float(c.scale)
    fwd = s * (T.sum() + gamma(n_acc) * np.abs(r.J).sum()) + 2 * U * abs(r.out)
    gs = abs(float(np.float32(c.g)) * s)
    common = e_pa + e_pb + 4 * U * pq
    e_ga = gs * (d * (np.abs(1 - 2 * r.p) * e_pa + 2 * U) + spa * (da + db + U * d) + common + 4 * U * spa * d)
    e_gb = gs * (d * (np.abs(1 - 2 * r.q) * e_pb + 2 * U) + spb * (da + db + U * d) + common + 4 * U * spb * d)
    s1, s2 = split_len(m, n, 1), split_len(m, n, 2)
    n_u, n_a = 2 * s1 + -(-n // s1), s2 + -(-m // s2)
    aga, agb = np.abs(r.ga), np.abs(r.gb)
    bU = e_ga @ aA + e_gb @ aB + gamma(n_u) * (aga @ aA + agb @ aB) + n_u * 2.0 ** -149
    bA = e_ga.T @ aU + gamma(n_a) * (aga.T @ aU) + n_a * 2.0 ** -149
    bB = e_gb.T @ aU + gamma(n_a) * (agb.T @ aU) + n_a * 2.0 ** -149
    return r, fwd, bU, bA, bB


def _arr(got):
    return got.detach().cpu().double().numpy() if isinstance(got, torch.Tensor) else np.asarray(got, np.float64)


def _compare(got, ref, bound, name):
    g = _arr(got)
    assert g.shape == np.shape(ref), (name, g.shape, np.shape(ref))
    assert np.isfinite(ref).all() and np.isfinite(g).all(), (name, "not finite", int((~np.isfinite(g)).sum()))
    err = np.abs(g - ref)
    viol = err > bound
    assert not viol.any(), (name, "beyond the bound", int(viol.sum()), "first at", np.argwhere(viol)[0].tolist(),
                            float(g[viol][0]), float(np.asarray(ref)[viol][0]), float(np.broadcast_to(bound, g.shape)[viol][0]))
    return float((err / np.maximum(bound, 1e-300)).max(initial=0.0))


def check_fwd(got, c, name="", bd=None):
    """the scalar against float64 within the forward bound; returns err / bound"""
    r, fwd = (bd or bounds_of(c))[:2]
    return _compare(np.reshape(_arr(got), ()), np.float64(r.out), np.float64(fwd), name + " out")


def check_bwd(dU, dA, dB, c, name="", bd=None):
    """the three gradients within their bounds; sparse: every off-target row of dA and dB EQUALS 0"""
    r, _, bU, bA, bB = bd or bounds_of(c)
    if c.sparse:
        off = np.ones(c.n, bool)
        off[c.targets] = False
        for nm, t in (("dA", dA), ("dB", dB)):
            rows = _arr(t)[off]
            assert not rows.any(), (name, nm, "an off-target row is not zero", int(np.count_nonzero(rows.any(axis=1))))
    return max(_compare(dU, r.dU, bU, name + " dU"), _compare(dA, r.dA, bA, name + " dA"), _compare(dB, r.dB, bB, name + " dB"))


# ------------------------------------------------------------------------------------------------ no GPU: the constant, the axes
def sigmoid32(x):
    """the kernels' sigmoid in fp32 numpy: e = exp(-|z|), (z >= 0 ? 1 : e) / (1 + e), one rounding each"""
    x = np.asarray(x, np.float32)
    e = np.exp(-np.abs(x))
    return (np.where(x >= 0, np.float32(1), e) / (np.float32(1) + e)).astype(np.float32)


def test_E_SIG_covers_these_cases():
    """worst error of the fp32 sigmoid (numpy, on the CPU) against float64 in units of u, over the logits of every float case"""
    worst = 0.0
    for c in float_cases():
        r = ref64(c)
        for x in (r.a, r.b):
            x32 = x.astype(np.float32)
            worst = max(worst, float((np.abs(sigmoid32(x32).astype(np.float64) - sigmoid64(x32.astype(np.float64))) / U).max()))
    print("fp32 sigmoid against float64, worst error in units of u: %.3f" % worst)
    assert E_SIG == E_EXP + 2.0 and 4.0 * worst <= E_SIG, (worst, E_SIG)


def test_cases_span_every_axis():
    cs = [case(k) for k in range(CASES)]
    ns = axis_n()
    s = split_len(257, n_split(), 1)
    assert s > 64 and n_split() % s == 1 and n_split() // s >= 2 and len(set(ns)) == 10
    assert n_split() % split_len(257, n_split(), 0) == 1 and split_len(257, 4097, 0) > 64 and 4097 % split_len(257, 4097, 0) == 1
    assert {c.m for c in cs} == set(MS) and {c.n for c in cs} == set(ns) and {c.kind for c in cs} == set(KINDS)
    for n in (4097, n_split()):
        assert {c.sparse for c in cs if c.m == 257 and c.n == n} == {True, False}
    assert split_len(257, 4097, 1) > 64 and -(-4097 // split_len(257, 4097, 1)) > 1        # the gradients' splits too
    for c in cs:
        if c.sparse:
            r = ref64(c)
            off = np.ones(c.n, bool)
            off[c.targets] = False
            assert np.array_equal(c.A[off], c.B[off]) and not r.J[:, off].any() and not r.ga[:, off].any() and not r.gb[:, off].any()
            assert np.array_equal(c.U * 8, np.round(c.U * 8)) and np.array_equal(c.B * 8, np.round(c.B * 8))
            assert {0, c.n - 1} <= set(c.targets) and float(np.abs(r.J[:, c.targets]).sum()) > 0
    e = next(c for c in cs if c.sparse and c.n == n_split() and c.m == 257)
    assert {s - 1, s, e.n - 1, 63, 64} <= set(e.targets)
    assert max(float(np.abs(ref64(c).a).max()) for c in float_cases()) > 3.0
    tie = [c for c in cs if c.kind == "tie"]
    assert max(float(np.abs(ref64(c).a - ref64(c).b).max()) for c in tie) < 0.1


def test_a_dropped_column_exceeds_the_bound_tenfold():
    """sharpness: on the float cases of 31 to 129 columns the forward bound is at most a tenth of what ONE lost column moves the
    result by (the bound is dominated by gamma(64) of the logits' chains, about 2e-5 of the result where |U| reaches 8: at 4,097
    columns one column is 2.4e-4 of it)"""
    checked = 0
    for c in float_cases():
        if c.kind != "float" or not 31 <= c.n <= 129 or c.m < 31:
            continue
        r, fwd = bounds_of(c)[:2]
        col = int(np.argmax(r.J.sum(axis=0)))
        moved = float(c.scale) * float(r.J[:, col].sum())
        assert moved >= 10.0 * fwd, (c.seed, c.m, c.n, moved, fwd)
        with pytest.raises(AssertionError):
            check_fwd(r.out - moved, c)
        checked += 1
    assert checked >= 3, checked


# ------------------------------------------------------------------------------------------------ GPU: the raw C ABI, guarded
def _on(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def _guarded(n):
    buf = torch.full((n + 2 * GUARD,), SENTINEL, dtype=torch.int32, device="cuda:0")
    return buf, buf[GUARD:GUARD + n].view(torch.float32)


def _guards_ok(buf, n, name):
    b = buf.cpu().numpy()
    assert (b[:GUARD] == SENTINEL).all() and (b[GUARD + n:] == SENTINEL).all(), (name, "wrote outside the output")
    assert not (b[GUARD:GUARD + n] == SENTINEL).any(), (name, "entries never written", int((b[GUARD:GUARD + n] == SENTINEL).sum()))


def _workspace(m, n):
    nbytes = int(_lib().mmrec_mutual_kl_workspace_bytes(m, n, D))
    return torch.full((nbytes // 4 + 4,), SENTINEL, dtype=torch.int32, device="cuda:0")      # a NaN wherever nothing was written


def raw_fwd(c, Ud, Ad, Bd, name="fwd"):
    from mmrec_amd import hip_ops
    p, lib = hip_ops._p, _lib()
    buf, out = _guarded(1)
    ws = _workspace(c.m, c.n)
    rc = lib.mmrec_mutual_kl_f32(p(Ud), p(Ad), p(Bd), c.m, c.n, D, c.scale, p(out), p(ws), hip_ops._stream())
    assert rc == 0, (name, rc)
    torch.cuda.synchronize()
    _guards_ok(buf, 1, name)
    return out.clone()


def raw_bwd(c, Ud, Ad, Bd, g, name="bwd", want=(True, True, True)):
    from mmrec_amd import hip_ops
    p, lib = hip_ops._p, _lib()
    sizes = (c.m * D, c.n * D, c.n * D)
    bufs = [_guarded(s) if w else (None, None) for s, w in zip(sizes, want)]
    ws = _workspace(c.m, c.n)
    rc = lib.mmrec_mutual_kl_bwd_f32(p(Ud), p(Ad), p(Bd), c.m, c.n, D, c.scale, p(g), p(bufs[0][1]), p(bufs[1][1]), p(bufs[2][1]),
                                     p(ws), hip_ops._stream())
    assert rc == 0, (name, rc)
    torch.cuda.synchronize()
    out = []
    for (buf, t), s, nm, rows in zip(bufs, sizes, ("dU", "dA", "dB"), (c.m, c.n, c.n)):
        if buf is None:
            out.append(None)
            continue
        _guards_ok(buf, s, name + " " + nm)
        out.append(t.clone().view(rows, D))
    return out


def _bits(t):
    return t.contiguous().view(torch.int32)


@pytest.mark.gpu
@pytest.mark.parametrize("k", range(CASES))
def test_mutual_kl_fuzz(k):
    c = case(k)
    name = "case %d (m %d n %d %s)" % (k, c.m, c.n, c.kind)
    Ud, Ad, Bd, g = _on(c.U), _on(c.A), _on(c.B), _on(np.array([c.g], np.float32))
    bd = bounds_of(c)
    out = raw_fwd(c, Ud, Ad, Bd, name)
    print("%s: out %.9g ref %.9g bound %.3g" % (name, float(out), bd[0].out, bd[1]))
    w_f = check_fwd(out, c, name, bd)
    dU, dA, dB = raw_bwd(c, Ud, Ad, Bd, g, name)
    w_b = check_bwd(dU, dA, dB, c, name, bd)
    print("%s: worst err / bound forward %.3f backward %.3f" % (name, w_f, w_b))
    # the same launch twice: the same bits, forward and all three gradients
    out2 = raw_fwd(c, Ud, Ad, Bd, name)
    again = raw_bwd(c, Ud, Ad, Bd, g, name)
    assert torch.equal(_bits(out), _bits(out2)), name
    for t, t2 in zip((dU, dA, dB), again):
        assert torch.equal(_bits(t), _bits(t2)), name


@pytest.mark.gpu
def test_a_sweep_nobody_wants_is_skipped_and_the_others_keep_their_bits():
    c = case(15)
    Ud, Ad, Bd, g = _on(c.U), _on(c.A), _on(c.B), _on(np.array([c.g], np.float32))
    full = raw_bwd(c, Ud, Ad, Bd, g)
    for want in ((True, False, False), (False, True, False), (False, False, True), (False, True, True)):
        got = raw_bwd(c, Ud, Ad, Bd, g, want=want)
        for t, f, w in zip(got, full, want):
            assert (t is None) == (not w)
            if w:
                assert torch.equal(_bits(t), _bits(f)), want


@pytest.mark.gpu
def test_a_nan_row_of_u_follows_the_float64_pattern():
    """a NaN in one row of U: the scalar is NaN, that row of dU is NaN and no other, dA and dB are NaN wherever the float64
    formulas (and autograd's GEMMs) make them so"""
    base = case(15)
    for row in (0, 45, 128, 256):
        c = Case()
        c.__dict__.update(base.__dict__)
        c.U = base.U.copy()
        c.U[row, 7] = np.nan
        Ud, Ad, Bd, g = _on(c.U), _on(c.A), _on(c.B), _on(np.array([c.g], np.float32))
        out = raw_fwd(c, Ud, Ad, Bd)
        assert bool(torch.isnan(out).all()), row
        r = ref64(c)
        assert np.isnan(r.out)
        for got, ref in zip(raw_bwd(c, Ud, Ad, Bd, g), (r.dU, r.dA, r.dB)):
            assert np.array_equal(np.isnan(_arr(got)), np.isnan(ref)), row
            assert np.isfinite(_arr(got)[~np.isnan(ref)]).all(), row
        assert np.isnan(r.dU[row]).all() and not np.isnan(np.delete(r.dU, row, axis=0)).any()


@pytest.mark.gpu
def test_saturated_logits_stay_finite_and_within_the_bound():
    """logits of +-30: the composition is NaN (0 * log 0), J and its gradients are finite and meet the float bound"""
    from mmrec_amd import hip_ops
    rng = np.random.default_rng(77)
    c = Case()
    c.seed, c.m, c.n, c.kind, c.sparse, c.targets, c.g = 0, 33, 65, "float", False, None, 1.0
    unit = lambda x: x / np.linalg.norm(x, axis=1, keepdims=True)      # noqa: E731
    A, B = unit(rng.standard_normal((c.n, D))), unit(rng.standard_normal((c.n, D)))
    Um = 30.0 * np.where(rng.random((c.m, 1)) < 0.5, 1.0, -1.0) * A[rng.integers(0, c.n, c.m)]
    c.U, c.A, c.B = (np.ascontiguousarray(x, np.float32) for x in (Um, A, B))
    c.scale = float(np.float32(1.0 / (c.m * c.n)))
    r = ref64(c)
    assert float(np.abs(r.a).max()) > 29.0 and float(np.abs(r.a).min()) < 10.0
    Ud, Ad, Bd, g = _on(c.U), _on(c.A), _on(c.B), _on(np.array([c.g], np.float32))
    bd = bounds_of(c)
    out = raw_fwd(c, Ud, Ad, Bd)
    assert bool(torch.isfinite(out).all())
    w_f = check_fwd(out, c, "saturated", bd)
    w_b = check_bwd(*raw_bwd(c, Ud, Ad, Bd, g), c, "saturated", bd)
    print("saturated logits: out %.9g, worst err / bound forward %.3f backward %.3f" % (float(out), w_f, w_b))
    assert not bool(torch.isfinite(hip_ops.mutual_kl_torch(Ud, Ad, Bd)))          # the documented difference


@pytest.mark.gpu
def test_no_m_by_n_block_is_ever_held():
    """m = 257, n = 4,097 through the op, forward + backward: the peak above the inputs stays under the workspace + the three
    gradients and the scalar + 1 MB; the composition's peak exceeds eight [m, n] blocks"""
    from mmrec_amd import hip_ops
    c = case(15)
    m, n = c.m, c.n

    def peak_of(fn):
        # `max_memory_allocated` counts whole blocks: a cached block left by an earlier test is handed out unsplit when it is up
        # to 1 MB larger than the request, and would be charged to the op.  With the cache emptied every block is cut to size.
        gc.collect()
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        Ud, Ad, Bd = (_on(x).requires_grad_() for x in (c.U, c.A, c.B))
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        out = fn(Ud, Ad, Bd)
        out.backward()
        torch.cuda.synchronize()
        return torch.cuda.max_memory_allocated() - base, out.detach(), (Ud.grad, Ad.grad, Bd.grad)
    assert hip_ops.mutual_kl_served(_on(c.U), _on(c.A), _on(c.B))
    peak, out, grads = peak_of(hip_ops.mutual_kl)
    limit = int(_lib().mmrec_mutual_kl_workspace_bytes(m, n, D)) + (m + 2 * n) * D * 4 + 4 + (1 << 20)
    peak_t, out_t, _ = peak_of(hip_ops.mutual_kl_torch)
    print("peak above the inputs: op %.2f MB (limit %.2f MB), composition %.2f MB (one block %.2f MB)"
          % (peak / 2 ** 20, limit / 2 ** 20, peak_t / 2 ** 20, m * n * 4 / 2 ** 20))
    assert peak < limit, (peak, limit)
    assert peak_t > 8 * m * n * 4, peak_t
    c1 = Case()
    c1.__dict__.update(c.__dict__)
    c1.g = 1.0
    bd = bounds_of(c1)
    check_fwd(out, c1, "op", bd)
    check_bwd(*grads, c1, "op", bd)
    assert abs(float(out) - float(out_t)) <= 1e-5 * abs(float(out_t))


@pytest.mark.gpu
def test_forward_and_backward_replay_from_a_captured_graph():
    """m = 64, n = 200: forward + backward captured on one stream and replayed give the eager bits (no host synchronisation, no
    data-dependent launch shape)"""
    from mmrec_amd import hip_ops
    rng = np.random.default_rng(9)
    u0, a0, b0 = (rng.standard_normal(s).astype(np.float32) * 0.3 for s in ((64, 64), (200, 64), (200, 64)))

    def step(Ud, Ad, Bd):
        Ud.grad = Ad.grad = Bd.grad = None
        out = hip_ops.mutual_kl(Ud, Ad, Bd)
        (out * 1.5).backward()
        return out.detach(), Ud.grad, Ad.grad, Bd.grad
    Ud, Ad, Bd = (_on(x).requires_grad_() for x in (u0, a0, b0))
    eager = [t.clone() for t in step(Ud, Ad, Bd)]
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        held = step(Ud, Ad, Bd)
    with torch.no_grad():                                   # other inputs in the same buffers, then the first ones again
        Ud.copy_(_on(u0[::-1].copy())), Ad.copy_(_on(a0[::-1].copy()))
    graph.replay()
    torch.cuda.synchronize()
    other = [t.clone() for t in held]
    with torch.no_grad():
        Ud.copy_(_on(u0)), Ad.copy_(_on(a0))
    graph.replay()
    torch.cuda.synchronize()
    for a, b, o in zip(eager, held, other):
        assert torch.equal(_bits(a), _bits(b))
        assert not torch.equal(_bits(a), _bits(o))          # the replay really computed
