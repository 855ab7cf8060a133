"""GPU: seeded differential fuzz of MVGAE's encoder heads kernels (csrc/encoder_heads.hip: mmrec_encoder_heads_fwd_f32 /
_bwd_f32) against float64 numpy of the formulas of include/mmrec_hip.h, computed from the fp32 arrays each call was given -- never
against another kernel or the torch composition.  The raw C ABI is called over guarded, sentinel-filled outputs and a
sentinel-filled workspace of exactly the reported size.

    a = AX W_h + b_h, nrm = max(||a||, 1e-12), u = a / nrm, d = u scale_h, hh = leaky(d), p = X L_h^T + bl_h
    out_h = hh G_h^T + bg_h + leaky(p)
    dhh = g_h G_h, du = dhh leaky'(d) scale_h, da = (du - u <u, du>) / nrm (||a|| >= 1e-12) or du / 1e-12, dp = g_h leaky'(p)
    dAX = sum_h da W_h^T, dX = sum_h dp L_h, dW_h = AX^T da, db_h = colsum(da), dG_h = g_h^T hh, dbg_h = colsum(g_h),
    dL_h = dp^T X, dbl_h = colsum(dp)

ACCEPTANCE: |got - ref| <= (1 + 2^-10) e, with e a first-order bound that is carried along the float64 evaluation, operation by
operation as the PLAN of include/mmrec_hip.h names them (u = 2^-24, gamma(n) = n u / (1 - n u), 2^-149 per rounding for
underflow, none where the operands are exact and the result is an exact zero) -- derived from that text, not tuned to a result:
    one rounding (+, -, *, /, fma)   e = (the operands' errors through the operation's partial derivatives at the reference's
                                     magnitudes) + u |value|
    a chain of n fma from a start    e = e_A |B| + e_start + gamma(n) (|A| |B| + |start|).  a, p, dhh: n = 64;  the out chain: 64
                                     from bg, then one addition;  ss and the dot <u, du>: 4 fma + 4 butterfly additions, n = 8;
                                     dAX, dX: ONE chain of 64 H terms over the heads
    sqrtf                            correctly rounded: the interval [ss - e, ss + e] through the square root, + u |value|
    the clamp                        the branch is the REFERENCE's (||a|| < 1e-12f); tests/test_encoder_heads_cpu.py shows that no
                                     row of any case has ||a|| within its bound of the constant, so the kernel takes the same one.
                                     A clamped row's nrm is the constant, exact.
    leaky(z)                         the largest slope on [z - e, z + e] times e, + u |value|
    leaky'(z)                        1 or slope by the reference's sign (0 takes slope).  Where the bound cannot decide the sign
                                     (|z| <= e and e > 0: with e == 0 the kernel's z IS the reference's) the kernel may take the
                                     other factor: the entry's gradient bound is WIDENED by (1 - slope) |incoming| (incoming:
                                     dhh scale, or g), never excluded; the CPU file caps the share of such entries at 2e-4
    weight gradients                 one fma chain over the R rows of a block (R from the library), then the finish,
                                     F = ceil(blocks / 4) + 3: gamma(R + F);  db, dbg, dbl: R / 16 + 16 + F additions
The worst err / bound per family (out;  dx: dAX, dX;  dw: dW, dG, dL;  db: db, dbg, dbl) is printed by every case and recorded in
EXPERIMENTS.md section 4.
EXACTNESS, every case: the same calls again give the same bits; guards and sentinels intact; with g zero every gradient is zero;
where a head's rows are all dropped (scale == 0) its dW and db are exactly 0; H = 5 is MMREC_ERR_UNSUPPORTED and touches nothing.
`test_cases_span_every_axis` needs no GPU; the checker's own tests (an fp32 emulation of the plan passes, planted errors do not,
the kink and clamp conditions) are in tests/test_encoder_heads_cpu.py."""
import numpy as np
import pytest
import torch

from tests.test_hyper_fuzz_gpu import _bits, _collect, _lib, _outs, compare, f64
from tests.test_edge_softmax_fuzz_gpu import GUARD, SENTINEL
from tests.test_spmm_fuzz_gpu import U, _on, gamma

D = 64
PART = 3 * (D * D + D)                         # floats of one block's partial of one head
MAX_BLOCKS = 256
BIG = 20011                                    # 157 blocks of two tiles: every thread of the finish adds 39 or 40 partials
CASES = 36
KINDS = ("mixed", "zero_b0", "zero_b", "tiny", "zerox")
SCALES = ("null", "bern", "rows")
SLACK = 1.0 + 2.0 ** -10
TINY = 2.0 ** -149
SLOPE = 0.01
EPS = float(np.float32(1e-12))
UNSUPPORTED = 10002
OPERANDS = ("AX", "X", "W", "b", "G", "bg", "L", "bl")
GRADS = ("dAX", "dX", "dW", "db", "dG", "dbg", "dL", "dbl")
FAMILY = dict(out="out", dAX="dx", dX="dx", dW="dw", dG="dw", dL="dw", db="db", dbg="db", dbl="db")


def rows_per_block(n):
    return int(_lib().mmrec_encoder_heads_rows_per_block(int(n)))


def blocks(n):
    return -(-n // rows_per_block(n)) if n > 0 else 0


def n_finish(n):
    return -(-blocks(n) // 4) + 3


def axis_n():
    r = rows_per_block(1)
    return tuple(sorted({0, 1, 2, 63, 64, 65, r - 1, r, r + 1, 2 * r + 1}))


class Case:
    pass


def _shape(c, name):
    return ((c.n, D) if name in ("dAX", "dX") else (c.H, c.n, D) if name == "out" else (c.H, D, D) if name in ("dW", "dG", "dL")
            else (c.H, D))


def case(k):
    ns = axis_n()
    c = Case()
    c.k = k
    c.unsupported = k == CASES - 1                                        # H = 5: refused, nothing touched
    c.n = n = BIG if k == 5 else 65 if c.unsupported else ns[k % len(ns)]
    c.H = H = 2 if k == 5 else 5 if c.unsupported else 1 + k % 3
    c.kind = "mixed" if k == 5 else KINDS[k % 5]
    c.scale_mode = "bern" if k == 5 else SCALES[(k // 3) % 3]
    c.g_zero = k % 9 == 4
    rng = np.random.default_rng(7300 + k)
    want = rng.random(8) < 0.6
    if k % 6 == 5:
        want[:] = True
    if k % 6 == 2:
        want[2:] = False                                                  # no weight gradient: the finish is not launched
    c.want = tuple(bool(w) for w in want)
    c.null_ws = not any(c.want[2:]) and k % 4 != 0
    rows = lambda: rng.standard_normal((n, D)) * rng.choice([1.0, 1e-3, 1e3], size=(n, 1), p=[0.6, 0.2, 0.2])     # noqa: E731
    AX, X = rows(), rows()
    lin = lambda *s: rng.uniform(-0.125, 0.125, s)                        # noqa: E731  (nn.Linear's init for 64 inputs)
    w = dict(W=lin(H, D, D), b=lin(H, D), G=lin(H, D, D), bg=lin(H, D), L=lin(H, D, D), bl=lin(H, D))
    c.planted = np.zeros(n, bool)                                         # rows on the clamp's side, or decades above it
    c.below = np.zeros(n, bool)                                           # ... those with ||a|| < 1e-12
    if c.kind != "mixed" and n:
        pick = rng.random(n) < 0.3
        pick[rng.integers(0, n)] = True
        if c.kind in ("zero_b0", "zero_b"):
            AX[pick] = 0.0
            if c.kind == "zero_b0":
                w["b"][:] = 0.0                                           # a = 0 exactly: the clamp branch with u = 0
                c.planted, c.below = pick, pick
        if c.kind == "tiny":                                              # ||a|| about 1e-14, and about 1e-8, with b = 0
            w["b"][:] = 0.0
            low = pick & (rng.random(n) < 0.5)
            low[np.flatnonzero(pick)[0]] = True
            AX[pick] = rng.standard_normal((int(pick.sum()), D)) * 1e-9
            AX[low] = rng.standard_normal((int(low.sum()), D)) * 2e-15
            c.planted, c.below = pick, low
        if c.kind == "zerox":
            X[pick] = 0.0
    c.ops = {key: np.ascontiguousarray(v, np.float32) for key, v in dict(AX=AX, X=X, **w).items()}
    c.scale, c.head0_dropped = None, False
    if c.scale_mode != "null":
        s = (rng.random((H, n, D)) < 0.9) / 0.9
        if c.scale_mode == "rows":
            s[rng.random((H, n)) < 0.3] = 0.0                             # whole rows dropped
            if k % 2 == 0:
                s[0] = 0.0                                                # ... and every row of head 0
                c.head0_dropped = True
        c.scale = np.ascontiguousarray(s, np.float32)
    c.g = np.zeros((H, n, D), np.float32) if c.g_zero else rng.standard_normal((H, n, D)).astype(np.float32)
    return c


def name_of(c):
    return "case %d (n %d H %d %s scale %s%s want %s%s)" % (c.k, c.n, c.H, c.kind, c.scale_mode, " g0" if c.g_zero else "",
                                                           "".join("x" if w else "." for w in c.want), " no ws" if c.null_ws else "")


# ------------------------------------------------------------------------------------------------ the reference and its bound
# a quantity is a pair (float64 value, first-order bound of the kernel's error in it)
def ex(v):
    v = np.asarray(v, np.float64)
    return v, np.zeros_like(v)


def _r(v, e):
    """one rounding; an exact zero of exact operands is exact"""
    return v, e + U * np.abs(v) + np.where((v == 0) & (e == 0), 0.0, TINY)


def t_add(a, b):
    return _r(a[0] + b[0], a[1] + b[1])


def t_mul(a, b):
    return _r(a[0] * b[0], np.abs(a[0]) * b[1] + np.abs(b[0]) * a[1])


def t_fma(a, b, c):
    return _r(a[0] * b[0] + c[0], np.abs(a[0]) * b[1] + np.abs(b[0]) * a[1] + c[1])


def t_div(a, b):
    v = a[0] / b[0]
    return _r(v, (a[1] + np.abs(v) * b[1]) / np.abs(b[0]))


def t_neg(a):
    return -a[0], a[1]


def t_chain(A, B, start, n):
    """a chain of n fma: A [r, s] times the exact matrix B [s, c], from `start`"""
    mag = np.abs(A[0]) @ np.abs(B) + np.abs(start[0])
    e = A[1] @ np.abs(B) + start[1]
    return A[0] @ B + start[0], e + gamma(n) * mag + np.where((mag == 0) & (e == 0), 0.0, n * TINY)


def t_rowdot(a, b, n=8):
    v = (a[0] * b[0]).sum(axis=1, keepdims=True)
    e = (np.abs(a[0]) * b[1] + np.abs(b[0]) * a[1]).sum(axis=1, keepdims=True)
    mag = (np.abs(a[0]) * np.abs(b[0])).sum(axis=1, keepdims=True)
    return v, e + gamma(n) * mag + np.where((mag == 0) & (e == 0), 0.0, n * TINY)


def t_sqrt(x):
    v = np.sqrt(x[0])
    e = np.maximum(np.sqrt(x[0] + x[1]) - v, v - np.sqrt(np.maximum(x[0] - x[1], 0.0)))
    return v, e + U * v


def t_leaky(z, slope):
    v = np.where(z[0] > 0, z[0], slope * z[0])
    return _r(v, np.where(z[0] + z[1] > 0, 1.0, slope) * z[1])


def undecided(z):
    """the entries whose sign the bound cannot decide"""
    return (np.abs(z[0]) <= z[1]) & (z[1] > 0)


def t_colsum(t, n):
    return t[0].sum(axis=0), t[1].sum(axis=0) + gamma(n) * np.abs(t[0]).sum(axis=0) + n * TINY


def t_outer(dz, X, n):
    """sum over rows of dz^T X, each output one chain of n roundings"""
    mag = np.abs(dz[0]).T @ np.abs(X[0])
    return dz[0].T @ X[0], dz[1].T @ np.abs(X[0]) + np.abs(dz[0]).T @ X[1] + gamma(n) * mag + n * TINY


def bounds(ops, scale, g, slope=SLOPE, R=None, F=None, info=None):
    """-> {name: (float64 reference, bound)} for out and the eight gradients; `info`: a dict that receives, per head, the norms
    ||a|| with their bounds and the undecided entries of d and p"""
    o = {k: f64(v) for k, v in ops.items()}
    AX, X = o["AX"], o["X"]
    n, H = AX.shape[0], o["W"].shape[0]
    R = rows_per_block(n) if R is None else R
    F = n_finish(n) if F is None else F
    s = float(np.float32(slope))
    n_col = R // 16 + 16 + F
    res = {k: [] for k in ("out", "dW", "db", "dG", "dbg", "dL", "dbl")}
    dAX, dX = [np.zeros((n, D)), np.zeros((n, D))], [np.zeros((n, D)), np.zeros((n, D))]
    for h in range(H):
        a = t_chain(ex(AX), o["W"][h], ex(o["b"][h][None, :]), 64)
        raw = t_sqrt(t_rowdot(a, a))
        clamped = raw[0] < EPS
        nrm = (np.where(clamped, EPS, raw[0]), np.where(clamped, 0.0, raw[1]))
        u = t_div(a, nrm)
        sc = None if scale is None else ex(f64(scale[h]))
        d = u if sc is None else t_mul(u, sc)
        hh = t_leaky(d, s)
        p = t_chain(ex(X), o["L"][h].T, ex(o["bl"][h][None, :]), 64)
        res["out"].append(t_add(t_chain(hh, o["G"][h].T, ex(o["bg"][h][None, :]), 64), t_leaky(p, s)))
        gh = ex(f64(g[h]))
        dhh = t_chain(gh, o["G"][h], ex(np.zeros((n, D))), 64)
        und_d, und_p = undecided(d), undecided(p)
        du = t_mul(dhh, ex(np.where(d[0] > 0, 1.0, s)))
        inc = np.abs(dhh[0]) + dhh[1]
        if sc is not None:
            du = t_mul(du, sc)
            inc = inc * np.abs(sc[0])
        du = (du[0], du[1] + und_d * (1.0 - s) * inc)
        dot = t_rowdot(u, du)
        live, dead = t_div(t_fma(t_neg(u), dot, du), nrm), t_div(du, nrm)
        da = (np.where(clamped, dead[0], live[0]), np.where(clamped, dead[1], live[1]))
        dp = t_mul(gh, ex(np.where(p[0] > 0, 1.0, s)))
        dp = (dp[0], dp[1] + und_p * (1.0 - s) * np.abs(gh[0]))
        for acc, t, M in ((dAX, da, o["W"][h].T), (dX, dp, o["L"][h])):
            acc[0] = acc[0] + t[0] @ M
            acc[1] = acc[1] + t[1] @ np.abs(M) + gamma(64 * H) * (np.abs(t[0]) @ np.abs(M))
        w = t_outer(da, ex(AX), R + F)
        res["dW"].append((w[0].T, w[1].T))
        w = t_outer(hh, gh, R + F)
        res["dG"].append((w[0].T, w[1].T))
        res["dL"].append(t_outer(dp, ex(X), R + F))
        res["db"].append(t_colsum(da, n_col))
        res["dbg"].append(t_colsum(gh, n_col))
        res["dbl"].append(t_colsum(dp, n_col))
        if info is not None:
            info.setdefault("raw", []).append(raw)
            info.setdefault("und_d", []).append(und_d)
            info.setdefault("und_p", []).append(und_p)
    out = {k: (np.stack([t[0] for t in v]), np.stack([t[1] for t in v])) for k, v in res.items()}
    out["dAX"] = (dAX[0], dAX[1] + 64 * H * TINY)
    out["dX"] = (dX[0], dX[1] + 64 * H * TINY)
    return {k: (v, SLACK * e) for k, (v, e) in out.items()}


def check(ops, scale, g, got, name, slope=SLOPE, R=None, F=None):
    """got: {name: array or tensor} of any subset of the outputs -> the worst err / bound per family"""
    b = bounds(ops, scale, g, slope, R, F)
    worst = {}
    for k, v in got.items():
        v = v.reshape(b[k][0].shape) if hasattr(v, "reshape") else v
        worst[FAMILY[k]] = max(worst.get(FAMILY[k], 0.0), compare(v, *b[k], name + " " + k))
    return worst


# ------------------------------------------------------------------------------------------------ no GPU: the axes
def test_cases_span_every_axis():
    cs = [case(k) for k in range(CASES)]
    ns = axis_n()
    r = rows_per_block(1)
    assert r == 64 and rows_per_block(BIG) == 128 and blocks(BIG) == 157 and n_finish(BIG) == 43
    assert {0, 1, 2, 63, 64, 65, r - 1, r, r + 1, 2 * r + 1} <= set(ns)
    assert set(ns) | {BIG} == {c.n for c in cs}
    assert {c.H for c in cs} == {1, 2, 3, 5} and [c.k for c in cs if c.unsupported] == [CASES - 1] and cs[-1].H == 5
    cs = cs[:-1]
    assert {c.kind for c in cs} == set(KINDS) and {c.scale_mode for c in cs} == set(SCALES)
    for kind in KINDS:
        sub = [c for c in cs if c.kind == kind and c.n]
        assert {c.scale_mode for c in sub} == set(SCALES) and {c.H for c in sub} == {1, 2, 3}, kind
        assert len({c.n for c in sub}) >= 5 and max(c.n for c in sub) > 64, kind
    for i in range(8):                                                    # every output wanted somewhere, and not wanted
        assert {c.want[i] for c in cs} == {True, False}, GRADS[i]
    assert any(all(c.want) for c in cs) and any(not any(c.want[2:]) for c in cs)
    assert {c.null_ws for c in cs} == {True, False} and all(not c.null_ws or not any(c.want[2:]) for c in cs)
    assert any(c.g_zero and c.n > 64 for c in cs) and any(c.head0_dropped and c.n > 64 and c.want[2] for c in cs)
    big = cs[5]
    assert big.n == BIG and big.H == 2 and all(big.want) and big.kind == "mixed" and big.scale_mode == "bern" and not big.g_zero
    for c in cs:
        assert (c.scale is None) == (c.scale_mode == "null")
        if c.n < 60:
            continue
        mags = np.abs(c.ops["AX"]).max(axis=1)
        if c.kind == "mixed":
            assert (mags > 100).any() and (mags < 0.1).any() and ((mags > 0.5) & (mags < 10)).any()
        if c.kind in ("zero_b0", "zero_b"):
            assert (mags == 0).any() and (np.abs(c.ops["b"]).max() == 0) == (c.kind == "zero_b0")
        if c.kind == "tiny":
            assert c.below.any() and (c.planted & ~c.below).any() and (mags[c.below] < 1e-13).all()
        if c.kind == "zerox":
            assert (np.abs(c.ops["X"]).max(axis=1) == 0).any()
        if c.scale_mode == "bern":
            assert 0.8 < float((c.scale > 0).mean()) < 0.97 and set(np.unique(c.scale)) == {np.float32(0), np.float32(1 / 0.9)}
        if c.scale_mode == "rows":
            assert (np.abs(c.scale).max(axis=2) == 0).any() and (c.scale[0].max() == 0) == c.head0_dropped


# ------------------------------------------------------------------------------------------------ GPU: the raw C ABI, guarded
def _workspace(n, H):
    nbytes = int(_lib().mmrec_encoder_heads_workspace_bytes(n, H))
    assert nbytes == blocks(n) * H * PART * 4 and blocks(n) <= MAX_BLOCKS
    return torch.full((nbytes // 4 + GUARD,), SENTINEL, dtype=torch.int32, device="cuda:0"), nbytes // 4


def run_case(c, rc_want=0):
    """the case's forward and backward through the raw ABI -> {name: tensor} of every output written"""
    from mmrec_amd import hip_ops
    p_, lib, name = hip_ops._p, _lib(), name_of(c)
    ops = [_on(c.ops[k]) for k in OPERANDS]
    scale = None if c.scale is None else _on(c.scale)
    g = _on(c.g)
    shapes = {"out": _shape(c, "out")}
    held, ptr = _outs(shapes)
    rc = lib.mmrec_encoder_heads_fwd_f32(*[p_(t) for t in ops], p_(scale), c.n, D, c.H, SLOPE, ptr["out"], hip_ops._stream())
    assert rc == rc_want, (name, rc)
    written = c.n and not rc_want
    out = _collect(held, shapes, name) if written else {}
    all_held = list(held.values())
    shapes = {k: _shape(c, k) if w else None for k, w in zip(GRADS, c.want)}
    held, ptr = _outs(shapes)
    ws, n_ws = (None, 0) if c.null_ws or rc_want else _workspace(c.n, c.H)
    if rc_want:                                                           # a workspace that must not be touched either
        ws, n_ws = torch.full((PART + GUARD,), SENTINEL, dtype=torch.int32, device="cuda:0"), 0
    rc = lib.mmrec_encoder_heads_bwd_f32(*[p_(t) for t in ops], p_(scale), p_(g), c.n, D, c.H, SLOPE, *[ptr[k] for k in GRADS],
                                         p_(ws), hip_ops._stream())
    assert rc == rc_want, (name, rc)
    if written:
        out.update(_collect(held, shapes, name))
    else:
        torch.cuda.synchronize()
        for buf, view in all_held + list(held.values()):                  # no launch: nothing is written
            assert bool((buf == SENTINEL).all()), name
    if ws is not None:
        assert bool((ws[n_ws:] == SENTINEL).all()), (name, "wrote beyond the workspace")
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("k", range(CASES))
def test_encoder_heads_fuzz(k):
    c = case(k)
    name = name_of(c)
    if c.unsupported:
        assert run_case(c, UNSUPPORTED) == {}
        return
    got = run_case(c)
    worst = check(c.ops, c.scale, c.g, got, name) if c.n else {}
    print("%s: worst err / bound %s" % (name, " ".join("%s %.3f" % kv for kv in sorted(worst.items()))))
    if c.n:
        assert set(got) == {"out"} | {k_ for k_, w in zip(GRADS, c.want) if w}, name
    if c.g_zero:
        for k_ in GRADS:
            if k_ in got:
                assert not bool(got[k_].any()), (name, k_, "a gradient of g = 0 is zeros")
    if c.head0_dropped:
        for k_ in ("dW", "db"):
            if k_ in got:
                assert not bool(got[k_][0].any()), (name, k_, "a head whose rows are all dropped gives its convolution nothing")
    again = run_case(c)                                                   # the same calls again: the same bits
    assert got.keys() == again.keys()
    for k_ in got:
        assert torch.equal(_bits(got[k_]), _bits(again[k_])), (name, k_, "not repeatable")


@pytest.mark.gpu
def test_wrapper_autograd_takes_the_kernels_and_honours_needs_input_grad():
    """hip_ops.encoder_heads with only some operands requiring gradients: the library is given NULL for the rest, the results meet
    the raw ABI's bounds, and an unserved call is the torch composition bit for bit"""
    from mmrec_amd import hip_ops
    c = case(34)
    assert c.n > 2 * 64 and c.H == 2 and c.scale is not None and not c.g_zero
    lib = _lib()
    seen = []
    real_b = lib.mmrec_encoder_heads_bwd_f32
    needs = dict(AX=True, X=False, W=True, b=False, G=False, bg=True, L=False, bl=False)
    ops = [_on(c.ops[k]).requires_grad_(needs[k]) for k in OPERANDS]
    scale, g = _on(c.scale), _on(c.g)
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(lib, "mmrec_encoder_heads_bwd_f32", lambda *a: seen.append(a) or real_b(*a))
        assert hip_ops.encoder_heads_served(*ops, scale)
        out = hip_ops.encoder_heads(*ops, scale)
        (out * g).sum().backward()
        torch.cuda.synchronize()
    assert len(seen) == 1
    a = seen[0]
    assert [x is not None for x in a[14:22]] == [needs[k] for k in OPERANDS] and a[22] is not None
    got = {"out": out.detach()}
    got.update({"d" + k: t.grad for k, t in zip(OPERANDS, ops) if needs[k]})
    assert all(t.grad is None for k, t in zip(OPERANDS, ops) if not needs[k])
    print("wrapper: worst err / bound", check(c.ops, c.scale, c.g, got, "wrapper"))
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(hip_ops, "ENCODER_HEADS", False)
        assert not hip_ops.encoder_heads_served(*ops, scale)
        off = hip_ops.encoder_heads(*ops, scale)
    ref = hip_ops.encoder_heads_torch(*ops, scale)
    assert torch.equal(_bits(off.detach()), _bits(ref.detach()))
    assert not hip_ops.encoder_heads_served(ops[0][:, ::2], *ops[1:]) and not hip_ops.encoder_heads_served(ops[0].cpu(), *ops[1:])
