"""GPU: seeded differential fuzz of MGCN's fuser kernels (csrc/modal_fusion.hip: mmrec_modal_fusion_fwd_f32 / _bwd_f32) against
float64 numpy of the formulas of include/mmrec_hip.h, computed from the fp32 arrays each call was given -- never against another
kernel or the torch composition.  The raw C ABI is called over guarded, sentinel-filled outputs and a sentinel-filled workspace of
exactly the reported size.

    zV = V Wq^T + bq, hV = tanh(zV), sV = <hV, q>  (zT, hT, sT alike);  (aV, aT) = softmax(sV, sT);  m = aV V + aT T
    pV = sigmoid(C Wv^T + bv), pT = sigmoid(C Wt^T + bt);  side = (pV (V - m) + pT (T - m) + m) / 3;  out = C + side
    G = g_side + g_out, G3 = G / 3;  dpV = G3 (V - m), dpT = G3 (T - m), dm = G3 (1 - pV - pT);  dsV = aV aT <dm, V - T> = -dsT
    dzV = dsV q (1 - hV^2), dzT alike;  duV = dpV pV (1 - pV), duT alike
    dV = G3 pV + aV dm + dzV Wq, dT alike;  dC = g_out + duV Wv + duT Wt
    dq = sum_rows (dsV hV + dsT hT), dWq = sum_rows (dzV^T V + dzT^T T), dbq = sum_rows (dzV + dzT), dWv = sum_rows duV^T C, ...

ACCEPTANCE: |got - ref| <= (1 + 2^-10) e, with e a first-order bound that is carried along the float64 evaluation, operation by
operation as the PLAN of include/mmrec_hip.h names them (u = 2^-24, gamma(n) = n u / (1 - n u), 2^-149 per rounding for
underflow) -- derived from that text, not tuned to a result:
    one rounding (+, -, *, /, fma)   e = (the operands' errors through the operation's partial derivatives at the reference's
                                     magnitudes) + u |value|:  a b -> |a| e_b + |b| e_a;  a / b -> (e_a + |a / b| e_b) / |b|
    a chain of n fma from a start    e = e_A |B| + |A| e_B + e_start + gamma(n) (|A| |B| + |start|): the product over absolute
                                     values.  z, u: n = 64 from the bias;  dV, dT: 64 from fma(a, dm, G3 p);  dC: 128 from g_out;
                                     s and the dot <dm, V - T>: 4 fma + 4 butterfly additions, n = 8
    expf(x)                          e^x (expm1(e_x) + E_EXP u e^(e_x)) + 2^-125: E_EXP u relative (the device constant measured in
                                     tests/test_edge_softmax_fuzz_gpu.py; every argument here is <= 0 and, for tanh / sigmoid,
                                     exact), the argument's error through the exponential, a flushed subnormal result
    tanh                             h = (1 - qe) / (1 + qe), qe = expf(-2 |z|): three roundings and qe's E_EXP u, which reaches h
                                     through dh / dqe = -2 / (1 + qe)^2 = -(1 - h^2) / (2 qe):
                                     e = D e_z + u ((1 - h^2) E_EXP / 2 + 3 |h|), D = 1 - tanh^2 taken where it is LARGEST on
                                     [|z| - e_z, |z| + e_z] (the mean value theorem, not the value at z)
    sigmoid                          p = (1 or qe) / (1 + qe), qe = expf(-|z|): e = D e_z + u (p (1 - p) E_EXP + 2 p), D = p (1 - p)
                                     where it is largest on the interval
    softmax                          nothing special: sV - mx, expf, eV + eT and the two divisions by the rules above
    weight gradients                 dWq: one fma chain over the 2 R terms of a block (R = rows per block, from the library), then
                                     the finish, F = ceil(blocks / 4) + 3: e = (e_dz)^T |V| + ... + gamma(2 R + F) (|dz|^T |V| + ...);
                                     dWv, dWt: gamma(R + F);  dbq, dbv, dbt, dq: the term's own roundings, then R / 16 + 16 + F
                                     additions
The worst err / bound per family (out: side, out;  dx: dV, dT, dC;  dw: the matrices;  db: dbq, dbv, dbt, dq) is printed by every
case and recorded in EXPERIMENTS.md section 4.
EXACTNESS, every case: the same calls again give the same bits; guards and sentinels intact; a wanted gradient with both g NULL
is zeros; where every row has V == T, dWq, dbq and dq are exactly 0 (aV = aT = 0.5 and the dot is exactly 0).
`test_cases_span_every_axis` needs no GPU; the checker's own tests (an fp32 emulation of the plan passes, planted errors do not)
are in tests/test_modal_fusion_cpu.py."""
import numpy as np
import pytest
import torch

from tests.test_hyper_fuzz_gpu import _bits, _collect, _lib, _outs, compare, f64
from tests.test_edge_softmax_fuzz_gpu import E_EXP, GUARD, SENTINEL
from tests.test_spmm_fuzz_gpu import U, _on, gamma

D = 64
PART = 3 * (D * D + D) + D                     # floats of one block's partial
MAX_BLOCKS = 256
BIG = 20011                                    # 157 blocks of two tiles: every thread of the finish adds 39 or 40 partials
CASES = 36
KINDS = ("mixed", "zeros", "equal", "onehot", "saturated")
SLACK = 1.0 + 2.0 ** -10
TINY = 2.0 ** -149
FLOOR = 2.0 ** -125
OPERANDS = ("V", "T", "C", "Wq", "bq", "q", "Wv", "bv", "Wt", "bt")
GRADS = ("dV", "dT", "dC", "dWq", "dbq", "dq", "dWv", "dbv", "dWt", "dbt")
FAMILY = dict(side="out", out="out", dV="dx", dT="dx", dC="dx", dWq="dw", dWv="dw", dWt="dw", dbq="db", dbv="db", dbt="db", dq="db")


def rows_per_block(n):
    return int(_lib().mmrec_modal_fusion_rows_per_block(int(n)))


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
    return (c.n, D) if name in ("V", "T", "C", "dV", "dT", "dC", "side", "out") else (D, D) if "W" in name else (D,)


def case(k):
    ns = axis_n()
    c = Case()
    c.k = k
    c.n = n = BIG if k == 5 else ns[k % len(ns)]
    c.kind = KINDS[k % 5]
    c.all_equal = c.kind == "equal" and k % 2 == 0                        # every row has V == T
    c.g_mask = 3 if k == 5 else (3 * k + 1) % 4                           # bit 0: g_side given, bit 1: g_out
    rng = np.random.default_rng(7100 + k)
    want = rng.random(10) < 0.6
    if c.all_equal:
        want[3:6] = True                                                  # dWq, dbq, dq: exactly zero there
    if k % 6 == 5:
        want[:] = True
    if k % 6 == 2:
        want[3:] = False                                                  # no weight gradient: the finish is not launched
    c.want = tuple(bool(w) for w in want)
    c.null_ws = not any(c.want[3:]) and k % 4 != 0
    rows = lambda: rng.standard_normal((n, D)) * rng.choice([1.0, 1e-3, 1e3], size=(n, 1), p=[0.6, 0.2, 0.2])     # noqa: E731
    V, T, C = rows(), rows(), rows()
    if c.kind in ("zeros", "equal") and n:
        pick = rng.random(n) < 0.4
        pick[rng.integers(0, n)] = True
        if c.kind == "zeros":
            V[pick] = 0.0
            T[rng.permutation(pick)] = 0.0
            C[pick] = 0.0
        else:
            T[pick | c.all_equal] = V[pick | c.all_equal]
    if c.kind in ("onehot", "saturated"):                                 # N(0, 1) rows: the weights carry the scale
        V, T, C = (rng.standard_normal((n, D)) for _ in range(3))
    lin = lambda *s: rng.uniform(-0.125, 0.125, s)                        # noqa: E731  (nn.Linear's init for 64 inputs)
    w = dict(Wq=lin(D, D), bq=lin(D), q=lin(D), Wv=lin(D, D), bv=lin(D), Wt=lin(D, D), bt=lin(D))
    if c.kind == "onehot":
        w["q"] *= 2000.0                                                  # the two scores differ by hundreds
    if c.kind == "saturated":
        for key in ("Wq", "Wv", "Wt"):
            w[key] *= 400.0                                               # pre-activations in the hundreds
    c.ops = dict(V=V, T=T, C=C, **w)
    c.ops = {key: np.ascontiguousarray(v, np.float32) for key, v in c.ops.items()}
    c.g = [rng.standard_normal((n, D)).astype(np.float32) if c.g_mask >> i & 1 else None for i in range(2)]
    return c


def name_of(c):
    return "case %d (n %d %s%s g %d want %s%s)" % (c.k, c.n, c.kind, " all" if c.all_equal else "", c.g_mask,
                                                  "".join("x" if w else "." for w in c.want), " no ws" if c.null_ws else "")


# ------------------------------------------------------------------------------------------------ the reference and its bound
# a quantity is a pair (float64 value, first-order bound of the kernel's error in it)
def ex(v):
    v = np.asarray(v, np.float64)
    return v, np.zeros_like(v)


def _r(v, e):
    return v, e + U * np.abs(v) + TINY


def t_add(a, b):
    return _r(a[0] + b[0], a[1] + b[1])


def t_sub(a, b):
    return _r(a[0] - b[0], a[1] + b[1])


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
    return A[0] @ B + start[0], A[1] @ np.abs(B) + start[1] + gamma(n) * mag + n * TINY


def t_rowdot(a, b, n=8):
    v = (a[0] * b[0]).sum(axis=1, keepdims=True)
    e = (np.abs(a[0]) * b[1] + np.abs(b[0]) * a[1]).sum(axis=1, keepdims=True)
    return v, e + gamma(n) * (np.abs(a[0]) * np.abs(b[0])).sum(axis=1, keepdims=True) + n * TINY


def t_exp(x):
    v = np.exp(x[0])
    return v, v * (np.expm1(x[1]) + E_EXP * U * np.exp(x[1])) + FLOOR


def t_tanh(z):
    h = np.tanh(z[0])
    dsup = 1.0 - np.tanh(np.maximum(np.abs(z[0]) - z[1], 0.0)) ** 2
    return h, dsup * z[1] + U * ((1.0 - h * h) * E_EXP / 2 + 3 * np.abs(h)) + FLOOR


def _sig(x):
    return np.where(x >= 0, 1.0 / (1.0 + np.exp(-np.abs(x))), np.exp(-np.abs(x)) / (1.0 + np.exp(-np.abs(x))))


def t_sigmoid(z):
    p = _sig(z[0])
    lo = _sig(np.maximum(np.abs(z[0]) - z[1], 0.0))
    return p, lo * (1.0 - lo) * z[1] + U * (p * (1.0 - p) * E_EXP + 2 * p) + FLOOR


def t_colsum(t, n):
    return t[0].sum(axis=0), t[1].sum(axis=0) + gamma(n) * np.abs(t[0]).sum(axis=0) + n * TINY


def t_outer(dz, X, n):
    """sum over rows of dz^T X with X exact, each output one chain of n roundings"""
    return dz[0].T @ X, dz[1].T @ np.abs(X) + gamma(n) * (np.abs(dz[0]).T @ np.abs(X)) + n * TINY


def bounds(ops, g, R=None, F=None):
    """-> {name: (float64 reference, bound)} for the two outputs and the ten gradients"""
    o = {k: f64(v) for k, v in ops.items()}
    V, T, C = o["V"], o["T"], o["C"]
    n = V.shape[0]
    R = rows_per_block(n) if R is None else R
    F = n_finish(n) if F is None else F
    one, three, q = ex(1.0), ex(3.0), ex(o["q"][None, :])
    h, s = {}, {}
    for key, X in (("V", V), ("T", T)):
        h[key] = t_tanh(t_chain(ex(X), o["Wq"].T, ex(o["bq"][None, :]), 64))
        s[key] = t_rowdot(h[key], q)
    mx = (np.maximum(s["V"][0], s["T"][0]), np.maximum(s["V"][1], s["T"][1]))
    eV, eT = t_exp(t_sub(s["V"], mx)), t_exp(t_sub(s["T"], mx))
    den = t_add(eV, eT)
    aV, aT = t_div(eV, den), t_div(eT, den)
    pV = t_sigmoid(t_chain(ex(C), o["Wv"].T, ex(o["bv"][None, :]), 64))
    pT = t_sigmoid(t_chain(ex(C), o["Wt"].T, ex(o["bt"][None, :]), 64))
    m = t_fma(aT, ex(T), t_mul(aV, ex(V)))
    xV, xT = t_sub(ex(V), m), t_sub(ex(T), m)
    side = t_div(t_fma(pT, xT, t_fma(pV, xV, m)), three)
    out = {"side": side, "out": t_add(ex(C), side)}
    zero = np.zeros((n, D))
    go = ex(zero if g[1] is None else f64(g[1]))
    G = go if g[0] is None else ex(f64(g[0])) if g[1] is None else t_add(ex(f64(g[0])), go)
    G3 = t_div(G, three)
    dm = t_mul(G3, t_sub(t_sub(one, pV), pT))
    dsV = t_mul(t_mul(aV, aT), t_rowdot(dm, t_sub(ex(V), ex(T))))
    dsT = t_neg(dsV)
    dzV = t_mul(t_mul(dsV, q), t_fma(t_neg(h["V"]), h["V"], one))
    dzT = t_mul(t_mul(dsT, q), t_fma(t_neg(h["T"]), h["T"], one))
    duV = t_mul(t_mul(G3, xV), t_mul(pV, t_sub(one, pV)))
    duT = t_mul(t_mul(G3, xT), t_mul(pT, t_sub(one, pT)))
    out["dV"] = t_chain(dzV, o["Wq"], t_fma(aV, dm, t_mul(G3, pV)), 64)
    out["dT"] = t_chain(dzT, o["Wq"], t_fma(aT, dm, t_mul(G3, pT)), 64)
    dc1 = t_chain(duV, o["Wv"], go, 128)
    dc2 = t_chain(duT, o["Wt"], ex(zero), 128)
    out["dC"] = (dc1[0] + dc2[0], dc1[1] + dc2[1])
    a, b = t_outer(dzV, V, 2 * R + F), t_outer(dzT, T, 2 * R + F)
    out["dWq"] = (a[0] + b[0], a[1] + b[1])
    out["dWv"], out["dWt"] = t_outer(duV, C, R + F), t_outer(duT, C, R + F)
    n_col = R // 16 + 16 + F
    out["dbq"] = t_colsum(t_add(dzV, dzT), n_col)
    out["dbv"], out["dbt"] = t_colsum(duV, n_col), t_colsum(duT, n_col)
    out["dq"] = t_colsum(t_fma(dsT, h["T"], t_mul(dsV, h["V"])), n_col)
    return {k: (v, SLACK * e) for k, (v, e) in out.items()}


def check(ops, g, got, name, R=None, F=None):
    """got: {name: array or tensor} of any subset of the outputs -> the worst err / bound per family"""
    b = bounds(ops, g, R, F)
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
    assert {c.g_mask for c in cs} == {0, 1, 2, 3} and {c.kind for c in cs} == set(KINDS)
    for kind in KINDS:
        assert {c.g_mask for c in cs if c.kind == kind} == {0, 1, 2, 3}, kind
        assert {c.n for c in cs if c.kind == kind} >= set(ns) - {ns[5 % len(ns)]}, kind
    for i in range(10):                                                   # every output wanted somewhere, and not wanted
        assert {c.want[i] for c in cs} == {True, False}, GRADS[i]
    assert any(all(c.want) for c in cs) and any(not any(c.want[3:]) for c in cs)
    assert {c.null_ws for c in cs} == {True, False} and all(not c.null_ws or not any(c.want[3:]) for c in cs)
    assert any(c.all_equal and c.n > 64 and c.want[3] and c.g_mask for c in cs)
    big = cs[5]
    assert big.n == BIG and all(big.want) and big.g_mask == 3 and big.kind == "mixed"
    for c in cs:
        if c.n < 60:
            continue
        V, T, q = c.ops["V"], c.ops["T"], c.ops["q"]
        mags = np.abs(V).max(axis=1)
        if c.kind == "mixed":
            assert (mags > 100).any() and (mags < 0.1).any() and ((mags > 0.5) & (mags < 10)).any()
        if c.kind == "zeros":
            assert (mags == 0).any() and (np.abs(c.ops["C"]).max(axis=1) == 0).any()
        if c.kind == "equal":
            same = (V == T).all(axis=1)
            assert same.any() and (same.all() == c.all_equal)
        z = lambda X, W, b: f64(X) @ f64(c.ops[W]).T + f64(c.ops[b])       # noqa: E731
        if c.kind == "onehot":
            s = np.tanh(z(V, "Wq", "bq")) @ f64(q) - np.tanh(z(T, "Wq", "bq")) @ f64(q)
            assert (np.abs(s) > 200).any() and np.isfinite(s).all()
        if c.kind == "saturated":
            for zz in (z(V, "Wq", "bq"), z(c.ops["C"], "Wv", "bv")):
                assert np.median(np.abs(zz)) > 100
                assert (np.tanh(zz).astype(np.float32) ** 2 == 1.0).mean() > 0.9      # the derivative factor is exactly 0


# ------------------------------------------------------------------------------------------------ GPU: the raw C ABI, guarded
def _workspace(n):
    nbytes = int(_lib().mmrec_modal_fusion_workspace_bytes(n))
    assert nbytes == blocks(n) * PART * 4 and blocks(n) <= MAX_BLOCKS
    return torch.full((nbytes // 4 + GUARD,), SENTINEL, dtype=torch.int32, device="cuda:0"), nbytes // 4


def run_case(c):
    """the case's forward and backward through the raw ABI -> {name: tensor} of every output written"""
    from mmrec_amd import hip_ops
    p_, lib, name = hip_ops._p, _lib(), name_of(c)
    ops = [_on(c.ops[k]) for k in OPERANDS]
    g = [None if t is None else _on(t) for t in c.g]
    shapes = {"side": (c.n, D), "out": (c.n, D)}
    held, ptr = _outs(shapes)
    rc = lib.mmrec_modal_fusion_fwd_f32(*[p_(t) for t in ops], c.n, D, ptr["side"], ptr["out"], hip_ops._stream())
    assert rc == 0, (name, rc)
    out = _collect(held, shapes, name) if c.n else {}
    shapes = {k: _shape(c, k) if w else None for k, w in zip(GRADS, c.want)}
    held, ptr = _outs(shapes)
    ws, n_ws = (None, 0) if c.null_ws else _workspace(c.n)
    rc = lib.mmrec_modal_fusion_bwd_f32(*[p_(t) for t in ops], p_(g[0]), p_(g[1]), c.n, D, *[ptr[k] for k in GRADS], p_(ws),
                                        hip_ops._stream())
    assert rc == 0, (name, rc)
    if c.n:
        out.update(_collect(held, shapes, name))
    else:
        torch.cuda.synchronize()
        for buf, view in held.values():                                   # n = 0: no launch, nothing is written
            assert bool((buf == SENTINEL).all()), name
    if ws is not None:
        assert bool((ws[n_ws:] == SENTINEL).all()), (name, "wrote beyond the workspace")
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("k", range(CASES))
def test_modal_fusion_fuzz(k):
    c = case(k)
    name = name_of(c)
    got = run_case(c)
    worst = check(c.ops, c.g, got, name) if c.n else {}
    print("%s: worst err / bound %s" % (name, " ".join("%s %.3f" % kv for kv in sorted(worst.items()))))
    if c.n:
        assert set(got) == {"side", "out"} | {k_ for k_, w in zip(GRADS, c.want) if w}, name
    if c.g_mask == 0:
        for k_ in GRADS:
            if k_ in got:
                assert not bool(got[k_].any()), (name, k_, "a gradient without any g is zeros")
    if c.all_equal:
        for k_ in ("dWq", "dbq", "dq"):
            if k_ in got:
                assert not bool(got[k_].any()), (name, k_, "rows with V == T give the attention's parameters exactly nothing")
    again = run_case(c)                                                   # the same calls again: the same bits
    assert got.keys() == again.keys()
    for k_ in got:
        assert torch.equal(_bits(got[k_]), _bits(again[k_])), (name, k_, "not repeatable")


@pytest.mark.gpu
def test_saturation_is_exact_and_never_a_nan():
    """|z| in the hundreds and beyond: h is exactly +-1, p exactly 1 or 0, their derivative factors exactly 0 -- with V = T = C one
    row of +-1000 and identity-like weights every pre-activation is +-1000 (the softmax ties: aV = aT = 0.5, m = V)"""
    from mmrec_amd import hip_ops
    p_, lib = hip_ops._p, _lib()
    n = 70
    sign = np.where(np.arange(D) % 2 == 0, 1.0, -1.0).astype(np.float32)
    X = np.tile(1000.0 * sign, (n, 1)).astype(np.float32)
    eye, zero = np.eye(D, dtype=np.float32), np.zeros(D, np.float32)
    ops = [_on(a) for a in (X, X, X, eye, zero, np.ones(D, np.float32), eye, zero, eye, zero)]
    g = _on(np.ones((n, D), np.float32))
    shapes = {"side": (n, D), "out": (n, D)}
    held, ptr = _outs(shapes)
    assert lib.mmrec_modal_fusion_fwd_f32(*[p_(t) for t in ops], n, D, ptr["side"], ptr["out"], hip_ops._stream()) == 0
    out = _collect(held, shapes, "saturated")
    # m = V, so side = (pV 0 + pT 0 + V) / 3 whatever p is -- finite, no NaN from 0 * anything
    assert torch.equal(out["side"].cpu(), torch.from_numpy(X / np.float32(3.0)))
    shapes = {k: ((n, D) if k in ("dV", "dT", "dC") else (D, D) if "W" in k else (D,)) for k in GRADS}
    held, ptr = _outs(shapes)
    ws, _ = _workspace(n)
    assert lib.mmrec_modal_fusion_bwd_f32(*[p_(t) for t in ops], p_(g), None, n, D, *[ptr[k] for k in GRADS], p_(ws),
                                          hip_ops._stream()) == 0
    got = _collect(held, shapes, "saturated")
    for k, t in got.items():
        assert bool(torch.isfinite(t).all()), k
    for k in ("dWq", "dbq", "dq", "dWv", "dbv", "dWt", "dbt", "dC"):       # 1 - h^2 = 0, p (1 - p) = 0, V - T = 0, g_out NULL
        assert not bool(got[k].any()), k
    # dV = G3 pV + aV dm with G3 = 1 / 3, p = 1 (z = 1000) or 0 (z = -1000), dm = G3 (1 - 2 p), a = 0.5
    third = np.float32(1.0) / np.float32(3.0)
    p = (sign > 0).astype(np.float32)
    want = (third * p + np.float32(0.5) * (third * ((1 - p) - p))).astype(np.float32)
    assert torch.equal(got["dV"].cpu(), torch.from_numpy(np.tile(want, (n, 1))))
    assert torch.equal(_bits(got["dV"]), _bits(got["dT"]))


@pytest.mark.gpu
def test_wrapper_autograd_takes_the_kernels_and_honours_needs_input_grad():
    """hip_ops.modal_fusion with only one output used and only some operands requiring gradients: the library is given NULL for
    the rest, the results meet the raw ABI's bounds, and an unserved call is the torch composition bit for bit"""
    from mmrec_amd import hip_ops
    c = case(20)
    assert c.n > 2 * 64
    lib = _lib()
    seen = []
    real_b = lib.mmrec_modal_fusion_bwd_f32
    needs = dict(V=True, T=False, C=True, Wq=True, bq=False, q=True, Wv=False, bv=True, Wt=False, bt=False)
    ops = [_on(c.ops[k].reshape(1, D) if k == "q" else c.ops[k]).requires_grad_(needs[k]) for k in OPERANDS]
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(lib, "mmrec_modal_fusion_bwd_f32", lambda *a: seen.append(a) or real_b(*a))
        assert hip_ops.modal_fusion_served(*ops)
        side, out = hip_ops.modal_fusion(*ops)
        (2 * out.sum()).backward()
        torch.cuda.synchronize()
    assert len(seen) == 1
    a = seen[0]
    assert a[10] is None and a[11] is not None                            # g_side never arrived
    assert [x is not None for x in a[14:24]] == [needs[k] for k in OPERANDS] and a[24] is not None
    got = {"side": side.detach(), "out": out.detach()}
    got.update({"d" + k: t.grad.reshape(c.ops[k].shape) for k, t in zip(OPERANDS, ops) if needs[k]})
    assert all(t.grad is None for k, t in zip(OPERANDS, ops) if not needs[k])
    print("wrapper: worst err / bound", check(c.ops, [None, 2 * np.ones((c.n, D), np.float32)], got, "wrapper"))
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(hip_ops, "MODAL_FUSION", False)
        assert not hip_ops.modal_fusion_served(*ops)
        off = hip_ops.modal_fusion(*ops)
    ref = hip_ops.modal_fusion_torch(*ops)
    assert all(torch.equal(_bits(a_.detach()), _bits(b_.detach())) for a_, b_ in zip(off, ref))
    assert not hip_ops.modal_fusion_served(ops[0][:, ::2], *ops[1:]) and not hip_ops.modal_fusion_served(ops[0].cpu(), *ops[1:])
