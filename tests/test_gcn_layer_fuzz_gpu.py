"""GPU: seeded differential fuzz of MMGCN's 64-wide layer kernels (csrc/gcn_layer.hip: mmrec_gcn_layer_fwd_f32 / _bwd_f32) against
float64 numpy of the formulas of include/mmrec_hip.h, computed from the fp32 arrays each call was given -- never against another
kernel or the torch composition.  The raw C ABI is called over guarded, sentinel-filled outputs and a sentinel-filled workspace
of exactly the reported size; the backward is given the forward's own `out`, as autograd gives it.

    a = AX Wc, h = leaky(a);  p = X Wl^T + bl, xh = leaky(p) + R;  q = h Gh^T + xh Gx^T + bg;  out = leaky(q)     (Wg = [Gh | Gx])
    dq = g leaky'(q), dh = dq Gh, da = dh leaky'(a), dxh = dq Gx = dR, dp = dxh leaky'(p), dAX = da Wc^T, dX = dp Wl,
    dWc = AX^T da, dWl = dp^T X, dWg = [dq^T h | dq^T xh], dbl = colsum(dp), dbg = colsum(dq)

ACCEPTANCE: |got - ref| <= (1 + 2^-10) e, with e a first-order bound that is carried along the float64 evaluation, operation by
operation as the PLAN of include/mmrec_hip.h names them (u = 2^-24, gamma(n) = n u / (1 - n u), 2^-149 per rounding for
underflow, none where the operands are exact and the result is an exact zero) -- the scheme, constants and helpers of
tests/test_encoder_heads_fuzz_gpu.py, derived from the header's text, not tuned to a result:
    a, p, dh, dxh, dAX, dX           a chain of 64 fma from a start (0, or bl): e = e_A |B| + e_start + gamma(64) (|A| |B| + |start|)
    q                                ONE chain of 128 fma from bg: e = e_h |Gh| + e_xh |Gx| + gamma(128) (|h| |Gh| + |xh| |Gx| + |bg|)
    leaky(z)                         the largest slope on [z - e, z + e] times e, + u |value|;  xh: one more addition
    leaky'(z)                        1 or slope by the reference's sign (0 takes slope).  Where the bound cannot decide the sign
                                     (|z| <= e and e > 0: with e == 0 the kernel's z IS the reference's) the kernel may take the
                                     other factor: the entry's gradient bound is WIDENED by (1 - slope) |incoming| (incoming: g
                                     for q, dh for a, dxh for p), never excluded; tests/test_gcn_layer_cpu.py caps the share of
                                     such entries at 2e-4.  The kernel reads q's sign from its own out: the same rule.
    weight gradients                 one fma chain over the R rows of a block (R from the library), then the finish,
                                     F = ceil(blocks / 4) + 3: gamma(R + F);  dbl, dbg: R / 16 + 16 + F additions
The worst err / bound per family (out;  dx: dAX, dX, dR;  dw: dWc, dWl, dWg;  db: dbl, dbg) is printed by every case and recorded
in EXPERIMENTS.md section 4.
EXACTNESS, every case: the same calls again give the same bits; guards and sentinels intact; with g zero every gradient is zero;
d = 32 and slope = 0 are MMREC_ERR_UNSUPPORTED and n = 0 is 0, and none of them touches an output or the workspace.
`test_cases_span_every_axis` and the checker's own tests (an fp32 emulation of the plan passes, planted errors do not,
the kink cap) are in tests/test_gcn_layer_cpu.py."""
import numpy as np
import pytest
import torch

from tests.test_encoder_heads_fuzz_gpu import (SLACK, TINY, ex, t_add, t_chain, t_colsum, t_leaky, t_mul, t_outer, undecided)
from tests.test_hyper_fuzz_gpu import _bits, _collect, _lib, _outs, compare, f64
from tests.test_edge_softmax_fuzz_gpu import GUARD, SENTINEL
from tests.test_spmm_fuzz_gpu import _on, gamma

D = 64
PART = 4 * D * D + 2 * D                       # floats of one block's partial
MAX_BLOCKS = 256
BIG = 20011                                    # 157 blocks of two tiles: every thread of the finish adds 39 or 40 partials
CASES = 36
KINDS = ("mixed", "zero_ax", "zero_x")
SLOPE = 0.01
UNSUPPORTED = 10002
OPERANDS = ("AX", "X", "R", "Wc", "Wl", "bl", "Wg", "bg")
GRADS = ("dAX", "dX", "dR", "dWc", "dWl", "dbl", "dWg", "dbg")
FAMILY = dict(out="out", dAX="dx", dX="dx", dR="dx", dWc="dw", dWl="dw", dWg="dw", dbl="db", dbg="db")


def rows_per_block(n):
    return int(_lib().mmrec_gcn_layer_rows_per_block(int(n)))


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
    return ((c.n, D) if name in ("out", "dAX", "dX", "dR") else (D, D) if name in ("dWc", "dWl") else (D, 2 * D) if name == "dWg"
            else (D,))


def case(k):
    ns = axis_n()
    c = Case()
    c.k = k
    c.n = n = BIG if k == 5 else ns[k % len(ns)]
    c.kind = "mixed" if k == 5 else KINDS[k % 3]
    c.r_null = k != 5 and (k // 3) % 2 == 1
    c.g_zero = k % 9 == 4
    rng = np.random.default_rng(9100 + k)
    want = rng.random(8) < 0.6
    if k % 6 == 5:
        want[:] = True
    if k % 6 == 2:
        want[3:] = False                                                  # no weight gradient: the finish is not launched
    if k % 12 == 8:
        want[:] = False                                                   # nothing wanted at all: no launch
    c.want = tuple(bool(w) for w in want)
    c.null_ws = not any(c.want[3:]) and k % 4 != 0
    rows = lambda: rng.standard_normal((n, D)) * rng.choice([1.0, 1e-3, 1e3], size=(n, 1), p=[0.6, 0.2, 0.2])     # noqa: E731
    AX, X, R = rows(), rows(), rows()
    lin = lambda *s: rng.uniform(-0.125, 0.125, s)                        # noqa: E731  (nn.Linear's init for 64 inputs)
    w = dict(Wc=lin(D, D), Wl=lin(D, D), bl=lin(D), Wg=lin(D, 2 * D), bg=lin(D))
    c.zero_rows = np.zeros(n, bool)
    if c.kind != "mixed" and n:
        pick = rng.random(n) < 0.3
        pick[rng.integers(0, n)] = True
        c.zero_rows = pick
        if c.kind == "zero_ax":
            AX[pick] = 0.0                                                # a = 0 exactly: leaky' at 0 is the slope
        if c.kind == "zero_x":
            X[pick] = 0.0
            w["bl"][:] = 0.0                                              # p = 0 exactly
    c.ops = {key: np.ascontiguousarray(v, np.float32) for key, v in dict(AX=AX, X=X, R=R, **w).items()}
    if c.r_null:
        c.ops["R"] = None
    c.g = np.zeros((n, D), np.float32) if c.g_zero else rng.standard_normal((n, D)).astype(np.float32)
    return c


def name_of(c):
    return "case %d (n %d %s R %s%s want %s%s)" % (c.k, c.n, c.kind, "null" if c.r_null else "given", " g0" if c.g_zero else "",
                                                   "".join("x" if w else "." for w in c.want), " no ws" if c.null_ws else "")


# ------------------------------------------------------------------------------------------------ the reference and its bound
def t_chain2(A1, B1, A2, B2, start):
    """ONE chain of 128 fma from `start`: the 64 terms of A1 B1, then the 64 terms of A2 B2 (B exact)"""
    mag = np.abs(A1[0]) @ np.abs(B1) + np.abs(A2[0]) @ np.abs(B2) + np.abs(start[0])
    e = A1[1] @ np.abs(B1) + A2[1] @ np.abs(B2) + start[1]
    return A1[0] @ B1 + A2[0] @ B2 + start[0], e + gamma(128) * mag + np.where((mag == 0) & (e == 0), 0.0, 128 * TINY)


def _dleaky(z, incoming, s):
    """incoming * leaky'(z): one rounding, widened where z's sign is undecided -> (the product, the undecided entries)"""
    und = undecided(z)
    d = t_mul(incoming, ex(np.where(z[0] > 0, 1.0, s)))
    return (d[0], d[1] + und * (1.0 - s) * (np.abs(incoming[0]) + incoming[1])), und


def bounds(ops, g, slope=SLOPE, R=None, F=None, info=None):
    """-> {name: (float64 reference, bound)} for out and the eight gradients; `info`: a dict that receives the undecided entries
    of a, p and q"""
    o = {k: f64(v) for k, v in ops.items()}
    AX, X = o["AX"], o["X"]
    n = AX.shape[0]
    R = rows_per_block(n) if R is None else R
    F = n_finish(n) if F is None else F
    s = float(np.float32(slope))
    n_col = R // 16 + 16 + F
    Gh, Gx = o["Wg"][:, :D], o["Wg"][:, D:]
    zero = ex(np.zeros((n, D)))
    a = t_chain(ex(AX), o["Wc"], zero, 64)
    h = t_leaky(a, s)
    p = t_chain(ex(X), o["Wl"].T, ex(o["bl"][None, :]), 64)
    xh = t_leaky(p, s)
    if o["R"] is not None:
        xh = t_add(xh, ex(o["R"]))
    q = t_chain2(h, Gh.T, xh, Gx.T, ex(o["bg"][None, :]))
    res = {"out": t_leaky(q, s)}
    dq, und_q = _dleaky(q, ex(f64(g)), s)
    dh = t_chain(dq, Gh, zero, 64)
    da, und_a = _dleaky(a, dh, s)
    dxh = t_chain(dq, Gx, zero, 64)
    dp, und_p = _dleaky(p, dxh, s)
    res["dR"] = dxh
    res["dAX"] = t_chain(da, o["Wc"].T, zero, 64)
    res["dX"] = t_chain(dp, o["Wl"], zero, 64)
    res["dWc"] = t_outer(ex(AX), da, R + F)
    res["dWl"] = t_outer(dp, ex(X), R + F)
    wh, wx = t_outer(dq, h, R + F), t_outer(dq, xh, R + F)
    res["dWg"] = (np.concatenate([wh[0], wx[0]], axis=1), np.concatenate([wh[1], wx[1]], axis=1))
    res["dbl"] = t_colsum(dp, n_col)
    res["dbg"] = t_colsum(dq, n_col)
    if info is not None:
        info.update(und_a=und_a, und_p=und_p, und_q=und_q, a=a, p=p, q=q)
    return {k: (v, SLACK * e) for k, (v, e) in res.items()}


def check(ops, g, got, name, slope=SLOPE, R=None, F=None):
    """got: {name: array or tensor} of any subset of the outputs -> the worst err / bound per family"""
    b = bounds(ops, g, slope, R, F)
    worst = {}
    for k, v in got.items():
        v = v.reshape(b[k][0].shape) if hasattr(v, "reshape") else v
        worst[FAMILY[k]] = max(worst.get(FAMILY[k], 0.0), compare(v, *b[k], name + " " + k))
    return worst


# ------------------------------------------------------------------------------------------------ no GPU: the axes
def cases_span_every_axis():
    """run by tests/test_gcn_layer_cpu.py::test_cases_span_every_axis"""
    cs = [case(k) for k in range(CASES)]
    ns = axis_n()
    r = rows_per_block(1)
    assert r == 64 and rows_per_block(BIG) == 128 and blocks(BIG) == 157 and n_finish(BIG) == 43
    assert {0, 1, 2, 63, 64, 65, r - 1, r, r + 1, 2 * r + 1} <= set(ns)
    assert set(ns) | {BIG} == {c.n for c in cs}
    assert {c.kind for c in cs} == set(KINDS) and {c.r_null for c in cs} == {True, False}
    for kind in KINDS:
        sub = [c for c in cs if c.kind == kind and c.n]
        assert {c.r_null for c in sub} == {True, False}, kind
        assert len({c.n for c in sub}) >= 5 and max(c.n for c in sub) > 64, kind
    for null in (True, False):
        assert {c.n for c in cs if c.r_null == null and c.n} >= set(ns) - {0}
    for i in range(8):                                                    # every output wanted somewhere, and not wanted
        assert {c.want[i] for c in cs if c.n} == {True, False}, GRADS[i]
    assert any(all(c.want) and c.n > 64 for c in cs) and any(not any(c.want[3:]) and any(c.want[:3]) and c.n for c in cs)
    assert any(not any(c.want) and c.n for c in cs)
    assert {c.null_ws for c in cs} == {True, False} and all(not c.null_ws or not any(c.want[3:]) for c in cs)
    assert any(c.g_zero and c.n > 64 and any(c.want[3:]) for c in cs)
    big = cs[5]
    assert big.n == BIG and all(big.want) and big.kind == "mixed" and not big.r_null and not big.g_zero
    for c in cs:
        assert (c.ops["R"] is None) == c.r_null
        if c.n < 60:
            continue
        mags = np.abs(c.ops["AX"]).max(axis=1)
        if c.kind == "mixed":
            assert (mags > 100).any() and (mags < 0.1).any() and ((mags > 0.5) & (mags < 10)).any()
        if c.kind == "zero_ax":
            assert (mags == 0).any() and (mags[c.zero_rows] == 0).all()
        if c.kind == "zero_x":
            assert (np.abs(c.ops["X"]).max(axis=1)[c.zero_rows] == 0).all() and not c.ops["bl"].any()


# ------------------------------------------------------------------------------------------------ GPU: the raw C ABI, guarded
def _workspace(n):
    nbytes = int(_lib().mmrec_gcn_layer_workspace_bytes(n))
    assert nbytes == blocks(n) * PART * 4 and blocks(n) <= MAX_BLOCKS
    return torch.full((nbytes // 4 + GUARD,), SENTINEL, dtype=torch.int32, device="cuda:0"), nbytes // 4


def _untouched(bufs, name):
    torch.cuda.synchronize()
    for buf in bufs:
        assert bool((buf == SENTINEL).all()), name


def run_case(c):
    """the case's forward and backward through the raw ABI -> {name: tensor} of every output written.  Before each real call the
    refused ones (d = 32, slope = 0) and the empty one (n = 0) on the same pointers: they return their codes and write nothing."""
    from mmrec_amd import hip_ops
    p_, lib, name = hip_ops._p, _lib(), name_of(c)
    ops = [None if c.ops[k] is None else _on(c.ops[k]) for k in OPERANDS]
    g = _on(c.g)
    st = hip_ops._stream()
    shapes = {"out": _shape(c, "out")}
    held, ptr = _outs(shapes)
    fw = lambda n, d, slope: lib.mmrec_gcn_layer_fwd_f32(*[p_(t) for t in ops], n, d, slope, ptr["out"], st)      # noqa: E731
    assert fw(c.n, 32, SLOPE) == UNSUPPORTED and fw(c.n, D, 0.0) == UNSUPPORTED and fw(0, D, SLOPE) == 0, name
    _untouched([buf for buf, _ in held.values()], name + " a refused forward wrote")
    assert fw(c.n, D, SLOPE) == 0, name
    out = _collect(held, shapes, name) if c.n else {}
    fwd_held = [buf for buf, _ in held.values()]
    out_dev = out["out"] if c.n else torch.zeros((0, D), device="cuda:0")
    shapes = {k: _shape(c, k) if w else None for k, w in zip(GRADS, c.want)}
    held, ptr = _outs(shapes)
    ws, n_ws = (None, 0) if c.null_ws else _workspace(c.n)
    bw = lambda n, d, slope: lib.mmrec_gcn_layer_bwd_f32(*[p_(t) for t in ops], p_(out_dev), p_(g), n, d, slope,  # noqa: E731
                                                         *[ptr[k] for k in GRADS], p_(ws), st)
    assert bw(c.n, 32, SLOPE) == UNSUPPORTED and bw(c.n, D, 0.0) == UNSUPPORTED and bw(0, D, SLOPE) == 0, name
    _untouched([buf for buf, _ in held.values()] + ([] if ws is None else [ws]), name + " a refused backward wrote")
    assert bw(c.n, D, SLOPE) == 0, name
    if c.n:
        out.update(_collect(held, shapes, name))
    else:
        _untouched(fwd_held + [buf for buf, _ in held.values()], name + " an empty call wrote")
    if ws is not None:
        torch.cuda.synchronize()
        assert bool((ws[n_ws:] == SENTINEL).all()), (name, "wrote beyond the workspace")
        if not any(c.want[3:]):
            assert bool((ws == SENTINEL).all()), (name, "no weight gradient wanted, yet the workspace was written")
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("k", range(CASES))
def test_gcn_layer_fuzz(k):
    c = case(k)
    name = name_of(c)
    got = run_case(c)
    worst = check(c.ops, c.g, got, name) if c.n else {}
    print("%s: worst err / bound %s" % (name, " ".join("%s %.3f" % kv for kv in sorted(worst.items()))))
    if c.n:
        assert set(got) == {"out"} | {k_ for k_, w in zip(GRADS, c.want) if w}, name
    else:
        assert got == {}
    if c.g_zero:
        for k_ in GRADS:
            if k_ in got:
                assert not bool(got[k_].any()), (name, k_, "a gradient of g = 0 is zeros")
    again = run_case(c)                                                   # the same calls again: the same bits
    assert got.keys() == again.keys()
    for k_ in got:
        assert torch.equal(_bits(got[k_]), _bits(again[k_])), (name, k_, "not repeatable")


@pytest.mark.gpu
def test_wrapper_autograd_takes_the_kernels_and_honours_needs_input_grad():
    """hip_ops.gcn_layer with only some operands requiring gradients: the library is given NULL for the rest, the results meet
    the raw ABI's bounds, and an unserved call is the torch composition bit for bit"""
    from mmrec_amd import hip_ops
    c = case(6)
    assert c.n > 2 * 64 and not c.r_null and not c.g_zero
    lib = _lib()
    seen = []
    real_b = lib.mmrec_gcn_layer_bwd_f32
    needs = dict(AX=True, X=False, R=False, Wc=True, Wl=False, bl=False, Wg=False, bg=True)
    ops = [_on(c.ops[k]).requires_grad_(needs[k]) for k in OPERANDS]
    g = _on(c.g)
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(lib, "mmrec_gcn_layer_bwd_f32", lambda *a: seen.append(a) or real_b(*a))
        assert hip_ops.gcn_layer_served(*ops)
        out = hip_ops.gcn_layer(*ops)
        (out * g).sum().backward()
        torch.cuda.synchronize()
    assert len(seen) == 1
    a = seen[0]
    assert [x is not None for x in a[13:21]] == [needs[k] for k in OPERANDS] and a[21] is not None
    got = {"out": out.detach()}
    got.update({"d" + k: t.grad for k, t in zip(OPERANDS, ops) if needs[k]})
    assert all(t.grad is None for k, t in zip(OPERANDS, ops) if not needs[k])
    print("wrapper: worst err / bound", check(c.ops, c.g, got, "wrapper"))
    no_r = list(ops)
    no_r[2] = None
    assert hip_ops.gcn_layer_served(*no_r)
    got = hip_ops.gcn_layer(*no_r)
    print("wrapper, R None: worst err / bound", check(dict(c.ops, R=None), c.g, {"out": got.detach()}, "wrapper R None"))
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(hip_ops, "GCN_LAYER", False)
        assert not hip_ops.gcn_layer_served(*ops)
        off = hip_ops.gcn_layer(*ops)
    ref = hip_ops.gcn_layer_torch(*ops)
    assert torch.equal(_bits(off.detach()), _bits(ref.detach()))
    assert not hip_ops.gcn_layer_served(ops[0][:, ::2], *ops[1:]) and not hip_ops.gcn_layer_served(ops[0].cpu(), *ops[1:])
    assert not hip_ops.gcn_layer_served(*ops, slope=0.0)
