"""GPU: seeded differential fuzz of SMORE's spectrum kernels (csrc/spectrum.hip: mmrec_spectrum_fwd_f32 / _bwd_f32) against float64
numpy computed from the fp32 arrays each call was given, never against another kernel or against fp32 DFT matrices.  The raw C ABI
is called over guarded, sentinel-filled outputs and a sentinel-filled workspace.

    forward reference   np.fft.rfft / irfft (norm='ortho'):  irfft(rfft(x) w_img), irfft(rfft(y) w_txt), irfft(rfft(y) rfft(x) w_fus)
    backward reference  the closed forms with float64 matrices C, S (rfft = x C + i x S) and Ci, Si (irfft = P Ci + Q Si), per filter
        dP = g Ci^T, dQ = g Si^T;  dwr = sum_rows (dP p + dQ q), dwi = sum_rows (-dP q + dQ p);  dp = dP wr + dQ wi, dq = -dP wi + dQ wr
        image: da += dp, db += dq;  text: dc += dp, de += dq;  fusion: da += dp c + dq e, db += -dp e + dq c, dc += dp a + dq b,
        de += -dp b + dq a;  dx = da C^T + db S^T, dy = dc C^T + de S^T          (`terms64`; a NULL g is zeros)

Acceptance: |got - ref| <= (1 + 2^-10) gamma(n) MAG + n 2^-149 with u = 2^-24, gamma(n) = n u / (1 - n u), MAG the same formula in
float64 over absolute values (|x| |C|, |w|, |Ci| ..., every subtraction an addition: `terms64(absolute=True)`), and n the longest
chain of roundings a term of the output meets in the kernel's plan AS WRITTEN IN include/mmrec_hip.h -- derived from the plan, not
tuned to the result.  A product with a DFT matrix is one fma chain of 64 terms, plus two for the fp32 twiddle: S = 66.  A filter
expression (p wr - q wi, the fusion product c a - e b, dp c + dq e onto dp1 ...) is a multiply and an fma: 2.
    out_img, out_txt   S + 2 + S = 134                       out_fus   (S + S) + 2 + 2 + S = 202     (p3 is a product of two spectra)
    dx, dy             the longest term is dp3 c:  (S + 2) + S + 2, then the last product:  3 S + 4 = 202
    dw_img, dw_txt     S + S + 2 = 134, dw_fus S + (2 S + 2) + 2 = 202 for a row's term; then `n_red(n)`: R / 64 additions over a
                       block's tiles, 6 of the wave's butterfly, ceil(blocks / 64) + 6 in the finish (R, blocks from the library)
The worst err / bound per family is printed by every case and recorded in EXPERIMENTS.md section 4.
Exactness, every case: the gradients of the imaginary weights of bins 0 and 32 are 0.0; with those weights replaced by NaN no
output bit changes; the same calls again give the same bits.  `test_cases_span_every_axis` needs no GPU; the checker's own tests
(an fp32 emulation of the plan passes, planted errors do not) are in tests/test_spectrum_cpu.py."""
import numpy as np
import pytest
import torch

from tests.test_hyper_fuzz_gpu import _bits, _collect, _lib, _outs, compare, f64
from tests.test_edge_softmax_fuzz_gpu import GUARD, SENTINEL
from tests.test_spmm_fuzz_gpu import _on, gamma

D, BINS = 64, 33
S_STAGE = 66
N_OUT = {"out_img": 2 * S_STAGE + 2, "out_txt": 2 * S_STAGE + 2, "out_fus": 3 * S_STAGE + 4}
N_DX = 3 * S_STAGE + 4
N_DW_TERM = {"dw_img": 2 * S_STAGE + 2, "dw_txt": 2 * S_STAGE + 2, "dw_fus": 3 * S_STAGE + 4}
BIG = 20011                                    # 313 blocks: every lane of the finish adds several partials
TWO_TILES = 65601                              # above 65,536 rows a block walks two tiles
CASES = 40
KINDS = ("mixed", "zeros", "impulse", "constant")
SLACK = 1.0 + 2.0 ** -10
TINY = 2.0 ** -149
BAD_ARG, UNSUPPORTED = 10001, 10002
FWD_NAMES = ("out_img", "out_txt", "out_fus")
DW_NAMES = ("dw_img", "dw_txt", "dw_fus")


def rows_per_block(n):
    return int(_lib().mmrec_spectrum_rows_per_block(int(n)))


def blocks(n):
    return -(-n // rows_per_block(n)) if n > 0 else 0


def n_red(n):
    """the additions a row's term of a weight gradient meets: the block's tiles, the wave's butterfly, the finish"""
    return rows_per_block(n) // 64 + 6 + -(-blocks(n) // 64) + 6


def axis_n():
    r = rows_per_block(1)
    return tuple(sorted({0, 1, 2, 15, 16, 17, 63, 64, 65, r - 1, r, r + 1, 2 * r + 1}))


class Case:
    pass


def _rows(rng, n, kind):
    t = rng.standard_normal((n, D)) * rng.choice([1.0, 1e-3, 1e3], size=(n, 1), p=[0.6, 0.2, 0.2])
    if kind != "mixed" and n:
        pick = rng.random(n) < 0.4
        pick[rng.integers(0, n)] = True
        m = int(pick.sum())
        if kind == "constant":
            t[pick] = rng.standard_normal((m, 1))                         # DC only
        else:
            t[pick] = 0.0
            if kind == "impulse":
                t[np.flatnonzero(pick), rng.integers(0, D, m)] = rng.standard_normal(m)
    return np.ascontiguousarray(t, np.float32)


def case(k):
    ns = axis_n()
    c = Case()
    c.k = k
    c.n = BIG if k == 5 else TWO_TILES if k == 17 else ns[k % len(ns)]
    c.kind = KINDS[k % 4]
    c.identity = k % 5 == 0                                               # w = (1, 0) in every bin: image_conv is x
    c.g_mask = 1 + k % 7                                                  # bit i: g_i is given
    c.out_mask = (3 * k + k // 8) % 8                                     # bit 0: dx, 1: dy, 2: the weight gradients wanted
    c.dw_mask = 7 if k % 4 == 3 else 1 + (k // 2) % 7                     # which of the three, where they are wanted
    c.null_ws = not (c.out_mask & 4) and k % 2 == 1
    rng = np.random.default_rng(9000 + k)
    c.x, c.y = _rows(rng, c.n, c.kind), _rows(rng, c.n, c.kind)
    c.w = rng.standard_normal((3, BINS, 2)).astype(np.float32)            # the model's init
    if c.identity:
        c.w[:, :, 0], c.w[:, :, 1] = 1.0, 0.0
    c.g = [rng.standard_normal((c.n, D)).astype(np.float32) if c.g_mask >> i & 1 else None for i in range(3)]
    return c


def name_of(c):
    return "case %d (n %d %s%s g %d out %d dw %d)" % (c.k, c.n, c.kind, " identity" if c.identity else "", c.g_mask, c.out_mask,
                                                      c.dw_mask)


# ------------------------------------------------------------------------------------------------ host references (float64)
def mats64():
    """C, S [64, 33] and Ci, Si [33, 64] of norm='ortho', n = 64, the angle reduced exactly before cos / sin"""
    j = (np.arange(D)[:, None] * np.arange(BINS)[None, :]) % D
    ang = 2.0 * np.pi * j / D
    cos, sin = np.cos(ang), np.sin(ang)
    sin[(j % 32) == 0] = 0.0
    cos[(j % 32) == 16] = 0.0
    wk = np.full((BINS, 1), 2.0)
    wk[0, 0] = wk[-1, 0] = 1.0
    return cos / 8, -sin / 8, wk * cos.T / 8, -wk * sin.T / 8


def fwd64(x, y, w):
    """np.fft -> (out_img, out_txt, out_fus)"""
    X, Y = np.fft.rfft(f64(x), axis=1, norm="ortho"), np.fft.rfft(f64(y), axis=1, norm="ortho")
    W = f64(w)[..., 0] + 1j * f64(w)[..., 1]
    inv = lambda Z: np.fft.irfft(Z, n=D, axis=1, norm="ortho")            # noqa: E731
    return inv(X * W[0]), inv(Y * W[1]), inv(Y * X * W[2])


def terms64(x, y, w, g, absolute=False):
    """the closed forms of the module docstring -> {name: array} for the three outputs and the five gradients; `absolute`: the
    same formulas over magnitudes, every subtraction an addition (MAG of the bound)"""
    ab = np.abs if absolute else (lambda t: t)
    sg = 1.0 if absolute else -1.0
    C, S, Ci, Si = (ab(m) for m in mats64())
    x, y, w = ab(f64(x)), ab(f64(y)), ab(f64(w))
    a, b, c, e = x @ C, x @ S, y @ C, y @ S
    p = (a, c, c * a + sg * e * b)
    q = (b, e, c * b + e * a)
    out = {}
    n = x.shape[0]
    d = [np.zeros((n, BINS)) for _ in range(4)]                           # da, db, dc, de
    for k in range(3):
        wr, wi = w[k, :, 0], w[k, :, 1]
        out[FWD_NAMES[k]] = (p[k] * wr + sg * q[k] * wi) @ Ci + (p[k] * wi + q[k] * wr) @ Si
        dw = np.zeros((BINS, 2))
        if g[k] is not None:
            gk = ab(f64(g[k]))
            dP, dQ = gk @ Ci.T, gk @ Si.T
            dw[:, 0] = (dP * p[k] + dQ * q[k]).sum(axis=0)
            dw[:, 1] = (dQ * p[k] + sg * dP * q[k]).sum(axis=0)
            dp, dq = dP * wr + dQ * wi, dQ * wr + sg * dP * wi
            if k == 0:
                d[0] += dp
                d[1] += dq
            elif k == 1:
                d[2] += dp
                d[3] += dq
            else:
                d[0] += dp * c + dq * e
                d[1] += dq * c + sg * dp * e
                d[2] += dp * a + dq * b
                d[3] += dq * a + sg * dp * b
        out[DW_NAMES[k]] = dw
    out["dx"] = d[0] @ C.T + d[1] @ S.T
    out["dy"] = d[2] @ C.T + d[3] @ S.T
    return out


def bounds(x, y, w, g):
    """-> {name: (ref, bound)} for every output of both calls"""
    n = np.asarray(x).shape[0]
    ref, mag = terms64(x, y, w, g), terms64(x, y, w, g, absolute=True)
    for name, r in zip(FWD_NAMES, fwd64(x, y, w)):
        ref[name] = r                                                     # the forward's reference is np.fft
    count = dict(N_OUT, dx=N_DX, dy=N_DX, **{k: v + n_red(n) for k, v in N_DW_TERM.items()})
    return {k: (ref[k], SLACK * gamma(count[k]) * mag[k] + count[k] * TINY) for k in ref}


def check(x, y, w, g, got, name):
    """got: {name: array or tensor} of any subset of the outputs -> the worst err / bound per family"""
    b = bounds(x, y, w, g)
    worst = {}
    for k, v in got.items():
        fam = "out" if k in FWD_NAMES else "dw" if k in DW_NAMES else "dxy"
        v = v.reshape(b[k][0].shape) if hasattr(v, "reshape") else v
        worst[fam] = max(worst.get(fam, 0.0), compare(v, *b[k], name + " " + k))
    return worst


# ------------------------------------------------------------------------------------------------ no GPU: the axes
def test_cases_span_every_axis():
    cs = [case(k) for k in range(CASES)]
    ns = axis_n()
    r = rows_per_block(1)
    assert r == 64 == rows_per_block(BIG) and rows_per_block(TWO_TILES) == 128 and rows_per_block(65536) == 64
    assert {0, 1, 2, 15, 16, 17, 63, 64, 65, r - 1, r, r + 1, 2 * r + 1} <= set(ns)
    assert set(ns) | {BIG, TWO_TILES} == {c.n for c in cs}
    assert blocks(BIG) > 4 * 64 and blocks(TWO_TILES) * 128 >= TWO_TILES > (blocks(TWO_TILES) - 1) * 128
    assert {c.g_mask for c in cs} == set(range(1, 8))                     # every NULL combination of the gradients but all three
    assert {c.out_mask for c in cs} == set(range(8))                      # every combination of wanted outputs
    assert {c.dw_mask for c in cs if c.out_mask & 4} == set(range(1, 8))
    assert {c.kind for c in cs} == set(KINDS) and {c.identity for c in cs} == {True, False}
    assert {c.null_ws for c in cs} == {True, False}
    for kind in KINDS:
        assert {c.g_mask for c in cs if c.kind == kind} >= {1, 2, 4}
    for n in ns:
        if n > 2:
            assert len({c.kind for c in cs if c.n == n}) >= 2, n             # (every kind keeps N(0, 1) rows of the three scales)
    for c in cs:
        for t in (c.x, c.y):
            if not c.n:
                continue
            mags = np.abs(t).max(axis=1)
            if c.kind == "zeros":
                assert (mags == 0).any()
            if c.kind == "impulse":
                assert ((t != 0).sum(axis=1) == 1).any()
            if c.kind == "constant":
                assert ((t == t[:, :1]).all(axis=1) & (mags > 0)).any()
            if c.kind == "mixed" and c.n > 60:
                assert (mags > 100).any() and (mags < 0.1).any() and ((mags > 0.5) & (mags < 10)).any()
    assert any(c.identity and c.n > 60 for c in cs)


# ------------------------------------------------------------------------------------------------ GPU: the raw C ABI, guarded
def _workspace(n):
    nbytes = int(_lib().mmrec_spectrum_workspace_bytes(n))
    assert nbytes == blocks(n) * 3 * BINS * 2 * 4
    return torch.full((nbytes // 4 + GUARD,), SENTINEL, dtype=torch.int32, device="cuda:0"), nbytes // 4


def run_case(c, w=None):
    """the case's forward and backward through the raw ABI -> {name: tensor} of every output written"""
    from mmrec_amd import hip_ops
    p_, lib, name = hip_ops._p, _lib(), name_of(c)
    w = c.w if w is None else w
    x, y, ws_ = _on(c.x), _on(c.y), [_on(np.ascontiguousarray(w[i])) for i in range(3)]
    g = [None if t is None else _on(t) for t in c.g]
    shapes = {k: (c.n, D) for k in FWD_NAMES}
    held, ptr = _outs(shapes)
    rc = lib.mmrec_spectrum_fwd_f32(p_(x), p_(y), p_(ws_[0]), p_(ws_[1]), p_(ws_[2]), c.n, D, ptr["out_img"], ptr["out_txt"],
                                    ptr["out_fus"], hip_ops._stream())
    assert rc == 0, (name, rc)
    out = _collect(held, shapes, name) if c.n else {}
    shapes = {"dx": (c.n, D) if c.out_mask & 1 else None, "dy": (c.n, D) if c.out_mask & 2 else None}
    shapes.update({k: (BINS, 2) if (c.out_mask & 4 and c.dw_mask >> i & 1) else None for i, k in enumerate(DW_NAMES)})
    held, ptr = _outs(shapes)
    ws, n_ws = (None, 0) if c.null_ws else _workspace(c.n)
    rc = lib.mmrec_spectrum_bwd_f32(p_(x), p_(y), p_(ws_[0]), p_(ws_[1]), p_(ws_[2]), p_(g[0]), p_(g[1]), p_(g[2]), c.n, D,
                                    ptr["dx"], ptr["dy"], ptr["dw_img"], ptr["dw_txt"], ptr["dw_fus"], p_(ws), hip_ops._stream())
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
def test_spectrum_fuzz(k):
    c = case(k)
    name = name_of(c)
    got = run_case(c)
    worst = check(c.x, c.y, c.w, c.g, got, name) if c.n else {}
    print("%s: worst err / bound %s" % (name, " ".join("%s %.3f" % kv for kv in sorted(worst.items()))))
    if c.identity and c.n:                                                # the identity filter gives the image rows back
        ref, bound = bounds(c.x, c.y, c.w, c.g)["out_img"]
        compare(got["out_img"], f64(c.x), bound + 8 * 2.0 ** -52 * np.abs(f64(c.x)), name + " identity")
    for k_ in DW_NAMES:
        if k_ in got:
            assert float(got[k_][0, 1]) == 0.0 and float(got[k_][BINS - 1, 1]) == 0.0, (name, k_)
    again = run_case(c)                                                   # the same calls again: the same bits
    poisoned = c.w.copy()
    poisoned[:, 0, 1] = poisoned[:, BINS - 1, 1] = np.nan                 # the two imaginary weights no real inverse reads
    other = run_case(c, poisoned)
    assert got.keys() == again.keys() == other.keys()
    for k_ in got:
        assert torch.equal(_bits(got[k_]), _bits(again[k_])), (name, k_, "not repeatable")
        assert torch.equal(_bits(got[k_]), _bits(other[k_])), (name, k_, "depends on the imaginary weight of bin 0 or 32")


@pytest.mark.gpu
def test_wrapper_autograd_takes_the_kernels_and_honours_needs_input_grad():
    """hip_ops.spectrum_fusion with only some outputs used and only some operands requiring gradients: the library is given NULL
    for the rest, the results meet the raw ABI's bounds, and an unserved call is the torch composition bit for bit"""
    from mmrec_amd import hip_ops
    c = case(9)
    assert c.n > 64
    lib = _lib()
    seen = []
    real_b = lib.mmrec_spectrum_bwd_f32
    x, y = _on(c.x).requires_grad_(), _on(c.y)
    w = [_on(c.w[i:i + 1].copy()).requires_grad_(i != 1) for i in range(3)]
    g_txt, g_fus = np.ones((c.n, D), np.float32), 2 * np.ones((c.n, D), np.float32)
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(lib, "mmrec_spectrum_bwd_f32", lambda *a: seen.append(a) or real_b(*a))
        assert hip_ops.spectrum_fusion_served(x, y, *w)
        oi, ot, of = hip_ops.spectrum_fusion(x, y, *w)
        (ot.sum() + 2 * of.sum()).backward()
        torch.cuda.synchronize()
    assert len(seen) == 1
    a = seen[0]
    assert a[5] is None and a[6] is not None and a[7] is not None         # g_img never arrived
    assert a[10] is not None and a[11] is None and a[12] is not None and a[13] is None and a[14] is not None
    assert y.grad is None and w[1].grad is None
    got = {"out_img": oi.detach(), "out_txt": ot.detach(), "out_fus": of.detach(), "dx": x.grad, "dw_img": w[0].grad[0],
           "dw_fus": w[2].grad[0]}
    print("wrapper: worst err / bound", check(c.x, c.y, c.w, [None, g_txt, g_fus], got, "wrapper"))
    assert float(w[0].grad.abs().max()) == 0.0 and float(w[2].grad.abs().max()) > 0
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(hip_ops, "SPECTRUM", False)
        assert not hip_ops.spectrum_fusion_served(x, y, *w)
        off = hip_ops.spectrum_fusion(x, y, *w)
    ref = hip_ops.spectrum_fusion_torch(x, y, *w)
    assert all(torch.equal(_bits(a_.detach()), _bits(b_.detach())) for a_, b_ in zip(off, ref))
    assert not hip_ops.spectrum_fusion_served(x[:, ::2], y[:, ::2], *w) and not hip_ops.spectrum_fusion_served(x.cpu(), y.cpu(), *w)


@pytest.mark.gpu
def test_forward_and_backward_replay_from_a_captured_graph():
    """forward + backward captured on one stream and replayed twice: the eager bits (no host synchronisation, no allocation
    inside the library, no data-dependent launch shape)"""
    from mmrec_amd import hip_ops
    c = case(9)
    x, y = _on(c.x).requires_grad_(), _on(c.y).requires_grad_()
    w = [_on(c.w[i:i + 1].copy()).requires_grad_() for i in range(3)]
    gi, gt, gf = (_on(np.random.default_rng(5 + i).standard_normal((c.n, D)).astype(np.float32)) for i in range(3))

    def step():
        for t in [x, y] + w:
            t.grad = None
        oi, ot, of = hip_ops.spectrum_fusion(x, y, *w)
        ((oi * gi).sum() + (ot * gt).sum() + (of * gf).sum()).backward()
        return [oi.detach(), ot.detach(), of.detach(), x.grad, y.grad] + [t.grad for t in w]
    eager = [t.clone() for t in step()]
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        held = step()
    with torch.no_grad():                                                 # other inputs in the same buffers, then the first ones again
        x.copy_(_on(c.x[::-1].copy()))
    graph.replay()
    torch.cuda.synchronize()
    other = [t.clone() for t in held]
    with torch.no_grad():
        x.copy_(_on(c.x))
    graph.replay()
    torch.cuda.synchronize()
    first = [t.clone() for t in held]
    graph.replay()
    torch.cuda.synchronize()
    for a, b, b2, o in zip(eager, first, held, other):
        assert torch.equal(_bits(a), _bits(b)) and torch.equal(_bits(b), _bits(b2))
    assert not torch.equal(_bits(eager[0]), _bits(other[0]))              # the replay really computed
    got = dict(zip(FWD_NAMES + ("dx", "dy"), held[:5]))
    got.update({k: t[0] for k, t in zip(DW_NAMES, held[5:])})
    print("graph replay: worst err / bound", check(c.x, c.y, c.w, [t.cpu().numpy() for t in (gi, gt, gf)], got, "graph"))
