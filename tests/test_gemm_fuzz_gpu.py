"""GPU: seeded differential fuzz of the general GEMM (`mmrec_gemm_nt_f32`, the 128 x 128 LDS-DMA tile of csrc/mfma_stream.h), the
blocked weight gradient (`mmrec_linear_bwd_w_f32`, out = 64 j in one launch over grid.z) and the five dense out = 64 projection
entry points, all through the C ABI with raw pointers, against float64 numpy written here from the formulas in
include/mmrec_hip.h:   C[M, :N] = A[M, K] B[N, K]^T + bias[N];   dW [out, F] = dY^T X, db [out] = column sums of dY;
Y [n, 64] = X W^T + b, dX [n, F] = dY W.  Every output is ONE matrix product C = A B^T (+ extra) of two arrays of the case, so one
checker serves every family (`Out`).

Two acceptance modes per family:
  exact  A / X / dY / bias are multiples of 1/16, B / W multiples of 1/8, all of magnitude <= 1, and the generator asserts
         sum |terms| + |bias| < 2^14 per output: every partial sum in ANY order is a multiple of 2^-8 below 2^14 and so an exact
         fp32 number -- the output must EQUAL float64 as a number.  Contraction lengths up to 4096 (4100 items for dW).  The
         split-operand entry points are held to the same equality: such values have at most 5 significant bits, the first fp16 /
         bf16 part of each operand holds them exactly, the other parts are zero and the power-of-two scales of the dX kernel
         are exact.
  float  normal draws, rows and columns scaled by 2^-10 ... 2^10, exact zeros (elements, whole rows), in one case of four a
         whole row of inf / -inf / NaN in one operand.  fp32 kernels:
             |got - ref64| <= gamma(n + 2) (sum_k |a_k b_k| + |bias|) + n 2^-149,      n = the contraction length,
         which holds for n products and n additions of fp32 in any order (no split plan of the code under test is restated);
         n <= 1024 keeps gamma below 6.2e-5, so an element off by 1e-4 of its magnitude sum is caught everywhere.  Split-operand
         entry points: `check` of test_linear_fuzz_gpu.py as it stands (2e-6 of the magnitude sum, 3e-5 where something is scaled
         up by more than 100).  Non-finite outputs must be float64's, value for value (with fp32's range), and may appear only
         where the operand row of that output row / column holds a non-finite value.

Outputs live in `Guarded` buffers pre-filled with a sentinel: the guard floats on both sides must survive, columns N .. ldc of
every row of C must still hold the sentinel, workspaces are exactly `*_workspace_bytes()` long with a guard behind them, and every
input is followed by a NaN-filled guard (a read past the end would show up in the output).  Each device case prints its worst
err / bound.  The unmarked tests check the generator (every axis value occurs, grid assertions) and the checker itself (an fp32
numpy restatement passes, each planted error fails)."""
import numpy as np
import pytest
import torch

from tests.test_linear_fuzz_gpu import check as split_check
from tests.test_loss_fuzz_gpu import GUARD, GUARD_VALUE, Guarded, P, Workspace, _ok, gamma

F32, F64 = np.float32, np.float64
FLT_MAX = 3.4028234663852886e38
TINY = 2.0 ** -149
SENTINEL = -7777.25
ERR_BAD_ARG, ERR_UNSUPPORTED = 10001, 10002
REF_BUDGET = 1000 * 500 * 4096                               # multiply-adds of the largest float64 reference

OPS = ("gemm_nt", "bwd_w_wide", "dense64_raw", "wide_autograd")
COUNT = {"gemm_nt": 64, "bwd_w_wide": 44, "dense64_raw": 126, "wide_autograd": 16}
FIRST = {op: sum(COUNT[o] for o in OPS[:i]) for i, op in enumerate(OPS)}
CASES = sum(COUNT.values())                                  # 250

GEMM_M = (1, 31, 32, 33, 127, 128, 129, 255, 257, 1000)
GEMM_N = (1, 3, 31, 64, 96, 127, 128, 129, 192, 256, 320, 384, 500)
GEMM_K = (32, 64, 96, 128, 256, 384, 1024, 4096)
LDC_KINDS = ("N", "N+1", "N+5", "round128", "N+128")
BWW_OUT = (64, 128, 192, 256, 320, 384)
BWW_F = (4, 36, 96, 128, 256, 320, 384, 1024, 4096)
BWW_N = (0, 1, 31, 32, 33, 64, 200, 257, 1000, 2049, 4100)
D64_ENTRIES = ("fwd", "fwd_split", "bwd_w", "bwd_x", "bwd_split")
D64_N = (1, 127, 128, 129, 300, 1100)
D64_F = (4, 40, 96, 128, 320, 384, 1024)
D64_WANT = ("all", "dW_dX", "dX", "dW", "dW_db")            # what mmrec_linear_bwd_split_f32 is asked for (the rest is NULL)
WIDE_SHAPES = ((300, 256, 256), (300, 384, 384), (300, 4096, 256), (33, 32, 128), (129, 96, 384), (1, 128, 128), (257, 64, 256),
               (200, 160, 128))                             # (n, F, out): MMGCN's three at n = 300 first
WIDE_GRADS = ("x", "w", "wb", "all")
SPLIT_ENTRIES = ("fwd_split", "bwd_split")


def ldc_of(kind, N):
    return {"N": N, "N+1": N + 1, "N+5": N + 5, "round128": -(-N // 128) * 128, "N+128": N + 128}[kind]


# ------------------------------------------------------------------------------------------------ cases
class Out:
    """one output of a case: C [rows, :cols] = A [rows, n] B [cols, n]^T (+ extra [cols] on every row), row stride ld"""

    def __init__(self, name, A, B, extra=None, ld=None, rule="f32"):
        assert A.shape[1] == B.shape[1] and A.dtype == F32 and B.dtype == F32
        self.name, self.A, self.B, self.extra, self.rule = name, A, B, extra, rule
        self.rows, self.cols, self.n = A.shape[0], B.shape[0], A.shape[1]
        self.ld = self.cols if ld is None else ld


class Case:
    def __init__(self, seed, op, mode, axes):
        self.seed, self.op, self.mode, self.axes = seed, op, mode, axes
        self.arr, self.outs, self.dominant = {}, [], False

    def tag(self):
        return "seed %d %s %s %s" % (self.seed, self.op, self.mode, " ".join("%s=%s" % kv for kv in self.axes.items()))


def draw_axes(seed):
    """(op, mode, axes) of a seed: cheap, no data"""
    rng = np.random.default_rng(1000 + seed)
    op = [o for o in OPS if FIRST[o] <= seed][-1]
    j = seed - FIRST[op]
    if op == "gemm_nt":
        M, N, K = GEMM_M[j % 10], GEMM_N[j % 13], GEMM_K[(j + j // 8) % 8]
        kind = LDC_KINDS[(j + j // 10) % 5]
        form = ("fwd", "dx")[int(rng.integers(0, 2))]      # B = W as it is stored | B = W^T of a W [K, N] (the dX call)
        bias = bool(rng.integers(0, 2))                     # drawn on its own: MMGCN's (x, W) with and (dY, W^T) without, and the other two
        mode = "exact" if K > 1024 or j % 3 == 0 else "float"
        axes = dict(M=M, N=N, K=K, ldc_kind=kind, ldc=ldc_of(kind, N), form=form, bias=bias)
    elif op == "bwd_w_wide":
        out, F, n = BWW_OUT[j % 6], BWW_F[(j + j // 9) % 9], BWW_N[j % 11]
        if out * F * n > REF_BUDGET:
            out = max(o for o in BWW_OUT if o * F * n <= REF_BUDGET)
        mode = "exact" if n > 1024 or (j // 11) % 2 == 0 else "float"
        axes = dict(out=out, F=F, n=n, db=bool(rng.integers(0, 2)))
    elif op == "dense64_raw":
        slot, F, n = j % 9, D64_F[j % 7], D64_N[(j + j // 9) % 6]      # slots 4 .. 8: bwd_split, one per NULL combination
        entry = D64_ENTRIES[min(slot, 4)]
        mode = "exact" if j < 63 or n > 1024 else "float"   # every (slot, F) pair once in either half
        axes = dict(entry=entry, n=n, F=F)
        if entry in ("fwd", "fwd_split"):
            axes["bias"] = (j // 9) % 2 == 0
        elif entry == "bwd_w":
            axes["db"] = (j // 9) % 2 == 0
        elif entry == "bwd_split":
            axes["want"] = D64_WANT[slot - 4]
    else:
        n, F, out = WIDE_SHAPES[j % 8]
        grads = WIDE_GRADS[(j + j // 8) % 4]
        mode = "exact" if F > 1024 or j < 8 else "float"
        axes = dict(n=n, F=F, out=out, grads=grads, b=grads in ("wb", "all") or (j // 4) % 2 == 0,
                    W_view=F == out and (j + j // 8) % 2 == 0)         # W arrives as base.t() of a square weight (as `_Conv.forward` passes it)
    return op, mode, axes


def _grid(rng, shape, q):
    return (rng.integers(-q, q + 1, size=shape) / float(q)).astype(F32)


def _normal(rng, c, shape, scale=1.0):
    a = rng.standard_normal(shape) * scale
    for axis in (0, 1):
        m = a.shape[axis]
        for i in rng.choice(m, size=min(m, int(rng.integers(0, 4))), replace=False) if m else ():
            f = 2.0 ** int(rng.integers(-10, 11))
            c.dominant |= f > 100.0
            if axis == 0:
                a[i] *= f
            else:
                a[:, i] *= f
    a[rng.random(shape) < 0.15] = 0.0
    if shape[0] > 2 and rng.random() < 0.3:
        a[int(rng.integers(0, shape[0]))] = 0.0
    return a.astype(F32)


def _mat(rng, c, shape, q):
    return _grid(rng, shape, q) if c.mode == "exact" else _normal(rng, c, shape)


def _bad(rng):
    return F32(rng.choice([np.inf, -np.inf, np.nan]))


def _assert_grid(c):
    """the exact mode's premise: operands on their grids, sum |terms| + |bias| < 2^14 for every output"""
    for o in c.outs:
        for a, q in ((o.A, 16), (o.B, 16), (o.extra, 16)):
            if a is not None and a.size:
                assert np.abs(a).max() <= 1.0 and (a * q == np.round(a * q)).all(), (c.tag(), o.name, "off the grid")
        assert o.n * 1.0 + 1.0 < 2.0 ** 14, (c.tag(), o.name)      # |a| |b| <= 1 per term, |bias| <= 1


def draw_case(seed):
    """deterministic in the seed"""
    return make_case(seed, *draw_axes(seed))


def make_case(seed, op, mode, ax, bad_row=None):
    c = Case(seed, op, mode, ax)
    rng = np.random.default_rng(seed)
    A_ = c.arr
    draw = rng.random() < 0.25
    bad_row = mode == "float" and (draw if bad_row is None else bad_row)      # a whole non-finite row of one operand
    if op == "gemm_nt":
        M, N, K = ax["M"], ax["N"], ax["K"]
        A_["A"] = _mat(rng, c, (M, K), 16)
        if ax["form"] == "fwd":
            A_["B"] = _mat(rng, c, (N, K), 8)
        else:                                               # W [out = K, F = N], handed over as W^T
            A_["B"] = np.ascontiguousarray(_mat(rng, c, (K, N), 8).T)
        if ax["bias"]:
            A_["bias"] = _mat(rng, c, (1, N), 16)[0]
        if bad_row:
            t = A_["A"] if rng.random() < 0.5 else A_["B"]
            t[int(rng.integers(0, t.shape[0]))] = _bad(rng)
        c.outs = [Out("C", A_["A"], A_["B"], A_.get("bias"), ld=ax["ldc"])]
    elif op == "bwd_w_wide":
        out, F, n = ax["out"], ax["F"], ax["n"]
        A_["dY"], A_["X"] = _mat(rng, c, (n, out), 16), _mat(rng, c, (n, F), 16)
        if bad_row and n:                                   # a column of dY (one row of dW, one entry of db) or a column of X
            if rng.random() < 0.5:
                A_["dY"][:, int(rng.integers(0, out))] = _bad(rng)
            else:
                A_["X"][:, int(rng.integers(0, F))] = _bad(rng)
        dYt = np.ascontiguousarray(A_["dY"].T)
        c.outs = [Out("dW", dYt, np.ascontiguousarray(A_["X"].T))]
        if ax["db"]:
            c.outs.append(Out("db", dYt, np.ones((1, n), F32)))
    else:
        n, F = ax["n"], ax["F"]
        out = 64 if op == "dense64_raw" else ax["out"]
        A_["X"], A_["W"], A_["dY"] = _mat(rng, c, (n, F), 16), _mat(rng, c, (out, F), 8), _mat(rng, c, (n, out), 16)
        A_["b"] = _mat(rng, c, (1, out), 16)[0]
        if c.mode == "float":
            A_["W"] = (A_["W"] / F32(np.sqrt(F))).astype(F32)
        if bad_row and n > 2:
            t = (A_["X"], A_["W"], A_["dY"])[int(rng.integers(0, 3))]
            t[int(rng.integers(0, t.shape[0]))] = _bad(rng)
        X, W, dY, b = A_["X"], A_["W"], A_["dY"], A_["b"]
        Wt, dYt, Xt = np.ascontiguousarray(W.T), np.ascontiguousarray(dY.T), np.ascontiguousarray(X.T)
        ones = np.ones((1, n), F32)
        if op == "dense64_raw":
            e = ax["entry"]
            rule = "split" if e in SPLIT_ENTRIES else "f32"
            want = ax.get("want", "")
            if e in ("fwd", "fwd_split"):
                c.outs = [Out("Y", X, W, b if ax["bias"] else None, rule=rule)]
            if e == "bwd_w" or want in ("all", "dW_dX", "dW", "dW_db"):
                c.outs.append(Out("dW", dYt, Xt, rule=rule))
            if (e == "bwd_w" and ax["db"]) or want in ("all", "dW_db"):
                c.outs.append(Out("db", dYt, ones, rule=rule))
            if e == "bwd_x" or want in ("all", "dW_dX", "dX"):
                c.outs.append(Out("dX", dY, Wt, rule=rule))
        else:
            g = ax["grads"]
            c.outs = [Out("Y", X, W, b if ax["b"] else None)]
            if g in ("x", "all"):
                c.outs.append(Out("dX", dY, Wt))
            if g in ("w", "wb", "all"):
                c.outs.append(Out("dW", dYt, Xt))
            if g in ("wb", "all"):
                c.outs.append(Out("db", dYt, ones))
    if mode == "exact":
        _assert_grid(c)
    for o in c.outs:
        assert mode == "exact" or o.n <= 1024, (c.tag(), "float cases keep the contraction at 1024 or below")
        assert o.rows * o.cols * max(o.n, 1) <= REF_BUDGET, c.tag()
    return c


# ------------------------------------------------------------------------------------------------ reference and checker
def reference(o):
    """float64: (ref with fp32's range, sum of magnitudes, where a non-finite value may stand)"""
    A, B = o.A.astype(F64), o.B.astype(F64)
    with np.errstate(invalid="ignore", over="ignore"):
        ref, mag = A @ B.T, np.abs(A) @ np.abs(B).T
        if o.extra is not None:
            ref, mag = ref + o.extra.astype(F64), mag + np.abs(o.extra.astype(F64))
        ref = np.where(np.abs(ref) > FLT_MAX, np.sign(ref) * np.inf, ref)
    may = ~np.isfinite(o.A).all(axis=1)[:, None] | ~np.isfinite(o.B).all(axis=1)[None, :]
    return ref, mag, may


def pack(body):
    """a payload between guard floats, as `Guarded` lays it out"""
    g = np.full(GUARD, GUARD_VALUE, F32)
    return np.concatenate([g, np.asarray(body, F32).ravel(), g])


def check_out(c, o, ref3, buf):
    """buf: the whole guarded buffer of output o as the device left it.  Returns the worst err / bound."""
    name = "%s %s" % (c.tag(), o.name)
    ref, mag, may = ref3
    buf = np.asarray(buf)
    assert buf.shape == (o.rows * o.ld + 2 * GUARD,), (name, buf.shape)
    assert (buf[:GUARD] == GUARD_VALUE).all() and (buf[GUARD + o.rows * o.ld:] == GUARD_VALUE).all(), (name, "guard floats overwritten")
    body = buf[GUARD:GUARD + o.rows * o.ld].reshape(o.rows, o.ld)
    assert (body[:, o.cols:] == F32(SENTINEL)).all(), (name, "columns N .. ldc written")
    got32 = body[:, :o.cols]
    got = got32.astype(F64)
    if c.mode == "exact":
        same = got == ref
        assert same.all(), (name, "not equal to float64", int((~same).sum()), np.argwhere(~same)[:4].tolist())
        return 0.0
    fin = np.isfinite(ref)
    assert not (~fin & ~may).any(), (name, "the reference is non-finite where no operand row is")
    if o.rule == "split":
        with np.errstate(invalid="ignore", over="ignore"):
            split_check(got32, o.A, np.ascontiguousarray(o.B.T),
                        extra=None if o.extra is None else np.broadcast_to(o.extra, got32.shape), name=name, dominant=c.dominant)
        bound = (3e-5 if c.dominant else 2e-6) * mag + 1e-40
    else:
        assert np.isfinite(got[fin]).all(), (name, "non-finite output where float64 is finite", int((~np.isfinite(got[fin])).sum()))
        assert np.array_equal(got[~fin], ref[~fin], equal_nan=True), (name, "non-finite outputs are not float64's")
        bound = gamma(o.n + 2) * mag + o.n * TINY
    if not fin.any():
        return 0.0
    with np.errstate(invalid="ignore"):
        err = np.where(fin, np.abs(got - ref), 0.0)
        ratio = np.where(fin, err / np.where(fin & (bound > 0), bound, 1.0), 0.0)
        viol = fin & (err > bound)
    assert not viol.any(), (name, "err / bound %.3g at %s" % (float(ratio.max()), np.argwhere(viol)[:4].tolist()), int(viol.sum()))
    return float(ratio.max())


def check_case(c, got, refs=None):
    """got: output name -> guarded buffer.  Every output the case asks for must be there."""
    refs = refs or {o.name: reference(o) for o in c.outs}
    assert sorted(got) == sorted(o.name for o in c.outs), (c.tag(), sorted(got))
    return max([check_out(c, o, refs[o.name], got[o.name]) for o in c.outs] + [0.0])


# ------------------------------------------------------------------------------------------------ fp32 numpy restatement
def mm32(A, B, drop=None):
    """A B^T in fp32, 32-wide k tiles in order; drop = (rows, cols, tile): that tile is left out of that output block"""
    acc = np.zeros((A.shape[0], B.shape[0]), F32)
    with np.errstate(invalid="ignore", over="ignore"):
        for t, k0 in enumerate(range(0, A.shape[1], 32)):
            part = (A[:, None, k0:k0 + 32] * B[None, :, k0:k0 + 32]).sum(axis=-1, dtype=F32)
            if drop is not None and drop[2] == t:
                part[drop[0], drop[1]] = 0.0
            acc += part
    return acc


def emulate_out(o, **kw):
    body = np.full((o.rows, o.ld), SENTINEL, F32)
    with np.errstate(invalid="ignore", over="ignore"):
        v = mm32(o.A, o.B, **kw)
        body[:, :o.cols] = v if o.extra is None else v + o.extra
    return body


def emulate(c):
    return {o.name: pack(emulate_out(o)) for o in c.outs}


def emulate_bwd_w(c, nsplit, lose=None, swap=None, db_to_zero=None):
    """mmrec_linear_bwd_w_f32's shape of work: per 64-column group z of dY, `nsplit` slabs over item chunks summed in order;
    lose = (z, slab), swap = (z1, z2) groups of dY taken for each other, db_to_zero = z: that group's db lands in group 0"""
    dY, X = c.arr["dY"], c.arr["X"]
    n, out = dY.shape
    chunk = -(-max(n, 1) // nsplit)
    nz = out // 64
    src = list(range(nz))
    if swap:
        src[swap[0]], src[swap[1]] = src[swap[1]], src[swap[0]]
    dW, db = np.zeros((out, X.shape[1]), F32), np.full(out, SENTINEL, F32)
    for z in range(nz):
        g = dY[:, 64 * src[z]:64 * src[z] + 64]
        acc, dacc = np.zeros((64, X.shape[1]), F32), np.zeros(64, F32)
        for s in range(nsplit):
            sl = slice(s * chunk, min(n, (s + 1) * chunk))
            if lose != (z, s):
                acc += mm32(np.ascontiguousarray(g[sl].T), np.ascontiguousarray(X[sl].T))
            dacc += g[sl].sum(axis=0, dtype=F32)
        dW[64 * z:64 * z + 64] = acc
        zz = 0 if db_to_zero == z else z
        db[64 * zz:64 * zz + 64] = dacc
    got = {"dW": pack(dW)}
    if c.axes["db"]:
        got["db"] = pack(db)
    return got


def _find(cond, lo=0, hi=CASES):
    for s in range(lo, hi):
        op, mode, ax = draw_axes(s)
        if cond(op, mode, ax):
            return s
    raise AssertionError("no case with the wanted axes")


def _small(c, limit=3e7):
    return all(o.rows * o.cols * max(o.n, 1) <= limit for o in c.outs)


def _finite(c):
    return all(np.isfinite(a).all() for a in c.arr.values())


def test_generator_is_deterministic_and_on_the_grid():
    """the same seed draws the same bits; every one of the cases passes the generator's assertions (inside draw_case: the grid
    and the magnitude sum in exact mode, the contraction length in float mode, the size of the reference)"""
    for s in range(CASES):
        op, mode, ax = draw_axes(s)
        c = draw_case(s)
        assert (c.op, c.mode, c.axes) == (op, mode, ax)
        if s % 9 == 0:
            d = draw_case(s)
            assert c.axes == d.axes and all(np.array_equal(c.arr[k], d.arr[k], equal_nan=True) for k in c.arr), s
        if op == "bwd_w_wide" and ax["out"] > 64 and ax["n"] > 0:
            g = [c.arr["dY"][:, 64 * z:64 * z + 64] for z in range(ax["out"] // 64)]
            assert all(not np.array_equal(g[a], g[b]) for a in range(len(g)) for b in range(a)), (s, "two groups of dY are the same")


def test_cases_span_every_axis():
    A = [draw_axes(s) for s in range(CASES)]

    def vals(op, key):
        return {ax[key] for o, _, ax in A if o == op and key in ax}
    for op in OPS:
        assert sum(o == op for o, _, _ in A) == COUNT[op]
        assert {m for o, m, _ in A if o == op} == {"exact", "float"}, op
    assert COUNT["gemm_nt"] >= 60 and COUNT["bwd_w_wide"] >= 40 and COUNT["dense64_raw"] >= 30
    assert vals("gemm_nt", "M") == set(GEMM_M) and vals("gemm_nt", "N") == set(GEMM_N) and vals("gemm_nt", "K") == set(GEMM_K)
    assert vals("gemm_nt", "ldc_kind") == set(LDC_KINDS) and vals("gemm_nt", "bias") == {False, True}
    assert {(ax["form"], ax["bias"]) for o, _, ax in A if o == "gemm_nt"} == {(f, b) for f in ("fwd", "dx") for b in (False, True)}
    G = [(m, ax) for o, m, ax in A if o == "gemm_nt"]
    assert {(ax["K"] // 32) % 2 for _, ax in G if ax["K"] > 32} == {0, 1} and any(ax["K"] == 32 for _, ax in G)
    assert all(m == "exact" for m, ax in G if ax["K"] > 1024)
    assert any(ax["M"] % 128 and ax["N"] % 128 and ax["M"] > 128 and ax["N"] > 128 for _, ax in G), "partial last row tile + partial last column tile"
    assert any(ax["ldc"] > ax["N"] and ax["bias"] for _, ax in G), "ldc > N with bias"
    assert any(ax["ldc"] > ax["N"] and ax["N"] % 128 == 0 for _, ax in G) and any(ax["ldc"] == ax["N"] for _, ax in G)
    assert vals("bwd_w_wide", "out") == set(BWW_OUT) and vals("bwd_w_wide", "F") == set(BWW_F) and vals("bwd_w_wide", "n") == set(BWW_N)
    assert vals("bwd_w_wide", "db") == {False, True}
    assert all(m == "exact" for o, m, ax in A if o == "bwd_w_wide" and ax["n"] > 1024)
    assert any(ax["n"] == 0 and ax["db"] for o, _, ax in A if o == "bwd_w_wide") and any(ax["n"] == 0 and not ax["db"] for o, _, ax in A if o == "bwd_w_wide")
    assert vals("dense64_raw", "entry") == set(D64_ENTRIES) and vals("dense64_raw", "n") == set(D64_N) and vals("dense64_raw", "F") == set(D64_F)
    assert vals("dense64_raw", "want") == set(D64_WANT) and vals("dense64_raw", "bias") == {False, True} and vals("dense64_raw", "db") == {False, True}
    for e in D64_ENTRIES:
        assert {m for o, m, ax in A if o == "dense64_raw" and ax["entry"] == e} == {"exact", "float"}, e
        assert {ax["F"] for o, _, ax in A if o == "dense64_raw" and ax["entry"] == e} == set(D64_F), e
    served = {ax["want"] for o, _, ax in A if o == "dense64_raw" and ax["entry"] == "bwd_split" and ax["F"] % 128 == 0}
    assert served == set(D64_WANT), "every NULL combination on the split-operand kernels"
    assert vals("wide_autograd", "out") == {128, 256, 384} and vals("wide_autograd", "grads") == set(WIDE_GRADS)
    assert vals("wide_autograd", "b") == {False, True} and vals("wide_autograd", "W_view") == {False, True}
    assert {(ax["F"], ax["W_view"]) for o, _, ax in A if o == "wide_autograd" and ax["F"] == ax["out"]} >= {(f, v) for f in (256, 384) for v in (False, True)}
    assert {(ax["n"], ax["F"], ax["out"]) for o, _, ax in A if o == "wide_autograd"} >= {(300, 256, 256), (300, 384, 384), (300, 4096, 256)}


def _rejects(c, got, refs):
    with pytest.raises(AssertionError):
        check_case(c, got, refs)


def test_checker_rejects_planted_errors():
    """an fp32 numpy restatement of every family passes in both modes; each planted error fails"""
    # ---- every family, both modes: the first small cases pass
    for op in OPS:
        for mode in ("exact", "float"):
            seeds = [s for s in range(FIRST[op], FIRST[op] + COUNT[op]) if draw_axes(s)[1] == mode][:12]
            done = 0
            for s in seeds:
                c = draw_case(s)
                if _small(c, 1e7) and done < 3:
                    check_case(c, emulate_bwd_w(c, 3) if op == "bwd_w_wide" else emulate(c))
                    done += 1
            assert done, (op, mode)
    # a float case with a non-finite operand row passes too, and fails with the pattern moved
    c = make_case(6, "gemm_nt", "float", dict(M=33, N=129, K=64, ldc_kind="N", ldc=129, form="fwd", bias=True), bad_row=True)
    assert not _finite(c)
    refs = {o.name: reference(o) for o in c.outs}
    good = emulate(c)
    check_case(c, good, refs)
    body = good["C"].copy()
    i = int(np.flatnonzero(~np.isfinite(body))[0])
    body[i] = 1.0
    _rejects(c, {"C": body}, refs)
    # ---- gemm_nt: M, N above one tile with partial last tiles, bias, ldc > N, at least three k tiles
    for mode in ("exact", "float"):
        c = make_case(7, "gemm_nt", mode, dict(M=257, N=192, K=96, ldc_kind="N+5", ldc=197, form="fwd", bias=True), bad_row=False)
        o = c.outs[0]
        refs = {"C": reference(o)}
        M, N, ld = o.rows, o.cols, o.ld
        clean = emulate_out(o)
        assert check_case(c, {"C": pack(clean)}, refs) <= 1.0

        def planted(f, **kw):
            body = emulate_out(o, **kw) if kw else clean.copy()
            f(body)
            _rejects(c, {"C": pack(body)}, refs)
        planted(lambda b: None, drop=(slice(128, M), slice(0, 128), 1))                    # one k tile of one output tile
        planted(lambda b: None, drop=(slice(0, 128), slice(128, N), o.n // 32 - 1))       # ... the last one, partial column tile

        def swap_cols(b):
            j = 128 + int(np.argmax(np.abs(clean[0, 128:N - 1] - clean[0, 129:N])))
            assert clean[0, j] != clean[0, j + 1]
            b[:, [j, j + 1]] = b[:, [j + 1, j]]
        planted(swap_cols)

        def bias_twice(b):
            b[:, :N] += o.extra
        planted(bias_twice)

        def bias_shifted(b):                                # the bias of column c - 128 on the columns of the second tile
            b[:, 128:N] += o.extra[:N - 128] - o.extra[128:N]
        planted(bias_shifted)

        def row_aliased(b):
            b[128:M, :N] = clean[:M - 128, :N]
        planted(row_aliased)

        def sentinel_hit(b):
            b[M - 1, N] = clean[M - 1, N - 1]
        planted(sentinel_hit)
        if mode == "float":
            def off_by_1e4(b):
                i, j = np.unravel_index(int(np.argmax(refs["C"][1])), (M, N))
                b[i, j] += F32(1e-4 * refs["C"][1][i, j])
            planted(off_by_1e4)
            for i, j in ((0, 0), (M - 1, N - 1), (128, 128)):      # ... and on any element, in terms of its magnitude sum
                body = clean.copy()
                body[i, j] = F32(refs["C"][0][i, j] + 1e-4 * refs["C"][1][i, j])
                if refs["C"][1][i, j] > 0:
                    _rejects(c, {"C": pack(body)}, refs)
        for at in (0, GUARD - 1, GUARD + M * ld, M * ld + 2 * GUARD - 1):
            buf = pack(clean)
            buf[at] = 1.0
            _rejects(c, {"C": buf}, refs)
    # ---- bwd_w_wide: several groups, db, several slabs
    for mode in ("exact", "float"):
        c = make_case(8, "bwd_w_wide", mode, dict(out=192, F=96, n=200, db=True), bad_row=False)
        refs = {o.name: reference(o) for o in c.outs}
        assert check_case(c, emulate_bwd_w(c, 4), refs) <= 1.0
        nz = c.axes["out"] // 64
        _rejects(c, emulate_bwd_w(c, 4, swap=(1, nz - 1)), refs)
        _rejects(c, emulate_bwd_w(c, 4, lose=(nz - 1, 3)), refs)
        _rejects(c, emulate_bwd_w(c, 4, lose=(0, 0)), refs)
        _rejects(c, emulate_bwd_w(c, 4, db_to_zero=nz - 1), refs)
        got = emulate_bwd_w(c, 4)
        got["db"][GUARD + 64 * nz] = 0.0                     # the float behind db
        _rejects(c, got, refs)
        got = emulate_bwd_w(c, 4)
        del got["db"]                                       # an output that was asked for and not produced
        _rejects(c, got, refs)
    # ---- the split-operand rule (float mode: `check` of the out = 64 fuzz): a 1e-4 element and a lost guard
    c = make_case(9, "dense64_raw", "float", dict(entry="bwd_split", n=129, F=128, want="all"), bad_row=False)
    refs = {o.name: reference(o) for o in c.outs}
    assert check_case(c, emulate(c), refs) <= 1.0
    for o in c.outs:
        got = emulate(c)
        i, j = np.unravel_index(int(np.argmax(refs[o.name][1])), refs[o.name][1].shape)
        got[o.name][GUARD + i * o.ld + j] += F32(1e-4 * refs[o.name][1][i, j])
        _rejects(c, got, refs)
        got = emulate(c)
        got[o.name][-1] = 0.0
        _rejects(c, got, refs)


# ------------------------------------------------------------------------------------------------ GPU plumbing
def _lib_stream():
    from mmrec_amd import _lib as L, hip_ops
    return L.load(), hip_ops._stream()


def _in(a):
    """an input on the device, followed by a NaN-filled guard (None stays None)"""
    if a is None:
        return None
    a = np.ascontiguousarray(a, F32).ravel()
    t = torch.full((a.size + GUARD,), float("nan"), device="cuda:0")
    t[:a.size].copy_(torch.from_numpy(a))
    return t


def _buf(g, name):
    g.get(name)                                             # (asserts the guards on its own)
    return g.buf.cpu().numpy()


def run_gpu(c):
    """the case through the C ABI (wide_autograd: through hip_ops.linear); output name -> guarded buffer"""
    lib, s = _lib_stream()
    ax, a, tag = c.axes, c.arr, c.tag()
    got = {}
    if c.op == "gemm_nt":
        A, B, bias = _in(a["A"]), _in(a["B"]), _in(a.get("bias"))
        C = Guarded(ax["M"] * ax["ldc"], fill=SENTINEL)
        _ok(lib.mmrec_gemm_nt_f32(P(A), P(B), P(bias), P(C.view), ax["M"], ax["N"], ax["K"], ax["ldc"], s), tag)
        torch.cuda.synchronize()
        got["C"] = _buf(C, tag)
    elif c.op == "bwd_w_wide" or (c.op == "dense64_raw" and ax["entry"] == "bwd_w"):
        out = ax.get("out", 64)
        n, F = ax["n"], ax["F"]
        dY, X = _in(a["dY"]), _in(a["X"])
        ws = Workspace(lib.mmrec_linear_workspace_bytes(n, F, out))
        dW, db = Guarded(out * F, fill=SENTINEL), (Guarded(out, fill=SENTINEL) if ax["db"] else None)
        _ok(lib.mmrec_linear_bwd_w_f32(P(dY), P(X), P(dW.view), P(db.view) if db else None, n, F, out, ws.p, s), tag)
        torch.cuda.synchronize()
        ws.ok(tag)
        got["dW"] = _buf(dW, tag)
        if db:
            got["db"] = _buf(db, tag)
    elif c.op == "dense64_raw":
        n, F, e = ax["n"], ax["F"], ax["entry"]
        X, W, dY = _in(a["X"]), _in(a["W"]), _in(a["dY"])
        if e in ("fwd", "fwd_split"):
            b = _in(a["b"]) if ax["bias"] else None
            ws = Workspace(lib.mmrec_linear_workspace_bytes(n, F, 64))
            Y = Guarded(n * 64, fill=SENTINEL)
            fn = lib.mmrec_linear_fwd_f32 if e == "fwd" else lib.mmrec_linear_fwd_split_f32
            _ok(fn(P(X), P(W), P(b), P(Y.view), n, F, 64, ws.p, s), tag)
            torch.cuda.synchronize()
            ws.ok(tag)
            got["Y"] = _buf(Y, tag)
        elif e == "bwd_x":
            dX = Guarded(n * F, fill=SENTINEL)
            _ok(lib.mmrec_linear_bwd_x_f32(P(dY), P(W), P(dX.view), n, F, 64, s), tag)
            torch.cuda.synchronize()
            got["dX"] = _buf(dX, tag)
        else:
            names = [o.name for o in c.outs]
            ws = Workspace(lib.mmrec_linear_bwd_split_workspace_bytes(n, F, 64))
            G = {k: Guarded(m, fill=SENTINEL) for k, m in (("dW", 64 * F), ("db", 64), ("dX", n * F)) if k in names}
            ptr = {k: (P(G[k].view) if k in G else None) for k in ("dW", "db", "dX")}      # NULL for what is not wanted
            _ok(lib.mmrec_linear_bwd_split_f32(P(dY), P(X), P(W), ptr["dW"], ptr["db"], ptr["dX"], n, F, 64, ws.p, s), tag)
            torch.cuda.synchronize()
            ws.ok(tag)
            for k in G:
                got[k] = _buf(G[k], tag)
    else:
        from mmrec_amd import hip_ops
        g = ax["grads"]
        dev = torch.device("cuda:0")
        X = torch.from_numpy(a["X"]).to(dev).requires_grad_(g in ("x", "all"))
        if ax["W_view"]:
            base = torch.from_numpy(np.ascontiguousarray(a["W"].T)).to(dev).requires_grad_(g in ("w", "wb", "all"))
            W = base.t()
            assert not W.is_contiguous()
        else:
            base = W = torch.from_numpy(a["W"]).to(dev).requires_grad_(g in ("w", "wb", "all"))
        b = torch.from_numpy(a["b"]).to(dev).requires_grad_(g in ("wb", "all")) if ax["b"] else None
        Y = hip_ops.linear(X, W, b)
        Y.backward(torch.from_numpy(a["dY"]).to(dev))
        torch.cuda.synchronize()
        got["Y"] = pack(Y.detach().cpu().numpy())
        if g in ("x", "all"):
            got["dX"] = pack(X.grad.cpu().numpy())
        if g in ("w", "wb", "all"):
            got["dW"] = pack((base.grad.t() if ax["W_view"] else base.grad).contiguous().cpu().numpy())
        if g in ("wb", "all"):
            got["db"] = pack(b.grad.cpu().numpy())
        assert (X.grad is None) == (g not in ("x", "all")) and (base.grad is None) == (g == "x"), tag
    return got


def _run_and_check(seed):
    c = draw_case(seed)
    worst = check_case(c, run_gpu(c))
    print("gemm fuzz %s: worst err / bound %.3e" % (c.tag(), worst))
    return c


def _seeds(op):
    return range(FIRST[op], FIRST[op] + COUNT[op])


@pytest.mark.gpu
@pytest.mark.parametrize("seed", _seeds("gemm_nt"))
def test_gemm_nt_fuzz(seed):
    _run_and_check(seed)


@pytest.mark.gpu
@pytest.mark.parametrize("seed", _seeds("bwd_w_wide"))
def test_bwd_w_wide_fuzz(seed):
    _run_and_check(seed)                                    # (n = 0: the reference of an empty contraction is zeros, which must be WRITTEN over the sentinel)


@pytest.mark.gpu
@pytest.mark.parametrize("seed", _seeds("dense64_raw"))
def test_dense64_raw_fuzz(seed):
    _run_and_check(seed)


@pytest.mark.gpu
@pytest.mark.parametrize("seed", _seeds("wide_autograd"))
def test_wide_autograd_fuzz(seed):
    """hip_ops.linear with out > 64 against float64 autograd of F.linear, which must agree with the formulas the bounds are built on"""
    c = _run_and_check(seed)
    if c.mode == "float" and not _finite(c):
        return
    a, ax = c.arr, c.axes
    X, W, b = (torch.from_numpy(a[k].astype(F64)).requires_grad_() for k in ("X", "W", "b"))
    Y = torch.nn.functional.linear(X, W, b if ax["b"] else None)
    Y.backward(torch.from_numpy(a["dY"].astype(F64)))
    auto = {"Y": Y.detach(), "dX": X.grad, "dW": W.grad, "db": b.grad}
    for o in c.outs:
        ref, mag, _ = reference(o)
        want = auto[o.name].numpy().reshape(ref.shape)
        assert (np.abs(want - ref) <= 1e-11 * mag).all(), (c.tag(), o.name, "float64 autograd and the header's formula differ")


@pytest.mark.gpu
def test_wide_linear_wants_a_multiple_of_32_columns():
    from mmrec_amd import _lib as L, hip_ops
    dev = torch.device("cuda:0")
    for F, out in ((36, 128), (100, 256), (4, 384)):
        with pytest.raises(L.MMRecHipError):
            hip_ops.linear(torch.zeros(5, F, device=dev), torch.zeros(out, F, device=dev), None)


REPEAT = [s for op in OPS for s in (FIRST[op] + 5, FIRST[op] + 13, FIRST[op] + COUNT[op] - 1)] + \
         [_find(lambda op, m, ax: op == "bwd_w_wide" and ax["n"] >= 2049 and ax["out"] > 64),
          _find(lambda op, m, ax: op == "dense64_raw" and ax.get("want") == "all" and ax["F"] % 128 == 0 and ax["n"] >= 127)]


@pytest.mark.gpu
@pytest.mark.parametrize("seed", sorted(set(REPEAT)))
def test_two_calls_give_the_same_bits(seed):
    """the header: deterministic, no float atomics"""
    c = draw_case(seed)
    one, two = run_gpu(c), run_gpu(c)
    for k in one:
        assert np.array_equal(one[k].view(np.int32), two[k].view(np.int32)), (c.tag(), k)


def _sentinels(*sizes):
    return [Guarded(n, fill=SENTINEL) for n in sizes]


def _untouched(bufs, what):
    torch.cuda.synchronize()
    for g in bufs:
        assert (g.get(what) == F32(SENTINEL)).all(), (what, "an output was written")


@pytest.mark.gpu
def test_argument_errors_before_any_launch():
    """the return codes of the two entry points in the order the code checks them (include/mmrec_hip.h); nothing is launched"""
    lib, s = _lib_stream()
    M, N, K = 5, 96, 64
    A, B, bias = _in(np.ones((M, K), F32)), _in(np.ones((N, K), F32)), _in(np.ones(N, F32))
    C, = _sentinels(M * (N + 8))

    def gemm(A_=A, B_=B, C_=C.view, M_=M, N_=N, K_=K, ldc=N + 8):
        rc = lib.mmrec_gemm_nt_f32(P(A_), P(B_), P(bias), P(C_), M_, N_, K_, ldc, s)
        _untouched([C], "gemm_nt misuse")
        return rc
    assert gemm(K_=0) == ERR_UNSUPPORTED and gemm(K_=-32) == ERR_UNSUPPORTED and gemm(K_=48) == ERR_UNSUPPORTED
    assert gemm(N_=0) == ERR_UNSUPPORTED and gemm(N_=-1) == ERR_UNSUPPORTED
    assert gemm(ldc=N - 1) == ERR_UNSUPPORTED and gemm(ldc=(1 << 21) + 1) == ERR_UNSUPPORTED
    assert gemm(K_=48, M_=-1) == ERR_UNSUPPORTED and gemm(K_=48, A_=None) == ERR_UNSUPPORTED      # the shape is looked at first
    assert gemm(M_=-1) == ERR_BAD_ARG and gemm(M_=-1, A_=None) == ERR_BAD_ARG
    assert gemm(M_=0) == 0 and gemm(M_=0, A_=None, B_=None, C_=None) == 0                        # nothing to do comes before the pointers
    assert gemm(A_=None) == ERR_BAD_ARG and gemm(B_=None) == ERR_BAD_ARG and gemm(C_=None) == ERR_BAD_ARG
    n, F, out = 40, 96, 128
    dY, X = _in(np.ones((n, out), F32)), _in(np.ones((n, F), F32))
    dW, db = _sentinels(out * F, out)
    ws = Workspace(lib.mmrec_linear_workspace_bytes(n, F, out))

    def bww(dY_=dY, X_=X, dW_=dW.view, db_=db.view, n_=n, F_=F, out_=out, ws_=ws.p):
        rc = lib.mmrec_linear_bwd_w_f32(P(dY_), P(X_), P(dW_), P(db_), n_, F_, out_, ws_, s)
        _untouched([dW, db], "bwd_w misuse")
        return rc
    assert bww(out_=96) == ERR_UNSUPPORTED and bww(out_=0) == ERR_UNSUPPORTED and bww(out_=-64) == ERR_UNSUPPORTED
    assert bww(F_=98) == ERR_UNSUPPORTED and bww(F_=0) == ERR_UNSUPPORTED
    assert bww(out_=96, n_=-1) == ERR_UNSUPPORTED and bww(F_=98, dW_=None) == ERR_UNSUPPORTED
    assert bww(n_=-1) == ERR_BAD_ARG and bww(dW_=None) == ERR_BAD_ARG and bww(n_=0, dW_=None) == ERR_BAD_ARG
    assert bww(dY_=None) == ERR_BAD_ARG and bww(X_=None) == ERR_BAD_ARG and bww(ws_=None) == ERR_BAD_ARG
    ws.ok("bwd_w misuse")
    # n = 0: zeros, from NULL inputs and a NULL workspace too
    assert lib.mmrec_linear_bwd_w_f32(None, None, P(dW.view), P(db.view), 0, F, out, None, s) == 0
    torch.cuda.synchronize()
    assert (dW.get("n = 0") == 0).all() and (db.get("n = 0") == 0).all()


@pytest.mark.gpu
@pytest.mark.parametrize("F", [96, 128])
def test_bwd_split_db_without_dw_is_an_error(F):
    """`db` without `dW` is MMREC_ERR_BAD_ARG on the shapes the split kernels serve (F % 128 == 0) AND on those handed to the fp32
    entry points (F = 96: this returned 0 there, with or without a dX, and left db unwritten -- the regression case), before
    anything is launched"""
    lib, s = _lib_stream()
    n = 33
    dY, X, W = _in(np.ones((n, 64), F32)), _in(np.ones((n, F), F32)), _in(np.ones((64, F), F32))
    db, dX = _sentinels(64, n * F)
    ws = Workspace(lib.mmrec_linear_bwd_split_workspace_bytes(n, F, 64))
    for dx in (None, dX.view):
        assert lib.mmrec_linear_bwd_split_f32(P(dY), P(X), P(W), None, P(db.view), P(dx), n, F, 64, ws.p, s) == ERR_BAD_ARG
        _untouched([db, dX], "db without dW")
    # nothing wanted at all is not an error and writes nothing
    assert lib.mmrec_linear_bwd_split_f32(P(dY), P(X), P(W), None, None, None, n, F, 64, ws.p, s) == 0
    _untouched([db, dX], "nothing wanted")
    ws.ok("db without dW")
