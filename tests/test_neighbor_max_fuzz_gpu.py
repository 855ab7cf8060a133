"""GPU: seeded differential fuzz of the neighbour max (csrc/neighbor_max.hip, mmrec_neighbor_max_f32 / _bwd_f32,
hip_ops.neighbor_max) through the raw C ABI over sentinel-guarded outputs, against a numpy restatement of the contract
(`rule_np`, `bwd64`) -- never against another form of the kernel.

THE SELECTION RULE: per (row, column) the chosen slot is the first in CSR order whose value is NaN; without a NaN the first in
CSR order that attains the maximum (-0 = +0).  Y holds the chosen value's BITS and arg the slot's position in the caller's
order; a row without present entries: Y = 0, arg = -1.  So the forward has no tolerance: Y must be bit-equal and arg equal.
  ties    values are multiples of 1/8 in [-2, 2] over a small table with NaN, +-inf and +-0 planted: almost every maximum is
          shared, and "whichever lane held it" cannot pass;
  normal  tie-free normal floats.
Backward, dX[s][c] = base[s][c] + sum of dY[r][c] over the slots of column s whose position arg[r][c] names:
  exact   dY and the base are multiples of 1/8 of magnitude <= 1: every partial sum is a multiple of 1/8 below 2^16 (columns of
          <= 40,000 entries), so dX must EQUAL float64;
  float   normal dY: |dX - ref| <= gamma(m) sum |terms|, m = the number of terms the element receives, the base among them
          (m terms are added with at most m - 1 roundings each, whatever the order).
`arg` of the backward cases is drawn, not computed: every (r, c) names a random slot of row r, or nothing, or a slot of
another row (which no slot of row r matches) -- the formula as written, independent of the forward.  The wrapper test then
runs forward and backward together against `hip_ops.neighbor_max_torch`.

The checker tests (`test_checker_rejects_planted_errors`, `test_cases_span_every_axis`, `test_draw_case_is_deterministic`)
need no GPU."""
import ctypes
import os

import numpy as np
import pytest
import torch

from tests.test_spmm_fuzz_gpu import _on, gamma

CASES = 28
LAYOUTS = ("lens", "hub3000", "hub40000", "one_row", "many", "dup", "oob")
SENTINEL = 0x7FC12345                          # a NaN no arithmetic produces and no case plants: "never written"
ARG_SENTINEL = -7777
GUARD = 64
D = 64
BAD_ARG, UNSUPPORTED = 10001, 10002


def group_max():
    from mmrec_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        from mmrec_amd.build import build
        build(verbose=False)
    return int(_lib.load().mmrec_neighbor_max_group_max())


def axis_lens():
    gm = group_max()
    return (0, 1, 2, 15, 16, 17, 63, 64, 65, gm - 1, gm, gm + 1, 1025)


# ------------------------------------------------------------------------------------------------ host references
def _present(ids, n_ids, pos, n_edges):
    return (ids >= 0) & (ids < n_ids) & (pos >= 0) & (pos < n_edges)


def rule_np(X, rowptr, colidx, perm, n_edges, *, last=False, ignore_perm=False, lose=None):
    """The contract restated row by row; -> (Y [n_rows, 64] fp32, arg [n_rows, 64] int32).  The keywords plant errors
    (test_checker_rejects_planted_errors): `last` the last instead of the first of tied entries, `ignore_perm` the CSR slot
    reported as the position, `lose` one CSR slot left out."""
    n_rows = rowptr.size - 1
    Y, arg = np.zeros((n_rows, D), np.float32), np.full((n_rows, D), -1, np.int32)
    col = np.arange(D)
    for r in range(n_rows):
        j = np.arange(rowptr[r], rowptr[r + 1])
        if lose is not None:
            j = j[j != lose]
        if not j.size:
            continue
        c = colidx[j].astype(np.int64)
        p = j.astype(np.int64) if perm is None else perm[j]
        ok = _present(c, X.shape[0], p, n_edges)
        if not ok.any():
            continue
        c, p, j = c[ok], p[ok], j[ok]
        m = X[c]
        isn = np.isnan(m)
        top = np.where(isn, -np.inf, m).max(0)
        cand = np.where(isn.any(0)[None, :], isn, m == top[None, :])
        first = (cand.shape[0] - 1 - np.argmax(cand[::-1], 0)) if last else np.argmax(cand, 0)     # argmax: the first True
        Y[r] = m[first, col]
        arg[r] = (j if ignore_perm else p)[first]
    return Y, arg


def bwd64(c, arg, dY, base):
    """float64 of the backward's sum; -> (ref, sum |terms|, number of terms) [n_cols, 64]"""
    jt = np.arange(c.ne)
    s = np.repeat(np.arange(c.n_seg), c.lens)                          # the column of transposed slot jt
    r = c.other[jt].astype(np.int64)
    p = jt.astype(np.int64) if c.perm is None else c.perm[jt]
    ok = _present(r, c.n_other, p, c.ne)
    s, r, p = s[ok], r[ok], p[ok]
    hit = arg[r] == p[:, None]                                         # [slots, 64]
    flat = (s[:, None] * D + np.arange(D)[None, :])[hit]
    terms = dY[r].astype(np.float64)[hit]
    size = c.n_seg * D
    ref = np.bincount(flat, weights=terms, minlength=size).reshape(c.n_seg, D)
    mag = np.bincount(flat, weights=np.abs(terms), minlength=size).reshape(c.n_seg, D)
    cnt = np.bincount(flat, minlength=size).reshape(c.n_seg, D).astype(np.float64)
    if base is not None:
        ref, mag, cnt = ref + base, mag + np.abs(base), cnt + 1
    return ref, mag, cnt


def check_fwd(Y, arg, want_Y, want_arg, name=""):
    Y, arg = np.asarray(Y), np.asarray(arg)
    bad = arg != want_arg
    assert not bad.any(), (name, "arg", int(bad.sum()), "first at", np.argwhere(bad)[0].tolist(),
                           int(arg[tuple(np.argwhere(bad)[0])]), int(want_arg[tuple(np.argwhere(bad)[0])]))
    bad = Y.view(np.int32) != want_Y.view(np.int32)
    assert not bad.any(), (name, "Y bits", int(bad.sum()), "first at", np.argwhere(bad)[0].tolist())


def check_bwd(dX, c, arg, dY, base, name=""):
    ref, mag, cnt = bwd64(c, arg, dY, base)
    got = np.asarray(dX, np.float64)
    if c.exact:
        bad = got != ref
        assert not bad.any(), (name, "exact mismatch", int(bad.sum()), "first at", np.argwhere(bad)[0].tolist())
        return 0.0
    err, tol = np.abs(got - ref), gamma(cnt) * mag
    viol = err > tol
    assert not viol.any(), (name, "beyond the bound", int(viol.sum()), "first at", np.argwhere(viol)[0].tolist())
    return float((err[tol > 0] / tol[tol > 0]).max(initial=0.0))


# ------------------------------------------------------------------------------------------------ cases
class Case:
    """One CSR: `lens` entries per segment (rows in the forward, COLUMNS of the transposed CSR in the backward: the same set
    of layouts serves both passes), `other` the id on the other side of every slot, `perm` slot -> position or None."""


def _seg_lens(layout, rng, k):
    al = axis_lens()
    small = lambda n: rng.integers(0, 40, n)
    if layout == "lens":
        return np.concatenate([[0, 0], rng.permutation(al), [0]])
    if layout == "hub3000":
        return np.concatenate([small(30), [3000], small(30)])
    if layout == "hub40000":
        return np.concatenate([small(20), [40000], small(20), [group_max() + 1]])
    if layout == "one_row":
        return np.array([al[1:][k % (len(al) - 1)]])
    if layout == "many":                                              # several workgroups of short rows, a few long ones
        lens = rng.geometric(0.08, 3000) - 1
        lens[rng.integers(0, 3000, 5)] = group_max() + rng.integers(1, 400, 5)
        return lens
    lens = small(120)                                                 # "dup", "oob"
    lens[[0, -1]] = 0
    lens[60], lens[61] = group_max() + 3, 700
    return lens


def draw_case(seed):
    rng = np.random.default_rng(9100 + seed)
    c = Case()
    c.seed = seed
    c.layout = LAYOUTS[seed % len(LAYOUTS)]
    c.exact = (seed // len(LAYOUTS)) % 2 == 0                         # forward: tie-heavy values; backward: exact sums
    c.shuffled = (seed // (2 * len(LAYOUTS))) % 2 == 1
    lens = np.asarray(_seg_lens(c.layout, rng, seed // len(LAYOUTS)), np.int64)
    c.lens, c.n_seg, c.ne = lens, lens.size, int(lens.sum())
    c.rowptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    c.n_other = 5 if c.layout == "dup" else int(rng.choice([37, 300]))    # "dup": every long row repeats each id many times
    c.other = rng.integers(0, c.n_other, c.ne).astype(np.int32)
    c.perm = rng.permutation(c.ne).astype(np.int64) if c.shuffled else None
    if c.layout == "oob" and c.ne:                                    # absent edges: ids and positions outside their ranges
        hit = rng.random(c.ne) < 0.1
        c.other[hit] = rng.choice([-1, c.n_other, c.n_other + 5, -2 ** 31, 2 ** 31 - 1], int(hit.sum()))
        first = int(c.rowptr[60])
        c.other[first:first + 3] = [c.n_other, 0, -1]                 # ... at the head of a long row too
        if c.perm is not None:
            hit = rng.random(c.ne) < 0.1
            c.perm[hit] = rng.choice([-1, c.ne, c.ne + 1, 2 ** 40, -2 ** 40], int(hit.sum()))
    # forward: the gathered table
    if c.exact:
        X = (rng.integers(-16, 17, (c.n_other, D)) / 8.0).astype(np.float32)
        for v in (np.nan, np.inf, -np.inf, -0.0):
            X[rng.random(X.shape) < 0.01] = v
    else:
        X = rng.standard_normal((c.n_other, D)).astype(np.float32)
    c.X = X
    # backward: the other side's rows of arg and dY, the base
    n_r = c.n_other
    if c.exact:
        c.dY = (rng.integers(-8, 9, (n_r, D)) / 8.0).astype(np.float32)
        c.base = (rng.integers(-8, 9, (c.n_seg, D)) / 8.0).astype(np.float32)
    else:
        c.dY = rng.standard_normal((n_r, D)).astype(np.float32)
        c.base = rng.standard_normal((c.n_seg, D)).astype(np.float32)
    pos = np.arange(c.ne, dtype=np.int64) if c.perm is None else c.perm
    ok = _present(c.other.astype(np.int64), n_r, pos, c.ne)
    arg = np.full((n_r, D), -1, np.int32)
    if ok.any():
        order = np.argsort(c.other[ok], kind="stable")
        by_row, deg = pos[ok][order], np.bincount(c.other[ok], minlength=n_r)
        start = np.concatenate([[0], np.cumsum(deg)])[:-1]
        pick = start[:, None] + (rng.random((n_r, D)) * deg[:, None]).astype(np.int64)
        has = np.broadcast_to(deg[:, None] > 0, (n_r, D))
        arg[has] = by_row[pick[has]].astype(np.int32)
        wild = rng.random((n_r, D))
        arg[wild < 0.05] = -1
        other_row = wild > 0.95                                       # a position that is some OTHER row's (or this row's: fine)
        arg[other_row] = by_row[rng.integers(0, by_row.size, int(other_row.sum()))].astype(np.int32)
    c.arg = arg
    return c


_CASES, _RULE = {}, {}


def case(seed):
    """the cases are drawn once and shared; nothing changes them"""
    if seed not in _CASES:
        _CASES[seed] = draw_case(seed)
    return _CASES[seed]


def rule(seed):
    """the forward's expected (Y, arg) of a case: computed once, shared, never changed"""
    if seed not in _RULE:
        c = case(seed)
        _RULE[seed] = rule_np(c.X, c.rowptr, c.other, c.perm, c.ne)
    return _RULE[seed]


# ------------------------------------------------------------------------------------------------ CPU: the checker and the cases
def test_draw_case_is_deterministic():
    a, b = draw_case(9), draw_case(9)
    assert np.array_equal(a.X, b.X, equal_nan=True) and np.array_equal(a.other, b.other) and np.array_equal(a.arg, b.arg)


def test_cases_span_every_axis():
    gm = group_max()
    from mmrec_amd import hip_ops
    assert gm == hip_ops.segment_softmax_group_max()
    seen = {"lens": set(), "combo": set(), "hub": set(), "one_row": set()}
    ties = pairs = 0
    for s in range(CASES):
        c = case(s)
        seen["lens"].update(int(x) for x in c.lens)
        seen["combo"].add((c.layout, c.exact, c.shuffled))
        if c.lens.max(initial=0) >= 3000:
            seen["hub"].add((int(c.lens.max()), c.exact, c.shuffled))
        if c.n_seg == 1:
            seen["one_row"].add(c.ne)
        assert c.rowptr[-1] == c.ne and c.other.size == c.ne
        if c.layout == "lens" and c.exact:                            # how often the maximum is shared by two or more slots
            Y, arg = rule(s)
            for r in np.flatnonzero(c.lens >= 16):
                m = c.X[c.other[c.rowptr[r]:c.rowptr[r + 1]]]
                isn = np.isnan(m)
                ties += int((np.where(isn.any(0), isn.sum(0), (m == Y[r][None, :]).sum(0)) >= 2).sum())
                pairs += D
    assert set(axis_lens()) | {3000, 40000} <= seen["lens"], sorted(seen["lens"])
    assert seen["combo"] == {(l, e, p) for l in LAYOUTS for e in (True, False) for p in (True, False)}
    assert {(h, e, p) for h in (3000, 40000) for e in (True, False) for p in (True, False)} <= seen["hub"]
    assert len(seen["one_row"]) >= 2
    assert pairs >= 1000 and ties > 0.5 * pairs                       # tie-heavy cases: shared maxima (or NaNs) are the norm
    dup = case(LAYOUTS.index("dup"))                                  # duplicate edges: a long row over 5 ids
    assert dup.n_other == 5 and dup.lens[60] == gm + 3
    oob = next(case(s) for s in range(CASES) if case(s).layout == "oob" and case(s).shuffled)
    assert (oob.other < 0).any() and (oob.other >= oob.n_other).any() and (oob.perm < 0).any() and (oob.perm >= oob.ne).any()
    nonfinite = case(0).X
    assert np.isnan(nonfinite).any() and np.isinf(nonfinite).any() and (np.signbit(nonfinite) & (nonfinite == 0)).any()


def test_checker_rejects_planted_errors():
    s = next(s for s in range(CASES) if case(s).layout == "lens" and case(s).exact and case(s).shuffled)
    c = case(s)
    Y, arg = rule(s)
    check_fwd(Y.copy(), arg.copy(), Y, arg, "clean")
    with pytest.raises(AssertionError):                               # the last instead of the first of tied entries
        check_fwd(*rule_np(c.X, c.rowptr, c.other, c.perm, c.ne, last=True), Y, arg)
    with pytest.raises(AssertionError):                               # perm ignored: the CSR slot for the position
        check_fwd(*rule_np(c.X, c.rowptr, c.other, c.perm, c.ne, ignore_perm=True), Y, arg)
    r = int(np.flatnonzero(c.lens == 17)[0])                          # an entry lost: the one column 0 of a 17-entry row chose
    inv = np.empty(c.ne, np.int64)
    inv[c.perm] = np.arange(c.ne)
    with pytest.raises(AssertionError):
        check_fwd(*rule_np(c.X, c.rowptr, c.other, c.perm, c.ne, lose=int(inv[arg[r, 0]])), Y, arg)
    flipped = Y.copy()                                                # -0 for +0: the bits, not the value
    z = np.argwhere(Y == 0)[0]
    flipped[tuple(z)] = -Y[tuple(z)]
    with pytest.raises(AssertionError):
        check_fwd(flipped, arg, Y, arg)
    # backward, exact and float: clean passes; a term lost, a term taken from the wrong position, the base forgotten do not
    for s in (s, next(s for s in range(CASES) if case(s).layout == "many" and not case(s).exact and case(s).shuffled)):
        c = case(s)
        ref, mag, cnt = bwd64(c, c.arg, c.dY, c.base)
        assert check_bwd(ref.astype(np.float32), c, c.arg, c.dY, c.base, "clean bwd") <= 1.0
        col = np.argwhere((cnt >= 3) & (mag > 0.5))[0]
        bad = ref.copy()
        bad[tuple(col)] -= mag[tuple(col)] / cnt[tuple(col)]
        with pytest.raises(AssertionError):
            check_bwd(bad.astype(np.float32), c, c.arg, c.dY, c.base)
        with pytest.raises(AssertionError):
            check_bwd(bwd64(c, c.arg, c.dY, None)[0].astype(np.float32), c, c.arg, c.dY, c.base)
        slot_as_pos = Case()
        slot_as_pos.__dict__.update(c.__dict__)
        slot_as_pos.perm = None
        with pytest.raises(AssertionError):
            check_bwd(bwd64(slot_as_pos, c.arg, c.dY, c.base)[0].astype(np.float32), c, c.arg, c.dY, c.base)


# ------------------------------------------------------------------------------------------------ GPU: the raw C ABI, guarded
class _Dev:
    def __init__(self, c):
        from mmrec_amd import hip_ops
        self.rowptr, self.other = _on(c.rowptr), _on(c.other)
        self.perm = None if c.perm is None else _on(c.perm)
        lr = hip_ops.segment_long_rows(c.rowptr)
        self.long, self.n_long = (_on(lr), lr.size) if lr.size else (None, 0)


def _guarded(n_rows, fill, dtype):
    buf = torch.full((n_rows * D + 2 * GUARD,), fill, dtype=torch.int32, device="cuda:0")
    return buf, buf[GUARD:GUARD + n_rows * D].view(dtype).view(n_rows, D)


def _guards_ok(buf, n_rows, fill, name):
    b = buf.cpu().numpy()
    assert (b[:GUARD] == fill).all() and (b[GUARD + n_rows * D:] == fill).all(), (name, "wrote outside the output")
    assert not (b[GUARD:GUARD + n_rows * D] == fill).any(), (name, "elements never written")


def raw_fwd(c, dev, X, with_list, name="fwd"):
    from mmrec_amd import hip_ops
    p, lib = hip_ops._p, hip_ops._lib.load()
    ybuf, Y = _guarded(c.n_seg, SENTINEL, torch.float32)
    abuf, arg = _guarded(c.n_seg, ARG_SENTINEL, torch.int32)
    rc = lib.mmrec_neighbor_max_f32(p(dev.rowptr), c.n_seg, p(dev.other), p(dev.perm), p(dev.long) if with_list else None,
                                    dev.n_long if with_list else 0, p(X), c.n_other, D, c.ne,
                                    ctypes.c_void_p(Y.data_ptr()), ctypes.c_void_p(arg.data_ptr()), hip_ops._stream())
    assert rc == 0, (name, rc)
    torch.cuda.synchronize()
    _guards_ok(ybuf, c.n_seg, SENTINEL, name + " Y")
    _guards_ok(abuf, c.n_seg, ARG_SENTINEL, name + " arg")
    return Y, arg


def raw_bwd(c, dev, arg, dY, base, with_list, name="bwd"):
    from mmrec_amd import hip_ops
    p, lib = hip_ops._p, hip_ops._lib.load()
    buf, dX = _guarded(c.n_seg, SENTINEL, torch.float32)
    rc = lib.mmrec_neighbor_max_bwd_f32(p(dev.rowptr), c.n_seg, p(dev.other), p(dev.perm), p(dev.long) if with_list else None,
                                        dev.n_long if with_list else 0, p(arg), c.n_other, p(dY), D, c.ne,
                                        ctypes.c_void_p(dX.data_ptr()), p(base), hip_ops._stream())
    assert rc == 0, (name, rc)
    torch.cuda.synchronize()
    _guards_ok(buf, c.n_seg, SENTINEL, name)
    return dX


@pytest.mark.gpu
@pytest.mark.parametrize("seed", range(CASES))
def test_neighbor_max_fuzz(seed):
    c = case(seed)
    dev = _Dev(c)
    assert (dev.n_long > 0) == bool((c.lens > group_max()).any())
    X, arg_in, dY, base = _on(c.X), _on(c.arg), _on(c.dY), _on(c.base)
    want_Y, want_arg = rule(seed)
    worst = 0.0
    for with_list in (True, False):                                   # the same graph with the lists and with n_long = 0
        tag = "seed %d %s" % (seed, "list" if with_list else "n_long = 0")
        Y, arg = raw_fwd(c, dev, X, with_list, "fwd " + tag)
        check_fwd(Y.cpu().numpy(), arg.cpu().numpy(), want_Y, want_arg, "fwd " + tag)
        for b in (base, None):                                        # the column pass: the same CSR as the transposed one
            dX = raw_bwd(c, dev, arg_in, dY, b, with_list, "bwd " + tag)
            worst = max(worst, check_bwd(dX.cpu().numpy(), c, c.arg, c.dY, None if b is None else c.base, "bwd " + tag))
    print("neighbor_max fuzz seed %d: %s %s %s segments %d edges %d longest %d worst bwd err / bound %.3f" % (
        seed, c.layout, "ties / exact" if c.exact else "normal / float", "shuffled" if c.shuffled else "csr order", c.n_seg,
        c.ne, int(c.lens.max(initial=0)), worst))


def _wrapper_graph(c):
    """a DynGraph over the case's present edges, rows = the segments"""
    from mmrec_amd import hip_ops
    seg = np.repeat(np.arange(c.n_seg), c.lens)
    order = np.arange(c.ne) if c.perm is None else np.argsort(c.perm, kind="stable")       # the caller's (COO) order
    return hip_ops.DynGraph(_on(seg[order].astype(np.int64)), _on(c.other[order].astype(np.int64)), c.n_seg, c.n_other)


@pytest.mark.gpu
@pytest.mark.parametrize("layout", ["lens", "hub3000", "dup"])
def test_wrapper_against_the_composition(layout):
    """forward + backward through hip_ops.neighbor_max on tie-heavy values against `neighbor_max_torch` on the same device
    tensors: the same arg everywhere, the same Y bits, and (dY in eighths: exact sums) the same dX"""
    from mmrec_amd import hip_ops
    seed = next(s for s in range(CASES) if case(s).layout == layout and case(s).exact and case(s).shuffled)
    c = case(seed)
    dyn = _wrapper_graph(c)
    dY = _on((np.random.default_rng(seed).integers(-8, 9, (c.n_seg, D)) / 8.0).astype(np.float32))
    out = []
    for served in (True, False):
        X = _on(c.X).requires_grad_()
        if served:
            assert hip_ops.neighbor_max_served(X, dyn)
            Y, arg = hip_ops.neighbor_max(X, dyn)
        else:
            Y, arg = hip_ops.neighbor_max_torch(X, dyn.rows, dyn.cols, dyn.n_rows)
        assert not arg.requires_grad and arg.dtype == torch.int32
        Y.backward(dY)
        torch.cuda.synchronize()
        out.append((Y.detach(), arg, X.grad))
    (Y1, a1, g1), (Y2, a2, g2) = out
    assert torch.equal(a1, a2) and torch.equal(Y1.view(torch.int32), Y2.view(torch.int32))
    finite = torch.isfinite(g2)                                       # (a planted NaN / inf never reaches dX: dY is finite)
    assert finite.all() and torch.equal(g1, g2) and float(g1.abs().max()) > 0
    # the values of the rule (the DynGraph orders a row's slots by position, the case by slot: the sign of a zero may differ)
    assert np.array_equal(Y1.cpu().numpy(), rule(seed)[0], equal_nan=True)


@pytest.mark.gpu
def test_hub_repeats_bit_for_bit():
    c = next(case(s) for s in range(CASES) if case(s).layout == "hub40000" and not case(s).exact and case(s).shuffled)
    dev = _Dev(c)
    X, arg_in, dY, base = _on(c.X), _on(c.arg), _on(c.dY), _on(c.base)
    for with_list in (True, False):
        a, b = raw_fwd(c, dev, X, with_list), raw_fwd(c, dev, X, with_list)
        assert torch.equal(a[0].view(torch.int32), b[0].view(torch.int32)) and torch.equal(a[1], b[1])
        a, b = raw_bwd(c, dev, arg_in, dY, base, with_list), raw_bwd(c, dev, arg_in, dY, base, with_list)
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.mark.gpu
def test_tie_rule_by_hand_on_the_kernel():
    """tests/test_neighbor_max_cpu.py's hand-written case through the wrapper"""
    from mmrec_amd import hip_ops
    from tests.test_neighbor_max_cpu import check_tie_case, tie_case
    X, rows, cols, want_src = tie_case()
    dY = (np.arange(3 * 64).reshape(3, 64) % 17 - 8).astype(np.float32) / 8.0
    dyn = hip_ops.DynGraph(_on(rows), _on(cols), 3, 6)
    Xt = _on(X).requires_grad_()
    assert hip_ops.neighbor_max_served(Xt, dyn)
    Y, arg = hip_ops.neighbor_max(Xt, dyn)
    Y.backward(_on(dY))
    check_tie_case(Y.detach().cpu().numpy(), arg.cpu().numpy(), Xt.grad.cpu().numpy(), X, rows, cols, want_src, dY)


@pytest.mark.gpu
def test_argument_errors():
    from mmrec_amd import hip_ops
    p, lib, st = hip_ops._p, hip_ops._lib.load(), hip_ops._stream()
    c = case(LAYOUTS.index("dup"))
    dev = _Dev(c)
    X, arg_in, dY = _on(c.X), _on(c.arg), _on(c.dY)
    Y = torch.zeros(c.n_seg, D, device="cuda:0")
    arg = torch.zeros(c.n_seg, D, dtype=torch.int32, device="cuda:0")
    dX = torch.zeros(c.n_seg, D, device="cuda:0")

    def fwd(rowptr=dev.rowptr, n_rows=c.n_seg, col=dev.other, lst=dev.long, n_long=dev.n_long, x=X, n_x=c.n_other, d=D,
            ne=c.ne, y=Y, a=arg):
        return lib.mmrec_neighbor_max_f32(p(rowptr), n_rows, p(col), p(dev.perm), p(lst), n_long, p(x), n_x, d, ne, p(y), p(a), st)

    def bwd(rowptr=dev.rowptr, n_cols=c.n_seg, row=dev.other, lst=dev.long, n_long=dev.n_long, a=arg_in, n_rows=c.n_other,
            dy=dY, d=D, ne=c.ne, dx=dX, base=None):
        return lib.mmrec_neighbor_max_bwd_f32(p(rowptr), n_cols, p(row), p(dev.perm), p(lst), n_long, p(a), n_rows, p(dy), d,
                                              ne, p(dx), p(base), st)
    assert fwd() == 0 and bwd() == 0
    assert fwd(d=32) == UNSUPPORTED and fwd(d=128) == UNSUPPORTED and bwd(d=32) == UNSUPPORTED
    assert fwd(d=32, n_rows=-1) == UNSUPPORTED                         # the documented order
    assert fwd(n_rows=-1) == BAD_ARG and fwd(ne=-1) == BAD_ARG and fwd(n_long=-1) == BAD_ARG and fwd(n_x=-1) == BAD_ARG
    assert fwd(n_rows=0, rowptr=None, y=None, a=None) == 0
    assert fwd(ne=2 ** 31) == UNSUPPORTED and fwd(n_x=2 ** 31) == UNSUPPORTED
    assert fwd(rowptr=None) == BAD_ARG and fwd(y=None) == BAD_ARG and fwd(a=None) == BAD_ARG
    assert fwd(col=None) == BAD_ARG and fwd(x=None) == BAD_ARG and fwd(lst=None) == BAD_ARG
    assert bwd(n_cols=-1) == BAD_ARG and bwd(ne=-1) == BAD_ARG and bwd(n_long=-1) == BAD_ARG and bwd(n_rows=-1) == BAD_ARG
    assert bwd(n_cols=0, rowptr=None, dx=None) == 0
    assert bwd(ne=2 ** 31) == UNSUPPORTED and bwd(n_rows=2 ** 31) == UNSUPPORTED
    assert bwd(rowptr=None) == BAD_ARG and bwd(dx=None) == BAD_ARG and bwd(base=dX) == BAD_ARG
    assert bwd(row=None) == BAD_ARG and bwd(a=None) == BAD_ARG and bwd(dy=None) == BAD_ARG and bwd(lst=None) == BAD_ARG
    torch.cuda.synchronize()
    # rows and no edges: Y = 0 and arg = -1 are written
    zero = _on(np.zeros(c.n_seg + 1, np.int32))
    Y.fill_(7.0), arg.fill_(7)
    assert fwd(rowptr=zero, col=None, x=None, lst=None, n_long=0, ne=0) == 0
    torch.cuda.synchronize()
    assert (Y == 0).all() and (arg == -1).all()
