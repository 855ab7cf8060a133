"""GPU: seeded differential fuzz of the fused edge attention backward (csrc/edge_attention.hip, mmrec_edge_attention_bwd_f32,
hip_ops.edge_attention(fused_backward=True)) against float64 autograd of the three formulas (`autograd64`, which is `grads64` of
tests/test_edge_attention_fuzz_gpu.py with the score's gradient kept as well), never against another kernel.  The raw C ABI is
called over guarded, sentinel-filled outputs; its alpha and Y are what the FORWARD kernel left for the same case.

With row r, slot j at caller position p, column c = colidx[j], alpha and Y the forward's:
    g_p = <dY[r], KV[c]> + dAlpha[p]      t_r = <dY[r], Y[r]> + sum_p alpha_p dAlpha[p]      ds_p = alpha_p (g_p - t_r)
    dQ[r] = sum_p ds_p KV[c]              dKV[c] = base[c] + sum over the edges of column c of (alpha_p dY[r] + ds_p Q[r])

The kernel's plan and the bound (u = 2^-24, gamma(k) = k u / (1 - k u); everything to first order, times 1 + 2^-10 for the products
of two errors, plus 2^-120 for gradual underflow, as the forward's gradient bound):
  inputs  alpha^, Y^ are the forward's: |alpha^ - alpha| <= ea = alpha rel + 4 * 2^-126 with rel = `forward_rel` under the forward's
          `plan_of`, and |Y^ - Y| <= eY = sum_p ea_p |KV[c_p]| + 2^-140 (that file's acceptance bounds).
  g       4 roundings in a lane's chain + 4 in the butterfly, one more when dAlpha is added:
              eg = gamma(8) sum_i |dY_ri KV_ci| + u |g|
  t       <dY, Y^> the same 8 (+ 1 for the sum of the two parts); the dAlpha part is a chain of fmas per lane -- ceil(len / 16)
          for a group, ceil(len / 256) for a listed row -- 4 butterfly steps, and for a listed row 16 additions in the order of the
          groups: na = ceil(len / 16) + 5, or ceil(len / 256) + 21:
              et = gamma(9) sum_i |dY_ri Y_ri| + sum_i |dY_ri| eY_ri + gamma(na) sum_p alpha_p |dAlpha_p| + sum_p ea_p |dAlpha_p|
  ds      a subtraction and a product:   eds = ea |g - t| + alpha (eg + et) + 2 u alpha |g - t|
  dQ      one fma per slot IN ORDER: n = len for a group; a listed row: 16 ceil(len / 256) in a group's walk + 16 additions of the
          states (`plan_of`'s n):
              |dQ^ - dQ| <= gamma(n + 2) sum_p |ds_p| |KV[c]| + sum_p eds_p |KV[c]|
  dKV     two fmas per slot (+ the base as the first term): nc = 2 len + 1 for a group, 32 ceil(len / 256) + 17 for a listed column:
              |dKV^ - dKV| <= gamma(nc + 2) (|base| + sum (alpha |dY[r]| + |ds| |Q[r]|)) + sum (ea |dY[r]| + eds |Q[r]|)
          (+ the base's own error when the base is the dQ the same call wrote: Q is KV).
The tests without the gpu mark hold the bound honest: an fp32 numpy emulation of both passes (lane chains, butterfly, in-order
walk, 16-state combine) passes the checker, fed with the forward's fp32 emulation; the fp32 torch composition passes it; each
planted error is rejected; and the bound is not vacuous (`test_bound_is_not_vacuous_on_these_cases`: median tol / |want| below
1e-3)."""
import ctypes

import numpy as np
import pytest
import torch

from tests.test_edge_attention_fuzz_gpu import (D, EPS, LAYOUTS, Case, _f32, _finish, _fma, _grad_case, _guarded, _guards_ok,
                                                _row_lens, _rows_sum, _wrapper_graph, attention64, emulate, forward_rel, grads64,
                                                group_max, plan_of, Ref)
from tests.test_edge_attention_fuzz_gpu import raw as raw_forward
from tests.test_edge_softmax_fuzz_gpu import TINY
from tests.test_spmm_fuzz_gpu import U, _on, gamma

IN_MODES = ("Y", "alpha", "both")                 # where the gradient arrives
OUT_MODES = ("dQ", "dKV", "both")                 # what is asked for
BASES = ("none", "array", "dQ")
CASES = 30
FLOOR = 2.0 ** -120
SLACK = 1.0 + 2.0 ** -10
SCORE_STD = (0.5, 1.0, 2.0)                       # of a row's scores
LISTS = ((True, True), (True, False), (False, True), (False, False))      # (row side, column side) with its long list


# ------------------------------------------------------------------------------------------------ cases
def draw_case(seed):
    """a layout of the forward's fuzz as drawn or TRANSPOSED (the layout's lengths are then the columns'), moderate scores (standard
    deviation 0.5 ... 2 per row: neither uniform weights nor one weight of 1, where ds itself is a cancellation), incoming gradients of order 1"""
    rng = np.random.default_rng(9100 + seed)
    c = Case()
    c.seed, c.exact = seed, False
    c.layout = LAYOUTS[seed % len(LAYOUTS)]
    c.transposed = (seed // 5) % 2 == 1
    c.shuffled = (seed // 10) % 2 == 1
    c.use = IN_MODES[seed % 3]
    c.base = BASES[(seed // 2) % 3]
    c.out = "both" if c.base == "dQ" else OUT_MODES[(seed // 3) % 3]
    if c.base != "none" and c.out == "dQ":
        c.base = "none"                                               # (no dKV: no base)
    c.eps = EPS[(seed % 7) % len(EPS)]
    lens = np.asarray(_row_lens(c.layout, rng, seed), np.int64)
    if c.layout == "one_row" and c.transposed:                        # ONE long column among short ones (alone it would leave every
        lens = np.concatenate([lens, rng.integers(0, 40, 24)])        # row a single source: ds = dQ = 0, nothing to compare)
    elif c.layout == "one_row" and c.base == "dQ":
        lens = np.concatenate([lens, np.zeros(24, np.int64)])         # square: the one row, and 24 empty ones
    n_other = 3 if c.layout == "dups" else int(rng.integers(40, 400))
    if c.base == "dQ":
        n_other = lens.size                                           # dQ is the base: a square graph
    ne = int(lens.sum())
    other = rng.integers(0, n_other, ne)
    if c.transposed:                                                  # the layout's rows are this case's COLUMNS
        cnt = np.bincount(other, minlength=n_other)
        _finish(c, rng, cnt, lens.size)
        cols_csr = np.repeat(np.arange(lens.size), lens)[np.argsort(other, kind="stable")]
    else:
        _finish(c, rng, lens, n_other)
        cols_csr = other
    c.colidx = cols_csr.astype(np.int32)
    c.cols = np.empty(ne, np.int64)
    c.cols[c.order] = cols_csr
    std = rng.choice(SCORE_STD, c.n_rows)                       # of a row's scores
    c.KV = rng.standard_normal((c.n_kv, D)).astype(np.float32)
    c.Q = (rng.standard_normal((c.n_rows, D)) * (std / 8.0)[:, None]).astype(np.float32)
    c.dY = rng.standard_normal((c.n_rows, D)).astype(np.float32)
    c.dA = rng.standard_normal(ne).astype(np.float32)
    c.base_arr = rng.standard_normal((c.n_kv, D)).astype(np.float32)
    c.ref = attention64(c.Q, c.KV, c.seg, c.cols, c.n_rows, c.eps)
    col_side(c, rng if c.shuffled else None)
    return c


def col_side(c, rng=None):
    """the transposed CSR of the case's edge list: slot j of column k is the edge at position perm_t[j], its row rowidx_t[j];
    with `rng` the order inside a column is random, else the stable one hip_ops.DynGraph builds"""
    key = rng.random(c.ne) if rng is not None else np.arange(c.ne)
    c.perm_t = np.lexsort((key, c.cols)).astype(np.int64)
    c.lens_t = np.bincount(c.cols, minlength=c.n_kv)
    c.rowptr_t = np.concatenate([[0], np.cumsum(c.lens_t)]).astype(np.int32)
    c.rowidx_t = c.seg[c.perm_t].astype(np.int32)


_CASES = {}


def case(seed):
    """the cases (and their float64 references) are drawn once and shared; nothing changes them"""
    if seed not in _CASES:
        _CASES[seed] = draw_case(seed)
    return _CASES[seed]


def _flags(c, use=None, out=None):
    use, out = use or c.use, out or c.out
    return use in ("Y", "both"), use in ("alpha", "both"), out in ("dQ", "both"), out in ("dKV", "both")


# ------------------------------------------------------------------------------------------------ host references
def autograd64(c, use_y, use_a, base=None, keep=None):
    """float64 autograd of the three formulas over the case's edges (`keep`: only those) -> (ds [ne], dQ, dKV + base); ds is 0
    where an edge is left out"""
    keep = np.ones(c.ne, bool) if keep is None else keep
    seg, cols = torch.from_numpy(c.seg[keep]), torch.from_numpy(c.cols[keep])
    Q = torch.from_numpy(c.Q).double().requires_grad_()
    KV = torch.from_numpy(c.KV).double().requires_grad_()
    s = (Q[seg] * KV[cols]).sum(-1)
    s.retain_grad()
    m = torch.full((c.n_rows,), -np.inf, dtype=torch.float64).scatter_reduce(0, seg, s.detach(), "amax")
    e = (s - m[seg]).exp()
    alpha = e / (torch.zeros(c.n_rows, dtype=torch.float64).index_add_(0, seg, e)[seg] + float(np.float32(c.eps)))
    Y = torch.zeros(c.n_rows, D, dtype=torch.float64).index_add_(0, seg, alpha.unsqueeze(1) * KV[cols])
    out = 0.0
    if use_y:
        out = out + (Y * torch.from_numpy(c.dY).double()).sum()
    if use_a:
        out = out + (alpha * torch.from_numpy(c.dA[keep]).double()).sum()
    out.backward()
    ds = np.zeros(c.ne)
    ds[keep] = s.grad.numpy()
    dKV = KV.grad.numpy() if KV.grad is not None else np.zeros((c.n_kv, D))
    return ds, Q.grad.numpy(), dKV + (0.0 if base is None else base.astype(np.float64))


def formulas64(c, use_y, use_a, base=None, alpha=None, Y=None, plant=None):
    """the kernel's five formulas in float64, from alpha and Y (default: float64's own) -> (ds, dQ, dKV).  `plant`: an error."""
    seg, cols, nr = c.seg, c.cols, c.n_rows
    al = c.ref.alpha if alpha is None else np.asarray(alpha, np.float64)
    Yv = c.ref.Y if Y is None else np.asarray(Y, np.float64)
    KV, Q, dY = c.KV.astype(np.float64), c.Q.astype(np.float64), c.dY.astype(np.float64)
    with np.errstate(invalid="ignore"):
        g, t = np.zeros(c.ne), np.zeros(nr)
        if use_y:
            g = (dY[seg] * KV[cols]).sum(1)
            t = (dY * Yv).sum(1)
        if use_a:
            g = g + c.dA
            w = al * c.dA
            if plant is not None and plant[0] == "drop_t":
                w = w.copy()
                w[plant[1]] = 0.0
            if plant != ("t_without_dA",):
                t = t + _bincount(seg, w, nr)
        elif plant is not None and plant[0] == "drop_t":              # (dY only: the edge's share of <dY, Y>)
            t = t - np.bincount(seg[plant[1]], weights=(al * g)[plant[1]], minlength=nr)
        ds = al * (g - t[seg])
        dQ = _rows_sum(ds, seg, cols, nr, c.KV)
        al_col = al
        if plant == ("alpha_at_perm",):                               # the column pass reads alpha through the ROW side's perm
            al_col = np.empty(c.ne)
            al_col[c.perm_t] = al[c.order]
        dKV = _rows_sum(ds, cols, seg, c.n_kv, c.Q)
        if use_y:
            dKV = dKV + _rows_sum(al_col, cols, seg, c.n_kv, c.dY)
        if base is not None:
            dKV = dKV + base.astype(np.float64) * (2.0 if plant == ("base_twice",) else 1.0)
    if plant == ("ds_csr_order",):
        ds = ds[c.order]
    return ds, dQ, dKV


def _bincount(idx, w, n):
    """np.bincount that lets a NaN through"""
    out = np.zeros(n)
    np.add.at(out, idx, w)
    return out


def _plan_n(lens, with_list):
    """roundings of a term in an in-order walk of one fma per slot (`plan_of`'s n)"""
    lens = np.asarray(lens, np.int64)
    return np.where(with_list & (lens > group_max()), 16 * -(-lens // 256) + 16, lens)


def bwd_bound(c, use_y, use_a, list_row, list_col, base=None, *, base_tol=None, score_n=8, composition=False):
    """(tol ds, tol dQ, tol dKV) of the module docstring; alpha^ and Y^ from a forward WITH its long list (c.order its CSR
    order).  composition: the fp32 torch ops instead of the kernels (dots of 64 products + their sum, serial sums)."""
    seg, cols, nr, ref = c.seg, c.cols, c.n_rows, c.ref
    n_f, R_f = plan_of(c.rowptr, c.order, ref, True, score_n, composition)
    rel = forward_rel(c, ref, n_f, R_f, score_n)
    al = ref.alpha
    ea = al * rel + TINY
    aQ, aKV, adY = (np.abs(x).astype(np.float64) for x in (c.Q, c.KV, c.dY))
    eY = _rows_sum(ea, seg, cols, nr, aKV) + 2.0 ** -140
    KV, dY = c.KV.astype(np.float64), c.dY.astype(np.float64)
    g, eg, t, et = np.zeros(c.ne), np.zeros(c.ne), np.zeros(nr), np.zeros(nr)
    if use_y:
        g = (dY[seg] * KV[cols]).sum(1)
        eg = gamma(score_n) * (adY[seg] * aKV[cols]).sum(1)
        t = (dY * ref.Y).sum(1)
        et = gamma(score_n + 1) * (adY * np.abs(ref.Y)).sum(1) + (adY * eY).sum(1)
    if use_a:
        g = g + c.dA
        eg = eg + U * np.abs(g)
        if composition:
            na = c.lens + 1
        else:
            na = np.where(list_row & (c.lens > group_max()), -(-c.lens // 256) + 21, -(-c.lens // 16) + 5)
        t = t + np.bincount(seg, weights=al * c.dA, minlength=nr)
        et = et + gamma(na) * np.bincount(seg, weights=al * np.abs(c.dA), minlength=nr) + np.bincount(
            seg, weights=ea * np.abs(c.dA), minlength=nr)
    ds = al * (g - t[seg])
    eds = ea * np.abs(g - t[seg]) + al * (eg + et[seg]) + 2 * U * np.abs(ds)
    n_q = (c.lens if composition else _plan_n(c.lens, list_row)) + 2
    tq = gamma(n_q)[:, None] * _rows_sum(np.abs(ds), seg, cols, nr, aKV) + _rows_sum(eds, seg, cols, nr, aKV)
    n_c = 2 * (c.lens_t if composition else _plan_n(c.lens_t, list_col)) + 1 + 2
    mag = _rows_sum(np.abs(ds), cols, seg, c.n_kv, aQ)
    tk = _rows_sum(eds, cols, seg, c.n_kv, aQ)
    if use_y:
        mag = mag + _rows_sum(al, cols, seg, c.n_kv, adY)
        tk = tk + _rows_sum(ea, cols, seg, c.n_kv, adY)
    if base is not None:
        mag = mag + np.abs(base).astype(np.float64)
    tk = tk + gamma(n_c)[:, None] * mag + (0.0 if base_tol is None else base_tol)
    return SLACK * eds + FLOOR, SLACK * tq + FLOOR, SLACK * tk + FLOOR


def check(got, want, tol, name=""):
    """(ds, dQ, dKV) -- None where not asked for -- against float64 within the bound; the worst err / bound"""
    worst = 0.0
    for nm, a, b, t in zip(("ds", "dQ", "dKV"), got, want, tol):
        if a is None:
            continue
        a = a.detach().cpu().double().numpy() if isinstance(a, torch.Tensor) else np.asarray(a, np.float64)
        assert a.shape == b.shape, (name, nm, a.shape, b.shape)
        assert np.isfinite(b).all() and np.isfinite(a).all(), (name, nm, "non-finite")
        err = np.abs(a - b)
        viol = err > t
        assert not viol.any(), (name, nm, "beyond the bound", int(viol.sum()), "worst err / bound", float((err / t).max()))
        worst = max(worst, float((err / t).max(initial=0.0)))
    return worst


# ------------------------------------------------------------------------------------------------ the plan in fp32 numpy
def _dot16(a, b):
    """rows of 64: the lane's chain (f4_dot) and the butterfly (xor 8, 4, 2, 1) -> one fp32 value per row"""
    a, b = a.reshape(-1, 16, 4), b.reshape(-1, 16, 4)
    lane = _f32(a[:, :, 3] * b[:, :, 3])
    for i in (2, 1, 0):
        lane = _fma(a[:, :, i], b[:, :, i], lane)
    return _butterfly(lane)


def _butterfly(lane):
    for m in (8, 4, 2, 1):
        lane = _f32(lane + lane[:, np.arange(16) ^ m])
    return lane[:, 0]


def _groups_of(a, b, listed):
    """the slot lists the walks take, in order: one for a group row, 16 (group g: slots 16 g ... 16 g + 15 of every 256) for a
    listed one"""
    if not listed:
        return [list(range(a, b))]
    return [[j for j in range(a, b) if ((j - a) // 16) % 16 == g] for g in range(16)]


def emulate_bwd(c, alpha, Y, use_y, use_a, list_row, list_col, base=None, *, drop_group=None):
    """both passes as the kernels run them, in fp32 numpy -> (ds, dQ, dKV).  drop_group = ("row" | "col", g): that group's state of
    the listed rows / columns left out of the combine (a planted error)."""
    gm = group_max()
    alpha, Y = _f32(alpha), _f32(Y)
    z = np.float32(0)
    rid = np.repeat(np.arange(c.n_rows), c.lens)
    pos = c.order
    gd = _dot16(c.dY[rid], c.KV[c.colidx]) if use_y else np.zeros(c.ne, np.float32)
    ty = _dot16(c.dY, Y) if use_y else np.zeros(c.n_rows, np.float32)
    ds, dQ = np.zeros(c.ne, np.float32), np.zeros((c.n_rows, D), np.float32)
    for r in np.flatnonzero(c.lens):
        a, b = int(c.rowptr[r]), int(c.rowptr[r + 1])
        listed = list_row and b - a > gm
        tr = ty[r]
        if use_a:
            lanes = 256 if listed else 16
            part = np.zeros(lanes, np.float32)
            for j in range(a, b):                                     # lane (j - a) % lanes: a chain of fmas in slot order
                part[(j - a) % lanes] = _fma(alpha[pos[j]], c.dA[pos[j]], part[(j - a) % lanes])
            parts = _butterfly(part.reshape(-1, 16))
            ta = z
            for x in parts:                                           # (one group: 0 + x = x)
                ta = _f32(ta + x)
            tr = _f32(tr + ta)
        states = []
        for slots in _groups_of(a, b, listed):
            acc = np.zeros(D, np.float32)
            for j in slots:
                p = pos[j]
                gg = _f32(gd[j] + (c.dA[p] if use_a else z))
                d = _f32(alpha[p] * _f32(gg - tr))
                acc = _fma(d, c.KV[c.colidx[j]], acc)
                ds[p] = d
            states.append(acc)
        if listed:
            y = np.zeros(D, np.float32)
            for g, acc in enumerate(states):
                if drop_group != ("row", g):
                    y = _f32(y + acc)
            dQ[r] = y
        else:
            dQ[r] = states[0]
    b0 = np.zeros((c.n_kv, D), np.float32) if base is None else _f32(base)
    dKV = b0.copy()
    for k in np.flatnonzero(c.lens_t):
        a, b = int(c.rowptr_t[k]), int(c.rowptr_t[k + 1])
        listed = list_col and b - a > gm
        states = []
        for gi, slots in enumerate(_groups_of(a, b, listed)):
            acc = np.zeros(D, np.float32) if listed else b0[k].copy()
            for j in slots:
                p, r = c.perm_t[j], c.rowidx_t[j]
                if use_y:
                    acc = _fma(alpha[p], c.dY[r], acc)
                acc = _fma(ds[p], c.Q[r], acc)
            states.append(acc)
        if listed:
            y = b0[k].copy()
            for g, acc in enumerate(states):
                if drop_group != ("col", g):
                    y = _f32(y + acc)
            dKV[k] = y
        else:
            dKV[k] = states[0]
    return ds, dQ, dKV


def _torch_composition(c, use_y, use_a, base):
    """forward and backward of the three ops in fp32 torch on the CPU (stock autograd) -> (ds, dQ, dKV + base)"""
    from mmrec_amd import hip_ops
    seg, cols = torch.from_numpy(c.seg), torch.from_numpy(c.cols)
    Q, KV = torch.from_numpy(c.Q).requires_grad_(), torch.from_numpy(c.KV).requires_grad_()
    s = (Q[seg] * KV[cols]).sum(-1)
    s.retain_grad()
    alpha = hip_ops.segment_softmax_torch(s, seg, c.n_rows, c.eps)
    Y = torch.zeros(c.n_rows, D).index_add_(0, seg, alpha.unsqueeze(1) * KV[cols])
    out = 0.0
    if use_y:
        out = out + (Y * torch.from_numpy(c.dY)).sum()
    if use_a:
        out = out + (alpha * torch.from_numpy(c.dA)).sum()
    out.backward()
    dKV = KV.grad if KV.grad is not None else torch.zeros_like(KV)
    return s.grad.numpy(), Q.grad.numpy(), (dKV if base is None else dKV + torch.from_numpy(base)).numpy()


def _base_of(c, dq=None):
    return {"none": None, "array": c.base_arr, "dQ": dq}[c.base]


def _small_cases():
    return [case(s) for s in range(CASES) if case(s).layout in ("lens", "dups", "one_row")]


# ------------------------------------------------------------------------------------------------ CPU: the checker and the cases
def test_draw_case_is_deterministic():
    a, b = draw_case(13), draw_case(13)
    for k in ("Q", "KV", "dY", "dA", "seg", "cols", "perm_t", "base_arr"):
        assert np.array_equal(getattr(a, k), getattr(b, k)), k


def test_cases_span_every_axis():
    gm = group_max()
    seen = {k: set() for k in ("combo", "use", "out", "base", "eps", "rows", "cols")}
    for s in range(CASES):
        c = case(s)
        seen["combo"].add((c.layout, c.transposed, c.shuffled))
        for k in ("use", "out", "base", "eps"):
            seen[k].add(getattr(c, k))
        seen["rows"].update(int(x) for x in c.lens)
        seen["cols"].update(int(x) for x in c.lens_t)
        assert c.n_rows <= 4200 and c.n_kv <= 4200
        assert np.array_equal(c.seg[c.order], np.repeat(np.arange(c.n_rows), c.lens))
        assert np.array_equal(c.cols[c.order], c.colidx) and np.array_equal(c.cols[c.perm_t], np.repeat(np.arange(c.n_kv), c.lens_t))
        assert np.array_equal(np.sort(c.perm_t), np.arange(c.ne))
        if c.base == "dQ":
            assert c.n_rows == c.n_kv and c.out == "both"
    axis = {0, 1, 2, 15, 16, 17, 63, 64, 65, gm - 1, gm, gm + 1, 1025, 3000}
    assert axis <= seen["rows"] and axis <= seen["cols"], (sorted(axis - seen["rows"]), sorted(axis - seen["cols"]))
    assert seen["combo"] == {(l, t, p) for l in LAYOUTS for t in (True, False) for p in (True, False)}
    assert seen["use"] == set(IN_MODES) and seen["out"] == set(OUT_MODES) and seen["base"] == set(BASES) and seen["eps"] == set(EPS)


def test_the_five_formulas_are_the_derivative():
    """float64: the kernel's formulas -- with t_r = <dY, Y> + sum alpha dAlpha, for every eps -- equal autograd of the forward"""
    for c in _small_cases():
        for use in IN_MODES:
            use_y, use_a = use in ("Y", "both"), use in ("alpha", "both")
            want = autograd64(c, use_y, use_a, c.base_arr)
            got = formulas64(c, use_y, use_a, c.base_arr)
            for a, b in zip(got, want):
                assert np.abs(a - b).max(initial=0.0) <= 1e-11 * max(1.0, np.abs(b).max(initial=0.0)), (c.seed, use)
    c = _grad_case(0)                                                 # and `grads64` of the forward's fuzz is the same reference
    col_side(c)
    want = grads64(c, True, True, False)
    got = autograd64(c, True, True)
    assert np.array_equal(got[1], want[0]) and np.array_equal(got[2], want[1])
    s = formulas64(c, True, True)
    assert np.abs(s[1] - want[0]).max() <= 1e-11 and np.abs(s[2] - want[1]).max() <= 1e-11


def test_bound_is_not_vacuous_on_these_cases():
    """the existing gradient test's condition, asked BEFORE any device run: the median of tol / |want| over the non-zero entries
    is below 1e-3.  For ds that holds in every single case.  dQ and dKV are sums whose terms cancel where the layout makes them
    (three source rows for everything, one row's 256 edges over 25 columns, a column fed by every row), while the bound adds
    magnitudes: there a single case's median reaches a few 1e-3.  So for dQ and dKV the condition is asked of each output over
    the entries of ALL cases together, per case with a ceiling of 5e-3 where the structure says the sum cancels (the rule is
    at the assertion) and of 1e-3 everywhere else -- and per output of the square graph the hip_ops test runs."""
    pooled, per_case = {"ds": [], "dQ": [], "dKV": []}, {"ds": [], "dQ": [], "dKV": []}
    for s in range(CASES):
        c = case(s)
        use_y, use_a, _, _ = _flags(c)
        base = _base_of(c, np.zeros((c.n_kv, D), np.float32))
        want = autograd64(c, use_y, use_a, base)
        tol = bwd_bound(c, use_y, use_a, True, True, base)
        for nm, b, t in zip(("ds", "dQ", "dKV"), want, tol):
            nz = np.abs(b) > 0
            assert nz.any(), (s, nm)
            ratio = np.broadcast_to(t, b.shape)[nz] / np.abs(b)[nz]
            pooled[nm].append(ratio)
            per_case[nm].append(float(np.median(ratio)))
            # per case: 1e-3, except where the output is a sum of many terms of random sign -- a typical row (column) of 63
            # entries or more, whose sum is ~ sqrt(63) = 8 times below the magnitudes the bound adds, or rows (columns) that
            # share 25 sources or fewer, where the terms of one source cancel first: there 5e-3
            typical, sources = ((c.lens, c.n_kv) if nm == "dQ" else (c.lens_t, c.n_rows)) if nm != "ds" else (np.ones(1), 1 << 30)
            cancelling = np.median(typical[typical > 0]) >= 63 or sources <= 25
            assert per_case[nm][-1] < (5e-3 if cancelling else 1e-3), (s, c.layout, c.transposed, nm, per_case[nm][-1])
    for nm in pooled:
        med = float(np.median(np.concatenate(pooled[nm])))
        print("%-3s median tol / |want|: all cases together %.2e; per case: median %.2e, worst %.2e, cases above 1e-3: %d" % (
            nm, med, np.median(per_case[nm]), max(per_case[nm]), sum(x >= 1e-3 for x in per_case[nm])))
        assert med < 1e-3, (nm, med)
    assert max(per_case["ds"]) < 1e-3, per_case["ds"]
    for same in (0, 1):                                               # the graph of the hip_ops test
        c = _grad_case(same)
        col_side(c)
        for use in IN_MODES:
            use_y, use_a = use in ("Y", "both"), use in ("alpha", "both")
            want, tol = autograd64(c, use_y, use_a), bwd_bound(c, use_y, use_a, True, True)
            for nm, b, t in zip(("ds", "dQ", "dKV"), want, tol):
                nz = np.abs(b) > 0
                assert float(np.median(np.broadcast_to(t, b.shape)[nz] / np.abs(b)[nz])) < 1e-3, (same, use, nm)


def test_plan_emulation_passes_the_checker():
    ran, worst = 0, 0.0
    for c in _small_cases():
        use_y, use_a, _, _ = _flags(c)
        alpha, Y = emulate(c, True)                                   # what the forward kernel leaves, in fp32
        want = None
        long = max(c.lens.max(initial=0), c.lens_t.max(initial=0)) > group_max()
        for list_row, list_col in (LISTS if long else LISTS[:1]):
            base = _base_of(c, None)
            if c.base == "dQ":                                        # the dQ this very call writes
                base = emulate_bwd(c, alpha, Y, use_y, use_a, list_row, list_col)[1]
                want = None
            if want is None:
                want = autograd64(c, use_y, use_a, base)
            got = emulate_bwd(c, alpha, Y, use_y, use_a, list_row, list_col, base)
            tol = bwd_bound(c, use_y, use_a, list_row, list_col, base)
            worst = max(worst, check(got, want, tol, "emulation seed %d lists %s %s" % (c.seed, list_row, list_col)))
            ran += 1
    print("fp32 emulation of both passes: %d runs, worst err / bound %.3f" % (ran, worst))
    assert ran >= 30 and worst <= 1.0


def test_torch_composition_passes_the_checker():
    ran, worst = 0, 0.0
    for c in (case(s) for s in range(CASES)):
        if max(c.lens.max(initial=0), c.lens_t.max(initial=0)) > 1100 or c.base == "dQ":
            continue
        use_y, use_a, _, _ = _flags(c)
        base = _base_of(c)
        tol = bwd_bound(c, use_y, use_a, True, True, base, score_n=65, composition=True)
        worst = max(worst, check(_torch_composition(c, use_y, use_a, base), autograd64(c, use_y, use_a, base), tol,
                                 "torch composition seed %d" % c.seed))
        ran += 1
    print("torch composition: %d cases, worst err / bound %.3f" % (ran, worst))
    assert ran >= 8


def _plant_case():
    """the lengths axis, shuffled, both gradients arriving, lengths beyond the group maximum on both sides"""
    rng = np.random.default_rng(4)
    c = Case()
    c.seed, c.exact, c.layout, c.shuffled, c.eps, c.use, c.out, c.base = -3, False, "plant", True, 1e-3, "both", "both", "array"
    lens = np.concatenate([[0], rng.permutation([1, 2, 15, 16, 17, 63, 64, 65, group_max() + 1, 700]), [0]])
    _finish(c, rng, lens, 12)
    cols_csr = rng.integers(0, 11, c.ne)                              # ~ 100 edges per column ...
    cols_csr[c.rowptr[np.argmax(lens)]:c.rowptr[np.argmax(lens)] + 400] = 11       # ... and one column of 400
    c.colidx = cols_csr.astype(np.int32)
    c.cols = np.empty(c.ne, np.int64)
    c.cols[c.order] = cols_csr
    c.KV = rng.standard_normal((c.n_kv, D)).astype(np.float32)
    c.Q = (rng.standard_normal((c.n_rows, D)) * 0.2).astype(np.float32)
    c.dY = rng.standard_normal((c.n_rows, D)).astype(np.float32)
    c.dA = rng.standard_normal(c.ne).astype(np.float32)
    c.base_arr = rng.standard_normal((c.n_kv, D)).astype(np.float32)
    c.ref = attention64(c.Q, c.KV, c.seg, c.cols, c.n_rows, c.eps)
    col_side(c, rng)
    return c


def test_checker_rejects_planted_errors():
    c = _plant_case()
    assert (c.lens > group_max()).sum() == 2 and (c.lens_t > group_max()).sum() == 1
    base = c.base_arr
    want = autograd64(c, True, True, base)
    tol = bwd_bound(c, True, True, True, True, base)
    f32 = lambda xs: tuple(_f32(x) for x in xs)                       # noqa: E731
    assert check(f32(formulas64(c, True, True, base)), want, tol, "clean") <= 1.0
    alpha, Y = emulate(c, True)
    assert check(emulate_bwd(c, alpha, Y, True, True, True, True, base), want, tol, "clean emulation") <= 1.0
    # an edge dropped from t_r: one that carries a thousandth of its row's weight or more, in a row of 15 ... 65
    rows = np.flatnonzero((c.lens >= 15) & (c.lens <= 65))
    q = next(int(q) for r in rows for q in np.flatnonzero(c.seg == r) if 1e-3 <= c.ref.alpha[q] <= 0.5 and abs(c.dA[q]) > 0.1)
    for plant in (("drop_t", [q]), ("t_without_dA",), ("ds_csr_order",), ("alpha_at_perm",), ("base_twice",)):
        with pytest.raises(AssertionError):
            check(f32(formulas64(c, True, True, base, plant=plant)), want, tol, str(plant))
    with pytest.raises(AssertionError):                               # the dropped edge with dY alone: its share of <dY, Y>
        check(f32(formulas64(c, True, False, base, plant=("drop_t", [q]))), autograd64(c, True, False, base),
              bwd_bound(c, True, False, True, True, base))
    # a listed row's / column's partial state (one group of 16) dropped from the combine
    for side in ("row", "col"):
        with pytest.raises(AssertionError):
            check(emulate_bwd(c, alpha, Y, True, True, True, True, base, drop_group=(side, 5)), want, tol, side)


# ------------------------------------------------------------------------------------------------ GPU: the raw C ABI, guarded
class _Dev:
    """a case's arrays on the device, the forward kernel's alpha^ and Y^ for it, and both long lists as hip_ops builds them"""

    def __init__(self, c, colidx=None, perm=None, rowidx_t=None, perm_t=None, forward=True):
        from mmrec_amd import hip_ops
        self.rowptr, self.colidx = _on(c.rowptr), _on(c.colidx if colidx is None else colidx)
        perm = c.perm if perm is None else perm
        self.perm = None if perm is None else _on(perm)
        self.rowptr_t, self.rowidx_t = _on(c.rowptr_t), _on(c.rowidx_t if rowidx_t is None else rowidx_t)
        self.perm_t = _on(c.perm_t if perm_t is None else perm_t)
        self.Q, self.KV, self.dY, self.dA, self.base = _on(c.Q), _on(c.KV), _on(c.dY), _on(c.dA), _on(c.base_arr)
        lr, lc = hip_ops.segment_long_rows(c.rowptr), hip_ops.segment_long_rows(c.rowptr_t)
        self.long_rows, self.n_long = (_on(lr), lr.size) if lr.size else (None, 0)
        self.long_cols, self.n_long_t = (_on(lc), lc.size) if lc.size else (None, 0)
        if forward:
            self.alpha, self.Y = (x.clone() for x in raw_forward(c, self, True, "forward for the backward"))


def raw(c, dev, use_y, use_a, want_q, want_kv, list_row, list_col, base="none", name="raw", ds_unwritten=None):
    """one call over guarded, sentinel-filled outputs -> (ds, dQ or None, dKV or None)"""
    from mmrec_amd import hip_ops
    p, lib = hip_ops._p, hip_ops._lib.load()
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())                     # noqa: E731
    sbuf, ds = _guarded(c.ne)
    qbuf, dq = _guarded(c.n_rows * D)
    kbuf, dkv = _guarded(c.n_kv * D)
    b = {"none": None, "array": p(dev.base), "dQ": ptr(dq)}[base]
    rc = lib.mmrec_edge_attention_bwd_f32(
        p(dev.rowptr), c.n_rows, p(dev.colidx), p(dev.perm), p(dev.long_rows) if list_row else None, dev.n_long if list_row else 0,
        p(dev.rowptr_t), p(dev.rowidx_t), p(dev.perm_t), p(dev.long_cols) if list_col else None, dev.n_long_t if list_col else 0,
        p(dev.Q), c.n_rows, p(dev.KV), c.n_kv, p(dev.Y) if use_y else None, p(dev.alpha), p(dev.dY) if use_y else None,
        p(dev.dA) if use_a else None, D, c.ne, ptr(ds), ptr(dq) if want_q else None, ptr(dkv) if want_kv else None, b,
        hip_ops._stream())
    assert rc == 0, (name, rc)
    torch.cuda.synchronize()
    _guards_ok(sbuf, c.ne, name + " ds", ds_unwritten)
    none_q, none_k = np.ones(c.n_rows * D, bool), np.ones(c.n_kv * D, bool)
    _guards_ok(qbuf, c.n_rows * D, name + " dQ", None if want_q else none_q)      # EVERY row is written -- or nothing at all
    _guards_ok(kbuf, c.n_kv * D, name + " dKV", None if want_kv else none_k)
    return ds, dq.view(c.n_rows, D) if want_q else None, dkv.view(c.n_kv, D) if want_kv else None


@pytest.mark.gpu
@pytest.mark.parametrize("seed", range(CASES))
def test_edge_attention_bwd_fuzz(seed):
    c = case(seed)
    dev = _Dev(c)
    gm = group_max()
    assert (dev.n_long > 0) == bool((c.lens > gm).any()) and (dev.n_long_t > 0) == bool((c.lens_t > gm).any())
    use_y, use_a, want_q, want_kv = _flags(c)
    worst, want = 0.0, None
    for list_row, list_col in LISTS:
        tag = "seed %d lists %s %s" % (seed, list_row, list_col)
        got = raw(c, dev, use_y, use_a, want_q, want_kv, list_row, list_col, c.base, tag)
        base, base_tol = _base_of(c, None), None
        if c.base == "dQ":                                            # the base is what the call itself wrote: exact for float64
            base = got[1].cpu().numpy()
            want = None
        if want is None:
            want = autograd64(c, use_y, use_a, base)
        tol = bwd_bound(c, use_y, use_a, list_row, list_col, base, base_tol=base_tol)
        worst = max(worst, check(got, want, tol, tag))
        if want_q:
            assert not got[1].cpu().numpy()[c.lens == 0].any(), (tag, "dQ of an empty row is not zero")
    print("edge_attention_bwd fuzz seed %d: %s%s %s from %s for %s base %s rows %d cols %d edges %d longest %d / %d eps %g "
          "worst err / bound %.3f" % (seed, c.layout, " transposed" if c.transposed else "", "shuffled" if c.shuffled else "csr order",
                                      c.use, c.out, c.base, c.n_rows, c.n_kv, c.ne, int(c.lens.max(initial=0)),
                                      int(c.lens_t.max(initial=0)), c.eps, worst))


# ------------------------------------------------------------------------------------------------ GPU: targeted tests
@pytest.mark.gpu
def test_out_of_range_ids_are_absent_edges():
    """a column id outside [0, n_kv) on the row side with a row id outside [0, n_rows) on the transposed side ("ids"), or a
    position outside [0, n_edges) on both sides ("positions"): an absent edge -- the results are float64's of the edge list
    without it, ds is 0 where the position is valid (and untouched where no slot maps to it), nothing outside the outputs is
    written, and a row left with absent edges only is a row of zeros.  The forward that left alpha and Y saw the same ids."""
    c = _plant_case()
    rng = np.random.default_rng(3)
    gone = rng.random(c.ne) < 0.1                                     # by COO position
    r0 = int(np.flatnonzero(c.lens == 2)[0])
    gone[c.seg == r0] = True                                          # a whole row
    keep = ~gone
    slot_of, slot_t_of = np.empty(c.ne, np.int64), np.empty(c.ne, np.int64)
    slot_of[c.order], slot_t_of[c.perm_t] = np.arange(c.ne), np.arange(c.ne)
    bad, bad_t = slot_of[gone], slot_t_of[gone]
    want = autograd64(c, True, True, c.base_arr, keep=keep)
    assert not want[1][r0].any() and not want[0][gone].any()
    # the case with float64's forward of the edge list WITHOUT them spread over all positions (an absent edge: score -inf, weight
    # 0), as the forward's own test does: the plans keep the lengths the kernels walk
    full = Case()
    full.__dict__.update(c.__dict__)
    sub = attention64(c.Q, c.KV, c.seg[keep], c.cols[keep], c.n_rows, c.eps)
    full.ref = Ref()
    for k, fill in (("s", -np.inf), ("A", 0.0), ("x", -np.inf), ("e", 0.0), ("alpha", 0.0)):
        v = np.full(c.ne, fill)
        v[keep] = getattr(sub, k)
        setattr(full.ref, k, v)
    full.ref.den, full.ref.Y = sub.den, sub.Y
    for what in ("ids", "positions"):
        colidx, perm, rowidx_t, perm_t = c.colidx.copy(), c.perm.copy(), c.rowidx_t.copy(), c.perm_t.copy()
        if what == "ids":
            colidx[bad] = rng.choice([-1, c.n_kv, c.n_kv + 12345, -(1 << 31), (1 << 31) - 1], bad.size)
            rowidx_t[bad_t] = rng.choice([-1, c.n_rows, c.n_rows + 12345, -(1 << 31), (1 << 31) - 1], bad.size)
        else:
            perm[bad] = rng.choice([-1, c.ne, c.ne + 12345, -(1 << 40), 1 << 40], bad.size)
            perm_t[bad_t] = rng.choice([-1, c.ne, c.ne + 12345, -(1 << 40), 1 << 40], bad.size)
        dev = _Dev(c, colidx=colidx, perm=perm, rowidx_t=rowidx_t, perm_t=perm_t, forward=False)
        dev.alpha, dev.Y = (x.clone() for x in raw_forward(c, dev, True, "forward, bad %s" % what, unwritten=gone))
        for list_row, list_col in LISTS:
            tag = "bad %s lists %s %s" % (what, list_row, list_col)
            got = raw(c, dev, True, True, True, True, list_row, list_col, "array", tag,
                      ds_unwritten=gone if what == "positions" else None)
            d = got[0].cpu().numpy()
            if what == "ids":
                assert not d[gone].any(), (tag, "ds of an absent edge is not 0")
            d = np.where(gone, 0.0, d)                                # (positions: never written, never read)
            check((d, got[1], got[2]), want, bwd_bound(full, True, True, list_row, list_col, c.base_arr), tag)
            assert not got[1].cpu().numpy()[r0].any()


@pytest.mark.gpu
def test_nan_alpha_poisons_its_row_and_its_columns_only():
    """rows whose alpha (and Y) are NaN -- a group row, a listed row, a hub: NaN in their own ds, in dQ[r] and in the dKV rows of
    their own columns, value by value, and nowhere else"""
    c = _plant_case()
    dev = _Dev(c)
    bad_rows = [int(np.flatnonzero(c.lens == n)[0]) for n in (1, 17, group_max() + 1)]
    assert not np.isin(np.arange(c.n_kv), c.cols[np.isin(c.seg, bad_rows)]).all()        # some column is spared
    alpha, Y = dev.alpha.cpu().numpy().copy(), dev.Y.cpu().numpy().copy()
    alpha[np.isin(c.seg, bad_rows)] = np.nan
    Y[bad_rows] = np.nan
    dev.alpha, dev.Y = _on(alpha), _on(Y)
    edge_bad = np.isin(c.seg, bad_rows)
    row_bad = np.isin(np.arange(c.n_rows), bad_rows)
    col_bad = np.isin(np.arange(c.n_kv), c.cols[edge_bad])
    f = formulas64(c, True, True, c.base_arr, alpha=alpha, Y=Y)       # float64 of the formulas: the same pattern
    assert np.array_equal(np.isnan(f[0]), edge_bad) and np.array_equal(np.isnan(f[1]), np.repeat(row_bad[:, None], D, 1))
    assert np.array_equal(np.isnan(f[2]), np.repeat(col_bad[:, None], D, 1))
    for use in IN_MODES:
        for list_row, list_col in LISTS:
            ds, dq, dkv = raw(c, dev, use in ("Y", "both"), use in ("alpha", "both"), True, True, list_row, list_col, "array",
                              "NaN %s %s %s" % (use, list_row, list_col))
            assert np.array_equal(np.isnan(ds.cpu().numpy()), edge_bad), use
            assert np.array_equal(np.isnan(dq.cpu().numpy()), np.repeat(row_bad[:, None], D, 1)), use
            assert np.array_equal(np.isnan(dkv.cpu().numpy()), np.repeat(col_bad[:, None], D, 1)), use


@pytest.mark.gpu
def test_two_runs_give_identical_bits():
    c = next(case(s) for s in range(CASES) if case(s).layout == "hub3000" and case(s).shuffled and not case(s).transposed)
    dev = _Dev(c)
    for list_row, list_col in LISTS:
        a = raw(c, dev, True, True, True, True, list_row, list_col, "dQ" if c.n_rows == c.n_kv else "array")
        b = raw(c, dev, True, True, True, True, list_row, list_col, "dQ" if c.n_rows == c.n_kv else "array")
        for x, y in zip(a, b):
            assert torch.equal(x.view(torch.int32), y.view(torch.int32)), (list_row, list_col)


# ------------------------------------------------------------------------------------------------ GPU: through hip_ops
BWD_CALLS = ("mmrec_edge_attention_bwd_f32", "mmrec_edge_dot_f32", "mmrec_segment_softmax_bwd_f32", "mmrec_spmm_csr_f32",
             "mmrec_spmm_csr_sched_f32")


def _logged(monkeypatch):
    from mmrec_amd import _lib
    lib, log = _lib.load(), []
    for fn in BWD_CALLS + ("mmrec_edge_attention_f32",):
        monkeypatch.setattr(lib, fn, lambda *a, _real=getattr(lib, fn), _fn=fn: log.append(_fn) or _real(*a))
    return log


def _run(c, same, use_y, use_a, fused_backward, dyn, q_grad=True, kv_grad=True):
    from mmrec_amd import hip_ops
    Q = _on(c.Q).requires_grad_(q_grad)
    KV = Q if same else _on(c.KV).requires_grad_(kv_grad)
    assert hip_ops.edge_attention_served(Q, KV, dyn)
    y, alpha = hip_ops.edge_attention(Q, KV, dyn, eps=c.eps, fused_backward=fused_backward)
    out = 0.0
    if use_y:
        out = out + (y * _on(c.dY)).sum()
    if use_a:
        out = out + (alpha * _on(c.dA)).sum()
    out.backward()
    torch.cuda.synchronize()
    return Q, KV, y, alpha


@pytest.mark.gpu
@pytest.mark.parametrize("same", [False, True], ids=["distinct", "Q_is_KV"])
@pytest.mark.parametrize("use", IN_MODES)
def test_gradients_through_hip_ops_vs_float64(same, use, monkeypatch):
    c = _grad_case(int(same))
    col_side(c)
    use_y, use_a = use in ("Y", "both"), use in ("alpha", "both")
    dyn = _wrapper_graph(c)
    order = np.argsort(c.seg, kind="stable")
    assert np.array_equal(order, dyn.perm.cpu().numpy()) and np.array_equal(c.perm_t, dyn.perm_t.cpu().numpy())
    log = _logged(monkeypatch)
    Q, KV, y, alpha = _run(c, same, use_y, use_a, True, dyn)
    assert log[0] == "mmrec_edge_attention_f32" and log[1:] == ["mmrec_edge_attention_bwd_f32"], log      # ONE call, nothing else
    want = grads64(c, use_y, use_a, same)
    wc = Case()
    wc.__dict__.update(c.__dict__)
    wc.order = order                                                  # the wrapper's own (stable) CSR order
    _, tq, tk = bwd_bound(wc, use_y, use_a, True, True)
    if same:                                                          # dQ is the column pass' first term: its error and one more term
        dq64 = autograd64(c, use_y, use_a)[1]
        _, _, tk = bwd_bound(wc, use_y, use_a, True, True, base=dq64, base_tol=tq)
    got, tol = ((Q.grad,), (tk,)) if same else ((Q.grad, KV.grad), (tq, tk))
    worst = 0.0
    for nm, a, b, t in zip(("dQ", "dKV"), got, want, tol):
        a = a.cpu().double().numpy()
        assert np.isfinite(a).all() and float(np.abs(b).max()) > 0
        err = np.abs(a - b)
        assert (err <= t).all(), (nm, use, same, int((err > t).sum()), float((err / t).max()))
        assert float(np.median(t[np.abs(b) > 0] / np.abs(b)[np.abs(b) > 0])) < 1e-3, nm      # the bound is not vacuous
        worst = max(worst, float((err / t).max()))
    print("edge_attention fused backward %s %s: worst err / bound %.3f" % ("Q is KV" if same else "distinct", use, worst))
    if same:
        return
    # needs_input_grad: a table that asks for no gradient gets none, and the other one's is the same bits
    for q_grad, kv_grad in ((True, False), (False, True)):
        Q2, KV2, y2, _ = _run(c, False, use_y, use_a, True, dyn, q_grad, kv_grad)
        assert torch.equal(y2, y)
        assert (Q2.grad is None) == (not q_grad) and (KV2.grad is None) == (not kv_grad)
        assert torch.equal(Q2.grad, Q.grad) if q_grad else torch.equal(KV2.grad, KV.grad)


@pytest.mark.gpu
def test_keyword_and_switch_decide_which_backward_runs(monkeypatch):
    from mmrec_amd import hip_ops
    c = _grad_case(0)
    dyn = _wrapper_graph(c)
    log = _logged(monkeypatch)

    def backward_calls(fused_backward):
        del log[:]
        Q, KV, _, _ = _run(c, False, True, True, fused_backward, dyn)
        assert log[0] == "mmrec_edge_attention_f32"
        return [x.replace("_sched", "") for x in log[1:]], Q.grad, KV.grad
    today = ["mmrec_edge_dot_f32", "mmrec_segment_softmax_bwd_f32", "mmrec_spmm_csr_f32", "mmrec_spmm_csr_f32", "mmrec_spmm_csr_f32"]
    off, q_off, kv_off = backward_calls(False)
    assert off == today, off                                          # the keyword off: today's sequence
    on, q_on, kv_on = backward_calls(True)
    assert on == ["mmrec_edge_attention_bwd_f32"], on
    np.testing.assert_allclose(q_on.cpu().numpy(), q_off.cpu().numpy(), rtol=1e-3, atol=1e-5)
    np.testing.assert_allclose(kv_on.cpu().numpy(), kv_off.cpu().numpy(), rtol=1e-3, atol=1e-5)
    monkeypatch.setattr(hip_ops, "EDGE_ATTENTION_BWD", False)
    sw, q_sw, kv_sw = backward_calls(True)
    assert sw == today, sw                                            # the switch off: the composed backward, today's bits
    assert torch.equal(q_sw, q_off) and torch.equal(kv_sw, kv_off)
