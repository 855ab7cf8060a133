"""GPU: seeded differential fuzz of the per-edge dot products (SDDMM: csrc/edge.hip, hip_ops.edge_dot, and d vals of
hip_ops.spmm_vals) against float64 results computed on the host, never against another form of the kernel.

The kernels' plan.  Forward out[e] = <A[rows[e]], B[cols[e]]>: a group of L = min(d, 64) / 4 lanes per edge; a lane holds one
float4 of each row per 64 columns and runs ONE fma chain over its own columns -- d / 16 of them (4 for the slices d = 8 / 16 /
32) -- then the group is summed by a butterfly of log2(L) adds.  A term therefore meets
        n(d) = d / 16 + 4  (d >= 64),   4 + log2(d / 4)  (d = 8, 16, 32: 5, 6, 7)
roundings; n(d) <= d at every served width (asserted: a larger n would mean another plan).
Backward dA[r] = sum over the edges of row r of g[e] B[cols[e]] (dB alike over the columns; `A is B`: both into one table):
  atomic  mmrec_edge_dot_bwd_f32: one rounded product per edge added by fp32 atomics in any order: n = (edges on the output
          row) + 1;
  dyn     the two sums as mmrec_spmm_csr_f32 over the edge list's CSR forms: n = tests.test_spmm_fuzz_gpu.plan_depth of the
          row's degree (+ 1 where the two gradients of `A is B` are added).

Two acceptance modes, those of tests/test_spmm_fuzz_gpu.py; each case uses one.
  exact  entries of A and B are multiples of 1/16 of magnitude <= 1, g multiples of 1/8 of magnitude <= 1.  A forward product
         is a multiple of 2^-8 and a sum of d <= 384 of them stays below 2^9; a backward term is a multiple of 2^-7 and a
         row's sum stays below 2^16 with at most 2^16 edges on it (the generator asserts it): every value any summation order
         can form is an exact fp32 number and the result must EQUAL float64 -- forward, atomic backward (a hub row of several
         thousand edges included), dyn backward and spmm_vals' d vals.
  float  normal values with scaled rows and columns, exact zeros, an occasional inf / NaN row.  |got - ref64| <= gamma(n) M +
         n 2^-149 with M the same expression on absolute values, gamma(n) = n u / (1 - n u), u = 2^-24; non-finite results must
         be float64's, value for value.

An edge whose row id is outside [0, n_a) or whose column id is outside [0, n_b) must give exactly 0 and add nothing to the
gradients; the ids used (-1, n, far beyond both tables in either direction) would address memory outside both tables if they
were used, so the cases check the guard's result (0, neighbours untouched) -- the kernels never form such an address.

`test_checker_rejects_planted_errors` and `test_cases_span_every_axis` need no GPU."""
import numpy as np
import pytest
import torch

from tests.test_spmm_fuzz_gpu import FLT_MAX, U, _grid, _on, check, csr, gamma, plan_depth

CASES = 66
WIDTHS = (8, 16, 32, 64, 128, 192, 256, 320, 384)
N_EDGES = (0, 1, 3, 4, 5, 255, 256, 257, 300007, 2000, 14000)
GRADS = ("both", "dA", "dB")
BAD_IDS = (-1, -(1 << 40), 1 << 40)                    # + n_a, n_b and n_a + n_b + 12345 (per case)
HUB = 3000


def forward_depth(d):
    n = d // 16 + 4 if d >= 64 else 4 + int(np.log2(d // 4))
    assert n <= d, "not the plan of the module docstring"
    return n


# ------------------------------------------------------------------------------------------------ host references
def edge_dots64(A, B, rows, cols):
    """float64 (ref, M) of the per-edge dots; an edge with an id outside its table: (0, 0)"""
    ok = (rows >= 0) & (rows < A.shape[0]) & (cols >= 0) & (cols < B.shape[0])
    ref, M = np.zeros(rows.size), np.zeros(rows.size)
    idx = np.flatnonzero(ok)
    with np.errstate(invalid="ignore", over="ignore"):
        for s in range(0, idx.size, 1 << 15):
            e = idx[s:s + (1 << 15)]
            a, b = A[rows[e]].astype(np.float64), B[cols[e]].astype(np.float64)
            ref[e] = (a * b).sum(1)
            M[e] = (np.abs(a) * np.abs(b)).sum(1)
    return ref, M, ok


def check_dots(got, A, B, rows, cols, *, exact, name=""):
    """got [n_edges] against float64 in the mode's sense (module docstring); returns the float mode's worst err / M"""
    g = got.detach().cpu().double().numpy() if isinstance(got, torch.Tensor) else np.asarray(got, np.float64)
    assert g.shape == rows.shape, (name, g.shape, rows.shape)
    ref, M, ok = edge_dots64(A, B, rows, cols)
    assert (g[~ok] == 0).all(), (name, "an edge with an id outside its table is not 0", int((g[~ok] != 0).sum()))
    if exact:
        assert np.isfinite(ref).all() and (M * 256 < 2.0 ** 23).all(), (name, "case outside the exact grid")
        bad = g != ref
        assert not bad.any(), (name, "exact mismatch", int(bad.sum()), "first at", int(np.argmax(bad)),
                               float(g[np.argmax(bad)]), float(ref[np.argmax(bad)]))
        return 0.0
    n = forward_depth(A.shape[1])
    ref32 = np.where(np.abs(ref) > FLT_MAX, np.copysign(np.inf, ref), ref)
    fin = np.isfinite(ref32)
    assert np.array_equal(np.isfinite(g), fin), (name, "non-finite pattern", int((np.isfinite(g) != fin).sum()))
    same = (g == ref32) | (np.isnan(g) & np.isnan(ref32))
    assert same[~fin].all(), (name, "non-finite values differ", int((~fin & ~same).sum()))
    with np.errstate(invalid="ignore"):
        err = np.where(fin, np.abs(g - ref32), 0.0)
        viol = fin & (err > gamma(n) * M + n * 2.0 ** -149)
    assert not viol.any(), (name, "beyond gamma(n) M", int(viol.sum()), "first at", int(np.argmax(viol)),
                            float(err[np.argmax(viol)]), float(M[np.argmax(viol)]), n)
    pos = fin & (M > 0)
    return float((err[pos] / M[pos]).max()) if pos.any() else 0.0


def edge_matrix(r, c, v, shape):
    """scipy CSR [shape] with one entry v[e] at (r[e], c[e]) per edge, duplicates kept as separate entries"""
    order = np.argsort(r, kind="stable")
    rowptr = np.zeros(shape[0] + 1, np.int64)
    np.cumsum(np.bincount(r, minlength=shape[0]), out=rowptr[1:])
    return csr(rowptr, c[order], v[order], shape)


# ------------------------------------------------------------------------------------------------ cases
class Case:
    pass


def _float_table(rng, n, d):
    X = rng.standard_normal((n, d))
    for i in rng.choice(n, size=min(n, 4), replace=False):
        X[i] *= 10.0 ** rng.uniform(-8, 8)
    for j in rng.choice(d, size=min(d, 4), replace=False):
        X[:, j] *= 10.0 ** rng.uniform(-4, 4)
    X[rng.random(X.shape) < 0.2] = 0.0
    return X


def draw_case(seed):
    rng = np.random.default_rng(9100 + seed)
    c = Case()
    c.seed = seed
    c.d = WIDTHS[seed % len(WIDTHS)]
    c.exact = (seed // len(WIDTHS)) % 2 == 0
    c.ne = N_EDGES[seed % len(N_EDGES)]
    c.same = (seed // 2) % 2 == 0                                     # `A is B`: one table on both sides, dA == dB
    c.grads = "same" if c.same else GRADS[(seed // 4) % 3]
    c.oob = seed % 3 == 1 and c.ne >= 3
    c.big = c.ne > 100000
    if c.big:
        c.n_a = 20000
        c.n_b = 20000 if c.same else 15000
    else:
        c.n_a = int(rng.integers(40, 3000))
        c.n_b = c.n_a if c.same else int(rng.integers(40, 3000))
        if c.n_b == c.n_a and not c.same:
            c.n_b += 7
    ne, n_a, n_b, d = c.ne, c.n_a, c.n_b, c.d
    rows, cols = rng.integers(0, n_a, ne), rng.integers(0, n_b, ne)
    c.hub_row = c.hub_col = None
    if ne >= 2000:                                                    # a hub row and a hub column (other nodes)
        k = min(ne // 4, HUB)
        where = rng.permutation(ne)
        c.hub_row, c.hub_col = int(rng.integers(0, n_a)), int(rng.integers(0, n_b))
        rows[where[:k]], cols[where[k:2 * k]] = c.hub_row, c.hub_col
    if ne >= 4:                                                       # duplicate edges, next to each other and far apart
        rows[1], cols[1] = rows[0], cols[0]
        src, dst = rng.integers(0, ne, max(1, ne // 20)), rng.integers(0, ne, max(1, ne // 20))
        rows[dst], cols[dst] = rows[src], cols[src]
    c.bad = np.zeros(ne, bool)
    if c.oob:                                                         # ids outside their table, in the middle of the list
        bad_ids = BAD_IDS + (n_a + n_b + 12345,)
        where = rng.choice(np.arange(1, ne), size=max(2, ne // 25) if ne > 3 else 2, replace=False)
        for i, e in enumerate(where):
            if i % 2 == 0:
                rows[e] = (bad_ids + (n_a,))[i // 2 % 5]
            else:
                cols[e] = (bad_ids + (n_b,))[i // 2 % 5]
        if n_a != n_b:                                                # an id inside the OTHER table only
            e = where[-1]
            rows[e], cols[e] = (n_b - 1, 0) if n_a < n_b else (0, n_a - 1)
        c.bad[where] = True
    c.rows, c.cols = rows.astype(np.int64), cols.astype(np.int64)
    c.inf_row = False
    if c.exact:
        c.A = _grid(rng, (n_a, d))
        c.B = c.A if c.same else _grid(rng, (n_b, d))
        c.g = (rng.integers(-8, 9, ne) / 8.0).astype(np.float32)
        # the exact grid: a row's (and, one table on both sides, a node's) backward sum of multiples of 2^-7 stays below 2^16
        ok = ~c.bad
        per_row = np.bincount(c.rows[ok], minlength=n_a).max(initial=0)
        per_col = np.bincount(c.cols[ok], minlength=n_b).max(initial=0)
        assert per_row + per_col <= 1 << 16, (seed, "backward outside the grid")
        assert d * 256 < 2 ** 23
    else:
        A = _float_table(rng, n_a, d)
        B = A if c.same else _float_table(rng, n_b, d)
        c.inf_row = seed % 4 >= 2 and ne >= 3
        if c.inf_row:                                                 # an inf / NaN row that edges do read
            e = int(np.flatnonzero(~c.bad)[ne // 2 % max(1, int((~c.bad).sum()))])
            A[c.rows[e], rng.random(d) < 0.5] = rng.choice([np.inf, -np.inf, np.nan])
            A[c.rows[e], 0] = np.inf
        c.A = A.astype(np.float32)
        c.B = c.A if c.same else B.astype(np.float32)
        g = rng.standard_normal(ne)
        g[rng.random(ne) < 0.05] = 0.0
        c.g = g.astype(np.float32)
    return c


def backward_terms(c):
    """{name: (terms for `check`, edges per output row)} of the wanted gradients; edges with an id outside its table add nothing"""
    ok = ~c.bad
    r, k, g = c.rows[ok], c.cols[ok], c.g[ok]
    Ma, Mb = edge_matrix(r, k, g, (c.n_a, c.n_b)), edge_matrix(k, r, g, (c.n_b, c.n_a))
    da, db = np.bincount(r, minlength=c.n_a), np.bincount(k, minlength=c.n_b)
    if c.same:
        return {"dA": ([(1.0, Ma, c.B), (1.0, Mb, c.A)], da + db)}
    out = {}
    if c.grads in ("both", "dA"):
        out["dA"] = ([(1.0, Ma, c.B)], da)
    if c.grads in ("both", "dB"):
        out["dB"] = ([(1.0, Mb, c.A)], db)
    return out


# ------------------------------------------------------------------------------------------------ CPU: the checker and the cases
def _fp32_dots(c, A=None, B=None):
    """an fp32 evaluation on the host: exact cases in fp32 arithmetic (any order is exact), float cases float64 rounded"""
    A, B = c.A if A is None else A, c.B if B is None else B
    ref, _, ok = edge_dots64(A, B, c.rows, c.cols)
    if c.exact:
        out = np.zeros(c.ne, np.float32)
        out[ok] = np.einsum("ij,ij->i", A[c.rows[ok]], B[c.cols[ok]], dtype=np.float32)
        return out
    with np.errstate(over="ignore"):
        return ref.astype(np.float32)


def _find(cond):
    for s in range(CASES):
        c = draw_case(s)
        if not c.big and cond(c):
            return c
    raise AssertionError("no such case")


def test_checker_rejects_planted_errors():
    for exact in (True, False):
        c = _find(lambda c: c.exact == exact and c.d == 128 and c.ne >= 255)
        good = _fp32_dots(c)
        assert check_dots(good, c.A, c.B, c.rows, c.cols, exact=exact, name="clean") <= 1.01 * U
        ref, M, ok = edge_dots64(c.A, c.B, c.rows, c.cols)
        with np.errstate(invalid="ignore"):
            share = np.where(np.isfinite(ref) & (M > 0), np.abs(ref) / np.where(M > 0, M, 1), 0)
        # one edge's result swapped with its neighbour's
        e = next(e for e in range(c.ne - 1) if np.isfinite(good[e:e + 2]).all() and ok[e:e + 2].all()
                 and abs(float(good[e]) - float(good[e + 1])) > 1e-3 * max(M[e], M[e + 1]))
        bad = good.copy()
        bad[e], bad[e + 1] = good[e + 1], good[e]
        with pytest.raises(AssertionError):
            check_dots(bad, c.A, c.B, c.rows, c.cols, exact=exact)
        # a dropped 64-column block at d = 128
        A2 = c.A.copy()
        A2[:, 64:] = 0.0
        dropped = _fp32_dots(c, A=A2, B=A2 if c.same else None)
        assert (dropped != good).any()
        with pytest.raises(AssertionError):
            check_dots(dropped, c.A, c.B, c.rows, c.cols, exact=exact)
        # a 1e-4 relative error (visible where |ref| is not a tiny part of M: gamma(12) M = 7e-7 M)
        e = int(np.argmax(share))
        assert share[e] > 0.05
        bad = good.copy()
        bad[e] = np.float32(ref[e] * (1 + 1e-4))
        with pytest.raises(AssertionError):
            check_dots(bad, c.A, c.B, c.rows, c.cols, exact=exact)
    c = _find(lambda c: c.oob and c.ne >= 255)                        # a value at an edge that has no row
    bad = _fp32_dots(c)
    bad[np.flatnonzero(c.bad)[0]] = 1.0
    with pytest.raises(AssertionError):
        check_dots(bad, c.A, c.B, c.rows, c.cols, exact=c.exact)
    c = _find(lambda c: c.inf_row and not np.isfinite(_fp32_dots(c)).all())      # a wrong non-finite value
    bad = _fp32_dots(c)
    bad[~np.isfinite(bad)] = 0.0
    with pytest.raises(AssertionError):
        check_dots(bad, c.A, c.B, c.rows, c.cols, exact=False)


def test_cases_span_every_axis():
    """every served width in both modes, every edge count, unsorted lists with duplicates, a hub row and a hub column of
    several thousand edges, one table on both sides and two tables of different sizes, ids outside their table of every kind
    (and one inside the OTHER table only), an inf / NaN row that reaches the output, every wanted-gradient combination"""
    seen = {k: set() for k in ("mode", "ne", "grads", "bad_row", "bad_col", "inf", "hub", "oob_mode")}
    other_table = False
    for s in range(CASES):
        c = draw_case(s)
        assert forward_depth(c.d) <= c.d
        seen["mode"].add((c.d, c.exact)), seen["ne"].add(c.ne), seen["grads"].add(c.grads)
        assert c.rows.size == c.ne and c.cols.size == c.ne
        if c.ne >= 255:
            assert (np.diff(c.rows) < 0).any()                                        # unsorted
            assert np.unique(np.stack([c.rows, c.cols]), axis=1).shape[1] < c.ne      # duplicate edges
        assert c.same == (c.A is c.B) and (c.same or c.n_a != c.n_b)
        if c.hub_row is not None:
            kr, kc = int((c.rows == c.hub_row).sum()), int((c.cols == c.hub_col).sum())
            assert kr >= 400 and kc >= 400
            if kr >= 2500 and kc >= 2500:
                seen["hub"].add((c.exact, c.same))
        out_r = (c.rows < 0) | (c.rows >= c.n_a)
        out_c = (c.cols < 0) | (c.cols >= c.n_b)
        assert np.array_equal(out_r | out_c, c.bad) and c.bad.any() == c.oob
        if c.oob:
            assert not c.bad[0] and (~c.bad).any()
            seen["oob_mode"].add(c.exact)
            seen["bad_row"].update(int(x) - c.n_a if 0 <= x - c.n_a < 1 << 20 else int(x) for x in c.rows[out_r])
            seen["bad_col"].update(int(x) - c.n_b if 0 <= x - c.n_b < 1 << 20 else int(x) for x in c.cols[out_c])
            other_table |= bool((out_r & (c.rows >= 0) & (c.rows < c.n_b)).any() or (out_c & (c.cols >= 0) & (c.cols < c.n_a)).any())
        if c.inf_row:
            ref, _, _ = edge_dots64(c.A, c.B, c.rows, c.cols)
            if not np.isfinite(ref).all():
                seen["inf"].add(c.d)
    assert seen["mode"] == {(d, e) for d in WIDTHS for e in (True, False)}
    assert seen["ne"] == set(N_EDGES) and {0, 1, 3, 4, 5, 255, 256, 257} <= seen["ne"] and max(seen["ne"]) > 290000
    assert seen["grads"] == {"same", "both", "dA", "dB"}
    assert seen["hub"] >= {(True, True), (True, False)} and len(seen["hub"]) >= 3
    for key in ("bad_row", "bad_col"):
        assert {-1, -(1 << 40), 1 << 40, 0} <= seen[key], (key, seen[key])          # 0: the id n itself
    assert other_table and seen["oob_mode"] == {True, False}
    assert len(seen["inf"]) >= 4


# ------------------------------------------------------------------------------------------------ GPU: the fuzz
def _tables_on(c, grads=True):
    A = _on(c.A)
    B = A if c.same else _on(c.B)
    if grads:
        if c.same or c.grads in ("both", "dA"):
            A.requires_grad_()
        if not c.same and c.grads in ("both", "dB"):
            B.requires_grad_()
    return A, B


def _backward_checked(c, form, rows, cols, dyn=None):
    """one forward + backward through hip_ops.edge_dot in the given form, everything against float64"""
    from mmrec_amd import hip_ops
    A, B = _tables_on(c)
    out = hip_ops.edge_dot(A, B, rows, cols, dyn=dyn)
    worst = check_dots(out, c.A, c.B, c.rows, c.cols, exact=c.exact, name="forward (%s) seed %d" % (form, c.seed))
    out.backward(_on(c.g))
    torch.cuda.synchronize()
    thr = hip_ops.default_long_row_threshold(max(c.n_a, c.n_b))
    for name, (terms, per_row) in backward_terms(c).items():
        got = (A if name == "dA" else B).grad
        depth = per_row + 1 if form == "atomic" else plan_depth(per_row, thr) + (1 if c.same else 0)
        worst = max(worst, check(got, terms, exact=c.exact, depth=depth, name="%s (%s) seed %d" % (name, form, c.seed)))
    if not c.same:
        assert (A.grad is None) == (c.grads == "dB") and (B.grad is None) == (c.grads == "dA")
    return worst


@pytest.mark.gpu
@pytest.mark.parametrize("seed", range(CASES))
def test_edge_dot_fuzz(seed):
    from mmrec_amd import hip_ops
    c = draw_case(seed)
    rows, cols = _on(c.rows), _on(c.cols)
    A, B = _tables_on(c, grads=False)
    assert hip_ops.edge_dot_served(A, B, rows, cols)
    out = hip_ops._edge_dot_fwd(A, B, rows, cols)                     # into a fresh buffer ...
    again = torch.full((c.ne,), float("nan"), device="cuda:0")        # ... and the raw entry point over a NaN-filled one
    p = hip_ops._p
    rc = hip_ops._lib.load().mmrec_edge_dot_f32(p(A), c.n_a, p(B), c.n_b, p(rows), p(cols), c.ne, c.d, p(again),
                                                hip_ops._stream())
    assert rc == 0
    torch.cuda.synchronize()
    worst = check_dots(out, c.A, c.B, c.rows, c.cols, exact=c.exact, name="forward seed %d" % seed)
    assert torch.equal(out.view(torch.int32), again.view(torch.int32)), "two runs, two results"
    forms = ["atomic"]
    worst = max(worst, _backward_checked(c, "atomic", rows, cols))
    if c.ne and not c.oob:                                            # a DynGraph holds ids inside the tables only
        dyn = hip_ops.DynGraph(rows, cols, c.n_a, c.n_b)
        worst = max(worst, _backward_checked(c, "dyn", rows, cols, dyn=dyn))
        forms.append("dyn")
        if c.exact:                                                   # d vals of the product with learned values: the same dots
            X, v = _on(c.B), _on(c.g).requires_grad_()
            hip_ops.spmm_vals(dyn, X, v).backward(_on(c.A))
            torch.cuda.synchronize()
            check_dots(v.grad, c.A, c.B, c.rows, c.cols, exact=True, name="spmm_vals d vals seed %d" % seed)
            forms.append("dvals")
        if seed % 4 == 0:                                             # `hip_deterministic` without a graph: one is built
            try:
                hip_ops.set_deterministic(True)
                worst = max(worst, _backward_checked(c, "deterministic", rows, cols))
            finally:
                hip_ops.set_deterministic(hip_ops.DETERMINISTIC_DEFAULT)
            forms.append("deterministic")
    print("edge_dot fuzz seed %d: d %d edges %d %s %s tables %d / %d grads %s%s%s forms %s worst err/M %.3e" % (
        seed, c.d, c.ne, "exact" if c.exact else "float", "one table" if c.same else "two tables", c.n_a, c.n_b, c.grads,
        " oob" if c.oob else "", " inf" if c.inf_row else "", "+".join(forms), worst))


# ------------------------------------------------------------------------------------------------ GPU: targeted tests
def _hub_case(rng, d, same=True, ne=40000, n=3000):
    rows, cols = rng.integers(0, n, ne), rng.integers(0, n, ne)
    rows[rng.permutation(ne)[:4000]] = 17
    cols[rng.permutation(ne)[:4000]] = 23
    A = rng.standard_normal((n, d)).astype(np.float32)
    B = A if same else rng.standard_normal((n, d)).astype(np.float32)
    return A, B, rows.astype(np.int64), cols.astype(np.int64), rng.standard_normal(ne).astype(np.float32)


@pytest.mark.gpu
@pytest.mark.parametrize("d", [16, 64, 256])
def test_forward_and_graph_backward_repeat_bit_for_bit(d):
    """two runs, the same bits: the forward always; the backward with `dyn`, and under set_deterministic(True) without one"""
    from mmrec_amd import hip_ops
    rng = np.random.default_rng(300 + d)
    for same in (True, False):
        A0, B0, r, k, g = _hub_case(rng, d, same)
        rows, cols, gt = _on(r), _on(k), _on(g)
        dyn = hip_ops.DynGraph(rows, cols, A0.shape[0], B0.shape[0])
        for form in ("dyn", "deterministic"):
            runs = []
            try:
                hip_ops.set_deterministic(form == "deterministic")
                for _ in range(2):
                    A = _on(A0).requires_grad_()
                    B = A if same else _on(B0).requires_grad_()
                    out = hip_ops.edge_dot(A, B, rows, cols, dyn=dyn if form == "dyn" else None)
                    out.backward(gt)
                    torch.cuda.synchronize()
                    runs.append([out.detach()] + [t.grad for t in ((A,) if same else (A, B))])
            finally:
                hip_ops.set_deterministic(hip_ops.DETERMINISTIC_DEFAULT)
            for a, b in zip(*runs):
                assert torch.equal(a.view(torch.int32), b.view(torch.int32)), (form, same)


@pytest.mark.gpu
def test_raw_backward_accumulates_and_skips_what_is_not_wanted():
    """mmrec_edge_dot_bwd_f32 adds into what the buffers hold (exact mode), with dA only, dB only, both, and dA == dB"""
    from mmrec_amd import hip_ops
    rng = np.random.default_rng(77)
    n_a, n_b, d, ne = 500, 300, 64, 6000
    A, B, A0, B0 = (_grid(rng, s) for s in ((n_a, d), (n_b, d), (n_a, d), (n_b, d)))
    r, k = rng.integers(0, n_a, ne), rng.integers(0, n_b, ne)
    r[:1500] = 3
    r[2000], k[2001] = -1, n_b
    g = (rng.integers(-8, 9, ne) / 8.0).astype(np.float32)
    ok = (r >= 0) & (k < n_b)
    Ma, Mb = edge_matrix(r[ok], k[ok], g[ok], (n_a, n_b)), edge_matrix(k[ok], r[ok], g[ok], (n_b, n_a))
    lib, p = hip_ops._lib.load(), hip_ops._p
    At, Bt, rt, kt, gt = _on(A), _on(B), _on(r), _on(k), _on(g)
    for want_a, want_b in ((True, True), (True, False), (False, True)):
        dA, dB = _on(A0), _on(B0)
        rc = lib.mmrec_edge_dot_bwd_f32(p(gt), p(At), n_a, p(Bt), n_b, p(rt), p(kt), ne, d, p(dA) if want_a else None,
                                        p(dB) if want_b else None, hip_ops._stream())
        assert rc == 0
        torch.cuda.synchronize()
        if want_a:
            check(dA, [(1.0, Ma, B)], acc_in=A0, acc_scale=1.0, exact=True, name="raw dA")
        else:
            assert torch.equal(dA, _on(A0))
        if want_b:
            check(dB, [(1.0, Mb, A)], acc_in=B0, acc_scale=1.0, exact=True, name="raw dB")
        else:
            assert torch.equal(dB, _on(B0))
    # one table on both sides, one buffer for both sums
    k2 = rng.integers(0, n_a, ne)
    k2[2001] = n_a
    ok = (r >= 0) & (k2 < n_a)
    Ma, Mb = edge_matrix(r[ok], k2[ok], g[ok], (n_a, n_a)), edge_matrix(k2[ok], r[ok], g[ok], (n_a, n_a))
    both, k2t = _on(A0), _on(k2)
    rc = lib.mmrec_edge_dot_bwd_f32(p(gt), p(At), n_a, p(At), n_a, p(rt), p(k2t), ne, d, p(both), p(both), hip_ops._stream())
    assert rc == 0
    torch.cuda.synchronize()
    check(both, [(1.0, Ma, A), (1.0, Mb, A)], acc_in=A0, acc_scale=1.0, exact=True, name="raw dA == dB")
    # dA == dB with two different tables is refused on the host
    assert lib.mmrec_edge_dot_bwd_f32(p(gt), p(At), n_a, p(Bt), n_b, p(rt), p(kt), ne, d, p(both), p(both),
                                      hip_ops._stream()) == 10001


@pytest.mark.gpu
@pytest.mark.parametrize("d", [32, 128])
def test_spmm_vals_at_other_widths_vs_float64(d):
    """hip_ops.spmm_vals away from d = 64: forward A(vals) X, dX = A^T dY and d vals_e = <dY[row_e], X[col_e]> on an unsorted
    COO with duplicate entries and a multi-chunk row -- exact mode"""
    from mmrec_amd import hip_ops
    rng = np.random.default_rng(500 + d)
    n_rows, n_cols = 600, 400
    deg = rng.integers(0, 25, n_rows)
    deg[[1, 2, n_rows - 1]] = [1100, 0, 300]
    r = np.repeat(np.arange(n_rows), deg)
    c = rng.integers(0, n_cols, r.size)
    c[deg[0] + 1:deg[0] + 20] = c[deg[0]]
    perm = rng.permutation(r.size)
    r, c = r[perm], c[perm]
    v = (rng.integers(-8, 9, r.size) / 8.0).astype(np.float32)
    X, dY = _grid(rng, (n_cols, d)), _grid(rng, (n_rows, d))
    dyn = hip_ops.DynGraph(_on(r), _on(c), n_rows, n_cols, long_row_threshold=32)
    Xt, vt = _on(X).requires_grad_(), _on(v).requires_grad_()
    out = hip_ops.spmm_vals(dyn, Xt, vt)
    assert tuple(out.shape) == (n_rows, d)
    out.backward(_on(dY))
    torch.cuda.synchronize()
    A = edge_matrix(r, c, v, (n_rows, n_cols))
    check(out.detach(), [(1.0, A, X)], exact=True, name="spmm_vals d %d" % d)
    check(Xt.grad, [(1.0, A.T, dY)], exact=True, name="spmm_vals dX d %d" % d)
    check_dots(vt.grad, dY, X, r, c, exact=True, name="spmm_vals d vals d %d" % d)


@pytest.mark.gpu
def test_switch_off_and_unserved_widths_take_the_composition(monkeypatch):
    from mmrec_amd import hip_ops
    rng = np.random.default_rng(8)
    A0, _, r, k, g = _hub_case(rng, 64, ne=5000, n=400)
    rows, cols = _on(r), _on(k)
    calls = []
    real = hip_ops._edge_dot_fwd
    monkeypatch.setattr(hip_ops, "_edge_dot_fwd", lambda *a: calls.append(1) or real(*a))
    A = _on(A0)
    on = hip_ops.edge_dot(A, A, rows, cols)
    assert calls == [1]
    monkeypatch.setattr(hip_ops, "EDGE_DOT", False)
    assert not hip_ops.edge_dot_served(A, A, rows, cols)
    off = hip_ops.edge_dot(A, A, rows, cols)
    assert calls == [1]
    np.testing.assert_allclose(off.cpu().numpy(), on.cpu().numpy(), rtol=1e-4, atol=1e-5)
    monkeypatch.setattr(hip_ops, "EDGE_DOT", True)
    W = _on(np.ascontiguousarray(A0[:, :40]))                         # a width the kernels do not have
    assert not hip_ops.edge_dot_served(W, W, rows, cols)
    assert torch.equal(hip_ops.edge_dot(W, W, rows, cols), (W[rows] * W[cols]).sum(-1)) and calls == [1]
