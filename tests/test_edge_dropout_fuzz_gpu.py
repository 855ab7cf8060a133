"""GPU: edge dropout inside the SpMM against float64 on the host, never against another masked form: the pack kernel
(mmrec_edge_keep_bits) against host-packed words; the raw masked launch (mmrec_spmm_csr_masked_f32) over the seeded cases of
tests/test_edge_dropout_cpu.py -- every row degree around the span, word, threshold and chunk sizes, every threshold, keep
pattern and epilogue, both long-row finishes, both rows-per-group regimes, d = 64 / 128 / 384 -- in the two acceptance modes of
tests/test_spmm_fuzz_gpu.py (exact: equality with float64; float: |err| <= gamma(n) M + n 2^-149 with that file's plan depth
plus one for vals * val_scale); and the two autograd ops.  tests/test_edge_dropout_cpu.py shows (without a GPU) that this
check passes an fp32 emulation of the plan and rejects every planted mask error.

Two equalities carry most of the weight: with every bit set and val_scale = 1 the output and dX are BIT-IDENTICAL to the
unmasked launch; with a random mask and finite X they EQUAL the unmasked launch on the zero-valued form."""
import numpy as np
import pytest
import torch

from tests.test_edge_dropout_cpu import CASES, check_case, draw_case, masked_csr, masked_depth, pack_bits
from tests.test_spmm_fuzz_gpu import (_grid, _on, _square_graph, _tickets, _tickets_zero, absolute, check, gamma, plan_depth)

pytestmark = pytest.mark.gpu


def _bits(t):
    return t.view(torch.int32)


def _words(t):
    return t.cpu().numpy().view(np.uint32)


# ------------------------------------------------------------------------------------------------ the pack kernel
@pytest.mark.parametrize("E", [0, 1, 63, 64, 65, 4097])
def test_pack_kernel_equals_host_packing(E):
    from mmrec_amd import hip_ops
    rng = np.random.default_rng(E)
    for p_keep in (0.5, 0.0, 1.0):
        keep = rng.random(E) < p_keep
        pa, pb = rng.permutation(E), rng.permutation(E)
        kt = _on(keep)
        n_words = max((E + 31) // 32, 1)
        want = lambda perm: np.concatenate([pack_bits(keep[perm]), np.zeros(n_words - (E + 31) // 32, np.uint32)])   # noqa: E731
        a, none = hip_ops.edge_keep_bits(kt)                          # identity, one output
        assert none is None and np.array_equal(_words(a), want(np.arange(E)))
        a, b = hip_ops.edge_keep_bits(kt, _on(pa), _on(pb))           # two orders in one launch
        assert np.array_equal(_words(a), want(pa)) and np.array_equal(_words(b), want(pb))
        a, b = hip_ops.edge_keep_bits(kt, None, _on(pb))              # identity + a permutation
        assert np.array_equal(_words(a), want(np.arange(E))) and np.array_equal(_words(b), want(pb))
        a, _ = hip_ops.edge_keep_bits(kt.to(torch.uint8) * 7, _on(pa))    # uint8: any nonzero byte is kept
        assert np.array_equal(_words(a), want(pa))
        if E % 32:                                                    # the trailing bits of the last word are zero
            assert int(_words(a)[-1]) >> (E % 32) == 0


# ------------------------------------------------------------------------------------------------ the raw launch, fuzzed
def _raw(c, g, bits, tickets):
    from mmrec_amd import hip_ops
    nan = lambda: torch.full((c.n_rows, c.d), float("nan"), device="cuda:0")      # noqa: E731
    Y = nan() if c.epi in ("Y", "Yacc", "YZ") else None
    Z = _on(c.Z) if c.epi == "YZ" else None
    acc_in, acc = (_on(c.acc_in), nan()) if c.epi in ("acc", "Yacc") else (None, None)
    hip_ops.spmm_masked_raw(g, g.vals, bits, _on(c.X), Y=Y, Z=Z, acc_in=acc_in, acc_out=acc, alpha=c.alpha, beta=c.beta,
                            acc_scale=c.acc_scale, val_scale=c.scale, tickets=tickets)
    torch.cuda.synchronize()
    return check_case(c, Y=Y, acc=acc, name="tickets %s" % tickets)


@pytest.mark.parametrize("seed", range(CASES))
def test_masked_spmm_fuzz(seed):
    from mmrec_amd import hip_ops
    c = draw_case(seed)
    g = hip_ops.CsrGraph.from_coo_host(np.stack([c.rows, c.cols]), c.vals, c.n_rows, c.n_cols, torch.device("cuda:0"),
                                       long_row_threshold=c.thr, row_schedule=False)
    assert g.long_row_threshold == c.thr_eff and g.nnz == c.keep.size
    bits, _ = hip_ops.edge_keep_bits(_on(c.keep))
    assert np.array_equal(_words(bits)[:(g.nnz + 31) // 32], pack_bits(c.keep))
    forms = (True, False) if g.n_chunks > g.n_long else (True,)      # the last-arriver finish and the two-launch finish
    worst = 0.0
    for tickets in forms:
        worst = max(worst, _raw(c, g, bits, tickets))
        _tickets_zero(g)
    print("masked spmm fuzz seed %d: d %d thr %s %s %s %s rows %d nnz %d kept %d scale %.4g forms %d worst err/M %.3e" % (
        seed, c.d, c.thr, "exact" if c.exact else "float", c.epi, c.pattern, c.n_rows, g.nnz, int(c.keep.sum()), c.scale,
        len(forms), worst))


# ------------------------------------------------------------------------------------------------ graphs for the ops
def _dyn_case(rng, n_rows, n_cols, deg, thr=32, shuffle=True):
    """a DynGraph over a shuffled COO (edge order != CSR order) + its host arrays and a value vector in edge order"""
    from mmrec_amd import hip_ops
    deg = np.asarray(deg, np.int64)
    r = np.repeat(np.arange(n_rows), deg)
    c = rng.integers(0, n_cols, r.size)
    if shuffle:
        p = rng.permutation(r.size)
        r, c = r[p], c[p]
    dyn = hip_ops.DynGraph(_on(r), _on(c), n_rows, n_cols, long_row_threshold=thr)
    return dyn, r, c


def _host_csr(r, c, v, keep, scale, n_rows, n_cols):
    """float64 masked matrix of a COO in edge order (entries of a row in edge order, as the stable sort leaves them)"""
    order = np.argsort(r, kind="stable")
    rowptr = np.zeros(n_rows + 1, np.int64)
    np.cumsum(np.bincount(r, minlength=n_rows), out=rowptr[1:])
    return masked_csr(rowptr, c[order], v[order], keep[order], scale, (n_rows, n_cols)), np.diff(rowptr)


def _baby_like(rng):
    """a [users; items] bipartite graph, symmetric structure, power-law item degrees, a few rows of several chunks"""
    nu, ni, E = 1900, 700, 14000
    u = rng.integers(0, nu, E)
    i = np.minimum((rng.pareto(1.2, E) * 6).astype(np.int64), ni - 1)
    r, c = np.concatenate([u, nu + i]), np.concatenate([nu + i, u])
    return nu + ni, r, c


def _multi_chunk(rng):
    n = 900
    deg = rng.integers(0, 30, n)
    deg[[0, 450, n - 1]] = [1300, 700, 2100]
    deg[[5, 6]] = 0
    r = np.repeat(np.arange(n), deg)
    c = rng.integers(0, n, r.size)
    c[rng.random(r.size) < 0.05] = 3                                  # a column of several chunks for the transposed side
    return n, r, c


@pytest.mark.parametrize("shape", ["baby_like", "multi_chunk"])
@pytest.mark.parametrize("d", [64, 128])
def test_all_bits_set_is_bit_identical_to_the_unmasked_launch(shape, d):
    """every bit set, val_scale = 1: spmm_edge_dropout and its dX carry the bits of spmm_vals (the unmasked launch on both
    sides), the raw launch those of spmm_raw -- with tickets and without"""
    from mmrec_amd import hip_ops
    rng = np.random.default_rng(11 + d)
    n, r, c = (_baby_like if shape == "baby_like" else _multi_chunk)(rng)
    p = rng.permutation(r.size)
    r, c = r[p], c[p]
    dyn = hip_ops.DynGraph(_on(r), _on(c), n, n, long_row_threshold=None if shape == "baby_like" else 32)
    assert dyn.fwd.n_chunks > dyn.fwd.n_long and dyn.bwd.n_chunks > dyn.bwd.n_long
    v = _on(rng.standard_normal(r.size).astype(np.float32) * 0.1)
    X, G = rng.standard_normal((n, d)).astype(np.float32), rng.standard_normal((n, d)).astype(np.float32)
    eg = hip_ops.EdgeDropoutGraph(dyn, v)
    keep = torch.ones(r.size, dtype=torch.bool, device="cuda:0")
    Xa, Xb = _on(X).requires_grad_(), _on(X).requires_grad_()
    ya = hip_ops.spmm_edge_dropout(eg, Xa, keep, 1.0)
    ya.backward(_on(G))
    yb = hip_ops.spmm_vals(dyn, Xb, v)
    yb.backward(_on(G))
    torch.cuda.synchronize()
    assert torch.equal(_bits(ya.detach()), _bits(yb.detach())) and torch.equal(_bits(Xa.grad), _bits(Xb.grad))
    g = dyn.fwd                                                       # (its vals are now v[perm]: spmm_vals left them there)
    bits, _ = hip_ops.edge_keep_bits(keep)
    for tickets in (True, False):
        with _tickets(tickets, g):
            want = hip_ops.spmm_raw(g, _on(X), Y=torch.empty(n, d, device="cuda:0"))
        got = hip_ops.spmm_masked_raw(g, eg.vals_fwd, bits, _on(X), Y=torch.empty(n, d, device="cuda:0"), tickets=tickets)
        torch.cuda.synchronize()
        assert torch.equal(_bits(got), _bits(want)), tickets
    _tickets_zero(dyn.fwd, dyn.bwd)
    assert float(ya.abs().max()) > 0 and float(Xa.grad.abs().max()) > 0


@pytest.mark.parametrize("shape", ["baby_like", "multi_chunk"])
def test_random_mask_equals_the_zero_valued_form(shape):
    """random mask, random finite X: spmm_edge_dropout and its dX equal, as numbers, spmm_vals on (vals * keep) * scale -- a
    dropped entry adds fma(+0, x, acc) = acc there and nothing here; the kept ones meet at the same places of the same sums.
    Two identical calls repeat bit for bit, forward and backward (no atomics); the shared DynGraph keeps serving spmm_vals."""
    from mmrec_amd import hip_ops
    rng = np.random.default_rng(23)
    n, r, c = (_baby_like if shape == "baby_like" else _multi_chunk)(rng)
    p = rng.permutation(r.size)
    r, c = r[p], c[p]
    dyn = hip_ops.DynGraph(_on(r), _on(c), n, n, long_row_threshold=None if shape == "baby_like" else 32)
    v = _on(rng.uniform(0.01, 0.2, r.size).astype(np.float32))
    eg = hip_ops.EdgeDropoutGraph(dyn, v)
    X, G = rng.standard_normal((n, 64)).astype(np.float32), rng.standard_normal((n, 64)).astype(np.float32)
    for rate in (0.1, 0.5, 0.9):
        keep = _on(rng.random(r.size) >= rate)
        scale = 1.0 / (1.0 - rate)
        outs = []
        for _ in range(2):
            Xa = _on(X).requires_grad_()
            ya = hip_ops.spmm_edge_dropout(eg, Xa, keep, scale)
            ya.backward(_on(G))
            outs.append((ya.detach(), Xa.grad))
        Xb = _on(X).requires_grad_()
        yb = hip_ops.spmm_vals(dyn, Xb, (v * keep.to(v.dtype)) * scale)
        yb.backward(_on(G))
        torch.cuda.synchronize()
        assert torch.equal(outs[0][0], yb.detach()) and torch.equal(outs[0][1], Xb.grad), rate
        assert torch.equal(_bits(outs[0][0]), _bits(outs[1][0])) and torch.equal(_bits(outs[0][1]), _bits(outs[1][1])), rate
        assert bool(torch.isfinite(yb).all()) and float(yb.abs().max()) > 0
    _tickets_zero(dyn.fwd, dyn.bwd)


def test_dropped_entry_with_nan_source_row_contributes_nothing():
    """the one intended difference from the zero-valued form: a DROPPED entry whose source row is NaN / inf leaves the output
    finite (the reference removes the entry); a kept one propagates it"""
    from mmrec_amd import hip_ops
    rng = np.random.default_rng(31)
    n = 400
    deg = rng.integers(1, 20, n)
    deg[3], deg[4] = 1100, 40                                         # a row of several chunks, a single-chunk long row
    dyn, r, c = _dyn_case(rng, n, n, deg)
    bad_col = 17
    v = _on(rng.uniform(0.1, 1.0, r.size).astype(np.float32))
    eg = hip_ops.EdgeDropoutGraph(dyn, v)
    X = rng.standard_normal((n, 64)).astype(np.float32)
    X[bad_col, ::2], X[bad_col, 1::2] = np.nan, np.inf
    hit = np.unique(r[c == bad_col])
    assert {3, 4} <= set(hit.tolist()) or hit.size > 5
    keep = rng.random(r.size) < 0.5
    keep[c == bad_col] = False
    y = hip_ops.spmm_edge_dropout(eg, _on(X), _on(keep), 2.0)
    assert bool(torch.isfinite(y).all())
    zero_valued = hip_ops.spmm_vals(dyn, _on(X), (v * _on(keep).to(v.dtype)) * 2.0)
    assert bool(torch.isnan(zero_valued[_on(hit)]).all())              # (what the composition gives)
    A, dg = _host_csr(r, c, v.cpu().numpy(), keep, 2.0, n, n)
    check(y, [(1.0, A, X)], exact=False, depth=masked_depth(dg, 32), name="NaN row dropped")
    keep[c == bad_col] = True
    y = hip_ops.spmm_edge_dropout(eg, _on(X), _on(keep), 2.0)
    rows_ok = np.setdiff1d(np.arange(n), hit)
    assert bool((~torch.isfinite(y[_on(hit)])).all()) and bool(torch.isfinite(y[_on(rows_ok)]).all())


# ------------------------------------------------------------------------------------------------ autograd against float64
def _square_dyn(rng, symmetric):
    """the graph of test_lightgcn_mean_vs_float64 (n = 1200, about 9000 entries, rows of 1300 / 700 / 520 entries, three empty
    rows) as a DynGraph over a shuffled edge list, its fixed values, and an ASYMMETRIC keep mask (drawn per directed entry)"""
    from mmrec_amd import hip_ops
    n = 1200
    g, A = _square_graph(rng, n, 9000, {0: 1300, 600: 700, n - 1: 520}, [5, 6, 7], symmetric)
    A = A.tocsr()
    r = np.repeat(np.arange(n), np.diff(A.indptr))
    c, v = A.indices.astype(np.int64), A.data.astype(np.float32)
    p = rng.permutation(r.size)
    r, c, v = r[p], c[p], v[p]
    keep = rng.random(r.size) < 0.6
    dyn = hip_ops.DynGraph(_on(r), _on(c), n, n, long_row_threshold=32)
    assert dyn.fwd.n_chunks > dyn.fwd.n_long
    if symmetric:                                                     # the structure is symmetric, the mask is not
        fwd = set(zip(r[keep].tolist(), c[keep].tolist()))
        assert sum((b, a) not in fwd for a, b in list(fwd)[:2000]) > 100
    return n, dyn, hip_ops.EdgeDropoutGraph(dyn, _on(v)), r, c, v, keep


def _float64_mean(M, V, L):
    ref = cur = V.astype(np.float64)
    mag = cabs = np.abs(ref)
    for _ in range(L):
        cur, cabs = np.asarray(M @ cur), np.asarray(absolute(M) @ cabs)
        ref, mag = ref + cur, mag + cabs
    return ref / (L + 1), mag / (L + 1)


@pytest.mark.parametrize("symmetric", [True, False])
@pytest.mark.parametrize("L", [0, 1, 2, 3])
def test_lightgcn_mean_edge_dropout_vs_float64(symmetric, L):
    """forward s sum_l B^l E0 and backward s sum_l (B^T)^l dOut, B = scale * (A o keep), s = 1 / (L + 1), within gamma(N) of the
    same sums on absolute values: N = L x (the plan's deepest row, epilogue included, + 1 for vals * val_scale) + 2"""
    from mmrec_amd import hip_ops
    rng = np.random.default_rng(140 + L + 10 * symmetric)
    n, dyn, eg, r, c, v, keep = _square_dyn(rng, symmetric)
    scale = 1.0 / (1.0 - 0.4)
    B, deg = _host_csr(r, c, v, keep, scale, n, n)
    E0, dOut = rng.standard_normal((n, 64)).astype(np.float32), rng.standard_normal((n, 64)).astype(np.float32)
    E = _on(E0).requires_grad_()
    out = hip_ops.lightgcn_mean_edge_dropout(eg, E, L, _on(keep), scale)
    out.backward(_on(dOut))
    torch.cuda.synchronize()
    assert out.data_ptr() != E.data_ptr()                             # L = 0 returns a copy
    for name, M, dg, V, got in (("forward", B, deg, E0, out.detach()),
                                ("backward", B.T.tocsr(), np.bincount(c, minlength=n), dOut, E.grad)):
        ref, mag = _float64_mean(M, V, L)
        N = L * (int(plan_depth(dg, 32).max()) + 1) + 2
        err = np.abs(got.cpu().double().numpy() - ref)
        ratio = float((err / np.maximum(mag, 1e-300)).max())
        print("lightgcn_mean_edge_dropout L %d %s %s: worst err / M %.3e, bound gamma(%d) = %.3e" % (
            L, "symmetric" if symmetric else "directed", name, ratio, N, gamma(N)))
        assert np.all(err <= gamma(N) * mag + N * 2.0 ** -149), (name, ratio, N)
    _tickets_zero(dyn.fwd, dyn.bwd)


@pytest.mark.parametrize("symmetric", [True, False])
@pytest.mark.parametrize("L", [0, 1, 2, 3])
def test_spmm_edge_dropout_chain_vs_float64(symmetric, L):
    """spmm_edge_dropout applied L times: B^L X forward, (B^T)^L dY backward (one pack per application; the backward of each is
    one masked launch on the transposed side), within gamma(L x (deepest depth + 1)) of the sums on absolute values"""
    from mmrec_amd import hip_ops
    rng = np.random.default_rng(180 + L + 10 * symmetric)
    n, dyn, eg, r, c, v, keep = _square_dyn(rng, symmetric)
    scale = 2.5
    B, deg = _host_csr(r, c, v, keep, scale, n, n)
    X0, dY = rng.standard_normal((n, 64)).astype(np.float32), rng.standard_normal((n, 64)).astype(np.float32)
    X = _on(X0).requires_grad_()
    out, kt = X, _on(keep)
    for _ in range(L):
        out = hip_ops.spmm_edge_dropout(eg, out, kt, scale)
    out.backward(_on(dY))
    torch.cuda.synchronize()
    for name, M, dg, V, got in (("forward", B, deg, X0, out.detach()),
                                ("backward", B.T.tocsr(), np.bincount(c, minlength=n), dY, X.grad)):
        ref, mag = V.astype(np.float64), np.abs(V.astype(np.float64))
        for _ in range(L):
            ref, mag = np.asarray(M @ ref), np.asarray(absolute(M) @ mag)
        N = max(L * (int(plan_depth(dg, 32).max()) + 1), 1)
        err = np.abs(got.cpu().double().numpy() - ref)
        ratio = float((err / np.maximum(mag, 1e-300)).max())
        print("spmm_edge_dropout x %d %s %s: worst err / M %.3e, bound gamma(%d) = %.3e" % (
            L, "symmetric" if symmetric else "directed", name, ratio, N, gamma(N)))
        assert np.all(err <= gamma(N) * mag + N * 2.0 ** -149), (name, ratio, N)


def test_exact_ops_on_a_rectangular_graph_and_the_unserved_width():
    """spmm_edge_dropout on a rectangular graph, X with more rows than the graph has columns, exact mode: d = 64 and 128 through
    the masked kernels, d = 32 (no masked form) and the switch off through the composition -- all equal float64; dX is exactly
    0 on the extra rows of X"""
    from mmrec_amd import hip_ops
    rng = np.random.default_rng(77)
    n_rows, n_cols, x_rows = 500, 350, 371
    deg = rng.integers(0, 25, n_rows)
    deg[[0, 250, n_rows - 1]] = [1500, 0, 600]
    dyn, r, c = _dyn_case(rng, n_rows, n_cols, deg, thr=16)
    v = (rng.integers(-8, 9, r.size) / 8.0).astype(np.float32)
    keep = rng.random(r.size) < 0.5
    eg = hip_ops.EdgeDropoutGraph(dyn, _on(v))
    A, _ = _host_csr(r, c, v, keep, 2.0, n_rows, n_cols)
    for d, switch in ((64, True), (128, True), (32, True), (64, False)):
        X, dY = _grid(rng, (x_rows, d), k=4), _grid(rng, (n_rows, d), k=4)
        hip_ops.EDGE_DROPOUT = switch
        try:
            assert hip_ops.edge_dropout_served(eg, _on(X)) == (switch and d != 32)
            Xt = _on(X).requires_grad_()
            if d == 32 or not switch:                                 # spmm_vals wants X [n_cols, d]
                Xt = _on(X[:n_cols]).requires_grad_()
            out = hip_ops.spmm_edge_dropout(eg, Xt, _on(keep), 2.0)
            out.backward(_on(dY))
        finally:
            hip_ops.EDGE_DROPOUT = True
        torch.cuda.synchronize()
        check(out.detach(), [(1.0, A, X)], exact=True, name="rect d %d switch %s" % (d, switch))
        check(Xt.grad, [(1.0, A.T.tocsr(), dY)], exact=True, name="rect dX d %d switch %s" % (d, switch))
        if Xt.shape[0] > n_cols:
            assert bool((Xt.grad[n_cols:] == 0).all())
    _tickets_zero(dyn.fwd, dyn.bwd)


def test_misuse_is_rejected_before_any_launch():
    from mmrec_amd import _lib, hip_ops
    rng = np.random.default_rng(9)
    n = 300
    deg = rng.integers(0, 20, n)
    deg[4] = 1200
    dyn, r, c = _dyn_case(rng, n, n, deg)
    v = _on(rng.standard_normal(r.size).astype(np.float32))
    eg = hip_ops.EdgeDropoutGraph(dyn, v)
    X = _on(rng.standard_normal((n, 64)).astype(np.float32))
    X0 = X.clone()
    keep = _on(rng.random(r.size) < 0.5)
    bits, _ = hip_ops.edge_keep_bits(keep, dyn.perm)
    Y = torch.full((n, 64), 7.0, device="cuda:0")
    calls = [lambda: hip_ops.spmm_edge_dropout(eg, X, keep.to(torch.uint8)),
             lambda: hip_ops.spmm_edge_dropout(eg, X, keep[:-1]),
             lambda: hip_ops.spmm_edge_dropout(eg, X[:n - 1], keep),
             lambda: hip_ops.spmm_edge_dropout(eg, X.cpu(), keep),
             lambda: hip_ops.spmm_edge_dropout(eg, X, keep.cpu()),
             lambda: hip_ops.lightgcn_mean_edge_dropout(eg, X, 2, keep.float()),
             lambda: hip_ops.lightgcn_mean_edge_dropout(eg, X, -1, keep),
             lambda: hip_ops.EdgeDropoutGraph(dyn, v.clone().requires_grad_()),
             lambda: hip_ops.EdgeDropoutGraph(dyn, v[:-1]),
             lambda: hip_ops.spmm_masked_raw(dyn.fwd, eg.vals_fwd, bits, X, Y=X),
             lambda: hip_ops.spmm_masked_raw(dyn.fwd, eg.vals_fwd, bits, X, acc_in=Y, acc_out=X),
             lambda: hip_ops.spmm_masked_raw(dyn.fwd, eg.vals_fwd, bits, X, Y=Y, acc_out=Y.clone()),
             lambda: hip_ops.spmm_masked_raw(dyn.fwd, eg.vals_fwd, bits[:-1], X, Y=Y),
             lambda: hip_ops.spmm_masked_raw(dyn.fwd, eg.vals_fwd, bits, X[:, :32].contiguous(), Y=Y[:, :32].contiguous())]
    for i, call in enumerate(calls):
        with pytest.raises(_lib.MMRecHipError):
            call()
        torch.cuda.synchronize()
        assert torch.equal(X, X0) and bool((Y == 7.0).all()), i
    _tickets_zero(dyn.fwd, dyn.bwd)
    assert dyn.fwd.vals.abs().sum() == 0 and dyn.bwd.vals.abs().sum() == 0      # the DynGraph's own values were never written
