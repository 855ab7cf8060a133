"""The row schedule of large graphs (CsrGraph(row_schedule=...), mmrec_spmm_csr_sched_f32[_layergcn], mmrec_spmm_row_keys):
the scheduled launch against the identity launch on the SAME arrays, torch.equal on every output the call writes (a row's sum
runs over the same entries in the same order, so not one bit may move), and the schedule itself against a numpy restatement
of its rule.  Small graphs, schedule forced with row_schedule=True; one 300,000-column graph for the default-on size rule."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

NAN = float("nan")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    return torch.device("cuda:0")


# ---- graphs ------------------------------------------------------------------------------------------------------------
def _coo_from_degrees(deg, n_cols, rng, fixed=None):
    rows = np.repeat(np.arange(len(deg), dtype=np.int64), deg)
    cols = rng.integers(0, n_cols, rows.shape[0])
    rp = np.concatenate([[0], np.cumsum(deg)])
    for r, cs in (fixed or {}).items():
        cols[rp[r]:rp[r + 1]] = cs
    vals = (rng.random(rows.shape[0]) - 0.5).astype(np.float32)
    return np.stack([rows, cols]), vals


def rect_arrays():
    """777 x 1,234 (threshold 16): empty rows at the start, the middle and the end, rows of exactly 16 and 17 nonzeros, one
    row of 1,300 (three chunks: finished by the last-arriving chunk block) between short rows, duplicate column ids"""
    rng = np.random.default_rng(11)
    deg = rng.integers(0, 15, 777)
    deg[[0, 1, 2, 400, 401, 775, 776]] = 0
    deg[[10, 300]] = 16
    deg[[11, 301]] = 17
    deg[[50, 51, 52]] = [3, 1300, 2]
    deg[[600, 601]] = [40, 700]
    deg[5] = 5
    idx, val = _coo_from_degrees(deg, 1234, rng, fixed={5: [7, 7, 7, 3, 3]})
    return idx, val, 777, 1234, False


def sym_arrays():
    """5,000 x 5,000 symmetric in structure and values, one hub of about 1,300 neighbours"""
    rng = np.random.default_rng(12)
    a, b = rng.integers(0, 5000, 16000), rng.integers(0, 5000, 16000)
    hub = rng.choice(5000, 1300, replace=False)
    a, b = np.concatenate([a, np.full(1300, 123)]), np.concatenate([b, hub])
    keep = a != b
    a, b = a[keep], b[keep]
    key = np.unique(np.minimum(a, b) * 5000 + np.maximum(a, b))
    a, b = key // 5000, key % 5000
    v = (rng.random(a.shape[0]) - 0.5).astype(np.float32)
    return np.stack([np.concatenate([a, b]), np.concatenate([b, a])]), np.concatenate([v, v]), 5000, 5000, True


def all_long_arrays():
    rng = np.random.default_rng(13)
    idx, val = _coo_from_degrees(rng.integers(17, 60, 90), 500, rng)
    return idx, val, 90, 500, False


def no_long_arrays():
    rng = np.random.default_rng(14)
    idx, val = _coo_from_degrees(rng.integers(0, 17, 1000), 1500, rng)
    return idx, val, 1000, 1500, False


ARRAYS = {"rect": rect_arrays, "sym": sym_arrays, "all_long": all_long_arrays, "no_long": no_long_arrays}
_pairs = {}


def pair(name, dev):
    """(scheduled, identity) CsrGraphs over the same device arrays, built once"""
    if name not in _pairs:
        from mmrec_amd import hip_ops
        idx, val, nr, nc, sym = ARRAYS[name]()
        ident = hip_ops.CsrGraph.from_coo_host(idx, val, nr, nc, dev, symmetric=sym, row_schedule=False)
        sched = hip_ops.CsrGraph(ident.rowptr, ident.colidx, ident.vals, nr, nc, symmetric=sym, rowptr_host=ident.rowptr_host,
                                 row_schedule=True)
        _pairs[name] = (sched, ident)
    return _pairs[name]


def rand(shape, dev, seed):
    return torch.rand(shape, device=dev, generator=torch.Generator(device=dev).manual_seed(seed)) - 0.5


def same(got, ref):
    """bitwise equal, and every row written (the buffers start as NaN; the identity launch visits every row)"""
    return not bool(torch.isnan(ref).any()) and torch.equal(got, ref)


EPILOGUES = ("plain", "z_beta", "acc", "acc_only", "alpha")


def run_epilogue(g, X, kind, Z, A0):
    from mmrec_amd import hip_ops
    new = lambda: torch.full((g.n_rows, X.shape[1]), NAN, device=X.device)
    if kind == "plain":
        Y = new()
        hip_ops.spmm_raw(g, X, Y=Y)
        return (Y,)
    if kind == "z_beta":
        Y = new()
        hip_ops.spmm_raw(g, X, Y=Y, Z=Z, beta=1.75)
        return (Y,)
    if kind == "acc":
        Y, acc = new(), new()
        hip_ops.spmm_raw(g, X, Y=Y, acc_in=A0, acc_out=acc, acc_scale=0.25)
        return Y, acc
    if kind == "acc_only":
        acc = new()
        hip_ops.spmm_raw(g, X, Y=None, acc_in=A0, acc_out=acc, acc_scale=0.5)
        return (acc,)
    Y, acc = new(), new()
    hip_ops.spmm_raw(g, X, Y=Y, Z=Z, acc_in=A0, acc_out=acc, alpha=0.37, beta=-1.5, acc_scale=0.125)
    return Y, acc


# ---- the scheduled launch against the identity launch --------------------------------------------------------------------
@pytest.mark.parametrize("name", list(ARRAYS))
@pytest.mark.parametrize("d", [64, 128, 384])
def test_scheduled_equals_identity(dev, name, d):
    gs, gi = pair(name, dev)
    assert gs.sched is not None and gi.sched is None
    assert gs.sched["n_short"] == gs.n_rows - gs.n_long
    if name == "rect":
        assert gs.sched["n_short"] % 64 and gs.n_chunks > gs.n_long > 0       # a ragged last block; multi-chunk rows
    if name == "sym":
        assert gs.sched["n_short"] % 64 and gs.max_row_chunks == 3
    if name == "all_long":
        assert gs.sched["n_short"] == 0
    if name == "no_long":
        assert gs.n_long == 0
    X = rand((gs.n_cols, d), dev, 1)
    Z, A0 = rand((gs.n_rows, d), dev, 2), rand((gs.n_rows, d), dev, 3)
    for kind in EPILOGUES:
        ref = run_epilogue(gi, X, kind, Z, A0)
        got = run_epilogue(gs, X, kind, Z, A0)
        again = run_epilogue(gs, X, kind, Z, A0)
        for a, b, c in zip(got, ref, again):
            assert same(a, b), (name, d, kind)
            assert torch.equal(a, c), (name, d, kind, "second launch")
        if gs.long_tickets is not None:
            assert int(gs.long_tickets.abs().sum()) == 0


def _layergcn_call(g, X, ego, acc_in, sched):
    from mmrec_amd import _lib, hip_ops
    lib, P = _lib.load(), hip_ops._p
    n = g.n_rows
    Y, scaled, acc = (torch.full((n, 64), NAN, device=X.device) for _ in range(3))
    w = torch.full((n,), NAN, device=X.device)
    args = (P(g.rowptr), P(g.colidx), P(g.vals), P(X), P(Y), P(ego), P(scaled), P(w), P(acc_in), P(acc), n, 64,
            g.long_row_threshold, P(g.long_rows), P(g.long_chunk_ptr), g.n_long, g.n_chunks, P(g.partials_for(64)),
            P(g.long_tickets))
    if sched:
        sc = g.sched
        rc = lib.mmrec_spmm_csr_sched_f32_layergcn(*args, P(sc["row"]), P(sc["span"]), P(sc["col"]), P(sc["val"]), sc["n_short"],
                                                   hip_ops._stream())
    else:
        rc = lib.mmrec_spmm_csr_f32_layergcn(*args, hip_ops._stream())
    assert rc == 0
    return Y, scaled, w, acc


def test_layergcn_epilogue(dev):
    from mmrec_amd import hip_ops
    gs, gi = pair("sym", dev)
    X, ego, A0 = rand((5000, 64), dev, 4), rand((5000, 64), dev, 5), rand((5000, 64), dev, 6)
    for acc_in in (None, A0):
        ref = _layergcn_call(gi, X, ego, acc_in, False)
        got = _layergcn_call(gs, X, ego, acc_in, True)
        for a, b in zip(got, ref):
            assert same(a, b)
    assert int(gs.long_tickets.abs().sum()) == 0
    # and through the op (which picks the entry itself), forward and backward
    outs = []
    for g in (gi, gs):
        E = X.clone().requires_grad_(True)
        out = hip_ops.layergcn_sum(g, E, 2)
        out.backward(A0)
        outs.append((out.detach(), E.grad))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])


def test_width_rules_of_the_entry(dev):
    """d = 64 k only: the feature slices keep the identity entry (host-side argument check: nothing is launched)"""
    from mmrec_amd import _lib
    lib = _lib.load()
    none = [None] * 8
    for d, rc in ((32, 10002), (24, 10002), (448, 10002)):
        assert lib.mmrec_spmm_csr_sched_f32(*none, 10, d, 1.0, 0.0, 1.0, 16, None, None, 0, 0, None, None,
                                            None, None, None, None, 10, None) == rc
    assert lib.mmrec_spmm_csr_sched_f32(*none, 10, 64, 1.0, 0.0, 1.0, 16, None, None, 0, 0, None, None,
                                        None, None, None, None, 10, None) == 10001
    assert lib.mmrec_spmm_row_keys(None, None, None, 5, 16, 128, None, None, None) == 10001


def test_feature_slice_keeps_identity_path(dev):
    from mmrec_amd import hip_ops
    gs, gi = pair("rect", dev)
    X = rand((gs.n_cols, 32), dev, 7)
    assert gs.scheduled(32) is None and gs.scheduled(64) is not None
    a, b = torch.full((gs.n_rows, 32), NAN, device=dev), torch.full((gs.n_rows, 32), NAN, device=dev)
    hip_ops.spmm_raw(gs, X, Y=a)
    hip_ops.spmm_raw(gi, X, Y=b)
    assert same(a, b)


def test_row_block_shard(dev):
    from mmrec_amd import hip_ops
    gs, gi = pair("rect", dev)
    X = rand((gs.n_cols, 64), dev, 8)
    whole = torch.full((gs.n_rows, 64), NAN, device=dev)
    hip_ops.spmm_raw(gs, X, Y=whole)
    for r0, r1 in ((0, 777), (3, 60), (40, 611), (700, 777)):
        blk = gs.row_block(r0, r1)
        assert blk.sched is not None and blk.sched["n_short"] == blk.n_rows - blk.n_long
        assert gi.row_block(r0, r1).sched is None
        Y = torch.full((r1 - r0, 64), NAN, device=dev)
        hip_ops.spmm_raw(blk, X, Y=Y)
        assert same(Y, whole[r0:r1])


def test_graph_replay(dev):
    from mmrec_amd import hip_ops
    gs, gi = pair("sym", dev)
    X = rand((5000, 64), dev, 9)
    ref = torch.empty(5000, 64, device=dev)
    hip_ops.spmm_raw(gi, X, Y=ref)
    Y = torch.empty_like(ref)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        hip_ops.spmm_raw(gs, X, Y=Y)
        cg = torch.cuda.CUDAGraph()
        with torch.cuda.graph(cg, stream=side):
            hip_ops.spmm_raw(gs, X, Y=Y)
    torch.cuda.current_stream().wait_stream(side)
    for _ in range(2):
        Y.fill_(NAN)
        cg.replay()
        torch.cuda.synchronize()
        assert same(Y, ref)
        assert int(gs.long_tickets.abs().sum()) == 0
    del cg


def test_default_on_above_2_18_columns(dev):
    """300,000 x 300,000, about 1.5M nonzeros: a schedule without being asked, bitwise the row_schedule=False result"""
    from mmrec_amd import hip_ops
    rng = np.random.default_rng(15)
    n = 300_000
    deg = rng.integers(0, 10, n)
    deg[rng.choice(n, 2000, replace=False)] = rng.integers(33, 90, 2000)
    deg[77] = 1300
    cols_pop = (n * rng.random(int(deg.sum())) ** 2.0).astype(np.int64)          # skewed: hot and cold columns
    rows = np.repeat(np.arange(n, dtype=np.int64), deg)
    val = (rng.random(rows.shape[0]) - 0.5).astype(np.float32)
    assert 1_200_000 < rows.shape[0] < 1_800_000
    g = hip_ops.CsrGraph.from_coo_host(np.stack([rows, cols_pop]), val, n, n, dev)
    g0 = hip_ops.CsrGraph(g.rowptr, g.colidx, g.vals, n, n, rowptr_host=g.rowptr_host, row_schedule=False)
    assert g.sched is not None and g.long_row_threshold == 32 and g0.sched is None
    assert g.sched["n_short"] == n - g.n_long and g.n_long >= 2000
    assert g.schedule_bytes() == 8 * int(g.sched["span"][-1, 1]) + 12 * g.sched["n_short"]
    X = rand((n, 64), dev, 10)
    Y, Y0 = torch.full((n, 64), NAN, device=dev), torch.full((n, 64), NAN, device=dev)
    hip_ops.spmm_raw(g, X, Y=Y)
    hip_ops.spmm_raw(g0, X, Y=Y0)
    assert same(Y, Y0)
    small = hip_ops.CsrGraph(g.rowptr[:1001].contiguous(), g.colidx, g.vals, 1000, 1 << 18)
    assert small.sched is None           # the size rule: strictly more than 2^18 columns


# ---- the schedule itself, against the rule restated in numpy ---------------------------------------------------------------
def numpy_schedule(rp, col, n_rows, n_cols, symmetric, long_t, deg_max):
    rp = rp.astype(np.int64)
    deg = np.diff(rp)
    coldeg = deg if symmetric else np.bincount(col, minlength=n_cols)
    recs = []
    for r in range(n_rows):
        if deg[r] > long_t:
            continue
        cs = col[rp[r]:rp[r + 1]]
        key, kd = -1, 0
        for c in cs:                                   # the largest column degree <= deg_max, the first among equals
            if coldeg[c] <= deg_max and coldeg[c] > kd:
                key, kd = int(c), int(coldeg[c])
        ref = key if key >= 0 else (int(cs[0]) if len(cs) else -1)
        band = 0 if ref > r else 1
        recs.append((band, -kd, key if key >= 0 else 0, r, key))
    recs.sort(key=lambda t: t[:4])
    return recs


@pytest.mark.parametrize("name", ["rect", "sym", "no_long", "all_long"])
def test_schedule_follows_the_rule(dev, name):
    from mmrec_amd import hip_ops
    gs, _ = pair(name, dev)
    sc = gs.sched
    rp, col, val = gs.rowptr_host.astype(np.int64), gs.colidx.cpu().numpy(), gs.vals.cpu().numpy()
    recs = numpy_schedule(rp, col, gs.n_rows, gs.n_cols, gs.symmetric, gs.long_row_threshold, hip_ops.spmm_key_deg_max())
    rows, span = sc["row"].cpu().numpy(), sc["span"].cpu().numpy()
    deg = np.diff(rp)
    assert sc["n_short"] == rows.shape[0] == len(recs)
    assert sorted(rows.tolist()) == np.flatnonzero(deg <= gs.long_row_threshold).tolist()      # a permutation of the short rows
    assert rows.tolist() == [t[3] for t in recs]
    by_row = {t[3]: t for t in recs}
    tup = [by_row[r][:4] for r in rows.tolist()]
    bands = [t[0] for t in tup]
    assert bands == sorted(bands)                                                             # band 0 precedes band 1
    assert all(a < b for a, b in zip(tup, tup[1:]))                                           # (-key degree, key, row) ascend
    key_dev, kdeg_dev = gs.row_key.cpu().numpy(), gs.row_key_degree.cpu().numpy()
    for t in recs:
        assert key_dev[t[3]] == t[4] and kdeg_dev[t[3]] == -t[1]
    assert span.shape == (rows.shape[0], 2) and (rows.shape[0] == 0 or span[0, 0] == 0)
    assert np.array_equal(span[1:, 0], span[:-1, 1])                                          # packed, no gaps
    scol, sval = sc["col"].cpu().numpy(), sc["val"].cpu().numpy()
    for r, (s, e) in zip(rows.tolist(), span.tolist()):
        assert np.array_equal(scol[s:e], col[rp[r]:rp[r + 1]]) and np.array_equal(sval[s:e], val[rp[r]:rp[r + 1]])
    if name in ("rect", "sym"):
        assert len({t[4] for t in recs if t[4] >= 0}) > 50 and any(t[4] < 0 for t in recs)    # many keys; rows without one
    again = hip_ops.CsrGraph(gs.rowptr, gs.colidx, gs.vals, gs.n_rows, gs.n_cols, symmetric=gs.symmetric,
                             rowptr_host=gs.rowptr_host, row_schedule=True).sched
    for k in ("row", "span", "col", "val"):
        assert torch.equal(again[k], sc[k])


def test_key_degree_ceiling(dev, monkeypatch):
    """MMREC_SPMM_KEY_DEG_MAX moves the ceiling (sweeps); the result stays the identity launch's"""
    from mmrec_amd import hip_ops
    gs, gi = pair("sym", dev)
    monkeypatch.setenv("MMREC_SPMM_KEY_DEG_MAX", "6")
    g6 = hip_ops.CsrGraph(gs.rowptr, gs.colidx, gs.vals, 5000, 5000, symmetric=True, rowptr_host=gs.rowptr_host, row_schedule=True)
    assert int(g6.row_key_degree.max()) == 6 and int(gs.row_key_degree.max()) > 6
    X = rand((5000, 64), dev, 16)
    a, b = torch.full((5000, 64), NAN, device=dev), torch.full((5000, 64), NAN, device=dev)
    hip_ops.spmm_raw(g6, X, Y=a)
    hip_ops.spmm_raw(gi, X, Y=b)
    assert same(a, b)


# ---- callers with their own values keep the identity path -----------------------------------------------------------------
def test_substituted_values_fall_back(dev):
    from mmrec_amd import hip_ops
    idx, val, nr, nc, sym = rect_arrays()
    gs = hip_ops.CsrGraph.from_coo_host(idx, val, nr, nc, dev, row_schedule=True)
    gi = hip_ops.CsrGraph(gs.rowptr, gs.colidx, gs.vals, nr, nc, rowptr_host=gs.rowptr_host, row_schedule=False)
    X = rand((nc, 64), dev, 17)
    other = rand((gs.nnz,), dev, 18)
    assert gs.scheduled(64) is not None
    got = hip_ops._spmm_with(gs, other, X)                   # swaps g.vals: the packed copy no longer matches
    assert gs.scheduled(64) is None
    ref = hip_ops._spmm_with(gi, other, X)
    assert torch.equal(got, ref)


def test_dyn_graph_has_no_schedule(dev):
    from mmrec_amd import hip_ops
    rng = np.random.default_rng(19)
    n = 270_000                                              # more than 2^18 columns: a CsrGraph would schedule by default
    rows = torch.from_numpy(rng.integers(0, n, 400_000)).to(dev)
    cols = torch.from_numpy(rng.integers(0, n, 400_000)).to(dev)
    dyn = hip_ops.DynGraph(rows, cols, n, n)
    assert dyn.fwd.sched is None and dyn.bwd.sched is None
    vals = rand((400_000,), dev, 20).requires_grad_(True)
    X = rand((n, 64), dev, 21)
    Y = hip_ops.spmm_vals(dyn, X, vals)
    ref_g = hip_ops.CsrGraph(dyn.fwd.rowptr, dyn.fwd.colidx, vals.detach()[dyn.perm].contiguous(), n, n, row_schedule=True)
    ref = torch.full((n, 64), NAN, device=dev)
    hip_ops.spmm_raw(ref_g, X, Y=ref)
    assert same(Y.detach(), ref)


def test_row_schedule_false_allocates_nothing(dev):
    from mmrec_amd import hip_ops
    idx, val, nr, nc, sym = no_long_arrays()
    g = hip_ops.CsrGraph.from_coo_host(idx, val, nr, nc, dev, row_schedule=True)
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    g0 = hip_ops.CsrGraph(g.rowptr, g.colidx, g.vals, nr, nc, rowptr_host=g.rowptr_host, row_schedule=False)
    torch.cuda.synchronize()
    assert torch.cuda.memory_allocated() == before
    assert g0.sched is None and g0.schedule_bytes() == 0 and not hasattr(g0, "row_key")
    assert g.schedule_bytes() == 8 * g.nnz + 12 * nr
