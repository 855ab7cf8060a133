"""The projection of LISTED rows of a feature table, `hip_ops.linear_rows(table, ids, W, b)` (mmrec_linear_rows_*: the kernels of
`hip_ops.linear` reading row ids[j] of the table where they read row j of X; freedom.py:203-209, bm3.py:102-104 under
`lazy_projection`).

GPU: the float64 differential fuzz of tests/test_linear_fuzz_gpu.py (its `draw_case`, its `check`, its seeds and tolerances) at
the widths the gathered kernels serve, with the drawn X rows planted at random positions of a larger table whose every other
row is NaN -- one wrong row read shows in the output -- and an id list that is unsorted and repeats rows; bit identity with
`hip_ops.linear` on `table.index_select(0, ids)` (what lets the models switch over without a changed number); the zero-row
rule for ids outside the table; a table above 4 GiB; no [n, F] allocation in the forward.
CPU: argument errors of the two entry points, the composition `linear_rows` is off the device, and a twin that shows the
table-gradient checker rejecting planted errors."""
import ctypes

import numpy as np
import pytest
import torch

from tests._cpu_ops import cpu_ops  # noqa: F401  (fixture)
from tests.test_linear_fuzz_gpu import CASES, WIDTHS, check, draw_case

SERVED = (128, 256, 384, 512, 1024, 4096)
SEEDS = [s for s in range(CASES) if WIDTHS[s % len(WIDTHS)] in SERVED]


def plant(seed, X):
    """X's rows at random positions of a table of n_table in [n, 4n] rows, NaN everywhere else; an id list of len(X) positions
    that is not sorted and names some rows twice (the rows those positions would have named stay in the table, unlisted).
    Returns table, ids and the gathered rows table[ids]."""
    rng = np.random.default_rng(100003 + seed)
    n, F = X.shape
    n_table = int(rng.integers(n, 4 * n + 1))
    pos = rng.choice(n_table, size=n, replace=False).astype(np.int64)        # random order: not sorted
    table = np.full((n_table, F), np.nan, dtype=np.float32)
    table[pos] = X
    ids = pos.copy()
    if n >= 2:
        dup = rng.choice(n, size=max(1, n // 8), replace=False)
        ids[dup] = pos[rng.integers(0, n, size=dup.shape[0])]
    return table, ids, table[ids]


def scatter_rows(ids, rows, n_table):
    """S^T rows in float64, S the one-hot [n, n_table] gather matrix of `ids`"""
    out = np.zeros((n_table, rows.shape[1]), dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        np.add.at(out, ids, rows.astype(np.float64))
    return out


def check_table_grad(got, ids, dY, W, dominant=False, name=""):
    """The table's gradient [n_table, F]: rows no id names are exactly 0; listed rows against float64 (S^T dY) W under the
    acceptance rule of tests/test_linear_fuzz_gpu.py::check, the magnitude taken as (S^T |dY|) |W|."""
    n_table = got.shape[0]
    listed = np.zeros(n_table, dtype=bool)
    listed[ids] = True
    assert (got[~listed] == 0).all(), (name, "unlisted rows touched", int((got[~listed] != 0).any(axis=1).sum()))
    rows = np.flatnonzero(listed)
    W64 = W.astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        ref = scatter_rows(ids, dY, n_table)[rows] @ W64
        mag = scatter_rows(ids, np.abs(dY), n_table)[rows] @ np.abs(W64)
        ref32 = np.where(np.abs(ref) > 3.4028234e38, np.sign(ref) * np.inf, ref)
    fin = np.isfinite(ref32) & np.isfinite(mag)
    g = got[rows].astype(np.float64)
    bad_pattern = np.isfinite(g) != fin
    near_overflow = mag > 1e37
    assert not (bad_pattern & ~near_overflow).any(), (name, "non-finite pattern", int((bad_pattern & ~near_overflow).sum()))
    ok = fin & ~near_overflow
    tol = 3e-5 if dominant else 2e-6
    with np.errstate(invalid="ignore"):
        err = np.abs(g - ref32)
        viol = ok & (err > tol * mag + 1e-40)
    assert not viol.any(), (name, int(viol.sum()), float(np.nanmax(np.where(ok, err / (mag + 1e-300), 0))))


def bits(t):
    return t.detach().contiguous().view(torch.int32)


def same_bits(a, b, what):
    assert a.shape == b.shape, (what, a.shape, b.shape)
    assert torch.equal(bits(a), bits(b)), (what, int((bits(a) != bits(b)).sum()))


# ------------------------------------------------------------------------------------------------------------------- CPU
def _lib_or_build():
    import os
    from mmrec_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        from mmrec_amd.build import build
        build(verbose=False)
    return _lib.load()


def test_argument_errors_without_gpu():
    """argument validation of the two entry points happens on the host before any launch"""
    lib = _lib_or_build()
    buf = ctypes.create_string_buffer(64)
    fake = ctypes.c_void_p(ctypes.addressof(buf))           # a non-NULL pointer that is never followed: the calls fail first
    fwd, bwd = lib.mmrec_linear_rows_fwd_f32, lib.mmrec_linear_rows_bwd_f32
    for split in (0, 1):
        assert fwd(None, 10, None, None, None, None, 4, 100, 64, split, None, None) == 10002        # F % 128
        assert fwd(None, 10, None, None, None, None, 4, 4160, 64, split, None, None) == 10002
        assert fwd(None, 10, None, None, None, None, 4, 128, 32, split, None, None) == 10002        # out != 64
        assert fwd(None, 10, None, None, None, None, 4, 128, 64, split, None, None) == 10001        # NULL pointers
        assert fwd(fake, 10, None, fake, None, fake, 4, 128, 64, split, fake, None) == 10001        # no id list
        assert fwd(fake, 10, fake, fake, None, fake, 4, 128, 64, split, None, None) == 10001        # no workspace
        assert fwd(fake, 10, fake, fake, None, fake, -1, 128, 64, split, fake, None) == 10001
        assert fwd(fake, -3, fake, fake, None, fake, 4, 128, 64, split, fake, None) == 10001
        assert fwd(None, 10, None, None, None, None, 0, 128, 64, split, None, None) == 0            # an empty list
    assert bwd(None, None, 10, None, None, None, None, None, 4, 96, 64, None, None) == 10002
    assert bwd(None, None, 10, None, None, None, None, None, 4, 4096, 128, None, None) == 10002
    assert bwd(None, None, 10, None, None, fake, None, None, 4, 4096, 64, fake, None) == 10001      # dW without the table
    assert bwd(fake, fake, 10, None, fake, fake, None, None, 4, 4096, 64, fake, None) == 10001      # dW without the ids
    assert bwd(fake, fake, 10, fake, None, None, None, fake, 4, 4096, 64, fake, None) == 10001      # dX without W
    assert bwd(fake, fake, 10, fake, fake, None, fake, None, 4, 4096, 64, fake, None) == 10001      # db without dW
    assert bwd(None, fake, 10, fake, fake, fake, None, None, 4, 4096, 64, fake, None) == 10001      # no dY
    assert bwd(fake, fake, 10, fake, fake, fake, None, None, 4, 4096, 64, None, None) == 10001      # no workspace
    assert bwd(fake, fake, 10, fake, fake, fake, None, None, -2, 4096, 64, fake, None) == 10001
    assert bwd(None, None, 10, None, None, None, None, None, 0, 4096, 64, None, None) == 0          # nothing wanted of nothing
    ws = lib.mmrec_linear_rows_workspace_bytes
    assert ws(4096, 4096, 64) >= lib.mmrec_linear_bwd_split_workspace_bytes(4096, 4096, 64) > 0
    assert ws(4096, 100, 64) == 0 and ws(4096, 4096, 128) == 0 and ws(0, 4096, 64) == 0


def test_linear_rows_on_cpu_tensors_is_the_composition(cpu_ops):  # noqa: F811
    """off the device `linear_rows` is `linear(table.index_select(0, ids), W, b)` through the module-level `linear` (here
    the CPU stand-in): values and all three gradients equal F.linear(table[ids], W, b)"""
    from mmrec_amd import hip_ops
    g = torch.Generator().manual_seed(5)
    table = torch.randn(50, 128, generator=g)
    W, b = torch.randn(64, 128, generator=g) / 11.0, torch.randn(64, generator=g)
    ids = torch.tensor([3, 49, 3, 0, 17, 17, 21], dtype=torch.int64)
    dY = torch.randn(ids.numel(), 64, generator=g)
    res = []
    for f in (lambda t, w, c: hip_ops.linear_rows(t, ids, w, c), lambda t, w, c: torch.nn.functional.linear(t[ids], w, c)):
        t, w, c = (x.clone().requires_grad_() for x in (table, W, b))
        y = f(t, w, c)
        y.backward(dY)
        res.append((y.detach(), t.grad, w.grad, c.grad))
    for a, r, what in zip(res[0], res[1], ("Y", "d table", "dW", "db")):
        torch.testing.assert_close(a, r, rtol=1e-5, atol=1e-5, msg=what)
    assert float(res[0][1][1].abs().max()) == 0.0           # a row no id names


def test_table_gradient_checker_catches_planted_errors():
    """CPU twin: the table-gradient rule passes an fp32 scatter of fp32 rows and rejects a row added at the wrong id, a dropped
    duplicate and a touched unlisted row"""
    X, W, _, dY, _ = draw_case(7)
    table, ids, _ = plant(7, X)
    n_table = table.shape[0]
    assert len(set(ids.tolist())) < ids.shape[0] and (np.diff(ids) < 0).any()       # repeats, not sorted
    dX = (dY.astype(np.float64) @ W.astype(np.float64)).astype(np.float32)

    def scatter(idx, rows):
        out = np.zeros((n_table, rows.shape[1]), dtype=np.float32)
        np.add.at(out, idx, rows)
        return out
    check_table_grad(scatter(ids, dX), ids, dY, W, name="clean")
    live = np.flatnonzero(np.abs(dX).max(axis=1) > 0)
    # a row added at the wrong (listed) id
    wrong = ids.copy()
    j = int(live[0])
    wrong[j] = ids[(j + 1) % ids.shape[0]] if ids[(j + 1) % ids.shape[0]] != ids[j] else ids[(j + 2) % ids.shape[0]]
    with pytest.raises(AssertionError):
        check_table_grad(scatter(wrong, dX), ids, dY, W)
    # a dropped duplicate: the second occurrence of a repeated id is left out
    seen, second = set(), None
    for k, i in enumerate(ids.tolist()):
        if i in seen and k in set(live.tolist()):
            second = k
            break
        seen.add(i)
    assert second is not None
    keep = np.arange(ids.shape[0]) != second
    with pytest.raises(AssertionError):
        check_table_grad(scatter(ids[keep], dX[keep]), ids, dY, W)
    # a row added at an id nobody listed
    listed = np.zeros(n_table, dtype=bool)
    listed[ids] = True
    stray = scatter(ids, dX)
    stray[int(np.flatnonzero(~listed)[0])] += dX[j]
    with pytest.raises(AssertionError):
        check_table_grad(stray, ids, dY, W)


# ------------------------------------------------------------------------------------------------------------------- GPU
def _run_rows(hip_ops, table, ids, W, b, dY, table_grad=True):
    dev = torch.device("cuda:0")
    Td = torch.from_numpy(table).to(dev).requires_grad_(table_grad)
    Wd = torch.from_numpy(W).to(dev).requires_grad_()
    bd = torch.from_numpy(b).to(dev).requires_grad_() if b is not None else None
    idd = torch.from_numpy(ids).to(dev)
    assert hip_ops.linear_rows_served(Td, idd, Wd)
    Y = hip_ops.linear_rows(Td, idd, Wd, bd)
    Y.backward(torch.from_numpy(dY).to(dev))
    torch.cuda.synchronize()
    return Y.detach(), Wd.grad, None if bd is None else bd.grad, Td.grad, (Td, idd, Wd, bd)


@pytest.mark.gpu
@pytest.mark.parametrize("split_everywhere", [True, False], ids=["split_min_f_0", "default_routing"])
@pytest.mark.parametrize("seed", SEEDS)
def test_linear_rows_fuzz(seed, split_everywhere, monkeypatch):
    from mmrec_amd import hip_ops
    if split_everywhere:        # the split-operand forward at every width, as tests/test_linear_fuzz_gpu.py runs it
        monkeypatch.setattr(hip_ops, "LINEAR_SPLIT_MIN_F", 0)
    X, W, b, dY, dom = draw_case(seed)
    table, ids, Xg = plant(seed, X)
    use_b = seed % 4 != 0
    Y, dW, db, dT, _ = _run_rows(hip_ops, table, ids, W, b if use_b else None, dY)
    n = Xg.shape[0]
    with np.errstate(invalid="ignore", over="ignore"):
        check(Y.cpu().numpy(), Xg, W.T.copy(), extra=np.broadcast_to(b, (n, 64)) if use_b else None, name="Y seed %d" % seed,
              dominant=dom)
        check(dW.cpu().numpy(), dY.T.copy(), Xg, name="dW seed %d" % seed, dominant=dom)
        if use_b:
            check(db.cpu().numpy()[None, :], np.ones((1, n), np.float32), dY, name="db seed %d" % seed, dominant=dom)
        check_table_grad(dT.cpu().numpy(), ids, dY, W, dominant=dom, name="d table seed %d" % seed)


def _bit_identity(hip_ops, table, ids, W, b, dY, table_grad=True):
    """Y, dW, db, the compact dX and the table's gradient of linear_rows == hip_ops.linear on table.index_select(0, ids)"""
    Y, dW, db, dT, (Td, idd, Wd, bd) = _run_rows(hip_ops, table, ids, W, b, dY, table_grad)
    Xc = Td.detach().index_select(0, idd).requires_grad_()
    W2 = Wd.detach().clone().requires_grad_()
    b2 = bd.detach().clone().requires_grad_() if bd is not None else None
    dYd = torch.from_numpy(dY).to(Td.device)
    Y2 = hip_ops.linear(Xc, W2, b2)
    Y2.backward(dYd)
    same_bits(Y, Y2, "Y")
    same_bits(dW, W2.grad, "dW")
    if bd is not None:
        same_bits(db, b2.grad, "db")
    _, _, dX = hip_ops._linear_rows_bwd(dYd, Td.detach(), idd, Wd.detach(), False, False, True)
    same_bits(dX, Xc.grad, "compact dX")
    if table_grad:      # what autograd builds for table[ids]
        same_bits(dT, torch.zeros_like(dT).index_put_((idd,), Xc.grad, accumulate=True), "d table")


@pytest.mark.gpu
@pytest.mark.parametrize("seed", SEEDS)
def test_linear_rows_bit_identical_to_linear_on_gathered_copy(seed, monkeypatch):
    from mmrec_amd import hip_ops
    X, W, b, dY, _ = draw_case(seed)
    table, ids, _ = plant(seed, X)
    for min_f in (0, hip_ops.LINEAR_SPLIT_MIN_F):           # both forward routings
        monkeypatch.setattr(hip_ops, "LINEAR_SPLIT_MIN_F", min_f)
        _bit_identity(hip_ops, table, ids, W, b if seed % 4 != 0 else None, dY)


@pytest.mark.gpu
def test_linear_rows_bit_identical_in_the_streaming_regime():
    """12,289 rows of 4096 columns: the rows that are read exceed 192 MB, where the forward streams non-temporally and rotates
    each row block's k walk"""
    from mmrec_amd import hip_ops
    rng = np.random.default_rng(12289)
    n, F, n_table = 12289, 4096, 14000
    table = np.full((n_table, F), np.nan, dtype=np.float32)
    pos = rng.choice(n_table, size=n, replace=False).astype(np.int64)
    table[pos] = rng.standard_normal((n, F)).astype(np.float32)
    ids = pos.copy()
    ids[rng.choice(n, size=700, replace=False)] = pos[rng.integers(0, n, size=700)]
    W = (rng.standard_normal((64, F)) / 64.0).astype(np.float32)
    b = rng.standard_normal(64).astype(np.float32)
    dY = (rng.standard_normal((n, 64)) * 1e-3).astype(np.float32)
    _bit_identity(hip_ops, table, ids, W, b, dY)


@pytest.mark.gpu
@pytest.mark.parametrize("F", [384, 1024, 4096])
def test_ids_outside_the_table_read_a_zero_row(F):
    """-1 ("no row") and n_table + 5 among valid ids: Y = b there; every other position's Y and all of dW are those of the same
    list with these positions pointing at an all-zero row of the table"""
    from mmrec_amd import hip_ops
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(F)
    n_table, n = 301, 333
    table = torch.randn(n_table, F, generator=g)
    table[n_table - 1] = 0.0                                 # the all-zero row
    ids = torch.randint(0, n_table - 1, (n,), generator=g)
    out = torch.tensor([0, 5, 127, 128, 200, n - 1])
    bad = ids.clone()
    bad[out] = torch.tensor([-1, n_table + 5, -1, n_table + 5, -1, n_table + 5])
    zero = ids.clone()
    zero[out] = n_table - 1
    W, b = (torch.randn(64, F, generator=g) / 30.0), torch.randn(64, generator=g)
    dY = torch.randn(n, 64, generator=g).to(dev)
    res = []
    for lst in (bad, zero):
        Wd, bd = W.to(dev).requires_grad_(), b.to(dev).requires_grad_()
        Y = hip_ops.linear_rows(table.to(dev), lst.to(dev), Wd, bd)
        Y.backward(dY)
        res.append((Y.detach(), Wd.grad, bd.grad))
    torch.cuda.synchronize()
    same_bits(res[0][0][out], b.to(dev).expand(out.numel(), 64), "Y at the positions without a row")
    same_bits(res[0][0], res[1][0], "Y")
    same_bits(res[0][1], res[1][1], "dW")
    same_bits(res[0][2], res[1][2], "db")


@pytest.mark.gpu
def test_table_above_4_gib():
    """270,000 x 4096 floats = 4.4 GB: a 32-bit row offset anywhere, forward or backward, reads the wrong row"""
    from mmrec_amd import hip_ops
    dev = torch.device("cuda:0")
    n_table, F, n = 270000, 4096, 640
    g = torch.Generator().manual_seed(270000)
    spread = torch.linspace(0, n_table - 1, n - 64).round().long()
    high = torch.randint(262144, n_table, (63,), generator=g)          # rows above the 4 GiB line
    ids = torch.cat([spread, high, torch.tensor([n_table - 1])])[torch.randperm(n, generator=g)].contiguous()
    assert int(ids.max()) == n_table - 1 and int((ids >= 262144).sum()) >= 64
    table = torch.zeros(n_table, F, dtype=torch.float32, device=dev)
    uniq = torch.unique(ids)
    rows = torch.randn(uniq.numel(), F, generator=g)
    rows[:, 0] = uniq.float()                                            # recognisable: a row carries its own id
    table[uniq.to(dev)] = rows.to(dev)
    W = (torch.randn(64, F, generator=g) / 64.0).to(dev)
    b = torch.randn(64, generator=g).to(dev)
    dY = (torch.randn(n, 64, generator=g) * 1e-2).to(dev)
    idd = ids.to(dev)
    W1, b1 = W.clone().requires_grad_(), b.clone().requires_grad_()
    Y = hip_ops.linear_rows(table, idd, W1, b1)
    Y.backward(dY)
    Xc = table.index_select(0, idd).requires_grad_()
    assert torch.equal(Xc.detach()[:, 0], idd.float())
    W2, b2 = W.clone().requires_grad_(), b.clone().requires_grad_()
    Y2 = hip_ops.linear(Xc, W2, b2)
    Y2.backward(dY)
    _, _, dX = hip_ops._linear_rows_bwd(dY, table, idd, W, False, False, True)
    torch.cuda.synchronize()
    same_bits(Y, Y2, "Y"), same_bits(W1.grad, W2.grad, "dW"), same_bits(b1.grad, b2.grad, "db")
    same_bits(dX, Xc.grad, "compact dX")


@pytest.mark.gpu
def test_forward_allocates_no_copy_of_the_rows():
    """the forward at (n, F) = (4096, 4096): Y and the workspace, a few MB -- far from the 64 MB a gathered copy takes"""
    from mmrec_amd import hip_ops
    dev = torch.device("cuda:0")
    n, F = 4096, 4096
    table = torch.randn(8192, F, device=dev)
    ids = torch.randint(0, 8192, (n,), device=dev)
    W, b = torch.randn(64, F, device=dev) / 64.0, torch.zeros(64, device=dev)
    hip_ops.linear_rows(table, ids, W, b)                               # (first call: whatever the runtime sets up once)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(dev)
    before = torch.cuda.memory_allocated(dev)
    Y = hip_ops.linear_rows(table, ids, W.requires_grad_(), b)
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated(dev) - before
    assert Y.shape == (n, 64)
    assert rise < n * F * 4 // 2, rise
