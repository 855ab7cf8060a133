"""Seeded differential fuzz of csrc/graph.hip -- `mmrec_coo_to_csr` with its workspace query, `mmrec_degree_count_i32`,
`mmrec_edge_norm_f32`, `mmrec_bipartite_expand` -- through the raw C ABI against numpy written here from the text of
include/mmrec_hip.h, and `hip_ops.bipartite_graph_from_edges` end to end against the host build `CsrGraph.from_coo_host`.

    degree count    counts[i] += #{e: ids[e] == i}, ids outside [0, n_bins) skipped      np.bincount on top of the start values
    COO -> CSR      order = STABLE argsort of the row keys; colidx = cols[order], vals_out = vals[order],
                    rowptr = [0, prefix sum of bincount(rows, n_rows)]                   np.argsort(kind="stable"), np.cumsum
    expand          rows = cat(eu, ei + n_users), cols = cat(ei + n_users, eu), vals = cat(w, w)
    edge norm       val[e] = fp32(1e-7 + du[eu[e]])^-1/2 * fp32(1e-7 + di[ei[e]])^-1/2   float64 of the fp32-rounded sums

Every integer output is compared EXACTLY.  The edge values of a COO -> CSR case are float32(position): distinct, so vals_out names
the permutation, and an order inside a row other than the COO order fails (the stability that makes a sharded run equal the
single-GPU run bit for bit).  Each conversion runs twice on the same input and must give the same bits.  The edge norm is held to
rtol 1e-6, the bound tests/test_hip_parity.py::test_graph_build_device_vs_golden already holds this kernel to: two powf of at most
2 ulp each and one product, (2 + 2 + 0.5) 2^-24 = 2.7e-7, leave a factor of three; the reference takes the SAME fp32 sum
1e-7 + deg (deg >= 2 absorbs the 1e-7, deg = 1 gives 1 + 2^-23, deg = 0 gives 3162.28 per endpoint), so no rounding of the argument
is charged to the kernel.

Every output (rowptr, colidx, vals_out, counts, rows, cols, vals, val) is pre-filled and carries GUARD sentinel elements on both
sides; the workspace has exactly `mmrec_coo_to_csr_workspace_bytes(nnz, n_rows)` bytes with guard bytes directly in front and
behind -- the query asks the sort for its needs without a bit range, the call sorts bits [0, end_bit) only: the guards show that
the first covers the second.  All guards are checked after each call.  The argument checks pass NULL or guard-only buffers, so a
launch would be visible.

`draw_case(seed)` is deterministic in the seed; `test_cases_span_every_axis` asserts every axis value to occur;
`test_checker_rejects_planted_errors` shows that the numpy restatement passes and each planted error (an unstable order inside a
row, rowptr not filled across an empty run, rowptr[n_rows] missing, a degree count that overwrites, one that folds an
out-of-range id to bin 0, an expand that offsets the user side) fails on at least one drawn case.

On one MI355X the 85 device tests take 2.8 s (the slowest 0.17 s, the first one with the library's load; a 2^20 + 3-entry
conversion, run twice with its numpy reference, 0.12 s); the 2 CPU tests 2 s.
"""
import ctypes

import numpy as np
import pytest
import torch

F32, F64, I64, I32 = np.float32, np.float64, np.int64, np.int32
GUARD = 64
GUARD_VALUE = 12345
FILL = -99
WS_GUARD = 4096                                             # bytes on either side of the workspace
BAD_ARG = 10001
INT32_MAX = 2 ** 31 - 1
RTOL_NORM = 1e-6

C_NNZ = (0, 1, 2, 255, 256, 257, 4095, 4096, 4097, 100_003, 2 ** 20 + 3)
C_ROWS = (1, 2, 3, 255, 256, 257, 1000, 2 ** 16, 2 ** 16 + 1, 2 ** 20 + 1)
C_PATTERNS = ("uniform", "row0", "last", "heavy", "even", "middle", "sorted", "reverse")
D_N = (0, 1, 255, 256, 257, 100_003)
D_BINS = (1, 2, 1000)
N_EDGES = (1, 255, 256, 257)
N_USERS = (0, 1, 1000)
NORM_EDGES = (1, 255, 256, 257, 5000)
NORM_DEGREES = (0, 1, 2, 4, 16, 4 ** 5, 4 ** 10, 10 ** 6)
N_CSR, N_DEG, N_NORM, N_EXP, N_E2E = 46, 18, 5, 12, 3
CSR_PLANTS = ("unstable", "rowptr_empty_run", "rowptr_last_missing")
DEG_PLANTS = ("overwrite", "fold_to_0")
EXP_PLANTS = ("offset_user_side",)


class Case:
    def axes(self):
        keys = ("seed", "kind", "nnz", "n_rows", "pattern", "n", "n_bins", "n_edges", "n_users", "n_items")
        return " ".join("%s=%s" % (k, getattr(self, k)) for k in keys if hasattr(self, k))


# ------------------------------------------------------------------------------------------------ cases
def _draw_csr(c, i, rng):
    c.kind = "csr"
    c.nnz = nnz = C_NNZ[i % 11]
    c.n_rows = nr = C_ROWS[(3 * i + i // 11) % 10]
    c.pattern = pat = C_PATTERNS[(i + 5 * (i // 11)) % 8]
    if i >= 44:                                             # the largest sort over the largest row counts
        c.nnz, c.n_rows, c.pattern = nnz, nr, pat = ((2 ** 20 + 3, 2 ** 20 + 1, "uniform"), (2 ** 20 + 3, 2 ** 16, "middle"))[i - 44]
    if pat == "row0":
        rows = np.zeros(nnz, I64)
    elif pat == "last":
        rows = np.full(nnz, nr - 1, I64)
    elif pat == "heavy":                                    # one row of nnz - 2 entries and two singles around it
        rows = np.full(nnz, nr // 2, I64)
        if nnz >= 3:
            at = rng.choice(nnz, 2, replace=False)
            rows[at[0]], rows[at[1]] = 0, nr - 1
    elif pat == "even":
        rows = 2 * rng.integers(0, (nr + 1) // 2, nnz)
    elif pat == "middle":                                   # a long run of empty rows in front and behind
        lo = nr // 3
        rows = rng.integers(lo, max(lo + 1, min(lo + 50, nr - nr // 3)), nnz)
    else:
        rows = rng.integers(0, nr, nnz)
        if pat == "sorted":
            rows = np.sort(rows)
        elif pat == "reverse":
            rows = np.sort(rows)[::-1]
    c.rows = np.ascontiguousarray(rows, I32)
    c.cols = rng.integers(0, 2 ** 31 - 1, nnz).astype(I32)
    c.vals = np.arange(nnz, dtype=F32)                      # distinct (nnz < 2^24): vals_out names the permutation
    assert nnz < 2 ** 24


def _draw_degree(c, i, rng):
    c.kind = "degree"
    c.n = n = D_N[i % 6]
    c.n_bins = nb = D_BINS[i // 6]
    ids = rng.integers(0, nb, n)
    if n >= 100_000:                                        # one hot bin takes 100,000 ids (the other three are skipped ones)
        ids[:] = nb - 1
    skipped = np.array([-1, nb, 2 ** 40, -2 ** 40], I64)
    if n >= 255:
        at = rng.choice(n, 40 if n < 100_000 else 3, replace=False)
        ids[at] = skipped[np.arange(at.size) % 4]
    elif n == 1 and i % 2 == 1:
        ids[0] = skipped[(i // 6) % 4]
    c.ids = ids.astype(I64)
    c.start = rng.integers(1, 1000, nb).astype(I32)         # the call ADDS: the counts do not start from zero


def _draw_norm(c, i, rng):
    c.kind = "norm"
    c.n_edges = ne = NORM_EDGES[i]
    c.n_users, c.n_items = 11, 13
    deg = np.array(NORM_DEGREES, I32)
    c.deg_u = deg[np.arange(11) % deg.size].astype(I32)
    c.deg_i = deg[(np.arange(13) * 3 + i) % deg.size].astype(I32)
    c.eu = rng.integers(0, 11, ne).astype(I64)
    c.ei = rng.integers(0, 13, ne).astype(I64)
    if ne >= 64:                                            # every pair of listed degrees at least once
        p = np.array([(a, b) for a in range(8) for b in range(8)])
        c.eu[:64] = p[:, 0]
        c.ei[:64] = np.array([int(np.flatnonzero(c.deg_i == deg[b])[0]) for b in p[:, 1]])


def _draw_expand(c, i, rng):
    c.kind = "expand"
    c.n_edges = ne = N_EDGES[i % 4]
    c.n_users = nu = N_USERS[i // 4]
    c.n_items = 77
    c.eu = rng.integers(0, max(nu, 1), ne).astype(I64)
    c.ei = rng.integers(0, c.n_items, ne).astype(I64)
    c.w = rng.random(ne).astype(F32) + F32(0.25)


def _draw_e2e(c, i, rng):
    c.kind = "e2e"
    c.n_users, c.n_items, c.n_edges = ((40, 30, 257), (300, 1000, 5000), (1000, 70, 4097))[i]
    users = rng.permutation(c.n_users)[:max(c.n_users * 2 // 3, 1)]      # a third of the users and items stay isolated,
    items = rng.permutation(c.n_items)[:max(c.n_items * 2 // 3, 1)]      # user 0 / the last item among them in case 0
    if i == 0:
        users, items = users[users != 0], items[items != c.n_items - 1]
    c.eu = users[(rng.zipf(1.5, c.n_edges) - 1) % users.size].astype(I64)
    c.ei = items[(rng.zipf(1.5, c.n_edges) - 1) % items.size].astype(I64)


_CASES = {}
_OFFSETS = np.cumsum([0, N_CSR, N_DEG, N_NORM, N_EXP, N_E2E])
_DRAW = (_draw_csr, _draw_degree, _draw_norm, _draw_expand, _draw_e2e)
CSR_SEEDS, DEG_SEEDS, NORM_SEEDS, EXP_SEEDS, E2E_SEEDS = (tuple(range(int(a), int(b))) for a, b in zip(_OFFSETS[:-1], _OFFSETS[1:]))
CASES = int(_OFFSETS[-1])


def draw_case(seed):
    if seed in _CASES:
        return _CASES[seed]
    rng = np.random.default_rng(9300 + seed)
    c = Case()
    c.seed = seed
    fam = int(np.searchsorted(_OFFSETS, seed, side="right")) - 1
    _DRAW[fam](c, seed - int(_OFFSETS[fam]), rng)
    _CASES[seed] = c
    return c


# ------------------------------------------------------------------------------------------------ the numpy restatement
def csr_ref(c, plant=None):
    """rowptr [n_rows + 1], colidx, vals_out; an entry a planted error leaves unwritten keeps FILL"""
    rows = c.rows.astype(I64)
    order = np.argsort(rows, kind="stable")
    counts = np.bincount(rows, minlength=c.n_rows)
    rowptr = np.zeros(c.n_rows + 1, I64)
    np.cumsum(counts, out=rowptr[1:])
    if plant == "unstable":                                 # the right rows, each row's segment back to front
        order = c.nnz - 1 - np.argsort(rows[::-1], kind="stable")
    if plant == "rowptr_empty_run" and c.nnz:               # only the rows that HAVE entries (and the end) get their start
        filled = np.full(c.n_rows + 1, FILL, I64)
        has = counts > 0
        filled[:-1][has] = rowptr[:-1][has]
        filled[-1] = rowptr[-1]
        rowptr = filled
    if plant == "rowptr_last_missing" and c.nnz:
        rowptr[-1] = FILL
    return rowptr.astype(I32), c.cols[order], c.vals[order]


def degree_ref(c, plant=None):
    ids = c.ids
    ok = (ids >= 0) & (ids < c.n_bins)
    if plant == "fold_to_0":
        ids, ok = np.where(ok, ids, 0), np.ones(ids.size, bool)
    add = np.bincount(ids[ok], minlength=c.n_bins)
    return (add if plant == "overwrite" and c.n else c.start.astype(I64) + add).astype(I32)


def expand_ref(c, plant=None):
    eu, ei, nu = c.eu, c.ei, c.n_users
    a, b = (eu + nu, ei) if plant == "offset_user_side" else (eu, ei + nu)
    return np.concatenate([a, b]).astype(I32), np.concatenate([b, a]).astype(I32), np.concatenate([c.w, c.w])


def norm_ref(deg_u, deg_i, eu, ei):
    """float64 of the fp32 sums 1e-7 + deg, to the power -1/2, both endpoints"""
    su = (F32(1e-7) + deg_u.astype(F32)).astype(F64)
    si = (F32(1e-7) + deg_i.astype(F32)).astype(F64)
    return su[eu] ** -0.5 * si[ei] ** -0.5


def same_exact(got, ref, name):
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.shape == ref.shape and got.dtype == ref.dtype, (name, got.shape, ref.shape, got.dtype, ref.dtype)
    bad = got.view(I32) != ref.view(I32) if got.dtype == F32 else got != ref
    assert not bad.any(), (name, "differs at %d of %d" % (int(bad.sum()), bad.size), "first at", int(np.argmax(bad)),
                           got[np.argmax(bad)], ref[np.argmax(bad)])


def check_csr(c, rowptr, colidx, vals_out):
    ref = csr_ref(c)
    same_exact(rowptr, ref[0], c.axes() + " rowptr")
    same_exact(colidx, ref[1], c.axes() + " colidx")
    same_exact(vals_out, ref[2], c.axes() + " vals_out (the permutation)")


def check_degree(c, counts):
    same_exact(counts, degree_ref(c), c.axes() + " counts")


def check_expand(c, rows, cols, vals):
    ref = expand_ref(c)
    for got, r, nm in zip((rows, cols, vals), ref, ("rows", "cols", "vals")):
        same_exact(got, r, c.axes() + " " + nm)


def check_norm(val, ref, name):
    val = np.asarray(val, F64)
    assert val.shape == ref.shape and np.isfinite(val).all(), (name, val.shape)
    err = np.abs(val - ref) / ref
    assert err.max(initial=0.0) <= RTOL_NORM, (name, "beyond rtol", float(err.max()), int(np.argmax(err)))
    return float(err.max(initial=0.0))


# ------------------------------------------------------------------------------------------------ CPU self-tests
def test_cases_span_every_axis():
    seen = {k: set() for k in ("nnz", "n_rows", "pattern", "big", "front", "back", "n", "n_bins", "dpair", "skipped", "hot", "n_edges",
                               "n_users", "epair", "norm_edges", "deg", "degpair")}
    for seed in range(CASES):
        c = draw_case(seed)
        assert c.axes() == draw_case(seed).axes()
        if c.kind == "csr":
            seen["nnz"].add(c.nnz), seen["n_rows"].add(c.n_rows), seen["pattern"].add(c.pattern)
            assert c.rows.size == c.nnz and (c.nnz == 0 or (0 <= c.rows.min() and c.rows.max() < c.n_rows))
            assert np.unique(c.vals).size == c.nnz
            if c.nnz >= 255 and c.n_rows >= 255:
                seen["big"].add(c.pattern)
                counts = np.bincount(c.rows, minlength=c.n_rows)
                occ = np.flatnonzero(counts)
                seen["front"].add(int(occ[0])), seen["back"].add(int(c.n_rows - 1 - occ[-1]))
                if c.pattern == "heavy":
                    assert sorted(counts[occ].tolist()) == [1, 1, c.nnz - 2]
                if c.pattern == "even":
                    assert not counts[1::2].any() and np.count_nonzero(counts) > 50
                if c.pattern == "sorted":
                    assert (np.diff(c.rows) >= 0).all()
                if c.pattern == "reverse":
                    assert (np.diff(c.rows) <= 0).all() and c.rows[0] > c.rows[-1]
                if c.pattern in ("row0", "last"):
                    assert (c.rows == (0 if c.pattern == "row0" else c.n_rows - 1)).all()
        elif c.kind == "degree":
            seen["n"].add(c.n), seen["n_bins"].add(c.n_bins), seen["dpair"].add((c.n, c.n_bins))
            assert (c.start > 0).all()
            seen["skipped"] |= set(int(x) if x != c.n_bins else "n_bins" for x in c.ids[(c.ids < 0) | (c.ids >= c.n_bins)])
            if c.n:
                seen["hot"].add(int(np.bincount(c.ids[(c.ids >= 0) & (c.ids < c.n_bins)], minlength=c.n_bins).max()) == 100_000)
        elif c.kind == "norm":
            seen["norm_edges"].add(c.n_edges)
            seen["deg"] |= set(c.deg_u.tolist()) | set(c.deg_i.tolist())
            seen["degpair"] |= set(zip(c.deg_u[c.eu].tolist(), c.deg_i[c.ei].tolist()))
        elif c.kind == "expand":
            seen["n_edges"].add(c.n_edges), seen["n_users"].add(c.n_users), seen["epair"].add((c.n_edges, c.n_users))
        else:
            du, di = np.bincount(c.eu, minlength=c.n_users), np.bincount(c.ei, minlength=c.n_items)
            assert (du == 0).sum() >= c.n_users // 4 and (di == 0).sum() >= c.n_items // 4 and du.max() > 10
            if c.seed == E2E_SEEDS[0]:
                assert du[0] == 0 and di[-1] == 0           # an empty first and an empty last row of the whole graph
    assert seen["nnz"] == set(C_NNZ) and seen["n_rows"] == set(C_ROWS) and seen["pattern"] == set(C_PATTERNS)
    assert seen["big"] == set(C_PATTERNS), seen["big"]      # every pattern at a size where it is what its name says
    assert max(seen["front"]) >= 4096 and max(seen["back"]) >= 4096      # one thread of the rowptr kernel fills thousands
    assert seen["n"] == set(D_N) and seen["n_bins"] == set(D_BINS) and len(seen["dpair"]) == 18
    assert seen["skipped"] >= {-1, "n_bins", 2 ** 40, -2 ** 40} and True in seen["hot"]
    assert seen["n_edges"] == set(N_EDGES) and seen["n_users"] == set(N_USERS) and len(seen["epair"]) == 12
    assert seen["norm_edges"] == set(NORM_EDGES) and seen["deg"] == set(NORM_DEGREES)
    assert seen["degpair"] >= {(a, b) for a in NORM_DEGREES for b in NORM_DEGREES}
    # the sort's forms: fewer entries than one block sorts, and more than a million
    assert any(draw_case(s).nnz == 2 ** 20 + 3 and draw_case(s).n_rows >= 2 ** 16 for s in CSR_SEEDS)


def test_checker_rejects_planted_errors():
    caught = {pl: [] for pl in CSR_PLANTS + DEG_PLANTS + EXP_PLANTS}
    for seed in range(CASES):
        c = draw_case(seed)
        fam = {"csr": (csr_ref, check_csr, CSR_PLANTS), "degree": (degree_ref, lambda c, x: check_degree(c, x), DEG_PLANTS),
               "expand": (expand_ref, check_expand, EXP_PLANTS)}.get(c.kind)
        if fam is None:
            continue
        ref, check, plants = fam
        out = ref(c)
        check(c, *(out if isinstance(out, tuple) else (out,)))              # the restatement passes its own checker
        for pl in plants if getattr(c, "nnz", 0) <= 100_003 else ():
            out = ref(c, pl)
            try:
                check(c, *(out if isinstance(out, tuple) else (out,)))
            except AssertionError:
                caught[pl].append(seed)
    print({pl: len(s) for pl, s in caught.items()})
    for pl, seeds in caught.items():
        assert seeds, (pl, "passes every case")
    # the edge norm's checker: 2e-6 off everywhere, in either direction, and 1.5e-6 off in one element all fail
    c = draw_case(NORM_SEEDS[2])
    ref = norm_ref(c.deg_u, c.deg_i, c.eu, c.ei)
    check_norm(ref.astype(F32), ref, "restated")
    for wrong in (ref * (1 + 2e-6), ref * (1 - 2e-6), np.where(np.arange(ref.size) == 77, ref * (1 + 1.5e-6), ref)):
        with pytest.raises(AssertionError):
            check_norm(wrong, ref, "planted")


# ------------------------------------------------------------------------------------------------ GPU plumbing
def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def P(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _lib():
    from mmrec_amd import _lib as L, hip_ops
    return L.load(), hip_ops._stream()


class Guarded:
    """an output of `n` elements (pre-filled with `init` or FILL) inside one tensor with GUARD sentinel elements on either side"""

    def __init__(self, n, dtype, init=None):
        self.n, self.dt = int(n), np.dtype(dtype)
        host = np.full(self.n + 2 * GUARD, GUARD_VALUE, self.dt)
        host[GUARD:GUARD + self.n] = FILL if init is None else init
        self.buf = _dev(host)
        self.view = self.buf[GUARD:GUARD + self.n]

    def get(self, name=""):
        b = self.buf.cpu().numpy()
        assert (b[:GUARD] == GUARD_VALUE).all() and (b[GUARD + self.n:] == GUARD_VALUE).all(), (name, "guard elements overwritten")
        return b[GUARD:GUARD + self.n].copy()

    def untouched(self, name=""):
        assert (self.get(name) == self.dt.type(FILL)).all(), (name, "written although nothing may be launched")


class Workspace:
    """exactly `nbytes` bytes with WS_GUARD guard bytes directly in front and behind (the offset keeps the 256-byte alignment)"""

    def __init__(self, nbytes):
        self.n = int(nbytes)
        self.buf = torch.full((self.n + 2 * WS_GUARD,), 0xA5, dtype=torch.uint8, device="cuda:0")
        assert (self.buf.data_ptr() + WS_GUARD) % 256 == 0
        self.ptr = ctypes.c_void_p(self.buf.data_ptr() + WS_GUARD)

    def check(self, name=""):
        b = self.buf.cpu().numpy()
        assert (b[:WS_GUARD] == 0xA5).all() and (b[WS_GUARD + self.n:] == 0xA5).all(), (name, "workspace guards overwritten", self.n)


def run_csr(c):
    lib, s = _lib()
    nbytes = lib.mmrec_coo_to_csr_workspace_bytes(c.nnz, c.n_rows)
    assert (nbytes == 0) == (c.nnz == 0) and nbytes >= 3 * 4 * c.nnz, (c.axes(), nbytes)
    ws = Workspace(nbytes)
    rowptr, colidx, vout = Guarded(c.n_rows + 1, I32), Guarded(c.nnz, I32), Guarded(c.nnz, F32)
    rows, cols, vals = (_dev(x) if c.nnz else None for x in (c.rows, c.cols, c.vals))
    rc = lib.mmrec_coo_to_csr(P(rows), P(cols), P(vals), c.nnz, c.n_rows, P(rowptr.view), P(colidx.view), P(vout.view), ws.ptr, s)
    assert rc == 0, (c.axes(), rc)
    torch.cuda.synchronize()
    ws.check(c.axes())
    if c.nnz:                                               # the inputs are inputs
        assert np.array_equal(rows.cpu().numpy(), c.rows) and np.array_equal(cols.cpu().numpy(), c.cols)
    return rowptr.get(c.axes()), colidx.get(c.axes()), vout.get(c.axes())


# ------------------------------------------------------------------------------------------------ device tests
@pytest.mark.gpu
@pytest.mark.parametrize("seed", CSR_SEEDS)
def test_coo_to_csr_exact_and_stable(seed):
    c = draw_case(seed)
    first = run_csr(c)
    check_csr(c, *first)
    if c.nnz == 0:
        assert not first[0].any()                           # rowptr all zero; colidx / vals_out have no element, their guards held
    for a, b, nm in zip(first, run_csr(c), ("rowptr", "colidx", "vals_out")):
        same_exact(a, b, c.axes() + " second call " + nm)


@pytest.mark.gpu
@pytest.mark.parametrize("seed", DEG_SEEDS)
def test_degree_count_adds_and_skips(seed):
    lib, s = _lib()
    c = draw_case(seed)
    counts = Guarded(c.n_bins, I32, init=c.start)
    ids = _dev(c.ids) if c.n else None
    assert lib.mmrec_degree_count_i32(P(ids), c.n, P(counts.view), c.n_bins, s) == 0
    torch.cuda.synchronize()
    check_degree(c, counts.get(c.axes()))


@pytest.mark.gpu
@pytest.mark.parametrize("seed", NORM_SEEDS)
def test_edge_norm_against_float64(seed):
    lib, s = _lib()
    c = draw_case(seed)
    val = Guarded(c.n_edges, F32)
    a = [_dev(x) for x in (c.eu, c.ei, c.deg_u, c.deg_i)]
    assert lib.mmrec_edge_norm_f32(P(a[0]), P(a[1]), c.n_edges, P(a[2]), P(a[3]), P(val.view), s) == 0
    torch.cuda.synchronize()
    worst = check_norm(val.get(c.axes()), norm_ref(c.deg_u, c.deg_i, c.eu, c.ei), c.axes())
    print("%s worst relative error %.3g" % (c.axes(), worst))


@pytest.mark.gpu
@pytest.mark.parametrize("seed", EXP_SEEDS)
def test_bipartite_expand_layout(seed):
    lib, s = _lib()
    c = draw_case(seed)
    rows, cols, vals = Guarded(2 * c.n_edges, I32), Guarded(2 * c.n_edges, I32), Guarded(2 * c.n_edges, F32)
    a = [_dev(x) for x in (c.eu, c.ei, c.w)]
    assert lib.mmrec_bipartite_expand(P(a[0]), P(a[1]), P(a[2]), c.n_edges, c.n_users, P(rows.view), P(cols.view), P(vals.view), s) == 0
    torch.cuda.synchronize()
    check_expand(c, rows.get(c.axes()), cols.get(c.axes()), vals.get(c.axes()))


@pytest.mark.gpu
@pytest.mark.parametrize("seed", E2E_SEEDS)
def test_bipartite_graph_from_edges_equals_host_build(seed):
    from mmrec_amd import hip_ops
    c = draw_case(seed)
    nu, n = c.n_users, c.n_users + c.n_items
    g = hip_ops.bipartite_graph_from_edges(_dev(c.eu), _dev(c.ei), c.n_users, c.n_items)
    w = norm_ref(np.bincount(c.eu, minlength=c.n_users).astype(I32), np.bincount(c.ei, minlength=c.n_items).astype(I32), c.eu, c.ei)
    idx = np.stack([np.concatenate([c.eu, c.ei + nu]), np.concatenate([c.ei + nu, c.eu])])
    w2 = np.concatenate([w, w])
    host = hip_ops.CsrGraph.from_coo_host(idx, w2.astype(F32), n, n, "cuda:0", symmetric=True)
    torch.cuda.synchronize()
    same_exact(g.rowptr.cpu().numpy(), host.rowptr.cpu().numpy(), c.axes() + " rowptr")
    same_exact(g.colidx.cpu().numpy(), host.colidx.cpu().numpy(), c.axes() + " colidx")
    assert g.n_rows == n and g.n_cols == n and int(g.rowptr[-1]) == 2 * c.n_edges
    check_norm(g.vals.cpu().numpy(), w2[np.argsort(idx[0], kind="stable")], c.axes() + " values")


@pytest.mark.gpu
def test_argument_checks_return_before_any_launch():
    """every early return of the four entry points as written in graph.hip, on NULL or guard-only buffers"""
    lib, s = _lib()
    i32, f32 = Guarded(16, I32), Guarded(16, F32)
    ids = _dev(np.zeros(8, I64))
    deg = _dev(np.ones(8, I32))
    w = _dev(np.ones(8, F32))
    o, f, big = P(i32.view), P(f32.view), 2 ** 31
    # degree count
    assert lib.mmrec_degree_count_i32(P(ids), -1, o, 4, s) == BAD_ARG and lib.mmrec_degree_count_i32(P(ids), 4, o, -1, s) == BAD_ARG
    assert lib.mmrec_degree_count_i32(None, 0, None, 4, s) == 0
    assert lib.mmrec_degree_count_i32(None, 4, o, 4, s) == BAD_ARG and lib.mmrec_degree_count_i32(P(ids), 4, None, 4, s) == BAD_ARG
    # edge norm
    args = [P(ids), P(ids), 4, P(deg), P(deg), f, s]
    assert lib.mmrec_edge_norm_f32(P(ids), P(ids), -1, P(deg), P(deg), f, s) == BAD_ARG
    assert lib.mmrec_edge_norm_f32(None, None, 0, None, None, None, s) == 0
    for k in (0, 1, 3, 4, 5):
        assert lib.mmrec_edge_norm_f32(*[None if j == k else x for j, x in enumerate(args)]) == BAD_ARG, k
    # expand
    args = [P(ids), P(ids), P(w), 4, 3, o, o, f, s]
    assert lib.mmrec_bipartite_expand(P(ids), P(ids), P(w), -1, 3, o, o, f, s) == BAD_ARG
    assert lib.mmrec_bipartite_expand(P(ids), P(ids), P(w), 4, -1, o, o, f, s) == BAD_ARG
    assert lib.mmrec_bipartite_expand(None, None, None, 0, 3, None, None, None, s) == 0
    for k in (0, 1, 2, 5, 6, 7):
        assert lib.mmrec_bipartite_expand(*[None if j == k else x for j, x in enumerate(args)]) == BAD_ARG, k
    # the workspace query
    for nnz, n_rows in ((0, 5), (-1, 5), (5, 0), (5, -1), (big, 5)):
        assert lib.mmrec_coo_to_csr_workspace_bytes(nnz, n_rows) == 0, (nnz, n_rows)
    assert lib.mmrec_coo_to_csr_workspace_bytes(INT32_MAX, 5) >= 3 * 4 * INT32_MAX
    # COO -> CSR
    r32 = _dev(np.zeros(8, I32))
    ws = Workspace(lib.mmrec_coo_to_csr_workspace_bytes(4, 5))
    args = [P(r32), P(r32), P(w), 4, 5, o, o, f, ws.ptr, s]
    for nnz, n_rows in ((-1, 5), (4, -1), (big, 5)):
        assert lib.mmrec_coo_to_csr(P(r32), P(r32), P(w), nnz, n_rows, o, o, f, ws.ptr, s) == BAD_ARG, (nnz, n_rows)
    assert lib.mmrec_coo_to_csr(None, None, None, 0, 5, None, None, None, None, s) == BAD_ARG         # rowptr is needed even then
    for k in (0, 1, 2, 5, 6, 7, 8):
        assert lib.mmrec_coo_to_csr(*[None if j == k else x for j, x in enumerate(args)]) == BAD_ARG, k
    torch.cuda.synchronize()
    i32.untouched("argument checks"), f32.untouched("argument checks"), ws.check("argument checks")
    # ... and nnz == 0 with nothing but rowptr: n_rows + 1 zeros, no other pointer read
    rowptr = Guarded(6, I32)
    assert lib.mmrec_coo_to_csr(None, None, None, 0, 5, P(rowptr.view), None, None, None, s) == 0
    torch.cuda.synchronize()
    assert not rowptr.get("nnz == 0").any()
