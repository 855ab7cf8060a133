"""CPU: edge dropout inside the SpMM (mmrec_edge_keep_bits, mmrec_spmm_csr_masked_f32, hip_ops.spmm_edge_dropout,
hip_ops.lightgcn_mean_edge_dropout) -- everything that needs no device.

  * the host checks of the ops and the argument checks of the two C entry points answer before any launch;
  * the composition of the older kernels is what runs for an unserved width and with the `EDGE_DROPOUT` switch off, and it
    computes the formula;
  * the cases of tests/test_edge_dropout_fuzz_gpu.py (drawn here) cover every axis the kernels branch on;
  * THE CHECKER PROVES ITSELF: an fp32 emulation of the kernels' plan in numpy (16-entry spans, 512-entry chunks, the 16-group
    tree, the chunk-order sum, the mask read by POSITION from the packed words) passes the check the GPU fuzz applies -- the
    float64 product of the kept entries with values vals * float32(val_scale), in the two acceptance modes of
    tests/test_spmm_fuzz_gpu.py, the float bound with one more rounding for vals * val_scale -- and every planted mask error is
    rejected;
  * the keep rule of `LightGCN_Encoder.draw_dropout` is floor(float32(1 - rate) + u) != 0."""
import ctypes

import numpy as np
import pytest
import torch

from tests.test_spmm_fuzz_gpu import CHUNK, EXACT_COEF, FLOAT_COEF, U, _grid, check, csr, plan_depth

CASES = 50
WIDTHS = (64, 64, 128, 64, 384)                               # seed % 5
THRESHOLDS = (0, 16, 32, 511, 512, 513, None)                 # seed % 7
PATTERNS = ("all", "none", "one_per_row", "chunk_clear", "long_row_clear", "b0.1", "b0.5", "b0.9", "last_only")   # seed % 9
EPILOGUES = ("Y", "acc", "Yacc", "YZ")                        # (seed // 3) % 4: what the mean op's forward and backward use
SPECIAL_DEGREES = (0, 1, 15, 16, 17, 31, 32, 33, 512, 513, 1024, 1025, 8200)    # + threshold - 1, threshold, threshold + 1
BIG_ROWS = (1 << 18) + 37                                     # four rows per 16-lane group
BIG_SEED, NNZ0_SEED = 48, 49
EXACT_SCALES = (1.0, 2.0, 0.5, 4.0)
FLOAT_RATES = (0.1, 0.5, 0.9)                                 # val_scale = 1 / (1 - rate), as the encoder passes it


# ------------------------------------------------------------------------------------------------ mask helpers (host)
def pack_bits(keep):
    """keep [E] (CSR order) -> uint32 words, entry k = bit (k & 31) of word k >> 5, trailing bits zero"""
    keep = np.asarray(keep, bool)
    n_words = (keep.size + 31) // 32
    padded = np.zeros(n_words * 32, np.uint64)
    padded[:keep.size] = keep
    return (padded.reshape(n_words, 32) << np.arange(32, dtype=np.uint64)).sum(1).astype(np.uint32)


def unpack_bits(words, pos):
    """the keep flags at entry positions `pos`, read from the packed words as the kernel reads them"""
    pos = np.asarray(pos, np.int64)
    return ((words[pos >> 5] >> (pos & 31).astype(np.uint32)) & 1).astype(bool)


def masked_csr(rowptr, cols, vals, keep, scale, shape):
    """the float64 matrix the masked launch stands for: kept entries only, values vals * float32(scale) (unrounded)"""
    keep = np.asarray(keep, bool)
    rows = np.repeat(np.arange(shape[0]), np.diff(rowptr))
    rp = np.zeros(shape[0] + 1, np.int64)
    np.cumsum(np.bincount(rows[keep], minlength=shape[0]), out=rp[1:])
    return csr(rp, np.asarray(cols)[keep], np.asarray(vals, np.float64)[keep] * float(np.float32(scale)), shape)


def masked_depth(deg, thr):
    """roundings a term meets: the FULL graph's plan (the chunk boundaries do not move with the mask) + 1 for vals * val_scale"""
    return plan_depth(deg, thr) + 1


def transpose_order(cols):
    """perm_t of a graph whose edge order is its CSR order: the stable sort by column"""
    return np.argsort(np.asarray(cols), kind="stable")


# ------------------------------------------------------------------------------------------------ cases
class Case:
    pass


def _keep_pattern(rng, c):
    nnz, rp, deg = int(c.rowptr[-1]), c.rowptr, c.deg
    p = c.pattern
    if p == "all":
        return np.ones(nnz, bool)
    if p == "none":
        return np.zeros(nnz, bool)
    keep = np.zeros(nnz, bool)
    if p == "one_per_row":
        rows = np.flatnonzero(deg > 0)
        keep[rp[rows] + (rng.random(rows.size) * deg[rows]).astype(np.int64)] = True
        return keep
    if p == "last_only":
        if nnz:
            keep[-1] = True
        return keep
    if p.startswith("b"):
        return rng.random(nnz) < float(p[1:])
    keep = rng.random(nnz) < 0.5
    for r in np.flatnonzero(deg > max(c.thr_eff, CHUNK)):             # rows of several chunks
        if p == "chunk_clear":
            k = int(rng.integers(0, -(-deg[r] // CHUNK)))
            keep[rp[r] + k * CHUNK:min(rp[r] + (k + 1) * CHUNK, rp[r + 1])] = False
        elif r % 2 == 0 or deg[r] == 8200:                            # long_row_clear
            keep[rp[r]:rp[r + 1]] = False
    return keep


def draw_case(seed):
    from mmrec_amd.hip_ops import default_long_row_threshold
    rng = np.random.default_rng(9100 + seed)
    c = Case()
    c.seed, c.big, c.nnz0 = seed, seed == BIG_SEED, seed == NNZ0_SEED
    c.d = 64 if c.big else WIDTHS[seed % len(WIDTHS)]
    c.thr = None if c.big else THRESHOLDS[seed % len(THRESHOLDS)]
    c.exact = c.big or (seed // 9 + seed) % 3 != 2             # (seed % 3 alone would tie the mode to the pattern)
    c.epi = "Y" if c.big else EPILOGUES[(seed // 3) % len(EPILOGUES)]
    c.pattern = "b0.5" if c.big else PATTERNS[seed % len(PATTERNS)]
    if c.big:
        c.n_rows, c.n_cols = BIG_ROWS, 3000
    else:
        c.n_rows, c.n_cols = int(rng.integers(60, 200)), int(rng.integers(50, 300))
    n_rows, n_cols, d = c.n_rows, c.n_cols, c.d
    c.thr_eff = default_long_row_threshold(n_cols) if c.thr is None else c.thr
    if c.big:
        deg = rng.integers(0, 4, n_rows)
    elif c.nnz0:
        deg = np.zeros(n_rows, np.int64)
    else:
        deg = rng.geometric(0.15, n_rows) - 1
        deg[rng.random(n_rows) < 0.2] = 0
        special = [k for k in SPECIAL_DEGREES + (c.thr_eff - 1, c.thr_eff, c.thr_eff + 1) if k >= 0]
        rng.shuffle(special)
        order = np.concatenate([[0, n_rows - 1], 1 + rng.permutation(n_rows - 2)])
        for r, k in zip(order, special):
            deg[r] = k
    c.deg = deg.astype(np.int64)
    c.rowptr = np.zeros(n_rows + 1, np.int64)
    np.cumsum(c.deg, out=c.rowptr[1:])
    nnz = int(c.rowptr[-1])
    c.rows = np.repeat(np.arange(n_rows), c.deg)
    c.cols = rng.integers(0, n_cols, nnz)
    c.keep = _keep_pattern(rng, c)
    c.alpha, c.beta, c.acc_scale = (float(rng.choice(EXACT_COEF if c.exact else FLOAT_COEF)) for _ in range(3))
    want_z, want_acc = c.epi == "YZ", c.epi in ("acc", "Yacc")
    if c.exact:
        # vals k / 8, X k / 16 with |x| <= 1 / 4, val_scale a power of two >= 1 / 2: every partial sum is a multiple of 2^-8,
        # 2^-10 after alpha, and the checker asserts all magnitudes below 2^14 -- exact fp32 numbers in any order
        c.scale = float(EXACT_SCALES[seed % len(EXACT_SCALES)])
        c.vals = (rng.integers(-8, 9, nnz) / 8.0).astype(np.float32)
        c.X = _grid(rng, (n_cols, d), k=4)
        c.Z = _grid(rng, (n_rows, d)) if want_z else None
        c.acc_in = _grid(rng, (n_rows, d)) if want_acc else None
    else:
        c.scale = 1.0 / (1.0 - FLOAT_RATES[seed % len(FLOAT_RATES)])
        vals = rng.standard_normal(nnz) * np.repeat(10.0 ** rng.uniform(-2, 2, n_rows), c.deg)
        vals[rng.random(nnz) < 0.05] = 0.0
        c.vals = vals.astype(np.float32)
        X = rng.standard_normal((n_cols, d))
        X[rng.random(X.shape) < 0.2] = 0.0
        c.X = X.astype(np.float32)
        c.Z = rng.standard_normal((n_rows, d)).astype(np.float32) if want_z else None
        c.acc_in = rng.standard_normal((n_rows, d)).astype(np.float32) if want_acc else None
        assert not ((c.deg <= c.thr_eff) & (c.deg > 1024)).any()      # float mode: sequential chains <= 1024 entries
    return c


def check_case(c, Y=None, acc=None, keep=None, name=""):
    """the GPU fuzz's acceptance of a raw masked launch on the case: Y and / or acc_out against float64"""
    keep = c.keep if keep is None else keep
    terms = [(c.alpha, masked_csr(c.rowptr, c.cols, c.vals, keep, c.scale, (c.n_rows, c.n_cols)), c.X)]
    depth = masked_depth(c.deg, c.thr_eff)
    worst = 0.0
    if Y is not None:
        worst = check(Y, terms, Z=c.Z, beta=c.beta, exact=c.exact, depth=depth, name="Y %s seed %d" % (name, c.seed))
    if acc is not None:
        worst = max(worst, check(acc, terms, Z=c.Z, beta=c.beta, acc_in=c.acc_in, acc_scale=c.acc_scale, exact=c.exact,
                                 depth=depth, name="acc %s seed %d" % (name, c.seed)))
    return worst


# ------------------------------------------------------------------------------------------------ fp32 emulation of the plan
def _fma(a, x, acc):
    return (np.float64(a) * x.astype(np.float64) + acc.astype(np.float64)).astype(np.float32)


def emulate(rowptr, cols, vals, kept, scale, X, thr, alpha=1.0, Z=None, beta=1.0):
    """y = alpha * (masked A) X + beta * Z in fp32 under the kernels' plan; `kept` [nnz]: the flags the kernel would have read"""
    f32 = np.float32
    vs = np.asarray(vals, f32) if scale is None else np.asarray(vals, f32) * f32(scale)
    n, d = len(rowptr) - 1, X.shape[1]
    zero = np.zeros(d, f32)
    out = np.zeros((n, d), f32)

    def span(acc, s, e):
        for k in range(s, e):
            if kept[k]:
                acc = _fma(vs[k], X[cols[k]], acc)
        return acc
    for r in range(n):
        s, e = int(rowptr[r]), int(rowptr[r + 1])
        if e - s <= thr:
            tot = span(zero, s, e)
        else:
            parts = []
            for cs in range(s, e, CHUNK):
                ce = min(cs + CHUNK, e)
                red = []
                for g in range(16):                                   # group g: spans g, g + 16, ... of the chunk
                    a = zero
                    for base in range(cs + g * 16, ce, 256):
                        a = span(a, base, min(base + 16, ce))
                    red.append(a)
                t = red[0]
                for i in range(1, 16):
                    t = t + red[i]
                parts.append(t)
            if len(parts) == 1:
                tot = parts[0]
            else:                                                     # group g sums chunks g, g + 16, ...; then the 16 groups
                red = []
                for g in range(16):
                    t = zero
                    for ch in range(g, len(parts), 16):
                        t = t + parts[ch]
                    red.append(t)
                tot = red[0]
                for i in range(1, 16):
                    tot = tot + red[i]
        y = f32(alpha) * tot
        out[r] = y if Z is None else _fma(f32(beta), Z[r], y)
    return out


def _emulate_case(c, kept, scale="case"):
    y = emulate(c.rowptr, c.cols, c.vals, kept, c.scale if scale == "case" else scale, c.X, c.thr_eff, c.alpha, c.Z, c.beta)
    if c.acc_in is None:
        return dict(Y=y)
    return dict(Y=y if c.epi == "Yacc" else None, acc=np.float32(c.acc_scale) * (c.acc_in + y))


def _planted(c):
    """name -> the flags a kernel with that mask error would read (positions into the packed words of c.keep)"""
    nnz, words = int(c.rowptr[-1]), pack_bits(c.keep)
    pos = np.arange(nnz)
    prev_row_start = np.concatenate([[0], c.rowptr[:-2]])             # row r reads at the previous row's positions
    shift = np.minimum(pos + 1, nnz - 1)
    last_word = unpack_bits(words, pos) | ((pos >> 5) == (nnz - 1) >> 5)
    rev = (pos & ~31) + 31 - (pos & 31)
    rev_ok = rev < words.size * 32
    return {
        "mask ignored": np.ones(nnz, bool),
        "mask shifted by one entry": unpack_bits(words, shift),
        "bit order reversed within a word": unpack_bits(words, np.where(rev_ok, rev, pos)),
        "clear bit of the last word treated as set": last_word,
        "previous row's bit positions": unpack_bits(words, np.repeat(prev_row_start, c.deg) + pos - c.rowptr[c.rows]),
    }


def _proof_case(exact):
    for s in range(CASES):
        c = draw_case(s)
        # a Bernoulli mask, a Z or acc term, rows of several chunks, the last word partly filled with a dropped entry in it
        if (c.exact == exact and c.pattern in ("b0.5", "b0.1") and not c.big and int(c.rowptr[-1]) % 32 and
                not c.keep[-(int(c.rowptr[-1]) % 32):].all()):
            return c
    raise AssertionError("no such case")


@pytest.mark.parametrize("exact", [True, False])
def test_emulated_plan_passes_and_planted_errors_are_rejected(exact):
    c = _proof_case(exact)
    nnz = int(c.rowptr[-1])
    words = pack_bits(c.keep)
    assert words.size == (nnz + 31) // 32 and int(words[-1]) >> (nnz % 32) == 0       # trailing bits zero
    good = unpack_bits(words, np.arange(nnz))
    assert np.array_equal(good, c.keep)
    worst = check_case(c, **_emulate_case(c, good), name="emulated")
    print("emulated plan, %s: worst err/M %.3e (u = %.3e)" % ("exact" if exact else "float", worst, U))
    assert (c.deg > c.thr_eff).any() and (c.rowptr[:-1][c.deg > 32] % 32 != 0).any()
    for name, kept in _planted(c).items():
        assert not np.array_equal(kept, good), name
        with pytest.raises(AssertionError):
            check_case(c, **_emulate_case(c, kept), name=name)
    with pytest.raises(AssertionError):                               # val_scale omitted
        assert c.scale != 1.0
        check_case(c, **_emulate_case(c, good, scale=None), name="val_scale omitted")


@pytest.mark.parametrize("exact", [True, False])
def test_forward_mask_on_the_transposed_side_is_rejected(exact):
    """the backward's launch runs on the transposed CSR: its bits are keep[perm_t]; the forward's words there are an error"""
    c = _proof_case(exact)
    rng = np.random.default_rng(c.seed)
    perm_t = transpose_order(c.cols)
    rp_t = np.zeros(c.n_cols + 1, np.int64)
    np.cumsum(np.bincount(c.cols, minlength=c.n_cols), out=rp_t[1:])
    t = Case()
    t.seed, t.exact, t.epi, t.n_rows, t.n_cols, t.thr_eff, t.scale = c.seed, exact, "Y", c.n_cols, c.n_rows, c.thr_eff, c.scale
    t.rowptr, t.deg, t.rows, t.cols, t.vals = rp_t, np.diff(rp_t), c.cols[perm_t], c.rows[perm_t], c.vals[perm_t]
    t.keep, t.alpha, t.beta, t.acc_scale, t.Z, t.acc_in = c.keep[perm_t], 1.0, 1.0, 1.0, None, None
    t.X = _grid(rng, (c.n_rows, 64), k=4) if exact else rng.standard_normal((c.n_rows, 64)).astype(np.float32)
    nnz = int(rp_t[-1])
    right = unpack_bits(pack_bits(c.keep[perm_t]), np.arange(nnz))
    wrong = unpack_bits(pack_bits(c.keep), np.arange(nnz))            # the forward's words, read at the transposed positions
    check_case(t, **_emulate_case(t, right), name="transposed")
    assert not np.array_equal(right, wrong)
    with pytest.raises(AssertionError):
        check_case(t, **_emulate_case(t, wrong), name="forward mask on the transposed side")


def test_cases_span_every_axis():
    seen = {k: set() for k in ("d", "thr", "pattern", "epi", "mode", "deg")}
    odd_start = odd_nnz = multi = 0
    for s in range(CASES):
        c = draw_case(s)
        nnz, t = int(c.rowptr[-1]), c.thr_eff
        assert c.keep.shape == (nnz,) and c.big == (c.n_rows > (1 << 18))
        if c.big:
            assert c.d == 64 and c.deg.max() == 3 and c.deg.min() == 0 and c.n_rows == BIG_ROWS
            continue
        if c.nnz0:
            assert nnz == 0
            continue
        seen["d"].add(c.d), seen["thr"].add(c.thr), seen["pattern"].add(c.pattern), seen["epi"].add(c.epi)
        seen["mode"].add((c.pattern, c.exact)), seen["mode"].add((c.d, c.exact))
        for k, nm in [(k, k) for k in SPECIAL_DEGREES] + [(t - 1, "t-1"), (t, "t"), (t + 1, "t+1")]:
            if k >= 0 and (c.deg == k).any():
                seen["deg"].add(nm)
        long_starts = c.rowptr[:-1][c.deg > t]
        odd_start += bool((long_starts % 32 != 0).any() and (long_starts % 16 != 0).any() and
                          (c.rowptr[:-1][(c.deg > 16) & (c.deg <= t)] % 16 != 0).any())
        odd_nnz += bool(nnz % 32 and nnz % 64)
        multi += bool((c.deg == 8200).any() and 8200 > t)            # 17 chunks: the 16-way chunk sum wraps
        if c.pattern == "chunk_clear":
            r = int(np.flatnonzero(c.deg == 8200)[0])
            kc = c.keep[c.rowptr[r]:c.rowptr[r + 1]]
            assert any(not kc[i:i + CHUNK].any() for i in range(0, 8200, CHUNK)) and kc.any()
        if c.pattern == "long_row_clear":
            r = int(np.flatnonzero(c.deg == 8200)[0])
            assert not c.keep[c.rowptr[r]:c.rowptr[r + 1]].any() and c.keep.any()
        if c.pattern == "last_only":
            assert c.keep[-1] and c.keep.sum() == 1
        if c.pattern == "one_per_row":
            assert np.array_equal(np.bincount(c.rows[c.keep], minlength=c.n_rows), (c.deg > 0).astype(np.int64))
    assert seen["d"] == {64, 128, 384} and seen["thr"] == set(THRESHOLDS) and seen["pattern"] == set(PATTERNS)
    assert seen["epi"] == set(EPILOGUES)
    assert seen["mode"] >= {(p, e) for p in PATTERNS for e in (True, False)} | {(64, True), (64, False), (128, True), (384, True)}
    assert seen["deg"] == set(SPECIAL_DEGREES) | {"t-1", "t", "t+1"}
    assert odd_start >= 10 and odd_nnz >= 10 and multi >= 40
    assert {draw_case(s).scale for s in range(CASES) if draw_case(s).exact} == set(EXACT_SCALES)


# ------------------------------------------------------------------------------------------------ the keep rule
def test_keep_rule_is_floor_of_float32_sum():
    """draw_dropout keeps entry e iff torch.floor(1 - rate + u_e) != 0 with u fp32: the Python double 1 - rate enters the sum as
    float32(1 - rate), the sum is one fp32 addition.  Checked at the neighbours of the boundary u = rate too."""
    rng = np.random.default_rng(0)
    for rate in [0.0, 0.1, 0.5, 0.9, 1.0 - 2.0 ** -24, 0.3333333333, float(rng.random()), float(rng.random())]:
        edge = np.float32(1.0) - np.float32(1 - rate)                  # about `rate`
        u = np.concatenate([rng.random(4096).astype(np.float32), [np.float32(0), np.nextafter(np.float32(1), np.float32(0))]])
        near = edge
        for _ in range(4):
            near = np.nextafter(near, np.float32(0))
        for _ in range(9):
            if 0 <= near < 1:
                u = np.append(u, near)
            near = np.nextafter(near, np.float32(1))
        u = u.astype(np.float32)
        want = torch.floor(1 - rate + torch.from_numpy(u)).to(torch.bool).numpy()
        got = np.floor(np.float32(1 - rate) + u) != 0
        assert (np.float32(1 - rate) + u).dtype == np.float32
        assert np.array_equal(got, want), rate
        if 0 < rate < 0.95:
            assert got.any() and not got.all()


# ------------------------------------------------------------------------------------------------ host checks, no device
def _stub_graph(rows, cols, n_rows, n_cols, vals):
    """an EdgeDropoutGraph over host tensors, built past the constructor's device check (nothing here launches)"""
    from mmrec_amd import hip_ops
    dyn = hip_ops.DynGraph.__new__(hip_ops.DynGraph)
    dyn.rows, dyn.cols, dyn.n_rows, dyn.n_cols = rows, cols, n_rows, n_cols
    dyn.perm, dyn.perm_t = torch.sort(rows, stable=True)[1], torch.sort(cols, stable=True)[1]
    eg = hip_ops.EdgeDropoutGraph.__new__(hip_ops.EdgeDropoutGraph)
    eg.dyn, eg.vals, eg.n_edges = dyn, vals, int(vals.numel())
    return eg


def _small():
    g = torch.Generator().manual_seed(3)
    n, E = 12, 40
    rows, cols = torch.randint(0, n, (E,), generator=g), torch.randint(0, n, (E,), generator=g)
    vals = torch.randn(E, generator=g)
    keep = torch.rand(E, generator=g) < 0.6
    return n, rows, cols, vals, keep, _stub_graph(rows, cols, n, n, vals)


def test_host_checks_raise_before_any_launch(monkeypatch):
    from mmrec_amd import _lib, hip_ops
    monkeypatch.setattr(_lib, "load", lambda: pytest.fail("a launch was prepared"))
    n, rows, cols, vals, keep, eg = _small()
    X = torch.randn(n, 64)
    bad = [
        (eg, X, keep),                                                # host tensors: no CPU path
        (eg, X, keep.to(torch.uint8)),                                # keep dtype
        (eg, X, keep.float()),
        (eg, X, keep[:-1]),                                           # keep length
        (eg, X[:n - 1], keep),                                        # X rows < n_cols
        (eg, X.double(), keep),
        ("not a graph", X, keep),
    ]
    for op in (lambda e, x, k: hip_ops.spmm_edge_dropout(e, x, k, 2.0),
               lambda e, x, k: hip_ops.lightgcn_mean_edge_dropout(e, x, 2, k, 2.0)):
        for args in bad:
            with pytest.raises(_lib.MMRecHipError):
                op(*args)
    grad = _stub_graph(rows, cols, n, n, vals.clone().requires_grad_())
    with pytest.raises(_lib.MMRecHipError, match="grad"):
        hip_ops.spmm_edge_dropout(grad, X, keep)
    # the constructor: wrong graph type, dtype, length, a value vector that requires grad, a host tensor
    dyn = eg.dyn
    for v in (vals.double(), vals[:-1], vals.clone().requires_grad_(), vals.reshape(-1, 1), vals):
        with pytest.raises(_lib.MMRecHipError):
            hip_ops.EdgeDropoutGraph(dyn, v)
    with pytest.raises(_lib.MMRecHipError):
        hip_ops.EdgeDropoutGraph("dyn", vals)
    with pytest.raises(_lib.MMRecHipError):
        hip_ops.edge_keep_bits(keep)                                  # host tensor
    with pytest.raises(_lib.MMRecHipError):
        hip_ops.edge_keep_bits(keep.float())


def test_raw_entries_reject_bad_arguments():
    from mmrec_amd import _lib
    lib = _lib.load()
    BAD, UNS = 10001, 10002
    P = ctypes.c_void_p
    a, b, c = P(4096), P(8192), P(12288)                              # never dereferenced: every call below is refused first

    def masked(rowptr=a, X=b, Y=c, acc_in=None, acc_out=None, bits=a, n_rows=10, d=64, thr=16, n_long=0, n_chunks=0):
        return lib.mmrec_spmm_csr_masked_f32(rowptr, a, a, X, Y, None, acc_in, acc_out, n_rows, d, 1.0, 0.0, 1.0, thr, None, None,
                                             n_long, n_chunks, None, None, bits, 1.0, None)
    assert masked(rowptr=None) == BAD and masked(X=None) == BAD and masked(bits=None) == BAD and masked(Y=None) == BAD
    assert masked(n_rows=-1) == BAD and masked(thr=-1) == BAD and masked(n_long=-1) == BAD and masked(n_chunks=-1) == BAD
    assert masked(Y=b) == BAD and masked(acc_in=c, acc_out=b) == BAD  # Y == X, acc_out == X
    assert masked(Y=None, acc_out=c) == BAD                           # acc_out without acc_in
    assert masked(n_long=2, n_chunks=3) == BAD                        # a plan without its arrays
    for d in (8, 16, 32, 24, 448, 0):                                 # the slices have no masked form
        assert masked(d=d) == UNS
    assert masked(n_rows=0) == 0                                      # nothing to do, nothing launched
    assert lib.mmrec_edge_keep_bits(None, 5, None, a, None, None, None) == BAD
    assert lib.mmrec_edge_keep_bits(a, 5, None, None, None, None, None) == BAD
    assert lib.mmrec_edge_keep_bits(a, -1, None, b, None, None, None) == BAD
    assert lib.mmrec_edge_keep_bits(a, 5, None, b, a, None, None) == BAD      # a second order without its output
    assert lib.mmrec_edge_keep_bits(a, 5, None, b, None, b, None) == BAD      # both outputs the same words
    assert lib.mmrec_edge_keep_bits(a, 5, None, a, None, None, None) == BAD   # in place
    assert lib.mmrec_edge_keep_bits(None, 0, None, None, None, None, None) == 0


# ------------------------------------------------------------------------------------------------ the composition
def _dense(rows, cols, vals, n):
    A = torch.zeros(n, n, dtype=torch.float64)
    A.index_put_((rows, cols), vals.double(), accumulate=True)
    return A


def test_composition_is_selected_and_computes_the_formula(monkeypatch):
    """unserved width or switch off -> spmm_vals on (vals * keep) * scale per layer and stack().mean(); the masked entry points
    are not reached.  spmm_vals is replaced by a dense host product here (its kernels are tested on the device)."""
    from mmrec_amd import hip_ops
    n, rows, cols, vals, keep, eg = _small()
    seen = []

    def dense_spmm_vals(dyn, X, v):
        assert dyn is eg.dyn
        seen.append(v.clone())
        return (_dense(dyn.rows, dyn.cols, v, n) @ X.double()).float()
    monkeypatch.setattr(hip_ops, "spmm_vals", dense_spmm_vals)
    monkeypatch.setattr(hip_ops, "_edge_dropout_check", lambda *a: None)          # (host tensors stand in for device ones)
    monkeypatch.setattr(hip_ops, "spmm_masked_raw", lambda *a, **k: pytest.fail("the masked launch ran"))
    monkeypatch.setattr(hip_ops, "edge_keep_bits", lambda *a, **k: pytest.fail("the pack ran"))
    scale = 1.0 / (1.0 - 0.3)
    A = _dense(rows, cols, vals * keep, n) * float(np.float32(scale))
    for width, switch in ((32, True), (64, False), (448, True)):
        monkeypatch.setattr(hip_ops, "EDGE_DROPOUT", switch)
        X = torch.randn(n, width, generator=torch.Generator().manual_seed(width))
        assert not hip_ops.edge_dropout_served(eg, X)
        seen.clear()
        out = hip_ops.spmm_edge_dropout(eg, X, keep, scale)
        assert len(seen) == 1 and torch.equal(seen[0], (vals * keep.to(vals.dtype)) * scale)
        torch.testing.assert_close(out.double(), A @ X.double(), rtol=1e-5, atol=1e-5)
        for L in (0, 1, 3):
            seen.clear()
            out = hip_ops.lightgcn_mean_edge_dropout(eg, X, L, keep, scale)
            assert len(seen) == L
            ref = cur = X.double()
            for _ in range(L):
                cur = A @ cur
                ref = ref + cur
            torch.testing.assert_close(out.double(), ref / (L + 1), rtol=1e-4, atol=1e-4)
    monkeypatch.setattr(hip_ops, "EDGE_DROPOUT", True)
    for width in (64, 128, 384):
        assert hip_ops.edge_dropout_served(eg, torch.zeros(n, width))
    assert hip_ops.EDGE_DROPOUT is True


def test_encoder_key_is_off_by_default_and_documented():
    import os
    import yaml
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    path = os.path.join(root, "mmrec_amd", "configs", "model", "SELFCFED_LGN.yaml")
    text = open(path).read()
    assert "fused_edge_dropout" in text
    assert "fused_edge_dropout" not in (yaml.safe_load(text) or {})   # a comment only: the shipped value stays off
