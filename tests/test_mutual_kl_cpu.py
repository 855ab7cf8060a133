"""No GPU: DAMRS's symmetric KL term (csrc/mutual_kl.hip, hip_ops.mutual_kl) -- the exports and the argument checks of the C entry
points, the plan and the workspace, what the wrapper serves, the composition that everything else (here: CPU tensors) takes bit
for bit, the collapsed form J against the composition's formula in float64, DAMRS's `fused_kl` key on the golden step, and the
checker of tests/test_mutual_kl_fuzz_gpu.py held honest: an fp32 numpy emulation of the forward's plan as include/mmrec_hip.h
states it passes, planted errors do not."""
import os

import numpy as np
import pytest
import torch

import tests.test_models_gpu as G
import tests.test_mutual_kl_fuzz_gpu as Z
from mmrec_amd import _lib
from tests._cpu_ops import cpu_ops  # noqa: F401  (fixture)
from tests.test_pseudo_labels_cpu import damrs_step, meets_the_golden

EXPORTS = ("mmrec_mutual_kl_f32", "mmrec_mutual_kl_bwd_f32", "mmrec_mutual_kl_workspace_bytes", "mmrec_mutual_kl_split_cols")
BAD, UNSUPPORTED = 10001, 10002
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        from mmrec_amd.build import build
        build(verbose=False)
    return _lib.load()


@pytest.fixture
def deterministic_torch():
    was = torch.are_deterministic_algorithms_enabled()
    torch.use_deterministic_algorithms(True)
    yield
    torch.use_deterministic_algorithms(was)


def test_exports_in_header_signatures_and_library(lib):
    import ctypes
    src = open(os.path.join(ROOT, "include", "mmrec_hip.h")).read()
    for name in EXPORTS:
        assert name in _lib.SIGNATURES and name in src and hasattr(lib, name), name
    assert "#define MMREC_ABI_VERSION 16" in src and lib.mmrec_abi_version() == 16 and _lib.ABI_VERSION == 16   # additive
    flat = " ".join(src.split())
    for decl in ("int32_t mmrec_mutual_kl_split_cols(int32_t m, int32_t n, int32_t mode);",
                 "size_t mmrec_mutual_kl_workspace_bytes(int32_t m, int32_t n, int32_t d);",
                 "int mmrec_mutual_kl_f32(const float* U, const float* A, const float* B, int32_t m, int32_t n, int32_t d, "
                 "float scale, float* out, void* workspace, mmrec_stream_t stream);",
                 "int mmrec_mutual_kl_bwd_f32(const float* U, const float* A, const float* B, int32_t m, int32_t n, int32_t d, "
                 "float scale, const float* g, float* dU, float* dA, float* dB, void* workspace, mmrec_stream_t stream);"):
        assert decl in flat, decl
    P, I, F = ctypes.c_void_p, ctypes.c_int32, ctypes.c_float
    assert _lib.SIGNATURES["mmrec_mutual_kl_split_cols"] == (I, [I, I, I])
    assert _lib.SIGNATURES["mmrec_mutual_kl_workspace_bytes"] == (ctypes.c_size_t, [I, I, I])
    assert _lib.SIGNATURES["mmrec_mutual_kl_f32"] == (I, [P, P, P, I, I, I, F, P, P, P])
    assert _lib.SIGNATURES["mmrec_mutual_kl_bwd_f32"] == (I, [P, P, P, I, I, I, F, P, P, P, P, P, P])
    from mmrec_amd.build import SOURCES
    assert "mutual_kl.hip" in SOURCES


def test_entry_points_refuse_bad_arguments_before_touching_memory(lib):
    """every call below would fault if a pointer were followed or a kernel launched: this machine has no device"""
    f, b = lib.mmrec_mutual_kl_f32, lib.mmrec_mutual_kl_bwd_f32
    assert f(None, None, None, 5, 7, 64, 1.0, None, None, None) == BAD                       # null pointers
    assert b(None, None, None, 5, 7, 64, 1.0, None, None, None, None, None, None) == BAD
    for d in (0, 32, 63, 65, 128, -64):                                                      # d is 64, checked first
        assert f(None, None, None, 5, 7, d, 1.0, None, None, None) == BAD, d
        assert b(None, None, None, 5, 7, d, 1.0, None, None, None, None, None, None) == BAD, d
    for m, n in ((-1, 7), (5, -7)):                                                          # negative sizes
        assert f(None, None, None, m, n, 64, 1.0, None, None, None) == BAD
        assert b(None, None, None, m, n, 64, 1.0, None, None, None, None, None, None) == BAD
    assert f(None, None, None, (1 << 30) + 1, 7, 64, 1.0, None, None, None) == UNSUPPORTED
    assert b(None, None, None, 5, (1 << 30) + 1, 64, 1.0, None, None, None, None, None, None) == UNSUPPORTED
    assert f(None, None, None, 0, 7, 64, 1.0, None, None, None) == BAD                       # no pair, but nowhere to write 0
    assert b(None, None, None, 0, 0, 64, 1.0, None, None, None, None, None, None) == 0
    wsb, sc = lib.mmrec_mutual_kl_workspace_bytes, lib.mmrec_mutual_kl_split_cols
    assert wsb(5, 7, 32) == 0 and wsb(5, 7, 128) == 0 and wsb(-1, 7, 64) == 0 and wsb(0, 7, 64) == 0 and wsb(5, 0, 64) == 0
    assert sc(5, 0, 0) == 0 and sc(0, 5, 0) == 0 and sc(5, 7, 3) == 0 and sc(5, 7, -1) == 0 and sc(-5, 7, 0) == 0


def test_workspace_is_linear_in_the_operands_and_the_splits(lib):
    """one float per forward workgroup, at most 4 (m + n) 64 floats of partials per gradient: never an [m, n] block; the plan is a
    function of (m, n) alone"""
    for m, n in ((2048, 4096), (2048, 3900), (1900, 4096), (2048, 19445), (2048, 192403), (257, 4097), (1, 4097), (4097, 1), (1, 1)):
        ws = lib.mmrec_mutual_kl_workspace_bytes(m, n, 64)
        s = [lib.mmrec_mutual_kl_split_cols(m, n, mode) for mode in range(3)]
        assert all(x > 0 and x % 64 == 0 for x in s), (m, n, s)
        parts = -(-m // 128) * -(-n // s[0])
        assert -(-n // s[0]) <= 64 and -(-n // s[1]) <= 16 and -(-m // s[2]) <= 16
        assert 4 * parts <= ws <= 4 * (max(parts, 12 * (m + n) * 64)), (m, n, ws)
        assert ws == lib.mmrec_mutual_kl_workspace_bytes(m, n, 64)
        assert s == [lib.mmrec_mutual_kl_split_cols(m, n, mode) for mode in range(3)]
        if m * n >= 1 << 22:
            assert ws < m * n * 4, (m, n, ws)                                                # under ONE block
    assert lib.mmrec_mutual_kl_split_cols(257, 4097, 0) > 64          # the fuzz's multi-tile split
    from mmrec_amd import hip_ops
    assert hip_ops.mutual_kl_split_cols(257, 4097, 1) == lib.mmrec_mutual_kl_split_cols(257, 4097, 1)


def test_served_is_about_device_dtype_shape_and_width():
    from mmrec_amd import hip_ops

    class OnDevice(torch.Tensor):                                    # a stand-in that says it lives on the device
        is_cuda = True
    dev = lambda t: t.as_subclass(OnDevice) if isinstance(t, torch.Tensor) else t                     # noqa: E731
    served = hip_ops.mutual_kl_served
    Um, A, B = torch.zeros(6, 64), torch.zeros(9, 64), torch.zeros(9, 64)
    assert not served(Um, A, B)                                       # CPU tensors: never
    assert not served(dev(Um), A, dev(B)) and not served(Um, dev(A), dev(B)) and not served(dev(Um), dev(A), B)
    assert served(dev(Um), dev(A), dev(B))
    assert served(dev(torch.zeros(1, 64)), dev(torch.zeros(1, 64)), dev(torch.zeros(1, 64)))
    X = dev(torch.zeros(9, 64))
    assert served(X, X, X)
    for bad in ((torch.zeros(6, 32), torch.zeros(9, 32), torch.zeros(9, 32)), (torch.zeros(6, 128), torch.zeros(9, 128), torch.zeros(9, 128)),
                (Um, torch.zeros(9, 32), B), (Um, A, torch.zeros(8, 64)),                                              # widths, lengths
                (torch.zeros(0, 64), A, B), (Um, torch.zeros(0, 64), torch.zeros(0, 64)),                              # empty
                (Um.double(), A, B), (Um, A.half(), B), (Um, A, B.to(torch.bfloat16)),                                 # dtype
                (torch.zeros(6, 128)[:, ::2], A, B), (Um, torch.zeros(18, 64)[::2], B), (Um, A, torch.zeros(64, 9).t()),   # layout
                (torch.zeros(6 * 64), A, B), (Um, A, torch.zeros(1, 9, 64)), (None, A, B), (Um, None, B), (Um, A, None)):
        assert not served(*(dev(t) for t in bad)), [getattr(t, "shape", None) for t in bad]


def _model_composition(Um, A, B):
    """DAMRS.calculate_loss's lines, with the model's own _kl"""
    from mmrec_amd.models.damrs import DAMRS
    p_g = torch.sigmoid(torch.mm(Um, A.t()))
    p_m = torch.sigmoid(torch.mm(Um, B.t()))
    return torch.mean(DAMRS._kl(p_g, p_m) + DAMRS._kl(p_m, p_g))


@pytest.mark.parametrize("shape", [(37, 211, 64), (5, 3, 24), (1, 1, 64)], ids=str)
def test_cpu_tensors_take_the_composition_bit_for_bit(deterministic_torch, shape):
    from mmrec_amd import hip_ops
    m, n, d = shape
    runs = []
    for fn in (hip_ops.mutual_kl, hip_ops.mutual_kl_torch, _model_composition):
        ts = [torch.from_numpy(np.random.default_rng(2 + j).standard_normal(s).astype(np.float32) * 0.4).requires_grad_()
              for j, s in enumerate(((m, d), (n, d), (n, d)))]
        assert not hip_ops.mutual_kl_served(*ts)
        out = fn(*ts)
        assert out.shape == () and out.dtype == torch.float32
        (out * 1.7).backward()
        runs.append((out.detach(), *(t.grad for t in ts)))
    for other in runs[1:]:
        for a, b in zip(runs[0], other):
            assert torch.equal(a, b)
    assert all(float(t.abs().max()) > 0 for t in runs[0])
    empty = hip_ops.mutual_kl(torch.zeros(0, 64), torch.zeros(3, 64), torch.zeros(3, 64))      # the composition's value: a mean of nothing
    assert bool(torch.isnan(empty))


def test_J_is_the_compositions_formula_in_float64():
    """(sigmoid(a) - sigmoid(b)) (a - b) = KL(p || q) + KL(q || p) on DAMRS-like operands: to 1e-15 absolute per pair and in the
    mean; past |logit| ~ 17 in fp32 the composition is NaN and J is not"""
    from mmrec_amd import hip_ops
    from mmrec_amd.models.damrs import DAMRS
    rng = np.random.default_rng(11)
    unit = lambda x: x / np.linalg.norm(x, axis=1, keepdims=True)      # noqa: E731
    Um = rng.standard_normal((300, 64)) * 0.1 * rng.uniform(0.2, 4.0, (300, 1))
    A, B = unit(rng.standard_normal((500, 64))), unit(rng.standard_normal((500, 64)))
    a, b = torch.from_numpy(Um @ A.T), torch.from_numpy(Um @ B.T)
    p, q = torch.sigmoid(a), torch.sigmoid(b)
    J = (p - q) * (a - b)
    kl = DAMRS._kl(p, q) + DAMRS._kl(q, p)
    worst = float((J - kl).abs().max())
    mean_gap = abs(float(J.mean()) - float(hip_ops.mutual_kl(*(torch.from_numpy(x) for x in (Um, A, B)))))
    print("float64: J against the composition, worst pair %.3e, the mean %.3e" % (worst, mean_gap))
    assert worst <= 1e-15 and mean_gap <= 1e-15 and float(J.abs().max()) > 1e-3
    r = Z.ref64(Z.case(1))
    assert np.array_equal(r.J, (Z.sigmoid64(r.a) - Z.sigmoid64(r.b)) * (r.a - r.b))
    big = torch.tensor([[30.0]]), torch.tensor([[1.0]]), torch.tensor([[-1.0]])
    assert not bool(torch.isfinite(hip_ops.mutual_kl_torch(*big)))
    x, y = torch.tensor(30.0), torch.tensor(-30.0)
    assert bool(torch.isfinite((torch.sigmoid(x) - torch.sigmoid(y)) * (x - y)))


# ------------------------------------------------------------------------------------------------ the model's key
def test_damrs_fused_kl_key_on_the_cpu(tmp_path, golden, cpu_ops, deterministic_torch, monkeypatch):  # noqa: F811
    """absent, False: today's path, mutual_kl never asked; True on CPU tensors: asked once (the composition), the reference's
    golden step met, and the key-off loss and gradients at the same tolerances; with fused_labels too"""
    from mmrec_amd import hip_ops
    monkeypatch.setattr(G, "USE_GPU", False)
    asked = []
    monkeypatch.setattr(hip_ops, "mutual_kl", lambda *a, _real=hip_ops.mutual_kl: asked.append([tuple(t.shape) for t in a]) or _real(*a))
    m0, loss0, g0, g = damrs_step(tmp_path / "absent", golden, {})
    m1, loss1, g1, _ = damrs_step(tmp_path / "off", golden, {"fused_kl": False})
    assert m0.fused_kl is False and m1.fused_kl is False and not asked
    assert torch.equal(loss0, loss1) and all(torch.equal(g0[k], g1[k]) for k in g0)
    for extra in ({"fused_kl": True}, {"fused_kl": True, "fused_labels": True}):
        del asked[:]
        m2, loss2, g2, _ = damrs_step(tmp_path / ("on%d" % len(extra)), golden, extra)
        assert m2.fused_kl is True and m2.fused_labels is ("fused_labels" in extra)
        assert len(asked) == 1 and asked[0][0][1] == 64 and asked[0][1] == asked[0][2]
        meets_the_golden(loss2, g2, g)
        G.close(loss2, loss0.numpy(), rtol=2e-5)
        for nm in ("user_embedding.weight", "item_id_embedding.weight"):
            G.close(g2[nm], g0[nm].numpy(), rtol=1e-3, atol=2e-7)
        assert set(g2) == set(g0)
    meets_the_golden(loss0, g0, g)


def test_the_yaml_names_the_key_in_a_comment_only():
    import yaml
    text = open(os.path.join(ROOT, "mmrec_amd", "configs", "model", "DAMRS.yaml")).read()
    loaded = yaml.safe_load(text)
    assert "# fused_kl: True" in text and "fused_kl" not in loaded
    assert "# fused_labels: True  # opt-in (absent = off): the neighbour-discrimination term without its" in text and "fused_labels" not in loaded


# ------------------------------------------------------------------------------------------------ the fuzz's checker
D_ROW = np.array([[(r & 3) + 8 * (r >> 2) + 4 * h for r in range(16)] for h in (0, 1)])
LANES = np.arange(64)


def _butterfly(v):
    """wave_sum over the last axis (64 lanes): xor 32, 16, 8, 4, 2, 1; every lane ends with the total"""
    for mask in (32, 16, 8, 4, 2, 1):
        v = v + v[..., LANES ^ mask]
    return v[..., 0]


def emulate_fwd(c, plant=None):
    """the forward's plan in fp32 numpy: logits as fma chains in k order, the kernels' sigmoid, J per pair, per lane (own row i,
    half h) the sum over the 32-row sub-tiles of its split in order (16 terms each: the items with bit 2 of i % 32 equal to h),
    the wave's butterfly (h first), the four waves in order, one partial per workgroup [split][own tile]; the finish: thread t
    the partials t, t + 256, ..., the butterfly, the four waves, times scale.
    `plant`: "drop" the last column of the first split, "double" the first column of the second tile, "scale" 1 / (m (n + 1))."""
    f32 = np.float32
    m, n = c.m, c.n
    a, b = np.zeros((m, n), f32), np.zeros((m, n), f32)
    for k in range(Z.D):
        u = c.U[:, k].astype(np.float64)[:, None]
        a = (u * c.A[:, k].astype(np.float64)[None, :] + a.astype(np.float64)).astype(f32)
        b = (u * c.B[:, k].astype(np.float64)[None, :] + b.astype(np.float64)).astype(f32)
    J = ((Z.sigmoid32(a) - Z.sigmoid32(b)) * (a - b)).astype(f32)
    s0 = Z.split_len(m, n, 0)
    if plant == "drop":
        J[:, min(s0, n) - 1] = 0
    if plant == "double":
        J[:, 64] *= f32(2)
    own_tiles, splits = -(-m // 128), -(-n // s0)
    Jp = np.zeros((own_tiles * 128, splits * s0), f32)
    Jp[:m, :n] = J
    parts = np.zeros((splits, own_tiles), f32)
    for sp in range(splits):
        Jb = Jp[:, sp * s0:(sp + 1) * s0].reshape(own_tiles, 4, 32, s0)
        acc = np.zeros((own_tiles, 4, 2, 32), f32)
        for t0 in range(0, s0, 32):
            for r in range(16):
                for h in (0, 1):
                    acc[:, :, h, :] = acc[:, :, h, :] + Jb[:, :, :, t0 + D_ROW[h][r]]
        w = _butterfly(acc.reshape(own_tiles, 4, 64))
        parts[sp] = ((w[:, 0] + w[:, 1]) + w[:, 2]) + w[:, 3]
    flat = parts.reshape(-1)
    rows = -(-flat.size // 256)
    grid = np.zeros(rows * 256, f32)
    grid[:flat.size] = flat
    grid = grid.reshape(rows, 256)
    th = np.zeros(256, f32)
    for e in range(rows):
        th = th + grid[e]
    w = _butterfly(th.reshape(4, 64))
    total = ((w[0] + w[1]) + w[2]) + w[3]
    scale = f32(1.0 / (float(m) * float(n + 1))) if plant == "scale" else f32(c.scale)
    return f32(scale * total)


def test_the_emulated_plan_passes_the_checker():
    ran, worst, kinds = 0, 0.0, set()
    for k in range(Z.CASES):
        c = Z.case(k)
        if c.m * c.n > 400000:
            continue
        worst = max(worst, Z.check_fwd(emulate_fwd(c), c, "emulated case %d" % k))
        kinds.add(c.kind)
        ran += 1
    print("emulated plan: %d cases, worst err / bound %.3f" % (ran, worst))
    assert ran >= 30 and worst <= 1.0 and kinds == set(Z.KINDS)


def _multi_split_case(kind):
    """the case of `kind` on 4,097 columns (two tiles a split, a last split of one column), 33 rows of it: quick to emulate"""
    base = next(c for c in map(Z.case, range(Z.CASES)) if c.kind == kind and c.n == 4097 and c.m == 257)
    c = Z.Case()
    c.__dict__.update(base.__dict__)
    c.m, c.U = 33, base.U[:33].copy()
    c.scale = float(np.float32(1.0 / (33.0 * 4097.0)))
    assert Z.split_len(c.m, c.n) == 128 and c.n % 128 == 1
    return c


@pytest.mark.parametrize("kind", ["sparse", "float"])
def test_checker_rejects_planted_errors_in_the_forward(kind):
    c = _multi_split_case(kind)
    if c.sparse:
        assert {63, 64, 127, 128} <= set(c.targets)
    assert Z.check_fwd(emulate_fwd(c), c, "clean") <= 1.0
    for plant in ("drop", "double", "scale"):          # a split's last column lost, a tile-boundary column twice, a wrong scale
        with pytest.raises(AssertionError):
            Z.check_fwd(emulate_fwd(c, plant), c, plant)


@pytest.mark.parametrize("kind", ["sparse", "float", "tie"])
def test_checker_rejects_planted_errors_in_the_backward(kind):
    """float64 of the formulas, rounded to fp32, passes; A and B swapped in the backward, a lost column, a doubled column and a
    wrong scale do not"""
    c = next(c for c in map(Z.case, range(Z.CASES)) if c.kind == kind and c.n >= 63 and c.m >= 31 and c.m * c.n < 100000)
    bd = Z.bounds_of(c)
    r = bd[0]
    f32 = lambda x: x.astype(np.float32)                              # noqa: E731
    assert Z.check_bwd(f32(r.dU), f32(r.dA), f32(r.dB), c, "clean", bd) <= 1.0
    with pytest.raises(AssertionError):                               # A and B swapped: dA and dB trade places
        Z.check_bwd(f32(r.dU), f32(r.dB), f32(r.dA), c, "swapped", bd)
    U64, A64, B64 = (x.astype(np.float64) for x in (c.U, c.A, c.B))
    col = c.targets[-1] if c.sparse else c.n - 1
    ga, gb = r.ga.copy(), r.gb.copy()
    ga[:, col] = gb[:, col] = 0.0                                     # the last column lost
    if kind != "tie":               # near a tie ga A[i] and gb B[i] cancel in dU to below the rounding of either: dA and dB tell
        with pytest.raises(AssertionError):
            Z.check_bwd(f32(ga @ A64 + gb @ B64), f32(r.dA), f32(r.dB), c, "dU lost a column", bd)
    with pytest.raises(AssertionError):
        Z.check_bwd(f32(r.dU), f32(ga.T @ U64), f32(r.dB), c, "dA lost a row", bd)
    col = c.targets[len(c.targets) // 2] if c.sparse else 32
    ga, gb = r.ga.copy(), r.gb.copy()
    ga[:, col] *= 2.0                                                 # a sub-tile boundary column twice
    gb[:, col] *= 2.0
    if kind != "tie":
        with pytest.raises(AssertionError):
            Z.check_bwd(f32(ga @ A64 + gb @ B64), f32(r.dA), f32(r.dB), c, "dU doubled a column", bd)
    with pytest.raises(AssertionError):
        Z.check_bwd(f32(r.dU), f32(r.dA), f32(gb.T @ U64), c, "dB doubled a row", bd)
    wrong = c.n / (c.n + 1.0)                                         # scale 1 / (m (n + 1))
    with pytest.raises(AssertionError):
        Z.check_bwd(f32(r.dU * wrong), f32(r.dA * wrong), f32(r.dB * wrong), c, "scale", bd)
    if c.sparse:                                                      # anything at all in an off-target row
        dA = f32(r.dA)
        off = next(i for i in range(c.n) if i not in c.targets)
        dA[off, 5] = 1e-30
        with pytest.raises(AssertionError):
            Z.check_bwd(f32(r.dU), dA, f32(r.dB), c, "off-target", bd)
