"""CPU: the contrastive log-sum-exp (mmrec_score_lse_f32, hip_ops.score_lse) without a GPU -- the exports and the argument
checks of the C entry points, what the wrapper serves, the torch composition that everything else (here: CPU tensors) takes bit
for bit, LGMRec's and PGL's `fused_ssl` key on the tiny golden data (with the stand-in ops both settings are torch: the same
loss and gradients within fp32 parity, the contrastive term compared alone, LGMRec's golden step still met), and the checker of
tests/test_score_lse_fuzz_gpu.py held honest: an fp32 numpy emulation of the kernel's plan passes it, planted errors do not."""
import os

import numpy as np
import pytest
import torch

import tests.test_models_gpu as G
import tests.test_score_lse_fuzz_gpu as Z
from mmrec_amd import _lib
from tests._cpu_ops import cpu_ops  # noqa: F401  (fixture)

EXPORTS = ("mmrec_score_lse_f32", "mmrec_score_lse_bwd_f32", "mmrec_score_lse_workspace_bytes", "mmrec_score_lse_split_cols")
RTOL = 1e-4                    # README: fp32 parity
BAD, UNSUPPORTED = 10001, 10002


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        from mmrec_amd.build import build
        build(verbose=False)
    return _lib.load()


@pytest.fixture
def deterministic_torch():
    """bit-for-bit comparisons of gradients run in torch's deterministic mode (tests/test_edge_attention_cpu.py)"""
    was = torch.are_deterministic_algorithms_enabled()
    torch.use_deterministic_algorithms(True)
    yield
    torch.use_deterministic_algorithms(was)


def test_exports_in_header_signatures_and_library(lib):
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mmrec_hip.h")).read()
    for name in EXPORTS:
        assert name in _lib.SIGNATURES and name in src and hasattr(lib, name), name
    assert "#define MMREC_ABI_VERSION 16" in src and lib.mmrec_abi_version() == 16 and _lib.ABI_VERSION == 16   # additive
    from mmrec_amd.build import SOURCES
    assert "score_lse.hip" in SOURCES


def test_entry_points_refuse_bad_arguments_before_touching_memory(lib):
    """every call below would fault if a pointer were followed or a kernel launched: this machine has no device"""
    f, b = lib.mmrec_score_lse_f32, lib.mmrec_score_lse_bwd_f32
    assert f(None, None, 5, 7, 64, 1.0, None, None, None) == BAD                    # null pointers
    assert f(None, None, 5, 7, 128, 1.0, None, None, None) == BAD
    for d in (0, 32, 63, 96, 256, -64):                                             # d is 64 or 128, checked first
        assert f(None, None, 5, 7, d, 1.0, None, None, None) == BAD, d
        assert b(None, None, 5, 7, d, 1.0, None, None, None, None, None, None) == BAD, d
    assert f(None, None, -1, 7, 64, 1.0, None, None, None) == BAD                   # negative sizes
    assert f(None, None, 5, -7, 64, 1.0, None, None, None) == BAD
    assert b(None, None, -1, 7, 64, 1.0, None, None, None, None, None, None) == BAD
    assert b(None, None, 5, -7, 64, 1.0, None, None, None, None, None, None) == BAD
    assert b(None, None, 5, 7, 64, 1.0, None, None, None, None, None, None) == BAD  # null pointers
    assert f(None, None, (1 << 30) + 1, 7, 64, 1.0, None, None, None) == UNSUPPORTED
    assert f(None, None, 0, 7, 64, 1.0, None, None, None) == 0                      # an empty batch: nothing to do
    assert b(None, None, 0, 0, 64, 1.0, None, None, None, None, None, None) == 0
    assert lib.mmrec_score_lse_workspace_bytes(5, 7, 32) == 0 and lib.mmrec_score_lse_workspace_bytes(-1, 7, 64) == 0
    assert lib.mmrec_score_lse_workspace_bytes(0, 7, 64) == 0
    assert lib.mmrec_score_lse_split_cols(5, 0, 0) == 0 and lib.mmrec_score_lse_split_cols(5, 7, 3) == 0


def test_workspace_is_linear_in_the_operands_and_the_splits(lib):
    """O((B + N) d + splits B): never the B x N matrix, and the plan is a function of the shape alone"""
    for B, N, d in ((2048, 7050, 64), (2048, 19445, 64), (2048, 192403, 64), (2048, 2048, 128), (1024, 32768, 64), (1, 1, 64)):
        ws = lib.mmrec_score_lse_workspace_bytes(B, N, d)
        s0 = lib.mmrec_score_lse_split_cols(B, N, 0)
        assert s0 % 64 == 0 and s0 > 0
        splits = -(-N // s0)
        assert 0 < ws <= 4 * (8 * (B + N) * d + 2 * splits * B), (B, N, d, ws)
        assert ws == lib.mmrec_score_lse_workspace_bytes(B, N, d)
        if B * N >= 1 << 24:
            assert ws < B * N * 4 // 4
    assert lib.mmrec_score_lse_split_cols(257, 4097, 0) > 64          # the fuzz's multi-tile split


@pytest.mark.parametrize("same", [False, True], ids=["distinct", "Q_is_K"])
@pytest.mark.parametrize("d", [64, 128, 24])
def test_cpu_tensors_take_the_torch_composition_bit_for_bit(deterministic_torch, same, d):
    from mmrec_amd import hip_ops
    rng = np.random.default_rng(4)
    B, N = (37, 37) if same else (37, 211)
    w = torch.from_numpy(rng.standard_normal(B).astype(np.float32))
    runs = []
    for fn in (hip_ops.score_lse, lambda Q, K, s: torch.logsumexp(s * (Q @ K.T), dim=1)):
        Q = torch.from_numpy(np.random.default_rng(2).standard_normal((B, d)).astype(np.float32)).requires_grad_()
        K = Q if same else torch.from_numpy(np.random.default_rng(3).standard_normal((N, d)).astype(np.float32)).requires_grad_()
        assert not hip_ops.score_lse_served(Q, K)
        lse = fn(Q, K, 2.5)
        assert lse.shape == (B,) and lse.dtype == torch.float32
        (lse * w).sum().backward()
        runs.append((lse.detach(), Q.grad, K.grad))
    for a, b in zip(*runs):
        assert torch.equal(a, b)
    assert float(runs[0][1].abs().max()) > 0
    # and it IS the formulas: float64 of lse, dQ and dK as the header writes them
    Q64, K64 = Q.detach().double(), K.detach().double()
    x = 2.5 * (Q64 @ K64.T)
    ref = torch.logsumexp(x, dim=1)
    tol = 2.5 * Z.gamma(d) * float((Q64.abs() @ K64.abs().T).max()) + 4 * Z.U * float(ref.abs().max())     # the dots, then the rest
    assert float((runs[0][0].double() - ref).abs().max()) <= tol
    p = torch.exp(x - ref[:, None])
    dQ, dK = 2.5 * w.double()[:, None] * (p @ K64), 2.5 * (p * w.double()[:, None]).T @ Q64
    if same:
        assert float((runs[0][1].double() - (dQ + dK)).abs().max()) <= RTOL * float((dQ + dK).abs().max())
    else:
        assert float((runs[0][1].double() - dQ).abs().max()) <= RTOL * float(dQ.abs().max())
        assert float((runs[0][2].double() - dK).abs().max()) <= RTOL * float(dK.abs().max())


def test_an_empty_table_gives_minus_infinity_and_an_empty_batch_nothing():
    from mmrec_amd import hip_ops
    Q = torch.zeros(3, 64, requires_grad=True)
    lse = hip_ops.score_lse(Q, torch.zeros(0, 64), 2.0)
    assert lse.shape == (3,) and bool(torch.isneginf(lse).all())
    assert hip_ops.score_lse(torch.zeros(0, 64), torch.zeros(5, 64), 2.0).shape == (0,)


def test_served_is_about_device_dtype_shape_and_width():
    from mmrec_amd import hip_ops

    class OnDevice(torch.Tensor):                                    # a stand-in that says it lives on the device
        is_cuda = True
    dev = lambda t: t.as_subclass(OnDevice)                          # noqa: E731
    Q, K = torch.zeros(6, 64), torch.zeros(9, 64)
    assert not hip_ops.score_lse_served(Q, K)                         # CPU tensors: never
    assert not hip_ops.score_lse_served(dev(Q), K) and not hip_ops.score_lse_served(Q, dev(K))
    assert hip_ops.score_lse_served(dev(Q), dev(K))
    assert hip_ops.score_lse_served(dev(torch.zeros(6, 128)), dev(torch.zeros(2, 128)))       # N < B, width 128
    assert hip_ops.score_lse_served(dev(Q), dev(torch.zeros(0, 64)))                          # an empty table
    X = dev(torch.zeros(6, 64))
    assert hip_ops.score_lse_served(X, X)                             # Q is K
    for bad_q, bad_k in ((torch.zeros(6, 32), torch.zeros(9, 32)), (torch.zeros(6, 256), torch.zeros(9, 256)),     # widths
                         (torch.zeros(6, 64), torch.zeros(9, 128)),
                         (torch.zeros(6, 64, dtype=torch.float64), K), (Q, torch.zeros(9, 64, dtype=torch.float16)),    # dtype
                         (torch.zeros(6, 128)[:, ::2], K), (Q, torch.zeros(18, 64)[::2]),                           # not contiguous
                         (torch.zeros(6 * 64), K), (None, K), (Q, None)):
        q = dev(bad_q) if isinstance(bad_q, torch.Tensor) else bad_q
        k = dev(bad_k) if isinstance(bad_k, torch.Tensor) else bad_k
        assert not hip_ops.score_lse_served(q, k), (getattr(bad_q, "shape", None), getattr(bad_k, "shape", None))


# ------------------------------------------------------------------------------------------------ the plugins' key
LGM_EXTRA = {"n_ui_layers": 2, "n_mm_layers": 2, "n_hyper_layer": 1, "hyper_num": 4, "keep_rate": 0.5, "alpha": 0.3,
             "cl_weight": 1e-4, "reg_weight": 1e-6}
PGL_EXTRA = {"dropout": 0.2, "reg_weight": 0.1, "mode": "local"}


def _step(tmp_path, golden, name, extra, fused):
    extra = dict(extra)
    if fused is not None:
        extra["fused_ssl"] = fused
    config, train_data, _, model = G.build(tmp_path, golden, name, extra)
    assert model.fused_ssl is bool(fused)
    batch = next(iter(train_data)).clone()
    model.train()
    torch.manual_seed(77)
    model.pre_epoch_processing()
    loss = model.calculate_loss(batch)
    loss.backward()
    return model, loss.detach(), {n: p.grad.detach().clone() for n, p in model.named_parameters() if p.grad is not None}


def _same_within_parity(loss_on, g_on, loss_off, g_off):
    assert np.isfinite(float(loss_on)) and abs(float(loss_on) - float(loss_off)) <= RTOL * abs(float(loss_off))
    assert set(g_on) == set(g_off) and len(g_on) >= 4
    for n in sorted(g_on):
        a, b = g_on[n].double().numpy(), g_off[n].double().numpy()
        scale = float(np.abs(b).max())
        assert np.isfinite(a).all() and float(np.abs(a - b).max()) <= RTOL * scale, (n, float(np.abs(a - b).max()), scale)


def _term_alone(fused_fn, plain_fn, shapes, seed):
    """the contrastive term on its own operands, value and gradients: the total hides it behind a small weight"""
    out = []
    for fn in (fused_fn, plain_fn):
        ts = [torch.from_numpy(np.random.default_rng(seed + j).standard_normal(s).astype(np.float32)).requires_grad_()
              for j, s in enumerate(shapes)]
        v = fn(*ts)
        v.backward()
        out.append((v.detach(), [t.grad for t in ts]))
    (v1, g1), (v0, g0) = out
    assert abs(float(v1) - float(v0)) <= RTOL * abs(float(v0)), (float(v1), float(v0))
    for a, b in zip(g1, g0):
        scale = float(b.abs().max())
        assert scale > 0 and float((a - b).abs().max()) <= RTOL * scale


def test_lgmrec_fused_ssl_key_on_the_cpu(tmp_path, golden, cpu_ops, deterministic_torch, monkeypatch):  # noqa: F811
    from mmrec_amd import hip_ops
    monkeypatch.setattr(G, "USE_GPU", False)
    asked = []
    real = hip_ops.score_lse
    monkeypatch.setattr(hip_ops, "score_lse", lambda *a, **k: asked.append(1) or real(*a, **k))
    _, loss0, g0 = _step(tmp_path / "absent", golden, "LGMRec", LGM_EXTRA, None)
    _, loss1, g1 = _step(tmp_path / "off", golden, "LGMRec", LGM_EXTRA, False)
    assert not asked                                                  # absent or False: today's path, untouched
    assert torch.equal(loss0, loss1) and all(torch.equal(g0[n], g1[n]) for n in g0)
    model, loss2, g2 = _step(tmp_path / "on", golden, "LGMRec", LGM_EXTRA, True)
    assert len(asked) == 2                                            # against all users, against all items
    _same_within_parity(loss2, g2, loss1, g1)
    for n in ("v_hyper", "t_hyper", "item_id_embedding.weight"):
        assert float(g2[n].abs().max()) > 0, n
    plain = type(model).ssl_triple_loss
    off = type("Off", (), {"fused_ssl": False, "tau": model.tau})()
    _term_alone(lambda a, b, c: model.ssl_triple_loss(a, b, c), lambda a, b, c: plain(off, a, b, c),
                ((48, 64), (48, 64), (301, 64)), 21)


def test_pgl_fused_ssl_key_on_the_cpu(tmp_path, golden, cpu_ops, deterministic_torch, monkeypatch):  # noqa: F811
    from mmrec_amd import hip_ops
    from mmrec_amd.models.pgl import PGL
    monkeypatch.setattr(G, "USE_GPU", False)
    asked = []
    real = hip_ops.score_lse
    monkeypatch.setattr(hip_ops, "score_lse", lambda *a, **k: asked.append(a[0].shape[1]) or real(*a, **k))
    _, loss0, g0 = _step(tmp_path / "absent", golden, "PGL", PGL_EXTRA, None)
    _, loss1, g1 = _step(tmp_path / "off", golden, "PGL", PGL_EXTRA, False)
    assert not asked
    assert torch.equal(loss0, loss1) and all(torch.equal(g0[n], g1[n]) for n in g0)
    _, loss2, g2 = _step(tmp_path / "on", golden, "PGL", PGL_EXTRA, True)
    assert asked == [128, 128]                                        # the user views, the item views: [image | text] rows
    _same_within_parity(loss2, g2, loss1, g1)                         # the same dropout draws from the same seed
    _term_alone(lambda a, b: PGL.InfoNCE_fused(a, b, 0.2), lambda a, b: PGL.InfoNCE(a, b, 0.2), ((40, 128), (40, 128)), 31)


def test_lgmrec_golden_step_is_met_with_the_key_on(tmp_path, golden, cpu_ops, monkeypatch):  # noqa: F811
    """tests/test_models_gpu.py::test_lgmrec_model's step -- the reference's weights, batch, Gumbel noise and dropout masks
    replayed -- with `fused_ssl: True`, at that test's tolerances"""
    monkeypatch.setattr(G, "USE_GPU", False)
    lgm = dict(np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lgmrec.npz")))
    config, _, valid_data, model = G.build(tmp_path, golden, "LGMRec", dict(LGM_EXTRA, fused_ssl=True))
    assert model.fused_ssl is True
    params = dict(model.named_parameters())
    for name, p in params.items():
        G.load(p, lgm["p_" + name])
    dev = model.device
    import mmrec_amd.models.lgmrec as lmod
    queue_n = [torch.as_tensor(lgm["gumbel_%d" % j]).to(dev) for j in range(4)]
    queue_m = [torch.as_tensor(lgm["drop_mask_%d" % j].astype(np.float32)).to(dev) for j in range(4)]
    monkeypatch.setattr(lmod.F, "gumbel_softmax", lambda logits, tau=1, hard=False, dim=-1: ((logits + queue_n.pop(0)) / tau).softmax(dim))
    monkeypatch.setattr(lmod.F, "dropout", lambda x, p=0.5, training=True, inplace=False: x * queue_m.pop(0) / (1.0 - p) if training else x)
    loss = model.calculate_loss(torch.as_tensor(lgm["batch1"]).to(dev))
    loss.backward()
    G.close(loss, lgm["loss1"], rtol=1e-5)
    for name in ("user_embedding.weight", "item_id_embedding.weight", "item_image_trs", "item_text_trs", "v_hyper", "t_hyper"):
        G.close(params[name].grad, lgm["g_" + name], rtol=5e-4, atol=1e-8)


# ------------------------------------------------------------------------------------------------ the fuzz's checker
D_ROW = np.array([[(r & 3) + 8 * (r >> 2) + 4 * h for r in range(16)] for h in (0, 1)])


def emulate_fwd(c, plant=None, arg=None):
    """the kernel's forward plan in fp32 numpy: scores as fma chains in k order (each step one rounding of the exact product
    plus the accumulator), one product with scale, per (row, half) the running maximum and rescaled sum over the 32-column
    sub-tiles of a column split in order, the halves combined (h = 0 first), the splits combined in split order, M + log L.
    `plant`: "drop" one column (arg), "skip_partial" the last partial sub-tile, "scale_twice", "no_rescale" the split partials
    added without bringing them to the common maximum."""
    f32 = np.float32
    B, N, d = c.B, c.N, c.d
    acc = np.zeros((B, N), f32)
    for k in range(d):
        acc = (c.Q[:, k].astype(np.float64)[:, None] * c.K[:, k].astype(np.float64)[None, :] + acc.astype(np.float64)).astype(f32)
    x = f32(c.scale) * acc
    if plant == "scale_twice":
        x = f32(c.scale) * x
    if plant == "drop":
        x[:, arg] = -np.inf
    n_cols = N - N % 32 if plant == "skip_partial" else N
    s0 = Z.split_len(B, N)
    pm, pl = [], []
    with np.errstate(invalid="ignore", over="ignore"):
        for lo in range(0, N, s0):
            m, l = np.full((2, B), -np.inf, f32), np.zeros((2, B), f32)
            for t0 in range(lo, min(lo + s0, N), 32):
                for h in (0, 1):
                    cols = t0 + D_ROW[h]
                    xs = np.where((cols < n_cols)[None, :], x[:, np.minimum(cols, N - 1)], f32(-np.inf))
                    m_new = np.maximum(m[h], xs.max(axis=1))
                    ms = np.where(np.isneginf(m_new), f32(0), m_new)
                    l[h] = l[h] * np.exp(m[h] - ms)
                    for r in range(16):
                        l[h] = l[h] + np.exp(xs[:, r] - ms)
                    m[h] = m_new
            M = np.maximum(m[0], m[1])
            ms = np.where(np.isneginf(M), f32(0), M)
            pm.append(M)
            pl.append(l[0] * np.exp(m[0] - ms) + l[1] * np.exp(m[1] - ms))
        M = np.full(B, -np.inf, f32)
        for v in pm:
            M = np.maximum(M, v)
        ms = np.where(np.isneginf(M), f32(0), M)
        L = np.zeros(B, f32)
        for a, b in zip(pm, pl):
            L = L + (b if plant == "no_rescale" else b * np.exp(a - ms))
        return (M + np.log(L)).astype(f32)


def test_the_emulated_plan_passes_the_checker():
    ran, worst = 0, 0.0
    for k in range(Z.CASES):
        c = Z.case(k)
        if c.B == 0 or c.B * c.N > 70000 and not (c.N == 4097 and c.B <= 65):
            continue
        worst = max(worst, Z.check_fwd(emulate_fwd(c), c, "emulated case %d" % k))
        ran += 1
    print("emulated plan: %d cases, worst err / bound %.3f" % (ran, worst))
    assert ran >= 25 and worst <= 1.0
    kinds = {Z.case(k).kind for k in range(Z.CASES)}
    assert kinds == set(Z.KINDS)


def _multi_split_case(kind):
    """a case of `kind` on the large table (several tiles per split, a partial last sub-tile), small enough to emulate quickly"""
    c = next(c for c in map(Z.case, range(Z.CASES)) if c.kind == kind and c.N == 4097 and c.B == 257)
    c.B, c.Q, c.g = 33, c.Q[:33].copy(), c.g[:33].copy()
    if c.exact:
        c.jstar = c.jstar[:33].copy()
    assert Z.split_len(c.B, c.N) > 64 and c.N % 32
    return c


def test_checker_rejects_planted_errors():
    c = _multi_split_case("raw")
    assert Z.check_fwd(emulate_fwd(c), c, "clean") <= 1.0
    ref, F = Z.forward_bound(c)
    p = np.exp(Z.scores64(c) - ref[:, None])
    # one column dropped: one that carries a thousandth of a row's sum or more
    col = int(np.argmax(p.max(axis=0) >= 1e-3))
    assert p[:, col].max() >= 1e-3
    with pytest.raises(AssertionError):
        Z.check_fwd(emulate_fwd(c, "drop", col), c)
    # scale applied twice
    with pytest.raises(AssertionError):
        Z.check_fwd(emulate_fwd(c, "scale_twice"), c)
    # the split partials added without rescaling to the common maximum
    with pytest.raises(AssertionError):
        Z.check_fwd(emulate_fwd(c, "no_rescale"), c)
    # the last, partial sub-tile skipped: the exact mode holds a target in the last column
    e = _multi_split_case("exact")
    assert Z.check_fwd(emulate_fwd(e), e, "clean exact") == 0.0
    assert (e.jstar == e.N - 1).any()
    with pytest.raises(AssertionError):
        Z.check_fwd(emulate_fwd(e, "skip_partial"), e)
    with pytest.raises(AssertionError):
        Z.check_fwd(emulate_fwd(e, "drop", int(e.jstar[0])), e)
    # ... and in float mode on normalised rows, where the last column carries 1 / N of every sum
    n = next(c for c in Z.float_cases() if c.kind.startswith("norm") and c.N in (33, 65) and c.B >= 31)
    assert Z.check_fwd(emulate_fwd(n), n, "clean normalised") <= 1.0
    with pytest.raises(AssertionError):
        Z.check_fwd(emulate_fwd(n, "skip_partial"), n)
    # backward: float64 of the formulas passes, a dropped column or a doubled scale does not
    dq, bq, dk, bk = Z.backward_bounds(n)
    assert Z.check_bwd(dq.astype(np.float32), dk.astype(np.float32), n, "clean bwd") <= 1.0
    with pytest.raises(AssertionError):
        Z.check_bwd((2 * dq).astype(np.float32), dk.astype(np.float32), n)
    dk2 = dk.copy()
    dk2[n.N - 1] = 0.0
    with pytest.raises(AssertionError):
        Z.check_bwd(dq.astype(np.float32), dk2.astype(np.float32), n)
