"""CPU: the fused edge attention (mmrec_edge_attention_f32, hip_ops.edge_attention) without a GPU -- the exports, what the
wrapper serves, the three-op composition that everything else (here: CPU tensors) takes bit for bit, forward and gradients, and
GRCN's `fused_attention` key, which on the CPU is that composition either way.  (The argument checks of the C entry point, the
fp32 emulation of the kernel's plan and the checker's own tests are in tests/test_edge_attention_fuzz_gpu.py, without the gpu
mark.)"""
import os
import types

import numpy as np
import pytest
import torch

import tests.test_models_gpu as G
from mmrec_amd import _lib
from tests._cpu_ops import cpu_ops  # noqa: F401  (fixture)

EXPORTS = ("mmrec_edge_attention_group_max", "mmrec_edge_attention_f32")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        from mmrec_amd.build import build
        build(verbose=False)
    return _lib.load()


def test_exports_in_header_signatures_and_library(lib):
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mmrec_hip.h")).read()
    for name in EXPORTS:
        assert name in _lib.SIGNATURES and name in src and hasattr(lib, name), name
    assert "#define MMREC_ABI_VERSION 16" in src and lib.mmrec_abi_version() == 16       # additive: the version stays
    # one long-row list per DynGraph serves the softmax and the attention
    assert lib.mmrec_edge_attention_group_max() == lib.mmrec_segment_softmax_group_max()


@pytest.fixture
def deterministic_torch():
    """torch's own CPU backward of a gather adds with several threads in arrival order: the same function run twice differs in
    the last ulp of a gradient.  Bit-for-bit comparisons of gradients run in torch's deterministic mode."""
    was = torch.are_deterministic_algorithms_enabled()
    torch.use_deterministic_algorithms(True)
    yield
    torch.use_deterministic_algorithms(was)


def _graph(rng, n_rows, n_cols, ne):
    rows = torch.from_numpy(rng.integers(0, n_rows, ne))
    cols = torch.from_numpy(rng.integers(0, n_cols, ne))
    return types.SimpleNamespace(rows=rows, cols=cols, n_rows=n_rows, n_cols=n_cols)


def _three_ops(hip_ops, Q, KV, dyn, eps=1e-16):
    score = hip_ops.edge_dot(Q, KV, dyn.rows, dyn.cols, dyn=dyn)
    alpha = hip_ops.edge_softmax(score, dyn, eps=eps)
    return hip_ops.spmm_vals(dyn, KV, alpha), alpha


@pytest.mark.parametrize("same", [False, True], ids=["distinct", "Q_is_KV"])
def test_cpu_tensors_take_the_three_ops_bit_for_bit(cpu_ops, deterministic_torch, same):  # noqa: F811
    from mmrec_amd import hip_ops
    assert hip_ops.EDGE_ATTENTION is True
    rng = np.random.default_rng(11)
    n = 40
    dyn = _graph(rng, n, n, 700)
    dY = torch.from_numpy(rng.standard_normal((n, 64)).astype(np.float32))
    dA = torch.from_numpy(rng.standard_normal(700).astype(np.float32))
    runs = []
    for fn in (hip_ops.edge_attention, lambda Q, KV, d: _three_ops(hip_ops, Q, KV, d)):
        Q = torch.from_numpy((np.random.default_rng(2).standard_normal((n, 64)) * 0.5).astype(np.float32)).requires_grad_()
        KV = Q if same else torch.from_numpy((np.random.default_rng(3).standard_normal((n, 64)) * 0.5).astype(np.float32)).requires_grad_()
        assert not hip_ops.edge_attention_served(Q, KV, dyn)
        Y, alpha = fn(Q, KV, dyn)
        assert Y.shape == (n, 64) and alpha.shape == (700,) and Y.dtype == alpha.dtype == torch.float32
        ((Y * dY).sum() + (alpha * dA).sum()).backward()
        runs.append((Y.detach(), alpha.detach(), Q.grad, KV.grad))
    for a, b in zip(*runs):
        assert torch.equal(a, b)
    assert float(runs[0][2].abs().max()) > 0
    # and it IS the formulas: float64
    Y, alpha = runs[0][0].double(), runs[0][1].double()
    Q64, KV64 = Q.detach().double(), KV.detach().double()
    s = (Q64[dyn.rows] * KV64[dyn.cols]).sum(-1)
    ref = hip_ops.segment_softmax_torch(s, dyn.rows, n)
    assert float((alpha - ref).abs().max()) <= 1e-6
    want = torch.zeros(n, 64, dtype=torch.float64).index_add_(0, dyn.rows, ref.unsqueeze(1) * KV64[dyn.cols])
    assert float((Y - want).abs().max()) <= 1e-5


def test_served_is_about_device_dtype_shape_lengths_and_the_switch(monkeypatch):
    from mmrec_amd import hip_ops
    dyn = _graph(np.random.default_rng(1), 6, 9, 12)

    class OnDevice(torch.Tensor):                                    # a stand-in that says it lives on the device
        is_cuda = True
    dev = lambda t: t.as_subclass(OnDevice)                          # noqa: E731
    Q, KV = torch.zeros(6, 64), torch.zeros(9, 64)
    assert not hip_ops.edge_attention_served(Q, KV, dyn)              # CPU tensors: never
    assert not hip_ops.edge_attention_served(dev(Q), KV, dyn) and not hip_ops.edge_attention_served(Q, dev(KV), dyn)
    assert hip_ops.edge_attention_served(dev(Q), dev(KV), dyn)
    for bad_q, bad_kv in ((torch.zeros(6, 32), torch.zeros(9, 32)),                          # another width
                          (torch.zeros(6, 128), torch.zeros(9, 128)),
                          (torch.zeros(6, 64, dtype=torch.float64), KV), (Q, torch.zeros(9, 64, dtype=torch.float16)),   # dtype
                          (torch.zeros(6, 128)[:, ::2], KV), (Q, torch.zeros(18, 64)[::2]),  # not contiguous
                          (torch.zeros(7, 64), KV), (torch.zeros(5, 64), KV), (Q, torch.zeros(8, 64)), (Q, torch.zeros(10, 64)),   # lengths
                          (torch.zeros(6 * 64), KV), (None, KV), (Q, None)):
        q = dev(bad_q) if isinstance(bad_q, torch.Tensor) else bad_q
        kv = dev(bad_kv) if isinstance(bad_kv, torch.Tensor) else bad_kv
        assert not hip_ops.edge_attention_served(q, kv, dyn), (getattr(bad_q, "shape", None), getattr(bad_kv, "shape", None))
    sq = _graph(np.random.default_rng(1), 6, 6, 12)
    X = dev(torch.zeros(6, 64))
    assert hip_ops.edge_attention_served(X, X, sq)                    # Q is KV
    monkeypatch.setattr(hip_ops, "EDGE_ATTENTION", False)
    assert not hip_ops.edge_attention_served(X, X, sq) and not hip_ops.edge_attention_served(dev(Q), dev(KV), dyn)


def _grcn_step(tmp_path, golden, fused):
    extra = {"reg_weight": 1e-3, "learning_rate": 1e-3, "n_layers": 3}
    if fused is not None:
        extra["fused_attention"] = fused
    config, train_data, _, model = G.build(tmp_path, golden, "GRCN", extra)
    assert model.v_gcn.fused_attention is bool(fused) and model.t_gcn.fused_attention is bool(fused)
    batch = next(iter(train_data)).clone()
    model.train()
    model.pre_epoch_processing()
    torch.manual_seed(77)
    loss = model.calculate_loss(batch)
    loss.backward()
    return loss.detach(), {n: p.grad.detach().clone() for n, p in model.named_parameters() if p.grad is not None}


def test_grcn_fused_attention_key_on_the_cpu_is_the_composition(tmp_path, golden, cpu_ops, deterministic_torch, monkeypatch):  # noqa: F811
    """GRCN on the tiny golden dataset with `fused_attention` absent, False and True: on the CPU all three are the three ops --
    the same loss and the same gradients, bit for bit -- and the key decides whether `hip_ops.edge_attention` is asked"""
    from mmrec_amd import hip_ops
    monkeypatch.setattr(G, "USE_GPU", False)
    asked = []
    real = hip_ops.edge_attention
    monkeypatch.setattr(hip_ops, "edge_attention", lambda *a, **k: asked.append(1) or real(*a, **k))
    loss0, g0 = _grcn_step(tmp_path / "absent", golden, None)
    loss1, g1 = _grcn_step(tmp_path / "off", golden, False)
    assert not asked
    loss2, g2 = _grcn_step(tmp_path / "on", golden, True)
    assert len(asked) == 2                                            # the image and the text content GCN
    assert torch.equal(loss0, loss1) and torch.equal(loss1, loss2) and np.isfinite(float(loss2))
    assert set(g0) == set(g1) == set(g2) and len(g2) >= 6
    for n in g1:
        assert torch.equal(g0[n], g1[n]) and torch.equal(g1[n], g2[n]), n
    for n in ("v_gcn.preference", "t_gcn.preference", "v_gcn.MLP.weight"):
        assert float(g2[n].abs().max()) > 0, n
