"""GPU: GRCN with `fused_attention` + `fused_attention_backward` (the attention's backward as ONE call, mmrec_edge_attention_bwd_f32)
against `fused_attention` alone (the backward composed of the older kernels) on the tiny golden dataset: one training step from
the same seed gives the same loss and every parameter's gradient within the project's fp32 tolerance; the key decides which
backward runs; under `hip_deterministic` every gradient repeats bit for bit; and an epoch replayed as a hipGraph with both keys on
gives the eager losses -- the backward does no host work after the first forward."""
import numpy as np
import pytest
import torch

from tests.test_edge_attention_models_gpu import EXTRA, RTOL
from tests.test_models_gpu import build

pytestmark = pytest.mark.gpu

BACKWARD = ("mmrec_edge_attention_bwd_f32", "mmrec_edge_dot_f32", "mmrec_segment_softmax_bwd_f32")


def _one_step(tmp_path, golden, monkeypatch, fused_backward, batch=None):
    """one loss + backward on the first batch of an epoch -> the batch, the loss, every parameter gradient and the library calls
    of the BACKWARD"""
    from mmrec_amd import _lib
    lib = _lib.load()
    calls = {fn: 0 for fn in BACKWARD + ("mmrec_edge_attention_f32",)}
    phase = ["fwd"]
    with monkeypatch.context() as m:
        for fn in calls:
            def spy(*a, _real=getattr(lib, fn), _fn=fn):
                if phase[0] == "bwd" or _fn == "mmrec_edge_attention_f32":
                    calls[_fn] += 1
                return _real(*a)
            m.setattr(lib, fn, spy)
        extra = dict(EXTRA, fused_attention=True)
        if fused_backward is not None:
            extra["fused_attention_backward"] = fused_backward
        config, train_data, _, model = build(tmp_path, golden, "GRCN", extra)
        assert model.v_gcn.fused_attention and model.t_gcn.fused_attention
        assert model.v_gcn.fused_attention_backward is bool(fused_backward)
        assert model.t_gcn.fused_attention_backward is bool(fused_backward)
        if batch is None:
            batch = next(iter(train_data)).clone()
        model.train()
        model.pre_epoch_processing()
        torch.manual_seed(77)
        loss = model.calculate_loss(batch.clone())
        phase[0] = "bwd"
        loss.backward()
        torch.cuda.synchronize()
        grads = {n: (None if p.grad is None else p.grad.detach().clone()) for n, p in model.named_parameters()}
    return batch, float(loss.detach()), grads, calls


def test_one_step_fused_backward_equals_the_composed_one(tmp_path, golden, monkeypatch):
    batch, loss_on, g_on, calls_on = _one_step(tmp_path / "on", golden, monkeypatch, True)
    _, loss_off, g_off, calls_off = _one_step(tmp_path / "off", golden, monkeypatch, None, batch)
    print("GRCN: loss %.9g / %.9g; calls with the key %s, without %s" % (loss_on, loss_off, calls_on, calls_off))
    # the key decides which backward runs: one call per modality, none of the composed ones
    assert calls_on["mmrec_edge_attention_f32"] == 2 and calls_off["mmrec_edge_attention_f32"] == 2
    assert calls_on["mmrec_edge_attention_bwd_f32"] == 2, calls_on
    assert calls_on["mmrec_segment_softmax_bwd_f32"] == 0, calls_on
    assert calls_off["mmrec_edge_attention_bwd_f32"] == 0 and calls_off["mmrec_segment_softmax_bwd_f32"] == 2, calls_off
    # (the id GCN's two value gradients are per-edge dots in both runs; the composed backward adds one per modality)
    assert calls_off["mmrec_edge_dot_f32"] == calls_on["mmrec_edge_dot_f32"] + 2, (calls_on, calls_off)
    assert abs(loss_on - loss_off) <= RTOL * abs(loss_off), (loss_on, loss_off)      # (the forward is the same code)
    assert set(g_on) == set(g_off)
    moved = 0
    for n in sorted(g_on):
        a, b = g_on[n], g_off[n]
        assert (a is None) == (b is None), n
        if a is None:
            continue
        a, b = a.cpu().double().numpy(), b.cpu().double().numpy()
        scale = float(np.abs(b).max())
        diff = float(np.abs(a - b).max())
        print("  %-32s |grad| max %.3e  max diff %.3e  ratio %.3e" % (n, scale, diff, diff / scale if scale else 0.0))
        assert np.isfinite(a).all() and diff <= RTOL * scale, (n, diff, scale)
        moved += scale > 0
    assert moved >= 4
    for n in ("v_gcn.preference", "t_gcn.preference", "v_gcn.MLP.weight"):       # the gradient passes the fused backward
        assert float(g_on[n].abs().max()) > 0, n


def test_fused_backward_repeats_bit_for_bit_when_deterministic(tmp_path, golden, monkeypatch):
    """`hip_deterministic` (the fused loss' scatters without atomics): two same-seed steps repeat every gradient bit for bit"""
    from mmrec_amd import hip_ops
    try:
        hip_ops.set_deterministic(True)
        batch, _, d1, calls = _one_step(tmp_path / "a", golden, monkeypatch, True)
        _, _, d2, _ = _one_step(tmp_path / "b", golden, monkeypatch, True, batch)
    finally:
        hip_ops.set_deterministic(hip_ops.DETERMINISTIC_DEFAULT)
    assert calls["mmrec_edge_attention_bwd_f32"] == 2, calls          # still the kernel
    assert float(d1["v_gcn.preference"].abs().max()) > 0
    for n in sorted(d1):
        if d1[n] is not None:
            assert torch.equal(d1[n].view(torch.int32), d2[n].view(torch.int32)), n


def test_replayed_grcn_epoch_with_both_keys_gives_the_eager_losses(tmp_path, golden, monkeypatch):
    """`hip_graph_step`: the epoch as one capture replayed, edge_attention forward and its one-call backward inside it; both long
    lists are built by the eager first batch's FORWARD, so the capture meets no host work in the backward and does not fail"""
    from mmrec_amd import _lib
    from mmrec_amd.common.trainer import Trainer
    lib = _lib.load()
    calls = [0]
    monkeypatch.setattr(lib, "mmrec_edge_attention_bwd_f32",
                        lambda *a, _real=lib.mmrec_edge_attention_bwd_f32: calls.__setitem__(0, calls[0] + 1) or _real(*a))
    runs = []
    for graphed in (False, True):
        extra = dict(EXTRA, train_batch_size=64, hip_graph_step=graphed, fused_attention=True, fused_attention_backward=True)
        config, train_data, _, model = build(tmp_path / str(graphed), golden, "GRCN", extra)
        config["hip_graph_step"] = graphed
        torch.manual_seed(123)
        trainer = Trainer(config, model)
        model.pre_epoch_processing()
        total, losses = trainer._train_epoch(train_data, 0)
        step = trainer._graphed_step(model.calculate_loss)
        assert (step is not None) == graphed
        if graphed:
            assert not step.failed and step.graph is not None
        runs.append((total, torch.stack([x.reshape(()) for x in losses]).cpu().numpy()))
    (t0, l0), (t1, l1) = runs
    assert calls[0] >= 2 * l0.size + 4                                # the eager epoch + the graphed one's eager batch and capture
    assert l0.size >= 3 and l0.size == l1.size
    print("eager", l0, "graphed", l1)
    np.testing.assert_allclose(l1, l0, rtol=1e-5)
    np.testing.assert_allclose(t1, t0, rtol=1e-5)
