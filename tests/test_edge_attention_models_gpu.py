"""GPU: GRCN with `fused_attention: True` (hip_ops.edge_attention, mmrec_edge_attention_f32: scores, softmax and aggregation of a
content GCN in one kernel) against the default three ops on the tiny golden dataset: one training step from the same seed gives
the same loss, attention weights and parameter gradients within the project's fp32 tolerance (1e-4 relative, README: parity);
the key decides which code runs; the fused path's attention weights and aggregate repeat bit for bit; and a GRCN epoch
replayed as a hipGraph with the key on gives the eager losses."""
import numpy as np
import pytest
import torch

from tests.test_models_gpu import build

pytestmark = pytest.mark.gpu

EXTRA = {"reg_weight": 1e-3, "learning_rate": 1e-3, "n_layers": 3}
RTOL = 1e-4
ENTRY_POINTS = ("mmrec_edge_attention_f32", "mmrec_segment_softmax_f32", "mmrec_segment_softmax_bwd_f32", "mmrec_edge_dot_f32")


def _one_step(tmp_path, golden, monkeypatch, fused, batch=None):
    """one loss + backward on the first batch of an epoch -> the batch, the loss, every parameter gradient, both modalities'
    attention weights (and the fused op's aggregates), the library calls of the forward, and the [n_edges, 64] gathers seen in
    the forward"""
    from mmrec_amd import _lib, hip_ops
    lib = _lib.load()
    calls = {fn: 0 for fn in ENTRY_POINTS}
    calls["gathers_fwd"] = 0
    alphas, aggs = [], []
    phase = ["fwd"]
    with monkeypatch.context() as m:
        for fn in ENTRY_POINTS:
            def spy(*a, _real=getattr(lib, fn), _fn=fn):
                if phase[0] == "fwd":
                    calls[_fn] += 1
                return _real(*a)
            m.setattr(lib, fn, spy)
        real_att, real_soft = hip_ops.edge_attention, hip_ops.edge_softmax

        def keep_att(*a, **k):
            y, alpha = real_att(*a, **k)
            aggs.append(y.detach().clone())
            alphas.append(alpha.detach().clone())
            return y, alpha

        def keep_soft(*a, **k):
            out = real_soft(*a, **k)
            alphas.append(out.detach().clone())
            return out
        m.setattr(hip_ops, "edge_attention", keep_att)
        m.setattr(hip_ops, "edge_softmax", keep_soft)
        config, train_data, _, model = build(tmp_path, golden, "GRCN", dict(EXTRA, fused_attention=fused))
        assert model.v_gcn.fused_attention is fused and model.t_gcn.fused_attention is fused
        if batch is None:
            batch = next(iter(train_data)).clone()
        model.train()
        model.pre_epoch_processing()
        n_edges = model.edges.dst.numel()
        real_gi = torch.Tensor.__getitem__

        def getitem(self, idx):
            out = real_gi(self, idx)
            if (phase[0] == "fwd" and isinstance(idx, torch.Tensor) and idx.dim() == 1 and self.dim() == 2 and
                    self.is_floating_point() and self.shape[1] == 64 and idx.numel() == n_edges):
                calls["gathers_fwd"] += 1
            return out
        m.setattr(torch.Tensor, "__getitem__", getitem)
        torch.manual_seed(77)
        loss = model.calculate_loss(batch.clone())
        phase[0] = "bwd"
        loss.backward()
        torch.cuda.synchronize()
        grads = {n: (None if p.grad is None else p.grad.detach().clone()) for n, p in model.named_parameters()}
    return batch, float(loss), grads, alphas, aggs, calls


def test_one_step_fused_equals_the_three_ops(tmp_path, golden, monkeypatch):
    batch, loss_on, g_on, a_on, y_on, calls_on = _one_step(tmp_path / "on", golden, monkeypatch, True)
    _, loss_off, g_off, a_off, _, calls_off = _one_step(tmp_path / "off", golden, monkeypatch, False, batch)
    print("GRCN: loss fused %.9g three ops %.9g; forward calls fused %s three ops %s" % (loss_on, loss_off, calls_on, calls_off))
    # the key decides which code runs: the image and the text content GCN
    assert calls_on["mmrec_edge_attention_f32"] == 2 and calls_on["mmrec_segment_softmax_f32"] == 0, calls_on
    assert calls_on["mmrec_edge_dot_f32"] == 0 and calls_on["gathers_fwd"] == 0, calls_on
    assert calls_off["mmrec_edge_attention_f32"] == 0 and calls_off["mmrec_segment_softmax_f32"] == 2, calls_off
    assert calls_off["mmrec_edge_dot_f32"] == 2, calls_off
    assert len(a_on) == 2 and len(a_off) == 2 and len(y_on) == 2
    for x, y in zip(a_on, a_off):
        np.testing.assert_allclose(x.cpu().numpy(), y.cpu().numpy(), rtol=RTOL, atol=1e-7)
        assert float(x.sum()) > 1.0
    assert abs(loss_on - loss_off) <= RTOL * abs(loss_off), (loss_on, loss_off)
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
    for n in ("v_gcn.preference", "t_gcn.preference", "v_gcn.MLP.weight"):       # the gradient passes the fused op
        assert float(g_on[n].abs().max()) > 0, n


def test_fused_path_repeats_bit_for_bit(tmp_path, golden, monkeypatch):
    """the key on, two runs from the same seed: the same attention weights and aggregates, bit for bit (forward results; the
    gradients of the step add the fused loss' atomic scatters unless `hip_deterministic` is set, as
    tests/test_edge_softmax_models_gpu.py explains -- in that mode every gradient repeats too)"""
    from mmrec_amd import hip_ops
    batch, _, _, a1, y1, _ = _one_step(tmp_path / "a", golden, monkeypatch, True)
    _, _, _, a2, y2, _ = _one_step(tmp_path / "b", golden, monkeypatch, True, batch)
    for x, y in zip(a1 + y1, a2 + y2):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32))
    try:
        hip_ops.set_deterministic(True)
        _, _, d1, b1, z1, calls = _one_step(tmp_path / "c", golden, monkeypatch, True, batch)
        _, _, d2, b2, z2, _ = _one_step(tmp_path / "d", golden, monkeypatch, True, batch)
    finally:
        hip_ops.set_deterministic(hip_ops.DETERMINISTIC_DEFAULT)
    assert calls["mmrec_edge_attention_f32"] == 2, calls              # still the kernel
    for x, y, z in zip(b1 + z1, b2 + z2, a1 + y1):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32)) and torch.equal(x.view(torch.int32), z.view(torch.int32))
    assert float(d1["v_gcn.preference"].abs().max()) > 0
    for n in sorted(d1):
        if d1[n] is not None:
            assert torch.equal(d1[n].view(torch.int32), d2[n].view(torch.int32)), n


def test_replayed_grcn_epoch_with_the_key_on_gives_the_eager_losses(tmp_path, golden, monkeypatch):
    """`hip_graph_step`: the epoch as one capture replayed (edge_attention forward and its composed backward inside it; the
    long-row list is built by the eager first batch) -- the per-batch losses are the eager epoch's"""
    from mmrec_amd import _lib
    from mmrec_amd.common.trainer import Trainer
    lib = _lib.load()
    calls = [0]
    monkeypatch.setattr(lib, "mmrec_edge_attention_f32",
                        lambda *a, _real=lib.mmrec_edge_attention_f32: calls.__setitem__(0, calls[0] + 1) or _real(*a))
    runs = []
    for graphed in (False, True):
        extra = dict(EXTRA, train_batch_size=64, hip_graph_step=graphed, fused_attention=True)
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
