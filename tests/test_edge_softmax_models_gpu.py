"""GPU: GRCN with the attention softmax on the segment-softmax kernels (hip_ops.edge_softmax, mmrec_segment_softmax_f32 /
_bwd_f32) and with `hip_ops.EDGE_SOFTMAX` off (the scatter / gather composition), on the tiny golden dataset: one training step
from the same seed gives the same loss and parameter gradients within the project's fp32 tolerance (1e-4 relative, README:
parity), the switch decides which code runs, the kernel path's attention weights and their gradient repeat bit for bit, and a
GRCN epoch replayed as a hipGraph gives the eager losses."""
import numpy as np
import pytest
import torch

from tests.test_models_gpu import build

pytestmark = pytest.mark.gpu

EXTRA = {"reg_weight": 1e-3, "learning_rate": 1e-3, "n_layers": 3}
RTOL = 1e-4
ENTRY_POINTS = ("mmrec_segment_softmax_f32", "mmrec_segment_softmax_bwd_f32")


def _one_step(tmp_path, golden, monkeypatch, on, batch=None):
    """one loss + backward on the first batch of an epoch -> the batch, the loss, every parameter gradient, both modalities'
    attention weights and the library calls of the softmax entry points"""
    from mmrec_amd import _lib, hip_ops
    lib = _lib.load()
    calls = {fn: 0 for fn in ENTRY_POINTS}
    alphas = []
    with monkeypatch.context() as m:
        m.setattr(hip_ops, "EDGE_SOFTMAX", on)
        for fn in ENTRY_POINTS:
            def spy(*a, _real=getattr(lib, fn), _fn=fn):
                calls[_fn] += 1
                return _real(*a)
            m.setattr(lib, fn, spy)
        real = hip_ops.edge_softmax

        def keep(*a, **k):
            out = real(*a, **k)
            alphas.append(out.detach().clone())
            return out
        m.setattr(hip_ops, "edge_softmax", keep)
        config, train_data, _, model = build(tmp_path, golden, "GRCN", EXTRA)
        if batch is None:
            batch = next(iter(train_data)).clone()
        model.train()
        model.pre_epoch_processing()
        torch.manual_seed(77)
        loss = model.calculate_loss(batch.clone())
        loss.backward()
        torch.cuda.synchronize()
        grads = {n: (None if p.grad is None else p.grad.detach().clone()) for n, p in model.named_parameters()}
    return batch, float(loss), grads, alphas, calls


def test_one_step_with_the_kernel_equals_the_composition(tmp_path, golden, monkeypatch):
    batch, loss_on, g_on, a_on, calls_on = _one_step(tmp_path / "on", golden, monkeypatch, True)
    _, loss_off, g_off, a_off, calls_off = _one_step(tmp_path / "off", golden, monkeypatch, False, batch)
    print("GRCN: loss on %.9g off %.9g; calls on %s off %s" % (loss_on, loss_off, calls_on, calls_off))
    # the switch decides which code runs: the image and the text content GCN, forward and backward
    assert calls_on == {"mmrec_segment_softmax_f32": 2, "mmrec_segment_softmax_bwd_f32": 2}, calls_on
    assert calls_off == {"mmrec_segment_softmax_f32": 0, "mmrec_segment_softmax_bwd_f32": 0}, calls_off
    assert len(a_on) == 2 and len(a_off) == 2
    for x, y in zip(a_on, a_off):
        np.testing.assert_allclose(x.cpu().numpy(), y.cpu().numpy(), rtol=RTOL, atol=1e-7)
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
    for n in ("v_gcn.preference", "t_gcn.preference", "v_gcn.MLP.weight"):       # the scores' gradient passes the softmax
        assert float(g_on[n].abs().max()) > 0, n


def _differing(x, y):
    return int((x.view(torch.int32) != y.view(torch.int32)).sum())


def test_kernel_path_repeats_bit_for_bit(tmp_path, golden, monkeypatch):
    """the switch on, two runs from the same seed: the same attention weights and the same gradient of the image GCN's user
    preferences, bit for bit.
    The attention weights are a forward result and repeat in every mode.  The gradient of `v_gcn.preference` is the sum of what
    comes back through the softmax and of two scatters over the batch's user ids -- the fused BPR loss' backward and the
    regulariser's gather-norm backward -- which add with fp32 atomics unless `hip_deterministic` is set (hip_ops.DETERMINISTIC:
    "a batch with duplicated ids is order-dependent in the last ulp"); the golden batch names users more than once.  Gradient
    bits are therefore promised, and asserted here, in the mode the project promises them in; the default mode's figures are
    printed, not asserted."""
    from mmrec_amd import hip_ops
    batch, _, g1, a1, _ = _one_step(tmp_path / "a", golden, monkeypatch, True)
    _, _, g2, a2, _ = _one_step(tmp_path / "b", golden, monkeypatch, True, batch)
    for x, y in zip(a1, a2):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32))
    x, y = g1["v_gcn.preference"], g2["v_gcn.preference"]
    print("default mode: v_gcn.preference.grad differs in %d of %d elements, max |diff| %.3e, max |grad| %.3e" % (
        _differing(x, y), x.numel(), float((x - y).abs().max()), float(x.abs().max())))
    try:
        hip_ops.set_deterministic(True)
        _, _, d1, b1, calls = _one_step(tmp_path / "c", golden, monkeypatch, True, batch)
        _, _, d2, b2, _ = _one_step(tmp_path / "d", golden, monkeypatch, True, batch)
    finally:
        hip_ops.set_deterministic(hip_ops.DETERMINISTIC_DEFAULT)
    assert calls == {"mmrec_segment_softmax_f32": 2, "mmrec_segment_softmax_bwd_f32": 2}, calls      # still the kernels
    for x, y, z in zip(b1, b2, a1):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32)) and torch.equal(x.view(torch.int32), z.view(torch.int32))
    x, y = d1["v_gcn.preference"], d2["v_gcn.preference"]
    assert float(x.abs().max()) > 0
    assert torch.equal(x.view(torch.int32), y.view(torch.int32)), _differing(x, y)
    for n in sorted(d1):                                              # and every other gradient of the step
        if d1[n] is not None:
            assert torch.equal(d1[n].view(torch.int32), d2[n].view(torch.int32)), (n, _differing(d1[n], d2[n]))


def test_replayed_grcn_epoch_gives_the_eager_losses(tmp_path, golden):
    """`hip_graph_step`: the epoch as one capture replayed (edge_softmax forward and backward inside it) -- the per-batch losses
    are the eager epoch's"""
    from mmrec_amd.common.trainer import Trainer
    runs = []
    for graphed in (False, True):
        extra = dict(EXTRA, train_batch_size=64, hip_graph_step=graphed)
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
    assert l0.size >= 3 and l0.size == l1.size                        # the eager first batch + two or more replayed ones
    print("eager", l0, "graphed", l1)
    np.testing.assert_allclose(l1, l0, rtol=1e-5)
    np.testing.assert_allclose(t1, t0, rtol=1e-5)
