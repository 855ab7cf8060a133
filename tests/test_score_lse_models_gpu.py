"""GPU: LGMRec and PGL with `fused_ssl: True` (hip_ops.score_lse, mmrec_score_lse_f32: the contrastive log-sum-exp against a whole
table on the fp32 MFMA) against the default torch path on the tiny golden dataset: one training step from the same seed and the
same batch gives the same loss and parameter gradients within the project's fp32 tolerance (1e-4 relative, README: parity); the
key decides which code runs; with the key on no [B, N] float matrix is produced in the forward; three steps stay finite."""
import numpy as np
import pytest
import torch

from tests.test_models_gpu import build

pytestmark = pytest.mark.gpu

RTOL = 1e-4
EXTRA = {"LGMRec": {"n_ui_layers": 2, "n_mm_layers": 2, "n_hyper_layer": 1, "hyper_num": 4, "keep_rate": 0.5, "alpha": 0.3,
                    "cl_weight": 1e-2, "reg_weight": 1e-6},          # the term's weight raised so that the total shows it
         "PGL": {"dropout": 0.2, "reg_weight": 0.1, "mode": "local"}}
ENTRY_POINTS = ("mmrec_score_lse_f32", "mmrec_score_lse_bwd_f32")


def _one_step(tmp_path, golden, monkeypatch, name, fused, batch=None):
    """one loss + backward on the first batch of an epoch -> the batch, the loss, every parameter gradient, the library calls and
    the shapes of every 2-d float matmul result of the forward"""
    from mmrec_amd import _lib
    lib = _lib.load()
    calls = {fn: 0 for fn in ENTRY_POINTS}
    products = []
    phase = ["fwd"]
    with monkeypatch.context() as m:
        for fn in ENTRY_POINTS:
            def spy(*a, _real=getattr(lib, fn), _fn=fn):
                calls[_fn] += 1
                return _real(*a)
            m.setattr(lib, fn, spy)
        config, train_data, _, model = build(tmp_path, golden, name, dict(EXTRA[name], fused_ssl=fused))
        assert model.fused_ssl is fused
        if batch is None:
            batch = next(iter(train_data)).clone()
        model.train()
        torch.manual_seed(77)
        model.pre_epoch_processing()
        for fn in ("matmul", "mm"):
            def keep(*a, _real=getattr(torch, fn), **k):
                out = _real(*a, **k)
                if phase[0] == "fwd" and out.dim() == 2 and out.is_floating_point():
                    products.append(tuple(out.shape))
                return out
            m.setattr(torch, fn, keep)
        loss = model.calculate_loss(batch.clone())
        phase[0] = "bwd"
        loss.backward()
        torch.cuda.synchronize()
        grads = {n: (None if p.grad is None else p.grad.detach().clone()) for n, p in model.named_parameters()}
    return batch, float(loss.detach()), grads, calls, products, model


def _tables(name, model, batch):
    """the [B, N] shapes the contrastive term of `name` scores"""
    b = batch.shape[1]
    return {(b, model.n_users), (b, model.n_items)} if name == "LGMRec" else {(b, b)}


@pytest.mark.parametrize("name", ["LGMRec", "PGL"])
def test_one_step_fused_equals_the_torch_term(tmp_path, golden, monkeypatch, name):
    batch, loss_on, g_on, calls_on, prod_on, model = _one_step(tmp_path / "on", golden, monkeypatch, name, True)
    _, loss_off, g_off, calls_off, prod_off, _ = _one_step(tmp_path / "off", golden, monkeypatch, name, False, batch)
    print("%s: loss fused %.9g torch %.9g; calls fused %s torch %s" % (name, loss_on, loss_off, calls_on, calls_off))
    # the key decides which code runs: two terms per step
    assert calls_on == {"mmrec_score_lse_f32": 2, "mmrec_score_lse_bwd_f32": 2}, calls_on
    assert calls_off == {"mmrec_score_lse_f32": 0, "mmrec_score_lse_bwd_f32": 0}, calls_off
    # no [B, N] matrix in the fused forward; the torch path produces exactly those
    tables = _tables(name, model, batch)
    assert not tables & set(prod_on), (tables, prod_on)
    assert tables <= set(prod_off), (tables, prod_off)
    assert np.isfinite(loss_on) and abs(loss_on - loss_off) <= RTOL * abs(loss_off), (loss_on, loss_off)
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
        moved += diff > 0
    assert moved >= 1                                                # the gradient really passed another code path


@pytest.mark.parametrize("name", ["LGMRec", "PGL"])
def test_three_steps_with_the_key_on_stay_finite(tmp_path, golden, name):
    config, train_data, _, model = build(tmp_path, golden, name, dict(EXTRA[name], fused_ssl=True, train_batch_size=64))
    opt = torch.optim.Adam(model.parameters(), lr=1e-3)
    model.train()
    torch.manual_seed(5)
    model.pre_epoch_processing()
    losses = []
    for step, batch in zip(range(3), train_data):
        opt.zero_grad()
        loss = model.calculate_loss(batch)
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    print(name, "losses with fused_ssl:", losses)
    assert len(losses) == 3 and np.isfinite(losses).all()
    assert all(bool(torch.isfinite(p).all()) for p in model.parameters())
