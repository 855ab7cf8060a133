"""GPU: MVGAE with `fused_recon: True` (hip_ops.hardest_negative_loss, csrc/hardest_neg.hip) on the reference's golden step --
tests/golden/mvgae.npz: weights, batch, the 12 dropout masks and 4 noise tables replayed in call order -- alone and together with
`fused_posterior` / `fused_heads`, at the tolerances of tests/test_models_gpu.py::test_mvgae_model; the kernels are really taken
(library calls counted, with their B and L) and the torch composition is not; three optimiser steps stay finite and a full
evaluation runs with fused and dense metrics equal; with the key absent the new entry points are never called."""
import numpy as np
import pytest
import torch

from tests.test_models_gpu import _golden, build, close, eval_topk, load, same_metrics

pytestmark = pytest.mark.gpu

ENTRY_POINTS = ("mmrec_hardest_neg_fwd_f32", "mmrec_hardest_neg_bwd_f32")
MVGAE_EXTRA = {"learning_rate": 1e-3, "beta": 0.1, "n_layers": 2}


def _spy(m):
    """count the library calls of the two entry points, with their (B, L)"""
    from mmrec_amd import _lib
    lib = _lib.load()
    calls = {fn: [] for fn in ENTRY_POINTS}
    for fn in ENTRY_POINTS:
        def spy(*a, _real=getattr(lib, fn), _fn=fn):
            calls[_fn].append((a[7], a[2]))
            return _real(*a)
        m.setattr(lib, fn, spy)
    return calls


def _no_composition(m):
    """the composition's pieces: the model's recon_loss, the batched lines of _fused_loss (their bmm) and the op's torch path"""
    import mmrec_amd.models.mvgae as mv
    from mmrec_amd import hip_ops
    fail = lambda *a, **k: pytest.fail("the torch composition ran with the key on")      # noqa: E731
    m.setattr(mv.MVGAE, "recon_loss", fail)
    m.setattr(mv.torch, "bmm", fail)
    m.setattr(hip_ops, "hardest_negative_loss_torch", fail)


@pytest.mark.parametrize("others", [{}, {"fused_posterior": True}, {"fused_posterior": True, "fused_heads": True}, {"fused_heads": True}],
                         ids=["alone", "posterior", "posterior+heads", "heads"])
def test_mvgae_golden_step_with_fused_recon(tmp_path, golden, monkeypatch, others):
    import mmrec_amd.models.mvgae as mv
    g = _golden("mvgae")
    config, _, valid_data, model = build(tmp_path, golden, "MVGAE", dict(MVGAE_EXTRA, fused_recon=True, **others))
    assert model.fused_recon is True and model.graph_capturable is False
    assert model.fused_posterior is bool(others.get("fused_posterior")) and model.fused_heads is bool(others.get("fused_heads"))
    params = dict(model.named_parameters())
    assert set(params) == {k[2:] for k in g if k.startswith("p_")}
    for name, p in params.items():
        load(p, g["p_" + name])
    dev = model.device
    masks = [torch.as_tensor(g["mask_%d" % j].astype(np.float32)).to(dev) for j in range(12)]
    noises = [torch.as_tensor(g["noise_%d" % j]).to(dev) for j in range(4)]
    batch = torch.as_tensor(g["batch1"]).to(dev)
    B = batch.shape[1]
    with monkeypatch.context() as m:
        calls = _spy(m)
        _no_composition(m)
        m.setattr(mv.F, "dropout", lambda x, p=0.5, training=True, inplace=False: x * masks.pop(0) / (1.0 - p) if training else x)
        m.setattr(mv.torch, "randn_like", lambda x, *a, **k: noises.pop(0))
        model.train()
        loss = model.calculate_loss(batch)
        loss.backward()
        torch.cuda.synchronize()
        want = [(B, 4)] if model.fused_posterior else [(B, 1)] * 4       # one stacked call, or one per latent
        assert calls == {fn: want for fn in ENTRY_POINTS}, calls
    assert not masks and not noises
    close(loss, g["loss1"], rtol=2e-5)
    close(model.result_embed, g["result"], rtol=1e-4, atol=2e-6)
    grads = {k[2:] for k in g if k.startswith("g_")}
    assert {name for name, p in params.items() if p.grad is not None} == grads
    for name in grads:
        close(params[name].grad, g["g_" + name], rtol=2e-3, atol=2e-5)
    model.eval()
    users, mask = next(iter(valid_data))
    for _ in valid_data:
        pass
    close(model.full_sort_predict([users, mask]), g["scores_first_batch"], rtol=1e-4, atol=2e-6)


@pytest.mark.parametrize("others", [{}, {"fused_posterior": True, "fused_heads": True}], ids=["alone", "all three"])
def test_three_steps_stay_finite_and_an_evaluation_runs(tmp_path, golden, monkeypatch, others):
    config, train_data, valid_data, model = build(tmp_path, golden, "MVGAE",
                                                  dict(MVGAE_EXTRA, fused_recon=True, train_batch_size=64, **others))
    opt = torch.optim.Adam(model.parameters(), lr=1e-3)
    model.train()
    torch.manual_seed(5)
    model.pre_epoch_processing()
    losses = []
    with monkeypatch.context() as m:
        calls = _spy(m)
        _no_composition(m)
        for step, batch in zip(range(3), train_data):
            opt.zero_grad()
            loss = model.calculate_loss(batch)
            loss.backward()
            opt.step()
            losses.append(float(loss.detach()))
        per_step = 1 if model.fused_posterior else 4
        assert all(len(v) == 3 * per_step for v in calls.values()), calls
        assert {L for v in calls.values() for _, L in v} == {4 if model.fused_posterior else 1}
    print("losses with fused_recon:", losses)
    assert len(losses) == 3 and np.isfinite(losses).all()
    assert all(bool(torch.isfinite(p).all()) for p in model.parameters())
    fused, dense = eval_topk(config, model, valid_data)
    same_metrics(fused, dense)


def test_key_absent_runs_the_composition_and_no_new_entry_point(tmp_path, golden, monkeypatch):
    import mmrec_amd.models.mvgae as mv
    g = _golden("mvgae")
    for extra in ({}, {"fused_recon": False, "fused_posterior": True}):
        config, _, _, model = build(tmp_path / ("p" if extra else "a"), golden, "MVGAE", dict(MVGAE_EXTRA, **extra))
        assert model.fused_recon is False
        seen = []
        real = mv.MVGAE.recon_loss
        with monkeypatch.context() as m:
            calls = _spy(m)
            m.setattr(mv.MVGAE, "recon_loss", lambda self, z, *a: seen.append(tuple(z.shape)) or real(self, z, *a))
            model.train()
            loss = model.calculate_loss(torch.as_tensor(g["batch1"]).to(model.device))
            loss.backward()
            torch.cuda.synchronize()
            assert all(not v for v in calls.values()), calls
        assert seen == ([] if extra else [(model.n_users + model.n_items, 64)] * 4), seen
        assert bool(torch.isfinite(loss))
