"""GPU: LGMRec with `fused_hyper: True` (hip_ops.hyper_assign / hyper_propagate, csrc/hypergraph.hip) on the reference's golden
step -- tests/golden/lgmrec.npz: weights, batch, Gumbel noise (`gumbel_0..3`) and dropout masks (`drop_mask_0..3`) replayed through
`_hyper_noise` / `_hyper_keep` -- at the tolerances of tests/test_models_gpu.py::test_lgmrec_model, alone and together with
`fused_ssl`; the kernels are really taken (library calls counted); with the model's own draws the loss is finite and a full
evaluation runs; with the key absent the model calls F.gumbel_softmax and F.dropout four times each in today's order."""
import os

import numpy as np
import pytest
import torch

from tests.test_hyper_cpu import LGM_EXTRA, replay_draws
from tests.test_models_gpu import build, close, eval_topk, load

pytestmark = pytest.mark.gpu

ENTRY_POINTS = ("mmrec_hyper_assign_fwd_f32", "mmrec_hyper_assign_bwd_f32", "mmrec_hyper_layer_fwd_f32", "mmrec_hyper_layer_bwd_f32")


def _golden():
    return dict(np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lgmrec.npz")))


def _spy(m):
    """count the library calls of the four entry points, with (n, H) of the assignments and (I, U, H) of the layers"""
    from mmrec_amd import _lib
    lib = _lib.load()
    calls = {fn: [] for fn in ENTRY_POINTS}
    for fn in ENTRY_POINTS:
        def spy(*a, _real=getattr(lib, fn), _fn=fn):
            calls[_fn].append(tuple(a[3:5]) if "assign" in _fn else tuple(a[6:9]) if "bwd" in _fn else tuple(a[3:6]))
            return _real(*a)
        m.setattr(lib, fn, spy)
    return calls


@pytest.mark.parametrize("ssl", [False, True], ids=["alone", "with_fused_ssl"])
def test_lgmrec_golden_step_with_fused_hyper(tmp_path, golden, monkeypatch, ssl):
    lgm = _golden()
    config, _, valid_data, model = build(tmp_path, golden, "LGMRec", dict(LGM_EXTRA, fused_hyper=True, fused_ssl=ssl))
    assert model.fused_hyper is True and model.fused_ssl is ssl
    params = dict(model.named_parameters())
    assert set(params) == {k[2:] for k in lgm if k.startswith("p_")}
    for name, p in params.items():
        load(p, lgm["p_" + name])
    dev = model.device
    nI, nU, H = model.n_items, model.n_users, model.hyper_num
    with monkeypatch.context() as m:
        calls = _spy(m)
        queue_n, queue_m = replay_draws(model, lgm, m)
        model.train()
        loss = model.calculate_loss(torch.as_tensor(lgm["batch1"]).to(dev))
        loss.backward()
        torch.cuda.synchronize()
        assert not queue_n and not queue_m
        # the kernels were really taken: iv, uv, it, ut assigned, one layer per modality, and the mirror of each
        assert calls["mmrec_hyper_assign_fwd_f32"] == [(nI, H), (nU, H), (nI, H), (nU, H)], calls
        assert sorted(calls["mmrec_hyper_assign_bwd_f32"]) == sorted([(nI, H), (nU, H)] * 2), calls
        assert calls["mmrec_hyper_layer_fwd_f32"] == [(nI, nU, H)] * 2 and calls["mmrec_hyper_layer_bwd_f32"] == [(nI, nU, H)] * 2, calls
        close(loss, lgm["loss1"], rtol=1e-5)
        for name in ("user_embedding.weight", "item_id_embedding.weight", "item_image_trs", "item_text_trs", "v_hyper", "t_hyper"):
            close(params[name].grad, lgm["g_" + name], rtol=5e-4, atol=1e-8)
        model.eval()
        queue_n.extend(torch.as_tensor(lgm["gumbel_%d" % j]).to(dev) for j in range(4))
        with torch.no_grad():
            u, i, hyper = model.forward()
        assert not queue_n and len(calls["mmrec_hyper_assign_fwd_f32"]) == 8 and len(calls["mmrec_hyper_layer_fwd_f32"]) == 4
        close(u, lgm["user_out"], atol=2e-6), close(i, lgm["item_out"], atol=2e-6)
        close(hyper[0], lgm["uv_hyper"], atol=2e-6), close(hyper[3], lgm["it_hyper"], atol=2e-6)
    # the model's own draws: a finite loss, a full evaluation runs
    model.train()
    torch.manual_seed(5)
    assert torch.isfinite(model.calculate_loss(torch.as_tensor(lgm["batch1"]).to(dev)))
    fused, _ = eval_topk(config, model, valid_data)
    assert 0.0 <= fused["recall@20"] <= 1.0


def test_two_hyper_layers_and_three_steps_stay_finite(tmp_path, golden, monkeypatch):
    """n_hyper_layer = 2: the inner layer asks for no user rows; three optimiser steps with the model's own draws"""
    config, train_data, _, model = build(tmp_path, golden, "LGMRec", dict(LGM_EXTRA, n_hyper_layer=2, fused_hyper=True, fused_ssl=True,
                                                                          train_batch_size=64))
    opt = torch.optim.Adam(model.parameters(), lr=1e-3)
    model.train()
    torch.manual_seed(5)
    model.pre_epoch_processing()
    losses = []
    with monkeypatch.context() as m:
        calls = _spy(m)
        for step, batch in zip(range(3), train_data):
            opt.zero_grad()
            loss = model.calculate_loss(batch)
            loss.backward()
            opt.step()
            losses.append(float(loss.detach()))
        assert len(calls["mmrec_hyper_layer_fwd_f32"]) == 3 * 2 * 2 and len(calls["mmrec_hyper_layer_bwd_f32"]) == 3 * 2 * 2, calls
    print("losses with fused_hyper, two layers:", losses)
    assert len(losses) == 3 and np.isfinite(losses).all()
    assert all(bool(torch.isfinite(p).all()) for p in model.parameters())


def test_key_absent_makes_todays_calls_in_todays_order(tmp_path, golden, monkeypatch):
    """absent: F.gumbel_softmax four times (iv, uv, it, ut), then F.dropout four times in the same order, and no library call of
    the new entry points; the shapes tell the order"""
    import mmrec_amd.models.lgmrec as lmod
    config, _, _, model = build(tmp_path, golden, "LGMRec", dict(LGM_EXTRA))
    assert model.fused_hyper is False
    lgm = _golden()
    seen = []
    real_g, real_d = lmod.F.gumbel_softmax, lmod.F.dropout
    with monkeypatch.context() as m:
        calls = _spy(m)
        m.setattr(lmod.F, "gumbel_softmax", lambda logits, *a, **k: seen.append(("gumbel", logits.shape[0])) or real_g(logits, *a, **k))
        m.setattr(lmod.F, "dropout", lambda x, *a, **k: seen.append(("dropout", x.shape[0])) or real_d(x, *a, **k))
        model.train()
        loss = model.calculate_loss(torch.as_tensor(lgm["batch1"]).to(model.device))
        loss.backward()
        torch.cuda.synchronize()
        assert all(not v for v in calls.values()), calls
    nI, nU = model.n_items, model.n_users
    assert nI != nU
    assert seen == [("gumbel", n) for n in (nI, nU, nI, nU)] + [("dropout", n) for n in (nI, nU, nI, nU)], seen
    assert bool(torch.isfinite(loss))
