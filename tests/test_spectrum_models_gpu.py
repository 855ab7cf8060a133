"""GPU: SMORE with `fused_spectrum: True` (hip_ops.spectrum_fusion, csrc/spectrum.hip) on the reference's golden step --
tests/golden/smore.npz: weights, batch, the three dropout masks replayed, the kNN graphs pinned to the golden's -- at the tolerances
of tests/test_models_gpu.py::test_smore_model; the kernels are really taken (library calls counted, with their row count); three
optimiser steps stay finite and a full evaluation runs; with the key absent `spectrum_convolution` runs and the new entry points
are never called."""
import os

import numpy as np
import pytest
import torch

from tests.test_models_gpu import build, close, eval_topk, load

pytestmark = pytest.mark.gpu

ENTRY_POINTS = ("mmrec_spectrum_fwd_f32", "mmrec_spectrum_bwd_f32")
SMORE_EXTRA = {"cl_loss": 0.01, "learning_rate": 1e-3, "n_ui_layers": 3, "image_knn_k": 10, "text_knn_k": 15, "reg_weight": 1e-4,
               "dropout_rate": 0.1}
GRADS = ("user_embedding.weight", "item_id_embedding.weight", "image_trs.weight", "text_embedding.weight", "image_embedding.weight",
         "gate_f.0.weight", "query_v.2.weight", "query_t.0.bias", "gate_fusion_prefer.0.bias", "image_complex_weight",
         "text_complex_weight", "fusion_complex_weight")


def _golden():
    return dict(np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "smore.npz")))


def _spy(m):
    """count the library calls of the two entry points, with their row count"""
    from mmrec_amd import _lib
    lib = _lib.load()
    calls = {fn: [] for fn in ENTRY_POINTS}
    for fn in ENTRY_POINTS:
        def spy(*a, _real=getattr(lib, fn), _fn=fn):
            calls[_fn].append(a[8] if "bwd" in _fn else a[5])
            return _real(*a)
        m.setattr(lib, fn, spy)
    return calls


def _pin_graphs(model, smo):
    """the kNN graphs of the golden (near-tie neighbours may swap), as test_smore_model pins them"""
    from mmrec_amd import hip_ops
    from mmrec_amd.models.smore import max_pool_fusion
    ni = model.n_items
    for key in ("image", "text"):
        g = hip_ops.CsrGraph.from_coo_host(smo[key + "_original_adj_idx"], smo[key + "_original_adj_val"], ni, ni, model.device)
        g.transpose()
        setattr(model, key + "_original_adj", g)
    model.fusion_adj = max_pool_fusion(model.image_original_adj, model.text_original_adj, ni)


def test_smore_golden_step_with_fused_spectrum(tmp_path, golden, monkeypatch):
    import mmrec_amd.models.smore as smod
    smo = _golden()
    config, _, valid_data, model = build(tmp_path, golden, "SMORE", dict(SMORE_EXTRA, fused_spectrum=True))
    assert model.fused_spectrum is True
    params = dict(model.named_parameters())
    assert set(params) == {k[2:] for k in smo if k.startswith("p_")}
    for name, p in params.items():
        load(p, smo["p_" + name])
    _pin_graphs(model, smo)
    dev, ni = model.device, model.n_items
    with monkeypatch.context() as m:
        calls = _spy(m)
        m.setattr(model, "spectrum_convolution", lambda *a: pytest.fail("the torch composition ran with the key on"))
        model.eval()
        with torch.no_grad():
            u, i = model.eval_embeddings()
        torch.cuda.synchronize()
        assert calls == {"mmrec_spectrum_fwd_f32": [ni], "mmrec_spectrum_bwd_f32": []}, calls     # eval: one forward, no backward
        close(u, smo["user_out"], atol=2e-6), close(i, smo["item_out"], atol=2e-6)
        users, mask = next(iter(valid_data))
        for _ in valid_data:
            pass
        close(model.full_sort_predict([users, mask]), smo["scores_first_batch"], rtol=1e-4, atol=2e-6)
        for v in calls.values():
            v.clear()
        model.train()
        masks = [torch.as_tensor(smo["drop_mask_%d" % j].astype(np.float32)).to(dev) for j in range(3)]
        m.setattr(smod.F, "dropout", lambda x, p=0.5, training=True, inplace=False: x * masks.pop(0) / (1.0 - p))
        loss = model.calculate_loss(torch.as_tensor(smo["batch1"]).to(dev))
        loss.backward()
        torch.cuda.synchronize()
        assert not masks
        assert calls == {"mmrec_spectrum_fwd_f32": [ni], "mmrec_spectrum_bwd_f32": [ni]}, calls   # the step: one call each way
    close(loss, smo["loss1"], rtol=1e-5)
    for name in GRADS:
        close(params[name].grad, smo["g_" + name], rtol=5e-4, atol=1e-8)
    for name in ("image_complex_weight", "text_complex_weight", "fusion_complex_weight"):
        g = params[name].grad
        assert float(g[0, 0, 1]) == 0.0 and float(g[0, -1, 1]) == 0.0      # as torch.fft: exactly zero


def test_three_steps_stay_finite_and_an_evaluation_runs(tmp_path, golden, monkeypatch):
    config, train_data, valid_data, model = build(tmp_path, golden, "SMORE", dict(SMORE_EXTRA, fused_spectrum=True,
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
        assert len(calls["mmrec_spectrum_fwd_f32"]) == 3 and len(calls["mmrec_spectrum_bwd_f32"]) == 3, calls
    print("losses with fused_spectrum:", losses)
    assert len(losses) == 3 and np.isfinite(losses).all()
    assert all(bool(torch.isfinite(p).all()) for p in model.parameters())
    fused, _ = eval_topk(config, model, valid_data)
    assert 0.0 <= fused["recall@20"] <= 1.0


def test_key_absent_runs_spectrum_convolution_and_no_new_entry_point(tmp_path, golden, monkeypatch):
    smo = _golden()
    config, _, _, model = build(tmp_path, golden, "SMORE", dict(SMORE_EXTRA))
    assert model.fused_spectrum is False
    seen = []
    real = model.spectrum_convolution
    with monkeypatch.context() as m:
        calls = _spy(m)
        m.setattr(model, "spectrum_convolution", lambda a, b: seen.append(tuple(a.shape)) or real(a, b))
        model.train()
        torch.manual_seed(5)
        loss = model.calculate_loss(torch.as_tensor(smo["batch1"]).to(model.device))
        loss.backward()
        torch.cuda.synchronize()
        assert all(not v for v in calls.values()), calls
    assert seen == [(model.n_items, 64)], seen
    assert bool(torch.isfinite(loss))
