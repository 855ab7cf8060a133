"""GPU: LGMRec at Clothing's hypergraph setting (hyper_num 64, n_hyper_layer 2, keep_rate 0.2) with `fused_hyper: True` on the tiny
golden dataset.  There is no golden at 64; the key-off path is width-agnostic torch already pinned to the reference at 4, so the
key-on step is held to it: the same weights, the same Gumbel noise and masks (drawn once with a seeded generator at the model's
shapes, fed through `replay_draws` of tests/test_hyper_cpu.py) -- loss, every parameter gradient and the evaluation forward within
the README's fp32 parity bar (RTOL of tests/test_hyper_cpu.py).  A spy on the library shows the mmrec_hyper64_* entry points taken
with the expected row counts and no narrow mmrec_hyper_* call; with the model's own draws three Adam steps stay finite and a full
evaluation runs; with the key absent neither family is called."""
import os

import numpy as np
import pytest
import torch

from tests.test_hyper64_cpu import CLOTHING, clothing_step, draws_for
from tests.test_hyper_cpu import RTOL, replay_draws
from tests.test_hyper_models_gpu import ENTRY_POINTS as NARROW
from tests.test_models_gpu import build, eval_topk

pytestmark = pytest.mark.gpu

WIDE = ("mmrec_hyper64_assign_fwd_f32", "mmrec_hyper64_assign_bwd_f32", "mmrec_hyper64_layer_fwd_f32", "mmrec_hyper64_layer_bwd_f32")


def _batch():
    return dict(np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lgmrec.npz")))["batch1"]


def _spy(m):
    """the library calls of both families: (n,) of a 64-wide assignment, (I, U) of a 64-wide layer, a mark for a narrow call"""
    from mmrec_amd import _lib
    lib = _lib.load()
    calls = {fn: [] for fn in WIDE + NARROW}
    for fn in WIDE:
        def spy(*a, _real=getattr(lib, fn), _fn=fn):
            calls[_fn].append(tuple(a[3:4]) if "assign" in _fn else tuple(a[6:8]) if "bwd" in _fn else tuple(a[3:5]))
            return _real(*a)
        m.setattr(lib, fn, spy)
    for fn in NARROW:
        m.setattr(lib, fn, lambda *a, _real=getattr(lib, fn), _fn=fn: calls[_fn].append(True) or _real(*a))
    return calls


def _within(a, b, name):
    a, b = a.detach().double().cpu().numpy(), b.detach().double().cpu().numpy()
    scale = float(np.abs(b).max())
    print("%s: max|on - off| %.3e, max|off| %.3e, ratio %.3e (bar %.0e)" % (name, float(np.abs(a - b).max()), scale,
                                                                         float(np.abs(a - b).max()) / scale if scale else 0.0, RTOL))
    assert np.isfinite(a).all() and float(np.abs(a - b).max()) <= RTOL * scale, (name, float(np.abs(a - b).max()), scale)


def test_clothing_setting_runs_the_64_family_and_agrees_with_the_key_off_step(tmp_path, golden, monkeypatch):
    batch = _batch()
    off, loss_off, g_off = clothing_step(tmp_path / "off", golden, monkeypatch, {}, batch)
    state = {k: v.clone() for k, v in off.state_dict().items()}
    nI, nU = off.n_items, off.n_users
    with monkeypatch.context() as m:
        calls = _spy(m)
        on, loss_on, g_on = clothing_step(tmp_path / "on", golden, m, {"fused_hyper": True}, batch, state)
        torch.cuda.synchronize()
        print("library calls with the key on:", {k: v for k, v in calls.items() if v})
        # the kernels were really taken: iv, uv, it, ut assigned; per modality an inner layer without user rows, then the last
        # one; the mirror of each; and nothing of the narrow family
        assert calls["mmrec_hyper64_assign_fwd_f32"] == [(nI,), (nU,), (nI,), (nU,)], calls
        assert sorted(calls["mmrec_hyper64_assign_bwd_f32"]) == sorted([(nI,), (nU,)] * 2), calls
        assert calls["mmrec_hyper64_layer_fwd_f32"] == [(nI, 0), (nI, nU)] * 2, calls
        assert sorted(calls["mmrec_hyper64_layer_bwd_f32"]) == sorted([(nI, 0), (nI, nU)] * 2), calls
        assert all(not calls[fn] for fn in NARROW), calls
    print("loss on %.9g off %.9g, relative difference %.3e" % (float(loss_on), float(loss_off),
                                                               abs(float(loss_on) - float(loss_off)) / abs(float(loss_off))))
    assert abs(float(loss_on) - float(loss_off)) <= RTOL * abs(float(loss_off)), (float(loss_on), float(loss_off))
    assert set(g_on) == set(g_off) and len(g_on) >= 6
    for n in sorted(g_on):
        _within(g_on[n], g_off[n], n)
    for n in ("v_hyper", "t_hyper", "item_id_embedding.weight", "user_embedding.weight"):
        assert float(g_on[n].abs().max()) > 0, n
    # the evaluation forward: noise drawn, no dropout
    outs = []
    for model in (on, off):
        model.eval()
        with monkeypatch.context() as m:
            queue_n, queue_m = replay_draws(model, draws_for(model, 65), m)
            with torch.no_grad():
                u, i, hyper = model.forward()
            assert not queue_n and len(queue_m) == 4
        outs.append([u, i] + list(hyper))
    for j, (a, b) in enumerate(zip(*outs)):
        _within(a, b, "eval output %d" % j)


def test_three_adam_steps_stay_finite_and_a_full_evaluation_runs(tmp_path, golden, monkeypatch):
    config, train_data, valid_data, model = build(tmp_path, golden, "LGMRec", dict(CLOTHING, fused_hyper=True, train_batch_size=64))
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
        assert len(calls["mmrec_hyper64_layer_fwd_f32"]) == 3 * 2 * 2 and len(calls["mmrec_hyper64_layer_bwd_f32"]) == 3 * 2 * 2, calls
        assert len(calls["mmrec_hyper64_assign_fwd_f32"]) == 3 * 4 and all(not calls[fn] for fn in NARROW), calls
    print("losses with fused_hyper at 64 hyperedges, two layers:", losses)
    assert len(losses) == 3 and np.isfinite(losses).all()
    assert all(bool(torch.isfinite(p).all()) for p in model.parameters())
    fused, _ = eval_topk(config, model, valid_data)
    assert 0.0 <= fused["recall@20"] <= 1.0


def test_key_absent_calls_neither_family(tmp_path, golden, monkeypatch):
    config, _, _, model = build(tmp_path, golden, "LGMRec", dict(CLOTHING))
    assert model.fused_hyper is False and model.hyper_num == 64
    with monkeypatch.context() as m:
        calls = _spy(m)
        model.train()
        torch.manual_seed(5)
        loss = model.calculate_loss(torch.as_tensor(_batch()).to(model.device))
        loss.backward()
        torch.cuda.synchronize()
        assert all(not v for v in calls.values()), calls
    assert bool(torch.isfinite(loss))
