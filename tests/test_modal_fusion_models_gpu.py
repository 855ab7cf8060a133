"""GPU: MGCN with `fused_fusion: True` (hip_ops.modal_fusion, csrc/modal_fusion.hip) on the reference's golden step --
tests/golden/mgcn.npz: weights, batch, the kNN graphs pinned to the golden's -- at the tolerances of
tests/test_models_gpu.py::test_mgcn_model; the kernels are really taken (library calls counted, with their row count) and the torch
composition is not; three optimiser steps stay finite and a full evaluation runs; with the key absent the new entry points are
never called; a captured forward + backward replays the eager bits."""
import os

import numpy as np
import pytest
import torch

from tests.test_models_gpu import build, close, eval_topk, load

pytestmark = pytest.mark.gpu

ENTRY_POINTS = ("mmrec_modal_fusion_fwd_f32", "mmrec_modal_fusion_bwd_f32")
MGCN_EXTRA = {"cl_loss": 0.01, "learning_rate": 1e-3}
GRADS = ("user_embedding.weight", "item_id_embedding.weight", "image_trs.weight", "text_embedding.weight", "image_embedding.weight",
         "gate_v.0.weight", "query_common.2.weight", "gate_text_prefer.0.bias", "text_trs.bias",              # test_mgcn_model's list
         "query_common.0.weight", "query_common.0.bias", "gate_image_prefer.0.weight")


def _golden():
    return dict(np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mgcn.npz")))


def _spy(m):
    """count the library calls of the two entry points, with their row count"""
    from mmrec_amd import _lib
    lib = _lib.load()
    calls = {fn: [] for fn in ENTRY_POINTS}
    for fn in ENTRY_POINTS:
        def spy(*a, _real=getattr(lib, fn), _fn=fn):
            calls[_fn].append(a[12] if "bwd" in _fn else a[10])
            return _real(*a)
        m.setattr(lib, fn, spy)
    return calls


def _no_composition(m, model):
    """the composition's pieces: the model's _query / _gate on the fuser's modules, and modal_fusion_torch"""
    from mmrec_amd import hip_ops
    m.setattr(model, "_query", lambda *a: pytest.fail("the torch composition ran with the key on"))
    m.setattr(hip_ops, "modal_fusion_torch", lambda *a: pytest.fail("the torch composition ran with the key on"))
    real = type(model)._gate
    prefer = (model.gate_image_prefer, model.gate_text_prefer)
    m.setattr(type(model), "_gate", staticmethod(
        lambda seq, x: pytest.fail("a preference gate ran as a composition") if seq in prefer else real(seq, x)))


def _pin_graphs(model, mgc):
    """the kNN graphs of the golden (near-tie neighbours may swap), as test_mgcn_model pins them"""
    from mmrec_amd import hip_ops
    ni = model.n_items
    for key in ("image", "text"):
        g = hip_ops.CsrGraph.from_coo_host(mgc[key + "_original_adj_idx"], mgc[key + "_original_adj_val"], ni, ni, model.device)
        g.transpose()
        setattr(model, key + "_original_adj", g)


def test_mgcn_golden_step_with_fused_fusion(tmp_path, golden, monkeypatch):
    mgc = _golden()
    config, _, valid_data, model = build(tmp_path, golden, "MGCN", dict(MGCN_EXTRA, fused_fusion=True))
    assert model.fused_fusion is True
    params = dict(model.named_parameters())
    assert set(params) == {k[2:] for k in mgc if k.startswith("p_")}
    for name, p in params.items():
        load(p, mgc["p_" + name])
    _pin_graphs(model, mgc)
    dev, n = model.device, model.n_users + model.n_items
    with monkeypatch.context() as m:
        calls = _spy(m)
        _no_composition(m, model)
        model.eval()
        with torch.no_grad():
            u, i = model.eval_embeddings()
        torch.cuda.synchronize()
        assert calls == {"mmrec_modal_fusion_fwd_f32": [n], "mmrec_modal_fusion_bwd_f32": []}, calls   # eval: one forward
        close(u, mgc["user_out"], atol=2e-6), close(i, mgc["item_out"], atol=2e-6)
        users, mask = next(iter(valid_data))
        for _ in valid_data:
            pass
        close(model.full_sort_predict([users, mask]), mgc["scores_first_batch"], rtol=1e-4, atol=2e-6)
        model.train()
        ua, ia, side, content = model.forward(model.norm_adj, train=True)
        close(ua, mgc["user_out"], atol=2e-6), close(ia, mgc["item_out"], atol=2e-6)
        close(side, mgc["side_embeds"], atol=2e-6), close(content, mgc["content_embeds"], atol=2e-6)
        del ua, ia, side, content
        for v in calls.values():
            v.clear()
        loss = model.calculate_loss(torch.as_tensor(mgc["batch1"]).to(dev))
        loss.backward()
        torch.cuda.synchronize()
        assert calls == {"mmrec_modal_fusion_fwd_f32": [n], "mmrec_modal_fusion_bwd_f32": [n]}, calls  # the step: one call each way
    close(loss, mgc["loss1"], rtol=1e-5)
    for name in GRADS:
        assert "g_" + name in mgc, name
        close(params[name].grad, mgc["g_" + name], rtol=5e-4, atol=1e-8)


def test_three_steps_stay_finite_and_an_evaluation_runs(tmp_path, golden, monkeypatch):
    config, train_data, valid_data, model = build(tmp_path, golden, "MGCN", dict(MGCN_EXTRA, fused_fusion=True, train_batch_size=64))
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
        assert len(calls["mmrec_modal_fusion_fwd_f32"]) == 3 and len(calls["mmrec_modal_fusion_bwd_f32"]) == 3, calls
    print("losses with fused_fusion:", losses)
    assert len(losses) == 3 and np.isfinite(losses).all()
    assert all(bool(torch.isfinite(p).all()) for p in model.parameters())
    fused, _ = eval_topk(config, model, valid_data)
    assert 0.0 <= fused["recall@20"] <= 1.0


def test_key_absent_runs_the_composition_and_no_new_entry_point(tmp_path, golden, monkeypatch):
    mgc = _golden()
    config, _, _, model = build(tmp_path, golden, "MGCN", dict(MGCN_EXTRA))
    assert model.fused_fusion is False
    seen = []
    real = model._query
    with monkeypatch.context() as m:
        calls = _spy(m)
        m.setattr(model, "_query", lambda x: seen.append(tuple(x.shape)) or real(x))
        model.train()
        loss = model.calculate_loss(torch.as_tensor(mgc["batch1"]).to(model.device))
        loss.backward()
        torch.cuda.synchronize()
        assert all(not v for v in calls.values()), calls
    assert seen == [(model.n_users + model.n_items, 64)] * 2, seen
    assert bool(torch.isfinite(loss))


def test_graphed_epoch_equals_eager_with_the_key_on(tmp_path, golden):
    """tests/test_models_gpu.py's graphed-equals-eager comparison (an epoch replayed as a hipGraph gives the eager epoch's
    parameters), run for MGCN with the key on: with it the step has no library GEMM left"""
    from tests.test_models_gpu import test_graphed_train_step_equals_eager
    test_graphed_train_step_equals_eager(tmp_path, golden, "MGCN", dict(MGCN_EXTRA, fused_fusion=True))


def test_forward_and_backward_replay_from_a_captured_graph():
    """forward + backward captured on one stream and replayed: the eager bits (no host synchronisation, no allocation inside the
    library, no data-dependent launch shape)"""
    import tests.test_modal_fusion_fuzz_gpu as Z
    from mmrec_amd import hip_ops
    from tests.test_hyper_fuzz_gpu import _bits
    from tests.test_spmm_fuzz_gpu import _on
    c = Z.case(20)
    assert c.n > 2 * 64
    ops = [_on(c.ops[k].reshape(1, 64) if k == "q" else c.ops[k]).requires_grad_() for k in Z.OPERANDS]
    gs, go = (_on(np.random.default_rng(5 + i).standard_normal((c.n, 64)).astype(np.float32)) for i in range(2))

    def step():
        for t in ops:
            t.grad = None
        side, out = hip_ops.modal_fusion(*ops)
        ((side * gs).sum() + (out * go).sum()).backward()
        return [side.detach(), out.detach()] + [t.grad for t in ops]
    eager = [t.clone() for t in step()]
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        held = step()
    with torch.no_grad():                                                 # other inputs in the same buffers, then the first ones again
        ops[0].copy_(_on(c.ops["V"][::-1].copy()))
    graph.replay()
    torch.cuda.synchronize()
    other = [t.clone() for t in held]
    with torch.no_grad():
        ops[0].copy_(_on(c.ops["V"]))
    graph.replay()
    torch.cuda.synchronize()
    first = [t.clone() for t in held]
    graph.replay()
    torch.cuda.synchronize()
    for a, b, b2 in zip(eager, first, held):
        assert torch.equal(_bits(a), _bits(b)) and torch.equal(_bits(b), _bits(b2))
    assert not torch.equal(_bits(eager[0]), _bits(other[0]))              # the replay really computed
    got = dict(zip(("side", "out") + Z.GRADS, [t.reshape(c.ops[k].shape) if k in c.ops else t
                                               for k, t in zip(("side", "out") + Z.OPERANDS, held)]))
    print("graph replay: worst err / bound", Z.check(c.ops, [t.cpu().numpy() for t in (gs, go)], got, "graph"))
