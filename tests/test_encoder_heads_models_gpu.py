"""GPU: MVGAE with `fused_heads: True` (hip_ops.encoder_heads, csrc/encoder_heads.hip) on the reference's golden step --
tests/golden/mvgae.npz: weights, batch, the 12 dropout masks and 4 noise tables replayed in call order -- alone and together with
`fused_posterior: True`, at the tolerances of tests/test_models_gpu.py::test_mvgae_model; the kernels are really taken (library
calls counted, with their row count) and the torch composition is not; three optimiser steps stay finite and a full evaluation
runs with fused and dense metrics equal; with the key absent the new entry points are never called; a captured forward + backward
replays the eager bits."""
import numpy as np
import pytest
import torch

from tests.test_models_gpu import _golden, build, close, eval_topk, load, same_metrics

pytestmark = pytest.mark.gpu

ENTRY_POINTS = ("mmrec_encoder_heads_fwd_f32", "mmrec_encoder_heads_bwd_f32")
MVGAE_EXTRA = {"learning_rate": 1e-3, "beta": 0.1, "n_layers": 2}


def _spy(m):
    """count the library calls of the two entry points, with their row count"""
    from mmrec_amd import _lib
    lib = _lib.load()
    calls = {fn: [] for fn in ENTRY_POINTS}
    for fn in ENTRY_POINTS:
        def spy(*a, _real=getattr(lib, fn), _fn=fn):
            calls[_fn].append(a[10] if "bwd" in _fn else a[9])
            return _real(*a)
        m.setattr(lib, fn, spy)
    return calls


def _no_composition(m):
    """the composition's pieces: the head convolutions' own forward, and encoder_heads_torch"""
    from mmrec_amd import hip_ops
    fail = lambda *a, **k: pytest.fail("the torch composition ran with the key on")      # noqa: E731
    m.setattr(hip_ops, "encoder_heads_torch", fail)
    return fail


@pytest.mark.parametrize("posterior", (False, True))
def test_mvgae_golden_step_with_fused_heads(tmp_path, golden, monkeypatch, posterior):
    import mmrec_amd.models.mvgae as mv
    g = _golden("mvgae")
    config, _, valid_data, model = build(tmp_path, golden, "MVGAE", dict(MVGAE_EXTRA, fused_heads=True, fused_posterior=posterior))
    assert model.fused_heads is True and model.fused_posterior is posterior and model.graph_capturable is False
    assert all(gcn.fused_heads for gcn in (model.v_gcn, model.t_gcn, model.c_gcn))
    params = dict(model.named_parameters())
    assert set(params) == {k[2:] for k in g if k.startswith("p_")}
    for name, p in params.items():
        load(p, g["p_" + name])
    dev, n = model.device, model.n_users + model.n_items
    masks = [torch.as_tensor(g["mask_%d" % j].astype(np.float32)).to(dev) for j in range(12)]
    noises = [torch.as_tensor(g["noise_%d" % j]).to(dev) for j in range(4)]
    with monkeypatch.context() as m:
        calls = _spy(m)
        fail = _no_composition(m)
        for gcn in (model.v_gcn, model.t_gcn, model.c_gcn):               # the head convolutions are never run on their own
            for j in (4, 5):
                m.setattr(getattr(gcn, "conv_embed_%d" % j), "forward", fail)
        m.setattr(mv.F, "dropout", lambda x, p=0.5, training=True, inplace=False: x * masks.pop(0) / (1.0 - p) if training else x)
        m.setattr(mv.torch, "randn_like", lambda x, *a, **k: noises.pop(0))
        model.train()
        loss = model.calculate_loss(torch.as_tensor(g["batch1"]).to(dev))
        loss.backward()
        torch.cuda.synchronize()
        assert calls == {"mmrec_encoder_heads_fwd_f32": [n] * 3, "mmrec_encoder_heads_bwd_f32": [n] * 3}, calls
    assert not masks and not noises                                       # all twelve masks consumed
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


def test_three_steps_stay_finite_and_an_evaluation_runs(tmp_path, golden, monkeypatch):
    config, train_data, valid_data, model = build(tmp_path, golden, "MVGAE",
                                                  dict(MVGAE_EXTRA, fused_heads=True, train_batch_size=64))
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
        assert len(calls["mmrec_encoder_heads_fwd_f32"]) == 9 and len(calls["mmrec_encoder_heads_bwd_f32"]) == 9, calls
    print("losses with fused_heads:", losses)
    assert len(losses) == 3 and np.isfinite(losses).all()
    assert all(bool(torch.isfinite(p).all()) for p in model.parameters())
    fused, dense = eval_topk(config, model, valid_data)
    same_metrics(fused, dense)


def test_key_absent_runs_the_composition_and_no_new_entry_point(tmp_path, golden, monkeypatch):
    from mmrec_amd import hip_ops
    g = _golden("mvgae")
    config, _, _, model = build(tmp_path, golden, "MVGAE", dict(MVGAE_EXTRA))
    assert model.fused_heads is False and not model.v_gcn.fused_heads
    seen = []
    with monkeypatch.context() as m:
        calls = _spy(m)
        m.setattr(hip_ops, "encoder_heads", lambda *a, **k: pytest.fail("hip_ops.encoder_heads ran with the key absent"))
        real = model.v_gcn.conv_embed_4.forward
        m.setattr(model.v_gcn.conv_embed_4, "forward", lambda x, graph: seen.append(tuple(x.shape)) or real(x, graph))
        model.train()
        loss = model.calculate_loss(torch.as_tensor(g["batch1"]).to(model.device))
        loss.backward()
        torch.cuda.synchronize()
        assert all(not v for v in calls.values()), calls
    assert seen == [(model.n_users + model.n_items, 64)], seen
    assert bool(torch.isfinite(loss))


def test_forward_and_backward_replay_from_a_captured_graph():
    """forward + backward captured on one stream and replayed: the eager bits (no host synchronisation, no allocation inside the
    library, no data-dependent launch shape); and the replay really recomputes after an input is overwritten"""
    import tests.test_encoder_heads_fuzz_gpu as Z
    from mmrec_amd import hip_ops
    from tests.test_hyper_fuzz_gpu import _bits
    from tests.test_spmm_fuzz_gpu import _on
    c = Z.case(34)
    assert c.n > 2 * 64 and c.H == 2 and c.scale is not None and not c.g_zero
    ops = [_on(c.ops[k]).requires_grad_() for k in Z.OPERANDS]
    scale, g = _on(c.scale), _on(c.g)

    def step():
        for t in ops:
            t.grad = None
        out = hip_ops.encoder_heads(*ops, scale)
        (out * g).sum().backward()
        return [out.detach()] + [t.grad for t in ops]
    assert hip_ops.encoder_heads_served(*ops, scale)
    eager = [t.clone() for t in step()]
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        held = step()
    with torch.no_grad():                                                 # other inputs in the same buffers, then the first ones again
        ops[0].copy_(_on(c.ops["AX"][::-1].copy()))
    graph.replay()
    torch.cuda.synchronize()
    other = [t.clone() for t in held]
    with torch.no_grad():
        ops[0].copy_(_on(c.ops["AX"]))
    graph.replay()
    torch.cuda.synchronize()
    first = [t.clone() for t in held]
    graph.replay()
    torch.cuda.synchronize()
    for a, b, b2 in zip(eager, first, held):
        assert torch.equal(_bits(a), _bits(b)) and torch.equal(_bits(b), _bits(b2))
    assert not torch.equal(_bits(eager[0]), _bits(other[0]))              # the replay really computed
    got = dict(zip(("out",) + Z.GRADS, held))
    print("graph replay: worst err / bound", Z.check(c.ops, c.scale, c.g, got, "graph"))
