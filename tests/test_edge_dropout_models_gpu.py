"""GPU: SELFCFED_LGN with `fused_edge_dropout: True` (the encoder's per-batch sparse dropout inside the SpMM,
hip_ops.lightgcn_mean_edge_dropout) on the tiny golden dataset: the reference's golden step at the tolerances of
tests/test_models_gpu.py::test_selfcfed_lgn_model; the `EDGE_DROPOUT` switch off gives the key-off step; the propagated tables
repeat bit for bit; a Trainer epoch with the model's own draws runs and evaluation does not change."""
import numpy as np
import pytest
import torch

from tests.test_models_gpu import _selfcf, build, close, load

pytestmark = pytest.mark.gpu

EXTRA = {"n_layers": 2, "dropout": 0.2, "reg_weight": 1e-3}
MASKED = ("mmrec_spmm_csr_masked_f32", "mmrec_edge_keep_bits")


def _golden_step(tmp_path, golden, monkeypatch, fused):
    """one loss + backward with the reference's parameters, batch and injected draws -> loss, gradients, library calls"""
    from mmrec_amd import _lib
    import mmrec_amd.models.selfcfed_lgn as smod
    scf = _selfcf()
    lib = _lib.load()
    calls = {fn: 0 for fn in MASKED}
    with monkeypatch.context() as m:
        for fn in calls:
            def spy(*a, _real=getattr(lib, fn), _fn=fn):
                calls[_fn] += 1
                return _real(*a)
            m.setattr(lib, fn, spy)
        extra = dict(EXTRA, fused_edge_dropout=True) if fused else dict(EXTRA)
        config, _, _, model = build(tmp_path, golden, "SELFCFED_LGN", extra)
        params = dict(model.named_parameters())
        for name, p in params.items():
            load(p, scf["s_p_" + name])
        dev, enc = model.device, model.online_encoder
        assert enc.fused_edge_dropout is fused
        keep = torch.as_tensor(scf["s_drop_keep"]).to(dev)
        enc.draw_dropout = lambda: (float(scf["s_drop_rate"]), keep)
        masks = [torch.as_tensor(scf["s_target_mask_" + k].astype(np.float32)).to(dev) for k in "ui"]
        m.setattr(smod.F, "dropout", lambda x, p=0.5, training=True, inplace=False: x * masks.pop(0) / (1.0 - p))
        loss = model.calculate_loss(torch.as_tensor(scf["s_batch1"]).to(dev))
        loss.backward()
        torch.cuda.synchronize()
        grads = {n: p.grad.detach().clone() for n, p in params.items()}
    return scf, loss.detach().clone(), grads, calls


def test_golden_step_with_the_key_on(tmp_path, golden, monkeypatch):
    scf, loss, grads, calls = _golden_step(tmp_path, golden, monkeypatch, True)
    assert calls == {"mmrec_spmm_csr_masked_f32": 4, "mmrec_edge_keep_bits": 1}, calls    # L = 2 forward + 2 backward, one pack
    print("SELFCFED_LGN fused_edge_dropout: loss %.9g, golden %.9g" % (float(loss), float(scf["s_loss1"])))
    close(loss, scf["s_loss1"], rtol=1e-5)
    for name, g in grads.items():
        close(g, scf["s_g_" + name], rtol=5e-4, atol=1e-8)


def test_switch_off_gives_the_key_off_step(tmp_path, golden, monkeypatch):
    """key on, `hip_ops.EDGE_DROPOUT = False`: the ops run the composition of the older kernels -- spmm_vals per layer and
    stack().mean(), the key-off code -- so loss and gradients are the key-off step's, bit for bit (`hip_deterministic`: the
    loss kernels' scatters without atomics, or no two steps would share their last bits)"""
    from mmrec_amd import hip_ops
    try:
        hip_ops.set_deterministic(True)
        monkeypatch.setattr(hip_ops, "EDGE_DROPOUT", False)
        _, loss_a, grads_a, calls = _golden_step(tmp_path / "a", golden, monkeypatch, True)
        monkeypatch.setattr(hip_ops, "EDGE_DROPOUT", True)
        _, loss_b, grads_b, _ = _golden_step(tmp_path / "b", golden, monkeypatch, False)
    finally:
        hip_ops.set_deterministic(hip_ops.DETERMINISTIC_DEFAULT)
    assert calls == {fn: 0 for fn in MASKED}, calls
    assert torch.equal(loss_a.view(torch.int32), loss_b.view(torch.int32)), (float(loss_a), float(loss_b))
    for n in sorted(grads_a):
        assert torch.equal(grads_a[n].view(torch.int32), grads_b[n].view(torch.int32)), n
    assert float(grads_a["online_encoder.embedding_dict.user_emb"].abs().max()) > 0


def test_propagated_tables_repeat_bit_for_bit(tmp_path, golden):
    """two same-seed forward + backward passes through the encoder with the key on (its own draws): tables and embedding
    gradients repeat bit for bit -- no atomics anywhere in the masked product"""
    runs = []
    for tag in "ab":
        config, _, _, model = build(tmp_path / tag, golden, "SELFCFED_LGN", dict(EXTRA, fused_edge_dropout=True))
        enc = model.online_encoder
        np.random.seed(5), torch.manual_seed(5)
        u, i = enc.all_embeddings(True)
        gen = torch.Generator(device=u.device).manual_seed(1)
        (u * torch.randn(u.shape, device=u.device, generator=gen)).sum().backward(retain_graph=True)
        (i * torch.randn(i.shape, device=u.device, generator=gen)).sum().backward()
        torch.cuda.synchronize()
        runs.append([u.detach(), i.detach(), enc.embedding_dict["user_emb"].grad, enc.embedding_dict["item_emb"].grad])
    for x, y in zip(*runs):
        assert float(x.abs().max()) > 0 and torch.equal(x.view(torch.int32), y.view(torch.int32))
    u, i = runs[0][:2]
    plain = model.online_encoder.all_embeddings(False)
    assert not torch.equal(u, plain[0])                               # (the dropout did something)


def test_trainer_epoch_and_evaluation(tmp_path, golden):
    """one Trainer epoch with the model's own draws ends with finite losses; `get_embedding` takes no dropout, so a model built
    with the key evaluates exactly as one built without"""
    from mmrec_amd.common.trainer import Trainer
    config, train_data, valid_data, model = build(tmp_path / "on", golden, "SELFCFED_LGN",
                                                  dict(EXTRA, fused_edge_dropout=True, train_batch_size=64))
    _, _, _, plain = build(tmp_path / "off", golden, "SELFCFED_LGN", dict(EXTRA, train_batch_size=64))
    with torch.no_grad():
        for (n, p), (n2, q) in zip(model.named_parameters(), plain.named_parameters()):
            assert n == n2
            q.copy_(p)
    for a, b in zip(model.get_embedding(), plain.get_embedding()):
        assert torch.equal(a, b)
    trainer = Trainer(config, model)
    res0 = trainer.evaluate(valid_data)
    assert res0 == Trainer(config, plain).evaluate(valid_data)
    total, losses = trainer._train_epoch(train_data, 0)
    vals = torch.stack([x.reshape(()) for x in losses]).cpu().numpy()
    assert vals.size >= 3 and np.isfinite(vals).all() and np.isfinite(float(total))
    assert model.online_encoder._edge_graph is not None and model.online_encoder._edge_graph.dyn is model.online_encoder._dyn
    res1 = trainer.evaluate(valid_data)
    assert all(np.isfinite(v) for v in res1.values())
