"""GPU: FREEDOM and BM3 with `hip_gathered_projection` -- the batch's feature rows projected straight from the table
(hip_ops.linear_rows / LazyRowEmbedding.project_rows; freedom.py:203-209, bm3.py:102-104 under `lazy_projection`) -- at
Amazon-Baby shape (4096-wide image and 384-wide text features, tests.test_config_shapes_gpu.build_shape).  The gathered kernels
return the bits of the two-step form (index_select, then linear), so under `hip_deterministic` training with the key on and
off must end in bit-identical parameters with bit-identical losses on the way; a replayed (hipGraph) epoch must match the eager
one; and the key must decide which code runs."""
import itertools

import numpy as np
import pytest
import torch

from tests.test_config_shapes_gpu import build_shape

pytestmark = pytest.mark.gpu

HYPER = {"FREEDOM": {"dropout": 0.8, "reg_weight": 1e-3},
         "BM3": {"n_layers": 2, "dropout": 0.3, "reg_weight": 0.1}}


def _three_steps(root, name, lazy_adam, gathered, batches=None):
    """three optimizer steps on three different batches -> (the batches, per-step losses, final parameters)"""
    from mmrec_amd import hip_ops
    from mmrec_amd.common.lazy_rows import LazyRowEmbedding, flush_lazy_tables
    from mmrec_amd.common.trainer import Trainer
    hyper = dict(HYPER[name], hip_deterministic=True, hip_graph_step=False, lazy_feature_adam=lazy_adam,
                 hip_gathered_projection=gathered)
    config, train_data, _, model = build_shape(root, name, "baby", hyper)
    assert model.gathered_projection == gathered and model.lazy_feature_adam == lazy_adam
    assert isinstance(model.image_embedding, LazyRowEmbedding) == lazy_adam
    assert {model.image_embedding.weight.shape[1], model.text_embedding.weight.shape[1]} == {4096, 384}
    try:
        trainer = Trainer(config, model)
        assert hip_ops.DETERMINISTIC
        if batches is None:
            batches = [b.clone() for b in itertools.islice(iter(train_data), 3)]
            assert len(batches) == 3 and not torch.equal(batches[0], batches[1])
        torch.manual_seed(4321)
        model.train()
        model.pre_epoch_processing()           # FREEDOM: the pruned graph (same draw in both runs)
        losses = []
        for step, batch in enumerate(batches):
            torch.manual_seed(1000 + step)     # BM3: the same dropout masks in both runs
            trainer.optimizer.zero_grad()
            loss = trainer._total(model.calculate_loss(batch.clone()))
            loss.backward()
            trainer.optimizer.step()
            losses.append(loss.detach().reshape(1).clone())
        flush_lazy_tables(model)
        torch.cuda.synchronize()
        return batches, torch.cat(losses).cpu(), {n: p.detach().cpu().clone() for n, p in model.named_parameters()}
    finally:
        hip_ops.set_deterministic(hip_ops.DETERMINISTIC_DEFAULT)


@pytest.mark.parametrize("lazy_adam", [False, True], ids=["dense_adam", "row_lazy_adam"])
@pytest.mark.parametrize("name", ["FREEDOM", "BM3"])
def test_gathered_projection_trains_bit_identically(tmp_path, name, lazy_adam):
    batches, loss_on, p_on = _three_steps(tmp_path / "on", name, lazy_adam, True)
    _, loss_off, p_off = _three_steps(tmp_path / "off", name, lazy_adam, False, batches)
    assert torch.equal(loss_on.view(torch.int32), loss_off.view(torch.int32)), (loss_on, loss_off)
    assert set(p_on) == set(p_off)
    for n in p_on:
        assert torch.equal(p_on[n].view(torch.int32), p_off[n].view(torch.int32)), \
            (n, int((p_on[n].view(torch.int32) != p_off[n].view(torch.int32)).sum()))
    moved = [n for n in p_on if n.endswith("_embedding.weight") and n.split("_")[0] in ("image", "text")]
    assert len(moved) == 2


def test_replayed_freedom_step_with_gathered_projection_equals_eager(tmp_path):
    """an epoch replayed as a hipGraph ends with the eager epoch's parameters (as tests/test_models_gpu.py::
    test_graphed_train_step_equals_eager), the key on, `hip_deterministic`"""
    from mmrec_amd import hip_ops
    from mmrec_amd.common.lazy_rows import flush_lazy_tables
    from mmrec_amd.common.trainer import Trainer
    results = []
    try:
        for graphed in (False, True):
            hyper = dict(HYPER["FREEDOM"], hip_deterministic=True, hip_graph_step=graphed, hip_gathered_projection=True)
            config, train_data, _, model = build_shape(tmp_path / str(graphed), "FREEDOM", "baby", hyper)
            assert model.gathered_projection
            torch.manual_seed(123)
            trainer = Trainer(config, model)
            assert trainer.optimizer.capturable == graphed
            model.pre_epoch_processing()
            total, _ = trainer._train_epoch(train_data, 0)
            assert (trainer._graphed_step(model.calculate_loss) is not None) == graphed
            if graphed:
                assert not trainer._graphed.failed
            flush_lazy_tables(model)
            results.append((total, [p.detach().cpu().numpy().copy() for p in model.parameters()]))
    finally:
        hip_ops.set_deterministic(hip_ops.DETERMINISTIC_DEFAULT)
    (t0, p0), (t1, p1) = results
    np.testing.assert_allclose(t1, t0, rtol=1e-5)
    for a, b in zip(p0, p1):
        np.testing.assert_allclose(b, a, rtol=1e-4, atol=1e-6)


@pytest.mark.parametrize("lazy_adam", [False, True], ids=["dense_adam", "row_lazy_adam"])
@pytest.mark.parametrize("name", ["FREEDOM", "BM3"])
def test_key_decides_which_projection_runs(tmp_path, monkeypatch, name, lazy_adam):
    from mmrec_amd import hip_ops
    from mmrec_amd.common.lazy_rows import LazyRowEmbedding
    calls = {"linear_rows": 0, "project_rows": 0, "select": 0}
    real_lr, real_pr = hip_ops.linear_rows, LazyRowEmbedding.project_rows

    def linear_rows(*a, **k):
        calls["linear_rows"] += 1
        return real_lr(*a, **k)

    def project_rows(self, *a, **k):
        calls["project_rows"] += 1
        return real_pr(self, *a, **k)
    monkeypatch.setattr(hip_ops, "linear_rows", linear_rows)
    monkeypatch.setattr(LazyRowEmbedding, "project_rows", project_rows)
    for gathered in (False, True):
        hyper = dict(HYPER[name], hip_graph_step=False, lazy_feature_adam=lazy_adam, hip_gathered_projection=gathered)
        config, train_data, _, model = build_shape(tmp_path / str(gathered), name, "baby", hyper)
        tables = {model.image_embedding.weight.data_ptr(), model.text_embedding.weight.data_ptr()}
        real_is, real_gi = torch.Tensor.index_select, torch.Tensor.__getitem__

        def index_select(self, *a, **k):
            calls["select"] += self.data_ptr() in tables and self.dim() == 2 and self.shape[1] in (4096, 384)
            return real_is(self, *a, **k)

        def getitem(self, idx):
            calls["select"] += (isinstance(idx, torch.Tensor) and self.data_ptr() in tables and self.dim() == 2 and
                                self.shape[1] in (4096, 384))
            return real_gi(self, idx)
        batch = next(iter(train_data))
        model.train()
        model.pre_epoch_processing()
        for k in calls:
            calls[k] = 0
        with monkeypatch.context() as m:
            m.setattr(torch.Tensor, "index_select", index_select)
            m.setattr(torch.Tensor, "__getitem__", getitem)
            loss = model.calculate_loss(batch)
            loss = loss if isinstance(loss, torch.Tensor) else sum(loss)
            loss.backward()
        torch.cuda.synchronize()
        if not gathered:
            assert calls["linear_rows"] == 0 and calls["project_rows"] == 0, calls
            assert calls["select"] == 2, calls                      # the two-step form gathers both tables' rows
        else:
            assert calls["project_rows" if lazy_adam else "linear_rows"] == 2, calls
            assert calls["linear_rows" if lazy_adam else "project_rows"] == 0, calls
            assert calls["select"] == 0, calls                      # no copy of the rows
