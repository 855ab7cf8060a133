"""GPU: LATTICE and GRCN with the per-edge dot products on the SDDMM kernel (hip_ops.edge_dot, mmrec_edge_dot_f32) and with
`hip_ops.EDGE_DOT` off (the gather-multiply-reduce composition), on the tiny golden dataset: one training step from the same
seed gives the same loss and parameter gradients within the project's fp32 tolerance (1e-4 relative, README: parity), the
switch decides which code runs, no [n_edges, d] gathered copy is made in the backward of the on path, and the step is still
capturable -- the ops under torch.cuda.graph, and a replayed LATTICE epoch against the eager one."""
import numpy as np
import pytest
import torch

from tests.test_models_gpu import build
from tests.test_spmm_fuzz_gpu import _grid, _on

pytestmark = pytest.mark.gpu

EXTRA = {"LATTICE": {"reg_weight": 1e-3, "learning_rate": 1e-3, "n_layers": 1, "cf_model": "lightgcn"},
         "GRCN": {"reg_weight": 1e-3, "learning_rate": 1e-3, "n_layers": 3}}
RTOL = 1e-4


def _one_step(tmp_path, golden, name, monkeypatch, on, batch=None):
    """one loss + backward on the first batch of an epoch (LATTICE: the graph-building one) -> the batch, the loss, every
    parameter gradient, the library calls of the SDDMM entry points, and the [n_edges, d] gathers seen during the backward"""
    from mmrec_amd import _lib, hip_ops
    lib = _lib.load()
    calls = {"mmrec_edge_dot_f32": 0, "mmrec_edge_dot_bwd_f32": 0, "gathers_fwd": 0, "gathers_bwd": 0}
    with monkeypatch.context() as m:
        m.setattr(hip_ops, "EDGE_DOT", on)
        for fn in ("mmrec_edge_dot_f32", "mmrec_edge_dot_bwd_f32"):
            def spy(*a, _real=getattr(lib, fn), _fn=fn):
                calls[_fn] += 1
                return _real(*a)
            m.setattr(lib, fn, spy)
        config, train_data, _, model = build(tmp_path, golden, name, EXTRA[name])
        if batch is None:
            batch = next(iter(train_data)).clone()
        model.train()
        model.pre_epoch_processing()
        edge_counts = set()
        real_gi = torch.Tensor.__getitem__
        phase = ["gathers_fwd"]

        def getitem(self, idx):
            out = real_gi(self, idx)
            if (isinstance(idx, torch.Tensor) and idx.dim() == 1 and self.dim() == 2 and self.is_floating_point() and
                    self.shape[1] == 64 and idx.numel() in edge_counts):
                calls[phase[0]] += 1
            return out
        if name == "GRCN":
            edge_counts.add(model.edges.dst.numel())
        else:
            edge_counts.add(model.n_items * model.knn_k)              # one modality's kNN pairs
        with monkeypatch.context() as m2:
            m2.setattr(torch.Tensor, "__getitem__", getitem)
            torch.manual_seed(77)
            loss = model.calculate_loss(batch.clone())
            loss = sum(loss) if isinstance(loss, tuple) else loss
            if name == "LATTICE":
                edge_counts.add(model.item_adj[0].rows.numel())       # learned + original pairs: the spmm_vals structure
            phase[0] = "gathers_bwd"
            loss.backward()
        torch.cuda.synchronize()
        grads = {n: (None if p.grad is None else p.grad.detach().cpu().double().numpy().copy())
                 for n, p in model.named_parameters()}
    return batch, float(loss), grads, calls


@pytest.mark.parametrize("name", ["LATTICE", "GRCN"])
def test_one_step_with_the_kernel_equals_the_composition(tmp_path, golden, monkeypatch, name):
    batch, loss_on, g_on, calls_on = _one_step(tmp_path / "on", golden, name, monkeypatch, True)
    _, loss_off, g_off, calls_off = _one_step(tmp_path / "off", golden, name, monkeypatch, False, batch)
    print("%s: loss on %.9g off %.9g; calls on %s off %s" % (name, loss_on, loss_off, calls_on, calls_off))
    # the switch decides which code runs
    # LATTICE: the similarities of both modalities + d vals of the one spmm_vals layer; GRCN: the scores of both modalities +
    # d vals of its four spmm_vals calls
    assert calls_on["mmrec_edge_dot_f32"] >= (2 + 1 if name == "LATTICE" else 2 + 4), calls_on
    assert calls_off["mmrec_edge_dot_f32"] == 0 and calls_off["mmrec_edge_dot_bwd_f32"] == 0, calls_off
    if name == "GRCN":                                                # the scores' backward is the SpMM over edges.dyn: no atomics
        assert calls_on["mmrec_edge_dot_bwd_f32"] == 0, calls_on
    # no [n_edges, d] gathered copy on the kernel path, forward or backward; the composition makes them (the spy sees them)
    assert calls_on["gathers_fwd"] == 0 and calls_on["gathers_bwd"] == 0, calls_on
    assert calls_off["gathers_fwd"] > 0 and calls_off["gathers_bwd"] > 0, calls_off
    assert abs(loss_on - loss_off) <= RTOL * abs(loss_off), (loss_on, loss_off)
    assert set(g_on) == set(g_off)
    moved = 0
    for n in sorted(g_on):
        a, b = g_on[n], g_off[n]
        assert (a is None) == (b is None), n
        if a is None:
            continue
        scale = float(np.abs(b).max())
        diff = float(np.abs(a - b).max())
        print("  %-32s |grad| max %.3e  max diff %.3e  ratio %.3e" % (n, scale, diff, diff / scale if scale else 0.0))
        assert np.isfinite(a).all() and diff <= RTOL * scale, (n, diff, scale)
        moved += scale > 0
    assert moved >= 4
    if name == "LATTICE":                                             # the similarities' gradient reaches the projections
        for n in ("image_trs.weight", "text_trs.weight", "modal_weight"):
            assert np.abs(g_on[n]).max() > 0, n


def test_ops_are_capturable_and_replay_the_eager_bits():
    """edge_dot forward + both backward forms and spmm_vals' backward recorded into a hipGraph and replayed: the eager results
    (exact-grid inputs: every summation order gives the same numbers)"""
    from mmrec_amd import hip_ops
    rng = np.random.default_rng(11)
    n, d, ne = 700, 64, 9000
    A0 = _grid(rng, (n, d))
    r, k = rng.integers(0, n, ne), rng.integers(0, n, ne)
    r[:2000] = 5
    g0 = (rng.integers(-8, 9, ne) / 8.0).astype(np.float32)
    rows, cols, gt = _on(r), _on(k), _on(g0)
    dyn = hip_ops.DynGraph(rows, cols, n, n)
    A = _on(A0).requires_grad_()
    v = _on(g0).requires_grad_()

    def step():
        out_a = hip_ops.edge_dot(A, A, rows, cols)
        out_d = hip_ops.edge_dot(A, A, rows, cols, dyn=dyn)
        y = hip_ops.spmm_vals(dyn, A, v)
        (ga,) = torch.autograd.grad(out_a, A, gt)
        (gd,) = torch.autograd.grad(out_d, A, gt)
        gx, gv = torch.autograd.grad(y, (A, v), A.detach())
        return [out_a, out_d, ga, gd, gx, gv]
    eager = [t.detach().clone() for t in step()]
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        static = step()
    for t in static:
        t.detach().zero_()
    graph.replay()
    graph.replay()
    torch.cuda.synchronize()
    for i, (a, b) in enumerate(zip(eager, static)):
        assert torch.equal(a, b.detach()), i
    assert torch.equal(eager[0], eager[1]) and torch.equal(eager[2], eager[3])
    assert float(eager[2].abs().max()) > 0 and float(eager[5].abs().max()) > 0


def test_replayed_lattice_epoch_gives_the_eager_losses(tmp_path, golden):
    """`hip_graph_step`: LATTICE's first batch of an epoch builds the learned graph (edge_dot, its backward) eagerly, the rest
    of the epoch is one capture replayed -- the per-batch losses are the eager epoch's"""
    from mmrec_amd.common.trainer import Trainer
    runs = []
    for graphed in (False, True):
        extra = dict(EXTRA["LATTICE"], train_batch_size=64, hip_graph_step=graphed)
        config, train_data, _, model = build(tmp_path / str(graphed), golden, "LATTICE", extra)
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
    assert l0.size >= 4 and l0.size == l1.size                        # the graph-building batch + three or more replayed ones
    print("eager", l0, "graphed", l1)
    np.testing.assert_allclose(l1, l0, rtol=1e-5)
    np.testing.assert_allclose(t1, t0, rtol=1e-5)
