"""GPU: DualGNN and DRAGON with `aggr_mode` 'mean' and 'max' on the HIP kernels against the reference's fixtures
(tests/golden/make_golden_dual_aggr.py; the test body is tests/test_neighbor_max_cpu.py's `dual_aggr_step`), the neighbour-max
kernels against their torch composition inside the models, the op's memory, and `aggr_mode='add'` against the code it
replaces."""
import numpy as np
import pytest
import torch

import tests.test_models_gpu as G
from tests.test_neighbor_max_cpu import dual_aggr_step

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("mode", ["mean", "max"])
@pytest.mark.parametrize("name", ["DualGNN", "DRAGON"])
def test_dual_family_aggr_modes_on_the_kernels(tmp_path, golden, name, mode, monkeypatch):
    from mmrec_amd import _lib, hip_ops
    lib, calls = _lib.load(), []
    for fn in ("mmrec_neighbor_max_f32", "mmrec_neighbor_max_bwd_f32"):
        monkeypatch.setattr(lib, fn, lambda *a, _real=getattr(lib, fn), _fn=fn: calls.append(_fn) or _real(*a))
    model, n_flips = dual_aggr_step(tmp_path, golden, name, mode)
    assert model.device.type == "cuda"
    if mode == "max":                                         # two modalities x two hops, forward and backward, on the kernels
        assert isinstance(model.graph, hip_ops.DynGraph)
        assert calls.count("mmrec_neighbor_max_f32") == 4 and calls.count("mmrec_neighbor_max_bwd_f32") == 4
    else:
        assert not calls and isinstance(model.graph, hip_ops.CsrGraph) and not model.graph.symmetric


@pytest.mark.parametrize("name", ["DualGNN", "DRAGON"])
def test_max_kernels_equal_the_composition_inside_the_model(tmp_path, golden, name, monkeypatch):
    """the same step with NEIGHBOR_MAX on and off: the inputs of every call are bitwise the same, so the argmax must be equal
    everywhere and `result` bit-equal; the parameter gradients differ by summation order only"""
    from mmrec_amd import hip_ops
    runs = []
    for on in (True, False):
        monkeypatch.setattr(hip_ops, "NEIGHBOR_MAX", on)
        model, _ = dual_aggr_step(tmp_path / ("on" if on else "off"), golden, name, "max")
        runs.append(model)
    a, b = runs
    for gcn in ("v_gcn", "t_gcn"):
        for hop in range(2):
            assert torch.equal(getattr(a, gcn).last_arg[hop], getattr(b, gcn).last_arg[hop]), (gcn, hop)
    assert torch.equal(a.result_embed.view(torch.int32), b.result_embed.view(torch.int32))
    pa, pb = dict(a.named_parameters()), dict(b.named_parameters())
    for n, p in pa.items():
        if p.grad is not None:
            G.close(p.grad, pb[n].grad.cpu().numpy(), rtol=5e-4, atol=2e-7)


def test_no_edge_sized_tensor():
    """2,048 rows x 200,000 edges (one [E, 64] fp32 tensor would be 51 MB): the peak allocation of forward + backward above the
    resident inputs stays below 8 MB (Y, arg and dX are 1.5 MB)"""
    from mmrec_amd import hip_ops
    rng = np.random.default_rng(3)
    n, ne = 2048, 200000
    rows = torch.from_numpy(rng.integers(0, n, ne)).cuda()
    cols = torch.from_numpy(rng.integers(0, n, ne)).cuda()
    dyn = hip_ops.DynGraph(rows, cols, n, n)
    X = torch.from_numpy(rng.standard_normal((n, 64)).astype(np.float32)).cuda().requires_grad_()
    dY = torch.from_numpy(rng.standard_normal((n, 64)).astype(np.float32)).cuda()
    assert hip_ops.neighbor_max_served(X, dyn)
    hip_ops.neighbor_max(X, dyn)[0].backward(dY)              # (the long lists are built at the first call)
    first = X.grad.clone()
    X.grad = None
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    resident = torch.cuda.memory_allocated()
    Y, arg = hip_ops.neighbor_max(X, dyn)
    Y.backward(dY)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - resident
    print("neighbor_max forward + backward at %d rows x %d edges: peak %.2f MB above the inputs" % (n, ne, peak / 2 ** 20))
    assert peak < 8 * 2 ** 20, peak
    assert torch.equal(first, X.grad) and float(X.grad.abs().max()) > 0
    chosen = cols[arg.long().clamp(min=0)]                    # spot check: Y is X at the chosen edges
    assert torch.equal(torch.where(arg >= 0, X.detach()[chosen, torch.arange(64, device="cuda")[None, :]],
                                   torch.zeros((), device="cuda")), Y.detach())


def test_add_is_bitwise_the_code_it_replaces(tmp_path, golden, monkeypatch):
    """`aggr_mode='add'` on the dualgnn.npz step: the graph is `sym_norm_graph`'s, and `result` and every parameter gradient
    have the bits of the model with the parent commit's GCN.forward (restated here) in its place -- in deterministic mode,
    where the fused loss kernels' scatters do not depend on the order of atomics"""
    import torch.nn.functional as F
    from mmrec_amd import hip_ops
    from mmrec_amd.models import dualgnn
    from mmrec_amd.models.mmgcn import _lin64

    def parent_forward(self, graph, features):
        temp = _lin64(self.MLP_1, F.leaky_relu(_lin64(self.MLP, features)))
        x = F.normalize(torch.cat((self.preference, temp), dim=0))
        return hip_ops.lightgcn_mean(graph, x, 2) * 3.0, self.preference

    base = G._golden("dualgnn")
    outs = []
    try:
        hip_ops.set_deterministic(True)
        for parent in (False, True):
            if parent:
                monkeypatch.setattr(dualgnn.GCN, "forward", parent_forward)
            root = tmp_path / ("parent" if parent else "now")
            G._write_user_graph(root, base)
            config, train_data, _, model = G.build(root, golden, "DualGNN",
                                                   {"reg_weight": 1e-3, "learning_rate": 1e-3, "aggr_mode": "add"})
            for pname, p in model.named_parameters():
                G.load(p, base["p_" + pname])
            if parent:
                inter = train_data.inter_matrix(form='coo').astype(np.float32)
                model.graph = dualgnn.sym_norm_graph(inter, model.n_users, model.n_items, model.device)
            model.pre_epoch_processing()
            model.calculate_loss(torch.as_tensor(base["batch1"]).to(model.device)).backward()
            g = model.graph
            outs.append((model.result_embed.clone(), {n: p.grad.clone() for n, p in model.named_parameters() if p.grad is not None},
                         (g.rowptr.clone(), g.colidx.clone(), g.vals.clone(), g.symmetric)))
    finally:
        hip_ops.set_deterministic(False)
        torch.use_deterministic_algorithms(False)
    (res_a, grads_a, graph_a), (res_b, grads_b, graph_b) = outs
    assert graph_a[3] and graph_b[3] and all(torch.equal(x, y) for x, y in zip(graph_a[:3], graph_b[:3]))
    G.close(res_a, base["result"], rtol=1e-4, atol=2e-6)
    assert torch.equal(res_a.view(torch.int32), res_b.view(torch.int32))
    assert set(grads_a) == set(grads_b) == {k[2:] for k in base if k.startswith("g_")}
    for n in grads_a:
        assert torch.equal(grads_a[n].view(torch.int32), grads_b[n].view(torch.int32)), n
