"""CPU: the neighbour max's torch composition (`hip_ops.neighbor_max_torch`) and DualGNN / DRAGON with `aggr_mode` 'mean' and
'max' against the reference's fixtures (tests/golden/make_golden_dual_aggr.py), with the op entry points swapped for the
torch-CPU restatements of tests/_cpu_ops.py.  `neighbor_max` itself is not swapped: on CPU tensors and on the stand-in's
DynGraph (rows, cols, n_rows, n_cols only) it takes its own composition, which is what is under test here.

THE SELECTION RULE (include/mmrec_hip.h): per (row, column) the first edge of the row, in edge-list order, whose value is NaN;
without a NaN the first that attains the maximum (-0 = +0); a row without edges gives 0 and arg = -1.

`dual_aggr_step` is shared with tests/test_neighbor_max_models_gpu.py, where the same body runs on the kernels."""
import numpy as np
import pytest
import torch

import tests.test_models_gpu as G
from tests._cpu_ops import cpu_ops  # noqa: F401  (fixture)
from tests.test_spmm_fuzz_gpu import gamma

EXTRA = {"DualGNN": {}, "DRAGON": {"n_mm_layers": 1, "knn_k": 10, "mm_image_weight": 0.1}}
TAGS = ("v1", "v2", "t1", "t2")                  # modality, hop: the four Base_gcn calls of a training step


def fixtures(name, mode):
    """(the 'add' run's fixture: dataset, user graph, initial parameters; the mode's; the mode's op records or None)"""
    base, fx = G._golden(name.lower()), G._golden(name.lower() + "_" + mode)
    return base, fx, (G._golden(name.lower() + "_max_ops") if mode == "max" else None)


def routed64(argsrc, gy, n):
    """float64 of the backward as a sum: ref[s][c] = sum of gy[r][c] over the r with argsrc[r][c] == s; -> (ref, sum |terms|,
    number of terms)"""
    ref, mag, cnt = np.zeros((n, 64)), np.zeros((n, 64)), np.zeros((n, 64))
    col = np.broadcast_to(np.arange(64), argsrc.shape)
    ok = argsrc >= 0
    np.add.at(ref, (argsrc[ok], col[ok]), gy[ok].astype(np.float64))
    np.add.at(mag, (argsrc[ok], col[ok]), np.abs(gy[ok].astype(np.float64)))
    np.add.at(cnt, (argsrc[ok], col[ok]), 1.0)
    return ref, mag, cnt


def check_routed(got, argsrc, gy, n, name):
    ref, mag, cnt = routed64(argsrc, gy, n)
    err, tol = np.abs(np.asarray(got, np.float64) - ref), gamma(cnt) * mag
    assert (err <= tol).all(), (name, int((err > tol).sum()), float(err.max()))


@pytest.mark.parametrize("name", ["DualGNN", "DRAGON"])
def test_composition_against_the_op_records(name):
    """x is the fixture's, so both sides see identical bits and no selection can differ: Y bit-equal, the chosen source equal
    everywhere, the gradient within gamma(m) sum |terms| of float64 of the recorded sum (m terms per element)"""
    from mmrec_amd import hip_ops
    base, fx, ops = fixtures(name, "max")
    src, dst = torch.from_numpy(base["edge_index"][0]), torch.from_numpy(base["edge_index"][1])
    n = int(base["edge_index"].max()) + 1
    col = np.arange(64)[None, :]
    for tag in TAGS:
        x, argsrc = ops["op_%s_x" % tag], fx["op_%s_argsrc" % tag]
        gy = ops["op_%s_gy" % tag].astype(np.float32) / 8.0
        X = torch.from_numpy(x).requires_grad_()
        Y, arg = hip_ops.neighbor_max_torch(X, dst, src, n)
        assert arg.dtype == torch.int32 and not arg.requires_grad and tuple(arg.shape) == (n, 64)
        assert np.array_equal(Y.detach().numpy().view(np.int32), x[argsrc, col].view(np.int32)), tag
        assert (arg >= 0).all()
        assert np.array_equal(src[arg.long()].numpy(), argsrc), tag
        Y.backward(torch.from_numpy(gy))
        check_routed(X.grad.numpy(), argsrc, gy, n, name + " " + tag)
        check_routed(ops["op_%s_gx" % tag], argsrc, gy, n, name + " " + tag + " (the record itself)")
        if tag.endswith("1"):                                 # hop 2 reads hop 1's output
            assert np.array_equal(Y.detach().numpy().view(np.int32), ops["op_%s2_x" % tag[0]].view(np.int32))


def tie_case():
    """node 0: three neighbours (3, 4, 5 in that order); node 1: none; node 2: neighbours 5, 4 (two NaNs: the first wins).
    columns of node 0:  0: first and third tied -> the first;  1: a NaN in second place -> the NaN;  2: -0 before +0 -> -0;
    3: +0 before -0 -> +0;  4: the third strictly greater;  5: -inf, -inf, -inf -> the first;  6: inf in third place"""
    nan, inf = np.nan, np.inf
    X = np.zeros((6, 64), np.float32)
    X[3, :7] = [1.0, 1.0, -0.0, 0.0, 1.0, -inf, 5.0]
    X[4, :7] = [0.5, nan, 0.0, -0.0, 2.0, -inf, nan]
    X[5, :7] = [1.0, 2.0, -1.0, -1.0, 3.0, -inf, inf]
    X[5, 7], X[4, 7] = nan, nan
    rows, cols = np.array([0, 2, 0, 0, 2], np.int64), np.array([3, 5, 4, 5, 4], np.int64)
    want_src = {0: [3, 4, 3, 3, 5, 3, 4], 2: [5, 4, 4, 4, 5, 5, 4, 5]}     # node 2, column 6: NaN (node 4, second) over inf
    return X, rows, cols, want_src


def check_tie_case(Y, arg, dX, X, rows, cols, want_src, dY):
    """the rule's answers on `tie_case`, for the composition and for the kernel alike (numpy arrays)"""
    for r, srcs in want_src.items():
        for c, s in enumerate(srcs):
            assert cols[arg[r, c]] == s and rows[arg[r, c]] == r, (r, c, int(arg[r, c]))
            assert Y[r, c:c + 1].view(np.int32) == X[s, c:c + 1].view(np.int32), (r, c)
    assert np.signbit(Y[0, 2]) and Y[0, 2] == 0 and not np.signbit(Y[0, 3])
    assert (arg[1] == -1).all() and (Y[1].view(np.int32) == 0).all()                       # the empty row
    assert (arg[0, 8:] == 0).all() and (arg[2, 8:] == 1).all()                             # all tied at 0: the first edge
    # the whole gradient goes to the chosen edge's source
    ref = np.zeros_like(X, dtype=np.float64)
    for r in (0, 2):
        for c in range(64):
            ref[cols[arg[r, c]], c] += dY[r, c]
    assert np.array_equal(dX.astype(np.float64), ref)


def test_tie_rule_by_hand():
    from mmrec_amd import hip_ops
    X, rows, cols, want_src = tie_case()
    dY = (np.arange(3 * 64).reshape(3, 64) % 17 - 8).astype(np.float32) / 8.0
    Xt = torch.from_numpy(X).requires_grad_()
    Y, arg = hip_ops.neighbor_max_torch(Xt, torch.from_numpy(rows), torch.from_numpy(cols), 3)
    Y.backward(torch.from_numpy(dY))
    check_tie_case(Y.detach().numpy(), arg.numpy(), Xt.grad.numpy(), X, rows, cols, want_src, dY)
    # no edges at all
    Y, arg = hip_ops.neighbor_max_torch(Xt, torch.zeros(0, dtype=torch.int64), torch.zeros(0, dtype=torch.int64), 3)
    assert (Y == 0).all() and (arg == -1).all() and tuple(Y.shape) == (3, 64)


def test_neighbor_max_on_the_stand_in_graph(cpu_ops):  # noqa: F811
    """`neighbor_max` on CPU tensors over the stand-in DynGraph (rows, cols, n_rows, n_cols only) is the composition"""
    from mmrec_amd import hip_ops
    X, rows, cols, want_src = tie_case()
    dyn = cpu_ops.DynGraph(torch.from_numpy(rows), torch.from_numpy(cols), 3, 6)
    Xt = torch.from_numpy(X)
    assert not hip_ops.neighbor_max_served(Xt, dyn)
    Y, arg = hip_ops.neighbor_max(Xt, dyn)
    Y2, arg2 = hip_ops.neighbor_max_torch(Xt, dyn.rows, dyn.cols, dyn.n_rows)
    assert torch.equal(Y.view(torch.int32), Y2.view(torch.int32)) and torch.equal(arg, arg2)


# ------------------------------------------------------------------------------------------------ the models
def arg_sources(model, gcn, hop):
    """last_arg (positions in the DynGraph's edge list) -> source nodes; the list has no duplicate edges, so positions map
    one-to-one to (target, source) pairs"""
    a = gcn.last_arg[hop].cpu().long()
    assert (a >= 0).all()
    return model.graph.cols.cpu()[a].numpy()


def flips(model, fx, ops):
    """The positions where the model's argmax differs from the fixture's; every one must have a fixture margin of at most
    1e-4 |max| + 2e-6 -- the forward tolerance the project accepts for these models, so a flip anywhere else is a wrong kernel
    (and one at a large margin among exactly tied entries a broken tie rule).  -> their number"""
    col = np.arange(64)[None, :]
    total = 0
    for tag in TAGS:
        gcn = model.v_gcn if tag[0] == "v" else model.t_gcn
        mine, ref = arg_sources(model, gcn, int(tag[1]) - 1), fx["op_%s_argsrc" % tag]
        diff = mine != ref
        top = ops["op_%s_x" % tag][ref, col]
        bad = diff & ~(fx["op_%s_margin" % tag] <= 1e-4 * np.abs(top) + 2e-6)
        assert not bad.any(), (tag, "argmax differs beyond the forward tolerance at", int(bad.sum()), "of", int(diff.sum()),
                               "differing positions; smallest such margin", float(fx["op_%s_margin" % tag][bad].min()))
        total += int(diff.sum())
    return total


def dual_aggr_step(tmp_path, golden, name, mode, before_step=None):
    """one training step of `name` with `aggr_mode = mode` from the reference's state against the mode's fixture"""
    from mmrec_amd import hip_ops
    base, fx, ops = fixtures(name, mode)
    G._write_user_graph(tmp_path, base)
    cfg = {"reg_weight": 1e-3, "learning_rate": 1e-3, "aggr_mode": mode}
    cfg.update(EXTRA[name])
    config, _, valid_data, model = G.build(tmp_path, golden, name, cfg)
    assert model.aggr_mode == mode and model.v_gcn.aggr_mode == mode
    params = dict(model.named_parameters())
    assert set(params) == {k[2:] for k in base if k.startswith("p_")}
    assert int(np.random.get_state()[2]) == int(base["np_pos_after_init"])
    for pname, p in params.items():
        G.load(p, base["p_" + pname])
    if name == "DRAGON":                                      # the reference's kNN item graph, as its cache file would provide it
        model.mm_adj = hip_ops.CsrGraph.from_coo_host(base["mm_adj_idx"], base["mm_adj_val"], model.n_items, model.n_items,
                                                      model.device)
        model.mm_adj.transpose()
    model.pre_epoch_processing()
    np.testing.assert_array_equal(model.epoch_user_graph, base["epoch_user_graph"])
    if before_step is not None:
        before_step(model)
    loss = model.calculate_loss(torch.as_tensor(base["batch1"]).to(model.device))
    loss.backward()
    G.close(model.result_embed, fx["result"], rtol=1e-4, atol=2e-6)
    G.close(loss, fx["loss1"], rtol=1e-5)
    grads = {k[2:] for k in fx if k.startswith("g_")}
    now = dict(model.named_parameters())
    assert {n for n, p in now.items() if p.grad is not None} == grads
    n_flips = flips(model, fx, ops) if mode == "max" else 0
    if n_flips == 0:
        for pname in grads:
            G.close(now[pname].grad, fx["g_" + pname], rtol=5e-4, atol=2e-7)
    else:       # near-ties within the forward tolerance resolved the other way: the gradient is routed elsewhere there
        print("%s %s: %d argmax positions differ within the forward tolerance; gradients not compared" % (name, mode, n_flips))
    model.eval()
    users, mask = next(iter(valid_data))
    for _ in valid_data:
        pass
    G.close(model.full_sort_predict([users, mask]), fx["scores_first_batch"], rtol=1e-4, atol=2e-6)
    return model, n_flips


@pytest.fixture
def on_cpu(cpu_ops, monkeypatch):  # noqa: F811
    monkeypatch.setattr(G, "USE_GPU", False)


@pytest.mark.parametrize("mode", ["mean", "max"])
@pytest.mark.parametrize("name", ["DualGNN", "DRAGON"])
def test_dual_family_aggr_modes(tmp_path, golden, on_cpu, name, mode):
    model, n_flips = dual_aggr_step(tmp_path, golden, name, mode)
    if mode == "max":
        assert [tuple(a.shape) for a in model.v_gcn.last_arg] == [(model.n_users + model.n_items, 64)] * 2
        assert not model.v_gcn.last_arg[0].requires_grad
    else:
        assert model.v_gcn.last_arg is None and not model.graph.symmetric


@pytest.mark.parametrize("name", ["DualGNN", "DRAGON"])
def test_unknown_aggr_mode_is_a_value_error(tmp_path, golden, on_cpu, name):
    G._write_user_graph(tmp_path, G._golden(name.lower()))
    cfg = {"reg_weight": 1e-3, "learning_rate": 1e-3, "aggr_mode": "softmax"}
    cfg.update(EXTRA[name])
    with pytest.raises(ValueError, match="'add', 'mean', 'max'"):
        G.build(tmp_path, golden, name, cfg)
