"""No GPU: the pseudo-label kernels' exports, argument checks and plan (csrc/tri_topk.hip); hip_ops.pseudo_labels on CPU tensors
is DAMRS._pseudo_labels list for list; the identity behind the second list (top-k of a softmax row with k entries zeroed = the
first k of the row's top-2k cosines that are not among them) in float64; DAMRS's `fused_labels` key absent / False / True on the
CPU; and the checker of tests/test_pseudo_labels_fuzz_gpu.py held honest: the fp32 torch composition passes it on the fuzz's own
cases within the leniency cap, six planted errors do not."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import tests.test_models_gpu as G
import tests.test_pseudo_labels_fuzz_gpu as Z
from mmrec_amd import _lib
from tests._cpu_ops import cpu_ops  # noqa: F401  (fixture)
from tests.test_hyper_cpu import lib  # noqa: F401  (fixture)

EXPORTS = ("mmrec_tri_topk_split_cols", "mmrec_tri_topk_workspace_bytes", "mmrec_tri_topk_f32", "mmrec_list_exclude_i32")
BAD, UNSUPPORTED = 10001, 10002
DAMRS_EXTRA = {"learning_rate": 1e-3, "kl_weight": 1, "neighbor_weight": 0.01, "n_mm_layers": 1, "n_ui_layers": 2, "knn_k": 10}
TARGETS = ((1, 2, 0), (0, 2, 1), (0, 1, 2))          # (the two others, the target) in the operand order of DAMRS.calculate_loss


def test_exports_in_header_signatures_and_library(lib):  # noqa: F811
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mmrec_hip.h")).read()
    for name in EXPORTS:
        assert name in _lib.SIGNATURES and name in src and hasattr(lib, name), name
    assert "#define MMREC_ABI_VERSION 16" in src and lib.mmrec_abi_version() == 16 and _lib.ABI_VERSION == 16   # additive
    from mmrec_amd.build import SOURCES
    assert "tri_topk.hip" in SOURCES


def test_hip_ops_has_the_entry_points():
    from mmrec_amd import hip_ops
    for name in ("pseudo_labels", "pseudo_labels_torch", "tri_softmax_topk", "tri_softmax_topk_torch", "tri_softmax_topk_served",
                 "list_exclude"):
        assert callable(getattr(hip_ops, name)), name
    assert hip_ops.TRI_TOPK is True


def test_entry_points_refuse_bad_arguments_before_touching_memory(lib):  # noqa: F811
    """every call below would fault if a pointer were followed or a kernel launched: this machine has no device"""
    f, x = lib.mmrec_tri_topk_f32, lib.mmrec_list_exclude_i32
    one = 1                                                                # a non-NULL pointer that must never be followed
    ok = dict(T0=one, T1=one, T2=one, N=50, ids=one, B=7, lse=one, W=one, k=10, out=one, val=None, ws=one)

    def call(**kw):
        a = dict(ok, **kw)
        return f(a["T0"], a["T1"], a["T2"], a["N"], a["ids"], a["B"], a["lse"], a["W"], a["k"], a["out"], a["val"], a["ws"], None)
    for k in (0, -1, 17, 64):
        assert call(k=k) == BAD, k
    assert call(N=9) == BAD and call(N=-1) == BAD and call(B=-1) == BAD    # N < k, negative sizes
    for hole in ("T0", "T1", "T2", "lse"):
        assert call(**{hole: None}) == BAD, hole
        assert call(**{hole: None, "B": 0}) == BAD, hole                   # ... before the empty batch is looked at
    assert call(N=(1 << 30) + 1) == UNSUPPORTED and call(B=(1 << 30) + 1) == UNSUPPORTED
    assert call(B=0, W=None, out=None, ws=None, ids=None) == 0             # no rows: nothing to do, nothing touched
    for hole in ("W", "out", "ws"):
        assert call(**{hole: None}) == BAD, hole
    assert x(one, one, 5, 20, 10, 11, one, None) == BAD                    # kc - ke < k
    assert x(one, one, 5, 20, 10, 0, one, None) == BAD and x(one, one, -1, 20, 10, 10, one, None) == BAD
    assert x(one, one, 5, -1, 0, 1, one, None) == BAD and x(one, one, 5, 20, -1, 1, one, None) == BAD
    assert x(None, None, 0, 20, 10, 10, None, None) == 0                   # no rows
    assert x(None, one, 5, 20, 10, 10, one, None) == BAD and x(one, one, 5, 20, 10, 10, None, None) == BAD
    assert x(one, None, 5, 20, 10, 10, one, None) == BAD


def test_plan_and_workspace(lib):  # noqa: F811
    """the plan is a function of the two sizes alone: whole 64-column tiles per split, at most 32 splits (32 x 16 merge slots)"""
    assert lib.mmrec_tri_topk_split_cols(-1, 5) == 0 and lib.mmrec_tri_topk_split_cols(5, 0) == 0
    for B in (1, 128, 129, 4096, 70000):
        for N in (1, 16, 64, 65, 97, 700, 3000, 7050, 18357, 500000):
            s = lib.mmrec_tri_topk_split_cols(B, N)
            splits = -(-N // s)
            assert s >= 64 and s % 64 == 0 and 1 <= splits <= 32, (B, N, s)
            row_tiles = -(-B // 128)
            assert splits == min(-(-N // 64), 32, -(-512 // row_tiles)) or splits * s >= N > (splits - 1) * s, (B, N, s)
            assert (splits == 1) == (N <= 64 or row_tiles >= 512), (B, N, s)
            for k in (1, 10, 16):
                assert lib.mmrec_tri_topk_workspace_bytes(B, N, k) == 8 * splits * 3 * B * k
    assert lib.mmrec_tri_topk_workspace_bytes(5, 50, 17) == 0 and lib.mmrec_tri_topk_workspace_bytes(5, 50, 0) == 0
    assert lib.mmrec_tri_topk_workspace_bytes(0, 50, 10) == 0
    big = (1 << 30) + 1                                              # beyond what the kernels index: no plan, no workspace
    assert lib.mmrec_tri_topk_split_cols(5, big) == 0 and lib.mmrec_tri_topk_split_cols(big, 50) == 0
    assert lib.mmrec_tri_topk_workspace_bytes(5, big, 10) == 0 and lib.mmrec_tri_topk_workspace_bytes(big, 50, 10) == 0
    assert lib.mmrec_tri_topk_split_cols(1 << 30, 1 << 30) == 1 << 30


def test_served_is_about_device_dtype_shape_and_width():
    from mmrec_amd import hip_ops

    class OnDevice(torch.Tensor):                                    # a stand-in that says it lives on the device
        is_cuda = True
    dev = lambda t: t.as_subclass(OnDevice)                          # noqa: E731
    T = [torch.zeros(30, 64) for _ in range(3)]
    ids, lse, W = torch.zeros(7, dtype=torch.int64), torch.zeros(3, 7), torch.ones(3, 3)
    served = hip_ops.tri_softmax_topk_served
    assert not served(T, ids, lse, W, 10)                            # CPU tensors: never
    dT = [dev(t) for t in T]
    assert served(dT, dev(ids), dev(lse), dev(W), 10) and served(dT, None, dev(lse), dev(W), 16)
    assert not served(dT, dev(ids), dev(lse), dev(W), 17) and not served(dT, dev(ids), dev(lse), dev(W), 0)
    assert not served(dT, dev(ids), dev(lse), dev(W), 31)        # k > 16 (and > N)
    assert not served(dT[:2], dev(ids), dev(lse), dev(W), 10)
    assert not served([dT[0], dT[1], T[2]], dev(ids), dev(lse), dev(W), 10)
    assert not served([dT[0], dT[1], dev(torch.zeros(30, 128))], dev(ids), dev(lse), dev(W), 10)
    assert not served([dT[0], dT[1], dev(torch.zeros(29, 64))], dev(ids), dev(lse), dev(W), 10)
    assert not served([dT[0], dT[1], dev(torch.zeros(30, 128)[:, ::2])], dev(ids), dev(lse), dev(W), 10)
    assert not served([dT[0], dT[1], dev(torch.zeros(30, 64).double())], dev(ids), dev(lse), dev(W), 10)
    assert not served(dT, dev(ids.int()), dev(lse), dev(W), 10) and not served(dT, dev(ids[:6]), dev(lse), dev(W), 10)
    assert not served(dT, dev(ids), dev(lse.double()), dev(W), 10) and not served(dT, dev(ids), dev(lse), dev(torch.ones(3, 4)), 10)
    try:
        hip_ops.TRI_TOPK = False
        assert not served(dT, dev(ids), dev(lse), dev(W), 10)
    finally:
        hip_ops.TRI_TOPK = True


# ------------------------------------------------------------------------------------------------ the composition on the CPU
def _tables(seed, n, clustered=False, dtype=torch.float32):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(3):
        if clustered:
            centres = rng.standard_normal((max(2, n // 15), 64))
            x = centres[rng.integers(0, centres.shape[0], n)] + 0.2 * rng.standard_normal((n, 64))
        else:
            x = rng.standard_normal((n, 64))
        out.append(F.normalize(torch.from_numpy(x).to(dtype), dim=1))
    return out


@pytest.mark.parametrize("seed,n,b,clustered", [(1, 300, 77, False), (2, 257, 257, True), (3, 20, 20, False), (4, 19, 11, False)])
def test_pseudo_labels_on_cpu_tensors_is_the_models_composition(seed, n, b, clustered):
    """hip_ops.pseudo_labels on CPU tensors (and for N < 2 k) returns exactly DAMRS._pseudo_labels' lists for all three targets"""
    from mmrec_amd import hip_ops
    from mmrec_amd.models.damrs import DAMRS
    T = _tables(seed, n, clustered)
    ids = torch.from_numpy(np.sort(np.random.default_rng(seed).permutation(n)[:b]))
    k = 10 if n >= 20 else 9
    mm, single = hip_ops.pseudo_labels(T, ids, k) if k != 10 else hip_ops.pseudo_labels(T, ids)
    assert mm.shape == single.shape == (3, b, k) and mm.dtype == single.dtype == torch.int64
    p = [F.softmax(torch.mm(t[ids], t.t()), dim=1) for t in T]
    for a, o, m in TARGETS:
        if k == 10:
            ref = DAMRS._pseudo_labels(p[a], p[o], p[m])
        else:
            top = torch.topk(p[a] + p[o] + p[m] + p[m], k, dim=-1).indices
            ref = (top, torch.topk(p[m].scatter(1, top, 0.0), k, dim=-1).indices)
        assert torch.equal(mm[m], ref[0]) and torch.equal(single[m], ref[1]), m


@pytest.mark.parametrize("seed,n,b,clustered", [(11, 700, 200, False), (12, 700, 200, True), (13, 3000, 150, True), (14, 20, 20, False),
                                                (15, 20, 20, True)])
def test_second_list_is_the_top_2k_minus_the_first_in_float64(seed, n, b, clustered):
    """scatter-then-topk of a softmax row = the first k of the row's top-2k cosines that are not in the first list: p > 0 and is
    monotone in the cosine within a row (float64: no two cosines of a row collapse to one probability); N = 20 = 2 k included"""
    T = _tables(seed, n, clustered, torch.float64)
    ids = torch.from_numpy(np.random.default_rng(seed).permutation(n)[:b])
    k = 10
    c = [torch.mm(t[ids], t.t()) for t in T]
    p = [torch.softmax(x, dim=1) for x in c]
    for a, o, m in TARGETS:
        mm_pos = torch.topk(p[a] + p[o] + 2 * p[m], k, dim=-1).indices
        want = torch.topk(p[m].scatter(1, mm_pos, 0.0), k, dim=-1).indices
        top2k = torch.sort(c[m], dim=1, descending=True, stable=True).indices[:, :2 * k]
        got = torch.stack([torch.tensor([j for j in top2k[r].tolist() if j not in set(mm_pos[r].tolist())][:k]) for r in range(b)])
        assert float(p[m].min()) > 0.0
        assert torch.equal(got, want), (m, int((got != want).any(dim=1).sum()))


def test_tri_softmax_topk_torch_is_the_first_list_and_marks_bad_ids():
    from mmrec_amd import hip_ops
    T = _tables(21, 120)
    ids = torch.tensor([5, 119, 0, 120, -1, 7, 7])
    safe = ids.clamp(0, 119)
    lse = torch.stack([torch.logsumexp(t[safe] @ t.t(), dim=1) for t in T])
    W = torch.ones(3, 3) + torch.eye(3)
    idx, val = hip_ops.tri_softmax_topk(T, ids, lse, W, 10, return_values=True)
    assert idx.dtype == torch.int64 and idx.shape == val.shape == (3, 7, 10)
    assert bool((idx[:, 3:5] == -1).all()) and bool(torch.isneginf(val[:, 3:5]).all())
    assert torch.equal(idx[:, 5], idx[:, 6])
    good = torch.tensor([0, 1, 2, 5])
    mm = hip_ops.pseudo_labels_torch(T, ids[good], 10)[0]
    assert torch.equal(idx[:, good], mm)
    assert bool((val[:, good][:, :, :-1] >= val[:, good][:, :, 1:]).all())
    assert torch.equal(hip_ops.tri_softmax_topk(T, None, lse[:, :3].contiguous(), W, 4),
                       hip_ops.tri_softmax_topk(T, torch.arange(3), lse[:, :3].contiguous(), W, 4))


# ------------------------------------------------------------------------------------------------ the model key on the CPU
def damrs_step(tmp_path, golden, extra, before_loss=None):
    """test_damrs_model's set-up (the reference's graphs and parameters, its first batch) with extra config keys -> (model, loss,
    {name: gradient}); tests/test_pseudo_labels_models_gpu.py runs the same on the device"""
    from mmrec_amd import hip_ops
    g = G._golden("damrs")
    rp, ids = g["ig_rowptr"], g["ig_ids"].tolist()
    missing = set(g["ig_missing"].tolist())
    item_graph = {i: [ids[rp[i]:rp[i + 1]], [1.0] * int(rp[i + 1] - rp[i])] for i in range(len(rp) - 1) if i not in missing}
    os.makedirs(os.path.join(str(tmp_path), "baby"), exist_ok=True)
    np.save(os.path.join(str(tmp_path), "baby", "item_graph_dict_2.npy"), item_graph, allow_pickle=True)
    config, _, _, model = G.build(tmp_path, golden, "DAMRS", dict(DAMRS_EXTRA, **extra))
    n = model.n_items
    for name in ("image_adj", "text_adj"):
        graph = hip_ops.CsrGraph.from_coo_host(g[name + "_idx"], g[name + "_val"], n, n, model.device)
        graph.transpose()
        setattr(model, name, graph)
    params = dict(model.named_parameters())
    for key in g:
        if key.startswith("p_"):
            G.load(params[key[2:]], g[key])
    if before_loss is not None:
        before_loss(model)
    loss = model.calculate_loss(torch.as_tensor(g["batch1"]).to(model.device))
    loss.backward()
    return model, loss.detach(), {nm: p.grad.detach().clone() for nm, p in params.items() if p.grad is not None}, g


def meets_the_golden(loss, grads, g):
    """test_damrs_model's own tolerances"""
    G.close(loss, g["loss1"], rtol=2e-5)
    assert set(grads) == {k[2:] for k in g if k.startswith("g_")}
    G.close(grads["user_embedding.weight"], g["g_user_embedding.weight"], rtol=1e-3, atol=2e-7)
    G.close(grads["item_id_embedding.weight"], g["g_item_id_embedding.weight"], rtol=1e-3, atol=2e-7)


def test_damrs_fused_labels_key_on_the_cpu(tmp_path, golden, cpu_ops, monkeypatch):  # noqa: F811
    """absent, False: today's path and none of the new functions; True on CPU tensors: the fallbacks, the key-off loss and both
    embedding gradients at test_damrs_model's tolerances (and the reference's golden)"""
    from mmrec_amd import hip_ops
    monkeypatch.setattr(G, "USE_GPU", False)
    asked = {"pseudo_labels": 0, "tri_softmax_topk": 0, "score_lse": 0, "edge_dot": 0, "list_exclude": 0}
    for name in asked:
        def counted(*a, _real=getattr(hip_ops, name), _name=name, **kw):
            asked[_name] += 1
            return _real(*a, **kw)
        monkeypatch.setattr(hip_ops, name, counted)
    m0, loss0, g0, g = damrs_step(tmp_path / "absent", golden, {})
    m1, loss1, g1, _ = damrs_step(tmp_path / "off", golden, {"fused_labels": False})
    assert m0.fused_labels is False and m1.fused_labels is False
    assert not any(asked.values()), asked                            # absent or False: today's path, untouched
    assert torch.equal(loss0, loss1) or abs(float(loss0) - float(loss1)) <= 1e-6 * abs(float(loss0))
    m2, loss2, g2, _ = damrs_step(tmp_path / "on", golden, {"fused_labels": True})
    assert m2.fused_labels is True
    assert asked == {"pseudo_labels": 1, "tri_softmax_topk": 0, "score_lse": 3, "edge_dot": 3, "list_exclude": 0}, asked
    for loss, grads in ((loss0, g0), (loss2, g2)):
        meets_the_golden(loss, grads, g)
    G.close(loss2, loss0.numpy(), rtol=2e-5)
    for nm in ("user_embedding.weight", "item_id_embedding.weight"):
        G.close(g2[nm], g0[nm].numpy(), rtol=1e-3, atol=2e-7)
    assert set(g2) == set(g0)


def test_the_yaml_names_the_key_in_a_comment_only():
    import yaml
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "mmrec_amd", "configs", "model", "DAMRS.yaml")
    text = open(path).read()
    assert "# fused_labels: True" in text and "fused_labels" not in yaml.safe_load(text)


# ------------------------------------------------------------------------------------------------ the fuzz's checker
CHECKED = (0, 2, 5, 9, 13, 17, 22, 26, 31, 38)         # a spread of the fuzz's cases: every table kind, W kind and ids mode


def test_the_checked_sample_spans_the_kinds():
    cs = [Z.case(k) for k in CHECKED]
    assert {c.tables for c in cs} == set(Z.TABLES) and {c.w_mode for c in cs} == set(Z.WS) and {c.ids_mode for c in cs} == set(Z.IDS)


def test_the_fp32_composition_passes_the_checker_within_the_cap():
    """every case of the fuzz, on the CPU: the fp32 materialised fallback meets the rule, and the pairs that differ from the
    float64 ranking stay within the 5 % cap on these seeds"""
    pairs = lenient = 0
    for k in range(Z.CASES):
        c = Z.case(k)
        idx, val = Z.torch_composition(c)
        n = Z.check(c, idx, val, name=Z.name_of(c))
        pairs, lenient = pairs + 3 * int(c.valid.sum()), lenient + n
    print("fp32 composition: %d of %d pairs differ from the float64 ranking (%.3f %%)" % (lenient, pairs, 100.0 * lenient / pairs))
    assert pairs > 5000 and lenient <= Z.LENIENT_CAP * pairs


def _planted(c, idx, S, plant):
    """one wrong list -> (idx with the error, the message the checker must give)"""
    idx = idx.copy()
    k, N = c.k, c.N
    want = Z.ranking64(S, k)
    rows = [r for r in range(c.B) if c.valid[r]]
    live = [t for t in range(3) if c.W[t].any()]
    r, t = rows[len(rows) // 2], live[0]
    if plant == "far_member":                    # the worst-scoring column instead of the last member
        idx[t, r, k - 1] = int(np.argmin(S[t, r]))
        return idx, "missing|well below"
    if plant == "duplicate":
        idx[t, r, k - 1] = idx[t, r, 0]
        return idx, "duplicate"
    if plant == "id_out_of_range":
        idx[t, r, k // 2] = N
        return idx, "outside"
    if plant == "ties_swapped":                  # two bit-identical columns, both listed, the higher first
        for r in rows:
            for t in live:
                lst = idx[t, r].tolist()
                for i in range(k - 1):
                    if c.dup[lst[i + 1]] == c.dup[lst[i]] and lst[i] < lst[i + 1]:
                        idx[t, r, i], idx[t, r, i + 1] = lst[i + 1], lst[i]
                        return idx, "exact tie"
        raise AssertionError("no listed pair of duplicates in this case")
    if plant == "other_target":                  # list t taken from another target's weights
        for r in rows:
            for t in live:
                for o in live:
                    far = np.setdiff1d(want[o, r], want[t, r])
                    if o != t and far.size and S[t, r, far].min() < S[t, r, want[t, r, k - 1]] * (1 - 1e-3):
                        idx[t, r] = want[o, r]
                        return idx, "missing|well below|descending"
        raise AssertionError("the targets' lists never differ clearly in this case")
    if plant == "ascending":
        idx[t, r] = idx[t, r, ::-1]
        return idx, "descending"
    raise KeyError(plant)


PLANTS = {"far_member": (2, 9, 26), "duplicate": (2, 9, 26), "id_out_of_range": (2, 9, 26), "ties_swapped": None,
          "other_target": (9, 26), "ascending": (2, 9, 26)}


def _dup_cases():
    return tuple(k for k in range(Z.CASES) if Z.case(k).tables == "duplicates" and Z.case(k).k >= 10 and Z.case(k).N >= 64)[:3]


@pytest.mark.parametrize("plant", sorted(PLANTS))
def test_planted_errors_do_not_pass(plant):
    """a far-score member swapped in; a duplicate; an id >= N; two exact ties in the wrong order; a list taken from another
    target's weights; a list in ascending order"""
    ks = PLANTS[plant] or _dup_cases()
    assert ks
    seen = 0
    for k in ks:
        c = Z.case(k)
        if c.k < 2:
            continue
        S, eps = Z.scores64(c), Z.eps_rows(c)
        idx, _ = Z.torch_composition(c)
        Z.check(c, idx, S=S, eps=eps, name="clean")
        try:
            bad, msg = _planted(c, idx, S, plant)
        except AssertionError:
            if plant in ("ties_swapped", "other_target"):
                continue                          # this case offers no such pair; another of the sample must
            raise
        with pytest.raises(AssertionError, match=msg):
            Z.check(c, bad, S=S, eps=eps, name=plant)
        seen += 1
    assert seen >= 1, plant
