"""CPU: host-side logic around the kernels (synthetic shapes, mask CSR, sharding map)."""
import os

import numpy as np
import pytest
import torch

from mmrec_amd import synth
from mmrec_amd.dist import BipartiteSharding
from mmrec_amd.hip_ops import mask_to_csr
from oracle import mmrec_oracle as orc


def test_shaped_edges_unique_and_sized():
    nu, ni, eu, ei = synth.shaped_edges("baby", seed=0)
    assert (nu, ni) == (19445, 7050) and eu.shape[0] == 118706
    key = eu * ni + ei
    assert np.unique(key).shape[0] == key.shape[0]
    assert eu.min() >= 0 and eu.max() < nu and ei.max() < ni


def test_sym_norm_matches_oracle_norm_adj():
    nu, ni, eu, ei = 50, 20, *synth.powerlaw_edges(50, 20, 300, seed=3)
    r, c, v = synth.sym_norm_coo(eu, ei, nu, ni)
    idx, val, n = orc.norm_adj_coo(eu, ei, nu, ni)
    np.testing.assert_array_equal(np.stack([r, c]), idx)   # same (row, col) order, bit-exact values
    np.testing.assert_array_equal(v, val)


def test_mask_to_csr_sorted_rows():
    mask = torch.tensor([[2, 0, 2, 1, 2], [9, 4, 1, 7, 5]])
    rp, col = mask_to_csr(mask, 4, "cpu")
    assert rp.tolist() == [0, 1, 2, 5, 5]
    assert col.tolist() == [4, 7, 1, 5, 9]


def test_bipartite_sharding_map():
    sh = BipartiteSharding(10, 7, 4)
    assert (sh.ub, sh.ib, sh.U_pad, sh.I_pad) == (3, 2, 12, 8)
    rows = np.array([0, 9, 10, 16])
    r, c = sh.padded_coo(rows, rows)
    assert r.tolist() == [0, 9, 12, 18]
    u, i = torch.arange(10.).view(10, 1), torch.arange(7.).view(7, 1) + 100
    x = sh.pad_embeddings(u, i)
    uu, ii = sh.unpad(x)
    assert torch.equal(uu, u) and torch.equal(ii, i)
    covered = sorted(sum([list(range(*sh.user_rows(r))) + list(range(*sh.item_rows(r))) for r in range(4)], []))
    assert covered == list(range(sh.N_pad))


def test_reference_graph_cache_formats(tmp_path):
    """LATTICE's dense [I, I] cache <-> COO round trip, and the loader's None for a missing file."""
    import torch
    from mmrec_amd.graph import coo_to_dense_adj, dense_adj_to_coo, load_cached_adj
    g = torch.Generator().manual_seed(0)
    n, k = 37, 5
    rows = torch.arange(n).repeat_interleave(k)
    cols = torch.stack([torch.randperm(n, generator=g)[:k] for _ in range(n)]).reshape(-1)
    vals = torch.rand(n * k, generator=g) + 0.1
    dense = coo_to_dense_adj(rows, cols, vals, n)
    assert dense.shape == (n, n) and int((dense != 0).sum()) == n * k
    r2, c2, v2 = dense_adj_to_coo(dense)
    o = torch.argsort(rows * n + cols)
    assert torch.equal(r2, rows[o]) and torch.equal(c2, cols[o]) and torch.equal(v2, vals[o])
    path = str(tmp_path / "image_adj_5.pt")
    assert load_cached_adj(path) is None
    torch.save(dense, path)
    assert torch.equal(load_cached_adj(path), dense)


def test_native_random_sample_range_equals_cpython():
    """mmrec_host_random_sample_range == random.sample(range(n), k) of this interpreter: same list, same generator
    state afterwards, in both branches of CPython's algorithm (pool / rejection against the chosen set)."""
    import random
    from mmrec_amd.utils.utils import random_sample_range
    for n, k in ((10, 3), (10, 10), (30, 6), (30, 29), (1000, 5), (1000, 6), (5000, 40), (118706, 106835), (118706, 100),
                 (1, 1), (7, 0)):
        random.seed(n * 31 + k)
        start = random.getstate()
        a = list(random_sample_range(n, k))
        state_a = random.getstate()
        random.setstate(start)
        assert a == random.sample(range(n), k) and random.getstate() == state_a, (n, k)


@pytest.mark.parametrize("kd", [64, 128])
def test_fp16_filter_error_bound_holds(kd):
    """The error bound the fp16 top-K filter (csrc/topk_filter.hip) relies on, restated in numpy: candidates centred by
    their mean row and scaled by ONE power of two, every query row scaled by ITS OWN power of two (thresholds are per
    query), both into fp16's normal range and rounded to fp16:
        |approx - exact| <= eps_q = 1.0e-3 |q| max|c'| + 2^-22 (|q| + max|c'|)
                                    (+ 4e-6 |q| (max|c'| + |mean|) for the fp32 rounding of the exact scores)
    in the scaled / centred units of the approximate score.  Cases: embeddings sharing a large common component (as
    after LightGCN propagation), tiny / huge magnitudes, and -- round-1 review -- HETEROGENEOUS query norms (rows scaled
    by 2^-20 .. 2^-34, an all-zero row, a huge row), which one global query scale pushed into fp16 subnormals
    (err / eps up to 71 there), plus candidates of very different norms and an almost constant candidate set.
    kd = 128 (round 3: VBPR / PGL / SELFCFED_LGN evaluate 128-wide rows): the two kd-dependent terms scale as the kernel
    scales them -- the exact scores' fp32 rounding with kd / 64, the subnormal term with sqrt(kd / 64)."""
    rng = np.random.default_rng(0)
    kb = kd / 64.0

    def scale_of(mx):                       # fp16_scale(): brings |x| <= mx below 2^13
        mx = np.asarray(mx, dtype=np.float32)
        ex = np.frexp(mx)[1]
        return np.where(mx > 0, np.exp2(np.minimum(13.0 - ex, 120.0)), 1.0)     # 2^120: the scale itself stays finite

    cases = []
    for common, mag in ((0.0, 0.2), (5.0, 0.2), (0.0, 1e-4), (50.0, 30.0)):
        Q = (rng.standard_normal((300, kd)) * mag + common).astype(np.float32)
        C = (rng.standard_normal((2000, kd)) * mag + common).astype(np.float32)
        cases.append((Q, C))
    # heterogeneous query norms
    Q = (rng.standard_normal((300, kd)) * 0.2).astype(np.float32)
    for r, e in enumerate((-20, -24, -28, -30, -34, -40, -60, -100, -126)):
        Q[r] *= np.float32(2.0) ** e
    Q[20] = 0.0
    Q[21] *= np.float32(1e30)
    Q[22, 1:] *= np.float32(2.0) ** -30                      # one dominant element, the rest far below it
    C = (rng.standard_normal((2000, kd)) * 0.2).astype(np.float32)
    cases.append((Q, C))
    # heterogeneous candidate norms (rows far below the largest one) under the same queries
    C2 = C.copy()
    C2[:500] *= np.float32(2.0) ** -20
    C2[500:600] *= np.float32(2.0) ** -40
    cases.append((Q, C2))
    # an almost constant candidate set: the centred rows are ~1e-6 of the uncentred ones
    C3 = (5.0 + rng.standard_normal((2000, kd)) * 1e-6).astype(np.float32)
    cases.append(((rng.standard_normal((300, kd)) * 0.2).astype(np.float32), C3))
    worst = 0.0
    for ci, (Q, C) in enumerate(cases):
        mean = C.sum(0, dtype=np.float32) / np.float32(C.shape[0])
        sq = scale_of(np.abs(Q).max(axis=1)).astype(np.float32)[:, None]          # per query row
        sc = np.float32(scale_of(2.0 * np.abs(C).max()))
        with np.errstate(over="ignore"):
            Qh = (Q * sq).astype(np.float16)
            Ch = ((C - mean) * sc).astype(np.float16)
        assert np.isfinite(Qh).all() and np.isfinite(Ch).all()
        approx = Qh.astype(np.float64) @ Ch.astype(np.float64).T
        exact = ((Q.astype(np.float64) * sq.astype(np.float64)) @ (C.astype(np.float64) - mean.astype(np.float64)).T) * float(sc)
        qn = np.linalg.norm(Qh.astype(np.float64), axis=1) * 1.0005
        cmax = np.linalg.norm(Ch.astype(np.float64), axis=1).max() * 1.0005
        eps = qn * (1.0e-3 * cmax + 4.0e-6 * kb * (cmax + float(sc) * np.linalg.norm(mean.astype(np.float64)))) + \
            2.4e-7 * np.sqrt(kb) * (qn + cmax)
        err = np.abs(approx - exact).max(axis=1)
        assert np.all(err <= eps), (ci, float((err / np.maximum(eps, 1e-300)).max()))
        worst = max(worst, float((err[eps > 0] / eps[eps > 0]).max()))
    assert worst > 1e-3      # the bound is a bound, not a vacuous one


def test_fp16_filter_clipped_rows_stay_lower_bounds():
    """Round 3: candidate sets of >= 131,072 rows CLIP their few rows of outlying norm (filter_clip_kernel): eps is
    proportional to the largest stored row norm, and one row of 20 x the median norm doubled every query's survivors at
    config 5.  Restated: norm histogram over float bits >> 20, tau = lower edge of the lowest bin with <= 32 rows in the bins
    from it upwards, rows of norm >= tau stored as fp16(f c'), f = tau (1 - 2^-9) / norm.  What the kernels' argument needs:
    (a) <= 32 rows are clipped and every stored row norm is <= tau;  (b) a clipped row's approximate score is within eps(tau)
    of f x its exact score, so wherever the approximate score is >= eps (the bound kernel checks T >= eps) the exact score
    is >= approx - eps: the group maxima of pass 1 stay lower bounds of real scores;  (c) unclipped rows keep the plain bound
    with tau in place of the largest norm."""
    rng = np.random.default_rng(3)
    kd, nc = 64, 140_000
    C = (rng.standard_normal((nc, kd)) * 0.1 + 0.05).astype(np.float32)
    big = rng.choice(nc, 20, replace=False)
    C[big] *= rng.uniform(3.0, 25.0, (20, 1)).astype(np.float32)
    Q = (rng.standard_normal((200, kd)) * 0.3).astype(np.float32)
    mean = C.sum(0, dtype=np.float32) / np.float32(nc)
    sc = np.float32(2.0 ** (13 - np.frexp(np.float32(2.0 * np.abs(C).max()))[1]))
    sq = (2.0 ** (13 - np.frexp(np.abs(Q).max(axis=1))[1])).astype(np.float32)[:, None]
    Ch = ((C - mean) * sc).astype(np.float16)
    norms = (np.linalg.norm(Ch.astype(np.float32), axis=1) * np.float32(1.0005)).astype(np.float32)
    bins = norms.view(np.uint32) >> 20
    hist = np.bincount(bins, minlength=2048)
    cum, b = 0, 2048
    for j in range(2047, -1, -1):
        if cum + hist[j] > 32:
            break
        cum, b = cum + hist[j], j
    assert 0 < cum <= 32
    tau = np.array([b << 20], dtype=np.uint32).view(np.float32)[0]
    out = norms >= tau
    assert out.sum() == cum
    f = (sc * (tau * np.float32(1.0 - 1.0 / 512.0) / norms[out])).astype(np.float32)[:, None]
    Ch[out] = ((C[out] - mean) * f).astype(np.float16)
    stored = np.linalg.norm(Ch.astype(np.float64), axis=1) * 1.0005
    assert stored.max() <= tau                                                            # (a)
    Qh = (Q * sq).astype(np.float16)
    qn = np.linalg.norm(Qh.astype(np.float64), axis=1) * 1.0005
    eps = qn * (1.0e-3 * tau + 4.0e-6 * (float(norms.max()) + float(sc) * np.linalg.norm(mean.astype(np.float64)))) + 2.4e-7 * (qn + tau)
    approx = Qh.astype(np.float64) @ Ch.astype(np.float64).T
    exact = ((Q.astype(np.float64) * sq.astype(np.float64)) @ (C.astype(np.float64) - mean.astype(np.float64)).T) * float(sc)
    ratio = (f[:, 0].astype(np.float64) / float(sc))                                      # f / scale < 1
    assert np.all(ratio < 1.0)
    assert np.all(np.abs(approx[:, out] - exact[:, out] * ratio[None, :]) <= eps[:, None])          # (b)
    pos = approx[:, out] >= eps[:, None]
    assert np.all((exact[:, out] >= approx[:, out] - eps[:, None])[pos])
    assert np.all(np.abs(approx[:, ~out] - exact[:, ~out]) <= eps[:, None])               # (c)
    assert tau < 0.5 * norms.max()                                                        # the clipping bought something


def test_config_helpers_for_added_keys():
    """eval_batch_size(): the reference's 4096 unless the fused evaluation runs on the GPU; lazy_adam_enabled(): off on
    the CPU / without the fused Adam / with gradient clipping, automatic only for large tables, forced by True / False;
    hipGraph replay of the step is no obstacle any more (the tables read the optimizer's device counters)."""
    from mmrec_amd.common.lazy_rows import AUTO_MIN_ELEMENTS, lazy_adam_enabled
    from mmrec_amd.utils.utils import eval_batch_size

    class Cfg(dict):
        def __getitem__(self, k):
            return self.get(k)
    gpu, cpu = torch.device("cuda", 0), torch.device("cpu")
    base = {"eval_batch_size": 4096, "learner": "adam", "hip_fused_adam": True}
    assert eval_batch_size(Cfg(base, device=cpu)) == 4096
    assert eval_batch_size(Cfg(base, device=gpu)) == 65536
    assert eval_batch_size(Cfg(base, device=gpu, hip_eval_batch_size=10000)) == 10000
    assert eval_batch_size(Cfg(base, device=gpu, hip_fused_eval=False)) == 4096
    from mmrec_amd.common.lazy_rows import AUTO_MIN_ELEMENTS_REPLAYED
    big, small = AUTO_MIN_ELEMENTS, AUTO_MIN_ELEMENTS_REPLAYED - 1
    assert lazy_adam_enabled(Cfg(base, device=gpu, hip_graph_step=False), big)
    assert not lazy_adam_enabled(Cfg(base, device=gpu, hip_graph_step=False), big - 1)       # eager steps: from 64 Mi elements
    for replayed in ("auto", True):                                                           # replayed steps (the default): from 16 Mi
        assert lazy_adam_enabled(Cfg(base, device=gpu, hip_graph_step=replayed), AUTO_MIN_ELEMENTS_REPLAYED)
    assert lazy_adam_enabled(Cfg(base, device=gpu), big) and not lazy_adam_enabled(Cfg(base, device=gpu), small)
    assert lazy_adam_enabled(Cfg(base, device=gpu, lazy_feature_adam=True), small)
    assert not lazy_adam_enabled(Cfg(base, device=gpu, lazy_feature_adam=False), big)
    assert not lazy_adam_enabled(Cfg(base, device=cpu, lazy_feature_adam=True), big)
    assert lazy_adam_enabled(Cfg(base, device=gpu, hip_graph_step=True), big)
    assert not lazy_adam_enabled(Cfg(base, device=gpu, learner="sgd"), big)
    assert not lazy_adam_enabled(Cfg(base, device=gpu, clip_grad_norm={"max_norm": 1.0}), big)
    assert not lazy_adam_enabled(Cfg(base, device=gpu, hip_fused_adam=False, lazy_feature_adam=True), big)


ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


def _reference_api():
    """what tests/golden/make_golden_reference_api.py recorded from the unmodified reference (values as digests)"""
    import json
    with open(os.path.join(GOLDEN, "reference_api.json")) as f:
        return json.load(f)


def _digest_diff(ref, mine):
    """keys of `ref` (key -> digest) that `mine` (key -> value) lacks or holds with another value"""
    from tests._env import config_digest
    return sorted(k for k, d in ref.items() if k not in mine or config_digest(mine[k]) != d)


def test_every_reference_model_has_a_plugin_and_an_equal_config():
    """Drop-in surface: each `src/models/<name>.py` of the reference has a same-named plugin exposing the same class,
    and each `configs/model/<Name>.yaml`, `configs/dataset/*.yaml` parses to the reference's values (ours may add keys
    to overall.yaml, never change one)."""
    import importlib
    import yaml
    api = _reference_api()
    ref_models = api["models"]
    assert len(ref_models) == 21
    ours = sorted(f[:-3] for f in os.listdir(os.path.join(ROOT, "mmrec_amd", "models")) if f.endswith(".py") and f[0] != "_")
    assert set(ref_models) <= set(ours), sorted(set(ref_models) - set(ours))
    files = [f for f in api["config_files"] if f != "overall.yaml"]
    assert sum(f.startswith("model/") for f in files) == 21 and any(f.startswith("dataset/") for f in files)
    for f in files:
        mine = os.path.join(ROOT, "mmrec_amd", "configs", f)
        assert os.path.exists(mine), mine
        with open(mine) as b:
            parsed = yaml.safe_load(b)
        ref = api["config_files"][f]
        assert sorted(parsed) == sorted(ref) and not _digest_diff(ref, parsed), (f, _digest_diff(ref, parsed))
        if f.startswith("model/"):
            name = f[len("model/"):-5]
            mod = importlib.import_module("mmrec_amd.models." + name.lower())
            assert hasattr(mod, name), name
    with open(os.path.join(ROOT, "mmrec_amd", "configs", "overall.yaml")) as b:
        mine = yaml.safe_load(b)
    assert not _digest_diff(api["config_files"]["overall.yaml"], mine), _digest_diff(api["config_files"]["overall.yaml"], mine)


def test_knn_graph_helpers_equal_the_reference_functions():
    """utils.utils kNN-graph helpers (kept for model code written against the reference's API): same values as the
    reference's functions (tests/golden/reference_knn_helpers.npz: their seeded inputs and outputs) incl. rows that sum
    to 0, dense and sparse, every normalisation.  The fixture equals ours bit for bit where it was written; on another
    CPU a BLAS product or a row sum may round in another order, hence 1e-6 relative on computed values (selections and
    indices stay exact)."""
    from mmrec_amd.utils import utils as ours
    g = {k: torch.from_numpy(v) for k, v in np.load(os.path.join(GOLDEN, "reference_knn_helpers.npz")).items()}

    def same(a, b):
        torch.testing.assert_close(a, b, rtol=1e-6, atol=0)
    same(ours.build_sim(g["feats"]), g["sim"])
    assert torch.equal(ours.build_knn_neighbourhood(g["sim"], 5), g["neighbourhood_5"])
    adj = g["adj"]
    assert float(adj[4].abs().sum()) == 0.0                                       # an empty row: 0, not inf / nan
    same(ours.compute_normalized_laplacian(adj), g["normalized_laplacian"])
    for norm in ("sym", "rw", "none"):
        same(ours.get_dense_laplacian(adj, norm), g["dense_laplacian_" + norm])
        same(ours.build_knn_normalized_graph(adj, 4, False, norm), g["knn_dense_" + norm])
        a = ours.build_knn_normalized_graph(adj, 4, True, norm)
        assert torch.equal(a._indices(), g["knn_sparse_indices_" + norm])
        same(a._values(), g["knn_sparse_values_" + norm])
        i1, w1 = ours.get_sparse_laplacian(g["edge_index_" + norm], g["edge_weight_" + norm], 30, norm)
        assert torch.equal(i1, g["sparse_laplacian_indices_" + norm])
        same(w1, g["sparse_laplacian_weights_" + norm])


def test_config_objects_equal_the_reference_configs():
    """`Config(model, dataset, overrides, mg)`: for every model, with and without the Mirror-Gradient file, every key
    the reference's merged configuration holds has the same value here (hyper-parameter list order included); ours only
    adds keys.  The reference's side: tests/golden/reference_api.json (make_golden_reference_api.py)."""
    from mmrec_amd.utils.configurator import Config
    from tests._env import config_digest
    api = _reference_api()
    models = sorted({k.split("/")[0] for k in api["final_configs"]})
    assert len(models) == 21
    for name in models:
        for mg in (False, True):
            ref = api["final_configs"]["%s/mg=%d" % (name, mg)]
            over = {"gpu_id": 0, "use_gpu": False, "learning_rate": 0.123, "brand_new_key": [1, 2]}
            b = Config(name, "sports", dict(over), mg)
            rb = dict(b.final_config_dict)
            missing = [k for k in ref["values"] if k not in rb]
            assert not missing, (name, mg, missing)
            device = rb.pop("device")
            diff = [k for k in _digest_diff(ref["values"], rb) if k != "device"]
            assert not diff, (name, mg, {k: rb[k] for k in diff})
            assert config_digest(str(device)) == ref["values"]["device"]
            assert ref["missing_key_is_none"] and b["no_such_key"] is None


def test_ground_truth_csr_from_flat_lists_equals_per_list_sort():
    """hip_ops.flat_to_csr (one global sort of (row, id) keys; what the device metrics use for 1M evaluation users) ==
    the per-list construction: row pointers, ids ascending inside every row, empty rows, an empty input."""
    from mmrec_amd import hip_ops
    rng = np.random.default_rng(2)
    lens = rng.integers(0, 7, 5000)
    lens[[0, 17, 4999]] = 0
    flat = rng.integers(0, 30000, int(lens.sum()))
    lists = np.split(flat, np.cumsum(lens)[:-1])
    rp, ids = hip_ops.flat_to_csr(flat, lens, "cpu")
    rp2, ids2 = hip_ops.lists_to_csr(lists, "cpu")
    assert torch.equal(rp, rp2) and torch.equal(ids, ids2) and rp.dtype == torch.int32 and ids.dtype == torch.int32
    ref = np.concatenate([np.sort(x) for x in lists])
    assert np.array_equal(ids.numpy(), ref) and np.array_equal(rp.numpy(), np.concatenate([[0], np.cumsum(lens)]))
    rp, ids = hip_ops.flat_to_csr(np.zeros(0, np.int64), np.zeros(3, np.int64), "cpu")
    assert rp.tolist() == [0, 0, 0, 0] and ids.numel() == 1


def test_locality_order_is_a_permutation_and_groups_neighbours():
    """hip_ops.locality_order (the relabelling behind hip_ops.PermutedGraph): 'degree' puts the highest-degree nodes first;
    'rcm' shrinks the bandwidth of a graph whose communities were hidden by a random id permutation (neighbours get nearby
    ids).  Host side, integer, deterministic."""
    import scipy.sparse as sp
    from mmrec_amd import hip_ops
    rng = np.random.default_rng(0)
    n, comm = 3000, 100                                            # 30 communities of 100 nodes, ids scrambled
    a = rng.integers(0, n, 30000)
    b = (a // comm) * comm + rng.integers(0, comm, 30000)          # edges inside a community
    scramble = rng.permutation(n)
    rows, cols = np.concatenate([scramble[a], scramble[b]]), np.concatenate([scramble[b], scramble[a]])
    m = sp.csr_matrix((np.ones(rows.shape[0]), (rows, cols)), shape=(n, n))
    m.sum_duplicates()
    rp, ci = m.indptr.astype(np.int64), m.indices
    for how in ("degree", "rcm", "community"):
        perm = hip_ops.locality_order(rp, ci, n, how)
        assert sorted(perm.tolist()) == list(range(n))
        assert np.array_equal(perm, hip_ops.locality_order(rp, ci, n, how))
    deg = np.diff(rp)
    pd = hip_ops.locality_order(rp, ci, n, "degree")
    assert deg[np.argsort(pd)][0] == deg.max() and np.all(np.diff(deg[np.argsort(pd)]) <= 0)
    pr = hip_ops.locality_order(rp, ci, n, "rcm")
    r_of = np.repeat(np.arange(n), deg)
    spread_before = np.abs(r_of - ci).mean()
    spread_after = np.abs(pr[r_of] - pr[ci]).mean()
    assert spread_after < 0.2 * spread_before, (spread_before, spread_after)
    # label propagation finds the hidden communities, also with 10 % of the edges going anywhere (where RCM's BFS levels blow up)
    far = rng.integers(0, n, 3000), rng.integers(0, n, 3000)
    m2 = sp.csr_matrix((np.ones(rows.shape[0] + 6000), (np.concatenate([rows, far[0], far[1]]), np.concatenate([cols, far[1], far[0]]))),
                       shape=(n, n))
    m2.sum_duplicates()
    rp2, ci2 = m2.indptr.astype(np.int64), m2.indices
    pc = hip_ops.locality_order(rp2, ci2, n, "community")
    r2 = np.repeat(np.arange(n), np.diff(rp2))
    assert np.abs(pc[r2] - pc[ci2]).mean() < 0.25 * np.abs(r2 - ci2).mean()
    with pytest.raises(ValueError):
        hip_ops.locality_order(rp, ci, n, "nope")


def test_lazy_adam_settled_parameter_bound_holds():
    """adam.hip adam_param_settled (the row-lazy catch-up replays only the moment decays once it holds): whenever
    1.01 * max_j L_j * |m| / (sqrt(v) * 0.99 * beta2^128 + eps) < 2^(exponent(p) - 25)  (a quarter ulp of p), NO decay-only Adam
    step of the next 256 can change p's bits.  Restated in numpy float32 over 200,000 elements of very different magnitudes
    (incl. exact zeros, powers of two, 1e-7-sized parameters, tiny second moments) and a decreasing step-size sequence: every
    element that tests 'settled' at a 32-step boundary keeps its parameter bits for the following 256 steps -- and the test
    does settle for most elements within 300 steps (it is not vacuous)."""
    rng = np.random.default_rng(0)
    n, T = 200_000, 640
    f32 = np.float32
    p = (rng.standard_normal(n) * 10.0 ** rng.uniform(-7, 1, n)).astype(f32)
    p[::11] = 0.0
    p[1::11] = f32(0.5)
    p[2::11] = f32(-4.0)
    g = (rng.standard_normal(n) * 10.0 ** rng.uniform(-6, 0, n)).astype(f32)
    b1, b2, eps = f32(0.9), f32(0.999), f32(1e-8)
    t0 = 40                                                   # optimizer steps taken before the row starts to sit out
    m = ((1 - b1) * g).astype(f32) * f32(rng.uniform(0.2, 3.0))     # some first / second moment left by earlier gradients
    v = ((1 - b2) * g * g).astype(f32) * f32(rng.uniform(0.2, 3.0))
    steps = np.arange(t0 + 1, t0 + T + 1)
    lr = f32(1e-3) * f32(0.96) ** (steps // 200)
    L = (lr / (1 - np.float64(b1) ** steps)).astype(f32)             # lr_j / (1 - b1^j)
    c = (1.0 / np.sqrt(1 - np.float64(b2) ** steps)).astype(f32)     # 1 / sqrt(1 - b2^j) >= 1
    v_fac = f32(0.99) * f32(np.float64(b2) ** 128)
    settled_at = np.full(n, -1)
    p_at = np.zeros(n, f32)
    first = np.full(n, -1)
    for j in range(T):
        if j % 32 == 0:
            tile_end = min((j // 256 + 1) * 256, T)
            l_max = L[j // 256 * 256:tile_end].max()
            bound = f32(1.01) * l_max * np.abs(m) / (np.sqrt(v) * v_fac + eps)
            quarter_ulp = (np.abs(p).view(np.uint32) & np.uint32(0x7f800000)).view(f32) * f32(2.0 ** -25)
            ok = (m == 0) | (bound < quarter_ulp)
            fresh = ok & (settled_at < 0)
            settled_at[fresh], p_at[fresh] = j, p[fresh]
            first[ok & (first < 0)] = j
        # one decay-only step (adam_decay_one), float32
        m = (m + (-(1 - b1)) * m).astype(f32)
        v = (v * b2).astype(f32)
        denom = (np.sqrt(v) * c[j] + eps).astype(f32)
        p_new = (p - L[j] * (m / denom).astype(f32)).astype(f32)
        watched = (settled_at >= 0) & (j < (settled_at // 256 + 1) * 256)        # the kernel re-tests at the next 256-step tile
        changed = watched & (p_new.view(np.uint32) != p.view(np.uint32))
        assert not changed.any(), (j, int(changed.sum()))
        p = p_new
        expired = (settled_at >= 0) & (j + 1 >= (settled_at // 256 + 1) * 256)
        settled_at[expired] = -1
    assert (first >= 0).mean() > 0.85 and np.median(first[first >= 0]) <= 320


def _adam_skipped_updates_direct(s0, n, lr, b1, b2, eps, m0, v0):
    """sum of the n updates dense Adam applies to a parameter whose gradient is zero from step s0 + 1 on (float64)"""
    jp = np.arange(1, n + 1, dtype=np.float64)[:, None]
    t = s0 + jp
    return ((lr / (1 - b1 ** t)) * b1 ** jp * m0[None] / (np.sqrt(v0[None] * b2 ** jp) / np.sqrt(1 - b2 ** t) + eps)).sum(0)


def _adam_skipped_updates_series(s0, n, lr, b1, b2, eps, m0, v0, K=6, J=256):
    """csrc/adam.hip: adam_fast_row_scalars + adam_fast_one in float64 (the opt-in fast-forward of a skipped row)"""
    jp = np.arange(1, min(n, J) + 1, dtype=np.float64)
    t = s0 + jp
    w = (lr / (1 - b1 ** t)) * b1 ** jp
    d = b2 ** (jp / 2) / np.sqrt(1 - b2 ** t)
    W = w.sum()
    dbar = (w * d).sum() / W
    de = d / dbar - 1
    M = [(w * de ** k).sum() for k in range(K + 1)]
    R = (np.abs(w) * np.abs(de) ** (K + 1)).sum() / abs(W)
    y = np.sqrt(v0) * dbar
    r = 1 / (y + eps)
    u = y * r
    s = M[K]
    for k in range(K - 1, 1, -1):
        s = M[k] - u * s
    return m0 * r * (W + u * u * s), R


def test_lazy_adam_fast_forward_series_equals_the_direct_sum():
    """The opt-in closed form of the row-lazy catch-up (include/mmrec_hip.h: mmrec_adam_rows_fastforward_f32): the sum of a
    skipped row's updates as a six-term series around the row's weighted-mean d.  For second moments over 22 decades (eps
    far above, near and far below sqrt(v)) the series is within 2 R of the direct sum, R being the remainder estimate the
    kernel forms; R <= 1e-7 -- the kernel's condition for using it -- holds from ~100 optimizer steps on for ANY gap, and is
    refused (exact replay) in the first steps, where the bias correction of v moves by per cents per step."""
    rng = np.random.default_rng(0)
    for s0 in (0, 3, 10, 30, 50, 100, 300, 683, 5000):
        for n in (13, 17, 122, 500, 3000):
            v0 = 10.0 ** rng.uniform(-22, 0, 1000)
            m0 = np.sqrt(v0) * rng.normal(size=1000) * 3
            direct = _adam_skipped_updates_direct(s0, n, 1e-3, 0.9, 0.999, 1e-8, m0, v0)
            series, R = _adam_skipped_updates_series(s0, n, 1e-3, 0.9, 0.999, 1e-8, m0, v0)
            err = np.max(np.abs(series - direct) / np.abs(direct))
            assert err <= 2 * R + 1e-11, (s0, n, R, err)
            if s0 >= 100:
                assert R <= 1e-7 and err <= 2e-7, (s0, n, R)
            if s0 <= 10 and n >= 100:
                assert R > 1e-7, (s0, n, R)            # refused: the kernel replays these rows exactly


@pytest.mark.parametrize("kd", [192, 384, 4096])
def test_wide_rows_error_bound_holds(kd):
    """The margin the wide-row path (csrc/topk_wide.h: kd = 192 ... 4096) tests its 64 approximate candidates with, restated in
    numpy: every query row scaled by its own power of two and the candidates by one, both below 2^8, rounded to fp16, products
    accumulated in fp32 (emulated: float32 partial sums over 16-wide k slices, as an MFMA chain accumulates):
        |approx - exact| <= eps_q = (1.0e-3 + kd 6e-8 + 4e-6 kd / 64) |q| max|c| + 2.4e-7 sqrt(kd / 64) (|q| + max|c|)
    in the scaled units of the approximate score (norms of the ROUNDED rows, inflated by 1.0005 as the kernel does).  Raw-
    feature-like inputs (non-negative with a large common component), rows of very different scales, tiny elements next to a
    dominant one."""
    rng = np.random.default_rng(kd)

    def scale_of(mx):                       # w_scale_for(): brings |x| <= mx below 2^8
        mx = np.asarray(mx, dtype=np.float32)
        ex = np.frexp(mx)[1]
        return np.where(mx > 0, np.exp2(np.minimum(8.0 - ex, 120.0)), 1.0)

    nq, nc = 40, 300
    cases = []
    base = np.maximum(rng.standard_normal((nc, kd)), 0).astype(np.float32) + 0.3
    cases.append((base[:nq] / np.linalg.norm(base[:nq], axis=1, keepdims=True), base / np.linalg.norm(base, axis=1, keepdims=True)))
    Q = (rng.standard_normal((nq, kd)) * 0.2).astype(np.float32)
    for r, e in enumerate((-20, -30, -60, -100, 20)):
        Q[r] *= np.float32(2.0) ** e
    Q[7, 1:] *= np.float32(2.0) ** -22                       # one dominant element
    C = (rng.standard_normal((nc, kd)) * 0.2).astype(np.float32)
    C[:50] *= np.float32(2.0) ** -18
    cases.append((Q, C))
    cases.append(((rng.standard_normal((nq, kd)) * 30 + 50).astype(np.float32), (rng.standard_normal((nc, kd)) * 30 + 50).astype(np.float32)))
    kb = kd / 64.0
    worst = 0.0
    for ci, (Q, C) in enumerate(cases):
        sq = scale_of(np.abs(Q).max(axis=1)).astype(np.float32)[:, None]
        sc = np.float32(scale_of(np.abs(C).max()))
        Qh, Ch = (Q * sq).astype(np.float16), (C * sc).astype(np.float16)
        assert np.isfinite(Qh).all() and np.isfinite(Ch).all()
        acc = np.zeros((nq, nc), dtype=np.float32)
        for k0 in range(0, kd, 16):                          # fp32 accumulation, 16 products per step
            acc = (acc + (Qh[:, k0:k0 + 16].astype(np.float32) @ Ch[:, k0:k0 + 16].astype(np.float32).T)).astype(np.float32)
        exact = (Q.astype(np.float64) * sq.astype(np.float64)) @ C.astype(np.float64).T * float(sc)
        qn = np.linalg.norm(Qh.astype(np.float64), axis=1) * 1.0005
        cmax = np.linalg.norm(Ch.astype(np.float64), axis=1).max() * 1.0005
        eps = qn * cmax * (1.0e-3 + kd * 6.0e-8 + 4.0e-6 * kb) + 2.4e-7 * np.sqrt(kb) * (qn + cmax)
        err = np.abs(acc.astype(np.float64) - exact).max(axis=1)
        assert np.all(err <= eps), (ci, float((err / np.maximum(eps, 1e-300)).max()))
        assert np.abs(acc).max() < 1e9                       # far from the -1e10 mask sentinel ("<= -1e9" reads as masked)
        worst = max(worst, float((err[eps > 0] / eps[eps > 0]).max()))
    assert worst > 1e-3


def test_split_operand_projection_error_bound_holds():
    """gemm.hip linear_fwd_dma_f16x3_kernel, restated in numpy: x = hi + lo, hi = fp16(x), lo' = fp16(2^11 (x - hi));
    x w ~ hi_x hi_w + 2^-11 (hi_x lo'_w + lo'_x hi_w) with two fp32 accumulator sets (hi hi / cross terms) combined once.
    Claim: error per product <= 2^-21 |x w|, i.e. the result is within 2^-21 sum|x w| + the fp32 accumulation
    rounding of the exact value -- as accurate as an fp32 GEMM.  K = 4096 like the image features; relu-like non-negative
    rows, signed rows, elements spanning 2^-20 ... 2^10 of magnitude (below fp16's normal range the lo' term is what keeps
    the precision)."""
    rng = np.random.default_rng(0)
    K, n = 4096, 64
    f16, f32, f64 = np.float16, np.float32, np.float64

    def split(a):
        hi = a.astype(f16)
        lo = ((a - hi.astype(f32)) * f32(2048.0)).astype(f16)
        return hi, lo

    cases = [(np.maximum(rng.standard_normal((n, K)), 0).astype(f32), (rng.random((64, K)) - 0.5).astype(f32)),
             ((rng.standard_normal((n, K)) * 10.0 ** rng.uniform(-6, 3, (n, K))).astype(f32), (rng.standard_normal((64, K)) * 0.05).astype(f32)),
             ((rng.standard_normal((n, K)) * 300).astype(f32), (rng.standard_normal((64, K)) * 2.0 ** rng.integers(-20, 3, (64, K))).astype(f32))]
    worst = 0.0
    for X, W in cases:
        xh, xl = split(X)
        wh, wl = split(W)
        hh = np.zeros((n, 64), f32)
        cx = np.zeros((n, 64), f32)
        for k0 in range(0, K, 16):                           # fp32 accumulators, 16 exact fp16 x fp16 products per MFMA step
            s = slice(k0, k0 + 16)
            hh = (hh + xh[:, s].astype(f32) @ wh[:, s].astype(f32).T).astype(f32)
            cx = (cx + xh[:, s].astype(f32) @ wl[:, s].astype(f32).T + xl[:, s].astype(f32) @ wh[:, s].astype(f32).T).astype(f32)
        got = (cx * f32(1.0 / 2048.0) + hh).astype(f32)
        exact = X.astype(f64) @ W.astype(f64).T
        mag = np.abs(X).astype(f64) @ np.abs(W).astype(f64).T
        # 2^-21 per product + fp32 accumulation over K / 16 steps of two accumulators (each step rounds once: 2^-24 of the
        # running magnitude) + the final combine
        bound = mag * (2.0 ** -21 + (K / 16 + 2) * 2.0 ** -24)
        err = np.abs(got.astype(f64) - exact)
        assert np.all(err <= bound), float((err / np.maximum(bound, 1e-300)).max())
        worst = max(worst, float((err / np.maximum(bound, 1e-300)).max()))
        # and it is as good as a plain fp32 GEMM with the same accumulation granularity
        ref = np.zeros((n, 64), f32)
        for k0 in range(0, K, 16):
            ref = (ref + X[:, k0:k0 + 16] @ W[:, k0:k0 + 16].T).astype(f32)
        assert err.max() <= 4 * max(np.abs(ref.astype(f64) - exact).max(), 1e-30) + 1e-30 or np.all(err <= mag * 2.0 ** -20)
    assert worst > 1e-4


def test_split_operand_projection_domain_rule():
    """The device-side guard of mmrec_linear_fwd_split_f32 (gemm.hip: SPLIT_ROW_MIN, redo flags), restated in numpy.  Rule: a row
    whose largest |x| is below 2^-10 (and not 0), or whose split result is non-finite, is recomputed by the fp32 kernel.  Shown
    here: (i) the rule is NEEDED -- rows scaled by 1e-7 / 1e-8 are wrong by > 1e-5 of sum |x w| in the raw split, and |x| >= 65520
    turns into inf / NaN although the fp32 product is finite; (ii) the rule is SUFFICIENT -- every row it does not flag meets
    |err| <= 2^-21 sum |x w| + 2^-25 max|x_row| sum |w_row| + fp32 accumulation, tiny elements inside ordinary rows included."""
    rng = np.random.default_rng(1)
    K, n = 4096, 48
    f16, f32, f64 = np.float16, np.float32, np.float64
    ROW_MIN = f32(2.0 ** -10)

    def split(a):
        with np.errstate(over="ignore", invalid="ignore"):
            hi = a.astype(f16)
            lo = ((a - hi.astype(f32)) * f32(2048.0)).astype(f16)
        return hi, lo

    X = np.maximum(rng.standard_normal((n, K)), 0).astype(f32)
    scale = np.ones(n)
    scale[:12] = [1e-7, 1e-8, 1e-5, 3e-4, 2e-3, 1e-2, 1e2, 1e4, 1.5e4, 1e5, 1e-12, 1e-30]
    X = (X * scale[:, None]).astype(f32)
    X[12, ::2] *= f32(1e-9)                       # an ordinary row, half of whose elements are tiny
    X[13, 1:] *= f32(1e-9)                        # one ordinary element, the rest tiny
    X[13, 0] = 1.0
    X[14] = 0
    W = (rng.standard_normal((64, K)) / 64).astype(f32)
    xh, xl = split(X)
    wh, wl = split(W)
    with np.errstate(over="ignore", invalid="ignore"):
        hh = np.zeros((n, 64), f32)
        cx = np.zeros((n, 64), f32)
        for k0 in range(0, K, 16):
            s = slice(k0, k0 + 16)
            hh = (hh + xh[:, s].astype(f32) @ wh[:, s].astype(f32).T).astype(f32)
            cx = (cx + xh[:, s].astype(f32) @ wl[:, s].astype(f32).T + xl[:, s].astype(f32) @ wh[:, s].astype(f32).T).astype(f32)
        got = (cx * f32(1.0 / 2048.0) + hh).astype(f32)
    exact = X.astype(f64) @ W.astype(f64).T
    mag = np.abs(X).astype(f64) @ np.abs(W).astype(f64).T
    rowmax = np.abs(X).max(1)
    flagged = ((rowmax > 0) & (rowmax < ROW_MIN)) | ~np.isfinite(got).all(1)
    with np.errstate(invalid="ignore", divide="ignore"):
        rel = np.abs(got.astype(f64) - exact) / mag
    # (i) needed
    print("raw split error / sum|xw| by row:", rel.max(1)[:15])
    assert flagged[0] and flagged[1] and rel[0].max() > 2e-6 and rel[1].max() > 2e-5
    assert flagged[9] and not np.isfinite(got[9]).all() and np.isfinite(exact[9]).all()      # 1e5 * relu-normal: some |x| > 65504
    assert flagged[10] and flagged[11] and flagged[2]
    assert not flagged[3:9].any() and not flagged[12:].any()      # 3e-4 x relu-normal: row max 1.2e-3, just inside
    # (ii) sufficient
    ok = ~flagged
    bound = mag * (2.0 ** -21 + (K / 16 + 2) * 2.0 ** -24) + 2.0 ** -25 * rowmax[:, None] * np.abs(W).astype(f64).sum(1)[None, :]
    err = np.abs(got.astype(f64) - exact)
    assert np.all(err[ok] <= bound[ok])
    assert np.nanmax(rel[ok & (rowmax > 0)]) <= 1e-6                         # the test the device suite applies
    assert np.array_equal(got[14], np.zeros(64, f32))



def _bf16_round(a):
    """fp32 -> bf16 -> fp32, round to nearest even (what v_cvt_pk_bf16_f32 does), on a float32 array"""
    u = np.ascontiguousarray(a, dtype=np.float32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return u.astype(np.uint32).view(np.float32)


def test_bf16_three_way_split_projection_gradient_claim():
    """gemm.hip linear_bwd_w_v2_kernel (fed by bwd_dy_split_kernel), restated in numpy: x = b1 + b2 + b3 with b1 = bf16(x), b2 = bf16(x - b1),
    b3 = bf16(x - b1 - b2); dW = sum over items of the six products b_i c_j with i + j <= 4 (the three dropped ones are
    <= 2^-23 |x y|).  Claims checked: (1) the three parts restore x to 2^-24 relative -- for magnitudes 1e-30 ... 1e30 alike,
    no scale involved; (2) dW's error against float64 is <= 2^-22 sum |dy x| per output on a gradient column that spans 2^44
    (the case one power-of-two scale per column cannot hold: the guarded fp16 form's fix-up) with X zero where the large
    gradients sit; (3) entries below 2^-110 degrade to an absolute 2^-133, not to garbage."""
    rng = np.random.default_rng(5)
    x = (rng.standard_normal(4096) * 10.0 ** rng.uniform(-30, 30, 4096)).astype(np.float32)
    b1 = _bf16_round(x)
    r1 = x - b1
    b2 = _bf16_round(r1)
    b3 = _bf16_round(r1 - b2)
    back = b1.astype(np.float64) + b2.astype(np.float64) + b3.astype(np.float64)
    assert np.max(np.abs(back - x.astype(np.float64)) / np.abs(x.astype(np.float64))) <= 2.0 ** -24

    def split(a):
        p1 = _bf16_round(a)
        q = a - p1
        p2 = _bf16_round(q)
        return [p.astype(np.float64) for p in (p1, p2, _bf16_round(q - p2))]
    n, F = 2048, 64
    e = rng.uniform(-44, 0, (n, 1))
    dy = (rng.standard_normal((n, 8)) * 2.0 ** e).astype(np.float32)
    X = np.maximum(rng.standard_normal((n, F)), 0).astype(np.float32)
    X[e[:, 0] > -38] = 0.0                                           # features only where the gradients are small: those rows ARE the result
    a, c = split(dy), split(X)
    got = sum(a[i].T @ c[j] for i in range(3) for j in range(3) if i + j <= 2)
    ref = dy.astype(np.float64).T @ X.astype(np.float64)
    mag = np.abs(dy.astype(np.float64)).T @ np.abs(X.astype(np.float64))
    assert np.max(np.abs(got - ref) / mag) <= 2.0 ** -22
    # one fp16 scale per column (the form this replaced): the small rows vanish below fp16's denormals
    sc = 2.0 ** (14 - np.ceil(np.log2(np.abs(dy).max(0))))
    with np.errstate(under="ignore"):
        h = (dy * sc).astype(np.float16).astype(np.float64)
        lo = ((dy * sc - h) * 2048.0).astype(np.float16).astype(np.float64) / 2048.0
    got16 = ((h + lo) / sc).T @ X.astype(np.float64)
    assert np.max(np.abs(got16 - ref) / mag) > 1e-4                  # (why that form needed its guard)
    tiny = (rng.standard_normal(512) * 1e-36).astype(np.float32)
    t = split(tiny)
    assert np.max(np.abs(t[0] + t[1] + t[2] - tiny.astype(np.float64))) <= 2.0 ** -133


def test_label_propagation_torch_form_equals_the_numpy_form():
    """Round-5 review 7: `reorder: community` ran its label-propagation sweeps on the host (7.4 s of a config-5 model build);
    hip_ops._mode_labels_device is the same integer rule -- most frequent neighbour label, ties to the smallest -- as two torch
    sorts (run on the device when the model is there).  Here, on CPU tensors, against the numpy form; the device run is
    tests/test_hip_parity.py::test_locality_order_on_device_equals_host."""
    import torch
    from mmrec_amd import hip_ops
    rng = np.random.default_rng(3)
    for n, nnz, n_lab in ((500, 4000, 40), (64, 2000, 3), (1000, 300, 1000)):
        rows, cols = np.sort(rng.integers(0, n, nnz)), rng.integers(0, n, nnz)
        lab = rng.integers(0, n_lab, n)
        a = hip_ops._mode_labels(rows, lab[cols], n, n)
        b = hip_ops._mode_labels_device(torch.from_numpy(rows), torch.from_numpy(lab[cols]), n, n).numpy()
        assert np.array_equal(a, b) and (a == -1).sum() == n - np.unique(rows).shape[0]


def test_run_configs_did_not_regress():
    """Round-5 review, next 2: MMGCN's training step once went 3.4 -> 9.5 ms per batch and no table showed it.  Every round
    commits `profiles/rNN_run_configs.json` (tools/run_config.py tier --json: Trainer-level ms per batch of VBPR and the five
    models north_star names, at their BASELINE shapes); this test fails when the newest file is more than 15 % slower than the
    previous round's on any configuration both hold (box-to-box spread of one build is ~5 %)."""
    import glob
    import json
    import os
    import re
    root = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles")
    files = sorted(f for f in glob.glob(os.path.join(root, "r*_run_configs.json")) if re.search(r"r\d+_run_configs\.json$", f))
    assert len(files) >= 2, "need two rounds of profiles/rNN_run_configs.json, found %s" % files
    prev, cur = (json.load(open(f))["configs"] for f in files[-2:])
    tier = {"c1", "c2", "c3", "c4", "lattice", "mmgcn"}
    assert tier <= set(cur), "the newest run-config file lacks %s" % sorted(tier - set(cur))
    worse = {k: (prev[k]["ms_per_batch"], cur[k]["ms_per_batch"]) for k in cur
             if k in prev and cur[k]["ms_per_batch"] > 1.15 * prev[k]["ms_per_batch"]}
    assert not worse, "ms per batch regressed by more than 15 %% (previous round, this round): %s" % worse
    assert cur["mmgcn"]["ms_per_batch"] <= 3.4, cur["mmgcn"]         # the review's bar for the regression it found
