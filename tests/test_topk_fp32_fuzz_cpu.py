"""CPU: the generator, the restated plan and the checker body of tests/test_topk_fp32_fuzz_gpu.py.

* the cases the GPU box runs span every path label, every split count 1 .. 16, every width and mask kind
  (`test_cases_span_every_axis`), and the restated `workspace_bytes` equals `mmrec_topk_workspace_bytes` for each of them
  (`test_workspace_query_equals_the_restated_plan`: the library loads without a device) -- a plan change that moves cases off a
  path fails here;
* generator + checker run on scaled-down cases against the torch-CPU stand-in of tests/_cpu_ops.py;
* the checker rejects what these paths can get wrong (`test_checker_rejects_planted_errors`)."""
import os

import numpy as np
import pytest
import torch

import tests.test_topk_fp32_fuzz_gpu as F
from tests._cpu_ops import cpu_ops  # noqa: F401  (fixture)
from tests.test_topk_fuzz_gpu import check_lists


def test_cases_span_every_axis():
    cases = F.CASES
    plans = [F.topk_plan(c["nq"], c["nc"], c["kd"], c["k"]) for c in cases]
    assert {c["path"] for c in cases} == set(F.PATHS)                         # no case on the fp16 paths, every fp32 path drawn
    by_path = {p: [(c, pl) for c, pl in zip(cases, plans) if c["path"] == p] for p in F.PATHS}
    fused = by_path["fused"]
    assert {pl.n_split for c, pl in fused if c["fam"] == 1} == set(range(1, 17))
    assert {c["kd"] for c, _ in fused if c["fam"] == 1} == set(F.F1_KD) and all(c["kd"] % 32 for c, _ in fused if c["fam"] == 1)
    assert {1, 2, 31, 32, 33, 63, 64} <= {c["k"] for c, _ in fused} and max(c["k"] for c, _ in fused) == 64
    assert set(F.F1_NQ) <= {c["nq"] for c, _ in fused}
    assert {1, 31, 32, 33, 63, 64, 65} <= {c["nc"] for c, _ in fused} and any(c["k"] == c["nc"] for c, _ in fused)
    assert any(pl.n_split * c["k"] == 512 and c["k"] == 32 for c, pl in fused) and any(pl.n_split * c["k"] == 512 and c["k"] == 64 for c, pl in fused)
    for k in F.F1_K:                                                          # both sides of nc = 4k, 8k, 64k
        for mult in (4, 8, 64):
            assert {mult * k - 1, mult * k} <= {c["nc"] for c, _ in fused if c["k"] == k} or mult * k - 1 < k, (k, mult)
    assert any(c["special"] == "ascending" and pl.n_split > 1 for c, pl in fused)
    # above 2,097,152 candidates: at most three cases, 33 queries, two-pass with splits, the fused form wide and narrow
    big = [(c, pl) for c, pl in zip(cases, plans) if c["fam"] == 2]
    assert len(big) <= 3 and all(c["nq"] == 33 and c["nc"] > 2 << 20 for c, _ in big) and {c["kd"] for c, _ in big} == {64, 128, 4}
    assert {c["nc"] for c, _ in big} == {(2 << 20) + 1, (2 << 20) + 4096 + 17} and {c["k"] for c, _ in big} == {1, 50, 64}
    assert all(pl.two_pass and pl.n_split > 1 and pl.n_groups <= 128 for c, pl in by_path["two_pass"])
    assert F.path_label(33, 2 << 20, 64, 50, F.NO_FILTER) == "mat64" and F.path_label(33, 2 << 20, 4, 1, 0) == "fused"
    assert F.path_label(33, 2 << 20, 96, 50, 0) == "matgen" and F.path_label(33, (2 << 20) + 1, 96, 50, 0) == "fused"
    assert all(c["fam"] in (2, 5) or c["nq"] * c["nc"] <= F.WORK for c in cases)
    # the block paths
    assert {32, 96, 128, 160, 192, 256, 384, 512} == {c["kd"] for c, _ in by_path["matgen"]}
    assert all(c["nc"] < 4096 for c, _ in by_path["matgen"] if c["kd"] <= 128 or c["kd"] in (160, 256, 512))
    assert all(c["nc"] >= 4096 and 32 < c["k"] <= 128 for c, _ in by_path["matgen"] if c["kd"] in (192, 384))
    for p in ("matgen", "mat64"):
        ks = {c["k"] for c, _ in by_path[p]}
        assert {65, 128} <= ks and {1, 64} <= ks and any(c["nc"] < 2 * c["k"] for c, _ in by_path[p]), p
    ncs = np.array([c["nc"] for c, _ in by_path["mat64"] if c["flags"] & F.NO_FILTER])
    for edge in F._NC_EDGES:
        assert (ncs == edge - 1).any() or edge == 4096, edge
        assert (ncs == edge + 1).any(), edge
    assert any(c["nc"] == 4095 and c["flags"] == 0 for c, _ in by_path["mat64"])
    assert all(c["flags"] == 0 for c, _ in by_path["mat64"] if c["nc"] < 4096)
    # heavy users whose k + m exceeds the <= 384 group maxima of the streaming GEMM: the bound's fallback
    assert any("heavy" in F.KIND_TAGS[c["kind"]] and c["nc"] >= 4096 for c, _ in by_path["mat64"])
    (c5, p5), = by_path["mat64_blocks"]
    assert c5["nc"] > 1_000_000 and p5.qb_rows < c5["nq"] <= 2 * p5.qb_rows and not F.filter_applicable(c5["nq"], c5["nc"], 64, c5["k"])
    assert F.workspace_bytes(c5["nq"], c5["nc"], 64, c5["k"]) < 6 << 30
    # each mask kind on each path (the two single-case paths also run without a mask: special == "unmasked_too")
    for p in F.PATHS:
        tags = set().union(*[F.KIND_TAGS[c["kind"]] for c, _ in by_path[p]])
        if any(c["special"] == "unmasked_too" for c, _ in by_path[p]):
            tags.add("none")
        assert tags == set(F.MASK_TAGS), (p, tags)


def test_generator_is_deterministic_and_masks_what_it_says():
    for i in (0, 40, F.N_CASES - 1):
        a, b = F.gen_case(i, small=True), F.gen_case(i, small=True)
        assert np.array_equal(a["Q"], b["Q"]) and np.array_equal(a["C"], b["C"]) and a["tags"] == b["tags"]
        assert (a["mask"] is None and b["mask"] is None) or np.array_equal(a["mask"], b["mask"])
    seen = set()
    for i, meta in enumerate(F.CASES):
        if meta["nq"] * meta["nc"] > 2e6:
            continue
        c = F.gen_case(i)
        seen |= set(c["tags"])
        if "fill" in c:                         # one split entirely masked for one user, another split starts on a masked id
            q, (a, b), first = c["fill"]
            mine = set(c["mask"][1][c["mask"][0] == q].tolist())
            assert set(range(a, b)) <= mine and first in mine and first in {r[0] for r in F.split_ranges(c["nq"], c["nc"], c["kd"], c["k"])}
            seen.add("fill")
        if "starved" in c:
            q, keep = c["starved"]
            assert c["nc"] - int((c["mask"][0] == q).sum()) <= keep <= c["k"]
    assert {"qspread", "cspread", "outliers", "zeroq", "ties", "dupq", "ascending", "fill"} <= seen, seen


@pytest.fixture(scope="module")
def lib():
    from mmrec_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        from mmrec_amd.build import build
        build(verbose=False)
    return _lib.load()


def test_workspace_query_equals_the_restated_plan(lib):
    """one formula per path in mmrec_topk_workspace_bytes: the restatement (and with it every path label) follows the library"""
    shapes = [(c["nq"], c["nc"], c["kd"], c["k"]) for c in F.CASES]
    shapes += [(nq, 4100, 64, 20) for nq in (96, 1, 12, 193, 289, 300)]                     # family 6, whole and in blocks
    shapes += [(1152, 1_000_001, 64, 50), (897, 1_000_001, 64, 50)]                         # family 5's blocks alone
    shapes += [(33, 2 << 20, 64, 50), (200, 20000, 192, 32), (700, 300_000, 128, 128), (19445, 7050, 64, 50), (8, 200, 260, 64)]
    for s in shapes:
        assert lib.mmrec_topk_workspace_bytes(*s) == F.workspace_bytes(*s) > 0, s
    for s in ((0, 10, 64, 5), (10, 0, 64, 5), (10, 10, 0, 5), (10, 10, 64, 0)):
        assert lib.mmrec_topk_workspace_bytes(*s) == F.workspace_bytes(*s) == 0, s
    for nc, kd in ((4096, 64), (131072, 128), (1_000_000, 64), (4095, 64), (1_000_001, 64), (5000, 96)):
        assert lib.mmrec_topk_prepared_bytes(nc, kd) == (F.filter_prepared_bytes(nc, kd) if F.filter_applicable(1, nc, kd, 1) else 0)


def standin_run(c, mask):
    from mmrec_amd import hip_ops             # its op entry points are the stand-ins while the `cpu_ops` fixture is active
    rp, col = (None, None) if mask is None else hip_ops.mask_to_csr(mask, c["nq"], torch.device("cpu"))
    return hip_ops.score_topk(torch.from_numpy(c["Q"]), torch.from_numpy(c["C"]), c["k"], rp, col, return_values=True)


@pytest.mark.parametrize("i", range(F.N_CASES), ids=F.case_id)
def test_fuzz_body_on_small_cases(cpu_ops, i):  # noqa: F811
    c = F.gen_case(i, small=True)
    F.check_case(c, standin_run)


# ------------------------------------------------------------------------------------------------ planted errors
def planted_case():
    """65 queries x 5000 candidates of kd = 20, k = 10: 16 splits of 320 candidates, three query waves, every mask kind; on top,
    query 5's two best candidates are an exact tie that straddles splits 0 and 5, and query 32 (the seam of 32-query blocks) has
    its best candidates masked while query 31 has not"""
    i = next(j for j, c in enumerate(F.CASES) if (c["nc"], c["kd"], c["k"], c["special"]) == (5000, 20, 10, None))
    c = F.gen_case(i)
    c.update(nq=65, kind="mix")
    rng = np.random.default_rng(99)
    c["Q"] = (rng.standard_normal((65, 20)) * 0.2).astype(np.float32)
    c["C"] = (rng.standard_normal((5000, 20)) * 0.2).astype(np.float32)
    c["C"][7] = c["C"][1700] = c["Q"][5] * np.float32(4.0)
    rg = F.split_ranges(65, 5000, 20, 10)
    assert len(rg) == 16 and rg[0][0] <= 7 < rg[0][1] and rg[5][0] <= 1700 < rg[5][1]
    s = c["Q"] @ c["C"].T
    best32 = np.argsort(-s[32])[:3]
    keep = np.array([11, 222, 3333])                                       # query 40 is starved: 3 candidates left
    drop = np.setdiff1d(np.arange(5000), keep)
    rows = np.concatenate([np.repeat(np.arange(65), 4), np.full(3, 32), np.full(drop.shape[0], 40), np.full(321, 50)])
    cols = np.concatenate([rng.integers(2000, 5000, 65 * 4), best32, drop, np.arange(*rg[3]), [rg[9][0]]])   # query 50: all of split 3, the first id of split 9
    ok = ~(((rows == 5) & np.isin(cols, (7, 1700))) | ((rows == 31) & np.isin(cols, np.argsort(-s[31])[:10])))
    key = np.unique(rows[ok].astype(np.int64) * 5000 + cols[ok])
    c.update(mask=np.stack([key // 5000, key % 5000]), check_rows=None, special=None, plan=F.topk_plan(65, 5000, 20, 10))
    return c, rg


def exact_lists(c, mask, drop=None):
    """what the kernels are specified to return, from fp32 scores; `drop` = (row, a, b): candidates [a, b) never reach row's list"""
    s = torch.from_numpy(c["Q"]) @ torch.from_numpy(c["C"]).t()
    s[torch.as_tensor(mask[0]), torch.as_tensor(mask[1])] = -1e10
    if drop is not None:
        s[drop[0], drop[1]:drop[2]] = float("-inf")
    val, idx = torch.sort(s, dim=1, descending=True, stable=True)
    return idx[:, :c["k"]].contiguous(), val[:, :c["k"]].contiguous()


PLANTS = ("split_dropped", "cursor_at_c_begin", "tie_across_splits", "padding_minus_one", "padding_int_max", "tail_value_inf",
          "tail_value_one_ulp", "second_wave_reads_first", "seam_row_neighbour_mask")


def plant(how, c, rg):
    mask, k = c["mask"], c["k"]
    idx, val = exact_lists(c, mask)
    if how == "split_dropped":                 # the split that holds query 3's best candidate hands nothing over
        a, b = next(r for r in rg if r[0] <= int(idx[3, 0]) < r[1])
        idx, val = exact_lists(c, mask, drop=(3, a, b))
    elif how == "cursor_at_c_begin":           # query 50's mask cursor starts one entry late in split 9: its first id is ranked
        first = rg[9][0]
        assert ((mask[0] == 50) & (mask[1] == first)).any()
        sc = float(c["Q"][50] @ c["C"][first])
        pos = int((val[50] >= sc).sum())
        pos = min(pos, k - 1)
        idx[50, pos + 1:], val[50, pos + 1:] = idx[50, pos:-1].clone(), val[50, pos:-1].clone()
        idx[50, pos], val[50, pos] = first, max(sc, float(val[50, -1]))
    elif how == "tie_across_splits":           # the merge ranks the higher id of an exact tie first
        assert idx[5, :2].tolist() == [7, 1700] and val[5, 0] == val[5, 1]
        idx[5, :2] = idx[5, :2].flip(0)
    elif how == "padding_minus_one":           # a split's padding (-1 / INT_MAX) reaches a row that has k candidates
        idx[9, -1] = -1
    elif how == "padding_int_max":
        idx[9, -1] = 2 ** 31 - 1
    elif how == "tail_value_inf":              # query 40 keeps 3 candidates: the tail is masked ids at exactly float32(-1e10)
        assert (val[40, 3:] == -1e10).all() and (val[40, :3] > -1e10).all()
        val[40, 3:] = float("-inf")
    elif how == "tail_value_one_ulp":
        val[40, -1] = float(np.nextafter(np.float32(-1e10), np.float32(-np.inf)))
    elif how == "second_wave_reads_first":     # lane q - 32's list
        idx[33], val[33] = idx[1].clone(), val[1].clone()
    elif how == "seam_row_neighbour_mask":     # the first row of the second 32-query block is ranked under the mask of the row before it
        wrong = mask.copy()
        own, prev = wrong[0] == 32, wrong[0] == 31
        wrong = np.concatenate([wrong[:, ~own], np.stack([np.full(int(prev.sum()), 32), wrong[1][prev]])], axis=1)
        wi, wv = exact_lists(c, wrong)
        idx[32], val[32] = wi[32], wv[32]
    return idx, val


def test_checker_passes_the_exact_lists_of_the_planted_case():
    c, _ = planted_case()
    check_lists("exact", *exact_lists(c, c["mask"]), torch.from_numpy(c["Q"]), torch.from_numpy(c["C"]), c["mask"], c["k"])


@pytest.mark.parametrize("how", PLANTS)
def test_checker_rejects_planted_errors(how):
    c, rg = planted_case()
    idx, val = plant(how, c, rg)
    ref = exact_lists(c, c["mask"])
    assert not (torch.equal(idx, ref[0]) and torch.equal(val, ref[1])), "nothing was planted"
    with pytest.raises(AssertionError):
        check_lists(how, idx, val, torch.from_numpy(c["Q"]), torch.from_numpy(c["C"]), c["mask"], c["k"])
