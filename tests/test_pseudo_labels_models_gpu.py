"""GPU: DAMRS with `fused_labels: True` (hip_ops.pseudo_labels, csrc/tri_topk.hip) on the reference's golden step --
tests/golden/damrs.npz, set up as tests/test_models_gpu.py::test_damrs_model sets it up -- at that test's tolerances; the kernels
are really taken (library calls counted); the step's peak memory against the key-off step's; the labels against the key-off
labels wherever float64 separates rank 10 from rank 11 by more than the fuzz's derived tolerance; a four-epoch Trainer.fit."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import tests.test_pseudo_labels_fuzz_gpu as Z
from tests.test_models_gpu import build
from tests.test_pseudo_labels_cpu import DAMRS_EXTRA, TARGETS, damrs_step, meets_the_golden

pytestmark = pytest.mark.gpu


def _spy(m):
    """count the library's tri-modal top-k calls and hip_ops.score_lse calls"""
    from mmrec_amd import _lib, hip_ops
    lib = _lib.load()
    calls = {"mmrec_tri_topk_f32": 0, "mmrec_list_exclude_i32": 0, "score_lse": 0}
    for fn in ("mmrec_tri_topk_f32", "mmrec_list_exclude_i32"):
        def spy(*a, _real=getattr(lib, fn), _fn=fn):
            calls[_fn] += 1
            return _real(*a)
        m.setattr(lib, fn, spy)

    def lse(*a, _real=hip_ops.score_lse, **kw):
        calls["score_lse"] += 1
        return _real(*a, **kw)
    m.setattr(hip_ops, "score_lse", lse)
    return calls


def test_damrs_golden_step_with_fused_labels(tmp_path, golden, monkeypatch):
    peaks = {}

    def measured(key):
        def start(model):
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            peaks[key] = torch.cuda.memory_allocated()
        return start

    def stop(key):
        torch.cuda.synchronize()
        peaks[key] = torch.cuda.max_memory_allocated() - peaks[key]
    damrs_step(tmp_path / "warm", golden, {})            # whatever the libraries allocate once is allocated before either measurement
    with monkeypatch.context() as m:
        calls = _spy(m)
        m0, loss0, g0, g = damrs_step(tmp_path / "off", golden, {}, before_loss=measured("off"))
        stop("off")
        assert m0.fused_labels is False and not any(calls.values()), calls
        m1, loss1, g1, _ = damrs_step(tmp_path / "on", golden, {"fused_labels": True}, before_loss=measured("on"))
        stop("on")
        assert m1.fused_labels is True
        assert calls == {"mmrec_tri_topk_f32": 1, "mmrec_list_exclude_i32": 1, "score_lse": 6}, calls
    print("loss key-off %.8f key-on %.8f golden %.8f; peak above the step's start: key-off %d B, key-on %d B"
          % (float(loss0), float(loss1), float(g["loss1"]), peaks["off"], peaks["on"]))
    meets_the_golden(loss0, g0, g)
    meets_the_golden(loss1, g1, g)
    assert peaks["on"] < peaks["off"], peaks


def test_key_on_labels_are_the_key_off_labels_away_from_near_ties(tmp_path, golden):
    from mmrec_amd import hip_ops
    from mmrec_amd.models.damrs import DAMRS
    model, _, _, g = damrs_step(tmp_path, golden, {"fused_labels": True})
    batch = torch.as_tensor(g["batch1"]).to(model.device)
    k = 10
    with torch.no_grad():
        _, _, h_t, h_v, h_s = model.forward()
        i_id = torch.unique(torch.cat((batch[1], batch[2])))
        hn = [hip_ops.row_normalize(h) for h in (h_t, h_v, h_s)]
        assert hip_ops.tri_softmax_topk_served(hn, i_id, torch.empty(3, i_id.numel(), device=model.device), torch.ones(3, 3, device=model.device), k)
        mm_on, s_on = hip_ops.pseudo_labels(hn, i_id, k)
        p = [F.softmax(DAMRS._cosine_block(h[i_id], h), dim=1) for h in (h_t, h_v, h_s)]
        off = {m: DAMRS._pseudo_labels(p[a], p[o], p[m]) for a, o, m in TARGETS}
    c = Z.Case()
    c.T = [x.cpu().numpy() for x in hn]
    c.rows = i_id.cpu().numpy()
    c.B, c.N, c.k, c.W = c.rows.size, c.T[0].shape[0], k, (np.ones((3, 3)) + np.eye(3)).astype(np.float32)
    c.valid, c.dup = np.ones(c.B, bool), np.arange(c.N)
    S, eps = Z.scores64(c), Z.eps_rows(c)
    l64 = Z.lse64(c)
    compared = [0, 0]
    for m in range(3):
        T64 = c.T[m].astype(np.float64)
        pm = np.exp(T64[c.rows] @ T64.T - l64[m][:, None])
        for r in range(c.B):
            s = np.sort(S[m, r])[::-1]
            if s[k - 1] - s[k] <= 2 * eps[r] * s[k - 1]:
                continue
            on, ref = sorted(mm_on[m, r].tolist()), sorted(off[m][0][r].tolist())
            assert on == ref, ("mm_pos", m, r, on, ref)
            compared[0] += 1
            rest = pm[r].copy()
            rest[ref] = 0.0
            s2 = np.sort(rest)[::-1]
            if s2[k - 1] - s2[k] <= 2 * eps[r] * s2[k - 1]:
                continue
            on, ref = sorted(s_on[m, r].tolist()), sorted(off[m][1][r].tolist())
            assert on == ref, ("single_pos", m, r, on, ref)
            compared[1] += 1
    print("rows compared: mm_pos %d, single_pos %d of %d" % (compared[0], compared[1], 3 * c.B))
    assert compared[0] >= 2 * c.B and compared[1] >= 2 * c.B


def test_pseudo_labels_in_query_blocks_are_the_same_lists(monkeypatch):
    """the top-2k cosines come in blocks of query rows once b rows x N columns of scores exceed PSEUDO_TOPK_BLOCK_BYTES: b = 300
    as one block and as three give the same lists, and they are the dense composition's away from near-ties (float64 as above)"""
    from mmrec_amd import hip_ops
    c = Z.case(39)                                                   # B 300, N 700, random unit tables
    T = [torch.from_numpy(t).to("cuda:0") for t in c.T]
    ids = torch.sort(torch.randperm(c.N, generator=torch.Generator().manual_seed(1))[:c.B]).values.to("cuda:0")
    calls = []
    monkeypatch.setattr(hip_ops, "score_topk", lambda Q, *a, _real=hip_ops.score_topk, **kw: calls.append(Q.shape[0]) or _real(Q, *a, **kw))
    one = hip_ops.pseudo_labels(T, ids)
    assert calls == [300] * 3
    monkeypatch.setattr(hip_ops, "PSEUDO_TOPK_BLOCK_BYTES", 1)
    blocks = hip_ops.pseudo_labels(T, ids)
    assert calls[3:] == [128, 128, 44] * 3
    assert torch.equal(one[0], blocks[0]) and torch.equal(one[1], blocks[1])
    dense = hip_ops.pseudo_labels_torch(T, ids)
    same = [float((torch.sort(a, dim=-1).values == torch.sort(b, dim=-1).values).all(dim=-1).float().mean()) for a, b in zip(one, dense)]
    print("share of lists equal to the dense composition's: mm_pos %.4f single_pos %.4f" % tuple(same))
    assert min(same) >= 0.95                                         # the leniency cap of the fuzz


def test_four_epochs_with_fused_labels(tmp_path, golden):
    from mmrec_amd.common.trainer import Trainer
    os.makedirs(os.path.join(str(tmp_path), "baby"), exist_ok=True)
    np.save(os.path.join(str(tmp_path), "baby", "item_graph_dict_2.npy"),
            {i: [[(i + 1) % 90, (i + 7) % 90], [1.0, 1.0]] for i in range(0, 90, 2)}, allow_pickle=True)
    cfg = dict(DAMRS_EXTRA, fused_labels=True, epochs=4, learning_rate=0.01)
    config, train_data, valid_data, model = build(tmp_path, golden, "DAMRS", cfg)
    assert model.fused_labels is True
    config["epochs"], config["learning_rate"] = 4, 0.01
    trainer = Trainer(config, model)
    trainer.fit(train_data, valid_data=valid_data, test_data=valid_data, verbose=False)
    losses = [trainer.train_loss_dict[e] for e in sorted(trainer.train_loss_dict)]
    print("losses with fused_labels:", losses)
    assert len(losses) == 4 and all(np.isfinite(losses)) and losses[-1] < losses[0]
