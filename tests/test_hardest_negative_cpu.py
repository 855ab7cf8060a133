"""No GPU: the hardest-negative loss's exports, argument checks, B == 0 contract and plan (csrc/hardest_neg.hip);
hip_ops.hardest_negative_loss on CPU tensors is `hardest_negative_loss_torch`, equal in float64 to the reference's own [B, B, 64]
formulation (restated here) in value and Z gradient for `squash` both ways, and MVGAE.recon_loss bit for bit in fp32; MVGAE's
`fused_recon` key absent / False / True on the CPU against the reference's golden; and the checker of
tests/test_hardest_negative_fuzz_gpu.py held honest: an fp32 numpy emulation of the kernels' plan as include/mmrec_hip.h states it
passes it on the fuzz's own cases, three planted errors do not; E_L1P is measured here."""
import os

import numpy as np
import pytest
import torch

import tests.test_hardest_negative_fuzz_gpu as Z
import tests.test_models_gpu as G
from mmrec_amd import _lib
from tests._cpu_ops import cpu_ops  # noqa: F401  (fixture)
from tests.test_hyper_cpu import deterministic_torch, fma32, lib  # noqa: F401  (fixtures)
from tests.test_posterior_fusion_cpu import _step

EXPORTS = ("mmrec_hardest_neg_split_cols", "mmrec_hardest_neg_workspace_bytes", "mmrec_hardest_neg_fwd_f32",
           "mmrec_hardest_neg_bwd_f32")
BAD = 10001
F32 = np.float32
D = 64
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_exports_in_header_signatures_and_library(lib):  # noqa: F811
    src = open(os.path.join(ROOT, "include", "mmrec_hip.h")).read()
    for name in EXPORTS:
        assert name in _lib.SIGNATURES and name in src and hasattr(lib, name), name
    assert "#define MMREC_ABI_VERSION 16" in src and lib.mmrec_abi_version() == 16 and _lib.ABI_VERSION == 16   # additive
    from mmrec_amd.build import SOURCES
    assert "hardest_neg.hip" in SOURCES
    assert "B == 0 CONTRACT" in src                                        # written where callers read it


def test_entry_points_refuse_bad_arguments_before_touching_memory(lib):  # noqa: F811
    """every call below would fault if a pointer were followed or a kernel launched: this machine has no device"""
    fw, bw = lib.mmrec_hardest_neg_fwd_f32, lib.mmrec_hardest_neg_bwd_f32
    one = 1                                                                # a non-NULL pointer that must never be followed
    f = lambda N, L, d, B, ptrs=(one,) * 9: fw(ptrs[0], N, L, d, ptrs[1], ptrs[2], ptrs[3], B, 1, *ptrs[4:], None)    # noqa: E731
    b = lambda N, L, d, B, ptrs=(one,) * 9: bw(ptrs[0], N, L, d, ptrs[1], ptrs[2], ptrs[3], B, 1, *ptrs[4:], None)    # noqa: E731
    for d in (0, 32, 63, 65, 128):                                         # the width is 64
        assert f(10, 1, d, 5) == BAD and b(10, 1, d, 5) == BAD and f(10, 1, d, 0) == BAD, d
    for L in (-1, 0, 9, 1 << 20):                                          # 1 .. 8 latents
        assert f(10, L, 64, 5) == BAD and b(10, L, 64, 5) == BAD, L
    for B in (-1, 65537, 1 << 30):                                         # 0 .. 65,536 samples
        assert f(10, 1, 64, B) == BAD and b(10, 1, 64, B) == BAD, B
    for N in (-1, 0, (1 << 30) + 1, 1 << 40):                              # 1 .. 2^30 rows
        assert f(N, 1, 64, 5) == BAD and b(N, 1, 64, 5) == BAD, N
    for hole in range(9):                                                  # a NULL input, output or workspace
        ptrs = [one] * 9
        ptrs[hole] = None
        assert f(10, 1, 64, 5, ptrs) == BAD, hole
        if hole != 8:
            assert b(10, 1, 64, 5, ptrs) == BAD, hole
    assert b(10, 1, 64, 5, [one] * 8 + [None]) == 0                        # no G wanted: nothing to do, no pointer followed
    # B == 0: 0 before any pointer is looked at; nothing is launched, so loss keeps the caller's bytes
    assert f(10, 1, 64, 0, [None] * 9) == 0 and b(10, 1, 64, 0, [None] * 9) == 0
    import ctypes
    loss = (ctypes.c_float * 8)(*[7.5] * 8)
    rc = fw(None, 10, 8, 64, None, None, None, 0, 1, ctypes.cast(loss, ctypes.c_void_p), None, None, None, None, None)
    assert rc == 0 and list(loss) == [7.5] * 8


def test_plan_and_workspace(lib):  # noqa: F811
    """the plan is a function of (B, L) alone: ceil(B / 64) tiles over at most 16 splits, about ceil(512 / L) workgroups a latent"""
    sc, wsb = lib.mmrec_hardest_neg_split_cols, lib.mmrec_hardest_neg_workspace_bytes
    for B, L in ((0, 1), (-1, 1), (65537, 1), (5, 0), (5, 9)):
        assert sc(B, L) == 0 and wsb(B, L) == 0, (B, L)

    def hand(B, L):
        own, tiles = -(-B // 128), -(-B // 64)
        want = max(1, min(-(-(-(-512 // L)) // own), 16, tiles))
        per = -(-tiles // want)
        return 64 * per, -(-tiles // per)
    edges = [1, 63, 64, 65, 127, 128, 129, 1023, 1024, 1025, 1151, 1152, 1153, 2047, 2048, 2049, 4096, 4097, 65535, 65536]
    for B in edges:
        for L in range(1, 9):
            cols, splits = hand(B, L)
            assert sc(B, L) == cols and wsb(B, L) == 4 * (2 * splits + 1) * L * B and splits <= 16, (B, L, sc(B, L), cols)
            assert Z.split_cols(B, L) == cols and Z.n_splits(B, L) == splits
    assert (sc(2048, 4), wsb(2048, 4)) == (256, 4 * 17 * 4 * 2048)          # the shipped batch: 16 x 8 x 4 = 512 workgroups
    assert sc(64, 1) == 64 and sc(65, 1) == 64 and sc(1025, 1) == 128 and sc(65536, 8) == 65536
    assert Z.n_additions(2048) == 2 + 6 + 16 and Z.n_additions(1) == 1 + 6 + 16


def test_served_is_about_device_dtype_shape_and_width():
    from mmrec_amd import hip_ops

    class OnDevice(torch.Tensor):                                    # a stand-in that says it lives on the device
        is_cuda = True
    dev = lambda t: t.as_subclass(OnDevice)                          # noqa: E731
    z, ids = torch.zeros(4, 6, 64), [torch.zeros(5, dtype=torch.int64) for _ in range(3)]
    served = hip_ops.hardest_negative_loss_served
    assert not served(z, *ids) and not served(dev(z), *ids) and not served(z, *[dev(t) for t in ids])       # CPU tensors: never
    assert served(dev(z), *[dev(t) for t in ids])
    for bad in (torch.zeros(4, 6, 32), torch.zeros(6, 64), torch.zeros(9, 6, 64), torch.zeros(0, 6, 64), torch.zeros(4, 0, 64),
                torch.zeros(4, 6, 64).double(), torch.zeros(4, 6, 128)[:, :, ::2], None):
        assert not served(None if bad is None else dev(bad), *[dev(t) for t in ids]), getattr(bad, "shape", None)
    for at in range(3):
        for bad in (torch.zeros(4, dtype=torch.int64), torch.zeros(5, dtype=torch.int32), torch.zeros(5, 1, dtype=torch.int64),
                    torch.zeros(10, dtype=torch.int64)[::2], torch.zeros(0, dtype=torch.int64), None):
            lst = [dev(t) for t in ids]
            lst[at] = None if bad is None else dev(bad)
            assert not served(dev(z), *lst), (at, getattr(bad, "shape", None))
    assert not served(dev(z), *[dev(torch.zeros(0, dtype=torch.int64)) for _ in range(3)])
    assert served(dev(torch.zeros(8, 1, 64)), *[dev(torch.zeros(65536, dtype=torch.int64)) for _ in range(3)])
    assert not served(dev(z), *[dev(torch.zeros(65537, dtype=torch.int64)) for _ in range(3)])
    try:
        hip_ops.HARDEST_NEGATIVE = False
        assert not served(dev(z), *[dev(t) for t in ids])
    finally:
        hip_ops.HARDEST_NEGATIVE = True


def reference_formulation(z, users, pos, neg, squash):
    """the reference's reconstruction term with its [B, B, 64] block (models/mvgae.py:73-89,164-170), restated"""
    s = torch.sigmoid(z) if squash else z
    block = s[users].unsqueeze(1) * s[neg].unsqueeze(0)                  # every user against every negative of the batch
    hardest = block.sum(dim=-1).max(dim=-1).values
    positive = torch.sigmoid((s[users] * s[pos]).sum(dim=1))
    return -torch.log2(torch.sigmoid(positive - torch.sigmoid(hardest))).sum()


def test_cpu_tensors_take_the_torch_path_the_reference_formula_and_recon_loss(cpu_ops, deterministic_torch):  # noqa: F811
    from mmrec_amd import hip_ops
    import mmrec_amd.models.mvgae as mv
    rng = np.random.default_rng(11)
    L, N, B = 3, 41, 29
    z32 = torch.from_numpy(rng.standard_normal((L, N, D)).astype(F32))
    users, pos, neg = (torch.from_numpy(rng.integers(0, N, B)) for _ in range(3))
    w = torch.from_numpy(rng.uniform(0.5, 2.0, L))
    for squash in (True, False):
        zs = z32 * (1.0 if squash else 0.2)
        runs = []
        for fn in (hip_ops.hardest_negative_loss, hip_ops.hardest_negative_loss_torch):
            z = zs.clone().requires_grad_()
            assert not hip_ops.hardest_negative_loss_served(z, users, pos, neg)
            loss, arg = fn(z, users, pos, neg, squash=squash, return_arg=True)
            assert loss.shape == (L,) and arg.shape == (L, B) and arg.dtype == torch.int32 and not arg.requires_grad
            (loss * w.float()).sum().backward()
            runs.append((loss.detach(), arg, z.grad))
        assert all(torch.equal(a, b) for a, b in zip(*runs))
        assert torch.equal(fn(zs, users, pos, neg, squash=squash), runs[0][0])                       # return_arg off: the loss alone
        # float64: the reference's formulation, value and gradient
        z = zs.double().requires_grad_()
        loss = hip_ops.hardest_negative_loss(z, users, pos, neg, squash=squash)
        (loss * w).sum().backward()
        z2 = zs.double().requires_grad_()
        ref = torch.stack([reference_formulation(z2[l], users, pos, neg, squash) for l in range(L)])
        (ref * w).sum().backward()
        assert float((loss - ref).abs().max()) <= 1e-12 * float(ref.abs().max())
        assert float((z.grad - z2.grad).abs().max()) <= 1e-12 * float(z2.grad.abs().max()) and float(z2.grad.abs().max()) > 0
        assert float((runs[0][0].double() - ref.detach()).abs().max()) <= 1e-5 * float(ref.abs().max())
    # MVGAE.recon_loss, bit for bit in fp32, value and gradient
    for l in range(L):
        z = z32[l].clone().requires_grad_()
        mine = hip_ops.hardest_negative_loss(z.unsqueeze(0), users, pos, neg)[0]
        mine.backward()
        z2 = z32[l].clone().requires_grad_()
        theirs = mv.MVGAE.recon_loss(None, z2, users, pos, neg)
        theirs.backward()
        assert torch.equal(mine.detach(), theirs.detach()) and torch.equal(z.grad, z2.grad), l
    # the tie rule: equal rows at several positions -- the lowest wins and takes the whole gradient
    z = z32[:1].clone()
    z[0, 7] = 9.0                                                        # the best row for every user
    neg2 = neg.clone()
    neg2[neg2 == 7] = 8
    neg2[[20, 4, 11]] = 7
    z.requires_grad_()
    loss, arg = hip_ops.hardest_negative_loss(z, users, pos, neg2, return_arg=True)
    assert bool((arg == 4).all())


def test_mvgae_fused_recon_key_on_the_cpu(tmp_path, golden, cpu_ops, deterministic_torch, monkeypatch):  # noqa: F811
    """absent, False, True (with and without fused_posterior): each meets the golden at test_mvgae_model's tolerances; absent and
    False are the same path (equal bits) and never ask hip_ops.hardest_negative_loss; True asks it -- once with the stacked
    [4, N, 64] under fused_posterior, four times with [1, N, 64] without -- and never the composition's recon_loss"""
    from mmrec_amd import hip_ops
    import mmrec_amd.models.mvgae as mv
    monkeypatch.setattr(G, "USE_GPU", False)
    g = G._golden("mvgae")
    asked = []
    monkeypatch.setattr(hip_ops, "hardest_negative_loss",
                        lambda *a, _real=hip_ops.hardest_negative_loss, **k: asked.append((tuple(a[0].shape), a[1].shape[0])) or _real(*a, **k))
    _, loss0, g0 = _step(tmp_path / "absent", golden, g, {}, monkeypatch)
    _, loss1, g1 = _step(tmp_path / "off", golden, g, {"fused_recon": False}, monkeypatch)
    _, loss1p, _ = _step(tmp_path / "off_p", golden, g, {"fused_recon": False, "fused_posterior": True}, monkeypatch)
    assert not asked                                                  # absent or False: today's paths, untouched
    assert torch.equal(loss0, loss1) and all(torch.equal(g0[n], g1[n]) for n in g0)
    B = int(np.asarray(g["batch1"]).shape[1])
    with monkeypatch.context() as m:
        m.setattr(mv.MVGAE, "recon_loss", lambda *a, **k: pytest.fail("the composition ran with the key on"))
        model, loss2, g2 = _step(tmp_path / "on", golden, g, {"fused_recon": True}, monkeypatch)
        n = model.n_users + model.n_items
        assert model.fused_recon is True and asked == [((1, n, 64), B)] * 4
        del asked[:]
        m.setattr(mv.torch, "bmm", lambda *a, **k: pytest.fail("the batched composition ran with the key on"))
        model, loss3, g3 = _step(tmp_path / "on_p", golden, g, {"fused_recon": True, "fused_posterior": True}, monkeypatch)
        assert asked == [((4, n, 64), B)]
    assert set(g0) == set(g2) == set(g3) and len(g0) >= 12
    assert abs(float(loss2) - float(loss0)) <= 2e-6 * abs(float(loss0))
    assert abs(float(loss3) - float(loss1p)) <= 2e-6 * abs(float(loss1p))


def test_the_yaml_names_the_key_in_a_comment_only():
    import yaml
    text = open(os.path.join(ROOT, "mmrec_amd", "configs", "model", "MVGAE.yaml")).read()
    assert "# fused_recon: True" in text and "fused_recon" not in yaml.safe_load(text)


# ------------------------------------------------------------------------------------------------ the fuzz's checker
ONE = F32(1.0)
INV = F32(1.4426950408889634)


def emu_sigmoid(z):
    q = np.exp(-np.abs(z).astype(F32)).astype(F32)
    return (np.where(z >= 0, ONE, q) / (ONE + q)).astype(F32)


def emu_chain(a, b):
    """[m, 64] x [n, 64] -> [m, n]: one fma chain from 0 in natural k order"""
    acc = np.zeros((a.shape[0], b.shape[0]), F32)
    for k in range(D):
        acc = fma32(a[:, k:k + 1], b[None, :, k], acc)
    return acc


def emu_tree(term):
    """the finish's tree: thread t adds its samples t, t + 1024, ... from 0; the wave's butterfly; the 16 waves in order"""
    lanes = np.zeros(Z.FINISH_THREADS, F32)
    for b0 in range(0, term.size, Z.FINISH_THREADS):
        part = term[b0:b0 + Z.FINISH_THREADS]
        lanes[:part.size] = (lanes[:part.size] + part).astype(F32)
    w = lanes.reshape(16, 64)
    idx = np.arange(64)
    for m in (32, 16, 8, 4, 2, 1):
        w = (w + w[:, idx ^ m]).astype(F32)
    total = F32(0.0)
    for i in range(16):
        total = F32(total + w[i, 0])
    return total


def emulate(c, g=None, plant=None):
    """fp32 numpy of the plan in include/mmrec_hip.h -> loss, arg, coef, G, dZ; `plant`: one of the errors the checker must see"""
    g = c.g if g is None else g
    L, N, B = c.L, c.N, c.B
    users, pos, neg = c.users, c.pos, c.neg
    S = emu_sigmoid(c.Z) if c.squash else c.Z
    u_ok, p_ok, n_ok = (Z.in_range(x, N) for x in (users, pos, neg))
    row = lambda l, ids, ok: (S[l, np.where(ok, ids, 0)] * ok[:, None]).astype(F32)      # noqa: E731
    out = {"loss": np.zeros(L, F32), "arg": np.full((L, B), -1, np.int32), "coef": np.zeros((L, B, 2), F32),
           "su": np.zeros((L, B, D), F32),
           "G": np.zeros((L, 3 * B, D), F32), "dZ": np.zeros((L, N, D), F32)}
    pad = -(-B // 64) * 64
    for l in range(L):
        up, pp, nn = row(l, users, u_ok), row(l, pos, p_ok), row(l, neg, n_ok)
        tile = np.zeros((pad, D), F32)                                    # the rows as they stand in the tiles: padding is zeros
        tile[:B] = nn
        sc = emu_chain(up, tile)
        cand = np.zeros(pad, bool)
        cand[:B] = n_ok
        if plant == "padding_wins":
            cand[:] = True
        sc = np.where(cand[None, :], sc, -np.inf)
        if plant == "tie_high":
            arg = pad - 1 - np.argmax(sc[:, ::-1], axis=1)
        else:
            arg = np.argmax(sc, axis=1)                                   # the first occurrence: the lowest position
        hmax = sc[np.arange(B), arg]
        ok = u_ok & p_ok & cand.any()
        dp = np.zeros(B, F32)
        for k in range(D):
            dp = fma32(up[:, k], pp[:, k], dp)
        a, sh = emu_sigmoid(dp), emu_sigmoid(np.where(ok, hmax, 0).astype(F32))
        x = (a - sh).astype(F32)
        sp = (np.maximum(-x, F32(0)) + np.log1p(np.exp(-np.abs(x)).astype(F32)).astype(F32)).astype(F32)
        term = (sp * INV).astype(F32)
        sg = (emu_sigmoid(-x) * INV).astype(F32)
        c1 = -(sg * (a * (ONE - a)).astype(F32)).astype(F32)
        c2 = (sg * (sh * (ONE - sh)).astype(F32)).astype(F32)
        out["arg"][l] = np.where(ok, arg, -1)
        out["su"][l] = np.where(ok[:, None], up, F32(0))
        out["coef"][l] = np.where(ok[:, None], np.stack([c1, c2], axis=1), F32(0))
        out["loss"][l] = emu_tree(np.where(ok, term, F32(0)).astype(F32))
    for l in range(L):
        up, pp, nn = row(l, users, u_ok), row(l, pos, p_ok), row(l, neg, n_ok)
        arg = out["arg"][l]
        ok = arg >= 0
        w1, w2 = ((F32(g[l]) * out["coef"][l, :, j]).astype(F32)[:, None] for j in (0, 1))
        chosen = np.where(ok & (arg < B), arg, 0)
        tu = np.where(ok[:, None], fma32(w2, nn[chosen], (w1 * pp).astype(F32)), F32(0))
        tp = np.where(ok[:, None], (w1 * up).astype(F32), F32(0))
        tn = np.zeros((B, D), F32)
        scan = out["arg"][(l + 1) % L] if plant == "wrong_latent" else arg
        for b in np.flatnonzero((scan >= 0) & (scan < B)):                # ascending b
            tn[scan[b]] = fma32(w2[b], up[b], tn[scan[b]])
        t = np.concatenate([tu, tp, tn]).astype(F32)
        own = np.concatenate([up, pp, nn])
        own_ok = np.concatenate([u_ok, p_ok, n_ok])[:, None]
        Gl = (t * (own * (ONE - own)).astype(F32)).astype(F32) if c.squash else t
        out["G"][l] = np.where(own_ok, Gl, F32(0))
        ids = np.concatenate([users, pos, neg])
        for s in np.argsort(ids, kind="stable"):                          # the sorted scatter: a row's slots in position order
            if 0 <= ids[s] < N:
                out["dZ"][l, ids[s]] = (out["dZ"][l, ids[s]] + out["G"][l, s]).astype(F32)
    return out


EMULATED = (0, 1, 2, 4, 5, 7, 8, 9, 10, 15, 16, 17, 18, 20, 21, 22, 23, 26, 27, 28, 33, 39, 41, 43)


@pytest.mark.parametrize("k", EMULATED)
def test_the_emulated_plan_passes_the_checker(k):
    c = Z.case(k)
    with np.errstate(all="ignore"):
        got = emulate(c)
    if c.family == "oor":
        del got["dZ"]                                                     # (the wrapper is never given an id out of range)
    worst = Z.check(c, got, Z.name_of(c))
    print("%s emulated: worst err / bound %s" % (Z.name_of(c), " ".join("%s %.3f" % kv for kv in sorted(worst.items()))))
    assert set(worst) >= {"loss", "coef", "G"}


def test_the_emulation_covers_every_axis():
    cs = [Z.case(k) for k in EMULATED]
    assert {c.family for c in cs} == set(Z.FAMILIES) and {c.L for c in cs} == set(Z.LS) and {c.N for c in cs} == set(Z.NS)
    assert {c.B for c in cs} >= set(Z.SMALL_B) | {Z.edge_B() - 1, Z.edge_B(), Z.edge_B() + 1}
    assert {c.squash for c in cs} == {True, False}


def _tie_case(B, L):
    """the planted winner at three positions on both sides of a tile and of a split"""
    return Z.planted(B, L, [B - 1, 64, 63], squash=True, seed=3)


def test_planted_errors_do_not_pass():
    """a padding row allowed to win; the tie going to the higher position; the neg-slot sum over arg_b == j of the wrong latent"""
    # (1) without the squash and with every score negative, a zero-scoring padding row wins
    c = next(Z.case(k) for k in range(Z.CASES) if Z.case(k).family == "allneg" and Z.case(k).B % 64 and 32 < Z.case(k).B < 200)
    with np.errstate(all="ignore"):
        clean, bad = emulate(c), emulate(c, plant="padding_wins")
    assert max(Z.check(c, clean, "clean").values()) <= 1.0
    assert (bad["arg"] >= c.B).any()
    with pytest.raises(AssertionError, match="arg is no candidate"):
        Z.check(c, {"arg": bad["arg"], "loss": bad["loss"]}, "padding_wins")
    c.neg[[3, c.B - 1]] = c.N, -1                                         # the same with the zero rows of ids out of range
    with np.errstate(all="ignore"):
        clean, bad = emulate(c), emulate(c, plant="padding_wins")
    del clean["dZ"]
    assert max(Z.check(c, clean, "clean").values()) <= 1.0
    assert (bad["arg"] == 3).all()
    with pytest.raises(AssertionError, match="arg is no candidate"):
        Z.check(c, {"arg": bad["arg"], "loss": bad["loss"]}, "padding_wins")
    # (2) the tie
    c = _tie_case(129, 1)
    with np.errstate(all="ignore"):
        clean, bad = emulate(c), emulate(c, plant="tie_high")
    assert (clean["arg"] == 63).all() and (bad["arg"] == 128).all()
    assert max(Z.check(c, clean, "clean").values()) <= 1.0
    with pytest.raises(AssertionError, match="arg is not the reference's|lowest position"):
        Z.check(c, {"arg": bad["arg"]}, "tie_high")
    # (3) the wrong latent's arg in the neg slots
    c = next(Z.case(k) for k in range(Z.CASES) if Z.case(k).family == "gauss" and Z.case(k).L == 4 and 60 < Z.case(k).B < 200
             and Z.case(k).N > 2)
    with np.errstate(all="ignore"):
        clean, bad = emulate(c), emulate(c, plant="wrong_latent")
    assert max(Z.check(c, clean, "clean").values()) <= 1.0
    assert (clean["arg"][0] != clean["arg"][1]).any()
    for key in ("G", "dZ"):
        with pytest.raises(AssertionError, match="beyond the bound|must be exact"):
            Z.check(c, {"arg": clean["arg"], key: bad[key]}, "wrong_latent")


def test_E_L1P_covers_the_softplus():
    """worst error of fp32 log1p (numpy, on the CPU) against float64 in units of u |log1p q| over q in (0, 1] -- the arguments
    exp(-|x|) the softplus gives it: E_L1P is 4 x that, rounded up, and not more than 8 x"""
    rng = np.random.default_rng(3)
    q = np.concatenate([np.exp(-np.abs(rng.uniform(-1.0, 1.0, 200000))), rng.uniform(0.0, 1.0, 200000) ** 4, [1.0]]).astype(F32)
    q = q[q > 0]
    a, b = np.log1p(q).astype(np.float64), np.log1p(q.astype(np.float64))
    worst = float((np.abs(a - b) / (Z.U * np.abs(b))).max())
    print("fp32 log1p against float64, worst error in units of u |log1p q|: %.3f" % worst)
    assert 4.0 * worst <= Z.E_L1P and (Z.E_L1P == 4.0 or Z.E_L1P <= 8.0 * worst), (worst, Z.E_L1P)
