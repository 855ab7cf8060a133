"""No GPU: the modal fusion's exports, argument checks and plan (csrc/modal_fusion.hip); hip_ops.modal_fusion on CPU tensors is
`modal_fusion_torch` and MGCN.forward's fuser bit for bit; MGCN's `fused_fusion` key absent / False / True on the CPU against the
reference's golden; and the checker of tests/test_modal_fusion_fuzz_gpu.py held honest: an fp32 numpy emulation of the kernels'
plan as include/mmrec_hip.h states it passes it on the fuzz's own cases, five planted errors do not."""
import os

import numpy as np
import pytest
import torch

import tests.test_models_gpu as G
import tests.test_modal_fusion_fuzz_gpu as Z
from mmrec_amd import _lib
from tests._cpu_ops import cpu_ops  # noqa: F401  (fixture)
from tests.test_hyper_cpu import deterministic_torch, fma32, lib  # noqa: F401  (fixtures)

EXPORTS = ("mmrec_modal_fusion_rows_per_block", "mmrec_modal_fusion_workspace_bytes", "mmrec_modal_fusion_fwd_f32",
           "mmrec_modal_fusion_bwd_f32")
BAD, UNSUPPORTED = 10001, 10002
F32 = np.float32
D = 64
MGCN_EXTRA = {"cl_loss": 0.01, "learning_rate": 1e-3}


def _golden():
    return dict(np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mgcn.npz")))


def test_exports_in_header_signatures_and_library(lib):  # noqa: F811
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mmrec_hip.h")).read()
    for name in EXPORTS:
        assert name in _lib.SIGNATURES and name in src and hasattr(lib, name), name
    assert "#define MMREC_ABI_VERSION 16" in src and lib.mmrec_abi_version() == 16 and _lib.ABI_VERSION == 16   # additive
    from mmrec_amd.build import SOURCES
    assert "modal_fusion.hip" in SOURCES


def test_entry_points_refuse_bad_arguments_before_touching_memory(lib):  # noqa: F811
    """every call below would fault if a pointer were followed or a kernel launched: this machine has no device"""
    fw, bw = lib.mmrec_modal_fusion_fwd_f32, lib.mmrec_modal_fusion_bwd_f32
    one = 1                                                                # a non-NULL pointer that must never be followed
    for d in (0, 32, 63, 65, 128):                                         # d is 64, checked first
        assert fw(*[None] * 10, 5, d, None, None, None) == UNSUPPORTED, d
        assert bw(*[None] * 12, 5, d, *[None] * 12) == UNSUPPORTED, d
        assert fw(*[None] * 10, -1, d, None, None, None) == UNSUPPORTED, d
    assert fw(*[one] * 10, (1 << 30) + 1, 64, one, one, None) == UNSUPPORTED
    assert bw(*[one] * 12, (1 << 30) + 1, 64, *[one] * 11, None) == UNSUPPORTED
    assert fw(*[one] * 10, -1, 64, one, one, None) == BAD                  # a negative size
    assert bw(*[one] * 12, -1, 64, *[one] * 11, None) == BAD
    assert fw(*[None] * 10, 0, 64, None, None, None) == 0                  # no rows: nothing to do, before the NULL checks
    assert bw(*[None] * 12, 0, 64, *[None] * 12) == 0
    for hole in range(10):                                                 # a NULL operand
        ptrs = [one] * 10
        ptrs[hole] = None
        assert fw(*ptrs, 5, 64, one, one, None) == BAD, hole
        assert bw(*ptrs, one, one, 5, 64, *[one] * 11, None) == BAD, hole
    assert fw(*[one] * 10, 5, 64, None, one, None) == BAD                  # a NULL forward output
    assert fw(*[one] * 10, 5, 64, one, None, None) == BAD
    for hole in range(3, 10):                                              # any weight gradient without a workspace
        outs = [None] * 10
        outs[hole] = one
        assert bw(*[one] * 10, None, None, 5, 64, *outs, None, None) == BAD, hole
    assert bw(*[one] * 10, None, None, 5, 64, *[None] * 10, None, None) == 0          # nothing wanted: nothing to do


def test_plan_and_workspace(lib):  # noqa: F811
    """the plan is a function of the row count alone: a multiple of 64 rows per block, never more than 256 blocks"""
    rpb, wsb = lib.mmrec_modal_fusion_rows_per_block, lib.mmrec_modal_fusion_workspace_bytes
    assert rpb(-1) == 0 and rpb((1 << 30) + 1) == 0 and wsb(-1) == 0 and wsb((1 << 30) + 1) == 0
    for n in (0, 1, 64, 7050, 16384, 16385, 26495, 54255, 1500000, 1 << 30):
        r = rpb(n)
        assert r >= 64 and r % 64 == 0 and -(-n // r) <= 256, (n, r)
        assert r == 64 * max(1, -(-n // 16384))
        assert wsb(n) == 4 * 12544 * Z.blocks(n) <= 256 * 12544 * 4
    assert Z.PART == 12544 and rpb(26495) == 128 and Z.blocks(26495) == 207 and Z.n_finish(26495) == 52 + 3


def _operands(rng, n, requires_grad=False):
    t = lambda *s: torch.from_numpy(rng.standard_normal(s).astype(np.float32))        # noqa: E731
    u = lambda *s: torch.from_numpy(rng.uniform(-0.125, 0.125, s).astype(np.float32))  # noqa: E731
    ops = [t(n, D), t(n, D), t(n, D), u(D, D), u(D), u(1, D), u(D, D), u(D), u(D, D), u(D)]
    return [o.requires_grad_() for o in ops] if requires_grad else ops


def test_served_is_about_device_dtype_shape_and_width():
    from mmrec_amd import hip_ops

    class OnDevice(torch.Tensor):                                    # a stand-in that says it lives on the device
        is_cuda = True
    dev = lambda t: t.as_subclass(OnDevice)                          # noqa: E731
    ops = _operands(np.random.default_rng(0), 6)
    assert not hip_ops.modal_fusion_served(*ops)                     # CPU tensors: never
    assert hip_ops.modal_fusion_served(*[dev(t) for t in ops])
    swaps = ((0, torch.zeros(6, 32)), (1, torch.zeros(7, 64)), (2, torch.zeros(6, 64).double()), (0, torch.zeros(6, 128)[:, ::2]),
             (3, torch.zeros(64, 32)), (3, torch.zeros(64, 64).double()), (4, torch.zeros(1, 64)), (5, torch.zeros(64)),
             (6, torch.zeros(64, 128)[:, ::2]), (9, torch.zeros(63)), (0, None))
    for at, bad in swaps:
        args = [dev(t) for t in ops]
        args[at] = dev(bad) if bad is not None else None
        assert not hip_ops.modal_fusion_served(*args), (at, getattr(bad, "shape", None))
    empty = [dev(torch.zeros(0, 64)) for _ in range(3)] + [dev(t) for t in ops[3:]]
    assert not hip_ops.modal_fusion_served(*empty)
    args = [dev(t) for t in ops]
    args[7] = ops[7]                                                 # one operand on the host
    assert not hip_ops.modal_fusion_served(*args)
    try:
        hip_ops.MODAL_FUSION = False
        assert not hip_ops.modal_fusion_served(*[dev(t) for t in ops])
    finally:
        hip_ops.MODAL_FUSION = True


class _Holder:
    """what MGCN.forward's fuser reads of its model"""


def _model_lines(h, image_embeds, text_embeds, content):
    """models/mgcn.py, the fuser with the `fused_fusion` key off, through the model's own _query and _gate"""
    from mmrec_amd.models.mgcn import MGCN
    w = torch.softmax(torch.cat([MGCN._query(h, image_embeds), MGCN._query(h, text_embeds)], dim=-1), dim=-1)
    common = w[:, 0].unsqueeze(1) * image_embeds + w[:, 1].unsqueeze(1) * text_embeds
    sep_image = MGCN._gate(h.gate_image_prefer, content) * (image_embeds - common)
    sep_text = MGCN._gate(h.gate_text_prefer, content) * (text_embeds - common)
    side = (sep_image + sep_text + common) / 3
    return side, content + side


def test_cpu_tensors_take_todays_inline_composition_bit_for_bit(cpu_ops, deterministic_torch):  # noqa: F811
    """hip_ops.modal_fusion on CPU tensors == modal_fusion_torch == the model's lines, on the golden's weights, outputs and all
    ten gradients; and it IS the formulas of the fuzz file, in float64"""
    from mmrec_amd import hip_ops
    mgc = _golden()
    rng = np.random.default_rng(8)
    n = 37
    names = ("query_common.0.weight", "query_common.0.bias", "query_common.2.weight", "gate_image_prefer.0.weight",
             "gate_image_prefer.0.bias", "gate_text_prefer.0.weight", "gate_text_prefer.0.bias")
    tables = [torch.from_numpy(rng.standard_normal((n, D)).astype(np.float32)) for _ in range(3)]
    gs = [torch.from_numpy(rng.standard_normal((n, D)).astype(np.float32)) for _ in range(2)]
    runs = []
    for how in ("fusion", "torch", "model"):
        ops = [t.clone().requires_grad_() for t in tables] + [torch.as_tensor(mgc["p_" + k]).clone().requires_grad_() for k in names]
        if how == "model":
            h = _Holder()
            h.query_common = torch.nn.Sequential(torch.nn.Linear(D, D), torch.nn.Tanh(), torch.nn.Linear(D, 1, bias=False))
            h.gate_image_prefer = torch.nn.Sequential(torch.nn.Linear(D, D), torch.nn.Sigmoid())
            h.gate_text_prefer = torch.nn.Sequential(torch.nn.Linear(D, D), torch.nn.Sigmoid())
            mods = (h.query_common[0], h.query_common[2], h.gate_image_prefer[0], h.gate_text_prefer[0])
            for mod, (W, b) in zip(mods, ((ops[3], ops[4]), (ops[5], None), (ops[6], ops[7]), (ops[8], ops[9]))):
                del mod._parameters["weight"]
                mod.weight = W                                        # the very leaf tensors, so that .grad lands on them
                if b is not None:
                    del mod._parameters["bias"]
                    mod.bias = b
            outs = _model_lines(h, *ops[:3])
        else:
            assert not hip_ops.modal_fusion_served(*ops)
            outs = (hip_ops.modal_fusion if how == "fusion" else hip_ops.modal_fusion_torch)(*ops)
        sum((o * g).sum() for o, g in zip(outs, gs)).backward()
        runs.append([o.detach() for o in outs] + [t.grad for t in ops])
    for a, b, c in zip(*runs):
        assert a is not None and torch.equal(a, b) and torch.equal(a, c)
    assert all(float(t.abs().max()) > 0 for t in runs[0])
    ops = dict(zip(Z.OPERANDS, [t.numpy() for t in tables] + [mgc["p_" + k].reshape(-1) if k.endswith("2.weight") else mgc["p_" + k]
                                                            for k in names]))
    ref = Z.bounds(ops, [g.numpy() for g in gs], 64, 4)
    for name, got in zip(("side", "out") + Z.GRADS, runs[0]):
        r = ref[name][0]
        assert float(np.abs(got.double().numpy().reshape(r.shape) - r).max()) <= 1e-4 * float(np.abs(r).max()), name


def _step(tmp_path, golden, mgc, extra):
    from mmrec_amd import hip_ops
    config, _, _, model = G.build(tmp_path, golden, "MGCN", dict(MGCN_EXTRA, **extra))
    assert model.fused_fusion is bool(extra.get("fused_fusion", False))
    params = dict(model.named_parameters())
    assert set(params) == {k[2:] for k in mgc if k.startswith("p_")}
    for name, p in params.items():
        G.load(p, mgc["p_" + name])
    ni = model.n_items
    for key in ("image", "text"):                                    # the golden's kNN graphs, as test_mgcn_model pins them
        g_ = hip_ops.CsrGraph.from_coo_host(mgc[key + "_original_adj_idx"], mgc[key + "_original_adj_val"], ni, ni, model.device)
        g_.transpose()
        setattr(model, key + "_original_adj", g_)
    model.train()
    ua, ia, side, content = model.forward(model.norm_adj, train=True)
    G.close(ua, mgc["user_out"], atol=2e-6), G.close(ia, mgc["item_out"], atol=2e-6)
    G.close(side, mgc["side_embeds"], atol=2e-6), G.close(content, mgc["content_embeds"], atol=2e-6)
    loss = model.calculate_loss(torch.as_tensor(mgc["batch1"]).to(model.device))
    loss.backward()
    G.close(loss, mgc["loss1"], rtol=1e-5)
    grads = {n: p.grad.detach().clone() for n, p in params.items() if p.grad is not None}
    for name in ("user_embedding.weight", "item_id_embedding.weight", "image_trs.weight", "query_common.2.weight",
                 "gate_text_prefer.0.bias", "query_common.0.weight", "query_common.0.bias", "gate_image_prefer.0.weight"):
        G.close(grads[name], mgc["g_" + name], rtol=5e-4, atol=1e-8)
    return model, loss.detach(), grads


def test_mgcn_fused_fusion_key_on_the_cpu(tmp_path, golden, cpu_ops, deterministic_torch, monkeypatch):  # noqa: F811
    """absent, False, True: each meets the golden; on CPU tensors the key-on path is the same composition, so loss and gradients
    are bit-equal; only True asks hip_ops.modal_fusion"""
    from mmrec_amd import hip_ops
    monkeypatch.setattr(G, "USE_GPU", False)
    mgc = _golden()
    asked = []
    monkeypatch.setattr(hip_ops, "modal_fusion",
                        lambda *a, _real=hip_ops.modal_fusion: asked.append(tuple(a[0].shape)) or _real(*a))
    _, loss0, g0 = _step(tmp_path / "absent", golden, mgc, {})
    _, loss1, g1 = _step(tmp_path / "off", golden, mgc, {"fused_fusion": False})
    assert not asked                                                  # absent or False: today's path, untouched
    model, loss2, g2 = _step(tmp_path / "on", golden, mgc, {"fused_fusion": True})
    assert asked == [(model.n_users + model.n_items, 64)] * 2          # forward(train=True), then calculate_loss
    assert torch.equal(loss0, loss1) and torch.equal(loss0, loss2)
    assert set(g0) == set(g1) == set(g2) and len(g0) >= 12
    for n in g0:
        assert torch.equal(g0[n], g1[n]) and torch.equal(g0[n], g2[n]), n


def test_the_yaml_names_the_key_in_a_comment_only():
    import yaml
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "mmrec_amd", "configs", "model", "MGCN.yaml")
    text = open(path).read()
    assert "# fused_fusion: True" in text and "fused_fusion" not in yaml.safe_load(text)


# ------------------------------------------------------------------------------------------------ the fuzz's checker
def _exp32(x):
    return np.exp(np.asarray(x, F32)).astype(F32)


def emu_tanh(z):
    q = _exp32(F32(-2.0) * np.abs(z))
    return np.copysign((F32(1.0) - q) / (F32(1.0) + q), z).astype(F32)


def emu_sigmoid(z):
    q = _exp32(-np.abs(z))
    return (np.where(z >= 0, F32(1.0), q) / (F32(1.0) + q)).astype(F32)


def emu_chain(A, B, start):
    """start [r, c] + A [r, 64] B [64, c]: one fma per summed index, ascending"""
    acc = np.broadcast_to(np.asarray(start, F32), (A.shape[0], B.shape[1])).copy()
    for s in range(D):
        acc = fma32(A[:, s:s + 1], B[s][None, :], acc)
    return acc


def emu_rowdot(a, b):
    """lane l of 16: fma over the columns l, l + 16, l + 32, l + 48 from 0; then the butterfly xor 8, 4, 2, 1"""
    part = np.zeros((a.shape[0], 16), F32)
    for j in range(4):
        part = fma32(a[:, 16 * j:16 * j + 16], np.broadcast_to(b, a.shape)[:, 16 * j:16 * j + 16], part)
    lanes = np.arange(16)
    for m in (8, 4, 2, 1):
        part = (part + part[:, lanes ^ m]).astype(F32)
    return part[:, :1]


def _blocked(X, n, R):
    nb = -(-n // R)
    P = np.zeros((nb * R,) + X.shape[1:], F32)
    P[:n] = X
    return P.reshape((nb, R // 64, 64) + X.shape[1:])


def emu_finish(part, plant=None):
    """part [blocks, ...]: the blocks j, j + 4, ... in order from 0 for j = 0 .. 3, then the four sums in order"""
    nb = part.shape[0] - (1 if plant == "finish_last_block" else 0)
    sums = []
    for j in range(4):
        a = np.zeros(part.shape[1:], F32)
        for b in range(j, nb, 4):
            a = (a + part[b]).astype(F32)
        sums.append(a)
    a = sums[0]
    for j in (1, 2, 3):
        a = (a + sums[j]).astype(F32)
    return a


def emu_outer(pairs, n, R, plant=None):
    """sum over rows of dz^T X for the (dz, X) pairs, per block one fma chain: per tile the 64 rows of each pair in turn"""
    blocked = [(_blocked(dz, n, R), _blocked(X, n, R)) for dz, X in pairs]
    nb = blocked[0][0].shape[0]
    acc = np.zeros((nb, D, D), F32)
    for t in range(R // 64):
        for dz, X in blocked:
            for r in range(64):
                acc = fma32(dz[:, t, r, :, None], X[:, t, r, None, :], acc)
    return emu_finish(acc, plant)


def emu_colsum(X, n, R, plant=None):
    """thread of row group g: its rows 4 g .. 4 g + 3 of every tile in order; then the 16 groups in order from 0; the finish"""
    B = _blocked(X, n, R)
    nb, tiles = B.shape[:2]
    B = B.reshape(nb, tiles, 16, 4, D)
    acc = np.zeros((nb, 16, D), F32)
    for t in range(tiles - (1 if plant == "bias_last_tile" else 0)):
        for i in range(4):
            acc = (acc + B[:, t, :, i]).astype(F32)
    a = np.zeros((nb, D), F32)
    for g in range(16):
        a = (a + acc[:, g]).astype(F32)
    return emu_finish(a)


def emulate(ops, g, plant=None):
    """fp32 numpy of the plan in include/mmrec_hip.h -> every output of both calls; `plant`: one of the errors the checker must see"""
    V, T, C = ops["V"], ops["T"], ops["C"]
    Wq, Wv, Wt, q = ops["Wq"], ops["Wv"], ops["Wt"], ops["q"][None, :]
    n = V.shape[0]
    R = Z.rows_per_block(n)
    one, three = F32(1.0), F32(3.0)
    hV, hT = emu_tanh(emu_chain(V, Wq.T, ops["bq"][None, :])), emu_tanh(emu_chain(T, Wq.T, ops["bq"][None, :]))
    sV, sT = emu_rowdot(hV, q), emu_rowdot(hT, q)
    mx = np.maximum(sV, sT)
    eV, eT = _exp32(sV - mx), _exp32(sT - mx)
    den = (eV + eT).astype(F32)
    aV, aT = (eV / den).astype(F32), (eT / den).astype(F32)
    pV = emu_sigmoid(emu_chain(C, Wv.T, ops["bv"][None, :]))
    pT = emu_sigmoid(emu_chain(C, Wt.T, ops["bt"][None, :]))
    m = fma32(aT, T, (aV * V).astype(F32))
    xV, xT = (V - m).astype(F32), (T - m).astype(F32)
    side = (fma32(pT, xT, fma32(pV, xV, m)) / three).astype(F32)
    out = {"side": side, "out": (C + side).astype(F32)}
    zero = np.zeros((n, D), F32)
    gs, go = (zero if t is None else t for t in g)
    G3 = ((gs + go).astype(F32) / three).astype(F32)
    dm = (G3 * ((one - pV).astype(F32) - pT).astype(F32)).astype(F32)
    dsV = ((aV * aT).astype(F32) * emu_rowdot(dm, (V - T).astype(F32))).astype(F32)
    dsT = dsV if plant == "dsT_sign" else -dsV
    slope = (lambda h: (one - np.abs(h)).astype(F32)) if plant == "tanh_1mh" else (lambda h: fma32(-h, h, one))
    dzV = ((dsV * q).astype(F32) * slope(hV)).astype(F32)
    dzT = ((dsT * q).astype(F32) * slope(hT)).astype(F32)
    duV = ((G3 * xV).astype(F32) * (pV * (one - pV).astype(F32)).astype(F32)).astype(F32)
    duT = ((G3 * xT).astype(F32) * (pT * (one - pT).astype(F32)).astype(F32)).astype(F32)
    out["dV"] = emu_chain(dzV, Wq, fma32(aV, dm, (G3 * pV).astype(F32)))
    out["dT"] = emu_chain(dzT, Wq, (G3 * pT).astype(F32) if plant == "no_aT_dm" else fma32(aT, dm, (G3 * pT).astype(F32)))
    out["dC"] = emu_chain(duT, Wt, emu_chain(duV, Wv, go))
    out["dWq"] = emu_outer([(dzV, V), (dzT, T)], n, R)
    out["dWv"] = emu_outer([(duV, C)], n, R, plant)
    out["dWt"] = emu_outer([(duT, C)], n, R)
    out["dbq"] = emu_colsum((dzV + dzT).astype(F32), n, R, plant)
    out["dbv"], out["dbt"] = emu_colsum(duV, n, R), emu_colsum(duT, n, R)
    out["dq"] = emu_colsum(fma32(dsT, hT, (dsV * hV).astype(F32)), n, R)
    return out


EMULATED = (1, 2, 3, 4, 6, 9, 11, 12, 13, 20, 27, 5)                  # every small row count and kind, then the 157-block case


@pytest.mark.parametrize("k", EMULATED)
def test_the_emulated_plan_passes_the_checker(k):
    c = Z.case(k)
    assert c.n
    worst = Z.check(c.ops, c.g, emulate(c.ops, c.g), Z.name_of(c))
    print("%s emulated: worst err / bound %s" % (Z.name_of(c), " ".join("%s %.3f" % kv for kv in sorted(worst.items()))))
    assert set(worst) == {"out", "dx", "dw", "db"} and (max(worst.values()) > 0.0 or c.n <= 2)   # (case 1 is one row of zeros)


PLANTS = {"no_aT_dm": "dT", "dsT_sign": "dT", "bias_last_tile": "dbq", "finish_last_block": "dWv", "tanh_1mh": "dV"}


# the two plants that drop rows of a sum are looked for where the dropped rows are not a single row of the smallest scale: the
# 157-block case (its last block has 43 rows, its blocks two tiles) and case 27
PLANTED = [(p, k) for p in sorted(PLANTS) for k in ((5, 27) if p == "finish_last_block" else (5, 20, 6, 27) if p == "bias_last_tile"
                                                    else (20, 6, 27))]


@pytest.mark.parametrize("plant,k", PLANTED)
def test_planted_errors_do_not_pass(k, plant):
    """the aT dm term of dT dropped; dsT with the sign of dsV; a bias gradient that skips a block's last tile; a finish that
    leaves the last block out; tanh' taken as 1 - |h|"""
    c = Z.case(k)
    assert c.n > 64 and c.kind in ("mixed", "zeros", "equal") and not c.all_equal
    rng = np.random.default_rng(k)
    g = [t if t is not None else rng.standard_normal((c.n, D)).astype(F32) for t in c.g]
    good = Z.check(c.ops, g, emulate(c.ops, g), "clean")
    assert max(good.values()) <= 1.0
    bad = emulate(c.ops, g, plant)
    with pytest.raises(AssertionError, match="beyond the bound"):
        Z.check(c.ops, g, {PLANTS[plant]: bad[PLANTS[plant]]}, plant)
    if plant == "dsT_sign":                                           # ... and the attention's own parameters see it too
        for name in ("dWq", "dbq", "dq"):
            with pytest.raises(AssertionError, match="beyond the bound"):
                Z.check(c.ops, g, {name: bad[name]}, plant)
