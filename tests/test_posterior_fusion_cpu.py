"""No GPU: the posterior fusion's exports, argument checks and plan (csrc/posterior.hip); hip_ops.posterior_fusion on CPU tensors is
`posterior_fusion_torch` and MVGAE's own product_of_experts / reparametrize / kl_loss chain bit for bit; MVGAE's `fused_posterior`
key absent / False / True on the CPU against the reference's golden; and the checker of tests/test_posterior_fusion_fuzz_gpu.py
held honest: an fp32 numpy emulation of the kernels' plan as include/mmrec_hip.h states it passes it on the fuzz's own cases, three
planted errors do not; E_LOG is measured here."""
import os

import numpy as np
import pytest
import torch

import tests.test_models_gpu as G
import tests.test_posterior_fusion_fuzz_gpu as Z
from mmrec_amd import _lib
from tests._cpu_ops import cpu_ops  # noqa: F401  (fixture)
from tests.test_hyper_cpu import deterministic_torch, fma32, lib  # noqa: F401  (fixtures)

EXPORTS = ("mmrec_posterior_fusion_rows_per_block", "mmrec_posterior_fusion_workspace_bytes", "mmrec_posterior_fusion_fwd_f32",
           "mmrec_posterior_fusion_bwd_f32")
BAD = 10001
F32 = np.float32
D = 64
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MVGAE_EXTRA = {"learning_rate": 1e-3, "beta": 0.1, "n_layers": 2}


def test_exports_in_header_signatures_and_library(lib):  # noqa: F811
    src = open(os.path.join(ROOT, "include", "mmrec_hip.h")).read()
    for name in EXPORTS:
        assert name in _lib.SIGNATURES and name in src and hasattr(lib, name), name
    assert "#define MMREC_ABI_VERSION 16" in src and lib.mmrec_abi_version() == 16 and _lib.ABI_VERSION == 16   # additive
    from mmrec_amd.build import SOURCES
    assert "posterior.hip" in SOURCES


def test_entry_points_refuse_bad_arguments_before_touching_memory(lib):  # noqa: F811
    """every call below would fault if a pointer were followed or a kernel launched: this machine has no device"""
    fw, bw = lib.mmrec_posterior_fusion_fwd_f32, lib.mmrec_posterior_fusion_bwd_f32
    one = 1                                                                # a non-NULL pointer that must never be followed
    good_f = lambda n, d: fw(*[one] * 10, n, d, one, one, one, one, None)  # noqa: E731
    good_b = lambda n, d: bw(*[one] * 12, n, d, *[one] * 6, None)          # noqa: E731
    for d in (0, 32, 63, 65, 128):                                         # d is 64
        assert good_f(5, d) == BAD and good_b(5, d) == BAD, d
        assert fw(*[None] * 10, 0, d, None, None, None, None, None) == BAD, d
    for n in (-1, (1 << 30) + 1, 1 << 40):                                 # n is 1 .. 2^30
        assert good_f(n, 64) == BAD and good_b(n, 64) == BAD, n
    assert fw(*[None] * 10, 0, 64, None, None, None, None, None) == 0      # no rows: nothing to do, before the NULL checks
    assert bw(*[None] * 12, 0, 64, *[None] * 6, None) == 0
    for hole in range(6):                                                  # a NULL input
        ptrs = [one] * 10
        ptrs[hole] = None
        assert fw(*ptrs, 5, 64, one, one, one, one, None) == BAD, hole
        assert bw(*ptrs, one, one, 5, 64, *[one] * 6, None) == BAD, hole
    for given in range(1, 15):                                             # some but not all of the noise pointers
        ptrs = [one] * 6 + [one if given >> i & 1 else None for i in range(4)]
        assert fw(*ptrs, 5, 64, one, one, one, one, None) == BAD, given
        assert bw(*ptrs, one, one, 5, 64, *[one] * 6, None) == BAD, given
    for hole in range(4):                                                  # a NULL Z, score, kl or workspace
        outs = [one] * 4
        outs[hole] = None
        assert fw(*[one] * 10, 5, 64, *outs, None) == BAD, hole
    # every noise pointer NULL is a served form: with nothing wanted the backward has nothing to do and follows no pointer
    assert bw(*[one] * 6, *[None] * 4, None, None, 5, 64, *[None] * 6, None) == 0
    assert bw(*[one] * 12, 5, 64, *[None] * 6, None) == 0


def test_plan_and_workspace(lib):  # noqa: F811
    """the plan is a function of the row count alone: 16 ceil(n / 16,384) rows per block, never more than 1,024 blocks of four
    partial sums"""
    rpb, wsb = lib.mmrec_posterior_fusion_rows_per_block, lib.mmrec_posterior_fusion_workspace_bytes
    assert rpb(-1) == 0 and rpb((1 << 30) + 1) == 0 and wsb(-1) == 0 and wsb((1 << 30) + 1) == 0
    hand = {0: (16, 0), 1: (16, 1), 16: (16, 1), 17: (16, 2), 16384: (16, 1024), 16385: (32, 513), 20011: (32, 626),
            26495: (32, 828), 54255: (64, 848), 1500000: (1472, 1020), 1 << 30: (1048576, 1024)}
    for n, (r, nb) in hand.items():
        assert rpb(n) == r and wsb(n) == 16 * nb, (n, rpb(n), wsb(n))
        assert r % 16 == 0 and nb <= 1024 and Z.blocks(n) == nb
    assert Z.n_additions(26495) == 3 + 4 + 2 + 16 + 13 + 6


def test_served_is_about_device_dtype_shape_and_width():
    from mmrec_amd import hip_ops

    class OnDevice(torch.Tensor):                                    # a stand-in that says it lives on the device
        is_cuda = True
    dev = lambda t: t.as_subclass(OnDevice)                          # noqa: E731
    ops = [torch.zeros(6, 64) for _ in range(6)]
    noise = [torch.zeros(6, 64) for _ in range(4)]
    assert not hip_ops.posterior_fusion_served(*ops) and not hip_ops.posterior_fusion_served(*ops, noise)    # CPU tensors: never
    assert hip_ops.posterior_fusion_served(*[dev(t) for t in ops])
    assert hip_ops.posterior_fusion_served(*[dev(t) for t in ops], [dev(t) for t in noise])
    for at, bad in ((0, torch.zeros(6, 32)), (1, torch.zeros(7, 64)), (2, torch.zeros(6, 64).double()),
                    (3, torch.zeros(6, 128)[:, ::2]), (5, torch.zeros(0, 64)), (4, None)):
        args = [dev(t) for t in ops]
        args[at] = dev(bad) if bad is not None else None
        assert not hip_ops.posterior_fusion_served(*args), (at, getattr(bad, "shape", None))
        if bad is not None:
            ns = [dev(t) for t in noise]
            ns[at % 4] = dev(bad)
            assert not hip_ops.posterior_fusion_served(*[dev(t) for t in ops], ns), at
    assert not hip_ops.posterior_fusion_served(*[dev(torch.zeros(0, 64)) for _ in range(6)])
    assert not hip_ops.posterior_fusion_served(*[dev(t) for t in ops], [dev(t) for t in noise[:3]])
    assert not hip_ops.posterior_fusion_served(*[dev(t) for t in ops[:5]], ops[5])          # one operand on the host
    try:
        hip_ops.POSTERIOR_FUSION = False
        assert not hip_ops.posterior_fusion_served(*[dev(t) for t in ops])
    finally:
        hip_ops.POSTERIOR_FUSION = True


class _Holder:
    """what MVGAE.reparametrize reads of its model"""
    training = True


def _model_chain(ops, noise, monkeypatch):
    """models/mvgae.py with the `fused_posterior` key off: forward's and calculate_loss's own lines"""
    import mmrec_amd.models.mvgae as mv
    v_mu, v_logvar, t_mu, t_logvar, c_mu, c_logvar = ops
    h = _Holder()
    draws = list(noise)
    monkeypatch.setattr(mv.torch, "randn_like", lambda x, *a, **k: draws.pop(0))
    pd_mu, pd_logvar = mv.product_of_experts(torch.stack([v_mu, t_mu]), torch.stack([v_logvar, t_logvar]))
    pd_mu, pd_logvar = mv.product_of_experts(torch.stack([pd_mu, c_mu]), torch.stack([pd_logvar, c_logvar]))
    pairs = ((pd_mu, pd_logvar), (v_mu, v_logvar), (t_mu, t_logvar), (c_mu, c_logvar))
    zs = [mv.MVGAE.reparametrize(h, m, l) for m, l in pairs]
    kls = [mv.MVGAE.kl_loss(h, m, l) for m, l in pairs]
    assert not draws
    return torch.stack(zs), torch.stack(kls), torch.sigmoid(pd_mu).detach()


def test_cpu_tensors_take_the_models_own_chain_bit_for_bit(cpu_ops, deterministic_torch, monkeypatch):  # noqa: F811
    """hip_ops.posterior_fusion on CPU tensors == posterior_fusion_torch == the model's lines, outputs and all six gradients; and
    it IS the formulas of the fuzz file, in float64"""
    from mmrec_amd import hip_ops
    rng = np.random.default_rng(8)
    n = 37
    t = lambda lo, hi: torch.from_numpy(rng.uniform(lo, hi, (n, D)).astype(F32))          # noqa: E731
    tables = [t(-2, 2), t(-12, 12), t(-2, 2), t(-12, 12), t(-2, 2), t(-12, 12)]
    noise = [torch.from_numpy(rng.standard_normal((n, D)).astype(F32)) for _ in range(4)]
    gZ = torch.from_numpy(rng.standard_normal((4, n, D)).astype(F32))
    gkl = torch.from_numpy(rng.uniform(0.5, 2.0, 4).astype(F32))
    runs = []
    for how in ("fusion", "torch", "model"):
        ops = [x.clone().requires_grad_() for x in tables]
        if how == "model":
            with monkeypatch.context() as m:
                outs = _model_chain(ops, noise, m)
        else:
            assert not hip_ops.posterior_fusion_served(*ops, noise)
            outs = (hip_ops.posterior_fusion if how == "fusion" else hip_ops.posterior_fusion_torch)(*ops, noise)
        assert not outs[2].requires_grad
        ((outs[0] * gZ).sum() + (outs[1] * gkl).sum()).backward()
        runs.append([o.detach() for o in outs] + [x.grad for x in ops])
    for a, b, c in zip(*runs):
        assert a is not None and torch.equal(a, b) and torch.equal(a, c)
    assert all(float(x.abs().max()) > 0 for x in runs[0])
    ops = dict(zip(Z.INPUTS, [x.numpy() for x in tables]))
    ref = Z.bounds(ops, dict(zip(Z.NOISE, [x.numpy() for x in noise])), gZ.numpy(), gkl.numpy(), 16, 3)
    got = dict(zip(("Z", "kl", "score") + Z.GRADS, runs[0]))
    got.update({"Z_" + k: got["Z"][i] for i, k in enumerate("pvtc")})
    del got["Z"]
    for name, g in got.items():
        r = ref[name][0]
        assert float(np.abs(g.double().numpy().reshape(r.shape) - r).max()) <= 1e-4 * float(np.abs(r).max()), name
    # evaluation mode: no noise, z = mu
    Z0, _, _ = hip_ops.posterior_fusion(*tables)
    assert all(torch.equal(Z0[i + 1], tables[2 * i]) for i in range(3))


def _step(tmp_path, golden, g, extra, monkeypatch):
    import mmrec_amd.models.mvgae as mv
    config, _, valid_data, model = G.build(tmp_path, golden, "MVGAE", dict(MVGAE_EXTRA, **extra))
    assert model.fused_posterior is bool(extra.get("fused_posterior", False)) and model.graph_capturable is False
    params = dict(model.named_parameters())
    assert set(params) == {k[2:] for k in g if k.startswith("p_")}
    for name, p in params.items():
        G.load(p, g["p_" + name])
    dev = model.device
    masks = [torch.as_tensor(g["mask_%d" % j].astype(np.float32)).to(dev) for j in range(12)]
    noises = [torch.as_tensor(g["noise_%d" % j]).to(dev) for j in range(4)]
    with monkeypatch.context() as m:                                 # test_mvgae_model's replay of the 12 masks and 4 noises
        m.setattr(mv.F, "dropout", lambda x, p=0.5, training=True, inplace=False: x * masks.pop(0) / (1.0 - p) if training else x)
        m.setattr(mv.torch, "randn_like", lambda x, *a, **k: noises.pop(0))
        model.train()
        loss = model.calculate_loss(torch.as_tensor(g["batch1"]).to(dev))
        loss.backward()
    assert not masks and not noises                                  # all are consumed
    G.close(loss, g["loss1"], rtol=2e-5)
    G.close(model.result_embed, g["result"], rtol=1e-4, atol=2e-6)
    assert not model.result_embed.requires_grad
    grads = {k[2:] for k in g if k.startswith("g_")}
    assert {n for n, p in params.items() if p.grad is not None} == grads       # who gets no gradient is unchanged
    for name in grads:
        G.close(params[name].grad, g["g_" + name], rtol=2e-3, atol=2e-5)
    model.eval()
    users, mask = next(iter(valid_data))
    for _ in valid_data:
        pass
    G.close(model.full_sort_predict([users, mask]), g["scores_first_batch"], rtol=1e-4, atol=2e-6)
    return model, loss.detach(), {n: params[n].grad.detach().clone() for n in grads}


def test_mvgae_fused_posterior_key_on_the_cpu(tmp_path, golden, cpu_ops, deterministic_torch, monkeypatch):  # noqa: F811
    """absent, False, True: each meets the golden at test_mvgae_model's tolerances; absent and False are the same path (equal
    bits); only True asks hip_ops.posterior_fusion, once, and never the composition's own product_of_experts / kl_loss"""
    from mmrec_amd import hip_ops
    import mmrec_amd.models.mvgae as mv
    monkeypatch.setattr(G, "USE_GPU", False)
    g = G._golden("mvgae")
    asked = []
    monkeypatch.setattr(hip_ops, "posterior_fusion",
                        lambda *a, _real=hip_ops.posterior_fusion: asked.append((tuple(a[0].shape), len(a[6]))) or _real(*a))
    _, loss0, g0 = _step(tmp_path / "absent", golden, g, {}, monkeypatch)
    _, loss1, g1 = _step(tmp_path / "off", golden, g, {"fused_posterior": False}, monkeypatch)
    assert not asked                                                  # absent or False: today's path, untouched
    assert torch.equal(loss0, loss1) and all(torch.equal(g0[n], g1[n]) for n in g0)
    with monkeypatch.context() as m:
        m.setattr(mv, "product_of_experts", lambda *a, **k: pytest.fail("the composition ran with the key on"))
        m.setattr(mv.MVGAE, "kl_loss", lambda *a, **k: pytest.fail("the composition ran with the key on"))
        model, loss2, g2 = _step(tmp_path / "on", golden, g, {"fused_posterior": True}, monkeypatch)
    assert asked == [((model.n_users + model.n_items, 64), 4)]
    assert set(g0) == set(g2) and len(g0) >= 12
    assert abs(float(loss2) - float(loss0)) <= 2e-6 * abs(float(loss0))            # the batched term: the same sum


def test_the_yaml_names_the_key_in_a_comment_only():
    import yaml
    text = open(os.path.join(ROOT, "mmrec_amd", "configs", "model", "MVGAE.yaml")).read()
    assert "# fused_posterior: True" in text and "fused_posterior" not in yaml.safe_load(text)


# ------------------------------------------------------------------------------------------------ the fuzz's checker
ONE = F32(1.0)


def _exp32(x):
    return np.exp(np.asarray(x, F32)).astype(F32)


def emu_expert(l):
    E = _exp32(l)
    return E, (ONE / (E + F32(1e-8)).astype(F32)).astype(F32)


def emu_poe(mu_a, xa, mu_b, xb):
    var = (ONE / (xa[1] + xb[1]).astype(F32)).astype(F32)
    m = (fma32(mu_b, xb[1], (mu_a * xa[1]).astype(F32)) * var).astype(F32)
    return var, m, np.log(var).astype(F32)


def emu_sigmoid(z):
    q = _exp32(-np.abs(z))
    return (np.where(z >= 0, ONE, q) / (ONE + q)).astype(F32)


def _butterfly(part, masks):
    lanes = np.arange(part.shape[-1])
    for m in masks:
        part = (part + part[..., lanes ^ m]).astype(F32)
    return part[..., 0]


def emu_kl(term, n, R):
    """term [n, 64] -> the sum, in the plan's order: a lane's four columns, the row's butterfly, the group's passes, the 16 groups,
    the finish's lanes (blocks j, j + 64, ...) and its butterfly"""
    nb = -(-n // R)
    P = np.zeros((nb * R, D), F32)
    P[:n] = term
    P = P.reshape(nb, R // 16, 16, 16, 4)                                 # block, pass, group, lane, column
    lane = P[..., 0]
    for j in (1, 2, 3):
        lane = (lane + P[..., j]).astype(F32)
    row = _butterfly(lane, (8, 4, 2, 1))                                  # [block, pass, group]
    acc = np.zeros((nb, 16), F32)
    for p in range(R // 16):
        acc = (acc + row[:, p]).astype(F32)
    part = np.zeros(nb, F32)
    for g in range(16):
        part = (part + acc[:, g]).astype(F32)
    lanes = np.zeros(64, F32)
    for j in range(64):
        for b in range(j, nb, 64):
            lanes[j] = F32(lanes[j] + part[b])
    return _butterfly(lanes[None, :], (32, 16, 8, 4, 2, 1))[0]


def emulate(ops, noise, gZ, g_kl, plant=None):
    """fp32 numpy of the plan in include/mmrec_hip.h -> every output of both calls; `plant`: one of the errors the checker must see"""
    n = ops["mu_v"].shape[0]
    R = Z.rows_per_block(n)
    inv_n = ONE / F32(n)
    x = {m: emu_expert(ops["lv_" + m]) for m in "vtc"}
    s1 = emu_poe(ops["mu_v"], x["v"], ops["mu_t"], x["t"])
    x1 = emu_expert(np.minimum(s1[2], F32(10.0)) if plant == "l1_clamped" else s1[2])
    s2 = emu_poe(s1[1], x1, ops["mu_c"], x["c"])
    pairs = dict(p=(s2[1], s2[2]), v=(ops["mu_v"], ops["lv_v"]), t=(ops["mu_t"], ops["lv_t"]), c=(ops["mu_c"], ops["lv_c"]))
    out, kl, up = {}, np.zeros(4, F32), {}
    zero = np.zeros((n, D), F32)
    for i, k in enumerate("pvtc"):
        mu, l = pairs[k]
        lh = np.minimum(l, F32(10.0))
        sd, el = _exp32(F32(0.5) * lh), _exp32(lh)
        E = zero if noise is None else noise["E_" + k]
        out["Z_" + k] = mu.copy() if noise is None else fma32((F32(0.1) * E).astype(F32), sd, mu)
        term = (fma32(-mu, mu, (ONE + lh).astype(F32)) - el).astype(F32)
        kl[i] = F32(F32(-0.5) * inv_n) * emu_kl(term, n, R)
        gz = zero if gZ is None else gZ[i]
        ck = F32(0.0) if g_kl is None else F32(g_kl[i] * inv_n)
        gm = fma32(ck, mu, gz)
        h = (F32(F32(0.5) * ck) * (ONE - el).astype(F32)).astype(F32)
        gl = fma32(gz, ((F32(0.05) * E).astype(F32) * sd).astype(F32), -h)
        up[k] = (gm, gl if plant == "clamp_passes" else np.where(l <= F32(10.0), gl, F32(0.0)).astype(F32))
    out["kl"] = kl
    out["score"] = emu_sigmoid(s2[1])

    def poe_bwd(mu_a, xa, s, gm, gl):
        E, T = xa
        var, m, _ = s
        w = (((T * T).astype(F32) * E).astype(F32) * var).astype(F32)
        return ((gm * T).astype(F32) * var).astype(F32), -(w * fma32(gm, (mu_a - m).astype(F32), -gl)).astype(F32)
    gm1, gl1 = poe_bwd(s1[1], x1, s2, *up["p"])
    share = {"c": poe_bwd(ops["mu_c"], x["c"], s2, *up["p"]), "v": poe_bwd(ops["mu_v"], x["v"], s1, gm1, gl1),
             "t": poe_bwd(ops["mu_t"], x["t"], s1, gm1, gl1)}
    for k in "vtc":
        out["d_mu_" + k] = (share[k][0] + up[k][0]).astype(F32)
        out["d_lv_" + k] = (share[k][1] + up[k][1]).astype(F32)
    if plant == "ulp64":                                                  # 64 ulp in one element of one output
        at = np.unravel_index(np.argmax(np.abs(ops["mu_v"])), (n, D))
        out["Z_v"][at] = out["Z_v"][at] * F32(1.0 + 64 * 2.0 ** -23)
    return out


EMULATED = (0, 1, 2, 3, 4, 6, 7, 8, 10, 11, 13, 14, 16, 19, 22, 5)           # every row count, kind and g mask, then the 626-block case


@pytest.mark.parametrize("k", EMULATED)
def test_the_emulated_plan_passes_the_checker(k):
    c = Z.case(k)
    with np.errstate(all="ignore"):
        got = emulate(c.ops, c.noise, c.gZ, c.g_kl)
    worst = Z.check(c.ops, c.noise, c.gZ, c.g_kl, got, Z.name_of(c))
    print("%s emulated: worst err / bound %s" % (Z.name_of(c), " ".join("%s %.3f" % kv for kv in sorted(worst.items()))))
    assert set(worst) == {"Z", "score", "kl", "d_mu", "d_lv"} and max(worst.values()) > 0.0
    if not c.noisy:
        assert all((got["Z_" + m].view(np.int32) == c.ops["mu_" + m].view(np.int32)).all() for m in "vtc")


def test_the_emulation_covers_every_axis():
    cs = [Z.case(k) for k in EMULATED]
    assert {c.n for c in cs} == set(Z.axis_n()) | {Z.BIG} and {c.kind for c in cs} == set(Z.KINDS)
    assert {c.g_mask for c in cs} == {0, 1, 2, 3} and {c.noisy for c in cs} == {True, False}


PLANTS = {"ulp64": ("Z_v",), "clamp_passes": ("d_lv_v", "d_lv_t", "d_lv_c"), "l1_clamped": ("Z_p", "score", "kl")}
PLANTED = [("ulp64", 4), ("ulp64", 40), ("ulp64", 5), ("clamp_passes", 40), ("clamp_passes", 14), ("clamp_passes", 22),
           ("l1_clamped", 40), ("l1_clamped", 8), ("l1_clamped", 5)]


@pytest.mark.parametrize("plant,k", PLANTED)
def test_planted_errors_do_not_pass(k, plant):
    """64 ulp in one element of Z[v]; a clamp gradient passed at lv > 10; l1 clamped before stage 2"""
    c = Z.case(k)
    rng = np.random.default_rng(k)
    assert c.n > 16
    noise = c.noise if c.noise is not None else {key: rng.standard_normal((c.n, D)).astype(F32) for key in Z.NOISE}
    gZ = c.gZ if c.gZ is not None else rng.standard_normal((4, c.n, D)).astype(F32)
    gkl = c.g_kl if c.g_kl is not None else np.array([1.0, -2.0, 0.5, 1.5], F32)
    with np.errstate(all="ignore"):
        clean, bad = emulate(c.ops, noise, gZ, gkl), emulate(c.ops, noise, gZ, gkl, plant)
    good = Z.check(c.ops, noise, gZ, gkl, clean, "clean")
    assert max(good.values()) <= 1.0
    for name in PLANTS[plant]:
        with pytest.raises(AssertionError, match="beyond the bound"):
            Z.check(c.ops, noise, gZ, gkl, {name: bad[name]}, plant)


def test_E_LOG_covers_these_cases():
    """worst error of fp32 log (numpy, on the CPU) against float64 in units of u max(|log x|, 1) over the arguments var1, var2 of
    every case: E_LOG is 4 x that, rounded up, and not more than 8 x"""
    worst = 0.0
    for k in range(Z.CASES):
        _, _, _, _, var1, var2 = Z.forward64(Z.case(k).ops)
        for var in (var1, var2):
            x = var.astype(F32)
            a, b = np.log(x).astype(np.float64), np.log(x.astype(np.float64))
            worst = max(worst, float((np.abs(a - b) / (Z.U * np.maximum(np.abs(b), 1.0))).max(initial=0.0)))
    print("fp32 log against float64, worst error in units of u max(|log x|, 1): %.3f" % worst)
    assert 4.0 * worst <= Z.E_LOG and (Z.E_LOG == 4.0 or Z.E_LOG <= 8.0 * worst), (worst, Z.E_LOG)
