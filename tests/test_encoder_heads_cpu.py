"""No GPU: the encoder heads' exports, argument checks and plan (csrc/encoder_heads.hip); `encoder_heads_torch` of spmm(graph, x)
IS the end of MVGAE's GCN.forward (float64, supplied masks: the reassociation A (x W) = (A x) W and the operand stacking change
nothing); hip_ops.encoder_heads on anything the kernels do not serve is `encoder_heads_torch`; and the checker of
tests/test_encoder_heads_fuzz_gpu.py held honest: an fp32 numpy emulation of the kernels' plan as include/mmrec_hip.h states it
passes it on the fuzz's own cases, five planted errors do not; the fuzz's kink and clamp conditions hold on its whole case list."""
import os

import numpy as np
import pytest
import torch

import tests.test_encoder_heads_fuzz_gpu as Z
from mmrec_amd import _lib
from tests.test_hyper_cpu import fma32, lib  # noqa: F401  (fixture)
from tests.test_modal_fusion_cpu import emu_chain, emu_colsum, emu_outer

EXPORTS = ("mmrec_encoder_heads_rows_per_block", "mmrec_encoder_heads_workspace_bytes", "mmrec_encoder_heads_fwd_f32",
           "mmrec_encoder_heads_bwd_f32")
BAD, UNSUPPORTED = 10001, 10002
F32 = np.float32
D = 64


def test_exports_in_header_signatures_and_library(lib):  # noqa: F811
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mmrec_hip.h")).read()
    for name in EXPORTS:
        assert name in _lib.SIGNATURES and name in src and hasattr(lib, name), name
    assert "#define MMREC_ABI_VERSION 16" in src and lib.mmrec_abi_version() == 16 and _lib.ABI_VERSION == 16   # additive
    from mmrec_amd.build import SOURCES
    assert "encoder_heads.hip" in SOURCES


def test_entry_points_refuse_bad_arguments_before_touching_memory(lib):  # noqa: F811
    """every call below would fault if a pointer were followed or a kernel launched: this machine has no device"""
    fw, bw = lib.mmrec_encoder_heads_fwd_f32, lib.mmrec_encoder_heads_bwd_f32
    one = 1                                                                # a non-NULL pointer that must never be followed
    for d in (0, 32, 63, 65, 128):                                         # d is 64, checked first
        assert fw(*[None] * 9, 5, d, 2, 0.01, None, None) == UNSUPPORTED, d
        assert bw(*[None] * 10, 5, d, 2, 0.01, *[None] * 10) == UNSUPPORTED, d
        assert fw(*[None] * 9, -1, d, 2, 0.01, None, None) == UNSUPPORTED, d
    for H in (-1, 0, 5, 64):                                               # one to four heads
        assert fw(*[one] * 9, 5, 64, H, 0.01, one, None) == UNSUPPORTED, H
        assert bw(*[one] * 10, 5, 64, H, 0.01, *[one] * 9, None) == UNSUPPORTED, H
    assert fw(*[one] * 9, (1 << 30) + 1, 64, 2, 0.01, one, None) == UNSUPPORTED
    assert bw(*[one] * 10, (1 << 30) + 1, 64, 2, 0.01, *[one] * 9, None) == UNSUPPORTED
    assert fw(*[one] * 9, -1, 64, 2, 0.01, one, None) == BAD               # a negative size
    assert bw(*[one] * 10, -1, 64, 2, 0.01, *[one] * 9, None) == BAD
    assert fw(*[None] * 9, 0, 64, 2, 0.01, None, None) == 0                # no rows: nothing to do, before the NULL checks
    assert bw(*[None] * 10, 0, 64, 2, 0.01, *[None] * 10) == 0
    for hole in range(8):                                                  # a NULL operand (scale, the ninth, may be NULL)
        ptrs = [one] * 8
        ptrs[hole] = None
        assert fw(*ptrs, None, 5, 64, 2, 0.01, one, None) == BAD, hole
        assert bw(*ptrs, None, one, 5, 64, 2, 0.01, *[one] * 9, None) == BAD, hole
    assert fw(*[one] * 9, 5, 64, 2, 0.01, None, None) == BAD               # a NULL forward output
    assert bw(*[one] * 9, None, 5, 64, 2, 0.01, *[one] * 9, None) == BAD   # a NULL g
    for hole in range(2, 8):                                               # any weight gradient without a workspace
        outs = [None] * 8
        outs[hole] = one
        assert bw(*[one] * 10, 5, 64, 2, 0.01, *outs, None, None) == BAD, hole
    assert bw(*[one] * 10, 5, 64, 2, 0.01, *[None] * 8, None, None) == 0   # nothing wanted: nothing to do


def test_plan_and_workspace(lib):  # noqa: F811
    """the plan is a function of the row count alone: a multiple of 64 rows per block, never more than 256 blocks"""
    rpb, wsb = lib.mmrec_encoder_heads_rows_per_block, lib.mmrec_encoder_heads_workspace_bytes
    assert rpb(-1) == 0 and rpb((1 << 30) + 1) == 0 and wsb(-1, 2) == 0 and wsb((1 << 30) + 1, 2) == 0
    assert wsb(100, 0) == 0 and wsb(100, 5) == 0
    from mmrec_amd import hip_ops
    for n in (0, 1, 64, 7050, 16384, 16385, 26495, 54255, 1500000, 1 << 30):
        r = rpb(n)
        assert r >= 64 and r % 64 == 0 and -(-n // r) <= 256, (n, r)
        assert r == 64 * max(1, -(-n // 16384)) == hip_ops.encoder_heads_rows_per_block(n)
        for H in (1, 2, 3, 4):
            assert wsb(n, H) == 4 * 12480 * H * Z.blocks(n) <= 256 * 4 * 12480 * 4
    assert Z.PART == 12480 and rpb(26495) == 128 and Z.blocks(26495) == 207 and Z.n_finish(26495) == 52 + 3
    # the kernels' LDS: three matrices, the biases and three (forward) or six (backward) tiles of 64 x 68 floats
    assert 4 * (9 * 64 * 68 + 192) == 157440 <= 163840 and 4 * (6 * 64 * 68 + 192) == 105216


def _operands(rng, n, H=2, d=D, dtype=torch.float32):
    t = lambda *s: torch.from_numpy(rng.standard_normal(s)).to(dtype)            # noqa: E731
    u = lambda *s: torch.from_numpy(rng.uniform(-0.125, 0.125, s)).to(dtype)     # noqa: E731
    return [t(n, d), t(n, d), u(H, d, d), u(H, d), u(H, d, d), u(H, d), u(H, d, d), u(H, d)]


def test_served_is_about_device_dtype_shape_and_width():
    from mmrec_amd import hip_ops

    class OnDevice(torch.Tensor):                                    # a stand-in that says it lives on the device
        is_cuda = True
    dev = lambda t: t.as_subclass(OnDevice)                          # noqa: E731
    ops = _operands(np.random.default_rng(0), 6)
    scale = torch.ones(2, 6, 64)
    assert not hip_ops.encoder_heads_served(*ops)                    # CPU tensors: never
    assert hip_ops.encoder_heads_served(*[dev(t) for t in ops]) and hip_ops.encoder_heads_served(*[dev(t) for t in ops], dev(scale))
    for H in (1, 3, 4):
        assert hip_ops.encoder_heads_served(*[dev(t) for t in _operands(np.random.default_rng(0), 6, H)])
    assert not hip_ops.encoder_heads_served(*[dev(t) for t in _operands(np.random.default_rng(0), 6, 5)])
    swaps = ((0, torch.zeros(6, 32)), (1, torch.zeros(7, 64)), (1, torch.zeros(6, 64).double()), (0, torch.zeros(6, 128)[:, ::2]),
             (2, torch.zeros(2, 64, 32)), (2, torch.zeros(64, 64)), (4, torch.zeros(2, 64, 64).double()), (3, torch.zeros(1, 64)),
             (5, torch.zeros(64)), (6, torch.zeros(2, 64, 128)[:, :, ::2]), (7, torch.zeros(2, 63)), (0, None), (6, torch.zeros(3, 64, 64)))
    for at, bad in swaps:
        args = [dev(t) for t in ops]
        args[at] = dev(bad) if bad is not None else None
        assert not hip_ops.encoder_heads_served(*args), (at, getattr(bad, "shape", None))
    for bad in (torch.ones(2, 6, 32), torch.ones(1, 6, 64), torch.ones(2, 7, 64), torch.ones(2, 6, 64).double(), scale):
        assert not hip_ops.encoder_heads_served(*[dev(t) for t in ops], bad if bad is scale else dev(bad))
    empty = [dev(torch.zeros(0, 64)) for _ in range(2)] + [dev(t) for t in ops[2:]]
    assert not hip_ops.encoder_heads_served(*empty)
    try:
        hip_ops.ENCODER_HEADS = False
        assert not hip_ops.encoder_heads_served(*[dev(t) for t in ops])
    finally:
        hip_ops.ENCODER_HEADS = True


def test_everything_unserved_runs_the_torch_composition(monkeypatch):
    """CPU tensors, width 32 and a non-contiguous operand all run `encoder_heads_torch` -- and give what it gives"""
    from mmrec_amd import hip_ops
    calls = []
    real = hip_ops.encoder_heads_torch
    monkeypatch.setattr(hip_ops, "encoder_heads_torch", lambda *a: calls.append(tuple(a[0].shape)) or real(*a))
    rng = np.random.default_rng(3)
    ops = _operands(rng, 9)
    scale = torch.from_numpy(((rng.random((2, 9, D)) < 0.9) / 0.9).astype(np.float32))
    narrow = _operands(rng, 9, d=32)
    wide = torch.zeros(9, 128)
    wide[:, ::2] = ops[0]
    strided = [wide[:, ::2]] + ops[1:]
    assert not strided[0].is_contiguous()
    for args in ((*ops, scale), ops, narrow, strided):
        got = hip_ops.encoder_heads(*args)
        assert torch.equal(got, real(*args)) and got.shape == (2, 9, args[0].shape[1])
    assert calls == [(9, 64), (9, 64), (9, 32), (9, 64)]


def _gcn(fused, masks, rng_seed=11):
    """one encoder of MVGAE in float64 on a dense random mean graph, its dropout masks supplied, spmm and linear as plain torch"""
    import mmrec_amd.models.mvgae as mv
    from mmrec_amd import hip_ops
    nu, ni = 7, 12
    n = nu + ni
    torch.manual_seed(rng_seed)
    gcn = mv.GCN(torch.randn(ni, 16), nu, 64, 1, 128, "cpu", fused_heads=fused).double()
    gcn.features, gcn.preference = gcn.features.double(), gcn.preference.double()
    for j in (4, 5):                                                 # nn.Linear-range biases, so that no term is trivially zero
        getattr(gcn, "conv_embed_%d" % j).bias.data.uniform_(-0.125, 0.125)
    rng = np.random.default_rng(rng_seed)
    A = torch.from_numpy((rng.random((n, n)) < 0.3) + np.eye(n)).double()
    A = A / A.sum(dim=1, keepdim=True)
    with pytest.MonkeyPatch.context() as m:
        m.setattr(hip_ops, "spmm", lambda g, X: g @ X)
        m.setattr(hip_ops, "linear", lambda X, W, b=None: torch.nn.functional.linear(X, W, b))
        todo = list(masks)
        m.setattr(mv.F, "dropout", lambda x, p=0.5, training=True, inplace=False: x * todo.pop(0) / (1.0 - p) if training else x)
        gcn.train()
        mu, logvar = gcn(A)
        assert not todo
    gm, gl = (torch.from_numpy(np.random.default_rng(5 + i).standard_normal((n, 64))) for i in range(2))
    ((mu * gm).sum() + (logvar * gl).sum()).backward()
    return mu.detach(), logvar.detach(), {k: p.grad for k, p in gcn.named_parameters() if p.grad is not None}


def test_the_op_is_the_end_of_gcn_forward_in_float64():
    """key off (the four lines of GCN.forward) against key on (one spmm, the stacked operands, `encoder_heads_torch`), float64,
    the same three masks: outputs and every gradient to 1e-12 relative"""
    rng = np.random.default_rng(2)
    masks = [torch.from_numpy((rng.random((19, 64)) < 0.9).astype(np.float64)) for _ in range(3)]
    off, on = _gcn(False, masks), _gcn(True, masks)
    assert set(off[2]) == set(on[2]) and len(on[2]) >= 16
    assert {"conv_embed_4.weight", "conv_embed_5.bias", "g_layer4.weight", "g_layer5.bias", "linear_layer4.weight",
            "linear_layer5.bias", "MLP.weight", "conv_embed_1.weight"} <= set(on[2])
    for a, b in list(zip(off[:2], on[:2])) + [(off[2][k], on[2][k]) for k in off[2]]:
        assert float((a - b).abs().max()) <= 1e-12 * float(a.abs().max()) and float(a.abs().max()) > 0


def test_the_torch_composition_is_the_fuzz_reference():
    """`encoder_heads_torch` in float64 == the float64 numpy that the fuzz compares the kernels with, outputs and gradients"""
    from mmrec_amd import hip_ops
    c = Z.case(34)
    assert c.n == 129 and c.H == 2 and c.scale is not None and not c.g_zero
    ref = Z.bounds(c.ops, c.scale, c.g)
    ops = [torch.from_numpy(c.ops[k]).double().requires_grad_() for k in Z.OPERANDS]
    out = hip_ops.encoder_heads_torch(*ops, torch.from_numpy(c.scale).double(), float(np.float32(Z.SLOPE)))
    (out * torch.from_numpy(c.g).double()).sum().backward()
    for name, got in [("out", out.detach())] + [("d" + k, t.grad) for k, t in zip(Z.OPERANDS, ops)]:
        r = ref[name][0]
        assert float(np.abs(got.numpy() - r).max()) <= 1e-11 * float(np.abs(r).max()), name


def test_the_yaml_names_the_key_in_a_comment_only():
    import yaml
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "mmrec_amd", "configs", "model", "MVGAE.yaml")
    text = open(path).read()
    assert "# fused_heads: True" in text and "fused_heads" not in yaml.safe_load(text)


# ------------------------------------------------------------------------------------------------ the fuzz's checker
def emu_rowdot(a, b):
    """lane l of 16: fma over the columns 4 l, 4 l + 1, 4 l + 2, 4 l + 3 from 0; then the butterfly xor 8, 4, 2, 1"""
    part = np.zeros((a.shape[0], 16), F32)
    for j in range(4):
        part = fma32(a[:, j::4], b[:, j::4], part)
    lanes = np.arange(16)
    for m in (8, 4, 2, 1):
        part = (part + part[:, lanes ^ m]).astype(F32)
    return part[:, :1]


def emulate(ops, scale, g, plant=None):
    """fp32 numpy of the plan in include/mmrec_hip.h -> every output of both calls; `plant`: one of the errors the checker must see"""
    AX, X = ops["AX"], ops["X"]
    n, H = AX.shape[0], ops["W"].shape[0]
    R = Z.rows_per_block(n)
    slope, eps, one = F32(Z.SLOPE), F32(1e-12), F32(1.0)
    if plant == "no_scale":
        scale = None
    leaky = lambda z: np.where(z > 0, z, (slope * z).astype(F32)).astype(F32)     # noqa: E731
    out = {k: [] for k in ("out", "dW", "db", "dG", "dbg", "dL", "dbl")}
    dAX, dX = np.zeros((n, D), F32), np.zeros((n, D), F32)
    for h in range(H):
        a = emu_chain(AX, ops["W"][h], ops["b"][h][None, :])
        raw = np.sqrt(emu_rowdot(a, a)).astype(F32)
        nrm = np.maximum(raw, eps)
        u = (a / nrm).astype(F32)
        d = u if scale is None else (u * scale[h]).astype(F32)
        hh = leaky(d)
        p = emu_chain(X, ops["L"][h].T, ops["bl"][h][None, :])
        out["out"].append((emu_chain(hh, ops["G"][h].T, ops["bg"][h][None, :]) + leaky(p)).astype(F32))
        dhh = emu_chain(g[h], ops["G"][h], np.zeros((1, D), F32))
        du = (dhh * np.where((d >= 0) if plant == "slope_at_0" else (d > 0), one, slope)).astype(F32)
        if scale is not None:
            du = (du * scale[h]).astype(F32)
        dot = emu_rowdot(u, du)
        live = (raw < eps) if plant == "clamp_branch" else (raw >= eps)
        da = (np.where(live, fma32(-u, dot, du), du) / nrm).astype(F32)
        dp = (g[h] * np.where(p > 0, one, slope)).astype(F32)
        dAX, dX = emu_chain(da, ops["W"][h].T, dAX), emu_chain(dp, ops["L"][h], dX)
        out["dW"].append(emu_outer([(AX, da)], n, R))
        out["dG"].append(emu_outer([(g[h], hh)], n, R))
        out["dL"].append(emu_outer([(dp, X)], n, R))
        out["db"].append(emu_colsum(da, n, R))
        out["dbg"].append(emu_colsum(g[h], n, R))
        out["dbl"].append(emu_colsum(dp, n, R))
    out = {k: np.stack(v) for k, v in out.items()}
    out["dAX"], out["dX"] = dAX, dX
    if plant == "swapped_heads":
        out["out"] = out["out"][::-1].copy()
    return out


EMULATED = (1, 2, 3, 4, 6, 8, 9, 11, 12, 13, 20, 27, 5)               # every small row count and kind, then the 157-block case


@pytest.mark.parametrize("k", EMULATED)
def test_the_emulated_plan_passes_the_checker(k):
    c = Z.case(k)
    assert c.n and not c.unsupported
    worst = Z.check(c.ops, c.scale, c.g, emulate(c.ops, c.scale, c.g), Z.name_of(c))
    print("%s emulated: worst err / bound %s" % (Z.name_of(c), " ".join("%s %.3f" % kv for kv in sorted(worst.items()))))
    assert set(worst) == {"out", "dx", "dw", "db"} and max(worst.values()) > 0.0


def _with_g(c):
    return c.g if not c.g_zero else np.random.default_rng(c.k).standard_normal(c.g.shape).astype(F32)


def test_a_slip_of_64_ulps_in_one_output_does_not_pass():
    """the entry of `out` whose bound is the smallest in units of its last place, moved by 64 of them"""
    c = Z.case(25)
    assert c.n == 64 and c.H == 2 and c.kind == "mixed"
    ref, e = Z.bounds(c.ops, c.scale, c.g)["out"]
    good = emulate(c.ops, c.scale, c.g)["out"]
    ulp = np.spacing(np.abs(good)).astype(np.float64)
    at = np.unravel_index(np.argmax(ulp / e), ref.shape)
    assert 64 * ulp[at] > 1.5 * e[at]                                  # ... is beyond the bound wherever in it the clean value lies
    assert Z.check(c.ops, c.scale, c.g, {"out": good}, "clean")["out"] <= 0.5
    bad = good.copy()
    bad[at] = good[at] + F32(64) * np.spacing(good[at])
    with pytest.raises(AssertionError, match="beyond the bound"):
        Z.check(c.ops, c.scale, c.g, {"out": bad}, "ulp")


# swapped heads: H >= 2; a missing scale: scale given; the slope at 0: rows with u = 0 exactly (zero_b0); the clamp: rows below it
PLANTS = {"swapped_heads": ("out", (25, 17, 34)), "no_scale": ("out", (25, 17, 34)), "slope_at_0": ("dAX", (11, 26, 31)),
          "clamp_branch": ("dAX", (3, 13, 18))}
PLANTED = [(p, k) for p in sorted(PLANTS) for k in PLANTS[p][1]]


@pytest.mark.parametrize("plant,k", PLANTED)
def test_planted_errors_do_not_pass(k, plant):
    """the two heads' outputs swapped; the dropout scale left out; leaky' taken as 1 at exactly 0; the clamp's branches swapped
    (seen in the rows above the constant: in a row with ||a|| = 1e-14 the two branches differ by |u|^2 = 1e-4 of the gradient)"""
    c = Z.case(k)
    g = _with_g(c)
    assert c.n > 1 and not c.unsupported
    if plant in ("swapped_heads", "no_scale"):
        assert c.H >= 2 and c.scale is not None
    if plant == "slope_at_0":
        assert c.kind == "zero_b0" and c.below.any()
    if plant == "clamp_branch":
        assert c.kind == "tiny" and c.below.any()
    good = Z.check(c.ops, c.scale, g, emulate(c.ops, c.scale, g), "clean")
    assert max(good.values()) <= 1.0
    bad = emulate(c.ops, c.scale, g, plant)
    name = PLANTS[plant][0]
    with pytest.raises(AssertionError, match="beyond the bound"):
        Z.check(c.ops, c.scale, g, {name: bad[name]}, plant)


def test_the_kink_and_clamp_conditions_hold_on_the_whole_case_list():
    """on the float64 reference alone.  Kink: the entries of d and p whose sign the bound cannot decide (their gradient bound is
    widened, they are not excluded) are at most 2e-4 of all entries.  Clamp: no unplanted row has ||a|| within its bound of
    1e-12; the planted rows are decades away on either side."""
    und, total = {"d": 0, "p": 0}, 0
    for k in range(Z.CASES - 1):
        c = Z.case(k)
        if not c.n:
            continue
        info = {}
        Z.bounds(c.ops, c.scale, c.g, info=info)
        for h in range(c.H):
            raw, e = (t[:, 0] for t in info["raw"][h])
            assert (np.abs(raw - Z.EPS) > e).all(), (k, h, "a row's norm is within its bound of the clamp")
            free = ~c.planted
            assert (raw[free] > 1e4 * Z.EPS).all(), (k, h)
            assert (raw[c.below] < 0.1 * Z.EPS).all() and (raw[c.planted & ~c.below] > 1e3 * Z.EPS).all(), (k, h)
            if c.kind == "tiny":
                assert (raw[c.below] > 1e-15).all() and (raw[c.below] < 5e-14).all()
            und["d"] += int(info["und_d"][h].sum())
            und["p"] += int(info["und_p"][h].sum())
            total += c.n * D
    print("undecided signs: d %d, p %d of %d entries each: %.2e, %.2e" % (und["d"], und["p"], total, und["d"] / total, und["p"] / total))
    assert total > 2e6 and (und["d"] + und["p"]) <= 2e-4 * 2 * total
    assert und["d"] <= 2e-4 * total and und["p"] <= 2e-4 * total
