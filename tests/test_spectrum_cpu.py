"""No GPU: the spectrum step's exports, argument checks and plan (csrc/spectrum.hip); hip_ops.spectrum_fusion on CPU tensors is
`spectrum_fusion_torch` and SMORE.spectrum_convolution bit for bit and meets the reference's golden; SMORE's `fused_spectrum` key
absent / False / True on the CPU; and the checker of tests/test_spectrum_fuzz_gpu.py held honest: an fp32 numpy emulation of the
kernels' plan passes it on the fuzz's own cases, five planted errors do not."""
import os

import numpy as np
import pytest
import torch

import tests.test_models_gpu as G
import tests.test_spectrum_fuzz_gpu as Z
from mmrec_amd import _lib
from tests._cpu_ops import cpu_ops  # noqa: F401  (fixture)
from tests.test_hyper_cpu import deterministic_torch, fma32, lib  # noqa: F401  (fixtures)

EXPORTS = ("mmrec_spectrum_rows_per_block", "mmrec_spectrum_workspace_bytes", "mmrec_spectrum_fwd_f32", "mmrec_spectrum_bwd_f32")
BAD, UNSUPPORTED = 10001, 10002
F32 = np.float32
SMORE_EXTRA = {"cl_loss": 0.01, "learning_rate": 1e-3, "n_ui_layers": 3, "image_knn_k": 10, "text_knn_k": 15, "reg_weight": 1e-4,
               "dropout_rate": 0.1}


def _golden():
    return dict(np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "smore.npz")))


def test_exports_in_header_signatures_and_library(lib):  # noqa: F811
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mmrec_hip.h")).read()
    for name in EXPORTS:
        assert name in _lib.SIGNATURES and name in src and hasattr(lib, name), name
    assert "#define MMREC_ABI_VERSION 16" in src and lib.mmrec_abi_version() == 16 and _lib.ABI_VERSION == 16   # additive
    from mmrec_amd.build import SOURCES
    assert "spectrum.hip" in SOURCES


def test_entry_points_refuse_bad_arguments_before_touching_memory(lib):  # noqa: F811
    """every call below would fault if a pointer were followed or a kernel launched: this machine has no device"""
    fw, bw = lib.mmrec_spectrum_fwd_f32, lib.mmrec_spectrum_bwd_f32
    one = 1                                                                # a non-NULL pointer that must never be followed
    for d in (0, 32, 63, 65, 128):                                         # d is 64, checked first
        assert fw(None, None, None, None, None, 5, d, None, None, None, None) == UNSUPPORTED, d
        assert bw(*[None] * 8, 5, d, *[None] * 7) == UNSUPPORTED, d
        assert fw(None, None, None, None, None, -1, d, None, None, None, None) == UNSUPPORTED, d
    assert fw(*[one] * 5, (1 << 30) + 1, 64, one, one, one, None) == UNSUPPORTED
    assert bw(*[one] * 8, (1 << 30) + 1, 64, *[one] * 6, None) == UNSUPPORTED
    assert fw(*[one] * 5, -1, 64, one, one, one, None) == BAD              # a negative size
    assert bw(*[one] * 8, -1, 64, *[one] * 6, None) == BAD
    for hole in range(5):                                                  # a NULL x / y / weight
        ptrs = [one] * 5
        ptrs[hole] = None
        assert fw(*ptrs, 5, 64, one, one, one, None) == BAD, hole
        assert bw(*ptrs, one, one, one, 5, 64, *[one] * 6, None) == BAD, hole
    for hole in range(3):                                                  # a NULL forward output
        outs = [one] * 3
        outs[hole] = None
        assert fw(*[one] * 5, 5, 64, *outs, None) == BAD, hole
    assert bw(*[one] * 8, 5, 64, None, None, one, None, None, None, None) == BAD      # a weight gradient without a workspace
    assert bw(*[one] * 8, 5, 64, None, None, None, None, None, None, None) == 0       # nothing wanted: nothing to do
    assert fw(*[None] * 5, 0, 64, None, None, None, None) == 0             # no rows: nothing to do
    assert bw(*[None] * 8, 0, 64, *[None] * 7) == 0


def test_plan_and_workspace(lib):  # noqa: F811
    """the plan is a function of the row count alone: a multiple of 64 rows per block, never more than 1,024 blocks"""
    assert lib.mmrec_spectrum_rows_per_block(-1) == 0 and lib.mmrec_spectrum_rows_per_block((1 << 30) + 1) == 0
    for n in (0, 1, 64, 7050, 18357, 65536, 65537, 500000, 1 << 20, 1 << 30):
        r = lib.mmrec_spectrum_rows_per_block(n)
        assert r >= 64 and r % 64 == 0 and -(-n // r) <= 1024, (n, r)
        assert (r == 64) == (n <= 65536)
        assert lib.mmrec_spectrum_workspace_bytes(n) == 4 * 198 * Z.blocks(n)
    assert lib.mmrec_spectrum_workspace_bytes(-1) == 0 and lib.mmrec_spectrum_workspace_bytes((1 << 30) + 1) == 0
    assert Z.n_red(7050) == 1 + 6 + 2 + 6 and Z.n_red(500000) == 8 + 6 + 16 + 6


def test_served_is_about_device_dtype_shape_and_width():
    from mmrec_amd import hip_ops

    class OnDevice(torch.Tensor):                                    # a stand-in that says it lives on the device
        is_cuda = True
    dev = lambda t: t.as_subclass(OnDevice)                          # noqa: E731
    x, y, w = torch.zeros(6, 64), torch.zeros(6, 64), torch.zeros(1, 33, 2)
    assert not hip_ops.spectrum_fusion_served(x, y, w, w, w)         # CPU tensors: never
    assert hip_ops.spectrum_fusion_served(dev(x), dev(y), dev(w), dev(w), dev(w))
    for bad in ((torch.zeros(6, 32), torch.zeros(6, 32), w), (x, torch.zeros(7, 64), w), (x.double(), y, w), (x, y, w.double()),
                (torch.zeros(6, 128)[:, ::2], y, w), (x, y, torch.zeros(33, 2)), (x, y, torch.zeros(1, 17, 2)),
                (torch.zeros(0, 64), torch.zeros(0, 64), w), (x, y, torch.zeros(1, 33, 4)[:, :, ::2]), (None, y, w)):
        args = [dev(t) if isinstance(t, torch.Tensor) else t for t in bad]
        assert not hip_ops.spectrum_fusion_served(args[0], args[1], args[2], args[2], args[2]), [getattr(t, "shape", None) for t in bad]
    assert not hip_ops.spectrum_fusion_served(dev(x), dev(y), dev(w), w, dev(w))
    try:
        hip_ops.SPECTRUM = False
        assert not hip_ops.spectrum_fusion_served(dev(x), dev(y), dev(w), dev(w), dev(w))
    finally:
        hip_ops.SPECTRUM = True


class _Holder:
    """what SMORE.spectrum_convolution reads of its model"""
    _dft = None


def test_cpu_tensors_take_todays_inline_composition_bit_for_bit(deterministic_torch):  # noqa: F811
    from mmrec_amd import hip_ops
    from mmrec_amd.models.smore import SMORE
    rng = np.random.default_rng(8)
    t = lambda *s: torch.from_numpy(rng.standard_normal(s).astype(np.float32))     # noqa: E731
    x0, y0, ws0, gs = t(37, 64), t(37, 64), [t(1, 33, 2) for _ in range(3)], [t(37, 64) for _ in range(3)]
    runs = []
    for how in ("fusion", "torch", "model"):
        x, y = x0.clone().requires_grad_(), y0.clone().requires_grad_()
        ws = [w.clone().requires_grad_() for w in ws0]
        if how == "model":
            h = _Holder()
            h.image_complex_weight, h.text_complex_weight, h.fusion_complex_weight = ws
            outs = SMORE.spectrum_convolution(h, x, y)
        else:
            assert not hip_ops.spectrum_fusion_served(x, y, *ws)
            outs = (hip_ops.spectrum_fusion if how == "fusion" else hip_ops.spectrum_fusion_torch)(x, y, *ws)
        sum((o * g).sum() for o, g in zip(outs, gs)).backward()
        runs.append([o.detach() for o in outs] + [x.grad, y.grad] + [w.grad for w in ws])
    for a, b, c in zip(*runs):
        assert torch.equal(a, b) and torch.equal(a, c)
    assert float(runs[0][3].abs().max()) > 0 and float(runs[0][7].abs().max()) > 0
    # ... and it IS the formulas of the fuzz file, in float64
    w = np.concatenate([v.numpy() for v in ws0])
    ref = Z.terms64(x0.numpy(), y0.numpy(), w, [g.numpy() for g in gs])
    for name, got in zip(Z.FWD_NAMES + ("dx", "dy") + Z.DW_NAMES, runs[0]):
        r = ref[name]
        assert float(np.abs(got.double().numpy().reshape(r.shape) - r).max()) <= 1e-4 * float(np.abs(r).max()), name


def test_cpu_fusion_meets_the_reference_golden():
    """the reference's torch.fft results on its own projected tables, at test_smore_model's tolerances"""
    from mmrec_amd import hip_ops
    smo = _golden()
    T = lambda k: torch.as_tensor(smo[k])                            # noqa: E731
    img = T("p_image_embedding.weight") @ T("p_image_trs.weight").T + T("p_image_trs.bias")
    txt = T("p_text_embedding.weight") @ T("p_text_trs.weight").T + T("p_text_trs.bias")
    outs = hip_ops.spectrum_fusion(img, txt, T("p_image_complex_weight"), T("p_text_complex_weight"), T("p_fusion_complex_weight"))
    for got, key in zip(outs, ("image_conv", "text_conv", "fusion_conv")):
        G.close(got, smo[key], rtol=1e-4, atol=2e-6)
    ref = Z.fwd64(img.numpy(), txt.numpy(), np.concatenate([smo["p_%s_complex_weight" % k] for k in ("image", "text", "fusion")]))
    for r, key in zip(ref, ("image_conv", "text_conv", "fusion_conv")):   # ... and so does the fuzz's float64 reference
        G.close(torch.as_tensor(r, dtype=torch.float32), smo[key], rtol=1e-4, atol=2e-6)


def _step(tmp_path, golden, monkeypatch, smo, extra):
    import mmrec_amd.models.smore as smod
    config, _, _, model = G.build(tmp_path, golden, "SMORE", dict(SMORE_EXTRA, **extra))
    assert model.fused_spectrum is bool(extra.get("fused_spectrum", False))
    params = dict(model.named_parameters())
    for name, p in params.items():
        G.load(p, smo["p_" + name])
    masks = [torch.as_tensor(smo["drop_mask_%d" % j].astype(np.float32)).to(model.device) for j in range(3)]
    with monkeypatch.context() as m:
        m.setattr(smod.F, "dropout", lambda x, p=0.5, training=True, inplace=False: x * masks.pop(0) / (1.0 - p))
        model.train()
        loss = model.calculate_loss(torch.as_tensor(smo["batch1"]).to(model.device))
        loss.backward()
    assert not masks
    return model, loss.detach(), {n: p.grad.detach().clone() for n, p in params.items() if p.grad is not None}


def test_smore_fused_spectrum_key_on_the_cpu(tmp_path, golden, cpu_ops, deterministic_torch, monkeypatch):  # noqa: F811
    """absent, False, True: on CPU tensors the key-on path is the same composition, so loss and gradients are bit-equal; only
    True asks hip_ops.spectrum_fusion"""
    from mmrec_amd import hip_ops
    monkeypatch.setattr(G, "USE_GPU", False)
    smo = _golden()
    asked = []
    monkeypatch.setattr(hip_ops, "spectrum_fusion",
                        lambda *a, _real=hip_ops.spectrum_fusion: asked.append(tuple(a[0].shape)) or _real(*a))
    _, loss0, g0 = _step(tmp_path / "absent", golden, monkeypatch, smo, {})
    _, loss1, g1 = _step(tmp_path / "off", golden, monkeypatch, smo, {"fused_spectrum": False})
    assert not asked                                                  # absent or False: today's path, untouched
    model, loss2, g2 = _step(tmp_path / "on", golden, monkeypatch, smo, {"fused_spectrum": True})
    assert asked == [(model.n_items, 64)]
    assert np.isfinite(float(loss0))
    assert torch.equal(loss0, loss1) and torch.equal(loss0, loss2)
    assert set(g0) == set(g1) == set(g2) and len(g0) >= 12
    for n in g0:
        assert torch.equal(g0[n], g1[n]) and torch.equal(g0[n], g2[n]), n
    for n in ("image_complex_weight", "text_complex_weight", "fusion_complex_weight"):
        assert float(g2[n].abs().max()) > 0, n


def test_the_yaml_names_the_key_in_a_comment_only():
    import yaml
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "mmrec_amd", "configs", "model", "SMORE.yaml")
    text = open(path).read()
    assert "# fused_spectrum: True" in text and "fused_spectrum" not in yaml.safe_load(text)


# ------------------------------------------------------------------------------------------------ the fuzz's checker
def mul32(a, b):
    return (np.asarray(a, F32) * np.asarray(b, F32)).astype(F32)


def emu_tables():
    """the kernel's twiddle table and its matrix F [j][slot]; slot k <= 32: re_k, slot 32 + k: im_k"""
    cos = np.cos(2 * np.pi * np.arange(64) / 64)
    cos[16] = cos[48] = 0.0
    cos = cos.astype(F32)
    n, s = np.arange(64)[:, None], np.arange(64)[None, :]
    j = (n * np.where(s <= 32, s, s - 32)) & 63
    return np.where(s <= 32, cos[j] * F32(0.125), -cos[(j - 16) & 63] * F32(0.125)).astype(F32)


def emu_stage(T, M):
    acc = np.zeros((T.shape[0], 64), F32)
    for s in range(64):
        acc = fma32(T[:, s:s + 1], M[s][None, :], acc)
    return acc


def _unpack(A):
    im = np.zeros((A.shape[0], 33), F32)
    im[:, 1:32] = A[:, 33:]
    return A[:, :33].copy(), im


def _pack(re, im):
    return np.concatenate([re, im[:, 1:32]], axis=1).astype(F32)


def _butterfly(v):
    """v [..., 64 lanes]: the wave's xor butterfly, every lane gets the total"""
    lanes = np.arange(64)
    for m in (32, 16, 8, 4, 2, 1):
        v = (v + v[..., lanes ^ m]).astype(F32)
    return v


def emu_reduce(t, n, plant=None):
    """t [n, 33] per-row terms -> the sum over rows in the kernels' order: per lane over the block's tiles, the butterfly, the
    partials' strided sums of the finish, the butterfly"""
    R, nb = Z.rows_per_block(n), Z.blocks(n)
    v = np.zeros((nb * R, 33), F32)
    v[:n] = t
    v = v.reshape(nb, R // 64, 64, 33)
    acc = np.zeros((nb, 64, 33), F32)
    for tile in range(R // 64):
        acc = (acc + v[:, tile]).astype(F32)
    part = _butterfly(acc.transpose(0, 2, 1))[..., 0]                 # [nb, 33]
    if plant == "drop_partial":
        part[0] = 0.0
    rounds = -(-nb // 64)
    padded = np.zeros((rounds * 64, 33), F32)
    padded[:nb] = part
    padded = padded.reshape(rounds, 64, 33)
    a = np.zeros((64, 33), F32)
    for r in range(rounds):
        a = (a + padded[r]).astype(F32)
    return _butterfly(a.T)[..., 0]


def emulate(x, y, w, g, plant=None):
    """fp32 numpy of the plan in include/mmrec_hip.h -> every output of both calls; `plant`: one of the errors the checker must see"""
    F = emu_tables()
    FT = np.ascontiguousarray(F.T)
    n = x.shape[0]
    wk = np.full(33, 2.0, F32)
    wk[0] = wk[32] = 1.0
    wk_f = np.ones(33, F32) if plant == "no_factor_2" else wk
    a, b = _unpack(emu_stage(x, F))
    c, e = _unpack(emu_stage(y, F))
    p3 = fma32(-e, b, mul32(c, a))
    q3 = fma32(-e if plant == "fus_sign" else e, a, mul32(c, b))
    ps, qs = (a, c, p3), (b, e, q3)
    out = {}
    d = [np.zeros((n, 33), F32) for _ in range(6)]                    # dp1, dq1, dp2, dq2, dp3, dq3
    for k in range(3):
        wr, wi = w[k, :, 0].astype(F32), w[k, :, 1].astype(F32).copy()
        wi[0] = wi[32] = 0.0
        P = wk_f * fma32(-qs[k], wi, mul32(ps[k], wr))
        Q = wk_f * fma32(ps[k], wi, mul32(qs[k], wr))
        if plant == "dc_leak" and k == 0:
            P[:, 0] = fma32(-ps[k][:, 0], w[k, 0, 1], mul32(ps[k][:, 0], wr[0]))
        out[Z.FWD_NAMES[k]] = emu_stage(_pack(P, Q), FT)
        dw = np.zeros((33, 2), F32)
        if g[k] is not None:
            dP, dQ = _unpack(emu_stage(g[k], F))
            dP, dQ = wk * dP, wk * dQ
            dw[:, 0] = emu_reduce(fma32(dQ, qs[k], mul32(dP, ps[k])), n, plant if k == 0 else None)
            dw[:, 1] = emu_reduce(fma32(dQ, ps[k], -mul32(dP, qs[k])), n)
            dw[0, 1] = dw[32, 1] = 0.0
            d[2 * k] = fma32(dQ, wi, mul32(dP, wr))
            d[2 * k + 1] = fma32(dQ, wr, -mul32(dP, wi))
        out[Z.DW_NAMES[k]] = dw
    dp1, dq1, dp2, dq2, dp3, dq3 = d
    da, db = fma32(dq3, e, fma32(dp3, c, dp1)), fma32(dq3, c, fma32(-dp3, e, dq1))
    dc, de = fma32(dq3, b, fma32(dp3, a, dp2)), fma32(dq3, a, fma32(-dp3, b, dq2))
    out["dx"] = emu_stage(_pack(dc, de) if plant == "dx_from_text" else _pack(da, db), FT)
    out["dy"] = emu_stage(_pack(dc, de), FT)
    return out


EMULATED = (1, 2, 3, 4, 6, 7, 8, 9, 15, 19, 5)                        # every small row count, then the 313-block case


@pytest.mark.parametrize("k", EMULATED)
def test_the_emulated_plan_passes_the_checker(k):
    c = Z.case(k)
    worst = Z.check(c.x, c.y, c.w, c.g, emulate(c.x, c.y, c.w, c.g), Z.name_of(c))
    print("%s emulated: worst err / bound %s" % (Z.name_of(c), " ".join("%s %.3f" % kv for kv in sorted(worst.items()))))
    assert worst and max(worst.values()) > 0.0


PLANTS = {"fus_sign": "out_fus", "no_factor_2": "out_img", "dc_leak": "out_img", "drop_partial": "dw_img", "dx_from_text": "dx"}


@pytest.mark.parametrize("k", (8, 9, 19))
@pytest.mark.parametrize("plant", sorted(PLANTS))
def test_planted_errors_do_not_pass(k, plant):
    """the sign of the fusion product's imaginary part flipped; the factor 2 of bins 1 .. 31 of the inverse dropped; the DC
    imaginary weight leaking into the output; one block's partial left out of a weight gradient; dx built from the text spectrum"""
    c = Z.case(k)
    assert c.n > 64 and not c.identity
    rng = np.random.default_rng(k)
    g = [t if t is not None else rng.standard_normal((c.n, 64)).astype(F32) for t in c.g]
    good = Z.check(c.x, c.y, c.w, g, emulate(c.x, c.y, c.w, g), "clean")
    assert max(good.values()) <= 1.0
    bad = emulate(c.x, c.y, c.w, g, plant)
    with pytest.raises(AssertionError, match="beyond the bound"):
        Z.check(c.x, c.y, c.w, g, {PLANTS[plant]: bad[PLANTS[plant]]}, plant)
