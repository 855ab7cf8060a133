"""No GPU: the GCN layer's exports, argument checks and plan (csrc/gcn_layer.hip); hip_ops.gcn_layer on anything the kernels do not
serve is `gcn_layer_torch`, and that composition of spmm(graph, x) IS one layer of MMGCN's GCN.forward (float64: the
reassociation A (x Wc) = (A x) Wc, the [Gh | Gx] split and leaky'(0) change nothing); and the checker of
tests/test_gcn_layer_fuzz_gpu.py held honest: an fp32 numpy emulation of the kernels' plan as include/mmrec_hip.h states it passes
it on the fuzz's own cases, planted errors do not; the fuzz's kink cap holds on its whole case list."""
import os

import numpy as np
import pytest
import torch

import tests.test_gcn_layer_fuzz_gpu as Z
from mmrec_amd import _lib
from tests.test_hyper_cpu import fma32, lib  # noqa: F401  (fixture)
from tests.test_modal_fusion_cpu import emu_chain, emu_colsum, emu_outer

EXPORTS = ("mmrec_gcn_layer_rows_per_block", "mmrec_gcn_layer_workspace_bytes", "mmrec_gcn_layer_fwd_f32",
           "mmrec_gcn_layer_bwd_f32")
BAD, UNSUPPORTED = 10001, 10002
F32 = np.float32
D = 64
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_exports_in_header_signatures_and_library(lib):  # noqa: F811
    src = open(os.path.join(ROOT, "include", "mmrec_hip.h")).read()
    for name in EXPORTS:
        assert name in _lib.SIGNATURES and name in src and hasattr(lib, name), name
    assert "#define MMREC_ABI_VERSION 16" in src and lib.mmrec_abi_version() == 16 and _lib.ABI_VERSION == 16   # additive
    from mmrec_amd.build import SOURCES
    assert "gcn_layer.hip" in SOURCES


def test_entry_points_refuse_bad_arguments_before_touching_memory(lib):  # noqa: F811
    """every call below would fault if a pointer were followed or a kernel launched: this machine has no device"""
    fw, bw = lib.mmrec_gcn_layer_fwd_f32, lib.mmrec_gcn_layer_bwd_f32
    one = 1                                                                # a non-NULL pointer that must never be followed
    for d in (0, 32, 63, 65, 128):                                         # d is 64, checked first
        assert fw(*[None] * 8, 5, d, 0.01, None, None) == UNSUPPORTED, d
        assert bw(*[None] * 10, 5, d, 0.01, *[None] * 10) == UNSUPPORTED, d
        assert fw(*[None] * 8, -1, d, 0.01, None, None) == UNSUPPORTED, d
    for slope in (0.0, -0.01, float("nan")):                               # the sign of out must be the sign of q
        assert fw(*[one] * 8, 5, 64, slope, one, None) == UNSUPPORTED, slope
        assert bw(*[one] * 10, 5, 64, slope, *[one] * 9, None) == UNSUPPORTED, slope
    assert fw(*[one] * 8, (1 << 30) + 1, 64, 0.01, one, None) == UNSUPPORTED
    assert bw(*[one] * 10, (1 << 30) + 1, 64, 0.01, *[one] * 9, None) == UNSUPPORTED
    assert fw(*[one] * 8, -1, 64, 0.01, one, None) == BAD                  # a negative size
    assert bw(*[one] * 10, -1, 64, 0.01, *[one] * 9, None) == BAD
    assert fw(*[None] * 8, 0, 64, 0.01, None, None) == 0                   # no rows: nothing to do, before the NULL checks
    assert bw(*[None] * 10, 0, 64, 0.01, *[None] * 10) == 0
    for hole in (0, 1, 3, 4, 5, 6, 7):                                     # a NULL operand (R, the third, may be NULL)
        ptrs = [one] * 8
        ptrs[hole] = None
        assert fw(*ptrs, 5, 64, 0.01, one, None) == BAD, hole
        assert bw(*ptrs, one, one, 5, 64, 0.01, *[one] * 9, None) == BAD, hole
    assert fw(*[one] * 8, 5, 64, 0.01, None, None) == BAD                  # a NULL forward output
    assert bw(*[one] * 8, None, one, 5, 64, 0.01, *[one] * 9, None) == BAD     # a NULL out
    assert bw(*[one] * 9, None, 5, 64, 0.01, *[one] * 9, None) == BAD      # a NULL g
    for hole in range(3, 8):                                               # any weight gradient without a workspace
        outs = [None] * 8
        outs[hole] = one
        assert bw(*[one] * 10, 5, 64, 0.01, *outs, None, None) == BAD, hole
    ptrs = [one, one, None] + [one] * 7                                    # R NULL, nothing wanted: nothing to do
    assert bw(*ptrs, 5, 64, 0.01, *[None] * 8, None, None) == 0


def test_plan_and_workspace(lib):  # noqa: F811
    """the plan is a function of the row count alone: a multiple of 64 rows per block, never more than 256 blocks"""
    rpb, wsb = lib.mmrec_gcn_layer_rows_per_block, lib.mmrec_gcn_layer_workspace_bytes
    assert rpb(-1) == 0 and rpb((1 << 30) + 1) == 0 and wsb(-1) == 0 and wsb((1 << 30) + 1) == 0
    from mmrec_amd import hip_ops
    for n in (0, 1, 64, 7050, 16384, 16385, 26495, 54255, 1500000, 1 << 30):
        r = rpb(n)
        assert r >= 64 and r % 64 == 0 and -(-n // r) <= 256, (n, r)
        assert r == 64 * max(1, -(-n // 16384)) == hip_ops.gcn_layer_rows_per_block(n)
        assert wsb(n) == 4 * 16512 * Z.blocks(n) <= 256 * 4 * 16512
    assert Z.PART == 16512 and rpb(26495) == 128 and Z.blocks(26495) == 207 and Z.n_finish(26495) == 52 + 3
    # the kernels' LDS: eight images of 64 x 68 floats (forward 4 matrices + 4 tiles, backward 2 + 6) and the two biases
    assert 4 * (8 * 64 * 68 + 128) == 139776 <= 163840


def _operands(rng, n, d=D, dtype=torch.float32):
    t = lambda *s: torch.from_numpy(rng.standard_normal(s)).to(dtype)            # noqa: E731
    u = lambda *s: torch.from_numpy(rng.uniform(-0.125, 0.125, s)).to(dtype)     # noqa: E731
    return [t(n, d), t(n, d), t(n, d), u(d, d), u(d, d), u(d), u(d, 2 * d), u(d)]


def test_served_is_about_device_dtype_shape_and_width():
    from mmrec_amd import hip_ops

    class OnDevice(torch.Tensor):                                    # a stand-in that says it lives on the device
        is_cuda = True
    dev = lambda t: t.as_subclass(OnDevice)                          # noqa: E731
    ops = _operands(np.random.default_rng(0), 6)
    assert not hip_ops.gcn_layer_served(*ops)                        # CPU tensors: never
    assert hip_ops.gcn_layer_served(*[dev(t) for t in ops])
    no_r = [dev(t) for t in ops]
    no_r[2] = None
    assert hip_ops.gcn_layer_served(*no_r)
    assert not hip_ops.gcn_layer_served(*[dev(t) for t in ops], slope=0.0)
    assert not hip_ops.gcn_layer_served(*[dev(t) for t in ops], slope=-0.1)
    swaps = ((0, torch.zeros(6, 32)), (1, torch.zeros(7, 64)), (1, torch.zeros(6, 64).double()), (0, torch.zeros(6, 128)[:, ::2]),
             (2, torch.zeros(7, 64)), (2, torch.zeros(6, 64).double()), (3, torch.zeros(64, 32)), (3, torch.zeros(1, 64, 64)),
             (4, torch.zeros(64, 64).double()), (5, torch.zeros(1, 64)), (6, torch.zeros(64, 64)), (6, torch.zeros(64, 256)[:, ::2]),
             (7, torch.zeros(63)), (0, None), (1, None), (6, None))
    for at, bad in swaps:
        args = [dev(t) for t in ops]
        args[at] = dev(bad) if bad is not None else None
        assert not hip_ops.gcn_layer_served(*args), (at, getattr(bad, "shape", None))
    args = [dev(t) for t in ops]
    args[2] = ops[2]                                                 # R on the host
    assert not hip_ops.gcn_layer_served(*args)
    empty = [dev(torch.zeros(0, 64)) for _ in range(3)] + [dev(t) for t in ops[3:]]
    assert not hip_ops.gcn_layer_served(*empty)
    try:
        hip_ops.GCN_LAYER = False
        assert not hip_ops.gcn_layer_served(*[dev(t) for t in ops])
    finally:
        hip_ops.GCN_LAYER = True


def test_everything_unserved_runs_the_torch_composition(monkeypatch):
    """CPU tensors, width 32, no id embedding and a non-contiguous operand all run `gcn_layer_torch` -- and give its bits"""
    from mmrec_amd import hip_ops
    calls = []
    real = hip_ops.gcn_layer_torch
    monkeypatch.setattr(hip_ops, "gcn_layer_torch", lambda *a: calls.append(tuple(a[0].shape)) or real(*a))
    rng = np.random.default_rng(3)
    ops = _operands(rng, 9)
    narrow = _operands(rng, 9, d=32)
    wide = torch.zeros(9, 128)
    wide[:, ::2] = ops[0]
    strided = [wide[:, ::2]] + ops[1:]
    assert not strided[0].is_contiguous()
    no_r = ops[:2] + [None] + ops[3:]
    for args in (ops, narrow, strided, no_r):
        got = hip_ops.gcn_layer(*args)
        assert torch.equal(got, real(*args)) and got.shape == (9, args[0].shape[1])
    assert calls == [(9, 64), (9, 32), (9, 64), (9, 64)]
    assert torch.equal(hip_ops.gcn_layer(*ops, slope=0.2), real(*ops, 0.2))
    assert not torch.equal(hip_ops.gcn_layer(*ops), hip_ops.gcn_layer(*no_r))


def test_the_op_is_one_layer_of_gcn_forward_in_float64():
    """the literal three lines of mmgcn.py's GCN.forward, spmm(graph, x @ Wc) form, against hip_ops.gcn_layer of (A x, x, ...) on
    CPU float64 tensors: the result and all seven gradients to 1e-5 relative.  Rows of x and of A are zero, with bl zero at some
    columns: a and p are exact zeros there in both forms, so leaky'(0) = slope is pinned too."""
    from mmrec_amd import hip_ops
    fn = torch.nn.functional
    rng = np.random.default_rng(21)
    n, slope = 37, 0.01
    A = (rng.random((n, n)) < 0.3) * rng.random((n, n))
    A[5] = 0.0
    A[11] = 0.0
    A = torch.from_numpy(A)
    vals = [t.double() for t in _operands(rng, n)][1:]                # x, R, Wc, Wl, bl, Wg, bg
    vals[0][3] = 0.0
    vals[0][11] = 0.0
    vals[4][:] = 0.0                                                  # bl: p of a zero x row is an exact zero
    gout = torch.from_numpy(rng.standard_normal((n, D)))

    def run(fused):
        x, R, Wc, Wl, bl, Wg, bg = leaves = [v.clone().requires_grad_() for v in vals]
        if fused:
            out = hip_ops.gcn_layer(A @ x, x, R, Wc, Wl, bl, Wg, bg, slope)
        else:
            h = fn.leaky_relu(A @ (x @ Wc), slope)
            x_hat = fn.leaky_relu(fn.linear(x, Wl, bl), slope) + R
            out = fn.leaky_relu(fn.linear(torch.cat((h, x_hat), dim=1), Wg, bg), slope)
        (out * gout).sum().backward()
        return [out.detach()] + [t.grad for t in leaves]
    lit, fused = run(False), run(True)
    assert len(lit) == 8
    for a, b in zip(lit, fused):
        assert float(a.abs().max()) > 0 and float((a - b).abs().max()) <= 1e-5 * float(a.abs().max())
    # leaky'(0) is the slope, and the halves of Wg are [Gh | Gx]: the closed form on one row whose a and p are exact zeros
    x, R, Wc, Wl, bl, Wg, bg = vals
    q = fn.leaky_relu(torch.zeros(D).double(), slope) @ Wg[:, :D].T + R[11] @ Wg[:, D:].T + bg
    assert float((lit[0][11] - fn.leaky_relu(q, slope)).abs().max()) <= 1e-12
    dq = gout[11] * torch.where(q > 0, torch.ones_like(q), torch.full_like(q, slope))
    assert float((fused[2][11] - dq @ Wg[:, D:]).abs().max()) <= 1e-12                       # dR = dq Gx


def test_the_torch_composition_is_the_fuzz_reference():
    """`gcn_layer_torch` in float64 == the float64 numpy that the fuzz compares the kernels with, outputs and gradients"""
    from mmrec_amd import hip_ops
    for k in (6, 27):
        c = Z.case(k)
        assert c.n == 129 and not c.g_zero and c.r_null == (k == 27)
        ref = Z.bounds(c.ops, c.g)
        ops = [None if c.ops[k_] is None else torch.from_numpy(c.ops[k_]).double().requires_grad_() for k_ in Z.OPERANDS]
        out = hip_ops.gcn_layer_torch(*ops, float(np.float32(Z.SLOPE)))
        (out * torch.from_numpy(c.g).double()).sum().backward()
        for name, got in [("out", out.detach())] + [("d" + k_, t.grad) for k_, t in zip(Z.OPERANDS, ops) if t is not None]:
            r = ref[name][0]
            assert float(np.abs(got.numpy() - r).max()) <= 1e-11 * float(np.abs(r).max()), name


def test_the_yaml_names_the_key_in_a_comment_only():
    import yaml
    text = open(os.path.join(ROOT, "mmrec_amd", "configs", "model", "MMGCN.yaml")).read()
    assert "# fused_layers: True" in text and "fused_layers" not in yaml.safe_load(text)


def test_cases_span_every_axis():
    Z.cases_span_every_axis()


# ------------------------------------------------------------------------------------------------ the fuzz's checker
def emulate(ops, g, plant=None):
    """fp32 numpy of the plan in include/mmrec_hip.h -> every output of both calls; `plant`: one of the errors the checker must see"""
    AX, X, Rt = ops["AX"], ops["X"], ops["R"]
    n = AX.shape[0]
    R = Z.rows_per_block(n)
    slope, one = F32(Z.SLOPE), F32(1.0)
    zero = np.zeros((1, D), F32)
    Gh, Gx = ops["Wg"][:, :D], ops["Wg"][:, D:]
    if plant == "swapped_halves":
        Gh, Gx = Gx, Gh
    if plant == "no_R":
        Rt = None
    leaky = lambda z: np.where(z > 0, z, (slope * z).astype(F32)).astype(F32)     # noqa: E731
    a = emu_chain(AX, ops["Wc"], zero)
    h = leaky(a)
    p = emu_chain(X, ops["Wl"].T, zero if plant == "no_bias" else ops["bl"][None, :])
    xh = leaky(p) if Rt is None else (leaky(p) + Rt).astype(F32)
    q = emu_chain(xh, Gx.T, emu_chain(h, Gh.T, ops["bg"][None, :]))
    res = {"out": leaky(q)}
    dq = (g * np.where(res["out"] > 0, one, slope)).astype(F32)
    dh = emu_chain(dq, Gh, zero)
    sign_a = (a < 0) if plant == "wrong_sign" else (a >= 0) if plant == "slope_at_0" else (a > 0)
    da = (dh * np.where(sign_a, one, slope)).astype(F32)
    dxh = emu_chain(dq, Gx, zero)
    dp = (dxh * np.where(p > 0, one, slope)).astype(F32)
    res["dR"] = dxh
    res["dAX"], res["dX"] = emu_chain(da, ops["Wc"].T, zero), emu_chain(dp, ops["Wl"], zero)
    res["dWc"] = emu_outer([(AX, da)], n, R)
    res["dWl"] = emu_outer([(dp, X)], n, R)
    res["dWg"] = np.concatenate([emu_outer([(dq, h)], n, R), emu_outer([(dq, xh)], n, R)], axis=1)
    res["dbl"], res["dbg"] = emu_colsum(dp, n, R), emu_colsum(dq, n, R)
    return res


EMULATED = (1, 2, 3, 4, 6, 9, 10, 11, 12, 13, 20, 27, 5)            # every small row count and kind, then the 157-block case


@pytest.mark.parametrize("k", EMULATED)
def test_the_emulated_plan_passes_the_checker(k):
    c = Z.case(k)
    assert c.n
    worst = Z.check(c.ops, c.g, emulate(c.ops, c.g), Z.name_of(c))
    print("%s emulated: worst err / bound %s" % (Z.name_of(c), " ".join("%s %.3f" % kv for kv in sorted(worst.items()))))
    assert set(worst) == {"out", "dx", "dw", "db"} and max(worst.values()) > 0.0


def test_the_emulation_covers_every_row_count_and_kind():
    cs = [Z.case(k) for k in EMULATED]
    assert {c.n for c in cs} == (set(Z.axis_n()) - {0}) | {Z.BIG} and {c.kind for c in cs} == set(Z.KINDS)
    assert {c.r_null for c in cs} == {True, False}


def _with_g(c):
    return c.g if not c.g_zero else np.random.default_rng(c.k).standard_normal(c.g.shape).astype(F32)


def test_a_slip_of_1024_ulps_in_one_output_does_not_pass():
    """the entry of `out` whose bound is the smallest in units of its last place, moved by 1024 of them (6e-5 of its value).  q is
    a chain of 128 terms of mixed signs, so even that entry's first-order bound is some 160 units wide"""
    c = Z.case(18)
    assert c.n == 64 and c.kind == "mixed"
    ref, e = Z.bounds(c.ops, c.g)["out"]
    good = emulate(c.ops, c.g)["out"]
    ulp = np.spacing(np.abs(good)).astype(np.float64)
    at = np.unravel_index(np.argmax(ulp / e), ref.shape)
    assert 1024 * ulp[at] > 1.5 * e[at] > 64 * ulp[at]                                 # ... is beyond the bound wherever in it the clean value lies
    assert Z.check(c.ops, c.g, {"out": good}, "clean")["out"] <= 0.5
    bad = good.copy()
    bad[at] = good[at] + F32(1024) * np.spacing(good[at])
    with pytest.raises(AssertionError, match="beyond the bound"):
        Z.check(c.ops, c.g, {"out": bad}, "ulp")


# swapped halves and a dropped bias: any case; a missing R: R given; the wrong sign: any case; the slope at 0: rows with a = 0 exactly
PLANTS = {"swapped_halves": ("out", (6, 18, 30)), "no_R": ("out", (6, 12, 30)), "no_bias": ("out", (6, 18, 27)),
          "wrong_sign": ("dAX", (6, 18, 27)), "slope_at_0": ("dAX", (10, 19, 34))}
PLANTED = [(p, k) for p in sorted(PLANTS) for k in PLANTS[p][1]]


@pytest.mark.parametrize("plant,k", PLANTED)
def test_planted_errors_do_not_pass(k, plant):
    """Gh and Gx swapped; the id embedding left out; bl dropped; leaky'(a) taken from the opposite sign; leaky' taken as 1 at
    exactly 0"""
    c = Z.case(k)
    g = _with_g(c)
    assert c.n > 1
    if plant == "no_R":
        assert not c.r_null
    if plant == "no_bias":
        assert c.kind != "zero_x"
    if plant == "slope_at_0":
        assert c.kind == "zero_ax" and c.zero_rows.any()
    good = Z.check(c.ops, g, emulate(c.ops, g), "clean")
    assert max(good.values()) <= 1.0
    bad = emulate(c.ops, g, plant)
    name = PLANTS[plant][0]
    with pytest.raises(AssertionError, match="beyond the bound"):
        Z.check(c.ops, g, {name: bad[name]}, plant)


def test_the_kink_cap_holds_on_the_whole_case_list():
    """on the float64 reference alone: the entries of a, p and q whose sign the bound cannot decide (their gradient bound is
    widened, they are not excluded) are at most 2e-4 of all entries.  Nothing is planted near a kink except exact zeros (zero AX
    rows; zero X rows with zero bl): their bound is 0, so their sign is decided."""
    und, total = {"a": 0, "p": 0, "q": 0}, 0
    for k in range(Z.CASES):
        c = Z.case(k)
        if not c.n:
            continue
        info = {}
        Z.bounds(c.ops, c.g, info=info)
        for z in und:
            und[z] += int(info["und_" + z].sum())
        if c.kind == "zero_ax":
            assert not info["a"][0][c.zero_rows].any() and not info["a"][1][c.zero_rows].any()
            assert not info["und_a"][c.zero_rows].any()
        if c.kind == "zero_x":
            assert not info["p"][0][c.zero_rows].any() and not info["p"][1][c.zero_rows].any()
            assert not info["und_p"][c.zero_rows].any()
        total += c.n * D
    print("undecided signs: a %d, p %d, q %d of %d entries each: %s" % (und["a"], und["p"], und["q"], total,
                                                                       ", ".join("%.2e" % (v / total) for v in und.values())))
    assert total > 1.2e6 and sum(und.values()) <= 2e-4 * 3 * total
    assert all(v <= 2e-4 * total for v in und.values())
