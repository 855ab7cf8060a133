"""CPU: LGMRec's hypergraph kernels at 64 hyperedges (csrc/hypergraph64.hip, hip_ops.hyper64_assign / hyper64_layer /
hyper64_propagate) without a GPU -- the exports and the argument checks of the C entry points, the plan queries, what the wrappers
serve, the torch compositions that everything else (here: CPU tensors) takes bit for bit, LGMRec with Clothing's setting and
`fused_hyper: True` on the tiny golden data (CPU tensors: the key-off model bit for bit with the same draws replayed), and the
checker of tests/test_hyper64_fuzz_gpu.py held honest: an fp32 numpy emulation of the documented plan passes it, planted errors
do not."""
import os

import numpy as np
import pytest
import torch

import tests.test_hyper64_fuzz_gpu as W
import tests.test_hyper_fuzz_gpu as Z
import tests.test_models_gpu as G
from mmrec_amd import _lib
from tests._cpu_ops import cpu_ops  # noqa: F401  (fixture)
from tests.test_hyper_cpu import LGM_EXTRA, deterministic_torch, fma32, lib, replay_draws  # noqa: F401  (fixtures)

EXPORTS = ("mmrec_hyper64_assign_fwd_f32", "mmrec_hyper64_assign_bwd_f32", "mmrec_hyper64_layer_fwd_f32",
           "mmrec_hyper64_layer_bwd_f32", "mmrec_hyper64_workspace_bytes", "mmrec_hyper64_rows_per_block")
BAD, UNSUPPORTED = 10001, 10002
F32 = np.float32
CLOTHING = dict(LGM_EXTRA, hyper_num=64, n_hyper_layer=2, keep_rate=0.2)


def test_exports_in_header_signatures_and_library(lib):  # noqa: F811
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mmrec_hip.h")).read()
    for name in EXPORTS:
        assert name in _lib.SIGNATURES and name + "(" in src and hasattr(lib, name), name
    assert "#define MMREC_ABI_VERSION 16" in src and lib.mmrec_abi_version() == 16 and _lib.ABI_VERSION == 16   # additive
    from mmrec_amd.build import SOURCES
    assert "hypergraph64.hip" in SOURCES and "hypergraph.hip" in SOURCES


def test_entry_points_refuse_bad_arguments_before_touching_memory(lib):  # noqa: F811
    """every call below would fault if a pointer were followed or a kernel launched: this machine has no device"""
    af, ab, lf, lb = (lib.mmrec_hyper64_assign_fwd_f32, lib.mmrec_hyper64_assign_bwd_f32, lib.mmrec_hyper64_layer_fwd_f32,
                      lib.mmrec_hyper64_layer_bwd_f32)
    assert af(None, None, None, -1, 1.0, 1.0, None, None, None) == BAD               # negative sizes
    assert ab(None, None, None, -1, 1.0, 1.0, None, None) == BAD
    assert lf(None, None, None, -1, 5, None, None, None, None, None) == BAD
    assert lf(None, None, None, 5, -1, None, None, None, None, None) == BAD
    assert lb(None, None, None, None, None, None, -1, 5, None, None, None, None, None) == BAD
    assert lb(None, None, None, None, None, None, 5, -1, None, None, None, None, None) == BAD
    big = (1 << 30) + 1                                                               # sizes above 2^30, before any pointer
    assert af(None, None, None, big, 1.0, 1.0, None, None, None) == UNSUPPORTED
    assert ab(None, None, None, big, 1.0, 1.0, None, None) == UNSUPPORTED
    assert lf(None, None, None, big, 5, None, None, None, None, None) == UNSUPPORTED
    assert lf(None, None, None, 5, big, None, None, None, None, None) == UNSUPPORTED
    assert lb(None, None, None, None, None, None, big, 5, None, None, None, None, None) == UNSUPPORTED
    assert af(None, None, None, 5, 1.0, 1.0, None, None, None) == BAD                # null pointers with n > 0
    assert ab(None, None, None, 5, 1.0, 1.0, None, None) == BAD
    assert lf(None, None, None, 5, 5, None, None, None, None, None) == BAD
    assert lb(None, None, None, None, None, None, 5, 5, None, None, None, None, None) == BAD
    fake = [_lib.ctypes.c_void_p(4096 * (j + 1)) for j in range(4)]                   # never followed: refused first
    assert af(fake[0], fake[1], None, 5, 1.0, 1.0, fake[2], fake[2], None) == BAD     # P == p_soft
    assert lf(fake[0], None, fake[1], 5, 5, fake[2], fake[3], fake[3], fake[3], None) == BAD      # U_out wanted, P_u NULL
    assert lb(None, fake[0], None, fake[1], None, None, 5, 0, None, None, fake[2], fake[3], None) == BAD      # I > 0, P_i NULL
    assert af(None, None, None, 0, 1.0, 1.0, None, None, None) == 0                  # no rows: nothing to do
    assert ab(None, None, None, 0, 1.0, 1.0, None, None) == 0


def test_plan_and_workspace(lib):  # noqa: F811
    """the plan is a function of the row count alone: R a multiple of 64, never more than 256 blocks a side; the workspace is dlat
    and one [64][64] partial per block of either side"""
    rpb, wsb = lib.mmrec_hyper64_rows_per_block, lib.mmrec_hyper64_workspace_bytes
    assert rpb(-1) == 0 and rpb((1 << 30) + 1) == 0
    for n in (0, 1, 64, 65, 7050, 16384, 16385, 23033, 39387, 1 << 20, 1 << 30):
        r = rpb(n)
        assert r >= 64 and r % 64 == 0 and -(-n // r) <= W.MAX_BLOCKS, (n, r)
        assert (r == 64) == (n <= 64 * W.MAX_BLOCKS) and r == 64 * max(1, -(-n // (64 * W.MAX_BLOCKS)))
        assert r == W.rows_per_block(n)
    for I, U in ((23033, 39387), (7050, 19445), (0, 5), (5, 0), (0, 0), (1 << 20, 1 << 20), (16385, 16384)):
        ws = wsb(I, U)
        assert ws == 4 * 4096 * (1 + W.blocks(I) + W.blocks(U)) and ws % 16 == 0, (I, U, ws)
    assert wsb(-1, 5) == 0 and wsb(5, -1) == 0 and wsb((1 << 30) + 1, 5) == 0 and wsb(5, (1 << 30) + 1) == 0


def test_served_is_about_device_dtype_contiguity_and_width_64():
    from mmrec_amd import hip_ops

    class OnDevice(torch.Tensor):                                    # a stand-in that says it lives on the device
        is_cuda = True
    dev = lambda t: t.as_subclass(OnDevice)                          # noqa: E731
    P_i, P_u, X = torch.zeros(6, 64), torch.zeros(9, 64), torch.zeros(6, 64)
    assert not hip_ops.hyper64_layer_served(P_i, P_u, X) and not hip_ops.hyper64_assign_served(P_i, P_i, None)    # CPU tensors: never
    assert hip_ops.hyper64_layer_served(dev(P_i), dev(P_u), dev(X))
    assert hip_ops.hyper64_assign_served(dev(P_i), dev(P_i), None) and hip_ops.hyper64_assign_served(dev(P_i), dev(P_i), dev(P_i))
    assert hip_ops.hyper64_layer_served(dev(torch.zeros(0, 64)), dev(torch.zeros(3, 64)), dev(torch.zeros(0, 64)))    # no items
    for width in (8, 63, 128):
        a, b = torch.zeros(6, width), torch.zeros(9, width)
        assert not hip_ops.hyper64_assign_served(dev(a), dev(a), None), width
        assert not hip_ops.hyper64_layer_served(dev(a), dev(b), dev(X)), width
    for bad in ((P_i, torch.zeros(9, 8), X), (P_i, P_u, torch.zeros(6, 32)), (P_i, P_u, torch.zeros(7, 64)),
                (P_i, P_u, torch.zeros(6, 128)[:, ::2]), (P_i.double(), P_u, X), (torch.zeros(6, 128)[:, ::2], P_u, X), (None, P_u, X)):
        args = [dev(t) if isinstance(t, torch.Tensor) else t for t in bad]
        assert not hip_ops.hyper64_layer_served(*args), [getattr(t, "shape", None) for t in bad]
    assert not hip_ops.hyper64_assign_served(dev(P_i), dev(P_u), None) and not hip_ops.hyper64_assign_served(dev(P_i), P_i, None)
    assert not hip_ops.hyper64_assign_served(dev(P_i), dev(P_i), dev(P_u)) and not hip_ops.hyper64_assign_served(dev(P_i), dev(P_i).double())
    assert not hip_ops.hyper_assign_served(dev(P_i), dev(P_i), None) and not hip_ops.hyper_layer_served(dev(P_i), dev(P_u), dev(X))   # the narrow family: still not at 64
    try:
        hip_ops.HYPER = False
        assert not hip_ops.hyper64_layer_served(dev(P_i), dev(P_u), dev(X)) and not hip_ops.hyper64_assign_served(dev(P_i), dev(P_i))
    finally:
        hip_ops.HYPER = True


@pytest.mark.parametrize("L", [1, 2])
@pytest.mark.parametrize("masked", [True, False])
def test_cpu_tensors_take_the_inline_composition_bit_for_bit(deterministic_torch, L, masked):  # noqa: F811
    """hyper64_assign / hyper64_propagate on CPU tensors against F.gumbel_softmax and F.dropout in the forms tests/test_models_gpu.py
    replays them, and the model file's own HGNNLayer"""
    from mmrec_amd import hip_ops
    from mmrec_amd.models.lgmrec import HGNNLayer
    rng = np.random.default_rng(64)
    I, Un, H, tau, q = 37, 53, 64, 0.2, 0.2
    t = lambda *s: torch.from_numpy(rng.standard_normal(s).astype(np.float32))     # noqa: E731
    a_i, a_u, g_i, g_u, E, w = t(I, H), t(Un, H), t(I, H), t(Un, H), t(I, 64), t(Un, 64)
    m_i, m_u = ((torch.from_numpy((rng.random((n, H)) < q).astype(np.float32)) if masked else None) for n in (I, Un))
    gumbel = lambda logits, noise: ((logits + noise) / tau).softmax(-1)            # noqa: E731
    drop = lambda x, m, p=1 - q: x if m is None else x * m / (1.0 - p)             # noqa: E731
    runs = []
    for new in (True, False):
        la, lu, e = a_i.clone().requires_grad_(), a_u.clone().requires_grad_(), E.clone().requires_grad_()
        if new:
            assert not hip_ops.hyper64_assign_served(la, g_i, m_i)
            P_i, P_u = hip_ops.hyper64_assign(la, g_i, m_i, tau, q), hip_ops.hyper64_assign(lu, g_u, m_u, tau, q)
            uo, xo = hip_ops.hyper64_propagate(P_i, P_u, e, L)
            one = hip_ops.hyper64_layer(P_i, P_u, e)
        else:
            P_i, P_u = drop(gumbel(la, g_i), m_i), drop(gumbel(lu, g_u), m_u)
            uo, xo = HGNNLayer(L)(P_i, P_u, e)
            one = HGNNLayer(1)(P_i, P_u, e)
        ((uo * w).sum() + (xo * xo).sum() + one[0].sum() + one[1].sum()).backward()
        runs.append((P_i.detach(), uo.detach(), xo.detach(), la.grad, lu.grad, e.grad))
    for a, b in zip(*runs):
        assert torch.equal(a, b)
    assert float(runs[0][3].abs().max()) > 0 and float(runs[0][5].abs().max()) > 0
    P64, _ = Z.assign64(a_i.numpy(), g_i.numpy(), None if m_i is None else m_i.numpy(), tau, q)     # ... and it IS the fuzz's formula
    assert float(np.abs(runs[0][0].double().numpy() - P64).max()) <= 1e-5
    with pytest.raises(_lib.MMRecHipError):
        hip_ops.hyper64_propagate(runs[0][0], runs[0][0], E, 0)


# ------------------------------------------------------------------------------------------------ the model's key at Clothing's setting
def draws_for(model, seed=64):
    """Gumbel noise and 0 / 1 masks at the model's shapes in the order iv, uv, it, ut, as the dict `replay_draws` reads"""
    gen = torch.Generator().manual_seed(seed)
    out = {}
    for j, n in enumerate((model.n_items, model.n_users, model.n_items, model.n_users)):
        out["gumbel_%d" % j] = (-torch.empty(n, model.hyper_num).exponential_(generator=gen).log()).numpy()
        out["drop_mask_%d" % j] = (torch.rand(n, model.hyper_num, generator=gen) < model.keep_rate).numpy()
    return out


def clothing_step(tmp_path, golden, monkeypatch, extra, batch, state=None, draws=None):
    """one training step of LGMRec at Clothing's hypergraph setting -> (model, loss, gradients); the same weights where `state`"""
    config, _, _, model = G.build(tmp_path, golden, "LGMRec", dict(CLOTHING, **extra))
    assert model.fused_hyper is bool(extra.get("fused_hyper", False)) and model.hyper_num == 64 and model.n_hyper_layer == 2
    if state is not None:
        model.load_state_dict(state)
    draws = draws_for(model) if draws is None else draws
    with monkeypatch.context() as m:
        queue_n, queue_m = replay_draws(model, draws, m)
        model.train()
        loss = model.calculate_loss(torch.as_tensor(batch).to(model.device))
        loss.backward()
        assert not queue_n and not queue_m                           # four draws of each, all consumed
    return model, loss.detach(), {n: p.grad.detach().clone() for n, p in model.named_parameters() if p.grad is not None}


def test_lgmrec_clothing_setting_key_on_is_the_key_off_model_on_the_cpu(tmp_path, golden, cpu_ops, deterministic_torch, monkeypatch):  # noqa: F811
    from mmrec_amd import hip_ops
    monkeypatch.setattr(G, "USE_GPU", False)
    batch = dict(np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lgmrec.npz")))["batch1"]
    asked = []
    for fn in ("hyper_assign", "hyper_propagate", "hyper64_assign", "hyper64_propagate"):
        monkeypatch.setattr(hip_ops, fn, lambda *a, _real=getattr(hip_ops, fn), _fn=fn, **k: asked.append(_fn) or _real(*a, **k))
    off, loss0, g0 = clothing_step(tmp_path / "off", golden, monkeypatch, {}, batch)
    assert not asked                                                  # key absent: today's path, untouched
    state = {k: v.clone() for k, v in off.state_dict().items()}
    on, loss1, g1 = clothing_step(tmp_path / "on", golden, monkeypatch, {"fused_hyper": True}, batch, state)
    assert asked == ["hyper64_assign"] * 4 + ["hyper64_propagate"] * 2               # iv, uv, it, ut; image, text: the 64 family
    assert np.isfinite(float(loss1)) and torch.equal(loss0, loss1)
    assert set(g0) == set(g1) and len(g1) >= 6
    for n in sorted(g1):
        assert torch.equal(g0[n], g1[n]), n
    for n in ("v_hyper", "t_hyper", "item_id_embedding.weight"):
        assert float(g1[n].abs().max()) > 0, n
    dev = torch.zeros(5, 64)
    assert not hip_ops.hyper_assign_served(dev, dev, None)            # the narrow family still refuses 64 (here: and CPU tensors)


# ------------------------------------------------------------------------------------------------ the fuzz's checker
def emulate_assign(a, g, m, tau, q, plant=None):
    """16 lanes per row, lane t the entries 4 t .. 4 t + 3: ((e0 + e1) + e2) + e3, then the butterfly at 8, 4, 2, 1"""
    tau, q = F32(tau), F32(q)
    x = ((a + g).astype(F32) / tau).astype(F32)
    if x.shape[0] == 0:
        return x.copy(), x.copy()
    e = np.exp((x - x.max(axis=1, keepdims=True)).astype(F32)).astype(F32)
    e4 = e.reshape(-1, 16, 4)
    s = (((e4[..., 0] + e4[..., 1]).astype(F32) + e4[..., 2]).astype(F32) + e4[..., 3]).astype(F32)
    p = (e / _butterfly(s)[:, None]).astype(F32)
    if m is None:
        return p, p
    P = (p * m).astype(F32)
    P = P if plant == "no_q" else (P / q).astype(F32)
    return P, (P if plant == "p_from_P" else p)


def _butterfly(v):
    lane = np.arange(16)
    for dist in (8, 4, 2, 1):
        v = (v + v[..., lane ^ dist]).astype(F32)
    return v[..., 0]


def emulate_assign_bwd(p, m, dP, tau, q):
    tau, q = F32(tau), F32(q)
    s = dP if m is None else ((dP * m).astype(F32) / q).astype(F32)
    p4, s4 = p.reshape(-1, 16, 4), s.reshape(-1, 16, 4)
    dot = np.zeros(p4.shape[:2], F32)
    for j in range(4):
        dot = fma32(p4[..., j], s4[..., j], dot)
    dot = _butterfly(dot)
    return ((p * (s - dot[:, None]).astype(F32)).astype(F32) / tau).astype(F32)


def emulate_partials(P, V, plant=None):
    """one [64, 64] partial per block of R rows: ONE fma chain over the block's rows in order (tile after tile)"""
    n = P.shape[0]
    if n == 0:
        return np.zeros((0, W.H, W.D), F32)
    R = W.rows_per_block(n)
    nb = -(-n // R)
    Pp, Vp = np.zeros((nb * R, W.H), F32), np.zeros((nb * R, W.D), F32)               # rows beyond n: fma(0, 0, acc) = acc
    Pp[:n], Vp[:n] = P, V
    if plant == "drop":
        live = np.flatnonzero(Pp[:min(R, n - 1) + 1].max(axis=1) > 0)                 # the first row of the second block, or the last
        if live.size:                                                                 # live row before it
            Pp[live[-1]] = 0.0
    Pp, Vp = Pp.reshape(nb, R, W.H), Vp.reshape(nb, R, W.D)
    acc = np.zeros((nb, W.H, W.D), F32)
    for t in range(R):
        acc = fma32(Pp[:, t, :, None], Vp[:, t, None, :], acc)
    return acc


def emulate_finish(parts, plant=None):
    """quarter k adds the blocks k, k + 4, ... in order from 0, then the four quarters in order"""
    nb = parts.shape[0]
    if plant == "skip_partial" and nb:
        parts = parts.copy()
        parts[nb - 1] = 0.0                                                           # the last block never added
    T = -(-nb // 4)
    pad = np.zeros((T * 4, W.H, W.D), F32)
    pad[:nb] = parts
    pad = pad.reshape(T, 4, W.H, W.D)
    a = np.zeros((4, W.H, W.D), F32)
    for t in range(T):
        a = (a + pad[t]).astype(F32)
    return (((a[0] + a[1]).astype(F32) + a[2]).astype(F32) + a[3]).astype(F32)


def emulate_mix(P, M):
    """out[r][c]: one chain of 64 fmas from 0 over h ascending of P[r][h] M[h][c]"""
    o = np.zeros((P.shape[0], M.shape[1]), F32)
    for h in range(P.shape[1]):
        o = fma32(P[:, h:h + 1], M[h][None, :], o)
    return o


def emulate_dots(acc, A, B):
    """acc[r][h] += the chain over c ascending of A[r][c] B[h][c]"""
    for c in range(A.shape[1]):
        acc = fma32(A[:, c:c + 1], B[None, :, c], acc)
    return acc


def emulate_layer(P_i, P_u, X, want_u, plant=None):
    lat = emulate_finish(emulate_partials(P_i, X, plant), plant)
    used = lat
    if plant == "swap_lat":
        used = lat.copy()
        used[[0, 1]] = lat[[1, 0]]                                                    # the row pass reads a neighbour's hyperedge
    out = {"lat": lat, "X_out": emulate_mix(P_i, used)}
    if want_u:
        out["U_out"] = emulate_mix(P_u, used)
    return out


def emulate_layer_bwd(P_i, P_u, X, lat, dU, dX):
    I, Un = P_i.shape[0], P_u.shape[0]
    parts = [emulate_partials(P, g) for P, g in ((P_i, dX), (P_u, dU)) if g is not None]
    dlat = emulate_finish(np.concatenate(parts) if parts else np.zeros((0, W.H, W.D), F32))
    dpi = np.zeros((I, W.H), F32)
    if dX is not None:
        dpi = emulate_dots(dpi, dX, lat)
    dpi = emulate_dots(dpi, X, dlat)
    dpu = np.zeros((Un, W.H), F32) if dU is None else emulate_dots(np.zeros((Un, W.H), F32), dU, lat)
    return {"dP_i": dpi, "dP_u": dpu, "dX_prev": emulate_mix(P_i, dlat)}


def emulate_case(c, plant=None):
    """tests/test_hyper64_fuzz_gpu.py::run_case with the emulation in the kernels' place"""
    name = W.name_of(c) + (" planted " + plant if plant else "")
    worst, Ps = 0.0, []
    for s in (c.i, c.u):
        P, p = emulate_assign(s.a, s.g, s.m, c.tau, c.q, plant)
        da = emulate_assign_bwd(p, s.m, s.dP, c.tau, c.q)
        worst = max(worst, Z.check_assign(c, s, P, p if s.m is not None else None, name),
                    Z.check_assign_bwd(c, s, p, da, name))
        Ps.append(P)
    P_i, P_u = Ps
    closed_f, closed_b = Z.exact_chain(c) if c.exact else (None, None)
    X, kept = c.E, []
    for l in range(c.L):
        got = emulate_layer(P_i, P_u, X, l == c.L - 1, plant)
        worst = max(worst, W.check_layer(c, P_i, P_u, X, got, closed_f[l][1:] if c.exact else None, name + " layer %d" % l))
        kept.append((X, got["lat"]))
        X = got["X_out"]
    dU = None if c.in_null & 1 else c.dU
    dX = None if c.in_null & 2 else c.dX
    for j, l in enumerate(reversed(range(c.L))):
        Xp, lat = kept[l]
        got = emulate_layer_bwd(P_i, P_u, Xp, lat, dU, dX)
        worst = max(worst, W.check_layer_bwd(c, P_i, P_u, Xp, lat, dU, dX, got, closed_b[j][:3] if c.exact else None,
                                             name + " layer bwd %d" % l))
        dU, dX = None, got["dX_prev"]
    return worst


EMULATED = (1, 3, 9, 14, 19, 27, 12, 0, 8, 13, 26, 5)              # float cases small and large (12: 129 + 102 blocks), then exact ones


@pytest.mark.parametrize("k", EMULATED)
def test_the_emulated_plan_passes_the_checker(k):
    c = W.case(k)
    worst = emulate_case(c)
    print("%s: emulation worst err / bound %.3f" % (W.name_of(c), worst))
    assert worst <= 1.0 and (c.exact or worst > 0.0)


PLANTED_ON = (8, 19, 9, 29)                                         # exact masked, float masked, float, exact: two blocks or more each


@pytest.mark.parametrize("plant", ["drop", "skip_partial", "swap_lat", "no_q", "p_from_P"])
@pytest.mark.parametrize("k", PLANTED_ON)
def test_planted_errors_do_not_pass(k, plant):
    """a row dropped at a block boundary, a partial skipped by the finish, a hyperedge's lat row swapped with its neighbour's in the
    row pass, a missing 1 / q, and a p taken from P (zero at the dropped entries), in both modes.  Without a mask the last two plant
    nothing, and the case must pass."""
    c = W.case(k)
    assert W.blocks(c.I) >= 2 and {W.case(j).exact for j in PLANTED_ON} == {True, False}
    assert {W.case(j).masked for j in PLANTED_ON} == {True, False}
    if plant in ("no_q", "p_from_P") and not c.masked:
        assert emulate_case(c, plant) <= 1.0
        return
    with pytest.raises(AssertionError, match="mismatch|beyond the bound"):
        emulate_case(c, plant)
