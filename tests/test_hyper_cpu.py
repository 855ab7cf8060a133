"""CPU: LGMRec's hypergraph kernels (csrc/hypergraph.hip, hip_ops.hyper_assign / hyper_layer / hyper_propagate) without a GPU --
the exports and the argument checks of the C entry points, the plan queries, what the wrappers serve, the torch compositions that
everything else (here: CPU tensors) takes bit for bit and that ARE today's inline code, LGMRec's `fused_hyper` key on the tiny
golden data (with CPU tensors both settings are torch: absent, False and True give the same loss and gradients within fp32 parity
with the same noise and masks replayed; the golden step is met with the key on, alone and with `fused_ssl`), and the checker of
tests/test_hyper_fuzz_gpu.py held honest: an fp32 numpy emulation of the kernels' plan passes it, planted errors do not."""
import os

import numpy as np
import pytest
import torch

import tests.test_hyper_fuzz_gpu as Z
import tests.test_models_gpu as G
from mmrec_amd import _lib
from tests._cpu_ops import cpu_ops  # noqa: F401  (fixture)

EXPORTS = ("mmrec_hyper_assign_fwd_f32", "mmrec_hyper_assign_bwd_f32", "mmrec_hyper_layer_fwd_f32", "mmrec_hyper_layer_bwd_f32",
           "mmrec_hyper_workspace_bytes", "mmrec_hyper_rows_per_block")
RTOL = 1e-4                    # README: fp32 parity (tests/test_score_lse_cpu.py)
BAD, UNSUPPORTED = 10001, 10002
F32 = np.float32


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        from mmrec_amd.build import build
        build(verbose=False)
    return _lib.load()


@pytest.fixture
def deterministic_torch():
    was = torch.are_deterministic_algorithms_enabled()
    torch.use_deterministic_algorithms(True)
    yield
    torch.use_deterministic_algorithms(was)


def test_exports_in_header_signatures_and_library(lib):
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mmrec_hip.h")).read()
    for name in EXPORTS:
        assert name in _lib.SIGNATURES and name in src and hasattr(lib, name), name
    assert "#define MMREC_ABI_VERSION 16" in src and lib.mmrec_abi_version() == 16 and _lib.ABI_VERSION == 16   # additive
    from mmrec_amd.build import SOURCES
    assert "hypergraph.hip" in SOURCES


def test_entry_points_refuse_bad_arguments_before_touching_memory(lib):
    """every call below would fault if a pointer were followed or a kernel launched: this machine has no device"""
    af, ab, lf, lb = (lib.mmrec_hyper_assign_fwd_f32, lib.mmrec_hyper_assign_bwd_f32, lib.mmrec_hyper_layer_fwd_f32,
                      lib.mmrec_hyper_layer_bwd_f32)
    for H in (0, 9, 64, -1):                                                        # H is 1 ... 8, checked first
        assert af(None, None, None, 5, H, 1.0, 1.0, None, None, None) == UNSUPPORTED, H
        assert ab(None, None, None, 5, H, 1.0, 1.0, None, None) == UNSUPPORTED, H
        assert lf(None, None, None, 5, 5, H, 64, None, None, None, None, None) == UNSUPPORTED, H
        assert lb(None, None, None, None, None, None, 5, 5, H, 64, None, None, None, None, None) == UNSUPPORTED, H
    for d in (0, 32, 63, 128):                                                      # ... and d is 64
        assert lf(None, None, None, 5, 5, 4, d, None, None, None, None, None) == UNSUPPORTED, d
        assert lb(None, None, None, None, None, None, 5, 5, 4, d, None, None, None, None, None) == UNSUPPORTED, d
    assert af(None, None, None, -1, 4, 1.0, 1.0, None, None, None) == BAD           # negative sizes
    assert ab(None, None, None, -1, 4, 1.0, 1.0, None, None) == BAD
    assert lf(None, None, None, -1, 5, 4, 64, None, None, None, None, None) == BAD
    assert lf(None, None, None, 5, -1, 4, 64, None, None, None, None, None) == BAD
    assert lb(None, None, None, None, None, None, 5, -1, 4, 64, None, None, None, None, None) == BAD
    assert af(None, None, None, (1 << 30) + 1, 4, 1.0, 1.0, None, None, None) == UNSUPPORTED
    assert lf(None, None, None, (1 << 30) + 1, 5, 4, 64, None, None, None, None, None) == UNSUPPORTED
    assert af(None, None, None, 5, 4, 1.0, 1.0, None, None, None) == BAD            # null pointers
    assert ab(None, None, None, 5, 4, 1.0, 1.0, None, None) == BAD
    assert lf(None, None, None, 5, 5, 4, 64, None, None, None, None, None) == BAD
    assert lb(None, None, None, None, None, None, 5, 5, 4, 64, None, None, None, None, None) == BAD
    assert af(None, None, None, 0, 4, 1.0, 1.0, None, None, None) == 0              # no rows: nothing to do
    assert ab(None, None, None, 0, 4, 1.0, 1.0, None, None) == 0


def test_plan_and_workspace(lib):
    """O(blocks H 64): the plan is a function of the row count alone, a multiple of 64, and never more than 2048 blocks"""
    assert lib.mmrec_hyper_rows_per_block(-1) == 0
    for n in (0, 1, 64, 7050, 19445, 35598, 131072, 131073, 1 << 20, 1 << 30):
        r = lib.mmrec_hyper_rows_per_block(n)
        assert r >= 64 and r % 64 == 0 and -(-n // r) <= 2048, (n, r)
        assert r == 64 or n > 131072
    for I, U, H in ((7050, 19445, 4), (18357, 35598, 4), (0, 5, 1), (5, 0, 8), (1 << 20, 1 << 20, 8)):
        ws = lib.mmrec_hyper_workspace_bytes(I, U, H)
        assert ws == 4 * (512 + (Z.blocks(I) + Z.blocks(U)) * H * 64) and ws % 16 == 0, (I, U, H, ws)
    assert lib.mmrec_hyper_workspace_bytes(5, 5, 9) == 0 and lib.mmrec_hyper_workspace_bytes(-1, 5, 4) == 0


def test_served_is_about_device_dtype_shape_and_width():
    from mmrec_amd import hip_ops

    class OnDevice(torch.Tensor):                                    # a stand-in that says it lives on the device
        is_cuda = True
    dev = lambda t: t.as_subclass(OnDevice)                          # noqa: E731
    P_i, P_u, X = torch.zeros(6, 4), torch.zeros(9, 4), torch.zeros(6, 64)
    assert not hip_ops.hyper_layer_served(P_i, P_u, X) and not hip_ops.hyper_assign_served(P_i, P_i, None)       # CPU tensors: never
    assert hip_ops.hyper_layer_served(dev(P_i), dev(P_u), dev(X))
    assert hip_ops.hyper_assign_served(dev(P_i), dev(P_i), None) and hip_ops.hyper_assign_served(dev(P_i), dev(P_i), dev(P_i))
    assert hip_ops.hyper_layer_served(dev(torch.zeros(0, 8)), dev(torch.zeros(3, 8)), dev(torch.zeros(0, 64)))    # no items, H = 8
    for bad in ((torch.zeros(6, 9), torch.zeros(9, 9), X), (P_i, torch.zeros(9, 3), X), (P_i, P_u, torch.zeros(6, 32)),
                (P_i, P_u, torch.zeros(7, 64)), (P_i, P_u, torch.zeros(6, 128)[:, ::2]), (P_i.double(), P_u, X),
                (torch.zeros(6, 8)[:, ::2], P_u, X), (None, P_u, X)):
        args = [dev(t) if isinstance(t, torch.Tensor) else t for t in bad]
        assert not hip_ops.hyper_layer_served(*args), [getattr(t, "shape", None) for t in bad]
    assert not hip_ops.hyper_assign_served(dev(torch.zeros(6, 64)), dev(torch.zeros(6, 64)), None)                # Clothing's H = 64
    assert not hip_ops.hyper_assign_served(dev(P_i), dev(P_u), None) and not hip_ops.hyper_assign_served(dev(P_i), P_i, None)
    assert not hip_ops.hyper_assign_served(dev(P_i), dev(P_i), dev(P_u))
    try:
        hip_ops.HYPER = False
        assert not hip_ops.hyper_layer_served(dev(P_i), dev(P_u), dev(X)) and not hip_ops.hyper_assign_served(dev(P_i), dev(P_i))
    finally:
        hip_ops.HYPER = True


@pytest.mark.parametrize("L", [1, 2])
@pytest.mark.parametrize("masked", [True, False])
def test_cpu_tensors_take_todays_inline_composition_bit_for_bit(deterministic_torch, L, masked):
    """hyper_assign / hyper_propagate on CPU tensors against F.gumbel_softmax and F.dropout in the forms tests/test_models_gpu.py
    replays them, and the model file's own HGNNLayer"""
    from mmrec_amd import hip_ops
    from mmrec_amd.models.lgmrec import HGNNLayer
    rng = np.random.default_rng(8)
    I, Un, H, tau, q = 37, 53, 4, 0.2, 0.5
    t = lambda *s: torch.from_numpy(rng.standard_normal(s).astype(np.float32))     # noqa: E731
    a_i, a_u, g_i, g_u, E, w = t(I, H), t(Un, H), t(I, H), t(Un, H), t(I, 64), t(Un, 64)
    m_i, m_u = ((torch.from_numpy((rng.random((n, H)) < q).astype(np.float32)) if masked else None) for n in (I, Un))
    gumbel = lambda logits, noise: ((logits + noise) / tau).softmax(-1)            # noqa: E731
    drop = lambda x, m, p=1 - q: x if m is None else x * m / (1.0 - p)             # noqa: E731
    runs = []
    for new in (True, False):
        la, lu, e = a_i.clone().requires_grad_(), a_u.clone().requires_grad_(), E.clone().requires_grad_()
        if new:
            assert not hip_ops.hyper_assign_served(la, g_i, m_i)
            P_i, P_u = hip_ops.hyper_assign(la, g_i, m_i, tau, q), hip_ops.hyper_assign(lu, g_u, m_u, tau, q)
            uo, xo = hip_ops.hyper_propagate(P_i, P_u, e, L)
            one = hip_ops.hyper_layer(P_i, P_u, e)
        else:
            P_i, P_u = drop(gumbel(la, g_i), m_i), drop(gumbel(lu, g_u), m_u)
            uo, xo = HGNNLayer(L)(P_i, P_u, e)
            one = HGNNLayer(1)(P_i, P_u, e)
        ((uo * w).sum() + (xo * xo).sum() + one[0].sum() + one[1].sum()).backward()
        runs.append((P_i.detach(), uo.detach(), xo.detach(), la.grad, lu.grad, e.grad))
    for a, b in zip(*runs):
        assert torch.equal(a, b)
    assert float(runs[0][3].abs().max()) > 0 and float(runs[0][5].abs().max()) > 0
    # ... and it IS the formulas of the fuzz file, in float64
    P64, _ = Z.assign64(a_i.numpy(), g_i.numpy(), None if m_i is None else m_i.numpy(), tau, q)
    assert float(np.abs(runs[0][0].double().numpy() - P64).max()) <= 1e-5


# ------------------------------------------------------------------------------------------------ the model's key
LGM_EXTRA = {"n_ui_layers": 2, "n_mm_layers": 2, "n_hyper_layer": 1, "hyper_num": 4, "keep_rate": 0.5, "alpha": 0.3,
             "cl_weight": 1e-4, "reg_weight": 1e-6}


def _golden():
    return dict(np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lgmrec.npz")))


def replay_draws(model, lgm, monkeypatch):
    """the reference's Gumbel noise and dropout masks: through F.* where the key is off (the forms of test_lgmrec_model), through
    `_hyper_noise` / `_hyper_keep` where it is on.  Returns the two queues."""
    import mmrec_amd.models.lgmrec as lmod
    dev = model.device
    queue_n = [torch.as_tensor(lgm["gumbel_%d" % j]).to(dev) for j in range(4)]
    queue_m = [torch.as_tensor(lgm["drop_mask_%d" % j].astype(np.float32)).to(dev) for j in range(4)]
    if model.fused_hyper:
        monkeypatch.setattr(model, "_hyper_noise", lambda logits: queue_n.pop(0))
        monkeypatch.setattr(model, "_hyper_keep", lambda x: queue_m.pop(0) if model.training else None)
    else:
        monkeypatch.setattr(lmod.F, "gumbel_softmax", lambda logits, tau=1, hard=False, dim=-1: ((logits + queue_n.pop(0)) / tau).softmax(dim))
        monkeypatch.setattr(lmod.F, "dropout", lambda x, p=0.5, training=True, inplace=False: x * queue_m.pop(0) / (1.0 - p) if training else x)
    return queue_n, queue_m


def _step(tmp_path, golden, monkeypatch, lgm, extra):
    config, _, _, model = G.build(tmp_path, golden, "LGMRec", dict(LGM_EXTRA, **extra))
    assert model.fused_hyper is bool(extra.get("fused_hyper", False))
    params = dict(model.named_parameters())
    for name, p in params.items():
        G.load(p, lgm["p_" + name])
    with monkeypatch.context() as m:
        queue_n, queue_m = replay_draws(model, lgm, m)
        model.train()
        loss = model.calculate_loss(torch.as_tensor(lgm["batch1"]).to(model.device))
        loss.backward()
        assert not queue_n and not queue_m                           # four draws of each, all consumed
    return model, loss.detach(), {n: p.grad.detach().clone() for n, p in params.items() if p.grad is not None}


def test_lgmrec_fused_hyper_key_on_the_cpu(tmp_path, golden, cpu_ops, deterministic_torch, monkeypatch):  # noqa: F811
    from mmrec_amd import hip_ops
    monkeypatch.setattr(G, "USE_GPU", False)
    lgm = _golden()
    asked = []
    for fn in ("hyper_assign", "hyper_propagate"):
        monkeypatch.setattr(hip_ops, fn, lambda *a, _real=getattr(hip_ops, fn), _fn=fn, **k: asked.append(_fn) or _real(*a, **k))
    _, loss0, g0 = _step(tmp_path / "absent", golden, monkeypatch, lgm, {})
    _, loss1, g1 = _step(tmp_path / "off", golden, monkeypatch, lgm, {"fused_hyper": False})
    assert not asked                                                  # absent or False: today's path, untouched
    assert torch.equal(loss0, loss1) and all(torch.equal(g0[n], g1[n]) for n in g0)
    _, loss2, g2 = _step(tmp_path / "on", golden, monkeypatch, lgm, {"fused_hyper": True})
    assert asked == ["hyper_assign"] * 4 + ["hyper_propagate"] * 2    # iv, uv, it, ut; image, text
    assert np.isfinite(float(loss2)) and abs(float(loss2) - float(loss1)) <= RTOL * abs(float(loss1))
    assert set(g2) == set(g1) and len(g2) >= 6
    for n in sorted(g2):
        a, b = g2[n].double().numpy(), g1[n].double().numpy()
        scale = float(np.abs(b).max())
        assert np.isfinite(a).all() and float(np.abs(a - b).max()) <= RTOL * scale, (n, float(np.abs(a - b).max()), scale)
    for n in ("v_hyper", "t_hyper", "item_id_embedding.weight"):
        assert float(g2[n].abs().max()) > 0, n


@pytest.mark.parametrize("ssl", [False, True], ids=["alone", "with_fused_ssl"])
def test_lgmrec_golden_step_is_met_with_the_key_on(tmp_path, golden, cpu_ops, monkeypatch, ssl):  # noqa: F811
    """tests/test_models_gpu.py::test_lgmrec_model's step and evaluation forward -- the reference's weights, batch, Gumbel noise
    and dropout masks replayed -- with `fused_hyper: True`, at that test's tolerances"""
    monkeypatch.setattr(G, "USE_GPU", False)
    lgm = _golden()
    model, loss, grads = _step(tmp_path, golden, monkeypatch, lgm, {"fused_hyper": True, "fused_ssl": ssl})
    assert model.fused_ssl is ssl
    G.close(loss, lgm["loss1"], rtol=1e-5)
    for name in ("user_embedding.weight", "item_id_embedding.weight", "item_image_trs", "item_text_trs", "v_hyper", "t_hyper"):
        G.close(grads[name], lgm["g_" + name], rtol=5e-4, atol=1e-8)
    model.eval()
    queue_n, queue_m = replay_draws(model, lgm, monkeypatch)
    with torch.no_grad():
        u, i, hyper = model.forward()
    assert not queue_n and len(queue_m) == 4                          # eval: noise drawn, no dropout
    G.close(u, lgm["user_out"], atol=2e-6), G.close(i, lgm["item_out"], atol=2e-6)
    G.close(hyper[0], lgm["uv_hyper"], atol=2e-6), G.close(hyper[3], lgm["it_hyper"], atol=2e-6)


def test_the_models_own_draws_have_the_right_distributions(tmp_path, golden, cpu_ops, monkeypatch):  # noqa: F811
    """`_hyper_noise`: -log(Exp(1)) (mean = Euler's constant, variance pi^2 / 6); `_hyper_keep`: Bernoulli(keep_rate) of 0 / 1 in
    training, None in eval"""
    monkeypatch.setattr(G, "USE_GPU", False)
    _, _, _, model = G.build(tmp_path, golden, "LGMRec", dict(LGM_EXTRA, fused_hyper=True, keep_rate=0.25))
    torch.manual_seed(3)
    x = torch.zeros(20000, 4)
    g = model._hyper_noise(x)
    assert g.shape == x.shape and g.dtype == x.dtype and bool(torch.isfinite(g).all())
    assert abs(float(g.mean()) - 0.5772) < 0.02 and abs(float(g.var()) - np.pi ** 2 / 6) < 0.06
    model.train()
    m = model._hyper_keep(x)
    assert m.shape == x.shape and m.dtype == x.dtype and set(m.unique().tolist()) == {0.0, 1.0} and abs(float(m.mean()) - 0.25) < 0.01
    model.eval()
    assert model._hyper_keep(x) is None
    model.train()
    assert bool(torch.isfinite(model.calculate_loss(torch.as_tensor(_golden()["batch1"]))))


# ------------------------------------------------------------------------------------------------ the fuzz's checker
def fma32(a, b, c):
    """fl32(a b + c): the product of two fp32 numbers is exact in float64"""
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(F32)


def emulate_assign(a, g, m, tau, q, plant=None):
    tau, q = F32(tau), F32(q)
    x = ((a + g).astype(F32) / tau).astype(F32)
    if x.shape[0] == 0:
        return x.copy(), x.copy()
    e = np.exp((x - x.max(axis=1, keepdims=True)).astype(F32)).astype(F32)
    s = np.zeros(x.shape[0], F32)
    for h in range(x.shape[1]):
        s = (s + e[:, h]).astype(F32)
    p = (e / s[:, None]).astype(F32)
    if m is None:
        return p, p
    P = (p * m).astype(F32)
    return (P if plant == "no_q" else (P / q).astype(F32)), p


def emulate_assign_bwd(p, m, dP, tau, q):
    tau, q = F32(tau), F32(q)
    s = dP if m is None else ((dP * m).astype(F32) / q).astype(F32)
    dot = np.zeros(p.shape[0], F32)
    for h in range(p.shape[1]):
        dot = fma32(p[:, h], s[:, h], dot)
    return ((p * (s - dot[:, None]).astype(F32)).astype(F32) / tau).astype(F32)


def emulate_partials(P, V):
    """one [H, 64] partial per block of R rows: four waves, R / 4 consecutive rows each as an fma chain, added in order"""
    n, H = P.shape
    if n == 0:
        return np.zeros((0, H, Z.D), F32)
    R = Z.rows_per_block(n)
    nb, q = -(-n // R), R // 4
    Pp, Vp = np.zeros((nb * R, H), F32), np.zeros((nb * R, Z.D), F32)                 # rows beyond n: fma(0, 0, acc) = acc
    Pp[:n], Vp[:n] = P, V
    Pp, Vp = Pp.reshape(nb, 4, q, H), Vp.reshape(nb, 4, q, Z.D)
    acc = np.zeros((nb, 4, H, Z.D), F32)
    for t in range(q):
        acc = fma32(Pp[:, :, t, :, None], Vp[:, :, t, None, :], acc)
    return (((acc[:, 0] + acc[:, 1]).astype(F32) + acc[:, 2]).astype(F32) + acc[:, 3]).astype(F32)


def emulate_finish(parts):
    nb, H = parts.shape[0], parts.shape[1]
    T = -(-nb // 16)
    pad = np.zeros((T * 16, H, Z.D), F32)
    pad[:nb] = parts
    pad = pad.reshape(T, 16, H, Z.D)
    a = np.zeros((16, H, Z.D), F32)
    for t in range(T):
        a = (a + pad[t]).astype(F32)
    v = a[0]
    for j in range(1, 16):
        v = (v + a[j]).astype(F32)
    return v


def emulate_mix(P, lat):
    o = (P[:, 0:1] * lat[0][None, :]).astype(F32)
    for h in range(1, P.shape[1]):
        o = fma32(P[:, h:h + 1], lat[h][None, :], o)
    return o


def _planted(P, plant, row):
    P = P.copy()
    live = np.flatnonzero(P[:row + 1].max(axis=1, initial=0.0) > 0)  # the last row at or before `row` that the mask has not dropped
    if not live.size:
        return P
    row = int(live[-1])
    if plant == "drop" and P.shape[0] > row:
        P[row] = 0.0                                                 # a row lost by the reduction
    if plant == "twice" and P.shape[0] > row:
        P[row] *= 2.0                                                # ... counted twice
    if plant == "wrong_edge" and P.shape[0] > row:
        P[row] = np.roll(P[row], 1)                                  # ... added to its neighbour's hyperedge
    return P


def emulate_layer(P_i, P_u, X, want_u, plant=None, row=0):
    lat = emulate_finish(emulate_partials(_planted(P_i, plant, row), X))
    out = {"lat": lat, "X_out": emulate_mix(P_i, lat)}
    if want_u:
        out["U_out"] = emulate_mix(P_u, lat)
    return out


def _dots(A, B, acc):
    """per lane of the row's 16 an fma chain over its 4 columns: A [n, 64], B [H, 64] -> acc [n, H, 16]"""
    A4, B4 = A.reshape(-1, 16, 4), B.reshape(-1, 16, 4)
    for j in range(4):
        acc = fma32(A4[:, None, :, j], B4[None, :, :, j], acc)
    return acc


def _butterfly(v):
    lane = np.arange(16)
    for mdist in (8, 4, 2, 1):
        v = (v + v[..., lane ^ mdist]).astype(F32)
    return v[..., 0]


def emulate_layer_bwd(P_i, P_u, X, lat, dU, dX, plant=None, row=0):
    I, H = P_i.shape
    Un = P_u.shape[0]
    parts = [emulate_partials(_planted(P, plant, row), g) for P, g in ((P_i, dX), (P_u, dU)) if g is not None]
    dlat = emulate_finish(np.concatenate(parts) if parts else np.zeros((0, H, Z.D), F32))
    zI, zU = np.zeros((I, Z.D), F32), np.zeros((Un, Z.D), F32)
    dpi = _butterfly(_dots(X, dlat, _dots(zI if dX is None else dX, lat, np.zeros((I, H, 16), F32))))
    dpu = _butterfly(_dots(zU if dU is None else dU, lat, np.zeros((Un, H, 16), F32)))
    return {"dP_i": dpi, "dP_u": dpu, "dX_prev": emulate_mix(P_i, dlat)}


def emulate_case(c, plant=None, row=0):
    """tests/test_hyper_fuzz_gpu.py::run_case with the emulation in the kernels' place"""
    name = Z.name_of(c) + (" planted " + plant if plant else "")
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
        got = emulate_layer(P_i, P_u, X, l == c.L - 1, plant, row)
        worst = max(worst, Z.check_layer(c, P_i, P_u, X, got, closed_f[l][1:] if c.exact else None, name + " layer %d" % l))
        kept.append((X, got["lat"]))
        X = got["X_out"]
    dU = None if c.in_null & 1 else c.dU
    dX = None if c.in_null & 2 else c.dX
    for j, l in enumerate(reversed(range(c.L))):
        Xp, lat = kept[l]
        got = emulate_layer_bwd(P_i, P_u, Xp, lat, dU, dX, plant[:-4] if plant and plant.endswith("_bwd") else None, row)
        worst = max(worst, Z.check_layer_bwd(c, P_i, P_u, Xp, lat, dU, dX, got, closed_b[j][:3] if c.exact else None,
                                             name + " layer bwd %d" % l))
        dU, dX = None, got["dX_prev"]
    return worst


EMULATED = (1, 3, 9, 11, 14, 27, 0, 5, 13, 26)                        # float cases small and large (11: 313 blocks), then exact ones


@pytest.mark.parametrize("k", EMULATED)
def test_the_emulated_plan_passes_the_checker(k):
    c = Z.case(k)
    worst = emulate_case(c)
    print("%s: emulation worst err / bound %.3f" % (Z.name_of(c), worst))
    assert worst <= 1.0 and (c.exact or worst > 0.0)


@pytest.mark.parametrize("plant", ["drop", "twice", "wrong_edge", "no_q", "drop_bwd"])
@pytest.mark.parametrize("k", [9, 14, 13, 5])
def test_planted_errors_do_not_pass(k, plant):
    """a dropped row, a row counted twice, a row added to the wrong hyperedge (each at a block or wave boundary of the reduction,
    forward; the dropped row in dlat's reduction too) and a missing 1 / q, in both modes.  Case 5 has no mask: there a missing
    1 / q plants nothing and the case must pass."""
    c = Z.case(k)
    assert c.H > 1 and c.in_null != 3 and {Z.case(j).exact for j in (9, 14, 13, 5)} == {True, False}
    row = min(Z.rows_per_block(c.I), c.I - 1)
    if plant == "no_q" and not c.masked:
        assert emulate_case(c, plant, row) <= 1.0
        return
    with pytest.raises(AssertionError, match="mismatch|beyond the bound"):
        emulate_case(c, plant, row)
