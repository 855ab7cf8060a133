"""GPU: seeded differential fuzz of MVGAE's posterior kernels (csrc/posterior.hip: mmrec_posterior_fusion_fwd_f32 / _bwd_f32)
against float64 numpy of the formulas of include/mmrec_hip.h, computed from the fp32 arrays each call was given -- never against
another kernel or the torch composition.  The raw C ABI is called over guarded, sentinel-filled outputs and a sentinel-filled
workspace of exactly the reported size.

    PoE((mu_a, l_a), (mu_b, l_b)):  T_x = 1 / (exp(l_x) + eps), S = T_a + T_b, var = 1 / S, m = (mu_a T_a + mu_b T_b) var, l = log var
    (m1, l1) = PoE(v, t);  (mu_p, l_p) = PoE((m1, l1), c);  for k in (p, v, t, c): lh_k = min(l_k, 10),
    Z[k] = mu_k + 0.1 E_k exp(0.5 lh_k),  kl[k] = -0.5 / n sum (1 + lh_k - mu_k^2 - exp(lh_k));  score = sigmoid(mu_p)
    up_k: gm_k = gZ[k] + g_kl[k] mu_k / n,  gl_k = [l_k <= 10] (gZ[k] 0.05 E_k exp(0.5 lh_k) - g_kl[k] 0.5 / n (1 - exp(lh_k)))
    PoE backward: d mu_a = gm T_a var,  d l_a = -T_a^2 exp(l_a) var (gm (mu_a - m) - gl);  stage 2 from up_p, stage 1 from its
    (g m1, g l1);  each of v, t, c adds its own up_k
(eps, 0.1, 0.05: the fp32 constants 1e-8f, 0.1f, 0.05f the kernel and torch's fp32 arithmetic both use).

ACCEPTANCE: |got - ref| <= (1 + 2^-10) e, with e a first-order bound that is carried along the float64 evaluation, operation by
operation as the PLAN of include/mmrec_hip.h names them, by the rules of tests/test_modal_fusion_fuzz_gpu.py (u = 2^-24, gamma(n),
2^-149 per rounding for underflow; one rounding: the operands' errors through the partial derivatives + u |value|; expf: E_EXP u
relative + the argument's error through the exponential; sigmoid as there, its slope written for the far tails) -- derived from that text, not tuned to a result:
    logf(x)      |log| of the argument's relative error, -log1p(-e_x / x), + E_LOG u max(|log x|, 1): the fp32 log's own error,
                 E_LOG 4 x the worst MEASURED ON THE CPU over these cases' own arguments (`test_E_LOG_covers_these_cases` in
                 tests/test_posterior_fusion_cpu.py, the rule of tests/test_score_lse_fuzz_gpu.py)
    fminf(l, 10) the error of l, or 0 where l - e_l > 10
    [l <= 10]    where |l - 10| <= e_l the kernel may stand on either side: the bound gains the gated term's magnitude
    kl[k]        every term's own error + gamma(A) sum |term|, A = 3 + 4 + R / 16 + 16 + ceil(blocks / 64) + 6 the additions of the
                 plan (columns, butterfly, passes, groups, finish, butterfly); then (-0.5 inv_n), inv_n = 1 / n with one rounding
The worst err / bound per family (Z, score, kl, d_mu, d_lv) is printed by every case and recorded in EXPERIMENTS.md section 4.
EXACTNESS, every case: the same calls again give the same bits; guards and sentinels intact; noise NULL: Z[k] is mu_k bit for bit
for k in (v, t, c); a wanted gradient with gZ and g_kl both NULL is zeros; where lv is the next float above 10 the clamp's share
is exactly 0 (d_lv there does not change by a bit when gZ[k] and g_kl[k] do, and is not zero: the PoE's share), where lv is exactly
10.0 it passes; where v == t and c carries no weight, Z[p] is mu_v to 12 u.
`test_cases_span_every_axis` needs no GPU; the checker's own tests (an fp32 emulation of the plan passes, planted errors do not)
are in tests/test_posterior_fusion_cpu.py."""
import numpy as np
import pytest
import torch

from tests.test_hyper_fuzz_gpu import _bits, _collect, _lib, _outs, compare, f64
from tests.test_edge_softmax_fuzz_gpu import E_EXP, GUARD, SENTINEL
from tests.test_spmm_fuzz_gpu import U, _on, gamma
from tests.test_modal_fusion_fuzz_gpu import FLOOR, SLACK, TINY, ex, t_add, t_div, t_exp, t_fma, t_mul, t_neg, t_sub

E_LOG = 9.0                                    # test_E_LOG_covers_these_cases: 4 x the measured 2.05, rounded up
D = 64
MAX_BLOCKS = 1024
BIG = 20011                                    # 626 blocks of two passes: every lane of the finish adds 9 or 10 partials
CASES = 64
KINDS = ("mixed", "zeros", "edge10", "equal")
INPUTS = ("mu_v", "lv_v", "mu_t", "lv_t", "mu_c", "lv_c")
NOISE = ("E_p", "E_v", "E_t", "E_c")
GRADS = ("d_mu_v", "d_lv_v", "d_mu_t", "d_lv_t", "d_mu_c", "d_lv_c")
ZS = ("Z_p", "Z_v", "Z_t", "Z_c")
FAMILY = dict(Z_p="Z", Z_v="Z", Z_t="Z", Z_c="Z", score="score", kl="kl", d_mu_v="d_mu", d_mu_t="d_mu", d_mu_c="d_mu",
              d_lv_v="d_lv", d_lv_t="d_lv", d_lv_c="d_lv")
F32 = np.float32
EPS, C01, C005 = float(F32(1e-8)), float(F32(0.1)), float(F32(0.05))
TEN = F32(10.0)
ABOVE = np.nextafter(TEN, F32(np.inf))


def rows_per_block(n):
    return int(_lib().mmrec_posterior_fusion_rows_per_block(int(n)))


def blocks(n):
    return -(-n // rows_per_block(n)) if n > 0 else 0


def n_additions(n, R=None, NB=None):
    """the additions a KL term meets: its lane's columns, the butterfly, the passes, the groups, the finish, its butterfly"""
    R = rows_per_block(n) if R is None else R
    NB = blocks(n) if NB is None else NB
    return 3 + 4 + R // 16 + 16 + -(-NB // 64) + 6


def axis_n():
    r = rows_per_block(1)
    return tuple(sorted({1, 2, 63, 64, 65, r - 1, r, r + 1, 2 * r + 1}))


class Case:
    pass


def case(k):
    ns = axis_n()
    c = Case()
    c.k = k
    c.n = n = BIG if k == 5 else ns[k % len(ns)]
    c.kind = "mixed" if k == 5 else KINDS[k % 4]
    c.g_mask = 3 if k == 5 else (k + k // 4) % 4                          # bit 0: gZ given, bit 1: g_kl
    c.noisy = k == 5 or k % 3 != 2
    mask = 63 if k == 5 else 6 if k == 63 else k % 63 + 1                 # every non-empty subset of the six gradients
    c.want = tuple(bool(mask >> i & 1) for i in range(6))
    rng = np.random.default_rng(9300 + k)
    rows = lambda: rng.standard_normal((n, D)) * rng.choice([1.0, 1e-3, 1e2], size=(n, 1), p=[0.6, 0.2, 0.2])     # noqa: E731
    o = {}
    for m in "vtc":
        o["mu_" + m] = rows()
        o["lv_" + m] = rng.uniform(-30.0, 30.0, (n, D)) if c.kind == "mixed" else rng.uniform(-12.0, 12.0, (n, D))
    noise = {key: rng.standard_normal((n, D)) for key in NOISE}
    c.cells = {}
    c.light = np.zeros(n, bool)                                           # equal: the rows where c carries no weight
    if c.kind == "zeros":
        pick = rng.random(n) < 0.5
        pick[rng.integers(0, n)] = True
        for key in o:
            o[key][pick if key[-1] != "t" else rng.permutation(pick)] = 0.0
        for key in noise:
            noise[key][pick] = 0.0
    if c.kind == "edge10":
        for m in "vtc":                                                   # exactly 10.0, and the next float above it
            where = rng.random((n, D))
            at, above = where < 0.15, where > 0.85
            at[0, rng.integers(0, D)] = True
            above[0, (np.argmax(at[0]) + 1) % D] = True
            at &= ~above
            o["lv_" + m] = o["lv_" + m].astype(F32)
            o["lv_" + m][at], o["lv_" + m][above] = TEN, ABOVE
            c.cells[m] = (at, above)
    if c.kind == "equal":
        o["lv_v"] = rng.uniform(-8.0, 12.0, (n, D))
        c.light = rng.random(n) < 0.5
        c.light[rng.integers(0, n)] = True
        o["lv_v"][c.light] = rng.uniform(-8.0, 5.0, (int(c.light.sum()), D))
        o["mu_c"][c.light], o["lv_c"][c.light] = 0.0, 30.0
        o["mu_t"], o["lv_t"] = o["mu_v"], o["lv_v"]
    c.ops = {key: np.ascontiguousarray(o[key], F32) for key in INPUTS}
    c.noise = {key: np.ascontiguousarray(v, F32) for key, v in noise.items()} if c.noisy else None
    c.gZ = rng.standard_normal((4, n, D)).astype(F32) if c.g_mask & 1 else None
    c.g_kl = rng.uniform(0.5, 2.0, 4).astype(F32) * rng.choice([-1.0, 1.0], 4).astype(F32) if c.g_mask & 2 else None
    return c


def name_of(c):
    return "case %d (n %d %s%s g %d want %s)" % (c.k, c.n, c.kind, "" if c.noisy else " no noise", c.g_mask,
                                                "".join("x" if w else "." for w in c.want))


# ------------------------------------------------------------------------------------------------ the reference and its bound
# a quantity is a pair (float64 value, first-order bound of the kernel's error in it), as in tests/test_modal_fusion_fuzz_gpu.py
def t_log(x):
    v = np.log(x[0])
    return v, -np.log1p(-np.minimum(x[1] / x[0], 0.5)) + E_LOG * U * np.maximum(np.abs(v), 1.0) + TINY


def t_sigmoid(z):
    """q = expf(-|z|), p = (z >= 0 ? 1 : q) / (1 + q): the rule of tests/test_modal_fusion_fuzz_gpu.py, with the slope p (1 - p)
    written as q / (1 + q)^2 -- far in the tails (|z| beyond 36, which MVGAE's means reach) 1 - p is 0 in float64"""
    q = np.exp(-np.abs(z[0]))
    p = np.where(z[0] >= 0, 1.0, q) / (1.0 + q)
    qlo = np.exp(-np.maximum(np.abs(z[0]) - z[1], 0.0))                   # the slope where it is LARGEST on [|z| - e, |z| + e]
    return p, qlo / (1.0 + qlo) ** 2 * z[1] + U * (q / (1.0 + q) ** 2 * E_EXP + 2 * p) + FLOOR


def t_half(x):
    return 0.5 * x[0], 0.5 * x[1]


def t_min10(l):
    return np.minimum(l[0], 10.0), np.where(l[0] - l[1] > 10.0, 0.0, l[1])


def _expert(l):
    E = t_exp(l)
    return E, t_div(ex(1.0), t_add(E, ex(EPS)))


def _poe(mu_a, xa, mu_b, xb):
    var = t_div(ex(1.0), t_add(xa[1], xb[1]))
    m = t_mul(t_fma(mu_b, xb[1], t_mul(mu_a, xa[1])), var)
    return var, m, t_log(var)


def _poe_bwd(mu_a, xa, s, gm, gl):
    E, T = xa
    var, m, _ = s
    w = t_mul(t_mul(t_mul(T, T), E), var)
    return t_mul(t_mul(gm, T), var), t_neg(t_mul(w, t_fma(gm, t_sub(mu_a, m), t_neg(gl))))


def _sum(t, A):
    return t[0].sum(), t[1].sum() + gamma(A) * np.abs(t[0]).sum() + A * TINY


def _join(a, b):
    """a + b, one rounding (t_add on arrays)"""
    return t_add(a, b)


def forward64(ops):
    """float64 values only -> (m1, l1, mu_p, l_p, var1, var2): what the span test and E_LOG's measurement read"""
    o = {k: f64(v) for k, v in ops.items()}
    T = lambda l: 1.0 / (np.exp(l) + EPS)                                 # noqa: E731
    Tv, Tt, Tc = T(o["lv_v"]), T(o["lv_t"]), T(o["lv_c"])
    var1 = 1.0 / (Tv + Tt)
    m1, l1 = (o["mu_v"] * Tv + o["mu_t"] * Tt) * var1, np.log(var1)
    T1 = T(l1)
    var2 = 1.0 / (T1 + Tc)
    return m1, l1, (m1 * T1 + o["mu_c"] * Tc) * var2, np.log(var2), var1, var2


def bounds(ops, noise, gZ, g_kl, R=None, NB=None):
    """-> {name: (float64 reference, bound, or None: exact)} for Z_p .. Z_c, score, kl and the six gradients"""
    o = {k: ex(f64(v)) for k, v in ops.items()}
    n = ops["mu_v"].shape[0]
    A = n_additions(n, R, NB)
    one = ex(1.0)
    inv_n = (np.float64(1.0) / n, U / n)
    x = {m: _expert(o["lv_" + m]) for m in "vtc"}
    s1 = _poe(o["mu_v"], x["v"], o["mu_t"], x["t"])
    x1 = _expert(s1[2])
    s2 = _poe(s1[1], x1, o["mu_c"], x["c"])
    pairs = dict(p=(s2[1], s2[2]), v=(o["mu_v"], o["lv_v"]), t=(o["mu_t"], o["lv_t"]), c=(o["mu_c"], o["lv_c"]))
    out, kls, tails = {}, [], {}
    for i, k in enumerate("pvtc"):
        mu, l = pairs[k]
        lh = t_min10(l)
        sd, el = t_exp(t_half(lh)), t_exp(lh)
        E = ex(0.0 if noise is None else f64(noise["E_" + k]))
        if noise is None:
            out["Z_" + k] = mu if k == "p" else (mu[0], None)
        else:
            out["Z_" + k] = t_fma(t_mul(ex(C01), E), sd, mu)
        term = t_sub(t_fma(t_neg(mu), mu, t_add(one, lh)), el)
        kls.append(t_mul(t_neg(t_half(inv_n)), _sum(term, A)))
        tails[k] = (mu, l, sd, el, E)
    out["kl"] = (np.array([v for v, _ in kls]), np.array([e for _, e in kls]))
    out["score"] = t_sigmoid(s2[1])
    up = {}
    for i, k in enumerate("pvtc"):
        mu, l, sd, el, E = tails[k]
        gz = ex(np.zeros((n, D)) if gZ is None else f64(gZ[i]))
        ck = ex(0.0) if g_kl is None else t_mul(ex(f64(g_kl[i])), inv_n)
        gm = t_fma(ck, mu, gz)
        gl = t_fma(gz, t_mul(t_mul(ex(C005), E), sd), t_neg(t_mul(t_half(ck), t_sub(one, el))))
        passes = l[0] <= 10.0
        unsure = (np.abs(l[0] - 10.0) <= l[1]) & (l[1] > 0)               # (an input's l is exact: never unsure)
        up[k] = (gm, (np.where(passes, gl[0], 0.0), np.where(passes | unsure, gl[1], 0.0) + np.where(unsure, np.abs(gl[0]), 0.0)))
    gm1, gl1 = _poe_bwd(s1[1], x1, s2, *up["p"])
    share = {"c": _poe_bwd(o["mu_c"], x["c"], s2, *up["p"]), "v": _poe_bwd(o["mu_v"], x["v"], s1, gm1, gl1),
             "t": _poe_bwd(o["mu_t"], x["t"], s1, gm1, gl1)}
    for k in "vtc":
        out["d_mu_" + k] = _join(share[k][0], up[k][0])
        out["d_lv_" + k] = _join(share[k][1], up[k][1])
    return {k: (v, None if e is None else SLACK * e) for k, (v, e) in out.items()}


def check(ops, noise, gZ, g_kl, got, name, R=None, NB=None):
    """got: {name: array or tensor} of any subset of the outputs (Z as Z_p .. Z_c) -> the worst err / bound per family"""
    b = bounds(ops, noise, gZ, g_kl, R, NB)
    worst = {}
    for k, v in got.items():
        v = v.reshape(b[k][0].shape) if hasattr(v, "reshape") else v
        worst[FAMILY[k]] = max(worst.get(FAMILY[k], 0.0), compare(v, *b[k], name + " " + k))
    return worst


# ------------------------------------------------------------------------------------------------ no GPU: the axes
def test_cases_span_every_axis():
    cs = [case(k) for k in range(CASES)]
    ns = axis_n()
    r = rows_per_block(1)
    assert r == 16 and rows_per_block(BIG) == 32 > r and blocks(BIG) == 626 and n_additions(BIG) == 3 + 4 + 2 + 16 + 10 + 6
    assert {1, 2, 63, 64, 65, r - 1, r, r + 1, 2 * r + 1} == set(ns)
    assert set(ns) | {BIG} == {c.n for c in cs}
    assert {c.g_mask for c in cs} == {0, 1, 2, 3} and {c.kind for c in cs} == set(KINDS)
    for kind in KINDS:
        mine = [c for c in cs if c.kind == kind]
        assert {c.g_mask for c in mine} == {0, 1, 2, 3}, kind
        assert {c.n for c in mine} >= set(ns), kind
        assert {c.noisy for c in mine} == {True, False}, kind
        assert {(c.noisy, c.g_mask) for c in mine} == {(a, b) for a in (True, False) for b in range(4)}, kind
    # every subset of the six gradients that a caller with some operand requiring a gradient can ask for
    assert {c.want for c in cs} == {tuple(bool(m >> i & 1) for i in range(6)) for m in range(1, 64)}
    big = cs[5]
    assert big.n == BIG and all(big.want) and big.g_mask == 3 and big.kind == "mixed" and big.noisy
    assert any(c.kind == "equal" and not c.noisy and c.n > 16 for c in cs)
    assert any(c.kind == "edge10" and c.g_mask == m and c.n > 16 and c.want[1] for c in cs for m in (1, 2, 3))
    for c in cs:
        lv = np.stack([c.ops["lv_" + m] for m in "vtc"])
        assert np.abs(lv).max() <= 30.0 and all(np.isfinite(v).all() for v in c.ops.values())   # the supported domain
        m1, l1, mu_p, l_p, var1, var2 = forward64(c.ops)
        if c.kind == "mixed" and c.n >= 60:
            assert lv.min() < -29 and lv.max() > 29 and (l_p > 10).any() and (l_p < -15).any()
            mags = np.abs(c.ops["mu_v"]).max(axis=1)
            assert (mags > 50).any() and (mags < 0.1).any()
        if c.kind == "zeros":
            assert any((np.abs(c.ops[a]).max(axis=1) == 0).any() for a in INPUTS)
        if c.kind == "edge10":
            for m in "vtc":
                at, above = c.cells[m]
                assert at.any() and above.any() and not (at & above).any()
                assert (c.ops["lv_" + m][at] == TEN).all() and (c.ops["lv_" + m][above] == ABOVE).all() and ABOVE > TEN
        if c.kind == "equal":
            assert c.light.any() and all((c.ops[a + "_v"] == c.ops[a + "_t"]).all() for a in ("mu", "lv"))
            lvv, muv = f64(c.ops["lv_v"]), f64(c.ops["mu_v"])
            assert np.abs(m1 - muv).max() <= 4e-16 * np.abs(muv).max()              # stage 1 of v == t: m1 = mu_v ...
            assert np.abs(l1 - (np.log(np.exp(lvv) + EPS) - np.log(2.0))).max() <= 1e-13
            assert np.abs(l1 - (lvv - np.log(2.0))).max() <= 1e-4                    # ... and l1 = lv - log 2 (exp(lv) >> eps)
            Tc, T1 = 1.0 / (np.exp(f64(c.ops["lv_c"])) + EPS), 1.0 / (np.exp(l1) + EPS)
            assert (Tc[c.light] < 2.0 ** -30 * T1[c.light]).all() and not c.ops["mu_c"][c.light].any()


# ------------------------------------------------------------------------------------------------ GPU: the raw C ABI, guarded
def _workspace(n):
    nbytes = int(_lib().mmrec_posterior_fusion_workspace_bytes(n))
    assert nbytes == blocks(n) * 4 * 4 and blocks(n) <= MAX_BLOCKS
    return torch.full((nbytes // 4 + GUARD,), SENTINEL, dtype=torch.int32, device="cuda:0"), nbytes // 4


def run_case(c, gZ="case", g_kl="case", want=None):
    """the case's forward and backward through the raw ABI -> {name: tensor} of every output written (Z as Z_p .. Z_c)"""
    from mmrec_amd import hip_ops
    p_, lib, name = hip_ops._p, _lib(), name_of(c)
    gZ, g_kl, want = (c.gZ if isinstance(gZ, str) else gZ), (c.g_kl if isinstance(g_kl, str) else g_kl), want or c.want
    ops = [_on(c.ops[k]) for k in INPUTS] + [None if c.noise is None else _on(c.noise[k]) for k in NOISE]
    shapes = {"Z": (4, c.n, D), "score": (c.n, D), "kl": (4,)}
    held, ptr = _outs(shapes)
    ws, n_ws = _workspace(c.n)
    rc = lib.mmrec_posterior_fusion_fwd_f32(*[p_(t) for t in ops], c.n, D, ptr["Z"], ptr["score"], ptr["kl"], p_(ws),
                                            hip_ops._stream())
    assert rc == 0, (name, rc)
    out = _collect(held, shapes, name)
    assert bool((ws[n_ws:] == SENTINEL).all()), (name, "wrote beyond the workspace")
    assert not bool((ws[:n_ws] == SENTINEL).any()), (name, "a block left no partial")
    out.update({"Z_" + k: out["Z"][i] for i, k in enumerate("pvtc")})
    del out["Z"]
    shapes = {k: (c.n, D) if w else None for k, w in zip(GRADS, want)}
    held, ptr = _outs(shapes)
    d_gZ, d_gkl = (None if gZ is None else _on(gZ)), (None if g_kl is None else _on(g_kl))      # held until the call is collected
    rc = lib.mmrec_posterior_fusion_bwd_f32(*[p_(t) for t in ops], p_(d_gZ), p_(d_gkl), c.n, D, *[ptr[k] for k in GRADS],
                                            hip_ops._stream())
    assert rc == 0, (name, rc)
    out.update(_collect(held, shapes, name))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("k", range(CASES))
def test_posterior_fusion_fuzz(k):
    c = case(k)
    name = name_of(c)
    got = run_case(c)
    assert set(got) == set(ZS) | {"score", "kl"} | {k_ for k_, w in zip(GRADS, c.want) if w}, name
    worst = check(c.ops, c.noise, c.gZ, c.g_kl, got, name)
    print("%s: worst err / bound %s" % (name, " ".join("%s %.3f" % kv for kv in sorted(worst.items()))))
    if not c.noisy:
        for m in "vtc":
            assert torch.equal(_bits(got["Z_" + m]), _bits(_on(c.ops["mu_" + m]))), (name, m, "noise NULL: Z[k] is mu_k")
    if c.g_mask == 0:
        for k_ in GRADS:
            if k_ in got:
                assert not bool(got[k_].any()), (name, k_, "a gradient without any g is zeros")
    if c.kind == "edge10" and c.g_mask:
        # the same call with three times the gradients of (v, t, c)'s own Z and kl: the PoE's share, from up_p alone, is the same
        gZ3 = None if c.gZ is None else c.gZ * np.array([1, 3, 3, 3], F32)[:, None, None]
        gkl3 = None if c.g_kl is None else c.g_kl * np.array([1, 3, 3, 3], F32)
        other = run_case(c, gZ3, gkl3)
        for m in "vtc":
            if "d_lv_" + m not in got:
                continue
            at, above = (torch.from_numpy(a).to("cuda:0") for a in c.cells[m])
            a, b = got["d_lv_" + m], other["d_lv_" + m]
            assert torch.equal(_bits(a[above]), _bits(b[above])), (name, m, "above 10 the clamp passes nothing")
            assert bool((a[above] != 0).any()), (name, m, "the PoE's share stays")
            moved = a[at] != b[at]
            if c.g_mask & 2:                                              # (gZ alone reaches l through the noise)
                assert bool(moved.all()), (name, m, "exactly 10 passes the gradient")
            elif c.noisy:
                assert bool(moved.any()), (name, m, "exactly 10 passes the gradient")
    if c.kind == "equal" and not c.noisy:
        light = torch.from_numpy(c.light).to("cuda:0")
        mu = _on(c.ops["mu_v"])[light].double()
        err = (got["Z_p"][light].double() - mu).abs()
        assert bool((err <= 12 * U * mu.abs() + TINY).all()), (name, "v == t, c without weight: mu_p is mu_v")
    again = run_case(c)                                                   # the same calls again: the same bits
    assert got.keys() == again.keys()
    for k_ in got:
        assert torch.equal(_bits(got[k_]), _bits(again[k_])), (name, k_, "not repeatable")


@pytest.mark.gpu
def test_wrapper_autograd_takes_the_kernels_and_honours_needs_input_grad():
    """hip_ops.posterior_fusion with only some operands requiring gradients and only some outputs used: the library is given NULL
    for the rest, the results meet the raw ABI's bounds, score carries no gradient, and an unserved call is the torch
    composition bit for bit"""
    from mmrec_amd import hip_ops
    c = case(40)
    assert c.n > 16 and c.noisy
    lib = _lib()
    needs = dict(mu_v=True, lv_v=False, mu_t=False, lv_t=True, mu_c=True, lv_c=True)
    ops = [_on(c.ops[k]).requires_grad_(needs[k]) for k in INPUTS]
    noise = [_on(c.noise[k]) for k in NOISE]
    for use in ("Z", "kl", "both"):
        seen = []
        real_b = lib.mmrec_posterior_fusion_bwd_f32
        for t in ops:
            t.grad = None
        with pytest.MonkeyPatch.context() as mp:
            mp.setattr(lib, "mmrec_posterior_fusion_bwd_f32", lambda *a: seen.append(a) or real_b(*a))
            assert hip_ops.posterior_fusion_served(*ops, noise)
            Z, kl, score = hip_ops.posterior_fusion(*ops, noise)
            assert not score.requires_grad and Z.requires_grad and kl.requires_grad
            w = torch.tensor([1.0, -2.0, 0.5, 1.5], device="cuda:0")
            ((2 * Z.sum() if use != "kl" else 0) + ((kl * w).sum() if use != "Z" else 0)).backward()
            torch.cuda.synchronize()
        assert len(seen) == 1
        a = seen[0]
        assert (a[10] is not None) == (use != "kl") and (a[11] is not None) == (use != "Z")
        assert [x is not None for x in a[14:20]] == [needs[k] for k in INPUTS]
        got = {"score": score.detach(), "kl": kl.detach()}
        got.update({"Z_" + k: Z.detach()[i] for i, k in enumerate("pvtc")})
        got.update({"d_" + k: t.grad for k, t in zip(INPUTS, ops) if needs[k]})
        assert all(t.grad is None for k, t in zip(INPUTS, ops) if not needs[k])
        gZ = None if use == "kl" else np.full((4, c.n, D), 2.0, F32)
        gkl = None if use == "Z" else w.cpu().numpy()
        print("wrapper (%s): worst err / bound" % use, check(c.ops, c.noise, gZ, gkl, got, "wrapper " + use))
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(hip_ops, "POSTERIOR_FUSION", False)
        assert not hip_ops.posterior_fusion_served(*ops, noise)
        off = hip_ops.posterior_fusion(*ops, noise)
    ref = hip_ops.posterior_fusion_torch(*ops, noise)
    assert all(torch.equal(_bits(a_.detach()), _bits(b_.detach())) for a_, b_ in zip(off, ref))
    assert not hip_ops.posterior_fusion_served(ops[0][:, ::2], *ops[1:]) and not hip_ops.posterior_fusion_served(ops[0].cpu(), *ops[1:])
    assert hip_ops.posterior_fusion_served(*ops) and not hip_ops.posterior_fusion_served(*ops, noise[:3])
