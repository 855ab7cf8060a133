"""GPU: seeded differential fuzz of MVGAE's hardest-negative reconstruction kernels (csrc/hardest_neg.hip:
mmrec_hardest_neg_fwd_f32 / _bwd_f32) and of hip_ops.hardest_negative_loss against float64 numpy of the formulas of
include/mmrec_hip.h, computed from the fp32 arrays each call was given -- never against another kernel or the torch composition.
The raw C ABI is called over guarded, sentinel-filled outputs and a sentinel-filled workspace of exactly the reported size.

    S = sigmoid(Z[l]) (squash) or Z[l];  u_b = S[users[b]], p_b = S[pos[b]], n_j = S[neg[j]]
    a_b = sigmoid(<u_b, p_b>),  h_b = max_j <u_b, n_j> over the candidates (j < B, neg[j] in [0, N)),  arg_b the LOWEST such j
    x_b = a_b - sigmoid(h_b),  loss[l] = sum_b softplus(-x_b) / ln 2
    c1 = -sg a (1 - a),  c2 = sg sh (1 - sh),  sg = sigmoid(-x) / ln 2;   G [L, 3 B, 64], slots users, pos, neg:
    user b: (g c1 p_b + g c2 n_arg_b) f(u_b);  pos b: g c1 u_b f(p_b);  neg j: (sum_{b: arg_b = j} g c2 u_b) f(n_j);  f(s) = s (1 - s) or 1
    dZ[l] = G[l] added at cat(users, pos, neg)

ACCEPTANCE: |got - ref| <= (1 + 2^-10) e, with e a first-order bound carried along the float64 evaluation, operation by operation
as the PLAN of include/mmrec_hip.h names them, by the rules of tests/test_modal_fusion_fuzz_gpu.py and
tests/test_posterior_fusion_fuzz_gpu.py (u = 2^-24, gamma(n), 2^-149 per rounding; expf: E_EXP u; the sigmoid of the far tails):
    score       a chain of 64 fma: the operands' errors through the products + gamma(64) |u| . |n|
    softplus    log1p(exp(-|y|)) + max(y, 0): the slope sigmoid(y) where it is largest on [y - e, y + e] times e, expf's E_EXP u q / (1 + q),
                E_L1P u |log1p q|: the fp32 log1p's own error, E_L1P 4 x the worst MEASURED ON THE CPU over (0, 1]
                (`test_E_L1P_covers_the_softplus` in tests/test_hardest_negative_cpu.py), and the last addition's u
    loss        every term's own error + gamma(A) sum |term|, A = ceil(B / 1024) + 6 + 16 the additions of the plan's tree
    neg slot    a chain of m fma over the m users that chose it: the terms' errors + gamma(m) sum |term|
    dZ          the slots of a row added in position order: their errors + gamma(count) sum |slot|
THE ARG.  Scores are evaluated once per DISTINCT negative id, so equal rows tie exactly in float64.  A user is SURE where its best
float64 score minus its bound exceeds every other distinct score plus that score's bound: there arg must be the reference's (the
lowest position of the best score).  Elsewhere the kernel's arg is accepted if it is a candidate within the two bounds of the best
and the lowest position of its id; that user's gradients are then checked against the reference evaluated AT THE KERNEL'S ARG.  No
case may have more than 2 % of its users unsure: `test_cases_span_every_axis` checks that on the float64 reference alone, without a
GPU.  The worst err / bound per family (loss, coef, G, dZ) is printed by every case and recorded in EXPERIMENTS.md section 4.
EXACTNESS, every case: the same calls again give the same bits; guards and sentinels intact; samples that do not contribute have
arg -1 and coefficients 0; slots without a gradient and rows no list names are exactly zero.
The checker's own tests (an fp32 emulation of the plan passes, planted errors do not) are in tests/test_hardest_negative_cpu.py."""
import numpy as np
import pytest
import torch

from tests.test_hyper_fuzz_gpu import _bits, _collect, _lib, _outs, compare, f64
from tests.test_edge_softmax_fuzz_gpu import E_EXP, GUARD, SENTINEL
from tests.test_spmm_fuzz_gpu import U, _on, gamma
from tests.test_modal_fusion_fuzz_gpu import FLOOR, SLACK, TINY, ex, t_add, t_fma, t_mul, t_neg, t_rowdot, t_sub
from tests.test_posterior_fusion_fuzz_gpu import t_sigmoid

E_L1P = 13.0                                  # test_E_L1P_covers_the_softplus: 4 x the measured 3.05, rounded up
D = 64
F32 = np.float32
INV_LN2 = float(F32(1.4426950408889634))       # the kernel's fp32 constant
FINISH_THREADS = 1024
SMALL_B = (1, 2, 31, 32, 33, 63, 64, 65, 127, 128, 129)
BIG_B = 2500
LS = (1, 4)
NS = (1, 2, 70, 5000)
FAMILIES = ("gauss", "allneg", "huge", "dups", "shared", "oor")
CASES = 45
UNSURE_MAX = 0.02
OOR = (-1, -7, -(1 << 40), 1 << 40)            # and N, N + 5: ids that are never an address


def split_cols(B, L):
    return int(_lib().mmrec_hardest_neg_split_cols(int(B), int(L)))


def n_splits(B, L):
    return -(-B // split_cols(B, L))


def edge_B():
    """a batch size that is a whole number of splits, for both L"""
    return 9 * split_cols(1100, 4)


def axis_B():
    e = edge_B()
    return SMALL_B + (e - 1, e, e + 1, BIG_B)


def n_additions(B):
    return -(-B // FINISH_THREADS) + 6 + 16


class Case:
    pass


def case(k):
    c = Case()
    c.k = k
    axis = axis_B()
    c.B = B = axis[k % len(axis)]
    c.family = FAMILIES[(k + k // len(axis)) % len(FAMILIES)]
    c.L = LS[(k + k // 2) % 2]
    c.N = N = NS[(k // 2 + k // 7) % 4]
    if c.family == "allneg" and N == 1:
        c.N = N = 2                                                        # users and negatives need rows of their own
    c.squash = {"gauss": k % 2 == 0, "allneg": False, "huge": False, "dups": True, "shared": k % 4 < 2, "oor": k % 2 == 1}[c.family]
    rng = np.random.default_rng(7100 + k)
    Z = rng.standard_normal((c.L, N, D)) * rng.choice([1.0, 0.1, 4.0], size=(c.L, N, 1), p=[0.6, 0.2, 0.2])
    if c.squash and k % 3 != 1:
        Z = Z - 3.0                                                        # most of S small: <u, p> of order 1, the sigmoids unsaturated
    ids = lambda lo, hi: rng.integers(lo, hi, B)                           # noqa: E731
    users, pos, neg = ids(0, N), ids(0, N), ids(0, N)
    if c.family == "allneg":                                               # users' rows positive, negatives' rows negative
        half = N // 2
        Z = np.abs(Z) + 0.01
        Z[:, half:] *= -1.0
        users, neg = ids(0, half), ids(half, N)
    if c.family == "huge":
        Z = Z * 1e16                                                       # scores about 1e34: finite
    if c.family == "dups":
        few = rng.integers(0, N, 3)
        users, pos, neg = few[ids(0, 3)], few[ids(0, 3)], few[ids(0, 3)]
    if c.family == "shared":
        pool = rng.integers(0, N, max(2, B // 2))
        users, pos, neg = (pool[ids(0, pool.size)] for _ in range(3))
    if c.family == "oor":
        bad = np.array(OOR + (N, N + 5), np.int64)
        for lst in (users, pos, neg):
            hit = rng.random(B) < 0.2
            lst[hit] = bad[rng.integers(0, bad.size, int(hit.sum()))]
        if B >= 31:
            neg[-1], users[0], pos[1] = N, -1, N + 5
    c.Z = np.ascontiguousarray(Z, F32)
    c.users, c.pos, c.neg = (np.ascontiguousarray(x, np.int64) for x in (users, pos, neg))
    c.g = (rng.uniform(0.5, 2.0, c.L) * rng.choice([-1.0, 1.0], c.L)).astype(F32)
    return c


def name_of(c):
    return "case %d (B %d L %d N %d %s%s)" % (c.k, c.B, c.L, c.N, c.family, " squash" if c.squash else "")


# ------------------------------------------------------------------------------------------------ the reference and its bound
def in_range(ids, N):
    return (ids >= 0) & (ids < N)


def squashed(Z, squash):
    """(value, bound) of S, [L, N, 64]"""
    return t_sigmoid(ex(f64(Z))) if squash else ex(f64(Z))


def rows(S, l, ids, ok):
    """the rows of latent l at ids (zeros where not ok) as a (value, bound) pair"""
    at = np.where(ok, ids, 0)
    return S[0][l, at] * ok[:, None], S[1][l, at] * ok[:, None]


def scores(S, l, users, neg, N):
    """-> (v, e [B, candidates], cand: their positions, ids of the candidates): one evaluation per DISTINCT negative id"""
    u_ok, n_ok = in_range(users, N), in_range(neg, N)
    cand = np.flatnonzero(n_ok)
    uniq, inv = np.unique(neg[cand], return_inverse=True)
    Uv, Ue = rows(S, l, users, u_ok)
    Kv, Ke = S[0][l, uniq], S[1][l, uniq]
    v = Uv @ Kv.T
    e = np.abs(Uv) @ Ke.T + Ue @ np.abs(Kv).T + gamma(D) * (np.abs(Uv) @ np.abs(Kv).T) + D * TINY
    return v[:, inv], e[:, inv], cand, neg[cand]


def select(v, e, cand):
    """-> (ref arg [B] as a position, its column, sure [B]): the lowest position of the best float64 score; sure where no other
    distinct score can overtake it within the bounds"""
    col = np.argmax(v, axis=1)                                             # first occurrence: the lowest position
    b = np.arange(v.shape[0])
    v1, e1 = v[b, col], e[b, col]
    other = np.where(v == v1[:, None], -np.inf, v + e)
    return cand[col], col, (v1 - e1) > other.max(axis=1, initial=-np.inf)


def t_softplus(y):
    """log(1 + exp(y)) as fmaxf(y, 0) + log1pf(expf(-|y|))"""
    q = np.exp(-np.abs(y[0]))
    lp = np.log1p(q)
    v = np.maximum(y[0], 0.0) + lp
    slope = 1.0 / (1.0 + np.exp(-(y[0] + y[1])))
    return v, slope * y[1] + U * (E_EXP * q / (1.0 + q) + E_L1P * lp + np.abs(v)) + FLOOR


def first_of_id(ids_of_cand, cand):
    """for every candidate column: the lowest candidate position that holds the same id"""
    order = np.argsort(ids_of_cand, kind="stable")
    first = np.empty(cand.size, np.int64)
    srt = ids_of_cand[order]
    head = np.r_[True, srt[1:] != srt[:-1]]
    first[order] = cand[order][np.flatnonzero(head)[np.cumsum(head) - 1]]
    return first


def unsure_fraction(c):
    """the float64 reference alone: the largest share of a latent's users whose best score is within the bounds of another"""
    S = squashed(c.Z, c.squash)
    worst = 0.0
    for l in range(c.L):
        v, e, cand, _ = scores(S, l, c.users, c.neg, c.N)
        if cand.size:
            worst = max(worst, float((~select(v, e, cand)[2]).mean()))
    return worst


def check(c, got, name, g=None):
    """got: {"arg": [L, B]} and any of loss [L], coef [L, B, 2], su [L, B, 64], G [L, 3 B, 64], dZ [L, N, 64] (arrays or tensors; g: the upstream
    gradient of G / dZ, default the case's) -> the worst err / bound per family"""
    Z, users, pos, neg, N, B, L = c.Z, c.users, c.pos, c.neg, c.N, c.B, c.L
    g = c.g if g is None else g
    arg = np.asarray(got["arg"].cpu() if isinstance(got["arg"], torch.Tensor) else got["arg"]).astype(np.int64).reshape(L, B)
    S = squashed(Z, c.squash)
    u_ok, p_ok, n_ok = in_range(users, N), in_range(pos, N), in_range(neg, N)
    one = ex(1.0)
    inv = (1.0 / np.log(2.0), 0.5 * U * INV_LN2)
    f = (lambda s: t_mul(s, t_sub(one, s))) if c.squash else None           # noqa: E731
    ref = {k: [] for k in ("loss", "coef", "su", "G", "dZ")}
    all_ids = np.concatenate([users, pos, neg])
    for l in range(L):
        v, e, cand, cand_ids = scores(S, l, users, neg, N)
        ok = u_ok & p_ok & (cand.size > 0)
        a = arg[l]
        assert (a[~ok] == -1).all(), (name, l, "a sample that does not contribute has arg -1")
        assert ((a[ok] >= 0) & (a[ok] < B)).all() and n_ok[a[ok]].all(), (name, l, "arg is no candidate")
        h = ex(np.zeros(B))
        if cand.size:
            ref_arg, col, sure = select(v, e, cand)
            assert float((~sure[ok]).mean()) <= UNSURE_MAX if ok.any() else True, (name, l, "too many unsure users")
            bad = ok & sure & (a != ref_arg)
            assert not bad.any(), (name, l, "arg is not the reference's", np.flatnonzero(bad)[:4], a[bad][:4], ref_arg[bad][:4])
            where = np.searchsorted(cand, np.where(ok, a, cand[0]))           # the kernel's arg as a column
            b = np.arange(B)
            v1, vk, ek = v[b, col], v[b, where], e[b, where]
            assert ((vk + ek >= v1 - e[b, col]) | ~ok).all(), (name, l, "arg's score is not within the bounds of the best")
            low = first_of_id(cand_ids, cand)[where]
            assert ((a == low) | ~ok).all(), (name, l, "arg is not the lowest position of equal rows", np.flatnonzero(ok & (a != low))[:4])
            h = (np.where(ok, v1, 0.0), np.where(ok, ek + (v1 - vk), 0.0))
        up, pp = rows(S, l, users, ok), rows(S, l, pos, ok)
        nn = rows(S, l, neg[np.where(ok, a, 0)], ok)
        col1 = lambda t: (t[0][:, None], t[1][:, None])                   # noqa: E731
        dp = t_rowdot(up, pp, D)
        av, sh = t_sigmoid(dp), t_sigmoid(col1(h))
        x = t_sub(av, sh)
        term = t_mul(t_softplus(t_neg(x)), inv)
        sg = t_mul(t_sigmoid(t_neg(x)), inv)
        c1 = t_neg(t_mul(sg, t_mul(av, t_sub(one, av))))
        c2 = t_mul(sg, t_mul(sh, t_sub(one, sh)))
        okc = ok[:, None]
        term, c1, c2 = ((np.where(okc, t[0], 0.0), np.where(okc, t[1], 0.0)) for t in (term, c1, c2))
        A = n_additions(B)
        ref["loss"].append((term[0].sum(), term[1].sum() + gamma(A) * np.abs(term[0]).sum() + A * TINY))
        ref["coef"].append((np.concatenate([c1[0], c2[0]], axis=1), np.concatenate([c1[1], c2[1]], axis=1)))
        ref["su"].append(up)
        if "G" not in got and "dZ" not in got:
            continue
        gl = ex(f64(g[l]))
        w1, w2 = t_mul(gl, c1), t_mul(gl, c2)
        tu = t_fma(w2, nn, t_mul(w1, pp))
        tp = t_mul(w1, up)
        M = np.zeros((B, B))                                                # neg slot j <- the samples that chose it
        M[a[ok], np.flatnonzero(ok)] = 1.0
        cnt = M.sum(axis=1)[:, None]
        prod = t_mul(w2, up)
        tn = (M @ prod[0], M @ (np.abs(w2[0]) * up[1] + np.abs(up[0]) * w2[1]) + gamma(cnt) * (M @ np.abs(prod[0])) + cnt * TINY)
        own = (rows(S, l, users, u_ok), rows(S, l, pos, p_ok), rows(S, l, neg, n_ok))
        slots = [t if f is None else t_mul(t, f(s)) for t, s in zip((tu, tp, tn), own)]
        live = np.concatenate([ok, ok, n_ok & (cnt[:, 0] > 0)])[:, None]   # every other slot is exactly zero
        Gv = np.where(live, np.concatenate([s[0] for s in slots]), 0.0)
        Ge = np.where(live, np.concatenate([s[1] for s in slots]), 0.0)
        ref["G"].append((Gv, Ge))
        if "dZ" in got:
            assert in_range(all_ids, N).all()                             # (the wrapper is never given an id out of range)
            dv, de, da, n_in = (np.zeros((N, D)) for _ in range(4))
            np.add.at(dv, all_ids, Gv)
            np.add.at(de, all_ids, Ge)
            np.add.at(da, all_ids, np.abs(Gv))
            np.add.at(n_in, all_ids, 1.0)
            ref["dZ"].append((dv, de + gamma(n_in) * da + n_in * TINY))
    worst = {}
    for k, pairs in ref.items():
        if k in got and pairs:
            val, err = np.stack([p[0] for p in pairs]), SLACK * np.stack([p[1] for p in pairs])
            v = got[k].reshape(val.shape)
            exact = err == 0.0                                            # a sample or slot without a share: exactly zero;
            mine = v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)      # an unsquashed row: a copy
            assert (mine[exact] == val[exact]).all(), (name, k, "an entry that must be exact (a zero, a copied row) is not")
            worst[k] = compare(v, val, np.where(exact, TINY, err), name + " " + k)
    return worst


# ------------------------------------------------------------------------------------------------ no GPU: the axes
def test_cases_span_every_axis():
    cs = [case(k) for k in range(CASES)]
    e = edge_B()
    assert {c.B for c in cs} == set(axis_B()) and {c.L for c in cs} == set(LS) and {c.N for c in cs} == set(NS)
    assert {c.family for c in cs} == set(FAMILIES) and {c.squash for c in cs} == {True, False}
    for L in LS:                                                          # just below, at and above a split boundary of the plan
        sc = split_cols(e, L)
        assert sc > 0 and e % sc == 0 and split_cols(e - 1, L) == sc == split_cols(e + 1, L), (L, sc)
        assert n_splits(e - 1, L) == n_splits(e, L) == n_splits(e + 1, L) - 1
    assert split_cols(65, 1) == 64 and n_splits(65, 1) == 2 and n_splits(64, 4) == 1 and n_splits(BIG_B, 4) > 4
    for fam in FAMILIES:
        mine = [c for c in cs if c.family == fam]
        assert {c.L for c in mine} == set(LS) and len({c.B for c in mine}) >= 6 and any(c.B > 1000 for c in mine), fam
    for c in cs:
        assert np.isfinite(c.Z).all() and c.Z.shape == (c.L, c.N, D) and c.users.shape == c.pos.shape == c.neg.shape == (c.B,)
        everything_in = all(in_range(x, c.N).all() for x in (c.users, c.pos, c.neg))
        assert everything_in == (c.family != "oor") or c.B < 8, name_of(c)
        S = squashed(c.Z, c.squash)
        for l in range(c.L):
            v, _, cand, _ = scores(S, l, c.users, c.neg, c.N)
            assert np.isfinite(v).all()
            if c.family == "allneg":
                assert (v < 0).all(), name_of(c)                          # a zero-scoring padding row would win
            if c.family == "huge" and c.B > 30 and c.N > 2:
                assert np.abs(v).max() > 1e30
        if c.family in ("dups", "shared") and c.B > 30:
            assert len(set(c.neg.tolist())) <= max(3, c.B // 2)
        if c.family == "shared" and c.B > 30 and c.N > 2:
            assert set(c.users.tolist()) & set(c.pos.tolist()) & set(c.neg.tolist())
        assert unsure_fraction(c) <= UNSURE_MAX, name_of(c)


# ------------------------------------------------------------------------------------------------ GPU: the raw C ABI, guarded
def _workspace(B, L):
    nbytes = int(_lib().mmrec_hardest_neg_workspace_bytes(B, L))
    assert nbytes == 4 * (2 * n_splits(B, L) + 1) * L * B
    return torch.full((nbytes // 4 + GUARD,), SENTINEL, dtype=torch.int32, device="cuda:0"), nbytes // 4


def run_raw(c, g=None, backward=True):
    """the case's forward and backward through the raw ABI -> {loss, arg, coef, G}"""
    from mmrec_amd import hip_ops
    p_, lib, name = hip_ops._p, _lib(), name_of(c)
    Z, users, pos, neg = _on(c.Z), _on(c.users), _on(c.pos), _on(c.neg)
    shapes = {"loss": (c.L,), "arg": (c.L, c.B), "coef": (c.L, c.B, 2), "su": (c.L, c.B, D)}
    held, ptr = _outs(shapes)
    ws, n_ws = _workspace(c.B, c.L)
    rc = lib.mmrec_hardest_neg_fwd_f32(p_(Z), c.N, c.L, D, p_(users), p_(pos), p_(neg), c.B, int(c.squash), ptr["loss"], ptr["arg"],
                                       ptr["coef"], ptr["su"], p_(ws), hip_ops._stream())
    assert rc == 0, (name, rc)
    out = _collect(held, shapes, name)
    assert bool((ws[n_ws:] == SENTINEL).all()), (name, "wrote beyond the workspace")
    assert not bool((ws[:n_ws] == SENTINEL).any()), (name, "a split left no (max, arg), or a sample no term")
    out["arg"] = out["arg"].view(torch.int32)
    if backward:
        shapes = {"G": (c.L, 3 * c.B, D)}
        held, ptr = _outs(shapes)
        d_g = _on(c.g if g is None else g)
        rc = lib.mmrec_hardest_neg_bwd_f32(p_(Z), c.N, c.L, D, p_(users), p_(pos), p_(neg), c.B, int(c.squash), p_(out["arg"]),
                                           p_(out["coef"]), p_(out["su"]), p_(d_g), ptr["G"], hip_ops._stream())
        assert rc == 0, (name, rc)
        out.update(_collect(held, shapes, name))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("k", range(CASES))
def test_hardest_negative_fuzz(k):
    c = case(k)
    name = name_of(c)
    got = run_raw(c)
    worst = check(c, got, name)
    print("%s: worst err / bound %s" % (name, " ".join("%s %.3f" % kv for kv in sorted(worst.items()))))
    assert set(worst) == {"loss", "coef", "su", "G"}
    again = run_raw(c)                                                    # the same calls again: the same bits
    for k_ in got:
        assert torch.equal(_bits(got[k_]), _bits(again[k_])), (name, k_, "not repeatable")


def planted(B, L, where, squash=True, seed=0):
    """a Gaussian case whose row N - 1 beats every other row for every user, named by neg at the positions `where` only"""
    c = Case()
    c.k, c.B, c.L, c.N, c.family, c.squash = -1, B, L, 300, "planted", squash
    rng = np.random.default_rng(7700 + seed)
    Z = rng.standard_normal((L, c.N, D))
    if not squash:
        Z = np.abs(Z)                                                     # every score positive, the planted row's the largest
    Z[:, -1] = 6.0
    c.Z = np.ascontiguousarray(Z, F32)
    c.users, c.pos, c.neg = (rng.integers(0, c.N - 1, B) for _ in range(3))
    c.neg[list(where)] = c.N - 1
    c.g = np.ones(L, F32)
    return c


def planted_positions(B, L):
    """first, last, the start of the last (partial) tile, and each side of every split boundary"""
    sc = split_cols(B, L)
    edges = [p for s in range(sc, B, sc) for p in (s - 1, s)]
    return sorted({0, B - 1, 64 * ((B - 1) // 64)} | set(edges[:2] + edges[-2:]))


@pytest.mark.gpu
@pytest.mark.parametrize("B,L", [(129, 1), ("above the edge", 4)])
def test_a_planted_winner_is_found_wherever_it_stands(B, L):
    B = B if isinstance(B, int) else edge_B() + 1
    spots = planted_positions(B, L)
    assert len(spots) >= 5 and (B - 1) % 64 != 63                         # the last tile is partial
    for n, p in enumerate(spots):
        c = planted(B, L, [p], squash=n % 2 == 0, seed=n)
        got = run_raw(c)
        assert bool((got["arg"] == p).all()), (B, L, p)
        check(c, got, "planted at %d" % p)
    # the same id at several positions, across tiles and splits: the LOWEST of them exactly -- equal rows score equal bits
    for n, where in enumerate(([spots[-1], spots[1], spots[2]], spots[1:], [B - 1, B - 2, 64, 63], [5, 4])):
        c = planted(B, L, where, squash=n % 2 == 1, seed=10 + n)
        got = run_raw(c, backward=False)
        assert bool((got["arg"] == min(where)).all()), (B, L, where)


@pytest.mark.gpu
def test_wrapper_autograd_takes_the_kernels():
    """hip_ops.hardest_negative_loss: loss, arg and dZ meet the raw ABI's bounds; rows no list names get exactly zero; the same
    bits on a second call; without a gradient wanted the backward is not launched; an unserved call is the torch composition"""
    from mmrec_amd import hip_ops
    lib = _lib()
    for k in (3, 17, 19, 41, 44):
        c = case(k)
        assert c.family != "oor"
        name = name_of(c)
        ids = [_on(x) for x in (c.users, c.pos, c.neg)]
        runs = []
        for _ in range(2):
            Z = _on(c.Z).requires_grad_()
            assert hip_ops.hardest_negative_loss_served(Z, *ids)
            loss, arg = hip_ops.hardest_negative_loss(Z, *ids, squash=c.squash, return_arg=True)
            assert loss.requires_grad and not arg.requires_grad and arg.dtype == torch.int32
            (loss * _on(c.g)).sum().backward()
            torch.cuda.synchronize()
            runs.append((loss.detach(), arg, Z.grad))
        for a, b in zip(*runs):
            assert torch.equal(_bits(a), _bits(b)), (name, "not repeatable")
        loss, arg, dZ = runs[0]
        worst = check(c, {"loss": loss, "arg": arg, "dZ": dZ}, "wrapper " + name)
        print("wrapper %s: worst err / bound %s" % (name, " ".join("%s %.3f" % kv for kv in sorted(worst.items()))))
        named = torch.zeros(c.N, dtype=torch.bool, device="cuda:0")
        named[torch.cat(ids)] = True
        assert not bool(dZ[:, ~named].any()), (name, "a row no list names got a gradient")
    c = case(3)
    ids = [_on(x) for x in (c.users, c.pos, c.neg)]
    seen = []
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(lib, "mmrec_hardest_neg_bwd_f32", lambda *a, _real=lib.mmrec_hardest_neg_bwd_f32: seen.append(a) or _real(*a))
        Z, w = _on(c.Z), torch.ones(c.L, device="cuda:0", requires_grad=True)
        (hip_ops.hardest_negative_loss(Z, *ids, squash=c.squash) * w).sum().backward()    # Z wants no gradient
        assert not seen and w.grad is not None
        Z = _on(c.Z).requires_grad_()
        hip_ops.hardest_negative_loss(Z, *ids, squash=c.squash).sum().backward()
        assert len(seen) == 1
    Z = _on(c.Z).requires_grad_()
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(hip_ops, "HARDEST_NEGATIVE", False)
        assert not hip_ops.hardest_negative_loss_served(Z, *ids)
        off = hip_ops.hardest_negative_loss(Z, *ids, squash=c.squash, return_arg=True)
    ref = hip_ops.hardest_negative_loss_torch(Z, *ids, squash=c.squash, return_arg=True)
    assert all(torch.equal(a, b) for a, b in zip(off, ref))
    p = planted(129, 1, [100, 70, 7])                                     # the two paths state one rule: the lowest position
    pz, pids = _on(p.Z), [_on(x) for x in (p.users, p.pos, p.neg)]
    for fn in (hip_ops.hardest_negative_loss, hip_ops.hardest_negative_loss_torch):
        assert bool((fn(pz, *pids, return_arg=True)[1] == 7).all()), fn.__name__
    assert not hip_ops.hardest_negative_loss_served(Z[:, :, ::2], *ids) and not hip_ops.hardest_negative_loss_served(Z.cpu(), *ids)
    assert not hip_ops.hardest_negative_loss_served(Z, ids[0], ids[1], ids[2][:-1].contiguous())
    assert not hip_ops.hardest_negative_loss_served(Z, ids[0].int(), ids[1], ids[2])


@pytest.mark.gpu
def test_forward_and_backward_replay_from_a_captured_graph():
    """forward + backward (the sort and the scatters included) captured on one stream and replayed: the eager bits; and the
    replay really recomputes after an input is overwritten"""
    from mmrec_amd import hip_ops
    c = case(12)
    assert c.B > 128 and c.family != "oor"
    Z = _on(c.Z).requires_grad_()
    ids = [_on(x) for x in (c.users, c.pos, c.neg)]
    w = _on(c.g)

    def step():
        Z.grad = None
        loss, arg = hip_ops.hardest_negative_loss(Z, *ids, squash=c.squash, return_arg=True)
        (loss * w).sum().backward()
        return [loss.detach(), arg, Z.grad]
    assert hip_ops.hardest_negative_loss_served(Z, *ids)
    eager = [t.clone() for t in step()]
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        held = step()
    with torch.no_grad():
        Z.copy_(_on(c.Z[:, ::-1].copy()))
    graph.replay()
    torch.cuda.synchronize()
    other = [t.clone() for t in held]
    with torch.no_grad():
        Z.copy_(_on(c.Z))
    graph.replay()
    torch.cuda.synchronize()
    first = [t.clone() for t in held]
    graph.replay()
    torch.cuda.synchronize()
    for a, b, b2 in zip(eager, first, held):
        assert torch.equal(_bits(a), _bits(b)) and torch.equal(_bits(b), _bits(b2))
    assert not torch.equal(_bits(eager[0]), _bits(other[0]))              # the replay really computed
    print("graph replay: worst err / bound", check(c, {"loss": held[0], "arg": held[1], "dZ": held[2]}, "graph"))
