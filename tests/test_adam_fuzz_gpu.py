"""Seeded differential fuzz of csrc/adam.hip -- the dense step (host / device-scalar form), the multi-tensor table, the row-lazy
catch-up / step (host and device form) and the opt-in fast-forward -- against dense Adam in float64 numpy written here from the
formulas of include/mmrec_hip.h and torch.optim.Adam, never against another form of the same kernels:

    g += wd p;  m += (1 - b1)(g - m);  v = b2 v + (1 - b2) g^2;  p -= A m / (sqrt(v) B + eps)
    A = fp32(lr / (1 - b1^t)),  B = fp32(1 / sqrt(1 - b2^t))        (the hyper pair: double arithmetic, rounded to fp32)

with the fp32 constants the ABI receives.  The reference runs on the WHOLE table every step (a zero gradient where a row is
absent); the row-lazy kernels are compared on the listed rows after each catch-up, after each step and after the final flush.
The C ABI is called with raw pointers; p, m, v, last_step, owner and hist carry GUARD sentinel elements on both sides, checked
after every call.  HipAdam / LazyRowEmbedding run on top for a subset of seeds.

Tolerance (derived, not tuned): next to the reference runs a first-order error bound per element (Em, Ev, Ep), u = 2^-24:
  1. one u per fp32 rounding of the formula (fma(wd, p, g): 1; g - m and the fma of m: 2; g g, v b2 and the fma of v: 3), carried
     from step to step (Em' = b1 Em + ..., Ev' = b2 Ev + ...); the moments' errors reach the update through d upd / d m = A / den
     and through the two-sided difference of sqrt(v +- Ev) (no derivative: v may be 0);
  2. p's own rounding: min(half an ulp of p, |update| + its bound) per step -- p itself is a representable candidate for the
     rounded difference, so an update below half an ulp costs at most itself (what the row-lazy "settled" shortcut relies on);
  3. E u |update| per step for the square root, the reciprocal and the three products.  E is MEASURED ON THE CPU
     (`test_E_is_four_times_the_measured_worst`): the fp32 numpy restatement of the update at the fp32-rounded float64 moments
     after EVERY step of every float case's reference (its own hyper pair, all elements) against float64, worst error in units of u |update|, times 4, not below 4, plus 2 for v_sqrt_f32 and
     v_rcp_f32 (1 ulp each by the instruction set; numpy's are correctly rounded).  Measured worst 3.83 (six roundings of at most u each bound it
     by 6) -> E = 4 x 3.83 + 2 = 17.4 (rounded up) = E_ADAM;
  4. 2^-63 B / eps relative to the update where v - Ev < 2^-126 (a denormal that the hardware square root may flush: sqrt is
     off by at most 2^-63 against a denominator >= eps), and FLOOR = 4 x 2^-126 on m, v and the update.  A gradient of 1e-20
     gives v ~ 1e-43: with eps = 1e-8 the term is 3e-10 of an update, harmless, and the test says so with this bound.
Fast-forward: the bound above for the trajectory plus what the header states for the closed form: 2e-6 of the distance p moved
in the gap, 1e-6 sqrt(n) of |m| and |v| (added for every row that MAY take the closed form: no weight decay, more than 12
steps after max(last visit, step 128), gap <= 256 or b1^256 < 1e-9).  Inside a whole row-lazy run (`run_lazy`) these allowances
stay with the row, and the moments' one reaches p through every LATER update, to first order d upd / upd = d m / m + d v / 2 v:
1.5e-6 sqrt(n) of each later |update| of the row is added to tol(p) (cumulative over the row's closed-form catch-ups; it is not
let decay although a gradient step shrinks the moments' relative error: an over-estimate).
Non-finite gradients (inf / NaN in a few elements) are cases of their own: those elements are non-finite exactly where the
formula is (g = inf: m = v = inf, p = NaN), every other element keeps the float bound.  Float cases keep |g| <= 1e18.
Sharpness (`test_tolerances_stay_sharp`, CPU, every float case): for >= 90 % of the elements that moved tol(p) <= 1 % of the
summed |update|; tol(m), tol(v) <= 1e-4 |ref| where |ref| > 1e-6 -- but for the two fast-forward cases with gaps of 3000 steps:
a replay rounds v once per step, 3000 u = 1.8e-4, whatever the inputs; they are held to the p condition.  Inputs: |p| <= 4, lr in {1e-4, 1e-3, 1e-2}, gradients
of the sign of a pre-filled m (no cancellation of the update).

Next to the bound, bit for bit: guards; rows not listed or listed as -1 unchanged in p, m, v, last_step; owner == INT_MAX after
every catch-up and step; last_step == t on exactly the listed rows; never-touched rows keep p through a catch-up (wd = 0);
gradients of the row-lazy cases are multiples of 2^k / 16 of magnitude <= 2^k, so a duplicated row's position-order sum is exact
in any order and a lost / doubled / misdirected occurrence moves m by far more than tol; multi-tensor == per-tensor kernel;
*_dev == host forms; presummed == in-kernel sum; fast-forward == catch-up where the exact replay is mandatory.

`draw_case(seed)` is deterministic in the seed; `test_cases_span_every_axis` asserts every axis value to occur;
`test_checker_rejects_planted_errors` shows that an fp32 restatement of each form passes and each planted error fails (CPU).
The row-lazy gap of 513 steps needs 540 optimizer steps: the one case above 300.
Each planted error of the row-lazy family runs on the cases chosen to catch it (LAZY_PLANT_CASES) and must fail on every one of
them.  On one MI355X the 73 device tests take 13 s (the slowest 1.5 s); the 4 CPU tests 24 s, 11 of them the float64 reference
of the two 4.2 M-element tensors that the grid-stride loop needs.
"""
import ctypes
import math

import numpy as np
import pytest
import torch

F32, F64 = np.float32, np.float64
U = 2.0 ** -24
FLOOR = 4 * 2.0 ** -126
E_ADAM = 17.4                                               # test_E_is_four_times_the_measured_worst
GUARD = 64
GUARD_VALUE = 12345
INT_MAX = 2 ** 31 - 1
MAX_IDS = 16000
BAD_ARG, UNSUPPORTED = 10001, 10002
GRID_CAP = 4096 * 256 * 4                                   # elements one pass of the capped grid covers

DENSE_N = (0, 1, 2, 3, 4, 5, 7, 1023, 1024, 1025, 4 * 256 * 3 + 1, GRID_CAP + 4 * 300 + 3)
STEPS_T = (1, 2, 10, 1000, 100000)
WDS = (0.0, 1e-2)
BETAS = ((0.9, 0.999), (0.95, 0.999), (0.5, 0.9))
EPSS = (1e-8, 1e-6)
LRS = (1e-4, 1e-3, 1e-2)
G_PATTERNS = ("dense", "rowsparse", "tiny", "large", "prefilled")
N_TENSORS = (0, 1, 23, 24, 25, 48, 49, 50)
SMALL_N = (1, 2, 3, 5, 7, 64, 1023, 1025, 4100)
LAZY_F = (4, 8, 1020, 1024, 1028, 4096, 4100, 8196)
LAZY_LENS = (1, 255, 256, 257, 16000, 16001)
LAZY_GAPS = (1, 12, 13, 31, 32, 33, 255, 256, 257, 513)
FF_GAPS = (12, 13, 100, 256, 257, 3000)
FF_S0 = (0, 50, 127, 128, 5000)
N_DENSE, N_MULTI, N_LAZY, N_FF = 26, 8, 10, 6
CASES = N_DENSE + N_MULTI + N_LAZY + N_FF                   # 50
DENSE_PLANTS = ("bc_t_minus_1", "eps_in_sqrt", "wd_on_m", "betas_swapped", "tail_skipped")
MULTI_PLANTS = ("skip_tensor_25", "lr_of_23_for_24")
LAZY_PLANTS = ("dup_dropped", "dup_twice", "lost_step", "stop_at_256", "second_tile_stale", "minus1_as_row0", "last_step_stuck")
# the row-lazy case(s) each planted error is run on (index into LAZY) -- and must fail on: duplicates and -1 ids in lists of
# 255 ... 257 and a 257-step replay (3), a second 4096-float tile (0), 16000-long lists of one id (5)
LAZY_PLANT_CASES = {3: ("dup_dropped", "dup_twice", "lost_step", "stop_at_256", "minus1_as_row0", "last_step_stuck"),
                    0: ("second_tile_stale", "lost_step", "last_step_stuck"), 5: ("dup_dropped", "dup_twice", "minus1_as_row0")}
LAZY_DEV_SEEDS = (N_DENSE + N_MULTI + 0, N_DENSE + N_MULTI + 3, N_DENSE + N_MULTI + 6)
LAZY_WRAPPER_SEEDS = (N_DENSE + N_MULTI + 3, N_DENSE + N_MULTI + 5)


def rnd(a, dt):
    """one fp32 rounding in the restatement (dt = F32); nothing in the reference"""
    a = np.asarray(a, F64)
    if dt is F32:
        with np.errstate(over="ignore", invalid="ignore", under="ignore"):
            return a.astype(F32).astype(F64)
    return a


def f32(x):
    return float(F32(x))


def hyper(lr, b1, b2, t):
    """the pair the header documents: double arithmetic on the fp32 constants, rounded to fp32"""
    b1, b2, lr = f32(b1), f32(b2), f32(lr)
    bc1, bc2 = 1.0 - b1 ** t, 1.0 - b2 ** t
    with np.errstate(all="ignore"):
        return float(F32(np.float64(lr) / np.float64(bc1))), float(F32(1.0 / np.sqrt(np.float64(bc2))))


# ------------------------------------------------------------------------------------------------ the formula and its bound
def adam_formula(p, g, m, v, A, B, hp, dt, plant=None):
    """one element-step on float64 arrays (dt = F32: every operation rounded to fp32, the stand-in for the kernels);
    returns p', m', v' and g (after weight decay), den, upd for the bound"""
    b1, b2, eps, wd = hp
    if plant == "betas_swapped":
        b1, b2 = b2, b1
    c1, c2 = 1.0 - b1, 1.0 - b2
    r = lambda x: rnd(x, dt)      # noqa: E731
    with np.errstate(all="ignore"):
        if wd != 0.0 and plant != "wd_on_m":
            g = r(wd * p + g)
        m2 = r(c1 * r(g - m) + m)
        if wd != 0.0 and plant == "wd_on_m":
            m2 = r(m2 + wd * p)
        v2 = r(c2 * r(g * g) + r(v * b2))
        arg = r(v2 + eps) if plant == "eps_in_sqrt" else v2
        root = np.sqrt(arg.astype(F32)).astype(F64) if dt is F32 else np.sqrt(arg)
        den = r(root * B) if plant == "eps_in_sqrt" else r(root * B + eps)
        upd = r(A * r(m2 * r(1.0 / den)))
        p2 = r(p - upd)
    return p2, m2, v2, g, den, upd


def half_ulp(x):
    with np.errstate(all="ignore"):
        return np.spacing(np.abs(np.asarray(x, F64)).astype(F32)).astype(F64) / 2


MEASURE_E = {"on": False, "worst": 0.0}                    # cpu_results: the restated update at every reference step


def _measure_update(m2, v2, A, B, eps, upd_unused=None):
    """worst |upd32 - upd64| / (u |upd64|) of the fp32 numpy restatement of the update at the fp32-rounded float64 moments"""
    m, v = rnd(m2, F32), rnd(v2, F32)
    r = lambda x: rnd(x, F32)      # noqa: E731
    with np.errstate(all="ignore"):
        u64 = A * (m / (np.sqrt(v) * B + eps))
        u32 = r(A * r(m * r(1.0 / r(np.sqrt(v.astype(F32)).astype(F64) * B + eps))))
        ok = np.isfinite(u64) & (np.abs(u64) > 1e-30) & np.isfinite(u32)
        if ok.any():
            MEASURE_E["worst"] = max(MEASURE_E["worst"], float((np.abs(u32 - u64)[ok] / (U * np.abs(u64[ok]))).max()))


class State:
    """p, m, v in float64 with their running bounds and the summed |update| per element"""

    def __init__(self, p, m, v):
        self.p, self.m, self.v = (np.array(x, F64) for x in (p, m, v))
        self.Ep, self.Em, self.Ev, self.acc = (np.zeros(self.p.shape) for _ in range(4))

    def step(self, g, A, B, hp, sel=None):
        """dense Adam step with gradient g (sel: only these rows take part -- the fast-forward cases' per-row start)"""
        b1, b2, eps, wd = hp
        c1, c2 = 1.0 - b1, 1.0 - b2
        p, m, v, Ep, Em, Ev = self.p, self.m, self.v, self.Ep, self.Em, self.Ev
        p2, m2, v2, gw, den, upd = adam_formula(p, g, m, v, A, B, hp, F64)
        if MEASURE_E["on"]:
            _measure_update(m2 if sel is None else m2[sel], v2 if sel is None else v2[sel], A, B, eps)
        with np.errstate(all="ignore"):
            Eg = wd * Ep + U * np.abs(gw) if wd != 0.0 else 0.0
            Em2 = b1 * Em + c1 * Eg + c1 * U * np.abs(gw - m) + U * np.abs(m2) + FLOOR
            Ev2 = b2 * Ev + 2 * c2 * np.abs(gw) * Eg + c2 * U * gw * gw + U * b2 * v + U * v2 + FLOOR
            s = np.sqrt(v2)
            lo = np.sqrt(np.maximum(v2 - Ev2, 0.0))
            dden = B * np.maximum(np.sqrt(v2 + Ev2) - s, s - lo)
            rel = dden / (lo * B + eps) + E_ADAM * U + np.where(v2 - Ev2 < 2.0 ** -126, 2.0 ** -63 * B / eps, 0.0)
            Eu = A * Em2 / (lo * B + eps) + np.abs(upd) * rel + FLOOR
            Ep2 = Ep + Eu + np.minimum(half_ulp(p2), np.abs(upd) + Eu)
            acc2 = self.acc + np.abs(upd)
        new = (p2, m2, v2, Ep2, Em2, Ev2, acc2)
        if sel is not None:
            old = (p, m, v, Ep, Em, Ev, self.acc)
            new = tuple(np.where(sel[:, None], a, b) for a, b in zip(new, old))
        self.p, self.m, self.v, self.Ep, self.Em, self.Ev, self.acc = new


# ------------------------------------------------------------------------------------------------ checks
def check_float(got, ref, tol, name):
    """|got - ref| <= tol where ref is finite, the same non-finite values elsewhere; returns the worst err / tol"""
    got, ref = np.asarray(got, F64), np.asarray(ref, F64)
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    tol = np.broadcast_to(np.asarray(tol, F64), ref.shape)
    fmax = float(np.finfo(F32).max)
    with np.errstate(invalid="ignore"):
        ref = np.where(np.abs(ref) > fmax, np.copysign(np.inf, ref), ref)
    fin = np.isfinite(ref)
    if not np.array_equal(np.isfinite(got), fin):
        i = tuple(int(x) for x in np.argwhere(np.isfinite(got) != fin)[0])
        raise AssertionError((name, "non-finite pattern", int((np.isfinite(got) != fin).sum()), "first at", i, float(got[i]),
                              float(ref[i])))
    same = (got == ref) | (np.isnan(got) & np.isnan(ref))
    if not same[~fin].all():
        raise AssertionError((name, "non-finite values differ", int((~fin & ~same).sum())))
    with np.errstate(invalid="ignore"):
        err = np.where(fin, np.abs(got - ref), 0.0)
        t = np.where(fin, tol, 1.0)
    assert not np.isnan(t).any() and (t >= 0).all(), (name, "tolerance undefined")
    viol = err > t
    if viol.any():
        i = tuple(int(x) for x in np.argwhere(viol)[0])
        raise AssertionError((name, "beyond tol", int(viol.sum()), "first at", i, "got", float(got[i]), "ref", float(ref[i]),
                              "err", float(err[i]), "tol", float(t[i])))
    pos = fin & (t > 0)
    return float((err[pos] / t[pos]).max()) if pos.any() else 0.0


def check_state(got, S, name, rows=None):
    """got = (p, m, v) against the reference state (on `rows`); the worst err / tol"""
    worst = 0.0
    for x, ref, tol, nm in zip(got, (S.p, S.m, S.v), (S.Ep, S.Em, S.Ev), "pmv"):
        if rows is not None:
            x, ref, tol = x[rows], ref[rows], tol[rows]
        worst = max(worst, check_float(x, ref, tol, name + " " + nm))
    return worst


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.int32)


def same_bits(a, b, name):
    a, b = bits(a), bits(b)
    assert a.shape == b.shape and np.array_equal(a, b), (name, "bits differ", int((a != b).sum()) if a.shape == b.shape else -1)


class Rep:
    """what one implementation did in a driver run: the worst err / tol, or the first failure"""

    def __init__(self):
        self.worst, self.err = 0.0, None

    def do(self, f, *a):
        if self.err is None:
            try:
                self.worst = max(self.worst, f(*a) or 0.0)
            except AssertionError as e:
                self.err = e


def sharp(Ss, name, moments=True):
    """the sharpness condition on a case's reference states, pooled (a tensor of 5 elements has no 90 % of its own)"""
    S = State(*[np.concatenate([getattr(x, k).ravel() for x in Ss] + [np.zeros(0)]) for k in "pmv"])
    S.Ep, S.Em, S.Ev, S.acc = (np.concatenate([getattr(x, k).ravel() for x in Ss] + [np.zeros(0)]) for k in ("Ep", "Em", "Ev", "acc"))
    with np.errstate(all="ignore"):
        moved = np.isfinite(S.p) & (S.acc > 0)
        if moved.any():
            ok = S.Ep[moved] <= 0.01 * S.acc[moved]
            assert ok.mean() >= 0.9, (name, "tol(p) not sharp", float(ok.mean()))
        for x, e, nm in ((S.m, S.Em, "m"), (S.v, S.Ev, "v")):
            big = np.isfinite(x) & (np.abs(x) > 1e-6)
            if moments and big.any():
                assert (e[big] <= 1e-4 * np.abs(x[big])).all(), (name, "tol(%s) not sharp" % nm, float((e[big] / np.abs(x[big])).max()))


# ------------------------------------------------------------------------------------------------ cases
class Case:
    def axes(self):
        keys = ("seed", "kind", "n", "t", "wd", "betas", "eps", "lr", "pattern", "nsteps", "nonfinite", "n_tensors", "R", "F", "T")
        return " ".join("%s=%s" % (k, getattr(self, k)) for k in keys if hasattr(self, k))

    @property
    def hp(self):
        return f32(self.betas[0]), f32(self.betas[1]), f32(self.eps), f32(self.wd)


def _fill(rng, n, pattern, prefilled, nsteps, wd=0.0):
    """p, m, v and nsteps gradients of one tensor; gradients have the sign of a pre-filled m, and under weight decay both have
    the sign of p (g + wd p and the lerp of m then add magnitudes: the update is not the remainder of a cancellation)"""
    p = rng.uniform(-4, 4, n).astype(F32)
    m, v = np.zeros(n, F32), np.zeros(n, F32)
    scale = None
    if prefilled or pattern == "prefilled":
        m = (rng.standard_normal(n) * 10.0 ** rng.uniform(-3, 0, n)).astype(F32)
        v = ((np.abs(m) * rng.uniform(0.5, 2, n)) ** 2).astype(F32)
        z = rng.random(n)
        if wd != 0.0:
            m = np.abs(m) * np.sign(p)
        scale = np.sqrt(v.astype(F64))
        m[z < 0.13], v[z < 0.1] = 0.0, 0.0                   # exact zeros: both moments, or the first alone
        scale[z < 0.1] = 0.0
    sign = np.where(m != 0, np.sign(m), np.sign(p) if wd != 0.0 else rng.choice([-1.0, 1.0], n))
    gs = []
    for _ in range(nsteps):
        mag = np.abs(rng.standard_normal(n)) * 10.0 ** rng.uniform(-3, 1, n) + 1e-4
        if scale is not None:                                # a gradient of the size of the moments it meets
            mag = np.where(scale > 0, scale * rng.uniform(0.3, 3, n), mag)
        if pattern == "tiny":
            mag = np.full(n, 1e-20)
        elif pattern == "large":
            mag = 1e18 * rng.uniform(0.5, 1.0, n)
        g = (sign * mag).astype(F32)
        if pattern == "rowsparse":
            g[np.repeat(rng.random(-(-n // 16)) < 0.7, 16)[:n]] = 0.0
        gs.append(g)
    if pattern == "tiny":                                    # (p = 0: an update of 1e-15 moves it; next to 4 it would vanish)
        p[:], m[:], v[:] = 0.0, 0.0, 0.0
    return p, m, v, gs


def _draw_dense(c, k, rng):
    c.kind = "dense"
    c.nonfinite = k >= 24
    c.n = n = (DENSE_N[k % 12] if k < 23 else 4099) if k < 24 else 1025
    c.t, c.wd, c.betas, c.eps = STEPS_T[k % 5], WDS[(k // 2) % 2], BETAS[k % 3], EPSS[(k // 3) % 2]
    c.lr, c.pattern = LRS[(k // 2) % 3], G_PATTERNS[(k // 5 + k) % 5] if k < 24 else "dense"
    c.nsteps = 1 if n > GRID_CAP else 1 + k % 4
    c.p, c.m, c.v, c.g = _fill(rng, n, c.pattern, c.t > 1, c.nsteps, c.wd)
    if c.nonfinite:
        c.nsteps = 2
        c.g = c.g[:1] * 2
        c.g = [x.copy() for x in c.g]
        c.g[0][[3, 500, 1024]] = (np.inf, -np.inf, np.nan) if k == 24 else (np.nan, np.inf, np.inf)


def _draw_multi(c, k, rng):
    c.kind = "multi"
    c.n_tensors = nt = N_TENSORS[k]
    c.wd, c.betas, c.eps = WDS[k % 2], BETAS[k % 3], EPSS[(k // 2) % 2]
    sizes = [int(SMALL_N[(i + k) % len(SMALL_N)]) for i in range(nt)]
    if nt >= 24 and k % 2 == 1:                              # zero-length entries: first, a middle and the last slot of a group
        sizes[0] = sizes[11] = sizes[23] = 0
    if nt >= 49:
        sizes[24:48] = [0] * 24                              # a whole group of zeros: no launch for it
    if nt == 25:
        sizes[24] = GRID_CAP + 4 * 256 + 5                   # above the per-tensor grid cap, among small ones
    c.sizes = sizes
    c.lr, c.t = LRS[k % 3], STEPS_T[(k + 1) % 5]             # the device form: one pair for every tensor
    c.lrs = [LRS[(i + k) % 3] for i in range(nt)]            # the host form: per tensor
    c.ts = [STEPS_T[(i + 2 * k) % 5] for i in range(nt)]
    if nt == 25:
        c.lrs[24], c.ts[24] = c.lr, c.t                      # (one reference serves both forms of the large tensor)
    c.tensors = [_fill(rng, n, G_PATTERNS[(i + k) % 5] if n <= 4100 else "dense", True, 1, c.wd) for i, n in enumerate(sizes)]


B0, B1, B2 = BETAS
LAZY = (
    dict(R=8, F=8196, T=20, lens=(1, 2, 3), pat="perm", gaps=(1, 12, 13), wd=0.0, lr=1e-3, betas=B0, eps=1e-8, single=True),
    dict(R=12, F=4100, T=40, lens=(1, 3), pat="perm", gaps=(31, 32, 33), wd=0.0, lr=1e-2, betas=B0, eps=1e-8),
    dict(R=10, F=4096, T=40, lens=(2, 4), pat="zipf", gaps=(12, 13, 32), wd=1e-2, lr=1e-3, betas=B2, eps=1e-6),
    dict(R=300, F=4, T=300, lens=(1, 255, 256, 257), pat="zipf", gaps=(255, 256, 257), wd=0.0, lr=1e-3, betas=B0, eps=1e-8),
    dict(R=40, F=8, T=540, lens=(1, 3, 17), pat="perm", gaps=(513,), wd=0.0, lr=1e-3, betas=B0, eps=1e-8, lr_change=200),
    dict(R=300, F=4, T=20, lens=(16000, 16001, 257, 1), pat="one", gaps=(1, 12), wd=1e-2, lr=1e-3, betas=B0, eps=1e-8),
    dict(R=64, F=1020, T=60, lens=(1, 17, 40), pat="perm", gaps=(1, 12, 13, 31, 32, 33), wd=1e-2, lr=1e-2, betas=B1, eps=1e-6),
    dict(R=32, F=1024, T=300, lens=(1, 5), pat="zipf", gaps=(255, 256, 257, 33), wd=0.0, lr=1e-4, betas=B0, eps=1e-8, settle=True),
    dict(R=20, F=1028, T=60, lens=(256, 257, 1), pat="one", gaps=(31, 32), wd=0.0, lr=1e-3, betas=B1, eps=1e-8),
    dict(R=100, F=8, T=24, lens=(255, 16000, 16001), pat="zipf", gaps=(13,), wd=0.0, lr=1e-2, betas=B2, eps=1e-6, lr_change=10),
)


def _draw_lazy(c, k, rng):
    c.kind = "lazy"
    for key, val in LAZY[k].items():
        setattr(c, key, val)
    R, F, T = c.R, c.F, c.T
    c.pattern = c.pat
    gap_rows = list(range(2, 2 + len(c.gaps)))               # row 0: only ever caught up; row 1: never named
    pool = np.arange(2 + len(c.gaps), R)
    events = {}
    c.gap_of = {}
    for i, n in enumerate(c.gaps):
        a = 1 + i % 3
        assert a + n + 1 <= T
        events.setdefault(a, []).append(gap_rows[i])
        events.setdefault(a + n + 1, []).append(gap_rows[i])
        c.gap_of[gap_rows[i]] = n
    c.single_row = gap_rows[1] if getattr(c, "single", False) else -1
    c.ids, c.g, c.extra, c.lrs = [None], [None], {}, [None]
    sgn = rng.choice([-1.0, 1.0], (R, F))
    c.gscale = gscale = 2.0 ** int(rng.integers(-6, 3))
    for t in range(1, T + 1):
        L = c.lens[t % len(c.lens)]
        if c.pat == "perm":
            ids = rng.permutation(pool)[:L]
        elif c.pat == "one":
            ids = np.full(L, pool[t % pool.size])
        else:
            ids = pool[(rng.zipf(1.3, L) - 1) % pool.size]
        ids = ids.astype(np.int64)
        forced = events.get(t, [])
        if L >= 8:
            hole = rng.choice(L, L // 16, replace=False)
            ids[hole] = -1                                   # "no row" mixed in
            if L >= 257:                                     # duplicates across a wave boundary and a pass boundary
                ids[63] = ids[64] = pool[0]
                ids[255] = ids[256] = pool[1]
            ids[1:1 + len(forced)] = forced
        elif forced:
            ids = np.concatenate([np.asarray(forced, np.int64), ids[:max(L - len(forced), 0)]])
        g = rng.integers(0, 17, (ids.size, F)) / 16.0 * gscale * sgn[ids]      # (one sign per element: m is no remainder of a cancellation)
        if c.single_row >= 0:                                # a tile with one non-zero moment element next to 4095 zeros
            occ = ids == c.single_row
            g[occ] = 0.0
            g[occ, 5000] = gscale
        c.ids.append(ids)
        c.g.append(g.astype(F32))
        if t % 7 == 3:                                       # a second catch-up of partly the same rows in the same step
            c.extra[t] = np.concatenate([ids[:max(ids.size // 2, 1)], [0, -1]]).astype(np.int64)
        change = getattr(c, "lr_change", None)
        c.lrs.append(c.lr if change is None or t < change else c.lr * 10 if c.lr < 1e-2 else c.lr / 10)
    p = rng.uniform(1, 4, (R, F))                            # (under weight decay p walks lr per step: it must not reach 0)
    if getattr(c, "settle", False):                          # |p| in [2, 4) settles at lr = 1e-4; p = 0 / 1e-6 keep moving
        p = rng.uniform(2, 3.9, (R, F))
        p[:, 300] = 0.0                                      # one mover inside wave 1 (columns 256 ... 511)
        p[:, 512:768] = 1e-6                                 # wave 2 moves as a whole; waves 0 and 3 settle
    c.p = (np.abs(p) * sgn).astype(F32)                      # (weight decay: g + wd p adds magnitudes)


def _draw_ff(c, k, rng):
    c.kind = "ff"
    c.F = F = 64
    spec = ((13, (13, 12), 0.0, B0), (150, (100, 23, 22, 12, 13, 150), 0.0, B0), (5300, (300, 257, 256, 100, 13, 12, 3000), 0.0, B0),
            (3128, (3000, 3001, 3078, 3128), 0.0, B0), (400, (100, 256, 257, 13), 0.0, B1), (400, (100, 256, 13, 12), 1e-2, B0))[k]
    c.t_now, gaps, c.wd, c.betas = spec
    c.eps, c.lr = 1e-8, 1e-3
    c.gaps = gaps
    c.s0 = np.array([c.t_now - g for g in gaps], np.int32)
    c.R = R = len(gaps)
    root = f32(c.eps) * 10.0 ** rng.uniform(-6, 6, (R, F))   # sqrt(v) from 1e-6 eps to 1e6 eps
    c.v = (root ** 2).astype(F32)
    c.m = (root * rng.uniform(0.3, 3, (R, F)) * rng.choice([-1.0, 1.0], (R, F))).astype(F32)
    c.m[rng.random((R, F)) < 0.1] = 0.0
    # p of the size of the distance it will move (about 10 lr |m| / (sqrt(v) + eps), from a tenth to thirty times that): next to
    # |p| ~ 1 every update of an element with sqrt(v) << eps is below half an ulp and tol(p) would be the whole distance.
    # Under weight decay p feeds back (g = wd p): |p| in [1, 4) of m's sign, as in the row-lazy cases
    dist = np.where(c.m != 0, 10 * c.lr * np.abs(c.m.astype(F64)) / (np.sqrt(c.v.astype(F64)) + f32(c.eps)), c.lr)
    sgn = np.where(c.m != 0, np.sign(c.m), rng.choice([-1.0, 1.0], (R, F)))
    if c.wd != 0.0:
        c.p = (sgn * rng.uniform(1, 4, (R, F))).astype(F32)
    else:
        c.p = np.clip(rng.choice([-1.0, 1.0], (R, F)) * dist * 10.0 ** rng.uniform(-1, 1.5, (R, F)), -4, 4).astype(F32)
        c.p[rng.random((R, F)) < 0.05] = 0.0
    c.ids = rng.permutation(R).astype(np.int64)


def ff_may_be_closed_form(c, s0):
    """the conditions of csrc/adam.hip under which a row MAY leave the exact replay (its series test R <= 1e-7 W aside)"""
    s_fast = max(int(s0), min(c.t_now, 128))
    n = c.t_now - s_fast
    return c.wd == 0.0 and n > 12 and (n <= 256 or f32(c.betas[0]) ** 256 < 1e-9), s_fast


_CASES = {}


def draw_case(seed):
    if seed in _CASES:
        return _CASES[seed]
    rng = np.random.default_rng(7000 + seed)
    c = Case()
    c.seed = seed
    if seed < N_DENSE:
        _draw_dense(c, seed, rng)
    elif seed < N_DENSE + N_MULTI:
        _draw_multi(c, seed - N_DENSE, rng)
    elif seed < N_DENSE + N_MULTI + N_LAZY:
        _draw_lazy(c, seed - N_DENSE - N_MULTI, rng)
    else:
        _draw_ff(c, seed - N_DENSE - N_MULTI - N_LAZY, rng)
    _CASES[seed] = c
    return c


# ------------------------------------------------------------------------------------------------ drivers
def run_dense(c, impls):
    """impls: name -> object with dense_step(c, k) -> (p, m, v); returns the reports and the reference state"""
    S = State(c.p, c.m, c.v)
    reps = {name: Rep() for name in impls}
    for k in range(c.nsteps):
        A, B = hyper(c.lr, c.betas[0], c.betas[1], c.t + k)
        S.step(c.g[k].astype(F64), A, B, c.hp)
        for name, im in impls.items():
            reps[name].do(lambda: check_state(im.dense_step(c, k), S, "%s step %d %s" % (name, k, c.axes())))
    return reps, S


def run_multi(c, impls, dev):
    """impls: name -> object with multi_step(c, dev) -> list of (p, m, v)"""
    refs = []
    memo = c.__dict__.setdefault("_refs", {})                # (a tensor with the same lr and step in both forms: one reference)
    for i, (p, m, v, gs) in enumerate(c.tensors):
        key = (i,) + ((c.lr, c.t) if dev else (c.lrs[i], c.ts[i]))
        if key not in memo:
            memo[key] = S = State(p, m, v)
            A, B = hyper(key[1], c.betas[0], c.betas[1], key[2])
            S.step(gs[0].astype(F64), A, B, c.hp)
        refs.append(memo[key])
    reps = {name: Rep() for name in impls}
    for name, im in impls.items():
        def one(im=im, name=name):
            got = im.multi_step(c, dev)
            return max([check_state(got[i], refs[i], "%s tensor %d %s" % (name, i, c.axes())) for i in range(c.n_tensors)] + [0.0])
        reps[name].do(one)
    return reps, refs


def _bookkeeping(before, after, rows, t, name, stepped):
    """exact checks around one catch-up (stepped False) or step call: snapshots are (p, m, v, last_step, owner)"""
    un = np.setdiff1d(np.arange(after[0].shape[0]), rows)
    for a, b, nm in zip(before[:3], after[:3], "pmv"):
        same_bits(a[un], b[un], name + " unlisted rows of " + nm)
    assert np.array_equal(before[3][un], after[3][un]), (name, "last_step of an unlisted row changed")
    assert (after[4] == INT_MAX).all(), (name, "owner marks left", int((after[4] != INT_MAX).sum()))
    want = np.maximum(before[3][rows], t) if not stepped else np.full(rows.size, t)
    assert np.array_equal(after[3][rows], want), (name, "last_step of the listed rows", after[3][rows][:8], t)
    return 0.0


def run_lazy(c, impls, fast=()):
    """impls: name -> object with start(c), catchup(ids, t_now), step(ids, g, t, lr), flush(t), read() -> (p, m, v, last_step,
    owner); names in `fast` use the closed form: their tolerance is the widened one.  Returns reports and the reference."""
    R, F = c.p.shape
    S = State(c.p, np.zeros((R, F)), np.zeros((R, F)))
    X = {nm: np.zeros((R, F)) for nm in ("p", "m", "v")}     # the closed form's allowance, carried next to the float bound
    acc_at = np.zeros((R, F))                                # summed |update| at each row's last visit
    relX = np.zeros((R, 1))                                  # ... and of the moments, relative: it reaches every later update
    last = np.zeros(R, np.int64)
    reps = {name: Rep() for name in impls}
    for im in impls.values():
        im.start(c)
    hp = c.hp

    def widen(rows, t_now):
        for r in rows:
            n = t_now - max(int(last[r]), min(t_now, 128))
            if hp[3] == 0.0 and n > 12 and (n <= 256 or hp[0] ** 256 < 1e-9):
                X["p"][r] += 2e-6 * (S.acc[r] - acc_at[r])
                X["m"][r] += 1e-6 * math.sqrt(n) * np.abs(S.m[r])
                X["v"][r] += 1e-6 * math.sqrt(n) * np.abs(S.v[r])
                relX[r] += 1.5e-6 * math.sqrt(n)

    def visited(rows, t):
        last[rows] = np.maximum(last[rows], t)
        acc_at[rows] = S.acc[rows]

    def compare(name, got, rows):
        if name not in fast:
            return check_state(got, S, name, rows)
        worst = 0.0
        for x, ref, tol, nm in zip(got, (S.p, S.m, S.v), (S.Ep, S.Em, S.Ev), "pmv"):
            worst = max(worst, check_float(x[rows], ref[rows], tol[rows] + X[nm][rows], name + " " + nm))
        return worst

    def call(name, im, what, ids, t, *args):
        rows = np.unique(ids[ids >= 0]) if ids is not None else np.arange(R)
        before = im.read()
        never = rows[(before[1][rows] == 0).all(1) & (before[2][rows] == 0).all(1)] if hp[3] == 0.0 and what != "step" else rows[:0]
        getattr(im, what)(*args)
        after = im.read()
        tag = "%s %s t=%d %s" % (name, what, t, c.axes())
        _bookkeeping(before, after, rows, t, tag, what == "step")
        same_bits(before[0][never], after[0][never], tag + " never-touched rows")
        return compare(tag, after[:3], rows)

    for t in range(1, c.T + 1):
        ids, g, lr = c.ids[t], c.g[t], c.lrs[t]
        for lst in [ids] + ([c.extra[t]] if t in c.extra else []):
            rows = np.unique(lst[lst >= 0])
            widen(rows, t - 1)
            for name, im in impls.items():
                reps[name].do(call, name, im, "catchup", lst, t - 1, lst, t - 1)
            visited(rows, t - 1)
        G = np.zeros((R, F))
        np.add.at(G, ids[ids >= 0], g[ids >= 0].astype(F64))
        A, B = hyper(lr, c.betas[0], c.betas[1], t)
        acc_before = S.acc
        S.step(G, A, B, hp)
        X["p"] += relX * (S.acc - acc_before)
        for name, im in impls.items():
            reps[name].do(call, name, im, "step", ids, t, ids, g, t, lr)
        visited(np.unique(ids[ids >= 0]), t)
    widen(np.arange(R), c.T)
    for name, im in impls.items():
        reps[name].do(call, name, im, "flush", None, c.T, c.T)
    return reps, S


def run_ff(c, impls, fast=()):
    """impls: name -> object with ff(c) -> (p, m, v, last_step) after the catch-up of every row to c.t_now"""
    S = State(c.p, c.m, c.v)
    hp = c.hp
    elig = [ff_may_be_closed_form(c, s) for s in c.s0]
    acc0 = np.zeros(c.p.shape)
    for j in range(int(c.s0.min()) + 1, c.t_now + 1):
        for r, (ok, s_fast) in enumerate(elig):
            if j == s_fast + 1:
                acc0[r] = S.acc[r]
        A, B = hyper(c.lr, c.betas[0], c.betas[1], j)
        S.step(np.zeros(c.p.shape), A, B, hp, sel=c.s0 < j)
    X = {nm: np.zeros(c.p.shape) for nm in "pmv"}
    for r, (ok, s_fast) in enumerate(elig):
        if ok:
            n = c.t_now - s_fast
            X["p"][r] = 2e-6 * (S.acc[r] - acc0[r])
            X["m"][r], X["v"][r] = 1e-6 * math.sqrt(n) * np.abs(S.m[r]), 1e-6 * math.sqrt(n) * np.abs(S.v[r])
    reps = {name: Rep() for name in impls}
    outs = {}
    for name, im in impls.items():
        def one(im=im, name=name):
            got = outs[name] = im.ff(c)
            assert (got[3] == c.t_now).all(), (name, "last_step", got[3])
            worst = 0.0
            for x, ref, tol, nm in zip(got, (S.p, S.m, S.v), (S.Ep, S.Em, S.Ev), "pmv"):
                worst = max(worst, check_float(x, ref, tol + (X[nm] if name in fast else 0.0), "%s %s %s" % (name, nm, c.axes())))
            return worst
        reps[name].do(one)
    return reps, S, outs, [ok for ok, _ in elig]


# ------------------------------------------------------------------------------------------------ the fp32 restatement
class Restated:
    """every form in fp32 numpy (values held as float64), optionally with one planted error"""

    def __init__(self, plant=None):
        self.plant = plant
        self.dense = None

    def _one(self, p, g, m, v, lr, t, c, plant=None):
        hp = c.hp
        b1, b2 = c.betas
        if plant == "bc_t_minus_1":
            t = t - 1
        with np.errstate(all="ignore"):
            A, B = hyper(lr, b1, b2, t) if t >= 1 else (np.inf, np.inf)
        p2, m2, v2 = adam_formula(p, g, m, v, A, B, hp, F32, plant)[:3]
        if plant == "tail_skipped" and p.size & 3:
            k = p.size - (p.size & 3)
            p2[k:], m2[k:], v2[k:] = p[k:], m[k:], v[k:]
        return p2, m2, v2

    def dense_step(self, c, k):
        if k == 0:
            self.dense = tuple(x.astype(F64) for x in (c.p, c.m, c.v))
        p, m, v = self.dense
        self.dense = self._one(p, c.g[k].astype(F64), m, v, c.lr, c.t + k, c, self.plant)
        return self.dense

    def multi_step(self, c, dev):
        out = []
        for i, (p, m, v, gs) in enumerate(c.tensors):
            lr, t = (c.lr, c.t) if dev else (c.lrs[i], c.ts[i])
            if self.plant == "lr_of_23_for_24" and i == 24 and not dev:
                lr = c.lrs[23]
            if self.plant == "skip_tensor_25" and i == 24:
                out.append(tuple(x.astype(F64) for x in (p, m, v)))
                continue
            out.append(self._one(p.astype(F64), gs[0].astype(F64), m.astype(F64), v.astype(F64), lr, t, c))
        return out

    # ---- row-lazy
    def start(self, c):
        self.c = c
        R, F = c.p.shape
        self.p, self.m, self.v = c.p.astype(F64), np.zeros((R, F)), np.zeros((R, F))
        self.last, self.hist = np.zeros(R, np.int64), {}

    def read(self):
        return self.p.copy(), self.m.copy(), self.v.copy(), self.last.copy(), np.full(self.last.size, INT_MAX, np.int64)

    def catchup(self, ids, t_now):
        c, pl = self.c, self.plant
        if ids is None:
            rows = np.arange(self.p.shape[0])
        else:
            ids = np.where(ids < 0, 0, ids) if pl == "minus1_as_row0" else ids
            rows = np.unique(ids[ids >= 0])
        rows = rows[self.last[rows] < t_now]
        if rows.size == 0:
            return
        s0 = self.last[rows].copy()
        cols = slice(0, 4096) if pl == "second_tile_stale" else slice(None)
        for j in range(int(s0.min()) + 1, t_now + 1):
            act = s0 < j
            if pl == "lost_step":
                act &= ~((j == t_now) & (t_now - s0 >= 2))
            if pl == "stop_at_256":
                act &= j <= s0 + 256
            r = rows[act]
            if r.size:
                A, B = self.hist[j]
                self.p[r, cols], self.m[r, cols], self.v[r, cols] = adam_formula(
                    self.p[r, cols], 0.0, self.m[r, cols], self.v[r, cols], A, B, c.hp, F32)[:3]
        self.last[rows] = t_now

    def flush(self, t):
        self.catchup(None, t)

    def step(self, ids, g, t, lr):
        c, pl = self.c, self.plant
        self.hist[t] = hyper(lr, c.betas[0], c.betas[1], t)
        ids = np.where(ids < 0, 0, ids) if pl == "minus1_as_row0" else ids
        keep = ids >= 0
        G = np.zeros(self.p.shape)
        np.add.at(G, ids[keep], g[keep].astype(F64))
        if pl in ("dup_dropped", "dup_twice"):
            u, first, cnt = np.unique(ids[keep], return_index=True, return_counts=True)
            if (cnt > 1).any():
                row = u[cnt > 1][0]
                lastocc = np.flatnonzero(ids == row)[-1]
                G[row] += g[lastocc].astype(F64) * (1.0 if pl == "dup_twice" else -1.0)
        rows = np.unique(ids[keep])
        A, B = self.hist[t]
        self.p[rows], self.m[rows], self.v[rows] = adam_formula(self.p[rows], rnd(G[rows], F32), self.m[rows], self.v[rows], A, B, c.hp, F32)[:3]
        if pl != "last_step_stuck":
            self.last[rows] = t

    def ff(self, c):
        p, m, v = (x.astype(F64) for x in (c.p, c.m, c.v))
        for j in range(int(c.s0.min()) + 1, c.t_now + 1):
            A, B = hyper(c.lr, c.betas[0], c.betas[1], j)
            new = adam_formula(p, 0.0, m, v, A, B, c.hp, F32)[:3]
            sel = (c.s0 < j)[:, None]
            p, m, v = (np.where(sel, a, b) for a, b in zip(new, (p, m, v)))
        return p, m, v, np.full(c.R, c.t_now)


_CPU = {}


def cpu_results(seed):
    """one pass of the reference per case with the restatement and every planted error of its family: shared by the CPU tests"""
    if seed in _CPU:
        return _CPU[seed]
    c = draw_case(seed)
    out = {}
    MEASURE_E["on"] = True
    try:
        out = _cpu_results(c, seed)
    finally:
        MEASURE_E["on"] = False
    _CPU[seed] = out
    return out


def _cpu_results(c, seed):
    if c.kind == "dense":
        plants = DENSE_PLANTS if c.n <= 5000 else ()
        impls = {"restated": Restated()}
        impls.update({pl: Restated(pl) for pl in plants})
        reps, S = run_dense(c, impls)
        out = dict(reps=reps, states=[S])
    elif c.kind == "multi":
        impls = {"restated": Restated()}
        impls.update({pl: Restated(pl) for pl in MULTI_PLANTS})
        reps, refs = run_multi(c, impls, dev=False)
        reps["restated_dev"] = run_multi(c, {"restated": Restated()}, dev=True)[0]["restated"]
        out = dict(reps=reps, states=refs)
    elif c.kind == "lazy":
        impls = {"restated": Restated()}
        impls.update({pl: Restated(pl) for pl in LAZY_PLANT_CASES.get(seed - N_DENSE - N_MULTI, ())})
        reps, S = run_lazy(c, impls)
        out = dict(reps=reps, states=[S])
    else:
        reps, S, _, elig = run_ff(c, {"restated": Restated()})
        out = dict(reps=reps, states=[S], elig=elig)
    return out


# ------------------------------------------------------------------------------------------------ CPU self-tests
def test_E_is_four_times_the_measured_worst():
    for seed in range(CASES):                                # (the measurement runs inside every step of every reference)
        cpu_results(seed)
    worst = MEASURE_E["worst"]
    print("measured worst, in u |update|: %.3f" % worst)
    assert 1.0 <= worst <= 6.0, worst                        # six roundings of at most u (relative) each
    assert max(4.0 * worst, 4.0) + 2.0 <= E_ADAM <= max(4.0 * worst, 4.0) + 2.0 + 0.5, (worst, E_ADAM)


def c_kind(seed):
    return draw_case(seed).kind


def test_checker_rejects_planted_errors():
    caught = {pl: [] for pl in DENSE_PLANTS + MULTI_PLANTS + LAZY_PLANTS}
    for seed in range(CASES):
        res = cpu_results(seed)
        for name, rep in res["reps"].items():
            if name.startswith("restated"):
                assert rep.err is None, (seed, name, rep.err)
                assert rep.worst <= 1.0
            elif rep.err is not None:
                caught[name].append(seed)
            else:
                assert c_kind(seed) != "lazy", (seed, name, "a row-lazy planted error passes a case chosen to catch it")
    for pl, seeds in caught.items():
        assert seeds, (pl, "passes every case")
    c = draw_case(N_DENSE + 4)                               # multi-tensor, 25 tensors: both table errors are caught THERE
    assert c.n_tensors == 25 and N_DENSE + 4 in caught["skip_tensor_25"] and N_DENSE + 4 in caught["lr_of_23_for_24"]
    # a lost or doubled duplicate is caught through m (dyadic gradients: the position-order sum is exact)
    for pl in ("dup_dropped", "dup_twice"):
        assert all(" step t=" in str(cpu_results(s)["reps"][pl].err) for s in caught[pl])
    print({pl: len(s) for pl, s in caught.items()})


def test_tolerances_stay_sharp():
    bad = []
    for seed in range(CASES):
        c = draw_case(seed)
        # a replay of n steps rounds v n times: n u = 1.8e-4 at n = 3000, beyond 1e-4 whatever the inputs -- the two fast-forward
        # cases with such gaps are held to the p condition alone
        try:
            sharp(cpu_results(seed)["states"], c.axes(), moments=c.kind != "ff" or max(c.gaps) <= 1000)
        except AssertionError as e:
            bad.append(e.args[0])
    assert not bad, bad


def test_cases_span_every_axis():
    seen = {k: set() for k in ("n", "t", "wd", "betas", "eps", "lr", "pattern", "nsteps", "nt", "zero_slots", "zero_group", "small",
                               "R", "F", "T", "len", "lpat", "gap", "lwd", "ffgap", "s0", "nonfinite")}
    for seed in range(CASES):
        c = draw_case(seed)
        assert c.axes() == draw_case(seed).axes()
        if c.kind == "dense":
            for k in ("n", "t", "wd", "betas", "eps", "lr", "pattern", "nsteps", "nonfinite"):
                seen[k].add(getattr(c, k))
            if c.pattern == "prefilled" and c.n >= 64:
                assert (c.m == 0).any() and (c.v == 0).any() and (c.m != 0).any()
            assert all(np.abs(g[np.isfinite(g)]).max(initial=0) <= 1e18 for g in c.g) and np.abs(c.p).max(initial=0) <= 4
        elif c.kind == "multi":
            seen["nt"].add(c.n_tensors)
            z = [i for i, n in enumerate(c.sizes) if n == 0]
            seen["zero_slots"].add({0, 11, 23} <= set(z))
            seen["zero_group"].add(set(range(24, 48)) <= set(z))
            seen["small"] |= {("lt4", any(0 < n < 4 for n in c.sizes)), ("tail", any(n & 3 for n in c.sizes)),
                              ("above_cap", any(n > GRID_CAP for n in c.sizes))}
            if c.n_tensors > 1:
                assert len(set(c.lrs)) > 1 and len(set(c.ts)) > 1
        elif c.kind == "lazy":
            seen["R"].add(c.R), seen["F"].add(c.F), seen["T"].add(c.T), seen["lpat"].add(c.pat), seen["lwd"].add(c.wd)
            seen["gap"] |= set(c.gaps)
            seen["lr"].add(c.lr)
            assert c.extra and all(0 in c.extra[t] and c.extra[t][0] == c.ids[t][0] for t in c.extra)      # the second catch-up
            for t in range(1, c.T + 1):
                ids = c.ids[t]
                seen["len"].add(ids.size)
                assert ((ids >= -1) & (ids < c.R)).all() and 1 not in ids
                if ids.size >= 257:
                    assert ids[63] == ids[64] >= 0 and ids[255] == ids[256] >= 0 and (ids == -1).any()
                q = c.g[t].astype(F64) * 16 / c.gscale
                assert (q == np.round(q)).all() and np.abs(q).max() <= 16 and (q != 0).any()
        else:
            seen["ffgap"] |= set(c.gaps)
            seen["s0"] |= set(int(s) for s in c.s0)
            root = np.sqrt(c.v.astype(F64)) / 1e-8
            assert root.min() < 1e-5 and root.max() > 1e5 and (c.m == 0).any() and (c.m > 0).any() and (c.m < 0).any()
    assert seen["n"] >= set(DENSE_N) and seen["t"] == set(STEPS_T) and seen["wd"] == set(WDS) and seen["betas"] == set(BETAS)
    assert seen["eps"] == set(EPSS) and seen["lr"] >= set(LRS) and seen["pattern"] == set(G_PATTERNS) and seen["nsteps"] == {1, 2, 3, 4}
    assert seen["nonfinite"] == {True, False}
    assert seen["nt"] == set(N_TENSORS) and seen["zero_slots"] == {True, False} and seen["zero_group"] == {True, False}
    assert seen["small"] >= {("lt4", True), ("tail", True), ("above_cap", True)}
    assert min(seen["R"]) == 8 and max(seen["R"]) == 300 and seen["F"] == set(LAZY_F) and min(seen["T"]) == 20 and 300 in seen["T"]
    assert seen["len"] >= set(LAZY_LENS) and seen["lpat"] == {"perm", "one", "zipf"} and seen["gap"] == set(LAZY_GAPS)
    assert seen["lwd"] == set(WDS) and seen["ffgap"] >= set(FF_GAPS) and seen["s0"] >= set(FF_S0)
    assert any(hasattr(draw_case(s), "lr_change") for s in range(CASES)) and any(getattr(draw_case(s), "settle", False) for s in range(CASES))
    assert any(getattr(draw_case(s), "single_row", -1) >= 0 for s in range(CASES))


# ------------------------------------------------------------------------------------------------ GPU plumbing
def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def P(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def PA(ts):
    return (ctypes.c_void_p * len(ts))(*[None if t is None else t.data_ptr() for t in ts])


def _lib():
    from mmrec_amd import _lib as L, hip_ops
    return L.load(), hip_ops._stream()


def _ok(rc, what):
    assert rc == 0, (what, rc)


class Guarded:
    """an array inside one tensor with GUARD sentinel elements on either side, handed over by offset pointer (GUARD elements of
    4 bytes keep the 16-byte alignment)"""

    def __init__(self, init, dtype=torch.float32):
        init = np.ascontiguousarray(init)
        self.shape, self.n = init.shape, init.size
        self.buf = torch.full((self.n + 2 * GUARD,), GUARD_VALUE, dtype=dtype, device="cuda:0")
        self.view = self.buf[GUARD:GUARD + self.n]
        if self.n:
            self.view.copy_(_dev(init.ravel()).to(dtype))

    def get(self, name=""):
        b = self.buf.cpu().numpy()
        assert (b[:GUARD] == GUARD_VALUE).all() and (b[GUARD + self.n:] == GUARD_VALUE).all(), (name, "guard elements overwritten")
        return b[GUARD:GUARD + self.n].reshape(self.shape).copy()


class Tensor3:
    """p, m, v of one tensor, guarded"""

    def __init__(self, p, m, v):
        self.p, self.m, self.v = Guarded(p), Guarded(m), Guarded(v)

    def get(self, name=""):
        return tuple(x.get(name).astype(F64) for x in (self.p, self.m, self.v))

    def ptrs(self):
        return P(self.p.view), P(self.m.view), P(self.v.view)


class DevScalars:
    """the device scalars of the *_dev forms: step (int64), lr, the hyper pair, the overflow flag"""

    def __init__(self, steps_taken, lr):
        self.step = torch.full((1,), int(steps_taken), dtype=torch.int64, device="cuda:0")
        self.lr = torch.full((1,), float(lr), dtype=torch.float32, device="cuda:0")
        self.hyper = torch.zeros(2, dtype=torch.float32, device="cuda:0")
        self.overflow = torch.zeros(1, dtype=torch.int32, device="cuda:0")

    def prepare(self, lib, s, c, lr=None):
        if lr is not None:
            self.lr.fill_(float(lr))
        _ok(lib.mmrec_adam_prepare(P(self.step), P(self.lr), c.hp[0], c.hp[1], P(self.hyper), s), "prepare")


class GpuDense:
    def __init__(self, dev):
        self.dev = dev

    def dense_step(self, c, k):
        lib, s = _lib()
        b1, b2, eps, wd = c.hp
        if k == 0:
            self.T = Tensor3(c.p, c.m, c.v)
            self.sc = DevScalars(c.t - 1, c.lr)
        g = _dev(c.g[k]) if c.n else None
        pp, pm, pv = self.T.ptrs()
        if self.dev:
            self.sc.prepare(lib, s, c)
            _ok(lib.mmrec_adam_step_dev_f32(pp, P(g), pm, pv, c.n, P(self.sc.hyper), b1, b2, eps, wd, s), "step_dev")
        else:
            _ok(lib.mmrec_adam_step_f32(pp, P(g), pm, pv, c.n, f32(c.lr), b1, b2, eps, wd, c.t + k, s), "step")
        torch.cuda.synchronize()
        return self.T.get(c.axes())


class GpuMulti:
    def __init__(self, per_tensor=False):
        self.per_tensor = per_tensor

    def multi_step(self, c, dev):
        lib, s = _lib()
        b1, b2, eps, wd = c.hp
        nt = c.n_tensors
        Ts = [Tensor3(p, m, v) for p, m, v, _ in c.tensors]
        gs = [_dev(t[3][0]) if t[0].size else None for t in c.tensors]
        sc = DevScalars(c.t - 1, c.lr)
        if dev:
            sc.prepare(lib, s, c)
        if self.per_tensor:
            for i, T in enumerate(Ts):
                pp, pm, pv = T.ptrs()
                if dev:
                    _ok(lib.mmrec_adam_step_dev_f32(pp, P(gs[i]), pm, pv, c.sizes[i], P(sc.hyper), b1, b2, eps, wd, s), "step_dev")
                else:
                    _ok(lib.mmrec_adam_step_f32(pp, P(gs[i]), pm, pv, c.sizes[i], f32(c.lrs[i]), b1, b2, eps, wd, c.ts[i], s), "step")
        else:
            arr = lambda xs: PA(xs) if nt else None      # noqa: E731
            pp, gg = arr([T.p.view for T in Ts]), arr(gs)
            mm, vv = arr([T.m.view for T in Ts]), arr([T.v.view for T in Ts])
            nn_ = (ctypes.c_int64 * max(nt, 1))(*c.sizes)
            if dev:
                _ok(lib.mmrec_adam_multi_step_dev_f32(pp, gg, mm, vv, nn_, nt, P(sc.hyper), b1, b2, eps, wd, s), "multi_dev")
            else:
                lrs = (ctypes.c_float * max(nt, 1))(*c.lrs)
                ts = (ctypes.c_int64 * max(nt, 1))(*c.ts)
                _ok(lib.mmrec_adam_multi_step_f32(pp, gg, mm, vv, nn_, nt, lrs, ts, b1, b2, eps, wd, s), "multi")
        torch.cuda.synchronize()
        return [T.get("%s tensor %d" % (c.axes(), i)) for i, T in enumerate(Ts)]


def presum(ids, g):
    """what `presummed` expects: slot of a row's FIRST occurrence holds the row's summed gradient (float64 sum: exact here)"""
    out = np.zeros(g.shape, F64)
    first = {}
    for i, r in enumerate(ids.tolist()):
        if r >= 0:
            out[first.setdefault(r, i)] += g[i]
    return out.astype(F32)


class GpuLazy:
    def __init__(self, dev=False, fast=False, presummed_always=False):
        self.dev, self.fast, self.presummed_always = dev, fast, presummed_always

    def start(self, c, m=None, v=None, last=None, capacity=None, steps_taken=0):
        self.c = c
        R, F = c.p.shape
        z = np.zeros((R, F), F32)
        self.T = Tensor3(c.p, z if m is None else m, z if v is None else v)
        self.last = Guarded(np.zeros(R, np.int32) if last is None else last, torch.int32)
        self.owner = Guarded(np.full(R, INT_MAX, np.int32), torch.int32)
        self.capacity = capacity if capacity is not None else c.T + 2
        self.hist = Guarded(np.zeros((self.capacity, 2), F32))
        self.sc = DevScalars(steps_taken, c.lrs[1] if hasattr(c, "lrs") else c.lr)

    def read(self):
        torch.cuda.synchronize()
        tag = self.c.axes()
        self.hist.get(tag)
        return self.T.get(tag) + (self.last.get(tag).astype(np.int64), self.owner.get(tag).astype(np.int64))

    def catchup(self, ids, t_now):
        lib, s = _lib()
        c = self.c
        b1, b2, eps, wd = c.hp
        R, F = c.p.shape
        pp, pm, pv = self.T.ptrs()
        d = None if ids is None else _dev(ids)
        n = 0 if ids is None else ids.size
        if ids is not None:
            _ok(lib.mmrec_adam_rows_owner(P(d), n, P(self.owner.view), s), "owner")
        own = None if ids is None else P(self.owner.view)
        if self.dev:
            fn = lib.mmrec_adam_rows_fastforward_dev_f32 if self.fast else lib.mmrec_adam_rows_catchup_dev_f32
            _ok(fn(pp, pm, pv, P(d), own, n, R, F, P(self.last.view), P(self.hist.view), self.capacity, P(self.sc.step), b1, b2, eps,
                   wd, s), "catchup_dev")
        else:
            fn = lib.mmrec_adam_rows_fastforward_f32 if self.fast else lib.mmrec_adam_rows_catchup_f32
            _ok(fn(pp, pm, pv, P(d), own, n, R, F, P(self.last.view), P(self.hist.view), t_now, b1, b2, eps, wd, s), "catchup")

    def flush(self, t):
        self.catchup(None, t)

    def step(self, ids, g, t, lr):
        lib, s = _lib()
        c = self.c
        b1, b2, eps, wd = c.hp
        F = c.p.shape[1]
        pp, pm, pv = self.T.ptrs()
        d = _dev(ids)
        n = ids.size
        pre = n > MAX_IDS or self.presummed_always
        gd = _dev(presum(ids, g) if pre else g)
        if self.dev:
            self.sc.prepare(lib, s, c, lr)
            _ok(lib.mmrec_adam_hist_set_dev(P(self.hist.view), self.capacity, P(self.sc.step), P(self.sc.hyper), P(self.sc.overflow), s),
                "hist_set_dev")
        else:
            _ok(lib.mmrec_adam_hist_set(P(self.hist.view), t, f32(lr), b1, b2, s), "hist_set")
        _ok(lib.mmrec_adam_rows_owner(P(d), n, P(self.owner.view), s), "owner")
        if self.dev:
            _ok(lib.mmrec_adam_rows_step_dev_f32(pp, pm, pv, P(d), P(self.owner.view), P(gd), n, F, P(self.last.view), self.capacity,
                                                 P(self.sc.step), P(self.sc.hyper), b1, b2, eps, wd, int(pre), s), "rows_step_dev")
        else:
            _ok(lib.mmrec_adam_rows_step_f32(pp, pm, pv, P(d), P(self.owner.view), P(gd), n, F, P(self.last.view), t, f32(lr), b1, b2,
                                             eps, wd, int(pre), s), "rows_step")

    def ff(self, c):
        """the fast-forward cases: the given state, the scalar table uploaded (double arithmetic -> fp32, as hist_set writes it)"""
        c.T = c.t_now
        self.start(c, c.m, c.v, c.s0, steps_taken=c.t_now)
        h = np.zeros((self.capacity, 2), F32)
        for j in range(1, c.t_now + 1):
            h[j] = hyper(c.lr, c.betas[0], c.betas[1], j)
        self.hist.view.copy_(_dev(h.ravel()))
        self.catchup(c.ids, c.t_now)
        out = self.read()
        assert (out[4] == INT_MAX).all(), "owner marks left"
        return out[:4]


class WrappedLazy:
    """LazyRowEmbedding + HipAdam behind the driver's interface"""

    def __init__(self, fast):
        self.fast = fast

    def start(self, c):
        from mmrec_amd.common.lazy_rows import LazyRowEmbedding
        from mmrec_amd.common.optim import HipAdam
        self.c = c
        self.table = LazyRowEmbedding.from_pretrained(_dev(c.p), freeze=False)
        self.table.allow_missing, self.table.fast_forward = True, self.fast
        self.opt = HipAdam(self.table.parameters(), lr=c.lr, betas=c.betas, eps=c.eps, weight_decay=c.wd)

    def read(self):
        torch.cuda.synchronize()
        w = self.table.weight.detach()
        st = self.opt.state.get(self.table.weight)
        m = st["exp_avg"] if st else torch.zeros_like(w)
        v = st["exp_avg_sq"] if st else torch.zeros_like(w)
        R = w.shape[0]
        last = self.table._last_step.cpu().numpy().astype(np.int64) if self.table._last_step is not None else np.zeros(R, np.int64)
        owner = self.table._owner.cpu().numpy().astype(np.int64) if self.table._owner is not None else np.full(R, INT_MAX, np.int64)
        return tuple(x.cpu().numpy().astype(F64) for x in (w, m, v)) + (last, owner)

    def catchup(self, ids, t_now):
        self.table.rows(_dev(ids))

    def flush(self, t):
        self.table.flush()

    def step(self, ids, g, t, lr):
        self.opt.param_groups[0]["lr"] = lr
        (self.table.rows(_dev(ids)) * _dev(g)).sum().backward()          # (the rows are current: this catch-up replays nothing)
        self.opt.step()


def _report(reps):
    for name, rep in reps.items():
        if rep.err is not None:
            raise rep.err
    print("worst err / tol:", {k: round(r.worst, 3) for k, r in reps.items()})


# ------------------------------------------------------------------------------------------------ GPU tests
@pytest.mark.gpu
@pytest.mark.parametrize("seed", range(N_DENSE))
def test_dense_fuzz(seed):
    c = draw_case(seed)
    host, dev = GpuDense(False), GpuDense(True)
    reps, _ = run_dense(c, {"host": host, "dev": dev})
    _report(reps)
    for a, b, nm in zip(host.T.get(), dev.T.get(), "pmv"):    # the device-scalar form equals the host form bit for bit
        same_bits(a, b, "dev == host " + nm + " " + c.axes())


@pytest.mark.gpu
@pytest.mark.parametrize("dev", [False, True])
@pytest.mark.parametrize("seed", range(N_DENSE, N_DENSE + N_MULTI))
def test_multi_tensor_fuzz(seed, dev):
    c = draw_case(seed)
    outs = {}

    class Keep(GpuMulti):
        def multi_step(self, c, dev):
            outs[self.per_tensor] = GpuMulti.multi_step(self, c, dev)
            return outs[self.per_tensor]
    reps, _ = run_multi(c, {"multi": Keep(False), "per_tensor": Keep(True)}, dev)
    _report(reps)
    for i in range(c.n_tensors):                             # one table launch equals the per-tensor kernel bit for bit
        for a, b, nm in zip(outs[False][i], outs[True][i], "pmv"):
            same_bits(a, b, "multi == per tensor %d %s %s" % (i, nm, c.axes()))


@pytest.mark.gpu
@pytest.mark.parametrize("seed", range(N_DENSE + N_MULTI, N_DENSE + N_MULTI + N_LAZY))
def test_row_lazy_fuzz(seed):
    c = draw_case(seed)
    impls = {"host": GpuLazy()}
    if seed in LAZY_DEV_SEEDS:
        impls["dev"] = GpuLazy(dev=True)
    reps, _ = run_lazy(c, impls)
    _report(reps)
    if "dev" in impls:
        for a, b, nm in zip(impls["host"].read()[:4], impls["dev"].read()[:4], ("p", "m", "v", "last_step")):
            same_bits(a, b, "dev == host " + nm) if nm != "last_step" else np.testing.assert_array_equal(a, b)
        assert int(impls["dev"].sc.overflow.item()) == 0 and int(impls["dev"].sc.step.item()) == c.T


@pytest.mark.gpu
@pytest.mark.parametrize("seed", [N_DENSE + N_MULTI + 3, N_DENSE + N_MULTI + 8])
def test_presummed_equals_the_in_kernel_sum(seed):
    """rows_step with the pre-summed dyadic gradients in the owners' slots == the kernel's own position-order sum, bit for bit"""
    c = draw_case(seed)
    impls = {"summed_in_kernel": GpuLazy(), "presummed": GpuLazy(presummed_always=True)}
    reps, _ = run_lazy(c, impls)
    _report(reps)
    for a, b, nm in zip(impls["summed_in_kernel"].read()[:3], impls["presummed"].read()[:3], "pmv"):
        same_bits(a, b, "presummed == summed " + nm)


@pytest.mark.gpu
@pytest.mark.parametrize("seed", [N_DENSE + N_MULTI + 1, N_DENSE + N_MULTI + 3, N_DENSE + N_MULTI + 7])
def test_row_lazy_fast_forward_inside_a_run(seed):
    """the opt-in closed form inside whole row-lazy runs (wd = 0, gaps above 12), host and device form"""
    c = draw_case(seed)
    impls = {"ff": GpuLazy(fast=True), "ff_dev": GpuLazy(dev=True, fast=True)}
    reps, _ = run_lazy(c, impls, fast=("ff", "ff_dev"))
    _report(reps)
    for a, b, nm in zip(impls["ff"].read()[:3], impls["ff_dev"].read()[:3], "pmv"):
        same_bits(a, b, "ff_dev == ff " + nm)


@pytest.mark.gpu
@pytest.mark.parametrize("seed", range(N_DENSE + N_MULTI + N_LAZY, CASES))
def test_fast_forward_fuzz(seed):
    c = draw_case(seed)
    impls = {"ff": GpuLazy(fast=True), "ff_dev": GpuLazy(dev=True, fast=True), "catchup": GpuLazy()}
    reps, _, outs, elig = run_ff(c, impls, fast=("ff", "ff_dev"))
    _report(reps)
    for a, b, nm in zip(outs["ff"][:3], outs["ff_dev"][:3], "pmv"):
        same_bits(a, b, "ff_dev == ff " + nm)
    forced = np.array([not e for e in elig])                 # gap <= 12, wd != 0, b1 = 0.95 beyond 256 steps, t_now <= 128
    if c.wd != 0.0 or c.t_now <= 128:
        assert forced.all()
    for a, b, nm in zip(outs["ff"][:3], outs["catchup"][:3], "pmv"):
        same_bits(a[forced], b[forced], "ff == catchup where the replay is exact: " + nm)


@pytest.mark.gpu
def test_capacity_edge_of_the_device_forms():
    """capacity = 8: step 7 is the last one written; step 8 raises the sticky flag and from then on catch-up and step leave p, m,
    v and last_step bit for bit alone.  The owner marks of such a refused call are NOT released (the kernels return before they
    look at a row; include/mmrec_hip.h): the caller refills `owner` when it resumes, as LazyRowEmbedding.resume does."""
    c = Case()
    c.seed, c.kind, c.R, c.F, c.T = -1, "lazy", 8, 8, 7
    c.wd, c.betas, c.eps, c.lr = 0.0, B0, 1e-8, 1e-3
    rng = np.random.default_rng(5)
    c.p = rng.uniform(-1, 1, (8, 8)).astype(F32)
    c.ids = [None] + [rng.integers(0, 8, 5).astype(np.int64) for _ in range(9)]
    c.g = [None] + [(rng.integers(-16, 17, (5, 8)) / 16.0).astype(F32) for _ in range(9)]
    c.extra, c.lrs = {}, [None] + [c.lr] * 9
    im = GpuLazy(dev=True)
    orig_start = im.start
    im.start = lambda cc: orig_start(cc, capacity=8)
    reps, _ = run_lazy(c, {"dev": im})
    _report(reps)
    assert int(im.sc.overflow.item()) == 0 and int(im.sc.step.item()) == 7
    frozen = im.read()
    for t in (8, 9):
        im.catchup(c.ids[t], t - 1)                          # t = 8: step_dev = 7, nothing to replay; t = 9: refused
        assert (im.read()[4] == INT_MAX).all() == (t == 8)
        im.step(c.ids[t], c.g[t], t, c.lr)
        now = im.read()
        assert int(im.sc.overflow.item()) == 1 and int(im.sc.step.item()) == t
        for a, b, nm in zip(frozen[:3], now[:3], "pmv"):
            same_bits(a, b, "after the overflow: " + nm)
        assert np.array_equal(frozen[3], now[3])
        marked = np.unique(c.ids[t])
        assert (now[4][marked] != INT_MAX).all(), "the refused call keeps its owner marks (documented)"
    im.flush(9)
    now = im.read()
    for a, b, nm in zip(frozen[:3], now[:3], "pmv"):
        same_bits(a, b, "flush after the overflow: " + nm)


@pytest.mark.gpu
def test_misuse_is_rejected_before_any_launch():
    lib, s = _lib()
    n, R, F = 64, 4, 8
    T = Tensor3(np.ones(n + 4, F32), np.ones(n + 4, F32), np.ones(n + 4, F32))
    g = torch.ones(n + 4, device="cuda:0")
    off = lambda t: ctypes.c_void_p(t.data_ptr() + 4)      # noqa: E731
    pp, pm, pv = T.ptrs()
    hyper_dev = torch.ones(2, device="cuda:0")
    b = (0.9, 0.999, 1e-8, 0.0)
    one = lambda p_=pp, g_=P(g), m_=pm, v_=pv, n_=n, step=1: lib.mmrec_adam_step_f32(p_, g_, m_, v_, n_, 1e-3, *b, step, s)      # noqa: E731
    onedev = lambda p_=pp, g_=P(g), m_=pm, v_=pv, n_=n, h=P(hyper_dev): lib.mmrec_adam_step_dev_f32(p_, g_, m_, v_, n_, h, *b, s)      # noqa: E731
    for f in (one, onedev):
        assert f(p_=off(T.p.view)) == BAD_ARG and f(g_=off(g)) == BAD_ARG and f(m_=off(T.m.view)) == BAD_ARG
        assert f(v_=off(T.v.view)) == BAD_ARG and f(n_=-1) == BAD_ARG and f(p_=None) == BAD_ARG and f(g_=None) == BAD_ARG
    assert one(step=0) == BAD_ARG and onedev(h=None) == BAD_ARG
    arr1 = lambda x: (ctypes.c_void_p * 1)(x.value)      # noqa: E731
    n1, lr1 = (ctypes.c_int64 * 1)(n), (ctypes.c_float * 1)(1e-3)
    st1, st0, neg = (ctypes.c_int64 * 1)(1), (ctypes.c_int64 * 1)(0), (ctypes.c_int64 * 1)(-1)
    multi = lambda p_=pp, n_=n1, st=st1, lr=lr1, nt=1: lib.mmrec_adam_multi_step_f32(      # noqa: E731
        arr1(p_), arr1(P(g)), arr1(pm), arr1(pv), n_, nt, lr, st, *b, s)
    assert multi(p_=off(T.p.view)) == BAD_ARG and multi(n_=neg) == BAD_ARG and multi(st=st0) == BAD_ARG
    assert multi(lr=None) == BAD_ARG and multi(st=None) == BAD_ARG and multi(nt=-1) == BAD_ARG
    assert lib.mmrec_adam_multi_step_f32(None, None, None, None, None, 1, lr1, st1, *b, s) == BAD_ARG
    assert lib.mmrec_adam_multi_step_dev_f32(arr1(pp), arr1(P(g)), arr1(pm), arr1(pv), n1, 1, None, *b, s) == BAD_ARG
    assert lib.mmrec_adam_prepare(None, P(hyper_dev), 0.9, 0.999, P(hyper_dev), s) == BAD_ARG
    # row-lazy
    Tb = Tensor3(np.ones((R, F), F32), np.ones((R, F), F32), np.ones((R, F), F32))
    last, owner = Guarded(np.zeros(R, np.int32), torch.int32), Guarded(np.full(R, INT_MAX, np.int32), torch.int32)
    hist = Guarded(np.zeros((8, 2), F32))
    ids = torch.zeros(MAX_IDS + 1, dtype=torch.int64, device="cuda:0")
    gr = torch.zeros(8, F, device="cuda:0")
    step_dev, ovf = torch.ones(1, dtype=torch.int64, device="cuda:0"), torch.zeros(1, dtype=torch.int32, device="cuda:0")
    qp, qm, qv = Tb.ptrs()
    for fn in (lib.mmrec_adam_rows_catchup_f32, lib.mmrec_adam_rows_fastforward_f32):
        cu = lambda F_=F, t=1, p_=qp, h=P(hist.view), ow=P(owner.view), nid=2, ls=P(last.view): fn(      # noqa: E731
            p_, qm, qv, P(ids), ow, nid, R, F_, ls, h, t, *b, s)
        assert cu(F_=6) == BAD_ARG and cu(F_=0) == BAD_ARG and cu(t=-1) == BAD_ARG and cu(p_=None) == BAD_ARG
        assert cu(h=None) == BAD_ARG and cu(ow=None) == BAD_ARG and cu(nid=-1) == BAD_ARG and cu(ls=None) == BAD_ARG
    for fn in (lib.mmrec_adam_rows_catchup_dev_f32, lib.mmrec_adam_rows_fastforward_dev_f32):
        cud = lambda F_=F, cap=8, sd=P(step_dev), p_=qp: fn(p_, qm, qv, P(ids), P(owner.view), 2, R, F_, P(last.view), P(hist.view), cap, sd,      # noqa: E731
                                                         *b, s)
        assert cud(F_=6) == BAD_ARG and cud(cap=1) == BAD_ARG and cud(sd=None) == BAD_ARG and cud(p_=None) == BAD_ARG
    rs = lambda F_=F, t=1, nid=2, pre=0, g_=P(gr), p_=qp: lib.mmrec_adam_rows_step_f32(      # noqa: E731
        p_, qm, qv, P(ids), P(owner.view), g_, nid, F_, P(last.view), t, 1e-3, *b, pre, s)
    assert rs(F_=6) == BAD_ARG and rs(t=0) == BAD_ARG and rs(nid=-1) == BAD_ARG and rs(g_=None) == BAD_ARG and rs(p_=None) == BAD_ARG
    assert rs(nid=MAX_IDS + 1) == UNSUPPORTED
    rsd = lambda F_=F, cap=8, nid=2, sd=P(step_dev): lib.mmrec_adam_rows_step_dev_f32(      # noqa: E731
        qp, qm, qv, P(ids), P(owner.view), P(gr), nid, F_, P(last.view), cap, sd, P(hyper_dev), *b, 0, s)
    assert rsd(F_=6) == BAD_ARG and rsd(cap=1) == BAD_ARG and rsd(sd=None) == BAD_ARG and rsd(nid=MAX_IDS + 1) == UNSUPPORTED
    assert lib.mmrec_adam_hist_set(None, 1, 1e-3, 0.9, 0.999, s) == BAD_ARG
    assert lib.mmrec_adam_hist_set(P(hist.view), 0, 1e-3, 0.9, 0.999, s) == BAD_ARG
    assert lib.mmrec_adam_hist_set_dev(P(hist.view), 1, P(step_dev), P(hyper_dev), P(ovf), s) == BAD_ARG
    assert lib.mmrec_adam_hist_set_dev(P(hist.view), 8, None, P(hyper_dev), P(ovf), s) == BAD_ARG
    assert lib.mmrec_adam_rows_owner(None, 2, P(owner.view), s) == BAD_ARG and lib.mmrec_adam_rows_owner(P(ids), -1, P(owner.view), s) == BAD_ARG
    torch.cuda.synchronize()
    for x in (T.p, T.m, T.v, Tb.p, Tb.m, Tb.v, last, owner, hist):
        x.get("misuse")
    for a in T.get() + Tb.get():
        assert (a == 1.0).all()
    assert (last.get() == 0).all() and (owner.get() == INT_MAX).all() and (hist.get() == 0).all() and int(ovf.item()) == 0


@pytest.mark.gpu
@pytest.mark.parametrize("capturable", [False, True])
@pytest.mark.parametrize("multi_tensor", [True, False])
def test_hip_adam_wrapper_vs_float64(multi_tensor, capturable):
    """30 tensors, 4 steps; parameter 7 has no gradient in steps 2 and 3.  capturable=False: it follows its OWN step count (as
    torch.optim.Adam does).  capturable=True: every parameter of a group reads the group's ONE device counter (HipAdam's
    docstring), so the bias corrections of parameter 7 are the group's."""
    from mmrec_amd.common.optim import HipAdam
    rng = np.random.default_rng(77)
    sizes = [int(SMALL_N[i % len(SMALL_N)]) for i in range(30)]
    lr, betas, eps, wd = 1e-3, B0, 1e-8, 1e-2
    hp = (f32(betas[0]), f32(betas[1]), f32(eps), f32(wd))
    data = [_fill(rng, n, "dense", False, 4) for n in sizes]
    params = [torch.nn.Parameter(_dev(d[0])) for d in data]
    opt = HipAdam(params, lr=lr, betas=betas, eps=eps, weight_decay=wd, capturable=capturable, multi_tensor=multi_tensor)
    refs, own = [State(d[0], d[1], d[2]) for d in data], [0] * 30
    for k in range(4):
        for i, prm in enumerate(params):
            skip = i == 7 and k in (1, 2)
            prm.grad = None if skip else _dev(data[i][3][k])
            if not skip:
                own[i] += 1
                A, B = hyper(lr, betas[0], betas[1], k + 1 if capturable else own[i])
                refs[i].step(data[i][3][k].astype(F64), A, B, hp)
        opt.step()
        torch.cuda.synchronize()
        for i, prm in enumerate(params):
            st = opt.state[prm]
            if st:
                got = tuple(x.detach().cpu().numpy().astype(F64) for x in (prm, st["exp_avg"], st["exp_avg_sq"]))
                check_state(got, refs[i], "wrapper step %d tensor %d" % (k, i))
    assert opt.state[params[7]]["step"] == 2 and opt.state[params[0]]["step"] == 4


@pytest.mark.gpu
@pytest.mark.parametrize("fast", [False, True])
@pytest.mark.parametrize("seed", LAZY_WRAPPER_SEEDS)
def test_lazy_row_embedding_wrapper_vs_float64(seed, fast):
    c = draw_case(seed)
    reps, _ = run_lazy(c, {"wrapper": WrappedLazy(fast)}, fast=("wrapper",) if fast else ())
    _report(reps)
