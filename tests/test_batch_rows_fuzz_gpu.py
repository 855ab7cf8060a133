"""GPU: seeded differential fuzz of the batch-row propagation autograd nodes of mmrec_amd/hip_ops.py -- `spmm_rows`
(_SpmmRows), `lightgcn_mean_parts` (_LightGCNMeanParts), `lightgcn_mean_parts_rows` (_LightGCNMeanPartsRows),
`lightgcn_mean_rows_then_item_rows` (_MeanPartsRowsThenItemRows) and `layergcn_sum_parts` (_LayerGCNSumParts) -- forward and
every input gradient against float64 on the host (scipy / numpy; LayerGCN: float64 torch autograd), never against another
form of the ops.  The helpers and the two acceptance modes are those of tests/test_spmm_fuzz_gpu.py.

What is compared (A the user-item graph over [users; items], M the item-item graph, E0 = cat(U, I), s = 1 / (L + 1)):
  forward   at = s sum_{l <= L} A^l E0 read at the listed rows;  ia = (M I)[item_rows] + at[b:]
  backward  G = the compact upstream gradient scattered into [n, d], duplicates summed:  d E0 = s sum_{l <= L} (A^T)^l G,
            + M^T (P d_ia) on the item block; d Z_rows of spmm_rows = the upstream gradient
and M of the float criterion is the same expression on absolute values (|A|, |M|, |E0|, |G|).  `check` takes sums of
coefficient x matrix x table; the layer sums are handed to it as (ref + mag) / 2 - (mag - ref) / 2, two non-negative
tables whose difference is the float64 result and whose sum is the magnitude.

Axes (`make_case`; `test_cases_span_every_axis` shows each value occurs): L 0 ... 4, d 8 / 16 / 32 / 64, the plan of A (no long
row; single-chunk long rows; hub rows of 513 / 1024 / 1025 / 5000 nonzeros among the items, listed in the batch; a forced row
schedule), symmetric and directed A (the backward through transpose()), seven kinds of row list (an empty batch: every
gradient exactly 0), four table layouts, five forms of the upstream gradient, and the path switches (ROWS_LAST_LAYER off,
set_deterministic, either graph as a PermutedGraph, an item-item row beyond ROWS_MAX_CHUNKS).  The path each case must take is
restated from the case alone (`expected_path`) and asserted on `rows_servable`, `row_blocks_of_one_buffer` and the outputs'
`grad_fn`.

exact  L = 1 (s = 1/2) on every plan, about half of the L = 0 cases (a draw), and L = 3 (s = 1/4) on a low-degree graph
       whose values are multiples of 1/2:
       tables and gradients multiples of 1/16, values of A and M multiples of 1/8 -- every value any order can form is a multiple
       of 2^-9 (asserted in `make_case`), its magnitude is asserted by `check`, and the outputs must equal float64; the push
       kernel's fp32 atomics are exact on the grid.
float  |got - ref64| <= gamma(N) M + N 2^-149, N the most roundings a term meets on the path the case takes (`gpu_depths`),
       stage by stage from hip_ops.py (D(X) = plan_depth(degrees of X).max(), the epilogue's four included; m = the largest
       multiplicity of a listed row; push(X) = the most atomic adds into one element: the listed rows' nonzeros that hit one
       column, with multiplicity):
         layer mean, forward           L launches of A, of which the last may be the row-list kernel (the full launch's bits),
                                       the rounded s and the multiply by it (in the last epilogue, or on the compact rows)
                                                                                            N_at = L D(A) + 2
         ia                            row-list kernel on M with Z = at[b:] (a term of at meets the epilogue's four; a term of
                                       M I meets D(M))                                     max(D(M), N_at + 4)
                                       fallback spmm(M, I).index_select + Z_rows            max(D(M), N_at) + 1
         _LightGCNMeanPartsRows.backward   L = 0: one push of G into zeros                   m + 2
                                       L >= 1: the first step pushes s G through the listed rows into the table that also
                                       receives s G itself (max over elements of push(A) + multiplicity adds, + 2 for
                                       s * g and val * that, + 1 for the rounded s), then L - 1 times a launch of A^T and m
                                       more atomic adds of s G
                                                        N_b = max(push(A) + mult) + 3 + (L - 1) (D(A^T) + m)
         dense fallback (deterministic, PermutedGraph: index_select's backward is torch's index_add, then
                                       _LightGCNMean.backward)                               N_b = m + L D(A^T) + 2
         item-item push, one node      push(M) more atomic adds into the item block          N_b + push(M)
                         two nodes     autograd adds the two gradients of I                  max(N_b, push(M) + 2) + 1
                         fallback      index_add, then a launch of M^T                       max(N_b, m_items + D(M^T)) + 1
         lightgcn_mean_parts           forward N_at, backward (a PermutedGraph: cat, lightgcn_mean, split -- the same
                                       launches)                                             L D(A^T) + 2
       (a PermutedGraph keeps every row's entries and the threshold, so its D is the plain graph's; its permutations add and
       round nothing.)  `make_case` asserts N <= 1024 on every float case: gamma < 6.2e-5, a 1e-4 relative error is caught
       everywhere.  Half of the float cases have positive values and tables, as the normalised adjacency has.
Every element of every output is checked; each case prints its worst err / M next to gamma(N).

tests/test_batch_rows_cpu.py runs the same cases through the torch-CPU stand-ins (N from sequential chain lengths,
`cpu_depths`) and shows that the checker rejects each planted error."""
import contextlib
import types

import numpy as np
import pytest
import scipy.sparse as sp
import torch

from tests.test_spmm_fuzz_gpu import (GRID, _grid, _layergcn64, _on, _square_graph, absolute, check, csr, gamma, plan_depth,
                                      rows_of, scatter_matrix)

OPS = ("then", "parts_rows", "spmm_rows", "parts")
LAYERS = (0, 1, 2, 3, 4)
WIDTHS = (8, 16, 32, 64)
PLANS = ("none", "single", "multi", "sched")
LISTS = ("dup_users", "pos_is_neg", "hub_repeated", "empty_row", "ends", "one_id", "empty_batch")
STORAGE = ("adjacent", "offset", "swapped", "separate")
GRADS = ("both", "user_only", "item_only", "one_buffer", "noncontig")
SWITCHES = ("none", "last_layer_off", "deterministic", "perm_g", "perm_mm", "mm_beyond")
SWITCHES_OF = {"then": SWITCHES[1:], "parts_rows": ("last_layer_off", "deterministic", "perm_g"),
               "spmm_rows": ("deterministic", "perm_mm", "mm_beyond"), "parts": ("perm_g",)}
HUBS = (513, 1024, 1025, 5000)
CASES = 80                      # every (op, L, plan) once; the other axes cycle per op (make_case)
ROWS_MAX_CHUNKS, CHUNK = 480, 512
N_MAX = 1024


class Case:
    pass


# ------------------------------------------------------------------------------------------------ cases (host only)
def _sorted_coo(i, j, v, n):
    order = np.argsort(i, kind="stable")
    i, j, v = i[order], j[order], v[order]
    rowptr = np.zeros(n + 1, np.int64)
    np.cumsum(np.bincount(i, minlength=n), out=rowptr[1:])
    return i, j, v, rowptr


def _values(rng, c, k, half=False):
    if c.exact:
        return ((rng.integers(-2, 3, k) / 2.0) if half else (rng.integers(-8, 9, k) / 8.0)).astype(np.float32)
    sign = 1.0 if c.positive else rng.choice([-1.0, 1.0], k)
    return (rng.uniform(1 / 64, 1 / 8, k) * sign).astype(np.float32)


def _table(rng, c, shape):
    if c.exact:
        return _grid(rng, shape)
    t = rng.standard_normal(shape) * 0.5
    return (np.abs(t) if c.positive else t).astype(np.float32)


def _user_item_graph(rng, c):
    """A over [users; items], bipartite: the upper block's edges mirrored with their values (symmetric) or a lower block drawn
    on its own (directed); hub rows among the items; isolated users and items (empty rows and columns)"""
    nu, ni, n = c.nu, c.ni, c.n
    low = c.exact and c.L == 3
    n_edges = n if low else 6 * n
    c.g_thr = {"none": 4096, "single": int(rng.choice([8, 16, 32])), "multi": 32, "sched": 16}[c.plan]
    hub_items = [1, ni // 2, 9, ni - 2]
    hub_deg = {"none": (), "single": (100, 300, 400), "multi": HUBS, "sched": (60, 200)}[c.plan]
    c.hubs = dict(zip(hub_items, hub_deg))                             # item id -> nonzeros of its row
    c.iso_users, c.iso_items = [3, nu - 2], [4, ni - 3]

    def block(k):
        eu, ei = rng.integers(0, nu, k), rng.integers(0, ni, k)
        keep = ~(np.isin(eu, c.iso_users) | np.isin(ei, c.iso_items + list(c.hubs)))
        return eu[keep], ei[keep]

    eu, ei = block(n_edges)
    v = _values(rng, c, eu.size, low)
    hr = np.concatenate([np.full(k, h) for h, k in c.hubs.items()] + [np.zeros(0, np.int64)]).astype(np.int64)
    hc = rng.integers(0, nu, hr.size)
    hc[np.isin(hc, c.iso_users)] = 0
    hv = _values(rng, c, hr.size, low)
    if c.symmetric:
        i = np.concatenate([eu, nu + ei, nu + hr, hc])
        j = np.concatenate([nu + ei, eu, hc, nu + hr])
        vals = np.concatenate([v, v, hv, hv])
    else:
        eu2, ei2 = block(n_edges)
        i = np.concatenate([eu, nu + ei2, nu + hr])
        j = np.concatenate([nu + ei, eu2, hc])
        vals = np.concatenate([v, _values(rng, c, eu2.size, low), hv])
    c.g_rows, c.g_cols, c.g_vals, c.g_rowptr = _sorted_coo(i, j, vals.astype(np.float32), n)
    c.A = csr(c.g_rowptr, c.g_cols, c.g_vals, (n, n))
    c.g_deg, c.g_coldeg = np.diff(c.g_rowptr), np.bincount(c.g_cols, minlength=n)
    for h, k in c.hubs.items():
        assert c.g_deg[nu + h] == k
    assert c.g_deg[[3, nu - 2, nu + 4, nu + ni - 3]].sum() == 0 and c.g_coldeg[[3, nu - 2, nu + 4, nu + ni - 3]].sum() == 0
    multi = bool(((c.g_deg > c.g_thr) & (c.g_deg > CHUNK)).any())
    assert multi == (c.plan == "multi") and bool((c.g_deg > c.g_thr).any()) == (c.plan != "none")
    if c.symmetric:
        assert abs(c.A - c.A.T).max() < 1e-12


def _item_item_graph(rng, c):
    """M over the items, directed: about 20 nonzeros per row, two empty rows, one long row at the first hub item"""
    ni = c.ni
    deg = rng.integers(10, 31, ni)
    deg[c.iso_items] = 0
    c.mm_item = 1
    plan = c.plan if c.op == "spmm_rows" else ("multi" if c.plan == "multi" else "single")
    c.mm_thr = {"none": 4096, "single": 32, "multi": 32, "sched": 16}[plan]
    c.mm_sched = plan == "sched"
    c.mm_long = ROWS_MAX_CHUNKS * CHUNK + 1 if c.switch == "mm_beyond" else 700 if plan == "multi" else 300
    deg[c.mm_item] = c.mm_long
    rowptr = np.zeros(ni + 1, np.int64)
    np.cumsum(deg, out=rowptr[1:])
    c.mm_rows = np.repeat(np.arange(ni), deg)
    c.mm_cols = rng.integers(0, ni, c.mm_rows.size)
    c.mm_vals = _values(rng, c, c.mm_rows.size)
    c.mm_rowptr, c.mm_deg, c.mm_coldeg = rowptr, deg, np.bincount(c.mm_cols, minlength=ni)
    c.M = csr(rowptr, c.mm_cols, c.mm_vals, (ni, ni))


def _row_lists(rng, c):
    nu, ni = c.nu, c.ni
    # (symmetric hubs: every listed user pushes its ~5 entries of the 5000-nonzero hub's column into one element -- a float
    # case keeps that count, and so N, below 1024 with a smaller batch)
    B_max = 128 if (c.plan == "multi" and c.symmetric and not c.exact) else 257
    B = {"one_id": 1, "empty_batch": 0}.get(c.list, int(rng.integers(64, B_max + 1)))
    users, pos, neg = rng.integers(0, nu, B), rng.integers(0, ni, B), rng.integers(0, ni, B)
    hubs = list(c.hubs) or [c.mm_item]
    if B >= 16:
        pos[10:10 + len(hubs)] = hubs                                  # every hub row is in the batch
    if c.list == "dup_users":
        users[B // 2:] = users[:B - B // 2]
        users[:3] = users[5]
    elif c.list == "pos_is_neg":
        neg[0], neg[3] = pos[0], pos[5]
    elif c.list == "hub_repeated":
        pos[[1, 7]], neg[[2, 8]] = hubs[-1], hubs[-1]
        neg[20], neg[21] = hubs[0], c.mm_item
    elif c.list == "empty_row":
        users[4], pos[6], neg[6] = c.iso_users[0], c.iso_items[0], c.iso_items[1]
    elif c.list == "ends":
        users[0], users[-1], pos[0], neg[-1] = 0, nu - 1, 0, ni - 1
    elif c.list == "one_id" and (c.plan != "none" or c.switch == "mm_beyond"):
        pos[0] = c.mm_item if c.switch == "mm_beyond" else hubs[-1]
    c.B, c.users, c.item_rows = B, users.astype(np.int64), np.concatenate([pos, neg]).astype(np.int64)
    c.rows = np.concatenate([c.users, c.item_rows + nu])


def expected_path(c):
    """which form of each op the case must take, restated from the case alone (hip_ops.py: spmm_rows, lightgcn_mean_parts_rows,
    lightgcn_mean_rows_then_item_rows)"""
    det = c.switch == "deterministic"
    p = types.SimpleNamespace()
    p.serv_g = c.plan != "multi" or c.d == 64
    mm_multi = c.mm_long > CHUNK and c.mm_long > c.mm_thr
    p.serv_m = not mm_multi or (c.d == 64 and c.switch != "mm_beyond")
    p.rows_class = not det and c.switch != "perm_g"                    # _LightGCNMeanPartsRows (else the dense op + gather)
    p.spmm_rows_fast = not det and c.switch != "perm_mm" and p.serv_m  # _SpmmRows (else spmm + index_select)
    p.pull_last = p.rows_class and c.L >= 1 and c.switch != "last_layer_off" and p.serv_g     # the last layer at the listed rows
    p.one_node = (p.rows_class and p.spmm_rows_fast and c.d == 64 and c.L >= 1 and c.switch != "last_layer_off" and p.serv_g)
    p.adjacent = c.storage in ("adjacent", "offset")
    return p


def _push_counts(rowptr, cols, rows, n_cols):
    return np.bincount(rows_of(rowptr, cols, cols, rows)[1], minlength=n_cols)


def _counts(c):
    k = types.SimpleNamespace()
    k.mult = np.bincount(c.rows, minlength=c.n)
    k.m = int(k.mult.max(initial=0))
    k.push1 = int((_push_counts(c.g_rowptr, c.g_cols, c.rows, c.n) + k.mult).max(initial=0))
    k.pm = int(_push_counts(c.mm_rowptr, c.mm_cols, c.item_rows, c.ni).max(initial=0))
    k.mi = int(np.bincount(c.item_rows, minlength=c.ni).max(initial=0))
    return k


def _by_op(c, n_at, n_ia, n_b, n_di, n_parts_b, n_rows_fwd, n_rows_dx):
    return {"then": {"ua": n_at, "ia": n_ia, "dU": n_b, "dI": n_di},
            "parts_rows": {"at": n_at, "dU": n_b, "dI": n_b},
            "spmm_rows": {"out": n_rows_fwd, "dI": n_rows_dx, "dZ": 1},
            "parts": {"Uo": n_at, "Io": n_at, "dU": n_parts_b, "dI": n_parts_b}}[c.op]


def gpu_depths(c):
    """output name -> N on the path the case takes on the device (module docstring)"""
    p, k, L = expected_path(c), _counts(c), c.L
    Dg, Dgt = (int(plan_depth(x, c.g_thr).max()) for x in (c.g_deg, c.g_coldeg))
    Dm, Dmt = (int(plan_depth(x, c.mm_thr).max()) for x in (c.mm_deg, c.mm_coldeg))
    n_at = L * Dg + 2
    if p.rows_class:
        n_b = k.m + 2 if L == 0 else k.push1 + 3 + (L - 1) * (Dgt + k.m)
    else:
        n_b = k.m + L * Dgt + 2
    if p.one_node:
        n_ia, n_di = max(Dm, n_at + 4), n_b + k.pm
    elif p.spmm_rows_fast:
        n_ia, n_di = max(Dm, n_at + 4), max(n_b, k.pm + 2) + 1
    else:
        n_ia, n_di = max(Dm, n_at) + 1, max(n_b, k.mi + Dmt) + 1
    fwd, dx = (Dm, k.pm + 2) if p.spmm_rows_fast else (Dm + 1, k.mi + Dmt)
    return _by_op(c, n_at, n_ia, n_b, n_di, L * Dgt + 2, fwd, dx)


def cpu_depths(c):
    """the same for the torch-CPU stand-ins of tests/_cpu_ops.py: a product of index_add is a chain of the row's length + 1 for
    the multiply, its backward one of the column's length + 1; stack().mean() adds L + 1; autograd adds the two gradients of
    a table that is used twice; index_select's backward adds a row's multiplicity"""
    k, L = _counts(c), c.L
    Cg, Cgt = int(c.g_deg.max()) + 1, int(c.g_coldeg.max()) + 1
    Cm, Cmt = int(c.mm_deg.max()) + 1, int(c.mm_coldeg.max()) + 1
    n_at = L * Cg + L + 1
    n_b = k.m + L * (Cgt + 1) + 2
    return _by_op(c, n_at, max(Cm, n_at) + 1, n_b, max(n_b, k.mi + Cmt) + 1, L * (Cgt + 1) + 2, Cm + 1, k.mi + Cmt)


def make_case(k):
    rng = np.random.default_rng(8800 + k)
    c = Case()
    c.k = k
    c.op, c.L = OPS[k % 4], LAYERS[(k // 4) % 5]
    c.plan = PLANS[(k // 20 + k) % 4]                                 # every (op, L, plan) exactly once in 80 cases
    j = k // 4                                                        # the case's number among its op's 20
    if c.op == "then":                                                # (the one-node form is 64 wide)
        c.d = 64 if j % 7 != 3 else WIDTHS[(j // 7) % 3]
    else:
        c.d = WIDTHS[(j + j // 4) % 4]
    # the layouts (period 4, shifted every 4 cases), the gradient forms (period 5, shifted every 4) and the switches (every
    # third case) do not move together, nor with L (period 5): the cases that reach each node -- no switch, no fallback in
    # front of it -- see every layout and every gradient form (test_cases_span_every_axis asserts it node by node)
    c.list, c.storage, c.grads = LISTS[j % 7], STORAGE[(j + j // 4) % 4], GRADS[(4 * j + j // 4) % 5]
    c.symmetric = bool((j + j // 10) % 2)
    c.exact = c.L == 1 or (c.L == 3 and c.plan == "none") or (c.L == 0 and bool(rng.integers(0, 2)))
    c.positive = bool(rng.integers(0, 2))
    c.switch = "none"
    if j in (2, 11) if c.op == "parts" else j % 3 == 2:               # every third case of an op, its switches in turn
        c.switch = SWITCHES_OF[c.op][(j // 3) % len(SWITCHES_OF[c.op])]
        if c.switch == "mm_beyond":                                   # (a 245,761-term row is off the exact grid)
            c.switch, c.exact = ("none", True) if c.L in (1, 3) and c.exact else ("mm_beyond", False)
    c.has_z = bool(rng.random() < 0.75)                                # spmm_rows: with Z_rows
    c.nu, c.ni = int(rng.integers(800, 1750)), int(rng.integers(650, 1200))
    if c.nu == c.ni:
        c.nu += 7
    c.n = c.nu + c.ni
    _user_item_graph(rng, c)
    _item_item_graph(rng, c)
    _row_lists(rng, c)
    nu, ni, d, n_list = c.nu, c.ni, c.d, c.rows.size
    c.U0, c.I0 = _table(rng, c, (nu, d)), _table(rng, c, (ni, d))
    c.Z0 = _table(rng, c, (c.item_rows.size, d))
    up = (lambda shape: _grid(rng, shape)) if c.exact else (lambda shape: rng.standard_normal(shape).astype(np.float32))
    if c.op == "parts":
        c.G1, c.G2 = up((nu, d)), up((ni, d))
    elif c.op == "spmm_rows":
        c.G1, c.G2 = up((c.B, d)), up((c.B, d))                       # the positives' and the negatives' rows
    else:
        c.G1, c.G2 = up((c.B, d)), up((n_list - c.B, d))
    if c.grads == "user_only":
        c.G2 = np.zeros_like(c.G2)
    elif c.grads == "item_only":
        c.G1 = np.zeros_like(c.G1)
    if c.exact:
        # the grid: s a power of two, and the finest value any path forms -- s x (value granule)^L x 1/16, the item-item
        # product's 1/8 x 1/16 -- is a multiple of 1 / GRID; magnitudes are asserted by `check` on the actual sums
        s = 1.0 / (c.L + 1)
        granule = s * (0.5 if c.L == 3 else 0.125) ** c.L / 16.0
        assert s in (1.0, 0.5, 0.25) and min(granule, 1.0 / 128) * GRID >= 1.0, (k, "outside the exact grid")
    else:
        worst = max(gpu_depths(c).values())
        assert worst <= N_MAX, (k, "float case with N = %d" % worst)
    return c


_CACHE = {}


def case(k):
    """the case, drawn once per process (the CPU module and the planted-error test read the same ones)"""
    if k not in _CACHE:
        _CACHE[k] = make_case(k)
    return _CACHE[k]


# ------------------------------------------------------------------------------------------------ float64 reference
def _layer_sum(A, V, mag, L, s, drop=None):
    """s sum_{l <= L} A^l V and the same on absolute values (drop: a planted error, the term l left out)"""
    absA = absolute(A)
    cur, cabs = V, mag
    ref = np.zeros_like(V) if drop == 0 else V.copy()
    tot = mag.copy()
    for layer in range(1, L + 1):
        cur, cabs = np.asarray(A @ cur), np.asarray(absA @ cabs)
        if drop != layer:
            ref = ref + cur
        tot = tot + cabs
    return s * ref, s * tot


def reference(c, dedup=False, no_transpose=False, drop=None, s=None, no_item_push=False, shift=False):
    """output name -> (float64 result, magnitude), forward outputs and input gradients of the case's op.  The keywords plant
    errors (tests/test_batch_rows_cpu.py); with none of them this is the reference"""
    f8 = np.float64
    nu, ni, n, B, L = c.nu, c.ni, c.n, c.B, c.L
    s = 1.0 / (L + 1) if s is None else s
    U, I = c.U0.astype(f8), c.I0.astype(f8)
    G = np.concatenate([c.G1, c.G2]).astype(f8)
    out = {}
    if c.op == "spmm_rows":
        Mr = csr(*rows_of(c.mm_rowptr, c.mm_cols, c.mm_vals, c.item_rows), (c.item_rows.size, ni))
        z = c.Z0.astype(f8) if c.has_z else np.zeros((c.item_rows.size, c.d))
        out["out"] = (np.asarray(Mr @ I) + z, np.asarray(absolute(Mr) @ np.abs(I)) + np.abs(z))
        out["dI"] = (np.asarray(Mr.T @ G), np.asarray(absolute(Mr).T @ np.abs(G)))
        if c.has_z:
            out["dZ"] = (G, np.abs(G))
        return out
    E0 = np.concatenate([U, I])
    fwd, fmag = _layer_sum(c.A, E0, np.abs(E0), L, s, drop=None)
    At = c.A if no_transpose else c.A.T.tocsr()
    if c.op == "parts":
        out["Uo"], out["Io"] = (fwd[:nu], fmag[:nu]), (fwd[nu:], fmag[nu:])
        d, dmag = _layer_sum(At, G, np.abs(G), L, s, drop)
    else:
        rows = c.rows + (np.arange(c.rows.size) >= B) * (1 if shift else 0)
        rows = np.minimum(rows, n - 1)
        at, amag = fwd[rows], fmag[rows]
        P = scatter_matrix(c.rows, n)
        if dedup:                                                     # a duplicated row's gradients: the first of them only
            keep = np.zeros(c.rows.size)
            keep[np.unique(c.rows, return_index=True)[1]] = 1.0
            P = P @ sp.diags(keep)
        Gf, Gabs = np.asarray(P @ G), np.asarray(P @ np.abs(G))
        d, dmag = _layer_sum(At, Gf, Gabs, L, s, drop)
        if c.op == "parts_rows":
            out["at"] = (at, amag)
        else:
            Mr = csr(*rows_of(c.mm_rowptr, c.mm_cols, c.mm_vals, c.item_rows), (c.item_rows.size, ni))
            out["ua"] = (at[:B], amag[:B])
            out["ia"] = (np.asarray(Mr @ I) + at[B:], np.asarray(absolute(Mr) @ np.abs(I)) + amag[B:])
            if not no_item_push:
                d, dmag = d.copy(), dmag.copy()
                d[nu:] += np.asarray(Mr.T @ G[B:])
                dmag[nu:] += np.asarray(absolute(Mr).T @ np.abs(G[B:]))
    out["dU"], out["dI"] = (d[:nu], dmag[:nu]), (d[nu:], dmag[nu:])
    return out


def rounded(ref):
    """the float64 results rounded to fp32: the best any fp32 implementation can give"""
    return {name: r.astype(np.float32) for name, (r, _) in ref.items()}


def accept(c, got, depths, ref=None):
    """every output of the case against float64 in the case's mode -> name -> (worst err / M, N); an empty batch's gradients
    must be exactly 0"""
    ref = reference(c) if ref is None else ref
    assert set(got) == set(ref), (sorted(got), sorted(ref))
    report = {}
    for name, (r, mag) in ref.items():
        g = got[name]
        assert tuple(g.shape) == r.shape, (c.k, name, tuple(g.shape), r.shape)
        if c.list == "empty_batch" and name in ("dU", "dI", "dZ") and c.op != "parts":
            gn = g.detach().cpu().numpy() if isinstance(g, torch.Tensor) else np.asarray(g)
            assert not gn.any(), (c.k, name, "gradient of an empty batch is not exactly 0")
        N = depths[name]
        eye = sp.identity(r.shape[0], format="csr")
        worst = check(g, [(1.0, eye, (mag + r) / 2), (-1.0, eye, (mag - r) / 2)], exact=c.exact,
                      depth=np.full(r.shape[0], N), name="case %d %s %s" % (c.k, c.op, name))
        report[name] = (worst, N)
    return report


def describe(c, report):
    parts = " ".join("%s %.2e/%.2e(N %d)" % (nm, w, gamma(N), N) for nm, (w, N) in report.items())
    return ("batch rows case %d: %s L %d d %d %s %s %s list %s storage %s grads %s switch %s B %d: worst err/M / gamma(N): %s" % (
        c.k, c.op, c.L, c.d, c.plan, "symmetric" if c.symmetric else "directed", "exact" if c.exact else "float", c.list,
        c.storage, c.grads, c.switch, c.B, parts))


# ------------------------------------------------------------------------------------------------ running a case
def tables(parts, storage, to_dev):
    """the tables as leaves in the layout: adjacent in one allocation in this order / behind a storage offset / in one
    allocation in the reverse order / separate allocations"""
    if storage == "separate":
        return [to_dev(p).requires_grad_() for p in parts]
    pad = 1 if storage == "offset" else 0
    order = list(parts)[::-1] if storage == "swapped" else list(parts)
    d = parts[0].shape[1]
    buf = to_dev(np.concatenate([np.zeros((pad, d), np.float32)] + order + [np.zeros((pad, d), np.float32)]))
    views, r = [], pad
    for p in order:
        views.append(buf[r:r + p.shape[0]].detach().requires_grad_())
        r += p.shape[0]
    assert (views[0].storage_offset() != 0) == (storage == "offset")
    return views[::-1] if storage == "swapped" else views


def send_gradients(outs, grads, how, to_dev):
    """backward from the two outputs with upstream gradients in the form `how`"""
    if how == "user_only":
        outs, grads = outs[:1], grads[:1]
    elif how == "item_only":
        outs, grads = outs[1:], grads[1:]
    if how == "one_buffer":
        buf = to_dev(np.concatenate(grads))
        g = list(buf.split([x.shape[0] for x in grads]))
    elif how == "noncontig":
        g = [to_dev(np.ascontiguousarray(x.T)).t() for x in grads]
        assert all(not x.is_contiguous() for x in g if x.shape[0] > 1)
    else:
        g = [to_dev(x) for x in grads]
    torch.autograd.backward(list(outs), g)


@contextlib.contextmanager
def switched(hip_ops, c, on_gpu):
    saved = hip_ops.ROWS_LAST_LAYER
    det = on_gpu and c.switch == "deterministic"
    try:
        if on_gpu and c.switch == "last_layer_off":
            hip_ops.ROWS_LAST_LAYER = False
        if det:
            hip_ops.set_deterministic(True)
        yield
    finally:
        hip_ops.ROWS_LAST_LAYER = saved
        if det:
            hip_ops.set_deterministic(False)


def _fn(t):
    return type(t.grad_fn).__name__


def run_case(c, hip_ops, dev, on_gpu):
    """the case's op through `hip_ops` (the HIP ops, or the stand-ins patched into it) -> name -> tensor.  on_gpu: the path
    switches are applied and the path taken is asserted; the stand-ins have one path"""
    to_dev = _on if on_gpu else (lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev))
    p = expected_path(c)
    kw_g = {"row_schedule": True} if on_gpu and c.plan == "sched" else {}
    kw_m = {"row_schedule": True} if on_gpu and c.mm_sched else {}
    g = hip_ops.CsrGraph.from_coo_host(np.stack([c.g_rows, c.g_cols]), c.g_vals, c.n, c.n, dev, symmetric=c.symmetric,
                                       long_row_threshold=c.g_thr, **kw_g)
    mm = hip_ops.CsrGraph.from_coo_host(np.stack([c.mm_rows, c.mm_cols]), c.mm_vals, c.ni, c.ni, dev,
                                        long_row_threshold=c.mm_thr, **kw_m)
    if on_gpu:
        assert hip_ops.rows_servable(g, c.d) == p.serv_g and hip_ops.rows_servable(mm, c.d) == p.serv_m
        assert (g.sched is not None) == (c.plan == "sched") and (g.transpose() is g) == c.symmetric
        if c.switch == "mm_beyond":
            assert mm.max_row_chunks == ROWS_MAX_CHUNKS + 1 == hip_ops.ROWS_MAX_CHUNKS + 1
        if c.switch == "perm_g":
            g = hip_ops.PermutedGraph(g, "degree")
        if c.switch == "perm_mm":
            mm = hip_ops.PermutedGraph(mm, "degree")
    U, I = tables((c.U0, c.I0), c.storage, to_dev)
    if on_gpu:
        assert hip_ops.row_blocks_of_one_buffer((U, I)) == p.adjacent
    users, item_rows, rows = to_dev(c.users), to_dev(c.item_rows), to_dev(c.rows)
    got = {}
    with switched(hip_ops, c, on_gpu):
        if c.op == "then":
            ua, ia = hip_ops.lightgcn_mean_rows_then_item_rows(g, U, I, c.L, users, item_rows, mm)
            if on_gpu:
                assert (_fn(ua) == "_MeanPartsRowsThenItemRowsBackward") == p.one_node == (ia.grad_fn is ua.grad_fn), _fn(ua)
                if not p.one_node:
                    assert (_fn(ia) == "_SpmmRowsBackward") == p.spmm_rows_fast, _fn(ia)
                    inner = type(ua.grad_fn.next_functions[0][0]).__name__
                    assert (inner == "_LightGCNMeanPartsRowsBackward") == p.rows_class, inner
            got["ua"], got["ia"] = ua.detach(), ia.detach()
            send_gradients((ua, ia), (c.G1, c.G2), c.grads, to_dev)
        elif c.op == "parts_rows":
            at = hip_ops.lightgcn_mean_parts_rows(g, (U, I), c.L, rows)
            if on_gpu:
                assert (_fn(at) == "_LightGCNMeanPartsRowsBackward") == p.rows_class, _fn(at)
            got["at"] = at.detach()
            send_gradients((at[:c.B], at[c.B:]), (c.G1, c.G2), c.grads, to_dev)
        elif c.op == "spmm_rows":
            Z = to_dev(c.Z0).requires_grad_() if c.has_z else None
            out = hip_ops.spmm_rows(mm, I, item_rows, Z_rows=Z)
            if on_gpu:
                assert (_fn(out) == "_SpmmRowsBackward") == p.spmm_rows_fast, _fn(out)
            got["out"] = out.detach()
            send_gradients((out[:c.B], out[c.B:]), (c.G1, c.G2), c.grads, to_dev)
            if c.has_z:
                got["dZ"] = Z.grad
        else:
            Uo, Io = hip_ops.lightgcn_mean_parts(g, (U, I), c.L)
            if on_gpu:                                                # (a relabelled graph: cat, lightgcn_mean, split)
                assert (_fn(Uo) == "_LightGCNMeanPartsBackward") == (c.switch != "perm_g"), _fn(Uo)
                assert c.switch == "perm_g" or Io.grad_fn is Uo.grad_fn
            got["Uo"], got["Io"] = Uo.detach(), Io.detach()
            send_gradients((Uo, Io), (c.G1, c.G2), c.grads, to_dev)
    if on_gpu:
        torch.cuda.synchronize()
        assert hip_ops.ROWS_LAST_LAYER is True and hip_ops.DETERMINISTIC is False
        assert not torch.are_deterministic_algorithms_enabled()
    if c.op != "spmm_rows":
        assert U.grad is not None, "the user table received no gradient"
        got["dU"] = U.grad
    assert I.grad is not None, "the item table received no gradient"
    got["dI"] = I.grad
    return got


# ------------------------------------------------------------------------------------------------ CPU: the cases
def test_cases_span_every_axis():
    """every (op, L, plan) once; every width, list, layout, gradient form and switch, with the ops it bears on; exact mode at
    L = 1 on every plan (multi-chunk hubs included) and at L = 3; the one-node form on every plan, symmetric and directed;
    every fallback of it; hubs listed; N <= 1024 on every float case (asserted by make_case).  Layouts and gradient forms are
    counted on the cases that reach each node, not on those a switch or an unserved width sends round it"""
    cs = [case(k) for k in range(CASES)]
    assert {(c.op, c.L, c.plan) for c in cs} == {(o, L, p) for o in OPS for L in LAYERS for p in PLANS}
    for axis, values in (("d", WIDTHS), ("list", LISTS), ("storage", STORAGE), ("grads", GRADS), ("switch", SWITCHES),
                         ("symmetric", (True, False)), ("exact", (True, False))):
        assert {getattr(c, axis) for c in cs} == set(values), axis
    rows_ops = [c for c in cs if c.op in ("then", "parts_rows")]
    assert {c.list for c in rows_ops if c.op == "then"} == set(LISTS) == {c.list for c in rows_ops if c.op == "parts_rows"}
    # the cases that REACH each node -- no fallback in front of it -- see every layout and every gradient form, the two that
    # select other code in a backward (blocks of one buffer; both outputs) at L >= 1, and an offset table under as_strided
    reach = {"then": lambda c: expected_path(c).one_node,                                 # _MeanPartsRowsThenItemRows
             "parts_rows": lambda c: c.switch == "none" and expected_path(c).pull_last,   # _LightGCNMeanPartsRows, last layer pulled
             "parts": lambda c: c.switch == "none"}                                       # _LightGCNMeanParts
    for op, reaches in reach.items():
        mine = [c for c in cs if c.op == op and reaches(c)]
        assert {c.storage for c in mine} == set(STORAGE) and {c.grads for c in mine} == set(GRADS), op
        assert {c.grads for c in mine if c.L >= 1} >= {"one_buffer", "both"}, op
        assert {c.storage for c in mine if c.L >= 1} == set(STORAGE), op
        assert {c.symmetric for c in mine if c.L >= 1} == {True, False}, op
        for grads in ("one_buffer", "both"):                                              # ... on adjacent and on separate tables
            assert {expected_path(c).adjacent for c in mine if c.grads == grads} == {True, False}, (op, grads)
    assert sum(c.op == "parts" and c.switch == "perm_g" for c in cs) == 2
    for op, switches in SWITCHES_OF.items():
        assert {c.switch for c in cs if c.op == op} == set(switches) | {"none"}, op
    assert {c.d for c in cs if c.op == "parts_rows"} == set(WIDTHS) == {c.d for c in cs if c.op == "spmm_rows"}
    assert any(c.op == "parts_rows" and c.plan == "multi" and c.d < 64 and c.L >= 1 and expected_path(c).rows_class for c in cs)
    one = [c for c in cs if c.op == "then" and expected_path(c).one_node]
    assert {c.plan for c in one} == set(PLANS) and {c.L for c in one} == {1, 2, 3, 4}
    assert {c.symmetric for c in one} == {True, False} and {c.exact for c in one} == {True, False}
    assert len({c.list for c in one}) >= 4
    two = [c for c in cs if c.op == "then" and not expected_path(c).one_node]
    assert {expected_path(c).spmm_rows_fast for c in two} == {True, False}
    assert {expected_path(c).rows_class for c in two} == {True, False}
    assert {c.plan for c in cs if c.L == 1 and c.exact} == set(PLANS) and all(c.exact for c in cs if c.L == 1)
    assert {c.op for c in cs if c.L == 1 and c.plan == "multi"} == set(OPS)
    assert sum(c.L == 3 and c.exact for c in cs) == 4
    assert {c.positive for c in cs if not c.exact} == {True, False}
    for c in cs:
        assert c.nu != c.ni and 1450 <= c.n <= 3000 and c.B <= 257
        assert (c.B == 0) == (c.list == "empty_batch") and (c.B == 1) == (c.list == "one_id")
        if c.plan == "multi":
            assert sorted(c.g_deg[c.nu + np.array(list(c.hubs))]) == sorted(HUBS)
            if c.B >= 16:
                assert set(c.hubs) <= set(c.item_rows.tolist())
        if c.list == "dup_users":
            assert np.bincount(c.users).max() >= 3
        if c.list == "pos_is_neg":
            assert np.intersect1d(c.item_rows[:c.B], c.item_rows[c.B:]).size >= 1
        if c.list == "hub_repeated":
            assert np.bincount(c.item_rows).max() >= 4
        if c.list == "empty_row":
            assert c.g_deg[c.users].min() == 0 and c.g_deg[c.nu + c.item_rows].min() == 0 and c.mm_deg[c.item_rows].min() == 0
        if c.list == "ends":
            assert c.rows.min() == 0 and c.rows.max() == c.n - 1
        if c.switch == "mm_beyond":
            assert c.mm_deg.max() == ROWS_MAX_CHUNKS * CHUNK + 1 and not c.exact and not expected_path(c).serv_m
            assert c.mm_item in c.item_rows


# ------------------------------------------------------------------------------------------------ GPU: the fuzz
@pytest.mark.gpu
@pytest.mark.parametrize("k", range(CASES))
def test_batch_rows_fuzz(k):
    from mmrec_amd import hip_ops
    c = case(k)
    got = run_case(c, hip_ops, torch.device("cuda:0"), True)
    print(describe(c, accept(c, got, gpu_depths(c))))


# every (layout, gradient form) pair; L on a period of its own: every depth with every layout and every gradient form
LAYERGCN_CASES = [(STORAGE[i % 4], GRADS[i % 5], 1 + (i // 5) % 4) for i in range(20)]
_LAYERGCN_REF = {}


def run_layergcn(hip_ops, to_dev, storage, grads, L):
    """layergcn_sum_parts forward and backward against the float64 autograd restatement of the SpMM fuzz (`_layergcn64`) on
    its graph (symmetric, positive values, hub rows of several chunks, empty rows, zero ego rows -- one at each side of the
    split), by its criterion: every row within 1e-4 of a norm -- the forward of the products the cosines re-weight, the
    gradient of its own row.  The reference is computed once per (L, gradient form)"""
    rng = np.random.default_rng(90 + L)
    nu, ni = 700, 500
    n = nu + ni
    g, A = _square_graph(rng, n, 9000, {0: 1400, 900: 600}, [3, 4, n - 1], signed=False)
    if (L, grads) not in _LAYERGCN_REF:
        E0 = (rng.standard_normal((n, 64)) * 0.1).astype(np.float32)
        E0[[5, 6, 4, nu, nu - 1]] = 0.0
        G = rng.standard_normal((n, 64)).astype(np.float32)
        if grads == "user_only":
            G[nu:] = 0.0
        elif grads == "item_only":
            G[:nu] = 0.0
        coo = A.tocoo()
        A64 = torch.sparse_coo_tensor(torch.from_numpy(np.stack([coo.row, coo.col]).astype(np.int64)),
                                      torch.from_numpy(coo.data), (n, n)).coalesce()
        E64 = torch.from_numpy(E0.astype(np.float64)).requires_grad_()
        ref, mag = _layergcn64(A64, E64, L)
        ref.backward(torch.from_numpy(G.astype(np.float64)))
        _LAYERGCN_REF[(L, grads)] = types.SimpleNamespace(nu=nu, E0=E0, G=G, ref=ref.detach().numpy(), mag=mag.numpy(),
                                                          dE=E64.grad.numpy())
    r = _LAYERGCN_REF[(L, grads)]
    U, I = tables((r.E0[:r.nu], r.E0[r.nu:]), storage, to_dev)
    Uo, Io = hip_ops.layergcn_sum_parts(g, (U, I), L)
    out = torch.cat((Uo.detach(), Io.detach())).cpu().double().numpy()
    send_gradients((Uo, Io), (r.G[:r.nu], r.G[r.nu:]), grads, to_dev)
    dE = torch.cat((U.grad, I.grad)).cpu().double().numpy()
    worst = []
    for name, got, want, scale in (("forward", out, r.ref, r.mag), ("dE0", dE, r.dE, r.dE)):
        row = np.linalg.norm(scale, axis=1, keepdims=True)
        err = np.abs(got - want)
        worst.append(float((err / np.maximum(row, 1e-300)).max()))
        assert np.all(err <= 1e-4 * row), (name, storage, grads, L, worst[-1])
    print("layergcn_sum_parts L %d %s %s: worst err / row norm forward %.3e dE0 %.3e" % (L, storage, grads, *worst))
    return g, (U, I), Uo


@pytest.mark.gpu
@pytest.mark.parametrize("storage,grads,L", LAYERGCN_CASES)
def test_layergcn_sum_parts_vs_float64_autograd(storage, grads, L):
    from mmrec_amd import hip_ops
    g, (U, I), Uo = run_layergcn(hip_ops, _on, storage, grads, L)
    assert g.n_chunks > g.n_long and _fn(Uo) == "_LayerGCNSumPartsBackward"
    assert hip_ops.row_blocks_of_one_buffer((U, I)) == (storage in ("adjacent", "offset"))
