"""Host side of the MI355X hot path: torch tensors in, HIP kernels (libmmrec_hip.so, C ABI) out.

Every op here enqueues hand-written gfx950 kernels on torch's current stream through ctypes and is
wrapped in a `torch.autograd.Function` so the reference's `Trainer` (one Adam over
`model.parameters()`, trainer.py:111-128) works unchanged.  There is no CPU or eager fallback: a
missing library or a CPU tensor raises.

Reference call sites each op replaces are cited in include/mmrec_hip.h.
"""
from __future__ import annotations

import ctypes
import math

import numpy as np
import torch

from . import _lib

EMB_DIM = 64
# The 4096 -> 64 projection's forward on the 16-bit matrix cores with split operands (x = hi + 2^-11 lo' in fp16, three fp16 MFMA
# products per 16 k; as accurate against float64 as the fp32-MFMA kernel, which is bound by the 1/16-rate fp32 matrix pipe and
# not by the stream of X).  Rows / weights outside fp16's range -- |.| >= 65520, inf, NaN, a whole row below 2^-10 -- are found on
# the device and recomputed by the fp32 kernel inside the same call (csrc/gemm.hip), so the result is fp32-accurate over all of
# fp32's range.  False (config `hip_linear_split: False`): the fp32 kernel for everything.
LINEAR_F16X3_DEFAULT = True       # what `hip_linear_split: null` means (the Trainer applies the config value on every build)
LINEAR_F16X3 = LINEAR_F16X3_DEFAULT
SLICE_WIDTHS = (8, 16, 32)    # one feature slice of a 64-wide table: 64 / P columns per rank of the feature-sliced layout (csrc/spmm_narrow.hip)
SPMM_CHUNK = 512
LONG_ROW_DEFAULT = None    # by graph size, see default_long_row_threshold


def default_long_row_threshold(n_cols):
    """Rows with more nonzeros than this go to the chunk blocks (16 groups share the row) instead of one 16-lane group.
    Measured (tools/spmm_sweep.py, profiles/r02_spmm_plan_sweep.log): cache-resident graphs are bound by their longest
    serial gather chains -- 16 beats 64 by 30-38 % at Baby / Sports / Clothing size; HBM-sized graphs prefer 32 (-4 % at
    C5; 16 costs 12 % there: too many 256-thread workgroups for 20-nonzero rows).  A function of the COLUMN count only, so
    a graph and its row blocks (same columns) get the same plan: row shards stay bit-identical to the whole graph."""
    import os
    forced = os.environ.get("MMREC_LONG_ROW_THRESHOLD")      # measurement aid (tools/, A/B runs of bench.py)
    if forced:
        return int(forced)
    return 16 if n_cols <= (1 << 18) else 32


ROW_SCHEDULE_MIN_COLS = 1 << 18    # graphs with more columns get a row schedule (CsrGraph(row_schedule=None))
SPMM_KEY_DEG_MAX = 128             # MMREC_SPMM_KEY_DEG_MAX: a column gathered by more rows than this is never a row's key


def spmm_key_deg_max():
    """The largest column degree a row-schedule key may have.  Measured flat over 64 / 128 / 256 (tools/prof_spmm_row_order.py
    --key-deg-max); the environment override is a measurement aid like MMREC_LONG_ROW_THRESHOLD."""
    import os
    forced = os.environ.get("MMREC_SPMM_KEY_DEG_MAX")
    return int(forced) if forced else SPMM_KEY_DEG_MAX


TOPK_MAX = 128            # MMREC_TOPK_MAX: row widths that are a multiple of 32 with <= 2,097,152 candidates; 64 for every other shape (the library says so: MMREC_ERR_UNSUPPORTED)
BPR_LOGSIG, BPR_GAMMA = 0, 1

# `hip_deterministic` (config key; Trainer sets it): the backward scatters of the fused loss kernels (BPR, cosine, InfoNCE,
# gather-norm) add with hardware fp32 atomics, so a batch with duplicated ids is order-dependent in the last ulp and a
# training run is not bitwise repeatable, although the reference's CPU path is.  In deterministic mode the same
# kernels run on the batch's GATHERED rows with identity ids (every output row written once) and the rows are scattered into
# the tables by mmrec_scatter_add_rows_sorted_f32: duplicates summed in position order by one owner, no atomics.
DETERMINISTIC_DEFAULT = False     # what `hip_deterministic: null` means (the Trainer passes the config value on every build)
DETERMINISTIC = DETERMINISTIC_DEFAULT
_TORCH_DET_BY_US = False


def set_deterministic(flag=True):
    """Process-wide switch.  Also puts torch's own scatter ops around the kernels (index_add & co.) into their
    deterministic mode -- and takes them out of it again only if this function put them there."""
    global DETERMINISTIC, _TORCH_DET_BY_US
    DETERMINISTIC = bool(flag)
    if DETERMINISTIC and not torch.are_deterministic_algorithms_enabled():
        torch.use_deterministic_algorithms(True, warn_only=True)
        _TORCH_DET_BY_US = True
    elif not DETERMINISTIC and _TORCH_DET_BY_US:
        torch.use_deterministic_algorithms(False)
        _TORCH_DET_BY_US = False


def scatter_add_rows(ids, rows, out):
    """out[ids[b]] += rows[b], duplicates summed in position order (deterministic; ids < 0 skipped)"""
    lib = _lib.load()
    _chk(ids, torch.int64, "ids", 1)
    rows, out = _chk(rows.contiguous(), torch.float32, "rows", 2), _chk(out, torch.float32, "out", 2)
    order = torch.sort(ids, stable=True)[1]
    _lib.check(lib.mmrec_scatter_add_rows_sorted_f32(_p(order), _p(ids), _p(rows), ids.numel(), rows.shape[1], _p(out),
                                                     _stream()), "scatter_add_rows_sorted")
    return out


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _chk(t, dtype, name, dim=None):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise _lib.MMRecHipError("%s must be a device tensor (the hot path has no CPU fallback)" % name)
    if t.dtype != dtype:
        raise _lib.MMRecHipError("%s must be %s, got %s" % (name, dtype, t.dtype))
    if not t.is_contiguous():
        raise _lib.MMRecHipError("%s must be contiguous" % name)
    if dim is not None and t.dim() != dim:
        raise _lib.MMRecHipError("%s must be %d-d" % (name, dim))
    return t


def _dev_table(t, width=None, max_rows=None):
    """the operand test of the `*_served` predicates: a device fp32 contiguous 2-D tensor, of `width` columns and at most
    `max_rows` rows where given"""
    return bool(isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float32 and t.dim() == 2 and t.is_contiguous()
                and (width is None or t.shape[1] == width) and (max_rows is None or t.shape[0] <= max_rows))


def _fuser_table(t):
    """a whole-table fuser's operand (csrc/tile64.h): a device fp32 contiguous [n, 64] table, 1 <= n <= 2^30"""
    return _dev_table(t, EMB_DIM, 1 << 30) and t.shape[0] >= 1


def _dev_tensor(t, shape):
    """a device fp32 contiguous tensor of this shape"""
    return bool(isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and
                tuple(t.shape) == shape)


def _ws(nbytes, device):
    return torch.empty(max(int(nbytes), 16), dtype=torch.uint8, device=device)


# ------------------------------------------------------------------------------------------------
# CSR graph container (+ long-row plan)
# ------------------------------------------------------------------------------------------------
class CsrGraph:
    """Device CSR (int32 rowptr/colidx, fp32 vals) + the long-row plan the SpMM kernel wants.

    `symmetric=True` (structure and values; all D^-1/2 A D^-1/2 graphs) lets the
    backward reuse the same CSR; otherwise `transpose()` builds A^T once (graphs are frozen or
    rebuilt once per epoch).

    `row_schedule` (None: graphs with more than ROW_SCHEDULE_MIN_COLS columns -- a function of the column count, like the
    long-row threshold, so a graph and its row blocks decide alike; True / False: forced): the plan also holds a VISITING ORDER
    of the short rows in which rows that gather the same cold column are neighbours, with a packed copy of
    those rows' (column, value) entries in that order, and the 64 k-wide launches walk it.  Results are bit-identical to the
    identity order (each row sums the same entries in the same order).  It costs device memory: 8 B per short nonzero + 12 B
    per short row ON TOP of the CSR (about 131 MB at config 5: 14.2M short nonzeros, 1.46M short rows) and one plan-time
    pass (a key kernel, one sort, one gather).  The copy holds `vals` as they were at construction: a caller that swaps
    `g.vals` afterwards (spmm_vals, the DynGraph forms) is served by the identity path."""

    def __init__(self, rowptr, colidx, vals, n_rows, n_cols, symmetric=False,
                 long_row_threshold=LONG_ROW_DEFAULT, rowptr_host=None, row_schedule=None):
        self.rowptr = _chk(rowptr, torch.int32, "rowptr", 1)
        self.colidx = _chk(colidx, torch.int32, "colidx", 1)
        self.vals = _chk(vals, torch.float32, "vals", 1)
        self.n_rows, self.n_cols = int(n_rows), int(n_cols)
        self.nnz = int(colidx.numel())
        self.symmetric = bool(symmetric)
        self.long_row_threshold = int(default_long_row_threshold(self.n_cols) if long_row_threshold is None
                                      else long_row_threshold)
        self._t = self if symmetric else None
        self.row_schedule = bool(self.n_cols > ROW_SCHEDULE_MIN_COLS if row_schedule is None else row_schedule)
        self._plan(rowptr_host)

    # -- plan: rows longer than the threshold are cut into fixed-size chunks (host side, C helper)
    def _plan(self, rowptr_host):
        lib = _lib.load()
        rp = rowptr_host if rowptr_host is not None else self.rowptr.cpu().numpy()
        rp = np.ascontiguousarray(rp, dtype=np.int32)
        self.rowptr_host = rp
        n_long, n_chunks = ctypes.c_int32(0), ctypes.c_int32(0)
        _lib.check(lib.mmrec_spmm_plan_count(rp.ctypes.data_as(ctypes.c_void_p), self.n_rows,
                                             self.long_row_threshold, ctypes.byref(n_long),
                                             ctypes.byref(n_chunks)), "spmm_plan_count")
        self.n_long, self.n_chunks = n_long.value, n_chunks.value
        dev = self.rowptr.device
        if self.n_long > 0:
            lr = np.empty(self.n_long, dtype=np.int32)
            cp = np.empty(self.n_long + 1, dtype=np.int32)
            _lib.check(lib.mmrec_spmm_plan_fill(rp.ctypes.data_as(ctypes.c_void_p), self.n_rows,
                                                self.long_row_threshold,
                                                lr.ctypes.data_as(ctypes.c_void_p),
                                                cp.ctypes.data_as(ctypes.c_void_p)), "spmm_plan_fill")
            self.long_rows = torch.from_numpy(lr).to(dev)
            self.long_chunk_ptr = torch.from_numpy(cp).to(dev)
            self.max_row_chunks = int(np.diff(cp).max())          # chunks of the longest row (mmrec_spmm_rows_any_f32)
            # last-arriver counters of the multi-chunk rows (the launch finishes such a row itself): zero now, left at zero
            # by every launch
            self.long_tickets = torch.zeros(self.n_long, dtype=torch.int32, device=dev)
        else:
            self.long_rows = self.long_chunk_ptr = self.long_tickets = None
            self.max_row_chunks = 1
        self._partials = {}
        self.sched = None
        if self.row_schedule:
            self._plan_schedule()

    def _plan_schedule(self):
        """The visiting order of the short rows and their packed index stream (device work: one key kernel, torch sorts).

        key(row) = among the row's columns gathered by at most spmm_key_deg_max() rows the one gathered by the MOST rows (the
        first in row order among equals): L2 keeps the popular columns whatever the order, a cold one is fetched once per row
        that gathers it unless those rows run together.  Order: stable sort of the short rows by (band, key degree
        descending, key, row id), rows without a key last in their band -- the rows of one key fill consecutive slots, so one
        or two row blocks, and the big groups come first.  Band 0: rows whose reference column (the key; for a row without
        one its first column) has a LARGER id than the row; band 1: everything else (empty rows too).  On a [users; items]
        bipartite layout that is all user rows before all item rows, the phase order the identity launch has
        (profiles/r07_spmm_phases.log: mixing the two costs 2-25 %); on other graphs it is merely a fixed rule."""
        lib = _lib.load()
        dev, n = self.rowptr.device, self.n_rows
        deg = (self.rowptr[1:] - self.rowptr[:-1])
        short = torch.nonzero(deg <= self.long_row_threshold).squeeze(1)               # ascending row ids (int64)
        key = torch.full((n,), -1, dtype=torch.int32, device=dev)
        kdeg = torch.zeros(n, dtype=torch.int32, device=dev)
        if self.nnz > 0 and n > 0:
            if self.symmetric and self.n_cols == n:
                coldeg = deg.contiguous()
            else:
                coldeg = torch.bincount(self.colidx, minlength=self.n_cols).to(torch.int32)
            _lib.check(lib.mmrec_spmm_row_keys(_p(self.rowptr), _p(self.colidx), _p(coldeg), n, self.long_row_threshold,
                                               spmm_key_deg_max(), _p(key), _p(kdeg), _stream()), "spmm_row_keys")
        self.row_key, self.row_key_degree = key, kdeg          # the hook for other keys (community labels): a follow-up
        k, kd, dg = key[short].long(), kdeg[short].long(), deg[short].long()
        first = self.colidx[self.rowptr[:-1][short].long().clamp_(max=max(self.nnz - 1, 0))].long() if self.nnz > 0 else k
        ref = torch.where(k >= 0, k, torch.where(dg > 0, first, torch.full_like(k, -1)))
        band = (ref <= short).long()
        # one 63-bit composite: band | 2^31 - 1 - key degree (no key: degree 0, last) | key ; the stable sort keeps row ids ascending
        comp = (band << 62) | (((1 << 31) - 1 - kd) << 31) | k.clamp(min=0)
        order = torch.sort(comp, stable=True)[1]
        rows = short[order]
        lens = dg[order]
        end = torch.cumsum(lens, 0)
        begin = end - lens
        total = int(end[-1].item()) if rows.numel() else 0
        src0 = self.rowptr[:-1].long()[rows]
        pos = torch.arange(total, dtype=torch.int64, device=dev) + torch.repeat_interleave(src0 - begin, lens, output_size=total)
        self.sched = {
            "row": rows.to(torch.int32).contiguous(),
            "span": torch.stack([begin, end], 1).to(torch.int32).contiguous(),
            "col": self.colidx.index_select(0, pos) if total else torch.zeros(1, dtype=torch.int32, device=dev),
            "val": self.vals.index_select(0, pos) if total else torch.zeros(1, dtype=torch.float32, device=dev),
            "n_short": int(rows.numel()),
            "vals_of": self.vals,       # the values the copy was packed from (see scheduled())
        }

    def scheduled(self, d):
        """the schedule, if this launch may use it: 64 k-wide rows, and `vals` still the tensor the schedule packed"""
        sc = self.sched
        return sc if sc is not None and d % EMB_DIM == 0 and sc["vals_of"] is self.vals else None

    def schedule_bytes(self):
        return 0 if self.sched is None else sum(self.sched[k].numel() * self.sched[k].element_size() for k in ("row", "span", "col", "val"))

    def checked(self, rc, what):
        """_lib.check for a launch that uses the last-arriver tickets: they are left at zero by every COMPLETED launch; after a
        failed one they are re-zeroed here, or every later SpMM on this graph would finish its long rows on a stale count."""
        try:
            _lib.check(rc, what)
        except _lib.MMRecHipError:
            if self.long_tickets is not None:
                try:
                    self.long_tickets.zero_()
                except RuntimeError:
                    pass                         # (a faulted device: nothing more will run on it anyway)
            raise

    def partials_for(self, d):
        """long-row workspace (n_chunks x d fp32), allocated once per embedding width"""
        if self.n_long == 0:
            return None
        if d not in self._partials:
            self._partials[d] = torch.empty(self.n_chunks * d, dtype=torch.float32, device=self.rowptr.device)
        return self._partials[d]

    @classmethod
    def from_coo_host(cls, idx, val, n_rows, n_cols, device, symmetric=False, **kw):
        """Stable COO->CSR on the host (numpy): entries of a row keep their COO order."""
        idx = np.asarray(idx, dtype=np.int64)
        val = np.asarray(val, dtype=np.float32)
        order = np.argsort(idx[0], kind="stable")
        rowptr = np.zeros(n_rows + 1, dtype=np.int64)
        np.cumsum(np.bincount(idx[0], minlength=n_rows), out=rowptr[1:])
        rp = rowptr.astype(np.int32)
        return cls(torch.from_numpy(rp).to(device),
                   torch.from_numpy(idx[1][order].astype(np.int32)).to(device),
                   torch.from_numpy(val[order]).to(device), n_rows, n_cols, symmetric=symmetric,
                   rowptr_host=rp, **kw)

    @classmethod
    def from_coo_device(cls, rows, cols, vals, n_rows, n_cols, symmetric=False, **kw):
        """Stable COO->CSR on the device (rocPRIM radix sort by row key inside the library)."""
        lib = _lib.load()
        _chk(rows, torch.int32, "rows", 1), _chk(cols, torch.int32, "cols", 1)
        _chk(vals, torch.float32, "vals", 1)
        nnz, dev = rows.numel(), rows.device
        rowptr = torch.empty(n_rows + 1, dtype=torch.int32, device=dev)
        colidx = torch.empty(nnz, dtype=torch.int32, device=dev)
        vout = torch.empty(nnz, dtype=torch.float32, device=dev)
        ws = _ws(lib.mmrec_coo_to_csr_workspace_bytes(nnz, n_rows), dev)
        _lib.check(lib.mmrec_coo_to_csr(_p(rows), _p(cols), _p(vals), nnz, n_rows, _p(rowptr),
                                        _p(colidx), _p(vout), _p(ws), _stream()), "coo_to_csr")
        return cls(rowptr, colidx, vout, n_rows, n_cols, symmetric=symmetric, **kw)

    def to_coo_host(self):
        rp = self.rowptr_host.astype(np.int64)
        rows = np.repeat(np.arange(self.n_rows, dtype=np.int64), np.diff(rp))
        return np.stack([rows, self.colidx.cpu().numpy().astype(np.int64)]), self.vals.cpu().numpy()

    def transpose(self):
        if self._t is None:
            idx, val = self.to_coo_host()
            self._t = CsrGraph.from_coo_host(idx[::-1], val, self.n_cols, self.n_rows,
                                             self.rowptr.device,
                                             long_row_threshold=self.long_row_threshold)
            self._t._t = self
        return self._t

    def row_block(self, r0, r1):
        """Rows [r0, r1) as their own CSR (column ids stay global): one rank's shard of a row-sharded
        graph.  Per-row data and order are untouched, so results equal the unsharded rows bit for bit."""
        rp = self.rowptr_host.astype(np.int64)
        s, e = int(rp[r0]), int(rp[r1])
        rph = (rp[r0:r1 + 1] - s).astype(np.int32)
        dev = self.rowptr.device
        return CsrGraph(torch.from_numpy(rph).to(dev), self.colidx[s:e].contiguous(),
                        self.vals[s:e].contiguous(), r1 - r0, self.n_cols,
                        long_row_threshold=self.long_row_threshold, rowptr_host=rph, row_schedule=self.row_schedule)


def _mode_labels(rows, lab_c, n_rows, n_labels):
    """for every row the most frequent label among its neighbours (ties: the smallest label); -1 for rows without any"""
    key = rows.astype(np.int64) * n_labels + lab_c
    key.sort()
    start = np.flatnonzero(np.concatenate([[True], key[1:] != key[:-1]]))
    cnt = np.diff(np.concatenate([start, [key.shape[0]]]))
    k = key[start]
    r, lab = k // n_labels, k % n_labels
    o = np.lexsort((lab, -cnt, r))               # per row: highest count first, then the smallest label
    r_s = r[o]
    first = np.concatenate([[True], r_s[1:] != r_s[:-1]])
    out = np.full(n_rows, -1, dtype=np.int64)
    out[r_s[first]] = lab[o][first]
    return out


def _mode_labels_device(rows, lab_c, n_rows, n_labels):
    """_mode_labels on the device (torch sorts of int64 keys: integer exact, the same answer): two sorts of nnz keys per sweep,
    milliseconds where the numpy form takes ~1 s per sweep at 20M nonzeros (7.4 s of a config-5 model build)."""
    key, _ = torch.sort(rows * n_labels + lab_c)
    uk, cnt = torch.unique_consecutive(key, return_counts=True)
    r, lab = torch.div(uk, n_labels, rounding_mode='floor'), uk % n_labels
    cmax = int(cnt.max().item()) + 1
    # per row: highest count first, then the smallest label -- one more sort of (row, cmax - count, label) packed in 63 bits
    if n_rows * cmax * n_labels >= 2 ** 62:
        raise OverflowError("label-propagation key does not fit 63 bits")
    k2, _ = torch.sort(r * (cmax * n_labels) + (cmax - cnt) * n_labels + lab)
    r2 = torch.div(k2, cmax * n_labels, rounding_mode='floor')
    first = torch.ones_like(r2, dtype=torch.bool)
    first[1:] = r2[1:] != r2[:-1]
    out = torch.full((n_rows,), -1, dtype=torch.int64, device=rows.device)
    out[r2[first]] = (k2 % n_labels)[first]
    return out


def locality_order(rowptr_host, colidx_host, n, how, n_left=None, iters=4, device=None):
    """A relabelling of the n nodes of a SQUARE graph for gather locality (round-3 review item 5): new id = perm[old id].
      'degree'     ids by descending degree (hot rows share cache lines and pages);
      'rcm'        reverse Cuthill-McKee on the structure (scipy.sparse.csgraph): good for mesh-like graphs, not for
                   interaction graphs (a few random edges make every BFS level the whole graph);
      'community'  `iters` rounds of label propagation (a node takes its neighbours' most frequent label), nodes then
                   ordered by label: the members of a community get adjacent ids, so the rows a workgroup gathers are the
                   rows its neighbours in the grid gather.  Bipartite graphs (`n_left`: ids below it are one side) update one
                   side from the other in turn.  A graph without communities just gets some permutation.
    Integer, deterministic; `device` (a CUDA device): the label-propagation sweeps run there (same permutation)."""
    rp = np.asarray(rowptr_host, dtype=np.int64)
    deg = np.diff(rp)
    ci = np.asarray(colidx_host, dtype=np.int64)
    if how == "degree":
        order = np.argsort(-deg, kind="stable")               # order[new] = old
    elif how == "rcm":
        import scipy.sparse as sp
        from scipy.sparse.csgraph import reverse_cuthill_mckee
        a = sp.csr_matrix((np.ones(ci.shape[0], dtype=np.int8), ci.astype(np.int32), rp.astype(np.int32)), shape=(n, n))
        order = np.asarray(reverse_cuthill_mckee(a, symmetric_mode=True), dtype=np.int64)
    elif how == "community" and device is not None and torch.device(device).type == "cuda":
        dev = torch.device(device)
        rows = torch.repeat_interleave(torch.arange(n, dtype=torch.int64, device=dev), torch.from_numpy(deg).to(dev))
        cols = torch.from_numpy(ci).to(dev)
        lab = torch.arange(n, dtype=torch.int64, device=dev)
        sides = [None] if not n_left else [rows < n_left, rows >= n_left]
        for _ in range(int(iters)):
            for side in sides:                                 # (bipartite: left from right, then right from the new left)
                r_s, c_s = (rows, cols) if side is None else (rows[side], cols[side])
                new = _mode_labels_device(r_s, lab[c_s], n, n)
                lab = torch.where(new >= 0, new, lab)
        order = torch.sort(lab, stable=True)[1].cpu().numpy()      # = np.lexsort((arange(n), lab))
    elif how == "community":
        rows = np.repeat(np.arange(n, dtype=np.int64), deg)
        lab = np.arange(n, dtype=np.int64)
        sides = [slice(None)] if not n_left else [rows < n_left, rows >= n_left]
        for _ in range(int(iters)):
            for side in sides:                                 # (bipartite: left from right, then right from the new left)
                new = _mode_labels(rows[side], lab[ci[side]], n, n)
                lab = np.where(new >= 0, new, lab)
        order = np.lexsort((np.arange(n), lab))
    else:
        raise ValueError("reorder must be 'degree', 'rcm' or 'community', got %r" % (how,))
    perm = np.empty(n, dtype=np.int64)
    perm[order] = np.arange(n, dtype=np.int64)
    return perm


class PermutedGraph:
    """A square CsrGraph with its node ids RELABELLED at build time (`reorder`: 'degree' | 'rcm' | 'community'; locality_order) and the
    permutation kept next to it.  Rows keep their nonzeros in their original order (stable relabelling), so every row's sum
    is the unpermuted graph's bit for bit: `lightgcn_mean(pg, E0, L)` / `spmm(pg, X)` permute the input once, run all
    layers in the relabelled space and permute the result back -- equal to the plain graph's results BITWISE."""

    def __init__(self, g: CsrGraph, reorder, n_left=None):
        if g.n_rows != g.n_cols:
            raise _lib.MMRecHipError("PermutedGraph needs a square graph")
        dev, n = g.rowptr.device, g.n_rows
        idx, val = g.to_coo_host()
        perm = locality_order(g.rowptr_host, idx[1], n, reorder, n_left=n_left)
        self.base, self.reorder = g, reorder
        self.perm = torch.from_numpy(perm).to(dev)                     # new id of old node
        inv = np.empty(n, dtype=np.int64)
        inv[perm] = np.arange(n, dtype=np.int64)
        self.inv = torch.from_numpy(inv).to(dev)                       # old node of new id
        self.graph = CsrGraph.from_coo_host(np.stack([perm[idx[0]], perm[idx[1]]]), val, n, n, dev, symmetric=g.symmetric,
                                            long_row_threshold=g.long_row_threshold)     # stable: in-row order kept
        self.n_rows = self.n_cols = n
        self.nnz = g.nnz

    def to_new(self, X):
        return X.index_select(0, self.inv)

    def to_old(self, Xp):
        return Xp.index_select(0, self.perm)


def spmm_raw(g: CsrGraph, X, Y=None, Z=None, acc_in=None, acc_out=None, alpha=1.0, beta=1.0,
             acc_scale=1.0):
    """Y = alpha*A@X (+ beta*Z);  acc_out = acc_scale*(acc_in + Y).  No autograd."""
    lib = _lib.load()
    _chk(X, torch.float32, "X", 2)
    d = X.shape[1]
    if (d not in SLICE_WIDTHS and (d % EMB_DIM or d > 6 * EMB_DIM)) or X.shape[0] < g.n_cols:
        raise _lib.MMRecHipError("X must be [>=%d, 64*k <= 384 (or a feature slice of 8 / 16 / 32 columns)], got %s" %
                                 (g.n_cols, tuple(X.shape)))
    for t, nm in ((Y, "Y"), (Z, "Z"), (acc_in, "acc_in"), (acc_out, "acc_out")):
        if t is not None:
            _chk(t, torch.float32, nm, 2)
            if t.shape[0] < g.n_rows or t.shape[1] != d:
                raise _lib.MMRecHipError("%s must be [>=%d, %d]" % (nm, g.n_rows, d))
    sc = g.scheduled(d)
    if sc is not None:      # large graph: the row blocks visit the short rows in the plan's order (same bits)
        g.checked(lib.mmrec_spmm_csr_sched_f32(_p(g.rowptr), _p(g.colidx), _p(g.vals), _p(X), _p(Y), _p(Z),
                                               _p(acc_in), _p(acc_out), g.n_rows, d, float(alpha),
                                               float(beta), float(acc_scale), g.long_row_threshold,
                                               _p(g.long_rows), _p(g.long_chunk_ptr), g.n_long, g.n_chunks,
                                               _p(g.partials_for(d)), _p(g.long_tickets), _p(sc["row"]), _p(sc["span"]),
                                               _p(sc["col"]), _p(sc["val"]), sc["n_short"], _stream()), "spmm_csr_sched_f32")
        return Y if Y is not None else acc_out
    g.checked(lib.mmrec_spmm_csr_f32(_p(g.rowptr), _p(g.colidx), _p(g.vals), _p(X), _p(Y), _p(Z),
                                     _p(acc_in), _p(acc_out), g.n_rows, d, float(alpha),
                                     float(beta), float(acc_scale), g.long_row_threshold,
                                     _p(g.long_rows), _p(g.long_chunk_ptr), g.n_long, g.n_chunks,
                                     _p(g.partials_for(d)), _p(g.long_tickets), _stream()), "spmm_csr_f32")
    return Y if Y is not None else acc_out


ROWS_MAX_CHUNKS = 480      # mmrec_spmm_rows_any_f32 keeps a listed row's chunk partials in LDS (256 B each)


def rows_servable(g: CsrGraph, d):
    """can the row-list kernels reproduce the full launch's bits on this graph?  Every width they have when no row spans
    several chunks (mmrec_spmm_rows_f32); d = 64 also with such rows, up to ROWS_MAX_CHUNKS chunks (mmrec_spmm_rows_any_f32)"""
    if d not in SLICE_WIDTHS + (EMB_DIM,):
        return False
    return g.n_chunks == g.n_long or (d == EMB_DIM and g.max_row_chunks <= ROWS_MAX_CHUNKS)


def spmm_rows_raw(g: CsrGraph, X, rows, Z=None, z_compact=False):
    """(A @ X)[rows] (+ Z[rows], or + Z for a compact Z [len(rows), d]) as a compact [len(rows), d] tensor -- the bits of
    spmm_raw(g, X, Z=Z)[rows], computed for the listed rows only (a training step that reads a propagated table at its batch
    rows).  No autograd."""
    lib = _lib.load()
    _chk(X, torch.float32, "X", 2), _chk(rows, torch.int64, "rows", 1)
    d = X.shape[1]
    if not rows_servable(g, d) or X.shape[0] < g.n_cols:
        raise _lib.MMRecHipError("spmm_rows: graph with multi-chunk rows, or X not [>=%d, 8 / 16 / 32 / 64]" % g.n_cols)
    if Z is not None and (_chk(Z, torch.float32, "Z", 2).shape[0] < (rows.numel() if z_compact else g.n_rows) or Z.shape[1] != d):
        raise _lib.MMRecHipError("Z must be [>=%d, %d]" % (rows.numel() if z_compact else g.n_rows, d))
    Y = torch.empty(rows.numel(), d, dtype=torch.float32, device=X.device)
    long_t = g.long_row_threshold if g.n_long > 0 else 2 ** 31 - 1
    if g.n_chunks == g.n_long:
        _lib.check(lib.mmrec_spmm_rows_f32(_p(g.rowptr), _p(g.colidx), _p(g.vals), _p(X), _p(Z), 1 if z_compact else 0, _p(rows),
                                           rows.numel(), d, long_t, _p(Y), _stream()), "spmm_rows_f32")
    else:       # rows of several chunks among the graph's: a workgroup per such listed row (ABI 12)
        _lib.check(lib.mmrec_spmm_rows_any_f32(_p(g.rowptr), _p(g.colidx), _p(g.vals), _p(X), _p(Z), 1 if z_compact else 0, _p(rows),
                                               rows.numel(), d, long_t, g.max_row_chunks, _p(Y), _stream()), "spmm_rows_any_f32")
    return Y


def spmm_push_rows_raw(g: CsrGraph, G, rows, dX=None, dZ=None, scale=1.0):
    """dX[c] += A[r, c] * scale * G[i] over the nonzeros of the listed rows r = rows[i]; dZ[r] += scale * G[i] (fp32 atomics,
    in place; dZ may be dX).  Any graph (one workgroup per listed row)."""
    lib = _lib.load()
    _chk(G, torch.float32, "G", 2), _chk(rows, torch.int64, "rows", 1)
    d = G.shape[1]
    if G.shape[0] != rows.numel() or d not in SLICE_WIDTHS + (EMB_DIM,):
        raise _lib.MMRecHipError("G must be [len(rows), 8 / 16 / 32 / 64]")
    for t, nm, n in ((dX, "dX", g.n_cols), (dZ, "dZ", g.n_rows)):
        if t is not None and (_chk(t, torch.float32, nm, 2).shape[0] < n or t.shape[1] != d):
            raise _lib.MMRecHipError("%s must be [>=%d, %d]" % (nm, n, d))
    _lib.check(lib.mmrec_spmm_push_rows_f32(_p(g.rowptr), _p(g.colidx), _p(g.vals), _p(G), float(scale), _p(rows), rows.numel(),
                                            d, _p(dX), _p(dZ), _stream()), "spmm_push_rows_f32")


class _SpmmRows(torch.autograd.Function):
    """(A @ X)[rows] + Z_rows for a batch's rows (spmm_rows_raw); backward: dX by the transpose-free push through the listed
    rows into a zero-filled table, dZ_rows = the incoming gradient"""

    @staticmethod
    def forward(ctx, X, Z_rows, g, rows):
        ctx.g, ctx.x_shape, ctx.has_z = g, tuple(X.shape), Z_rows is not None
        ctx.save_for_backward(rows)
        return spmm_rows_raw(g, X.contiguous(), rows, None if Z_rows is None else Z_rows.contiguous(), z_compact=True)

    @staticmethod
    def backward(ctx, dY):
        rows, = ctx.saved_tensors
        dY = dY.contiguous()
        dX = None
        if ctx.needs_input_grad[0]:
            dX = torch.zeros(ctx.x_shape, dtype=dY.dtype, device=dY.device)
            spmm_push_rows_raw(ctx.g, dY, rows, dX=dX)
        return dX, (dY if ctx.has_z and ctx.needs_input_grad[1] else None), None, None


def spmm_rows(g: CsrGraph, X, rows, Z_rows=None):
    """(g @ X)[rows] (+ Z_rows, compact) -- differentiable in X and Z_rows -- for a training step that reads a propagated
    table at its batch rows only (FREEDOM's item-item layer, freedom.py:173-177 read at :197-199): the listed rows carry the
    full launch's bits, the backward pushes through them with fp32 atomics.  `hip_deterministic` runs, and graphs with rows
    spanning several chunks, take the full launch."""
    if DETERMINISTIC or isinstance(g, PermutedGraph) or not rows_servable(g, X.shape[1]):
        out = spmm(g, X).index_select(0, rows)
        return out if Z_rows is None else out + Z_rows
    return _SpmmRows.apply(X, Z_rows, g, rows)


class _SpMM(torch.autograd.Function):
    @staticmethod
    def forward(ctx, X, Z, g):
        ctx.g, ctx.has_z, ctx.x_rows = g, Z is not None, X.shape[0]
        X = X.contiguous()
        Y = torch.empty(g.n_rows, X.shape[1], dtype=torch.float32, device=X.device)
        spmm_raw(g, X, Y=Y, Z=None if Z is None else Z.contiguous(), beta=1.0)
        return Y

    @staticmethod
    def backward(ctx, dY):
        dY = dY.contiguous()
        gt = ctx.g.transpose()
        dX = None
        if ctx.needs_input_grad[0]:
            # X may carry more rows than the graph has columns (spmm_raw allows it): they receive no gradient
            alloc = torch.empty if ctx.x_rows == gt.n_rows else torch.zeros
            dX = alloc(ctx.x_rows, dY.shape[1], dtype=torch.float32, device=dY.device)
            spmm_raw(gt, dY, Y=dX)
        return dX, (dY if ctx.has_z and ctx.needs_input_grad[1] else None), None


def spmm(g: CsrGraph, X, Z=None):
    """A @ X (+ Z), differentiable in X and Z.  replaces torch.sparse.mm (freedom.py:167,172) and PyG's
    mean-aggregating propagate (mmgcn.py:205-213).  Row widths that are not a multiple of 64 are
    zero-padded for the kernel (aggregation is column-wise independent) and sliced back."""
    if isinstance(g, PermutedGraph):
        out = spmm(g.graph, g.to_new(X), None if Z is None else g.to_new(Z))
        return g.to_old(out)
    d = X.shape[1]
    if d % EMB_DIM and d not in SLICE_WIDTHS:
        pad = EMB_DIM - d % EMB_DIM
        Xp = torch.nn.functional.pad(X, (0, pad))
        Zp = None if Z is None else torch.nn.functional.pad(Z, (0, pad))
        return _SpMM.apply(Xp, Zp, g)[:, :d]
    return _SpMM.apply(X, Z, g)


class _LightGCNMean(torch.autograd.Function):
    """mean_l(A^l E0), l = 0..L, with the layer sum fused into the SpMM epilogue
    (lightgcn.py:115-128, freedom.py:169-176, bm3.py:87-93).  Backward is the Horner form
    dE0 = s*(g + A^T(g + A^T(...)))  with s = 1/(L+1), again L launches of the same kernel."""

    @staticmethod
    def forward(ctx, E0, g, n_layers):
        ctx.g, ctx.L = g, int(n_layers)
        E0 = E0.contiguous()
        L = ctx.L
        if L == 0:
            return E0.clone()
        acc = torch.empty_like(E0)
        bufs = [torch.empty_like(E0) if L > 1 else None, torch.empty_like(E0) if L > 2 else None]
        cur = E0
        for layer in range(1, L + 1):
            last = layer == L
            Y = None if last else bufs[(layer - 1) % 2]
            spmm_raw(g, cur, Y=Y, acc_in=E0 if layer == 1 else acc, acc_out=acc,
                     acc_scale=1.0 / (L + 1) if last else 1.0)
            cur = Y
        return acc

    @staticmethod
    def backward(ctx, dOut):
        L, gt = ctx.L, ctx.g.transpose()
        dOut = dOut.contiguous()
        if L == 0:
            return dOut, None, None
        s = 1.0 / (L + 1)
        bufs = [torch.empty_like(dOut), torch.empty_like(dOut) if L > 1 else None]
        t = dOut
        for j in range(L):  # t <- s*dOut + A^T t   (first step also scales the inner term)
            out = bufs[j % 2]
            spmm_raw(gt, t, Y=out, Z=dOut, alpha=s if j == 0 else 1.0, beta=s)
            t = out
        return t, None, None


def lightgcn_mean(g, E0, n_layers):
    if isinstance(g, PermutedGraph):      # relabelled graph: one permutation in, all layers in the new id space, one out
        return g.to_old(_LightGCNMean.apply(g.to_new(E0), g.graph, n_layers))
    return _LightGCNMean.apply(E0, g, n_layers)


def row_blocks_of_one_buffer(ts):
    """True if the tensors are consecutive contiguous row blocks of ONE allocation, i.e. their cat already exists"""
    if any(t is None or not t.is_contiguous() or t.dtype != ts[0].dtype for t in ts):
        return False
    base = ts[0].untyped_storage().data_ptr()
    end = ts[0].data_ptr()
    for t in ts:
        if t.untyped_storage().data_ptr() != base or t.data_ptr() != end:
            return False
        end += t.numel() * t.element_size()
    return end <= base + ts[0].untyped_storage().nbytes()


class _LightGCNMeanParts(torch.autograd.Function):
    """_LightGCNMean on the row-wise concatenation of several tables (user table, item table), returning the mean split
    back into the same row blocks.  The same launches; what goes away is autograd's bookkeeping around them at 1.5M rows:
    the zero-filled [N, 64] gradients of the two output slices and their sum, and the split of the cat's gradient."""

    @staticmethod
    def forward(ctx, g, n_layers, *parts):
        ctx.sizes = [p.shape[0] for p in parts]
        if row_blocks_of_one_buffer(parts):        # models/_base.py AdjacentTablesMixin: the cat already exists
            E0 = parts[0].detach().as_strided((sum(ctx.sizes), parts[0].shape[1]), (parts[0].shape[1], 1))
        else:
            E0 = torch.cat([p.detach() for p in parts], dim=0)
        ctx.g, ctx.L = g, int(n_layers)
        out = _LightGCNMean.forward(ctx, E0, g, n_layers)
        return tuple(out.split(ctx.sizes))

    @staticmethod
    def backward(ctx, *grads):
        like = next(x for x in grads if x is not None)
        n, d = sum(ctx.sizes), like.shape[1]
        if row_blocks_of_one_buffer(grads):       # e.g. bpr_losses_shared_users(joint_grad=True): already laid out as cat(grads)
            dOut = grads[0].as_strided((n, d), (d, 1))
        else:
            dOut = torch.empty((n, d), dtype=like.dtype, device=like.device)
            for dst, src in zip(dOut.split(ctx.sizes), grads):
                dst.zero_() if src is None else dst.copy_(src)
        t = _LightGCNMean.backward(ctx, dOut)[0]
        return (None, None) + tuple(t.split(ctx.sizes))


def lightgcn_mean_parts(g: CsrGraph, parts, n_layers):
    """mean_l(A^l cat(parts)) as a tuple of row blocks, one per input table (freedom.py:165-178: cat, propagate, split)"""
    if isinstance(g, PermutedGraph):      # the node launches on a CsrGraph: a relabelled graph goes through lightgcn_mean
        return tuple(lightgcn_mean(g, torch.cat(list(parts), dim=0), n_layers).split([p.shape[0] for p in parts]))
    return _LightGCNMeanParts.apply(g, n_layers, *parts)


ROWS_LAST_LAYER = True      # lightgcn_mean_parts_rows: last layer at the listed rows only (False: full launches + gather, A/B)


class _LightGCNMeanPartsRows(torch.autograd.Function):
    """lightgcn_mean_parts consumed at LISTED rows only (the batch's users and items): the forward is the full propagation
    (every layer feeds the next) followed by a gather of the listed rows; the BACKWARD starts from the compact gradient of those
    rows, so its first step -- A^T applied to a gradient that is zero outside <= 3B rows, a launch over all rows in
    _LightGCNMean.backward -- is a push through the listed rows into a zero-filled table (one workgroup per row: popular
    items' rows have thousands of nonzeros), and the dense [N, d] gradient of the mean never exists.  The remaining L - 1
    steps are the usual full launches."""

    @staticmethod
    def forward(ctx, g, n_layers, rows, *parts):
        ctx.sizes = [p.shape[0] for p in parts]
        if row_blocks_of_one_buffer(parts):
            E0 = parts[0].detach().as_strided((sum(ctx.sizes), parts[0].shape[1]), (parts[0].shape[1], 1))
        else:
            E0 = torch.cat([p.detach() for p in parts], dim=0)
        ctx.save_for_backward(rows)
        L = int(n_layers)
        if L >= 1 and ROWS_LAST_LAYER and rows_servable(g, E0.shape[1]) and E0.shape[0] == g.n_rows == g.n_cols:
            # Round 6: the LAST layer is read at the listed rows only -- it feeds no further layer -- so it is computed there
            # (spmm_rows_raw: the full launch's bits row by row, long rows included), with the epilogue's
            # s * (running layer sum + y) done on the compact rows: a launch over all rows less per step (0.30 of a
            # config-5 step's 2.35 ms).
            ctx.g, ctx.L = g, L
            E0 = E0.contiguous()
            cur, acc = E0, E0
            if L > 1:
                acc = torch.empty_like(E0)
                bufs = [torch.empty_like(E0), torch.empty_like(E0) if L > 2 else None]
                for layer in range(1, L):
                    Y = bufs[(layer - 1) % 2]
                    spmm_raw(g, cur, Y=Y, acc_in=E0 if layer == 1 else acc, acc_out=acc, acc_scale=1.0)
                    cur = Y
            return spmm_rows_raw(g, cur, rows, Z=acc) * (1.0 / (L + 1))
        out = _LightGCNMean.forward(ctx, E0, g, n_layers)
        return out.index_select(0, rows)

    @staticmethod
    def backward(ctx, dRows):
        rows, = ctx.saved_tensors
        L, g = ctx.L, ctx.g
        dRows = dRows.contiguous()
        n, d = sum(ctx.sizes), dRows.shape[1]
        s = 1.0 / (L + 1)
        t = torch.zeros((n, d), dtype=dRows.dtype, device=dRows.device)
        if L == 0:
            spmm_push_rows_raw(g, dRows, rows, dZ=t)
            return (None, None, None) + tuple(t.split(ctx.sizes))
        # t1 = s * (A^T G + G) with G = the listed rows' gradient scattered: pushed, never materialised
        spmm_push_rows_raw(g, dRows, rows, dX=t, dZ=t, scale=s)
        gt = g.transpose()
        for _ in range(1, L):          # t <- A^T t + s G
            out = torch.empty_like(t)
            spmm_raw(gt, t, Y=out)
            spmm_push_rows_raw(g, dRows, rows, dZ=out, scale=s)
            t = out
        return (None, None, None) + tuple(t.split(ctx.sizes))


class _MeanPartsRowsThenItemRows(torch.autograd.Function):
    """FREEDOM's training-step forward at the batch rows as ONE autograd node: at = lightgcn_mean_parts_rows(g, (user table, item
    table), L, cat(users, nu + item_rows)), then ia = (mm @ item table)[item_rows] + at[b:] (freedom.py:165-178 read at
    :197-199).  As two nodes the item table receives two dense gradients -- the propagation's block and a zero-filled
    [n_items, d] buffer the item-item layer's backward pushes into -- that autograd then adds: at config 5 a 128 MB fill and a
    384 MB add per step (17 + 60 us of a 2.1 ms step).  Here the push goes straight into the propagation's gradient.
    Inputs: g, n_layers, rows, mm, item_rows, n_user_rows (b), then the two tables.  Forward bits: the two ops'."""

    @staticmethod
    def forward(ctx, g, n_layers, rows, mm, item_rows, b, user_table, item_table):
        import types
        inner = types.SimpleNamespace(saved=None)
        inner.save_for_backward = lambda *t: setattr(inner, 'saved', t)
        at = _LightGCNMeanPartsRows.forward(inner, g, n_layers, rows, user_table, item_table)
        ia = spmm_rows_raw(mm, item_table.detach().contiguous(), item_rows, at[b:].contiguous(), z_compact=True)
        ctx.inner = types.SimpleNamespace(sizes=inner.sizes, g=inner.g, L=inner.L)
        ctx.mm, ctx.b = mm, int(b)
        ctx.save_for_backward(rows, item_rows)
        return at[:b].contiguous(), ia

    @staticmethod
    def backward(ctx, d_user_rows, d_ia):
        rows, item_rows = ctx.saved_tensors
        inner = ctx.inner
        inner.saved_tensors = (rows,)
        d_ia = d_ia.contiguous()
        d_rows = torch.cat((d_user_rows.contiguous(), d_ia), dim=0)        # d at = (d user rows, d ia: Z passes its gradient on)
        grads = _LightGCNMeanPartsRows.backward(inner, d_rows)
        d_user_table, d_item_table = grads[3], grads[4]
        spmm_push_rows_raw(ctx.mm, d_ia, item_rows, dX=d_item_table)       # (atomics into the propagation's item block)
        return None, None, None, None, None, None, d_user_table, d_item_table


def lightgcn_mean_rows_then_item_rows(g: CsrGraph, user_table, item_table, n_layers, users, item_rows, mm: CsrGraph):
    """-> (propagated user rows [b, d], (mm @ item_table)[item_rows] + propagated item rows [len(item_rows), d]) for a training
    step that reads its tables at the batch rows only; one autograd node when every piece has its row-list kernel, the two
    ops otherwise (`hip_deterministic`, relabelled graphs, rows spanning too many chunks)."""
    b, nu, d = users.shape[0], user_table.shape[0], user_table.shape[1]
    rows = torch.cat((users, item_rows + nu))
    fast = (not DETERMINISTIC and not isinstance(g, PermutedGraph) and not isinstance(mm, PermutedGraph) and d == EMB_DIM
            and int(n_layers) >= 1 and ROWS_LAST_LAYER and rows_servable(g, d) and rows_servable(mm, d)
            and user_table.shape[0] + item_table.shape[0] == g.n_rows == g.n_cols and mm.n_rows == mm.n_cols == item_table.shape[0])
    if not fast:
        at = lightgcn_mean_parts_rows(g, (user_table, item_table), n_layers, rows)
        return at[:b], spmm_rows(mm, item_table, item_rows, Z_rows=at[b:])
    return _MeanPartsRowsThenItemRows.apply(g, n_layers, rows, mm, item_rows, b, user_table, item_table)


def lightgcn_mean_parts_rows(g: CsrGraph, parts, n_layers, rows):
    """lightgcn_mean_parts(g, parts, n_layers) read at `rows` (int64 ids in the concatenated id space) -> [len(rows), d];
    same forward bits, the backward starts from the compact gradient (see the class).  `hip_deterministic`: the dense path."""
    if DETERMINISTIC or isinstance(g, PermutedGraph) or parts[0].shape[1] not in SLICE_WIDTHS + (EMB_DIM,):
        return torch.cat(lightgcn_mean_parts(g, parts, n_layers), dim=0).index_select(0, rows)
    return _LightGCNMeanPartsRows.apply(g, n_layers, rows, *parts)


class _LayerGCNSum(torch.autograd.Function):
    """sum_l w_l * (A E_{l-1}),  w_l = cos(A E_{l-1}, E0) per row, E_l = w_l * A E_{l-1}
    (layergcn.py:125-138).  SpMM kernel + fused cos-scale/accumulate kernel per layer."""

    @staticmethod
    def forward(ctx, E0, g, n_layers):
        lib = _lib.load()
        E0 = E0.contiguous()
        L, n = int(n_layers), E0.shape[0]
        if E0.shape[1] != EMB_DIM or E0.shape[0] != g.n_rows or g.n_cols != g.n_rows:
            raise _lib.MMRecHipError("layergcn_sum needs E0 [n, %d] over a square graph of n rows" % EMB_DIM)
        acc = torch.zeros_like(E0) if L == 0 else torch.empty_like(E0)
        need_y = any(ctx.needs_input_grad)        # the unscaled products are only read by the backward
        ys, ws = [], []
        cur = E0
        for layer in range(L):                    # SpMM + cosine re-weighting + layer sum: ONE launch per layer
            y = torch.empty_like(E0) if need_y else None
            out, w = torch.empty_like(E0), torch.empty(n, dtype=torch.float32, device=E0.device)
            args = (_p(g.rowptr), _p(g.colidx), _p(g.vals), _p(cur), _p(y), _p(E0), _p(out), _p(w),
                    _p(acc) if layer > 0 else None, _p(acc), g.n_rows, EMB_DIM, g.long_row_threshold, _p(g.long_rows),
                    _p(g.long_chunk_ptr), g.n_long, g.n_chunks, _p(g.partials_for(EMB_DIM)), _p(g.long_tickets))
            sc = g.scheduled(EMB_DIM)
            if sc is not None:
                g.checked(lib.mmrec_spmm_csr_sched_f32_layergcn(*args, _p(sc["row"]), _p(sc["span"]), _p(sc["col"]), _p(sc["val"]),
                                                                sc["n_short"], _stream()), "spmm_sched_layergcn")
            else:
                g.checked(lib.mmrec_spmm_csr_f32_layergcn(*args, _stream()), "spmm_layergcn")
            ys.append(y), ws.append(w)
            cur = out
        ctx.g, ctx.L = g, L
        if need_y:
            ctx.save_for_backward(E0, *ys, *ws)
        return acc

    @staticmethod
    def backward(ctx, dSum):
        lib = _lib.load()
        L, gt = ctx.L, ctx.g.transpose()
        saved = ctx.saved_tensors
        E0, ys, ws = saved[0], saved[1:1 + L], saved[1 + L:]
        dSum = dSum.contiguous()
        n = E0.shape[0]
        dEgo = torch.zeros_like(E0)
        dOut = dSum  # gradient w.r.t. the last layer's output
        for layer in range(L - 1, -1, -1):
            dY = torch.empty_like(E0)
            _lib.check(lib.mmrec_cos_scale_bwd_f32(_p(dOut), _p(ys[layer]), _p(E0), _p(ws[layer]),
                                                   _p(dY), _p(dEgo), n, EMB_DIM, _stream()),
                       "cos_scale_bwd")
            nxt = torch.empty_like(E0)
            # layer > 0: grad of the previous layer's output = A^T dY + dSum ; layer 0: input is E0
            spmm_raw(gt, dY, Y=nxt, Z=dSum if layer > 0 else dEgo, beta=1.0)
            dOut = nxt
        return dOut, None, None


def layergcn_sum(g: CsrGraph, E0, n_layers):
    return _LayerGCNSum.apply(E0, g, n_layers)


class _LayerGCNSumParts(torch.autograd.Function):
    """_LayerGCNSum on the row-wise concatenation of several tables, result split back into the same row blocks (see
    _LightGCNMeanParts: the same launches without autograd's cat / slice bookkeeping around them)."""

    @staticmethod
    def forward(ctx, g, n_layers, *parts):
        ctx.sizes = [p.shape[0] for p in parts]
        if row_blocks_of_one_buffer(parts):
            E0 = parts[0].detach().as_strided((sum(ctx.sizes), parts[0].shape[1]), (parts[0].shape[1], 1))
        else:
            E0 = torch.cat([p.detach() for p in parts], dim=0)
        return tuple(_LayerGCNSum.forward(ctx, E0, g, n_layers).split(ctx.sizes))

    @staticmethod
    def backward(ctx, *grads):
        like = next(x for x in grads if x is not None)
        n, d = sum(ctx.sizes), like.shape[1]
        if row_blocks_of_one_buffer(grads):
            dSum = grads[0].as_strided((n, d), (d, 1))
        else:
            dSum = torch.empty((n, d), dtype=like.dtype, device=like.device)
            for dst, src in zip(dSum.split(ctx.sizes), grads):
                dst.zero_() if src is None else dst.copy_(src)
        t = _LayerGCNSum.backward(ctx, dSum)[0]
        return (None, None) + tuple(t.split(ctx.sizes))


def layergcn_sum_parts(g: CsrGraph, parts, n_layers):
    """sum_l w_l (A E_{l-1}) over cat(parts) as a tuple of row blocks, one per input table (layergcn.py:125-138)"""
    return _LayerGCNSumParts.apply(g, n_layers, *parts)


# ------------------------------------------------------------------------------------------------
# P4  sampled scoring
# ------------------------------------------------------------------------------------------------
def _bpr_bwd_deterministic(U, I, users, pos, neg, coef, g, scale, dU, dI):
    """the fused BPR backward without atomics on the tables: the kernel runs on the gathered rows U[users], I[pos], I[neg]
    with identity ids (each per-sample gradient row is written once), the rows are then scattered in position order"""
    lib = _lib.load()
    B, d = users.numel(), U.shape[1]
    ar = torch.arange(B, device=U.device)
    Ug = U.index_select(0, users)
    Ig = torch.cat((I.index_select(0, pos), I.index_select(0, neg)), 0)
    dUg = torch.zeros_like(Ug) if dU is not None else None
    dIg = torch.zeros_like(Ig) if dI is not None else None
    arn = (ar + B).contiguous()
    _lib.check(lib.mmrec_bpr_bwd_f32(_p(Ug), _p(Ig), _p(Ig), _p(ar), _p(ar), _p(arn), B, d, _p(coef), _p(g), scale, _p(dUg),
                                     _p(dIg), _p(dIg), _stream()), "bpr_bwd")
    if dU is not None:
        scatter_add_rows(users, dUg, dU)
    if dI is not None:
        scatter_add_rows(torch.cat((pos, neg)), dIg, dI)


class _BprLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, U, I, users, pos, neg, variant, scale):
        lib = _lib.load()
        U, I = _chk(U.contiguous(), torch.float32, "U", 2), _chk(I.contiguous(), torch.float32, "I", 2)
        for t, nm in ((users, "users"), (pos, "pos"), (neg, "neg")):
            _chk(t, torch.int64, nm, 1)
        B, dev = users.numel(), U.device
        loss = torch.empty((), dtype=torch.float32, device=dev)
        coef = torch.empty(max(B, 1), dtype=torch.float32, device=dev)
        ws = _ws(lib.mmrec_bpr_workspace_bytes(B), dev)
        if U.shape[1] != I.shape[1] or U.shape[1] % EMB_DIM:
            raise _lib.MMRecHipError("U and I need the same row width, a multiple of %d" % EMB_DIM)
        _lib.check(lib.mmrec_bpr_fwd_f32(_p(U), _p(I), _p(I), _p(users), _p(pos), _p(neg), B, U.shape[1],
                                         int(variant), float(scale), _p(loss), _p(coef), _p(ws),
                                         _stream()), "bpr_fwd")
        ctx.save_for_backward(U, I, users, pos, neg, coef)
        ctx.scale = float(scale)
        return loss

    @staticmethod
    def backward(ctx, g):
        lib = _lib.load()
        U, I, users, pos, neg, coef = ctx.saved_tensors
        g = g.contiguous().to(torch.float32)
        dU = torch.zeros_like(U) if ctx.needs_input_grad[0] else None
        dI = torch.zeros_like(I) if ctx.needs_input_grad[1] else None
        if DETERMINISTIC:
            _bpr_bwd_deterministic(U, I, users, pos, neg, coef, g, ctx.scale, dU, dI)
            return dU, dI, None, None, None, None, None
        _lib.check(lib.mmrec_bpr_bwd_f32(_p(U), _p(I), _p(I), _p(users), _p(pos), _p(neg),
                                         users.numel(), U.shape[1], _p(coef), _p(g), ctx.scale, _p(dU),
                                         _p(dI), _p(dI), _stream()), "bpr_bwd")
        return dU, dI, None, None, None, None, None


class _BprLossShared(torch.autograd.Function):
    """Several BPR terms over the SAME user rows U[users] (FREEDOM's id term and its two modality terms,
    freedom.py:197-211), one loss scalar per term.  The same forward / backward kernels as _BprLoss, but ONE dense
    gradient buffer for U that the backward launches accumulate into, instead of one zero-filled [n_users, d] buffer per
    term and their sums."""

    @staticmethod
    def forward(ctx, U, users, variant, scale, n_terms, joint, sum_over_ranks, *flat):
        lib = _lib.load()
        ctx.joint = bool(joint)
        U = _chk(U.contiguous(), torch.float32, "U", 2)
        _chk(users, torch.int64, "users", 1)
        B, dev = users.numel(), U.device
        tables, ids, coefs, losses = [], [], [], []
        ws = _ws(lib.mmrec_bpr_workspace_bytes(B), dev)
        d = U.shape[1]
        sliced = sum_over_ranks is not None
        if sliced:          # column slices: partial <u, p>, <u, n> of every term, ONE sum over the ranks, then the losses
            dots = torch.empty((n_terms, 2, max(B, 1)), dtype=torch.float32, device=dev)
        for t in range(n_terms):
            I, pos, neg = flat[3 * t], flat[3 * t + 1], flat[3 * t + 2]
            I = _chk(I.contiguous(), torch.float32, "I", 2)
            _chk(pos, torch.int64, "pos", 1), _chk(neg, torch.int64, "neg", 1)
            if d != I.shape[1] or (d % EMB_DIM and not (sliced and d in SLICE_WIDTHS)):
                raise _lib.MMRecHipError("U and I need the same row width, a multiple of %d%s" %
                                         (EMB_DIM, " or a slice of 8 / 16 / 32 columns" if sliced else ""))
            tables.append(I), ids.extend((pos, neg))
            if sliced:
                _lib.check(lib.mmrec_bpr_dots_f32(_p(U), _p(I), _p(I), _p(users), _p(pos), _p(neg), B, d, _p(dots[t]),
                                                  _stream()), "bpr_dots")
                continue
            loss = torch.empty((), dtype=torch.float32, device=dev)
            coef = torch.empty(max(B, 1), dtype=torch.float32, device=dev)
            _lib.check(lib.mmrec_bpr_fwd_f32(_p(U), _p(I), _p(I), _p(users), _p(pos), _p(neg), B, d,
                                             int(variant), float(scale), _p(loss), _p(coef), _p(ws), _stream()), "bpr_fwd")
            coefs.append(coef), losses.append(loss)
        if sliced:
            sum_over_ranks(dots)                                  # in place
            for t in range(n_terms):
                loss = torch.empty((), dtype=torch.float32, device=dev)
                coef = torch.empty(max(B, 1), dtype=torch.float32, device=dev)
                _lib.check(lib.mmrec_bpr_loss_from_dots_f32(_p(dots[t]), B, int(variant), float(scale), _p(loss), _p(coef),
                                                            _p(ws), _stream()), "bpr_loss_from_dots")
                coefs.append(coef), losses.append(loss)
        ctx.save_for_backward(U, users, *tables, *ids, *coefs)
        ctx.scale, ctx.n_terms = float(scale), n_terms
        return tuple(losses)

    @staticmethod
    def backward(ctx, *gs):
        lib = _lib.load()
        n = ctx.n_terms
        saved = ctx.saved_tensors
        U, users = saved[0], saved[1]
        tables, ids, coefs = saved[2:2 + n], saved[2 + n:2 + 3 * n], saved[2 + 3 * n:]
        dU = dI0 = None
        if ctx.joint and ctx.needs_input_grad[0] and ctx.needs_input_grad[7]:
            # the gradients of U and of the first item table as adjacent row blocks of one zero-filled buffer: when both
            # came out of lightgcn_mean_parts, its backward takes the buffer as the gradient of its output, copy-free
            both = torch.zeros((U.shape[0] + tables[0].shape[0], U.shape[1]), dtype=U.dtype, device=U.device)
            dU, dI0 = both[:U.shape[0]], both[U.shape[0]:]
        elif ctx.needs_input_grad[0]:
            dU = torch.zeros_like(U)
        out = []
        for t in range(n):
            I, pos, neg = tables[t], ids[2 * t], ids[2 * t + 1]
            need_i = ctx.needs_input_grad[7 + 3 * t]
            own = dI0 if t == 0 and dI0 is not None else None
            if gs[t] is None or (dU is None and not need_i):
                out.extend(((own if own is not None else torch.zeros_like(I)) if need_i else None, None, None))
                continue
            dI = (own if own is not None else torch.zeros_like(I)) if need_i else None
            g = gs[t].contiguous().to(torch.float32)
            if DETERMINISTIC:       # terms in order, each scattered without atomics: the shared dU gets them one after the other
                _bpr_bwd_deterministic(U, I, users, pos, neg, coefs[t], g, ctx.scale, dU, dI)
            else:
                _lib.check(lib.mmrec_bpr_bwd_f32(_p(U), _p(I), _p(I), _p(users), _p(pos), _p(neg), users.numel(), U.shape[1],
                                                 _p(coefs[t]), _p(g), ctx.scale, _p(dU), _p(dI), _p(dI), _stream()), "bpr_bwd")
            out.extend((dI, None, None))
        return (dU, None, None, None, None, None, None) + tuple(out)


class _BprWeightedTotal(torch.autograd.Function):
    """sum_t w_t bpr_loss(U, I_t, users, pos_t, neg_t): mmrec_bpr_multi_fwd_f32 / _bwd_f32 (ABI 14) -- every term's per-sample
    work in ONE launch (grid.y = term), one finish launch for the weighted total, one backward launch.  Inputs: U, users, variant,
    scale, weights (tuple), joint, then I_0, pos_0, neg_0, I_1, ...; `joint`: the gradients of U and of the first table are
    adjacent row blocks of one zero-filled buffer (what lightgcn_mean_parts' backward takes copy-free)."""

    @staticmethod
    def forward(ctx, U, users, variant, scale, weights, joint, *flat):
        lib = _lib.load()
        n = len(weights)
        U = _chk(U.contiguous(), torch.float32, "U", 2)
        _chk(users, torch.int64, "users", 1)
        B, d, dev = users.numel(), U.shape[1], U.device
        tables = [_chk(flat[3 * t].contiguous(), torch.float32, "I", 2) for t in range(n)]
        pos, neg = [flat[3 * t + 1] for t in range(n)], [flat[3 * t + 2] for t in range(n)]
        for t in range(n):
            _chk(pos[t], torch.int64, "pos", 1), _chk(neg[t], torch.int64, "neg", 1)
            if tables[t].shape[1] != d or d % EMB_DIM or pos[t].numel() != B or neg[t].numel() != B:
                raise _lib.MMRecHipError("U and every table need the same row width (a multiple of %d), every id list B entries" % EMB_DIM)
        ptrs = lambda ts: (ctypes.c_void_p * n)(*[t.data_ptr() for t in ts])
        ctx.arrays = (ptrs(tables), ptrs(pos), ptrs(neg), (ctypes.c_float * n)(*[float(w) for w in weights]))
        total = torch.empty((), dtype=torch.float32, device=dev)
        coef = torch.empty(n, max(B, 1), dtype=torch.float32, device=dev)
        ws = _ws(lib.mmrec_bpr_multi_workspace_bytes(n, B), dev)
        _lib.check(lib.mmrec_bpr_multi_fwd_f32(_p(U), _p(users), *ctx.arrays, n, B, d, int(variant), float(scale), _p(total), None,
                                               _p(coef), _p(ws), _stream()), "bpr_multi_fwd")
        ctx.save_for_backward(U, users, coef, *tables, *pos, *neg)
        ctx.n, ctx.scale, ctx.joint = n, float(scale), bool(joint)
        return total

    @staticmethod
    def backward(ctx, g):
        lib = _lib.load()
        n = ctx.n
        U, users, coef = ctx.saved_tensors[:3]
        tables = ctx.saved_tensors[3:3 + n]
        g = g.contiguous().to(torch.float32)
        need_u = ctx.needs_input_grad[0]
        need_i = [ctx.needs_input_grad[6 + 3 * t] for t in range(n)]
        dU = None
        grads = [None] * n
        if ctx.joint and need_u and need_i[0]:
            both = torch.zeros((U.shape[0] + tables[0].shape[0], U.shape[1]), dtype=U.dtype, device=U.device)
            dU, grads[0] = both[:U.shape[0]], both[U.shape[0]:]
        elif need_u:
            dU = torch.zeros_like(U)
        shared = {}
        for t in range(n):
            if need_i[t] and grads[t] is None:
                key = tables[t].data_ptr()
                if key not in shared:
                    shared[key] = torch.zeros_like(tables[t])
                grads[t] = shared[key]
        dI = (ctypes.c_void_p * n)(*[None if x is None else x.data_ptr() for x in grads])
        _lib.check(lib.mmrec_bpr_multi_bwd_f32(_p(U), _p(users), *ctx.arrays, n, users.numel(), U.shape[1], _p(coef), _p(g), ctx.scale,
                                               _p(dU), dI, _stream()), "bpr_multi_bwd")
        out, seen = [dU, None, None, None, None, None], set()
        for t in range(n):
            gi = grads[t]
            if gi is not None and id(gi) in seen:
                gi = None                                  # (a table named by two terms: its one buffer goes to the first)
            elif gi is not None:
                seen.add(id(gi))
            out += [gi, None, None]
        return tuple(out)


def bpr_weighted_total(U, users, terms, weights, variant=BPR_LOGSIG, reduction="mean", joint_grad=False):
    """sum_t weights[t] * bpr_loss(U, I_t, users, pos_t, neg_t) as ONE scalar (freedom.py:197-211: the id term + reg_weight times
    the modality terms) -- two launches forward, one backward (ABI 14); `hip_deterministic`, more than MMREC_BPR_MAX_TERMS terms
    or tables that share memory without being the same table (`_one_buffer_per_table`): the per-term form."""
    terms = list(terms)
    if DETERMINISTIC or not 1 <= len(terms) <= 4 or not _one_buffer_per_table([I for I, _, _ in terms]):
        losses = bpr_losses_shared_users(U, users, terms, variant, reduction, joint_grad=joint_grad)
        total = 0.0
        for w, l in zip(weights, losses):
            total = total + w * l
        return total
    B = users.numel()
    scale = 1.0 / max(B, 1) if reduction == "mean" else 1.0
    flat = [x for term in terms for x in term]
    return _BprWeightedTotal.apply(U, users, variant, scale, tuple(float(w) for w in weights), joint_grad, *flat)


def bpr_losses_shared_users(U, users, terms, variant=BPR_LOGSIG, reduction="mean", joint_grad=False, sum_over_ranks=None):
    """[bpr_loss(U, I_t, users, pos_t, neg_t) for (I_t, pos_t, neg_t) in terms] with one shared gradient buffer for U;
    joint_grad: the gradient of the FIRST term's table is the row block right after U's in the same buffer.
    sum_over_ranks (feature-sliced layout): U and the tables are this rank's COLUMNS (8 / 16 / 32 of them, or whole rows);
    the callable sums the [terms, 2, B] partial dot products over the ranks in place (one all-reduce), the losses come out
    replicated and every rank's backward scatters into its own columns -- the same kernels, no collective."""
    B = users.numel()
    scale = 1.0 / max(B, 1) if reduction == "mean" else 1.0
    flat = [x for term in terms for x in term]
    return _BprLossShared.apply(U, users, variant, scale, len(terms), joint_grad, sum_over_ranks, *flat)


def bpr_loss(U, I, users, pos, neg, variant=BPR_LOGSIG, reduction="mean"):
    """Fused gather-dot-(log)sigmoid BPR loss on rows U[users], I[pos], I[neg].
    variant LOGSIG/mean = FREEDOM.bpr_loss (freedom.py:180-187), LOGSIG/sum = LayerGCN
    (layergcn.py:140-152), GAMMA/mean = BPRLoss (common/loss.py:33-35)."""
    B = users.numel()
    scale = 1.0 / max(B, 1) if reduction == "mean" else 1.0
    return _BprLoss.apply(U, I, users, pos, neg, variant, scale)


class _InfoNCE(torch.autograd.Function):
    @staticmethod
    def forward(ctx, E1, E2, ids, tau):
        lib = _lib.load()
        E1, E2 = _chk(E1.contiguous(), torch.float32, "E1", 2), _chk(E2.contiguous(), torch.float32, "E2", 2)
        _chk(ids, torch.int64, "ids", 1)
        if E1.shape != E2.shape or E1.shape[1] != EMB_DIM:
            raise _lib.MMRecHipError("InfoNCE views must both be [n, %d]" % EMB_DIM)
        B = ids.numel()
        loss = torch.empty((), dtype=torch.float32, device=E1.device)
        ws = _ws(lib.mmrec_infonce_workspace_bytes(B), E1.device)
        _lib.check(lib.mmrec_infonce_fwd_f32(_p(E1), _p(E2), _p(ids), B, EMB_DIM, float(tau), _p(loss),
                                             _p(ws), _stream()), "infonce_fwd")
        ctx.save_for_backward(ids, ws)
        ctx.tau, ctx.shape = float(tau), E1.shape
        return loss

    @staticmethod
    def backward(ctx, g):
        lib = _lib.load()
        ids, ws = ctx.saved_tensors
        g = g.contiguous().to(torch.float32)
        dE1 = torch.zeros(ctx.shape, dtype=torch.float32, device=g.device) if ctx.needs_input_grad[0] else None
        dE2 = torch.zeros(ctx.shape, dtype=torch.float32, device=g.device) if ctx.needs_input_grad[1] else None
        if DETERMINISTIC:      # per-sample rows (identity ids: one write each), then the position-ordered scatter
            B = ids.numel()
            ar = torch.arange(B, device=g.device)
            r1 = torch.zeros(B, EMB_DIM, dtype=torch.float32, device=g.device) if dE1 is not None else None
            r2 = torch.zeros(B, EMB_DIM, dtype=torch.float32, device=g.device) if dE2 is not None else None
            _lib.check(lib.mmrec_infonce_bwd_f32(_p(ar), B, EMB_DIM, ctx.tau, _p(g), _p(r1), _p(r2), _p(ws), _stream()),
                       "infonce_bwd")
            if dE1 is not None:
                scatter_add_rows(ids, r1, dE1)
            if dE2 is not None:
                scatter_add_rows(ids, r2, dE2)
            return dE1, dE2, None, None
        _lib.check(lib.mmrec_infonce_bwd_f32(_p(ids), ids.numel(), EMB_DIM, ctx.tau, _p(g), _p(dE1),
                                             _p(dE2), _p(ws), _stream()), "infonce_bwd")
        return dE1, dE2, None, None


def infonce(E1, E2, ids, tau):
    """Fused in-batch InfoNCE between rows `ids` of two [n, 64] views (MGCN.InfoNCE, mgcn.py:224-231:
    F.normalize both, positives on the diagonal, all B columns as negatives, mean over the batch)."""
    return _InfoNCE.apply(E1, E2, ids, tau)


class _GatherSqNorm(torch.autograd.Function):
    @staticmethod
    def forward(ctx, E, ids):
        lib = _lib.load()
        E = _chk(E.contiguous(), torch.float32, "E", 2)
        _chk(ids, torch.int64, "ids", 1)
        out = torch.empty((), dtype=torch.float32, device=E.device)
        ws = _ws(4 * ids.numel(), E.device)
        _lib.check(lib.mmrec_gather_sqnorm_fwd_f32(_p(E), _p(ids), ids.numel(), E.shape[1], _p(out),
                                                   _p(ws), _stream()), "gather_sqnorm_fwd")
        ctx.save_for_backward(E, ids)
        return out

    @staticmethod
    def backward(ctx, g):
        lib = _lib.load()
        E, ids = ctx.saved_tensors
        coef = (2.0 * g).contiguous().to(torch.float32)
        dE = torch.zeros_like(E)
        if DETERMINISTIC:
            return scatter_add_rows(ids, E.index_select(0, ids) * coef, dE), None
        _lib.check(lib.mmrec_gather_scale_add_bwd_f32(_p(E), _p(ids), ids.numel(), E.shape[1], _p(coef),
                                                      _p(dE), _stream()), "gather_scale_add_bwd")
        return dE, None


def gather_sqnorm(E, ids):
    """sum_b ||E[ids[b]]||^2 (differentiable): building block of EmbLoss / L2Loss on batch rows
    (common/loss.py:46-62 as used at lightgcn.py:145-149, layergcn.py:154-161)."""
    return _GatherSqNorm.apply(E, ids)


class _RowsReg(torch.autograd.Function):
    """scale * sum_t f(sum_b ||E_t[ids_t[b]]||^2) for ALL terms of a step's regulariser: mmrec_rows_reg_fwd_f32 / _bwd_f32
    (ABI 14).  Inputs: mode, scale, then E_0, ids_0, E_1, ids_1, ...; a table that appears in several terms (the item table's
    positive and negative rows) gets ONE dense gradient buffer, returned for its first occurrence."""

    @staticmethod
    def forward(ctx, mode, scale, *flat):
        lib = _lib.load()
        tables = [_chk(flat[2 * t].contiguous(), torch.float32, "E", 2) for t in range(len(flat) // 2)]
        ids = [None if flat[2 * t + 1] is None else _chk(flat[2 * t + 1], torch.int64, "ids", 1) for t in range(len(flat) // 2)]
        n, d, dev = len(tables), tables[0].shape[1], tables[0].device
        if any(E.shape[1] != d for E in tables) or d % EMB_DIM:
            raise _lib.MMRecHipError("rows_reg: every table needs the same row width, a multiple of %d" % EMB_DIM)
        batch = (ctypes.c_int32 * n)(*[E.shape[0] if i is None else i.numel() for E, i in zip(tables, ids)])   # ids None: every row
        ctx.arrays = ((ctypes.c_void_p * n)(*[E.data_ptr() for E in tables]),
                      (ctypes.c_void_p * n)(*[None if i is None else i.data_ptr() for i in ids]), batch)
        out = torch.empty((), dtype=torch.float32, device=dev)
        coef = torch.empty(n, dtype=torch.float32, device=dev)
        ws = _ws(lib.mmrec_rows_reg_workspace_bytes(n, max(batch)), dev)
        _lib.check(lib.mmrec_rows_reg_fwd_f32(ctx.arrays[0], ctx.arrays[1], batch, n, d, int(mode), float(scale), _p(out), _p(coef),
                                              _p(ws), _stream()), "rows_reg_fwd")
        ctx.save_for_backward(coef, *tables, *[i for i in ids if i is not None])     # (the ids: kept alive for the backward's pointers)
        ctx.n = n
        return out

    @staticmethod
    def backward(ctx, g):
        lib = _lib.load()
        n = ctx.n
        coef, tables = ctx.saved_tensors[0], ctx.saved_tensors[1:1 + n]
        g = g.contiguous().to(torch.float32)
        grads, first, out = {}, {}, [None, None]
        for t, E in enumerate(tables):
            if E.data_ptr() not in grads:
                grads[E.data_ptr()], first[E.data_ptr()] = torch.zeros_like(E), t
        dE = (ctypes.c_void_p * n)(*[grads[E.data_ptr()].data_ptr() for E in tables])
        _lib.check(lib.mmrec_rows_reg_bwd_f32(ctx.arrays[0], ctx.arrays[1], ctx.arrays[2], n, tables[0].shape[1], _p(coef), _p(g), dE,
                                              _stream()), "rows_reg_bwd")
        for t, E in enumerate(tables):
            out += [grads[E.data_ptr()] if (first[E.data_ptr()] == t and ctx.needs_input_grad[2 + 2 * t]) else None, None]
        return tuple(out)


ROWS_REG_SQUARED, ROWS_REG_NORM = 0, 1


def _one_buffer_per_table(tables):
    """True when the multi-term backward kernels may give every distinct data_ptr() ONE dense gradient buffer: any two
    tables are either the same table (same pointer, same shape, same requires_grad) or do not share memory at all.  Views of one
    another's storage -- T[:k] next to T, two overlapping row ranges, a detached alias of a live tensor -- are not: a buffer
    sized by the first would be written past its end by the second, or a constant's gradient folded into the live tensor's."""
    seen = []
    for E in tables:
        if not E.is_contiguous():                  # (the fused ops take .contiguous() copies of such operands: the byte range below
            return False                           # would not be the view's)
        lo = E.data_ptr()
        span = (lo, lo + E.numel() * E.element_size(), tuple(E.shape), bool(E.requires_grad))
        for other in seen:
            if span[0] < other[1] and other[0] < span[1] and span != other:
                return False
        seen.append(span)
    return True


def rows_reg(terms, mode, scale=1.0):
    """The regulariser of a training step over batch rows, fused: scale * sum_t ||E_t[ids_t]||_F^2 (mode ROWS_REG_SQUARED: the L2
    regulariser of layergcn.py:154-161 / lattice.py:214-216) or scale * sum_t ||E_t[ids_t]||_F (ROWS_REG_NORM: EmbLoss,
    common/loss.py:46-51).  terms = [(table [n, 64 k], ids [B]) ...].  Two launches forward, one backward, whatever the number
    of terms; `hip_deterministic`, more than MMREC_ROWS_REG_MAX_TERMS terms or tables that share memory without being the same
    table (views of one another's storage, overlapping row ranges, a detached alias: `_one_buffer_per_table`) take the per-term
    ops."""
    terms = list(terms)
    same_rows = len({E.shape[1] for E, _ in terms}) == 1
    if (DETERMINISTIC or len(terms) > 6 or not terms or not same_rows or any(not E.is_contiguous() for E, _ in terms)
            or not _one_buffer_per_table([E for E, _ in terms])):
        total = 0.0
        for E, ids in terms:
            s = (E * E).sum() if ids is None else gather_sqnorm(E, ids)
            total = total + (s if mode == ROWS_REG_SQUARED else torch.sqrt(s))
        return scale * total
    flat = [x for E, ids in terms for x in (E, None if ids is None else ids.contiguous())]
    return _RowsReg.apply(mode, scale, *flat)


class _RowNormalize(torch.autograd.Function):
    @staticmethod
    def forward(ctx, X, eps):
        lib = _lib.load()
        X = _chk(X.contiguous(), torch.float32, "X", 2)
        if X.shape[1] % 4:
            raise _lib.MMRecHipError("row_normalize: rows of a multiple of 4 floats")
        Y = torch.empty_like(X)
        inv = torch.empty(max(X.shape[0], 1), dtype=torch.float32, device=X.device)
        _lib.check(lib.mmrec_row_normalize_fwd_f32(_p(X), X.shape[0], X.shape[1], float(eps), _p(Y), _p(inv), _stream()),
                   "row_normalize_fwd")
        ctx.save_for_backward(Y, inv)
        return Y

    @staticmethod
    def backward(ctx, G):
        lib = _lib.load()
        Y, inv = ctx.saved_tensors
        G = G.contiguous()
        dX = torch.empty_like(Y)
        _lib.check(lib.mmrec_row_normalize_bwd_f32(_p(Y), _p(G), _p(inv), Y.shape[0], Y.shape[1], _p(dX), _stream()),
                   "row_normalize_bwd")
        return dX, None


def row_normalize(X, eps=1e-12):
    """F.normalize(X, p=2, dim=1) in one launch each way (lattice.py:165, mmgcn.py:167)."""
    return _RowNormalize.apply(X, eps)


class _CatLeaky(torch.autograd.Function):
    @staticmethod
    def forward(ctx, A, B, R, slope):
        lib = _lib.load()
        A, B = _chk(A.contiguous(), torch.float32, "A", 2), _chk(B.contiguous(), torch.float32, "B", 2)
        if R is not None:
            R = _chk(R.contiguous(), torch.float32, "R", 2)
        n, wa, wb = A.shape[0], A.shape[1], B.shape[1]
        if B.shape[0] != n or (R is not None and R.shape != B.shape) or wa % 4 or wb % 4:
            raise _lib.MMRecHipError("cat_leaky: A [n, wa], B [n, wb], R [n, wb] with wa, wb multiples of 4")
        out = torch.empty(n, wa + wb, dtype=torch.float32, device=A.device)
        _lib.check(lib.mmrec_cat_leaky_fwd_f32(_p(A), _p(B), _p(R), n, wa, wb, float(slope), _p(out), _stream()), "cat_leaky_fwd")
        ctx.save_for_backward(A, B)
        ctx.slope = float(slope)
        return out

    @staticmethod
    def backward(ctx, dOut):
        lib = _lib.load()
        A, B = ctx.saved_tensors
        dOut = dOut.contiguous()
        dA = torch.empty_like(A) if ctx.needs_input_grad[0] else None
        dB = torch.empty_like(B) if ctx.needs_input_grad[1] else None
        dR = torch.empty_like(B) if ctx.needs_input_grad[2] else None
        _lib.check(lib.mmrec_cat_leaky_bwd_f32(_p(A), _p(B), _p(dOut), A.shape[0], A.shape[1], B.shape[1], ctx.slope, _p(dA), _p(dB),
                                               _p(dR), _stream()), "cat_leaky_bwd")
        return dA, dB, dR, None


def cat_leaky(A, B, R=None, slope=0.01):
    """cat((leaky_relu(A), leaky_relu(B) + R), dim=1) in one launch each way (mmgcn.py:170-173: h, x_hat and their cat)."""
    return _CatLeaky.apply(A, B, R, slope)


class _CosineMean(torch.autograd.Function):
    @staticmethod
    def forward(ctx, X, ix, Y, iy):
        lib = _lib.load()
        X, Y = _chk(X.contiguous(), torch.float32, "X", 2), _chk(Y.contiguous(), torch.float32, "Y", 2)
        for t, nm in ((ix, "ix"), (iy, "iy")):
            if t is not None:
                _chk(t, torch.int64, nm, 1)
        B = ix.numel() if ix is not None else (iy.numel() if iy is not None else X.shape[0])
        if X.shape[1] != Y.shape[1] or X.shape[1] % EMB_DIM:
            raise _lib.MMRecHipError("X and Y need the same row width, a multiple of %d" % EMB_DIM)
        if (ix is None and X.shape[0] != B) or (iy is None and Y.shape[0] != B):
            raise _lib.MMRecHipError("an operand without an index must have one row per sample")
        out = torch.empty((), dtype=torch.float32, device=X.device)
        coef = torch.empty(max(B, 1), 2, dtype=torch.float32, device=X.device)
        ws = _ws(lib.mmrec_cosine_workspace_bytes(B), X.device)
        _lib.check(lib.mmrec_cosine_fwd_f32(_p(X), _p(ix), _p(Y), _p(iy), B, X.shape[1], 1.0 / max(B, 1), _p(out),
                                            _p(coef), _p(ws), _stream()), "cosine_fwd")
        ctx.save_for_backward(X, Y, coef, *[t for t in (ix, iy) if t is not None])
        ctx.has = (ix is not None, iy is not None)
        ctx.B = B
        return out

    @staticmethod
    def backward(ctx, g):
        lib = _lib.load()
        X, Y, coef, *idx = ctx.saved_tensors
        ix = idx.pop(0) if ctx.has[0] else None
        iy = idx.pop(0) if ctx.has[1] else None
        dX = torch.zeros_like(X)
        g = g.contiguous().to(torch.float32)
        if DETERMINISTIC and ix is not None:      # gathered operands, one gradient row per sample, position-ordered scatter
            Xg = X.index_select(0, ix)
            Yg = Y.index_select(0, iy) if iy is not None else Y
            rows = torch.zeros_like(Xg)
            _lib.check(lib.mmrec_cosine_bwd_f32(_p(Xg), None, _p(Yg), None, ctx.B, X.shape[1], _p(coef), _p(g),
                                                1.0 / max(ctx.B, 1), _p(rows), _stream()), "cosine_bwd")
            return scatter_add_rows(ix, rows, dX), None, None, None
        _lib.check(lib.mmrec_cosine_bwd_f32(_p(X), _p(ix), _p(Y), _p(iy), ctx.B, X.shape[1], _p(coef), _p(g),
                                            1.0 / max(ctx.B, 1), _p(dX), _stream()), "cosine_bwd")
        return dX, None, None, None


class _CosineMeans(torch.autograd.Function):
    """sum_t w_t mean_b cos(X_t[ix_t[b]], Y_t[iy_t[b]]): mmrec_cosine_multi_fwd_f32 / _bwd_f32 (ABI 14).  Inputs: the weights
    (tuple of floats), then X_0, ix_0, Y_0, iy_0, X_1, ... (indices may be None); terms that share X share its gradient."""

    @staticmethod
    def forward(ctx, weights, *flat):
        lib = _lib.load()
        n = len(weights)
        X = [_chk(flat[4 * t].contiguous(), torch.float32, "X", 2) for t in range(n)]
        Y = [_chk(flat[4 * t + 2].contiguous(), torch.float32, "Y", 2) for t in range(n)]
        ix, iy = [flat[4 * t + 1] for t in range(n)], [flat[4 * t + 3] for t in range(n)]
        d, dev = X[0].shape[1], X[0].device
        batch = []
        for t in range(n):
            for i, nm in ((ix[t], "ix"), (iy[t], "iy")):
                if i is not None:
                    _chk(i, torch.int64, nm, 1)
            B = ix[t].numel() if ix[t] is not None else (iy[t].numel() if iy[t] is not None else X[t].shape[0])
            if X[t].shape[1] != d or Y[t].shape[1] != d or d % EMB_DIM:
                raise _lib.MMRecHipError("cosine_means: every operand needs the same row width, a multiple of %d" % EMB_DIM)
            if (ix[t] is None and X[t].shape[0] != B) or (iy[t] is None and Y[t].shape[0] != B):
                raise _lib.MMRecHipError("an operand without an index must have one row per sample")
            batch.append(B)
        ptrs = lambda ts: (ctypes.c_void_p * n)(*[None if t is None else t.data_ptr() for t in ts])
        ctx.arrays = (ptrs(X), ptrs(ix), ptrs(Y), ptrs(iy), (ctypes.c_float * n)(*[float(w) for w in weights]), (ctypes.c_int32 * n)(*batch))
        out = torch.empty((), dtype=torch.float32, device=dev)
        coef = torch.empty(n, max(max(batch), 1), 2, dtype=torch.float32, device=dev)
        ws = _ws(lib.mmrec_cosine_multi_workspace_bytes(n, max(batch)), dev)
        _lib.check(lib.mmrec_cosine_multi_fwd_f32(*ctx.arrays, n, d, _p(out), _p(coef), _p(ws), _stream()), "cosine_multi_fwd")
        ctx.save_for_backward(coef, *X, *Y, *[i for i in ix + iy if i is not None])
        ctx.n = n
        return out

    @staticmethod
    def backward(ctx, g):
        lib = _lib.load()
        n = ctx.n
        coef, X = ctx.saved_tensors[0], ctx.saved_tensors[1:1 + n]
        g = g.contiguous().to(torch.float32)
        grads, first = {}, {}
        for t, x in enumerate(X):
            if ctx.needs_input_grad[1 + 4 * t] and x.data_ptr() not in grads:
                grads[x.data_ptr()], first[x.data_ptr()] = torch.zeros_like(x), t
        dX = (ctypes.c_void_p * n)(*[grads[x.data_ptr()].data_ptr() if x.data_ptr() in grads else None for x in X])
        _lib.check(lib.mmrec_cosine_multi_bwd_f32(*ctx.arrays, n, X[0].shape[1], _p(coef), _p(g), dX, _stream()), "cosine_multi_bwd")
        out = [None]
        for t, x in enumerate(X):
            out += [grads[x.data_ptr()] if first.get(x.data_ptr()) == t else None, None, None, None]
        return tuple(out)


def cosine_means(terms):
    """sum_t w_t mean_b cosine_similarity(X_t[ix_t[b]], Y_t[iy_t[b]]) for terms = [(X, ix, Y, iy, w), ...] in one launch pair
    (Y constant, indices may be None): BM3's six BYOL terms (bm3.py:129-144).  `hip_deterministic`, more than
    MMREC_COSINE_MAX_TERMS terms, or X operands that share memory without being the same table (`_one_buffer_per_table`): the
    per-term op."""
    terms = list(terms)
    if DETERMINISTIC or not terms or len(terms) > 8 or not _one_buffer_per_table([X for X, *_ in terms]):
        total = 0.0
        for X, ix, Y, iy, w in terms:
            total = total + w * cosine_mean(X, ix, Y, iy)
        return total
    flat = [a for X, ix, Y, iy, _ in terms for a in (X, ix, Y.detach(), iy)]
    return _CosineMeans.apply(tuple(float(w) for *_, w in terms), *flat)


def cosine_mean(X, ix, Y, iy):
    """mean_b cosine_similarity(X[ix[b]], Y[iy[b]]) as ONE fused gather-dot-norm kernel (+ a scatter backward into X;
    Y is treated as a constant, as BM3's detached targets are): bm3.py:129-144, selfcfed_lgn.py:57-58.  ix / iy may
    be None (row b of the operand)."""
    return _CosineMean.apply(X, ix, Y.detach(), iy)


# ------------------------------------------------------------------------------------------------
# P3  modal projection
# ------------------------------------------------------------------------------------------------
LINEAR_SPLIT_MIN_F = 1024      # narrower inputs take the fp32-MFMA forward


class _Linear(torch.autograd.Function):
    @staticmethod
    def forward(ctx, X, W, b):
        lib = _lib.load()
        X = _chk(X.contiguous(), torch.float32, "X", 2)
        W = _chk(W.contiguous(), torch.float32, "W", 2)
        n, F = X.shape
        if W.shape != (64, F):
            raise _lib.MMRecHipError("W must be [64, %d], got %s" % (F, tuple(W.shape)))
        if b is not None:
            b = _chk(b.contiguous(), torch.float32, "b", 1)
        Y = torch.empty(n, 64, dtype=torch.float32, device=X.device)
        ws = _ws(lib.mmrec_linear_workspace_bytes(n, F, 64), X.device)
        # narrow tables (the 384-wide text features) are launch bound, not stream bound: the fp32 kernel is ONE launch where the
        # split form is three or four (W split, kernel, slab sum, guard fix-up): 19 us against 24 at 7,050 x 384
        fwd = lib.mmrec_linear_fwd_split_f32 if (LINEAR_F16X3 and F >= LINEAR_SPLIT_MIN_F) else lib.mmrec_linear_fwd_f32
        _lib.check(fwd(_p(X), _p(W), _p(b), _p(Y), n, F, 64, _p(ws), _stream()), "linear_fwd")
        ctx.save_for_backward(X, W)
        ctx.has_b = b is not None
        return Y

    @staticmethod
    def backward(ctx, dY):
        lib = _lib.load()
        X, W = ctx.saved_tensors
        n, F = X.shape
        dY = dY.contiguous()
        dX = dW = db = None
        want_w = ctx.needs_input_grad[1] or (ctx.has_b and ctx.needs_input_grad[2])
        if want_w:
            dW = torch.empty_like(W)
            db = torch.empty(64, dtype=torch.float32, device=X.device) if ctx.has_b else None
        if ctx.needs_input_grad[0]:
            dX = torch.empty_like(X)
        if LINEAR_F16X3 and n > 0 and F % 128 == 0:
            # dW, db and dX in one call on the 16-bit matrix cores with split operands (ABI 11: dW on three bf16 parts, dX on fp16
            # halves scaled by exact powers of two)
            ws = _ws(lib.mmrec_linear_bwd_split_workspace_bytes(n, F, 64), X.device)
            _lib.check(lib.mmrec_linear_bwd_split_f32(_p(dY), _p(X), _p(W), _p(dW), _p(db), _p(dX), n, F, 64, _p(ws),
                                                      _stream()), "linear_bwd_split")
            return dX, dW, db
        if want_w:
            ws = _ws(lib.mmrec_linear_workspace_bytes(n, F, 64), X.device)
            _lib.check(lib.mmrec_linear_bwd_w_f32(_p(dY), _p(X), _p(dW), _p(db), n, F, 64, _p(ws),
                                                  _stream()), "linear_bwd_w")
        if dX is not None:
            _lib.check(lib.mmrec_linear_bwd_x_f32(_p(dY), _p(W), _p(dX), n, F, 64, _stream()),
                       "linear_bwd_x")
        return dX, dW, db


class _LinearWide(torch.autograd.Function):
    """F.linear with out = 64 j > 64 and F % 32 == 0: forward and dX on the 128 x 128 LDS-DMA GEMM
    (mmrec_gemm_nt_f32), dW / db on the split-over-rows kernel, 64 output columns at a time."""

    @staticmethod
    def forward(ctx, X, W, b):
        lib = _lib.load()
        X = _chk(X.contiguous(), torch.float32, "X", 2)
        W = _chk(W.contiguous(), torch.float32, "W", 2)
        n, F = X.shape
        out = W.shape[0]
        if W.shape[1] != F or out % 64 or F % 32:
            raise _lib.MMRecHipError("wide linear needs W [64 j, F], F %% 32 == 0; got W %s, X %s" %
                                     (tuple(W.shape), tuple(X.shape)))
        if b is not None:
            b = _chk(b.contiguous(), torch.float32, "b", 1)
        Y = torch.empty(n, out, dtype=torch.float32, device=X.device)
        _lib.check(lib.mmrec_gemm_nt_f32(_p(X), _p(W), _p(b), _p(Y), n, out, F, out, _stream()), "gemm_nt")
        ctx.save_for_backward(X, W)
        ctx.has_b = b is not None
        return Y

    @staticmethod
    def backward(ctx, dY):
        lib = _lib.load()
        X, W = ctx.saved_tensors
        n, F = X.shape
        out = W.shape[0]
        dY = dY.contiguous()
        dX = dW = db = None
        if ctx.needs_input_grad[1] or (ctx.has_b and ctx.needs_input_grad[2]):
            dW = torch.empty_like(W)
            db = torch.empty(out, dtype=torch.float32, device=X.device) if ctx.has_b else None
            ws = _ws(lib.mmrec_linear_workspace_bytes(n, F, out), X.device)
            _lib.check(lib.mmrec_linear_bwd_w_f32(_p(dY), _p(X), _p(dW), _p(db), n, F, out, _p(ws),
                                                  _stream()), "linear_bwd_w")
        if ctx.needs_input_grad[0]:
            dX = torch.empty_like(X)
            Wt = W.t().contiguous()                         # [F, out]: dX = dY W = dY (W^T)^T
            _lib.check(lib.mmrec_gemm_nt_f32(_p(dY), _p(Wt), None, _p(dX), n, F, out, F, _stream()), "gemm_nt")
        return dX, dW, db


def linear(X, W, b=None):
    """X @ W^T + b on the fp32 matrix cores.  out = 64: nn.Linear image_trs / text_trs / item_linear
    (freedom.py:205,208; bm3.py:102,104; vbpr.py:70) on the projection kernels; out = 64 j with
    F % 32 == 0 (MMGCN's 256 / 384-wide layers): the general LDS-DMA GEMM."""
    if W.shape[0] == 64:
        return _Linear.apply(X, W, b)
    return _LinearWide.apply(X, W, b)


def linear_rows_served(table, ids, W):
    """True where `linear_rows` runs the gathered kernels (mmrec_linear_rows_*): device fp32 operands, W [64, F] with
    F % 128 == 0, a contiguous table, int64 ids, and the split-operand projection (`LINEAR_F16X3`) on."""
    return (LINEAR_F16X3 and _dev_table(table) and W.is_cuda and W.dtype == torch.float32 and W.dim() == 2 and
            W.shape[0] == 64 and W.shape[1] == table.shape[1] and table.shape[1] % 128 == 0 and
            isinstance(ids, torch.Tensor) and ids.is_cuda and ids.dtype == torch.int64 and ids.dim() == 1)


def _linear_rows_fwd(table, ids, W, b):
    lib = _lib.load()
    n, F = ids.numel(), table.shape[1]
    Y = torch.empty(n, 64, dtype=torch.float32, device=table.device)
    ws = _ws(lib.mmrec_linear_rows_workspace_bytes(n, F, 64), table.device)
    split = 1 if F >= LINEAR_SPLIT_MIN_F else 0         # _Linear.forward's choice
    _lib.check(lib.mmrec_linear_rows_fwd_f32(_p(table), table.shape[0], _p(ids), _p(W), _p(b), _p(Y), n, F, 64, split, _p(ws),
                                             _stream()), "linear_rows_fwd")
    return Y


def _linear_rows_bwd(dY, table, ids, W, want_w, has_b, want_x):
    """dW, db, compact dX [len(ids), F] (each None where not wanted) of the gathered projection"""
    lib = _lib.load()
    n, F = ids.numel(), table.shape[1]
    dY = dY.contiguous()
    dW = db = dX = None
    if want_w:
        dW = torch.empty_like(W)
        db = torch.empty(64, dtype=torch.float32, device=W.device) if has_b else None
    if want_x:
        dX = torch.empty(n, F, dtype=torch.float32, device=W.device)
    if want_w or want_x:
        ws = _ws(lib.mmrec_linear_rows_workspace_bytes(n, F, 64), W.device)
        _lib.check(lib.mmrec_linear_rows_bwd_f32(_p(dY), _p(table), table.shape[0], _p(ids), _p(W), _p(dW), _p(db), _p(dX), n, F,
                                                 64, _p(ws), _stream()), "linear_rows_bwd")
    return dW, db, dX


class _LinearRows(torch.autograd.Function):
    @staticmethod
    def forward(ctx, table, ids, W, b):
        W = _chk(W.contiguous(), torch.float32, "W", 2)
        if b is not None:
            b = _chk(b.contiguous(), torch.float32, "b", 1)
        ids = ids.contiguous()
        ctx.save_for_backward(table, ids, W)
        ctx.has_b = b is not None
        return _linear_rows_fwd(table, ids, W, b)

    @staticmethod
    def backward(ctx, dY):
        table, ids, W = ctx.saved_tensors
        want_w = ctx.needs_input_grad[2] or (ctx.has_b and ctx.needs_input_grad[3])
        dW, db, dX = _linear_rows_bwd(dY, table, ids, W, want_w, ctx.has_b, ctx.needs_input_grad[0])
        dT = None
        if dX is not None:
            # the table's dense gradient exactly as autograd builds it for `table[ids]`: zeros + index_put_(accumulate)
            dT = torch.zeros_like(table).index_put_((ids,), dX, accumulate=True)
        return dT, None, dW, db


def linear_rows(table, ids, W, b=None):
    """linear(table[ids], W, b) -- the projection of the listed rows of a feature table (freedom.py:205-209, bm3.py:102-104
    under `lazy_projection`) -- WITHOUT the [len(ids), F] copy of the rows: the kernels of `linear` read row ids[j] of the
    table where they read row j of X (mmrec_linear_rows_*, ABI 15).  Y, dW, db and the rows of dX equal `linear` on
    `table.index_select(0, ids)` bit for bit; the table's gradient is built from the compact dX by the call autograd makes for
    `table[ids]` (a zero-filled buffer + index_put_(accumulate=True)).
    Served by the kernels (`linear_rows_served`): device fp32 tensors, W [64, F], F % 128 == 0, a contiguous table, int64 ids,
    `LINEAR_F16X3` on.  There an id outside [0, n_rows) -- -1 = "no row" -- reads as a row of zeros (Y = b, nothing in dW)
    and is never used as an address; such ids are only meaningful while the table itself wants no gradient.
    EVERY OTHER CASE (CPU tensors, other widths, a non-contiguous table, the split projection switched off) is the composition
    `linear(table.index_select(0, ids), W, b)` through this module's `linear`: a fallback to the two-step form, not a CPU path
    of the kernel."""
    if linear_rows_served(table, ids, W):
        return _LinearRows.apply(table, ids, W, b)
    return linear(table.index_select(0, ids), W, b)       # (module-level name, looked up now: test stand-ins patch it)


# ------------------------------------------------------------------------------------------------
# P5 / P6  fused score + mask + top-K
# ------------------------------------------------------------------------------------------------
def mask_to_csr(mask, n_rows, device):
    """[2, n] (row, item) mask of EvalDataLoader (dataloader.py:359-368) -> CSR with item ids sorted
    inside each row (the kernel binary-searches them).  Host side, integer exact."""
    m = mask.detach().cpu().numpy() if isinstance(mask, torch.Tensor) else np.asarray(mask)
    m = m.astype(np.int64)
    order = np.lexsort((m[1], m[0]))
    rowptr = np.zeros(n_rows + 1, dtype=np.int64)
    np.cumsum(np.bincount(m[0], minlength=n_rows), out=rowptr[1:])
    return (torch.from_numpy(rowptr.astype(np.int32)).to(device),
            torch.from_numpy(m[1][order].astype(np.int32)).to(device))


TOPK_NO_FILTER = 1


class TopkCandidates:
    """A candidate table [nc, kd] together with the candidate side of the fp16 top-K filter (column means, centred fp16
    copy, norms: mmrec_topk_prepare_f32), computed ONCE for all the query blocks ranked against it -- the batches of one
    evaluation and its valid / test pair (trainer.py:262,271,298-310: the item table is frozen while evaluating).
    `score_topk(Q, TopkCandidates(C), ...)` == `score_topk(Q, C, ...)` bit for bit.  Valid while C is unchanged."""

    def __init__(self, C):
        lib = _lib.load()
        self.C = _chk(C.contiguous(), torch.float32, "C", 2)
        nc, kd = self.C.shape
        nbytes = lib.mmrec_topk_prepared_bytes(nc, kd)
        self.prepared = None
        if nbytes:          # 0: the filter does not serve this shape; calls take the plain entry point
            self.prepared = _ws(nbytes, self.C.device)
            _lib.check(lib.mmrec_topk_prepare_f32(_p(self.C), nc, kd, _p(self.prepared), _stream()), "topk_prepare")


def topk_hint_served(nc, kd, k):
    """does the warm entry point (mmrec_score_topk_hinted_f32) serve this candidate table / k?  (the fp16 filter's shapes)"""
    return k <= TOPK_MAX and _lib.load().mmrec_topk_prepared_bytes(int(nc), int(kd)) > 0


TOPK_HINT_COLD, TOPK_HINT_KEEP = 1, 2


def topk_hint_width(k):
    """natural width of a list table for top-k calls: the final kernel ranks 64 (k <= 64) or 128 survivors anyway"""
    return 64 if k <= 64 else 128


def score_topk(Q, C, k, mask_rowptr=None, mask_col=None, return_values=False, use_filter=True, hint=None, hint_rows=None,
               queue_counts=None, hint_cold=False, hint_update=True):
    """top-k over candidates c of <Q[q], C[c]> per query with masked candidates at -1e10; never
    materialises the score matrix.  Returns int64 [nq, k] sorted by score desc (ties: lower id).
    C: a tensor, or a TopkCandidates (the candidate-side preparation of the fp16 filter done once for many calls).
    use_filter=False keeps the materialised fp32 path where the fp16 filter would serve the call (A/B measurements).
    hint (int32 [rows, k <= hk <= 128], IN / OUT, with hint_rows int64 [nq] or one row per query): a WARM call -- per query a
    list of ids expected to rank high (what a previous call left in the row for the same user); the filter takes its threshold
    from them and runs ONE matrix-core pass instead of two, and (hint_update) leaves this call's ranking -- top-k + runners-up
    -- in the row.  hint_cold: the rows are only written (the first evaluation).  The result does not depend on the hint
    (bit-identical to the plain call); shapes the filter does not serve ignore it.  queue_counts (int32 [2], device): +=
    queries the slow / overflow queues served."""
    lib = _lib.load()
    Q = _chk(Q.contiguous(), torch.float32, "Q", 2)
    prepared = None
    if isinstance(C, TopkCandidates):
        C, prepared = C.C, (C.prepared if use_filter else None)
    C = _chk(C.contiguous(), torch.float32, "C", 2)
    nq, kd = Q.shape
    nc = C.shape[0]
    if C.shape[1] != kd:
        raise _lib.MMRecHipError("Q and C must share the inner dim")
    if mask_rowptr is not None:
        _chk(mask_rowptr, torch.int32, "mask_rowptr", 1)
        if mask_col is None or mask_col.numel() == 0:
            mask_col = torch.zeros(1, dtype=torch.int32, device=Q.device)
        _chk(mask_col, torch.int32, "mask_col", 1)
    if hint is not None and not (use_filter and nc >= k and topk_hint_served(nc, kd, k)):
        hint = None
    if hint is not None:
        _chk(hint, torch.int32, "hint", 2)
        if hint.shape[1] < k or hint.shape[1] > TOPK_MAX:
            raise _lib.MMRecHipError("hint rows hold k <= hk <= %d ids, got %d for k = %d" % (TOPK_MAX, hint.shape[1], k))
        if hint_rows is not None:
            _chk(hint_rows, torch.int64, "hint_rows", 1)
            if hint_rows.numel() != nq:
                raise _lib.MMRecHipError("hint_rows: one row index per query")
        elif hint.shape[0] != nq:
            raise _lib.MMRecHipError("hint: one row per query (or pass hint_rows)")
        if queue_counts is not None:
            _chk(queue_counts, torch.int32, "queue_counts", 1)
    if nq > 2 * TOPK_QUERY_BLOCK and use_filter and (prepared is not None or lib.mmrec_topk_prepared_bytes(nc, kd) > 0):
        return _score_topk_blocked(Q, C, prepared, k, mask_rowptr, mask_col, return_values, hint, hint_rows, queue_counts,
                                   hint_cold, hint_update)
    idx = torch.empty(nq, k, dtype=torch.int64, device=Q.device)
    val = torch.empty(nq, k, dtype=torch.float32, device=Q.device) if return_values else None
    ws = _ws(lib.mmrec_topk_workspace_bytes(nq, nc, kd, k), Q.device)
    if hint is not None:
        _lib.check(lib.mmrec_score_topk_hinted_f32(_p(Q), _p(C), _p(prepared), nq, nc, kd, _p(mask_rowptr), _p(mask_col), k,
                                                   _p(hint), hint.shape[1], _p(hint_rows), _p(idx), _p(val), _p(ws),
                                                   _p(queue_counts), (TOPK_HINT_COLD if hint_cold else 0) |
                                                   (0 if hint_update else TOPK_HINT_KEEP), _stream()), "score_topk_hinted")
    elif prepared is not None:
        _lib.check(lib.mmrec_score_topk_prepared_f32(_p(Q), _p(C), _p(prepared), nq, nc, kd, _p(mask_rowptr), _p(mask_col), k,
                                                     _p(idx), _p(val), _p(ws), 0, _stream()), "score_topk_prepared")
    else:
        _lib.check(lib.mmrec_score_topk_f32(_p(Q), _p(C), nq, nc, kd, _p(mask_rowptr), _p(mask_col), k,
                                            _p(idx), _p(val), _p(ws), 0 if use_filter else TOPK_NO_FILTER, _stream()),
                   "score_topk")
    return (idx, val) if return_values else idx


TOPK_QUERY_BLOCK = 65536     # the Trainer's `hip_eval_batch_size`: 256 query blocks x 16 candidate ranges = 8 exact rounds of workgroups


def _score_topk_blocked(Q, C, prepared, k, mask_rowptr, mask_col, return_values, hint=None, hint_rows=None, queue_counts=None,
                        hint_cold=False, hint_update=True):
    """Very many queries in ONE call (a script ranking all 1M users at once): the fp16 filter's workspace is per query
    (~16 KB of word list at 500K candidates: 16 GB for 1M queries), so the call is walked in blocks of TOPK_QUERY_BLOCK queries
    against ONE preparation of the candidates -- what the Trainer's evaluation batches amount to.  One small device -> host
    read of the blocks' mask offsets (not for use under graph capture)."""
    nq = Q.shape[0]
    cands = TopkCandidates.__new__(TopkCandidates)
    cands.C = C
    cands.prepared = prepared if prepared is not None else TopkCandidates(C).prepared
    starts = list(range(0, nq, TOPK_QUERY_BLOCK))
    offs = None
    if mask_rowptr is not None:
        offs = mask_rowptr[torch.tensor(starts + [nq], device=mask_rowptr.device)].cpu().tolist()
    idx = torch.empty(nq, k, dtype=torch.int64, device=Q.device)
    val = torch.empty(nq, k, dtype=torch.float32, device=Q.device) if return_values else None
    for j, a in enumerate(starts):
        b = min(a + TOPK_QUERY_BLOCK, nq)
        rp = col = None
        if mask_rowptr is not None:
            rp = (mask_rowptr[a:b + 1] - offs[j]).contiguous()
            col = mask_col[offs[j]:max(offs[j + 1], offs[j] + 1)].contiguous()
        h = hr = None
        if hint is not None:
            h, hr = (hint, hint_rows[a:b]) if hint_rows is not None else (hint[a:b], None)
        out = score_topk(Q[a:b], cands, k, rp, col, return_values=return_values, hint=h, hint_rows=hr, queue_counts=queue_counts,
                         hint_cold=hint_cold, hint_update=hint_update)
        if return_values:
            idx[a:b], val[a:b] = out
        else:
            idx[a:b] = out
    return (idx, val) if return_values else idx


# ------------------------------------------------------------------------------------------------
# P1  graph build on device
# ------------------------------------------------------------------------------------------------
def degree_count(ids, n_bins):
    lib = _lib.load()
    _chk(ids, torch.int64, "ids", 1)
    counts = torch.zeros(n_bins, dtype=torch.int32, device=ids.device)
    _lib.check(lib.mmrec_degree_count_i32(_p(ids), ids.numel(), _p(counts), n_bins, _stream()),
               "degree_count")
    return counts


def edge_norm_values(eu, ei, n_users, n_items):
    """(du+1e-7)^-1/2 (di+1e-7)^-1/2 per edge in fp32 (freedom.py:145-154)."""
    lib = _lib.load()
    du, di = degree_count(eu, n_users), degree_count(ei, n_items)
    val = torch.empty(eu.numel(), dtype=torch.float32, device=eu.device)
    _lib.check(lib.mmrec_edge_norm_f32(_p(eu), _p(ei), eu.numel(), _p(du), _p(di), _p(val), _stream()),
               "edge_norm")
    return val


def bipartite_graph_from_edges(eu, ei, n_users, n_items, long_row_threshold=LONG_ROW_DEFAULT):
    """Symmetric normalised adjacency of the given (user,item) edges as a CsrGraph, built on device:
    re-normalise on this edge set, expand to cat(edges, flipped) and stable-sort into CSR.
    replaces pre_epoch_processing's masked_adj build (freedom.py:136-143, layergcn.py:63-70)."""
    lib = _lib.load()
    eu, ei = _chk(eu.contiguous(), torch.int64, "eu", 1), _chk(ei.contiguous(), torch.int64, "ei", 1)
    E, dev = eu.numel(), eu.device
    w = edge_norm_values(eu, ei, n_users, n_items)
    rows = torch.empty(2 * E, dtype=torch.int32, device=dev)
    cols = torch.empty(2 * E, dtype=torch.int32, device=dev)
    vals = torch.empty(2 * E, dtype=torch.float32, device=dev)
    _lib.check(lib.mmrec_bipartite_expand(_p(eu), _p(ei), _p(w), E, n_users, _p(rows), _p(cols),
                                          _p(vals), _stream()), "bipartite_expand")
    n = n_users + n_items
    return CsrGraph.from_coo_device(rows, cols, vals, n, n, symmetric=True,
                                    long_row_threshold=long_row_threshold)


# ------------------------------------------------------------------------------------------------
# SpMM with differentiable VALUES (LATTICE's learned item graph, lattice.py:137-163)
# ------------------------------------------------------------------------------------------------
class DynGraph:
    """Structure (rows, cols) of a sparse matrix whose values carry gradient and change every build.

    The CSR structure and its transpose are derived on the device (stable sort of the row / column
    ids: plumbing), the HIP SpMM does the arithmetic; `perm` maps the caller's COO order to CSR order so
    a values tensor can be re-used without rebuilding anything."""

    def __init__(self, rows, cols, n_rows, n_cols, long_row_threshold=LONG_ROW_DEFAULT):
        _chk(rows, torch.int64, "rows", 1), _chk(cols, torch.int64, "cols", 1)
        self.rows, self.cols, self.n_rows, self.n_cols = rows, cols, int(n_rows), int(n_cols)
        dev = rows.device
        zeros = torch.zeros(rows.numel(), dtype=torch.float32, device=dev)

        def build(r, c, nr, nc):
            perm = torch.sort(r, stable=True)[1]
            rowptr = torch.zeros(nr + 1, dtype=torch.int64, device=dev)
            rowptr[1:] = torch.cumsum(torch.bincount(r, minlength=nr), 0)
            g = CsrGraph(rowptr.to(torch.int32), c[perm].to(torch.int32).contiguous(), zeros, nr, nc,
                         long_row_threshold=long_row_threshold, row_schedule=False)   # the values change every call
            return g, perm
        self.fwd, self.perm = build(rows, cols, self.n_rows, self.n_cols)
        self.bwd, self.perm_t = build(cols, rows, self.n_cols, self.n_rows)
        self._long_rows = {}                               # by -> device list (or None) for the per-row edge ops: `side`

    def side(self, by):
        """(CsrGraph, perm, long_rows or None, n_long) of one direction, by="row" or "col", for the per-row edge ops (segment
        softmax, edge attention, neighbour max).  The long-row list is built on the host once per DynGraph and direction and
        checked against the row lengths (`segment_long_rows`)."""
        if by not in ("row", "col"):
            raise ValueError("DynGraph.side: by must be 'row' or 'col', got %r" % (by,))
        g, perm = (self.fwd, self.perm) if by == "row" else (self.bwd, self.perm_t)
        if by not in self._long_rows:
            lr = segment_long_rows(g.rowptr_host)
            self._long_rows[by] = torch.from_numpy(lr).to(g.rowptr.device) if lr.size else None
        lr = self._long_rows[by]
        return g, perm, lr, 0 if lr is None else lr.numel()


class _SpMMVals(torch.autograd.Function):
    @staticmethod
    def forward(ctx, X, vals, dyn):
        X = X.contiguous()
        dyn.fwd.vals = vals.detach()[dyn.perm].contiguous()
        Y = torch.empty(dyn.n_rows, X.shape[1], dtype=torch.float32, device=X.device)
        spmm_raw(dyn.fwd, X, Y=Y)
        ctx.dyn = dyn
        ctx.save_for_backward(X, vals)
        return Y

    @staticmethod
    def backward(ctx, dY):
        dyn = ctx.dyn
        X, vals = ctx.saved_tensors
        dY = dY.contiguous()
        dX = dvals = None
        if ctx.needs_input_grad[0]:
            dyn.bwd.vals = vals.detach()[dyn.perm_t].contiguous()
            dX = torch.empty(dyn.n_cols, X.shape[1], dtype=torch.float32, device=dY.device)
            spmm_raw(dyn.bwd, dY, Y=dX)
        if ctx.needs_input_grad[1]:                        # d val_e = <dY[row_e], X[col_e]>
            if edge_dot_served(dY, X, dyn.rows, dyn.cols):
                dvals = _edge_dot_fwd(dY, X, dyn.rows, dyn.cols)
            else:
                dvals = (dY[dyn.rows] * X[dyn.cols]).sum(-1)
        return dX, dvals, None


def spmm_vals(dyn: DynGraph, X, vals):
    """A(vals) @ X, differentiable in X and in the per-entry values (COO order of `dyn`), at every width `spmm_raw` serves.
    The values' gradient is one dot product per entry: the SDDMM kernel (`EDGE_DOT`), no [n_edges, d] copies."""
    return _SpMMVals.apply(X, vals, dyn)


# ------------------------------------------------------------------------------------------------
# Edge dropout inside the SpMM (common/encoders.py:77-103): fixed values, a fresh keep mask per call, one bit per entry
# (mmrec_edge_keep_bits, mmrec_spmm_csr_masked_f32; additive to ABI 16)
# ------------------------------------------------------------------------------------------------
EDGE_DROPOUT = True   # False: both edge-dropout ops are the spmm_vals / stack().mean() composition (A/B runs)


class EdgeDropoutGraph:
    """A `DynGraph` with a FIXED value vector `vals` [E] (fp32, the DynGraph's edge order, no gradient) whose entries are
    dropped per call by a keep mask.  The two permuted value copies (CSR order, transposed CSR order) are made here, once;
    `dyn.fwd.vals` / `dyn.bwd.vals` are not touched, so the same DynGraph keeps serving `spmm_vals`."""

    def __init__(self, dyn, vals):
        if not isinstance(dyn, DynGraph):
            raise _lib.MMRecHipError("EdgeDropoutGraph wants a DynGraph")
        if not isinstance(vals, torch.Tensor) or vals.dtype != torch.float32 or vals.dim() != 1:
            raise _lib.MMRecHipError("vals must be a 1-d float32 tensor")
        if vals.numel() != dyn.rows.numel():
            raise _lib.MMRecHipError("vals must have one value per edge of the DynGraph (%d), got %d" %
                                     (dyn.rows.numel(), vals.numel()))
        if vals.requires_grad:
            raise _lib.MMRecHipError("vals must not require grad: the masked product is differentiable in X only "
                                     "(learned values: spmm_vals)")
        _chk(vals, torch.float32, "vals", 1)
        self.dyn, self.vals, self.n_edges = dyn, vals, int(vals.numel())
        self.vals_fwd = vals[dyn.perm].contiguous()
        self.vals_bwd = vals[dyn.perm_t].contiguous()


def _edge_dropout_check(eg, X, keep):
    """the host checks of both ops, before any launch (shapes and types first, so that they speak without a device too)"""
    if not isinstance(eg, EdgeDropoutGraph):
        raise _lib.MMRecHipError("eg must be an EdgeDropoutGraph")
    if eg.vals.requires_grad:
        raise _lib.MMRecHipError("vals must not require grad")
    if not isinstance(keep, torch.Tensor) or keep.dtype != torch.bool or keep.dim() != 1:
        raise _lib.MMRecHipError("keep must be a 1-d torch.bool tensor in edge order")
    if keep.numel() != eg.n_edges:
        raise _lib.MMRecHipError("keep must have one flag per edge (%d), got %d" % (eg.n_edges, keep.numel()))
    if not isinstance(X, torch.Tensor) or X.dim() != 2 or X.dtype != torch.float32:
        raise _lib.MMRecHipError("X must be a 2-d float32 tensor")
    if X.shape[0] < eg.dyn.n_cols:
        raise _lib.MMRecHipError("X must have at least %d rows, got %d" % (eg.dyn.n_cols, X.shape[0]))
    if not (X.is_cuda and keep.is_cuda and eg.vals.is_cuda):
        raise _lib.MMRecHipError("X, keep and vals must be device tensors (the hot path has no CPU fallback)")


def edge_dropout_served(eg, X):
    """True where the edge-dropout ops run the masked kernels: the `EDGE_DROPOUT` switch on, X 64 k <= 384 wide (the feature
    slices have no masked form) and the entry positions within int32.  Otherwise they run the composition of the older
    kernels, `spmm_vals` on the zero-valued form."""
    d = X.shape[1]
    return bool(EDGE_DROPOUT and d > 0 and d % EMB_DIM == 0 and d <= 6 * EMB_DIM and eg.n_edges < 2 ** 31)


def edge_keep_bits(keep, perm_a=None, perm_b=None, two=False):
    """keep [E] (bool / uint8, edge order) -> packed int32 words, bit j = keep[perm[j]] (None: identity), for one order or
    (`two`, or a `perm_b`) two in ONE launch; bits past E are zero.  Returns (bits_a, bits_b or None)."""
    if not isinstance(keep, torch.Tensor) or keep.dtype not in (torch.bool, torch.uint8) or keep.dim() != 1:
        raise _lib.MMRecHipError("keep must be a 1-d bool / uint8 tensor")
    if not keep.is_cuda or not keep.is_contiguous():
        raise _lib.MMRecHipError("keep must be a contiguous device tensor")
    E = keep.numel()
    for t, nm in ((perm_a, "perm_a"), (perm_b, "perm_b")):
        if t is not None and _chk(t, torch.int64, nm, 1).numel() != E:
            raise _lib.MMRecHipError("%s must have %d entries" % (nm, E))
    two = two or perm_b is not None
    lib = _lib.load()
    words = torch.zeros(2 if two else 1, max((E + 31) // 32, 1), dtype=torch.int32, device=keep.device)
    k8 = keep.view(torch.uint8)
    _lib.check(lib.mmrec_edge_keep_bits(_p(k8), E, _p(perm_a), _p(words[0]), _p(perm_b), _p(words[1]) if two else None,
                                        _stream()), "edge_keep_bits")
    return words[0], (words[1] if two else None)


def spmm_masked_raw(g: CsrGraph, vals, keep_bits, X, Y=None, Z=None, acc_in=None, acc_out=None, alpha=1.0, beta=1.0,
                    acc_scale=1.0, val_scale=1.0, tickets=True):
    """spmm_raw on the CSR of `g` with the values `vals` [nnz] (CSR order; g.vals is not read) and the entries whose bit of
    `keep_bits` is clear removed.  `tickets=False`: the two-launch finish.  No autograd."""
    lib = _lib.load()
    _chk(X, torch.float32, "X", 2), _chk(vals, torch.float32, "vals", 1), _chk(keep_bits, torch.int32, "keep_bits", 1)
    d = X.shape[1]
    if d % EMB_DIM or d > 6 * EMB_DIM or X.shape[0] < g.n_cols:
        raise _lib.MMRecHipError("X must be [>=%d, 64*k <= 384], got %s" % (g.n_cols, tuple(X.shape)))
    if vals.numel() != g.nnz or keep_bits.numel() * 32 < g.nnz:
        raise _lib.MMRecHipError("vals must be [%d] and keep_bits hold a bit for each" % g.nnz)
    for t, nm in ((Y, "Y"), (Z, "Z"), (acc_in, "acc_in"), (acc_out, "acc_out")):
        if t is not None:
            _chk(t, torch.float32, nm, 2)
            if t.shape[0] < g.n_rows or t.shape[1] != d:
                raise _lib.MMRecHipError("%s must be [>=%d, %d]" % (nm, g.n_rows, d))
    g.checked(lib.mmrec_spmm_csr_masked_f32(_p(g.rowptr), _p(g.colidx), _p(vals), _p(X), _p(Y), _p(Z), _p(acc_in),
                                            _p(acc_out), g.n_rows, d, float(alpha), float(beta), float(acc_scale),
                                            g.long_row_threshold, _p(g.long_rows), _p(g.long_chunk_ptr), g.n_long,
                                            g.n_chunks, _p(g.partials_for(d)), _p(g.long_tickets) if tickets else None,
                                            _p(keep_bits), float(val_scale), _stream()), "spmm_csr_masked_f32")
    return Y if Y is not None else acc_out


def _edge_dropout_values(eg, keep, scale):
    """the zero-valued form of the masked matrix: what the composition feeds spmm_vals"""
    return (eg.vals * keep.to(eg.vals.dtype)) * scale


def _spmm_edge_dropout_composed(eg, X, keep, scale):
    return spmm_vals(eg.dyn, X, _edge_dropout_values(eg, keep, scale))


def _lightgcn_mean_edge_dropout_composed(eg, E0, n_layers, keep, scale):
    vals = _edge_dropout_values(eg, keep, scale)
    layers = [E0]
    for _ in range(int(n_layers)):
        E0 = spmm_vals(eg.dyn, E0, vals)
        layers.append(E0)
    return torch.stack(layers, dim=1).mean(dim=1)


class _SpMMEdgeDropout(torch.autograd.Function):
    @staticmethod
    def forward(ctx, X, eg, keep, scale):
        dyn = eg.dyn
        X = X.contiguous()
        bits_f, bits_b = edge_keep_bits(keep, dyn.perm, dyn.perm_t)     # both orders, one launch
        Y = torch.empty(dyn.n_rows, X.shape[1], dtype=torch.float32, device=X.device)
        spmm_masked_raw(dyn.fwd, eg.vals_fwd, bits_f, X, Y=Y, val_scale=scale)
        ctx.eg, ctx.scale, ctx.x_rows = eg, scale, X.shape[0]
        ctx.save_for_backward(bits_b)
        return Y

    @staticmethod
    def backward(ctx, dY):
        bits_b, = ctx.saved_tensors
        eg, dyn = ctx.eg, ctx.eg.dyn
        if not ctx.needs_input_grad[0]:
            return None, None, None, None
        dY = dY.contiguous()
        # X may carry more rows than the graph has columns: they receive no gradient
        alloc = torch.empty if ctx.x_rows == dyn.n_cols else torch.zeros
        dX = alloc(ctx.x_rows, dY.shape[1], dtype=torch.float32, device=dY.device)
        spmm_masked_raw(dyn.bwd, eg.vals_bwd, bits_b, dY, Y=dX, val_scale=ctx.scale)
        return dX, None, None, None


def spmm_edge_dropout(eg: EdgeDropoutGraph, X, keep, scale=1.0):
    """(scale * (A o keep)) @ X, differentiable in X: A the fixed values of `eg`, keep a torch.bool [E] in edge order.  The
    dropped entries are absent -- never gathered -- not zeros (sparse_dropout, encoders.py:92-103).  One pack launch for
    both orders in the forward; the backward is one masked launch on the transposed side."""
    _edge_dropout_check(eg, X, keep)
    if not edge_dropout_served(eg, X):
        return _spmm_edge_dropout_composed(eg, X, keep, scale)
    return _SpMMEdgeDropout.apply(X, eg, keep, float(scale))


class _LightGCNMeanEdgeDropout(torch.autograd.Function):
    """_LightGCNMean on the masked matrix: L masked launches accumulating through the epilogue, Horner backward on the
    transposed side, one pack per call"""

    @staticmethod
    def forward(ctx, E0, eg, n_layers, keep, scale):
        ctx.eg, ctx.L, ctx.scale = eg, int(n_layers), scale
        dyn, L = eg.dyn, int(n_layers)
        E0 = E0.contiguous()
        if L == 0:
            return E0.clone()
        bits_f, bits_b = edge_keep_bits(keep, dyn.perm, dyn.perm_t)
        ctx.save_for_backward(bits_b)
        acc = torch.empty_like(E0)
        bufs = [torch.empty_like(E0) if L > 1 else None, torch.empty_like(E0) if L > 2 else None]
        cur = E0
        for layer in range(1, L + 1):
            last = layer == L
            Y = None if last else bufs[(layer - 1) % 2]
            spmm_masked_raw(dyn.fwd, eg.vals_fwd, bits_f, cur, Y=Y, acc_in=E0 if layer == 1 else acc, acc_out=acc,
                            acc_scale=1.0 / (L + 1) if last else 1.0, val_scale=scale)
            cur = Y
        return acc

    @staticmethod
    def backward(ctx, dOut):
        L, eg = ctx.L, ctx.eg
        dOut = dOut.contiguous()
        if L == 0:
            return dOut, None, None, None, None
        bits_b, = ctx.saved_tensors
        s = 1.0 / (L + 1)
        bufs = [torch.empty_like(dOut), torch.empty_like(dOut) if L > 1 else None]
        t = dOut
        for j in range(L):  # t <- s*dOut + A^T t   (first step also scales the inner term)
            out = bufs[j % 2]
            spmm_masked_raw(eg.dyn.bwd, eg.vals_bwd, bits_b, t, Y=out, Z=dOut, alpha=s if j == 0 else 1.0, beta=s,
                            val_scale=ctx.scale)
            t = out
        return t, None, None, None, None


def lightgcn_mean_edge_dropout(eg: EdgeDropoutGraph, E0, n_layers, keep, scale=1.0):
    """1/(L+1) * sum_{l=0..L} (scale * (A o keep))^l E0 on a square graph: the dropout branch of LightGCN_Encoder
    (encoders.py:105-127) with the layer mean in the SpMM's accumulator epilogue, as `lightgcn_mean` has it."""
    _edge_dropout_check(eg, E0, keep)
    if eg.dyn.n_rows != eg.dyn.n_cols or E0.shape[0] != eg.dyn.n_rows:
        raise _lib.MMRecHipError("lightgcn_mean_edge_dropout wants a square graph and E0 [n, d]")
    if int(n_layers) < 0:
        raise _lib.MMRecHipError("n_layers must be >= 0")
    if not edge_dropout_served(eg, E0):
        return _lightgcn_mean_edge_dropout_composed(eg, E0, n_layers, keep, scale)
    return _LightGCNMeanEdgeDropout.apply(E0, eg, int(n_layers), keep, float(scale))


# ------------------------------------------------------------------------------------------------
# Per-edge dot products (SDDMM): the other half of the learned-values pattern (mmrec_edge_dot_*, ABI 16)
# ------------------------------------------------------------------------------------------------
EDGE_DOT = True       # False: every edge_dot call (and d vals of spmm_vals) is the gather-multiply-reduce composition (A/B runs)


def _edge_width_served(d):
    return d in SLICE_WIDTHS or (d > 0 and d % EMB_DIM == 0 and d <= 6 * EMB_DIM)


def edge_dot_served(A, B, rows, cols):
    """True where `edge_dot` runs the kernels (mmrec_edge_dot_*): device fp32 contiguous 2-D A, B of one served width (8 /
    16 / 32 or 64 k <= 384: spmm_raw's), int64 1-D device rows / cols of equal length, and the `EDGE_DOT` switch on."""
    def ids(t):
        return isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.int64 and t.dim() == 1 and t.is_contiguous()
    return bool(EDGE_DOT and _dev_table(A) and _dev_table(B) and A.shape[1] == B.shape[1] and _edge_width_served(A.shape[1]) and
                ids(rows) and ids(cols) and rows.numel() == cols.numel())


def _edge_dot_fwd(A, B, rows, cols):
    lib = _lib.load()
    out = torch.empty(rows.numel(), dtype=torch.float32, device=A.device)
    _lib.check(lib.mmrec_edge_dot_f32(_p(A), A.shape[0], _p(B), B.shape[0], _p(rows), _p(cols), rows.numel(), A.shape[1],
                                      _p(out), _stream()), "edge_dot")
    return out


class _EdgeDot(torch.autograd.Function):
    """forward(A, B or None for `A is B`, rows, cols, dyn)"""

    @staticmethod
    def forward(ctx, A, B, rows, cols, dyn):
        ctx.same = B is None
        if ctx.same:
            B = A
        ctx.dyn, ctx.deterministic = dyn, DETERMINISTIC
        ctx.save_for_backward(A, B, rows, cols)
        return _edge_dot_fwd(A, B, rows, cols)

    @staticmethod
    def backward(ctx, g):
        A, B, rows, cols = ctx.saved_tensors
        dyn, same = ctx.dyn, ctx.same
        want_a, want_b = ctx.needs_input_grad[0], (ctx.needs_input_grad[0] if same else ctx.needs_input_grad[1])
        g = g.contiguous()
        dA = dB = None
        if dyn is None and ctx.deterministic and rows.numel():
            dyn = DynGraph(rows, cols, A.shape[0], B.shape[0])
        if dyn is not None:
            # the two sums as SpMMs over the edge list's CSR forms: CSR order, long rows on the chunk plan, no atomics
            if want_a:
                dyn.fwd.vals = g[dyn.perm].contiguous()
                dA = spmm_raw(dyn.fwd, B, Y=torch.empty(dyn.n_rows, A.shape[1], dtype=torch.float32, device=A.device))
            if want_b:
                dyn.bwd.vals = g[dyn.perm_t].contiguous()
                dB = spmm_raw(dyn.bwd, A, Y=torch.empty(dyn.n_cols, A.shape[1], dtype=torch.float32, device=A.device))
            if same:
                return (dA + dB if want_a else None), None, None, None, None
            return dA, dB, None, None, None
        if want_a:
            dA = torch.zeros_like(A)
        if same:
            dB = dA
        elif want_b:
            dB = torch.zeros_like(B)
        if want_a or want_b:
            _lib.check(_lib.load().mmrec_edge_dot_bwd_f32(_p(g), _p(A), A.shape[0], _p(B), B.shape[0], _p(rows), _p(cols),
                                                          rows.numel(), A.shape[1], _p(dA), _p(dB), _stream()), "edge_dot_bwd")
        return dA, (None if same else dB), None, None, None


def edge_dot(A, B, rows, cols, dyn=None):
    """out[e] = <A[rows[e]], B[cols[e]]> -- one dot product per edge (SDDMM): LATTICE's learned similarities of the kNN pairs
    (lattice.py:141,146 restricted to the kept pairs), GRCN's edge scores (grcn.py:63) -- WITHOUT the two [n_edges, d] gathered
    copies; differentiable in A and B.
    Served by the kernels (`edge_dot_served`): device fp32 contiguous tables of one width among 8 / 16 / 32 / 64 k <= 384, int64
    device ids, `EDGE_DOT` on.  There an id outside its table (-1 = "no edge") gives 0, adds nothing to the gradients and is
    never used as an address.  The forward's bits repeat run after run.  The backward is
      * with `dyn` (a DynGraph over EXACTLY these rows, cols -- n_rows = len(A), n_cols = len(B)), or under `DETERMINISTIC`
        (a DynGraph is then built): dA = spmm_raw(dyn.fwd with values g[dyn.perm], B), dB = spmm_raw(dyn.bwd with values
        g[dyn.perm_t], A) -- CSR order, long rows on the SpMM's chunk plan, no atomics: fixed bits, and a hub's gradient row is
        not thousands of contended atomics;
      * otherwise mmrec_edge_dot_bwd_f32: fp32 atomics into zeroed buffers (the last ulp depends on arrival order).
    `A is B`: the two gradients are summed.
    EVERY OTHER CASE (CPU tensors, other widths or dtypes, non-contiguous operands, the switch off) is the torch composition
    `(A[rows] * B[cols]).sum(-1)` with stock autograd: a fallback to the two-step form, not a CPU path of the kernel."""
    if edge_dot_served(A, B, rows, cols):
        return _EdgeDot.apply(A, None if A is B else B, rows, cols, dyn)
    return (A[rows] * B[cols]).sum(-1)


# ------------------------------------------------------------------------------------------------
# Softmax over the edges that share a node (mmrec_segment_softmax_*): between edge_dot and spmm_vals
# ------------------------------------------------------------------------------------------------
EDGE_SOFTMAX = True   # False: every edge_softmax call is the scatter / gather composition (A/B runs)


def segment_softmax_torch(score, index, n, eps=1e-16):
    """torch_geometric.utils.softmax: softmax over the entries sharing an index (eps in the denominator) -- the composition
    `edge_softmax` falls back to, and what GRCN ran before the kernel."""
    mx = torch.full((n,), float('-inf'), dtype=score.dtype, device=score.device)
    mx = mx.scatter_reduce(0, index, score.detach(), 'amax', include_self=True)
    e = (score - mx[index]).exp()
    den = torch.zeros(n, dtype=score.dtype, device=score.device).index_add_(0, index, e)
    return e / (den[index] + eps)


def segment_softmax_group_max():
    """rows longer than this go to one workgroup each (the library's constant)"""
    return int(_lib.load().mmrec_segment_softmax_group_max())


def segment_long_rows(rowptr_host):
    """The rows (int32, ascending, host) of a CSR rowptr that are longer than `segment_softmax_group_max()`: the SpMM's plan
    helper at that threshold.  Checked here against the lengths: the library cannot check a device list, and a list that
    disagrees with the kernel's constant would leave rows of the output unwritten.  One list serves the segment softmax, the
    edge attention and the neighbour max, so a library in which their three constants differ (MMREC_HIP_LIB may name any
    build) is refused here rather than served a list cut at the wrong length."""
    lib = _lib.load()
    rp = np.ascontiguousarray(rowptr_host, dtype=np.int32)
    n_rows, thr = rp.size - 1, segment_softmax_group_max()
    if not edge_attention_group_max() == neighbor_max_group_max() == thr:
        raise _lib.MMRecHipError("group maxima of the segment softmax, the edge attention and the neighbour max differ: %d, %d, %d"
                                 % (thr, edge_attention_group_max(), neighbor_max_group_max()))
    n_long, n_chunks = ctypes.c_int32(0), ctypes.c_int32(0)
    ptr = rp.ctypes.data_as(ctypes.c_void_p)
    _lib.check(lib.mmrec_spmm_plan_count(ptr, n_rows, thr, ctypes.byref(n_long), ctypes.byref(n_chunks)), "spmm_plan_count")
    lr, cp = np.empty(n_long.value, dtype=np.int32), np.empty(n_long.value + 1, dtype=np.int32)
    if n_long.value:
        _lib.check(lib.mmrec_spmm_plan_fill(ptr, n_rows, thr, lr.ctypes.data_as(ctypes.c_void_p),
                                            cp.ctypes.data_as(ctypes.c_void_p)), "spmm_plan_fill")
    want = np.flatnonzero(np.diff(rp.astype(np.int64)) > thr).astype(np.int32)
    if not np.array_equal(lr, want):
        raise _lib.MMRecHipError("segment softmax: the plan's long rows are not the rows longer than %d" % thr)
    return lr


def edge_softmax_served(score, dyn):
    """True where `edge_softmax` runs the kernels: a contiguous 1-D fp32 device tensor with one entry per edge of `dyn`, and
    the `EDGE_SOFTMAX` switch on."""
    return bool(EDGE_SOFTMAX and isinstance(score, torch.Tensor) and score.is_cuda and score.dtype == torch.float32 and
                score.dim() == 1 and score.is_contiguous() and score.numel() == dyn.rows.numel())


class _EdgeSoftmax(torch.autograd.Function):
    @staticmethod
    def forward(ctx, score, dyn, by, eps):
        g, perm, long_rows, n_long = dyn.side(by)
        alpha = torch.empty_like(score)
        _lib.check(_lib.load().mmrec_segment_softmax_f32(_p(g.rowptr), g.n_rows, _p(perm), _p(long_rows), n_long, _p(score),
                                                         score.numel(), eps, _p(alpha), _stream()), "segment_softmax")
        ctx.dyn, ctx.by = dyn, by
        ctx.save_for_backward(alpha)
        return alpha

    @staticmethod
    def backward(ctx, grad):
        (alpha,) = ctx.saved_tensors
        g, perm, long_rows, n_long = ctx.dyn.side(ctx.by)
        grad = grad.contiguous()
        ds = torch.empty_like(alpha)
        _lib.check(_lib.load().mmrec_segment_softmax_bwd_f32(_p(g.rowptr), g.n_rows, _p(perm), _p(long_rows), n_long,
                                                             _p(alpha), _p(grad), alpha.numel(), _p(ds), _stream()),
                   "segment_softmax_bwd")
        return ds, None, None, None


def edge_softmax(score, dyn, by="row", eps=1e-16):
    """Softmax of one score per edge over the edges that share `dyn.rows` (by="row") or `dyn.cols` (by="col"):
    alpha[e] = exp(s[e] - m) / (sum exp(s - m) + eps) with m the maximum of e's segment -- torch_geometric.utils.softmax, GRCN's
    attention weights (grcn.py:69).  Input and output are in the order of dyn's edge list; differentiable in `score`
    (d s[e] = alpha[e] (g[e] - sum alpha g) over the segment, from the saved alpha).
    Served by the kernels (`edge_softmax_served`): one launch forward, one backward (+ one each for the rows longer than
    `segment_softmax_group_max()`), over the CSR form the DynGraph already holds; no atomics, so both directions repeat bit
    for bit, with or without `DETERMINISTIC`.  A segment that holds a NaN, a +inf or nothing but -inf is NaN in every entry.
    EVERY OTHER CASE (CPU tensors, other dtypes, non-contiguous scores, the switch off) is `segment_softmax_torch` with stock
    autograd: the composition of scatter-max, gathers, exp, index_add and a division."""
    if edge_softmax_served(score, dyn):
        return _EdgeSoftmax.apply(score, dyn, by, float(eps))
    if by not in ("row", "col"):
        raise ValueError("edge_softmax: by must be 'row' or 'col', got %r" % (by,))
    index, n = (dyn.rows, dyn.n_rows) if by == "row" else (dyn.cols, dyn.n_cols)
    return segment_softmax_torch(score, index, n, eps)


# ------------------------------------------------------------------------------------------------
# Fused edge attention (mmrec_edge_attention_f32): edge_dot -> edge_softmax -> spmm_vals in one pass over the edges
# ------------------------------------------------------------------------------------------------
EDGE_ATTENTION = True   # False: every edge_attention call is the three-op composition (A/B runs)
EDGE_ATTENTION_BWD = True   # False: edge_attention(fused_backward=True) takes the backward composed of the older kernels (A/B runs)


def edge_attention_group_max():
    """rows longer than this go to one workgroup each (the library's constant; equal to `segment_softmax_group_max()`)"""
    return int(_lib.load().mmrec_edge_attention_group_max())


def edge_attention_served(Q, KV, dyn):
    """True where `edge_attention` runs the kernel: device fp32 contiguous [*, 64] tables with one row of Q per row of `dyn`
    and one row of KV per column, and the `EDGE_ATTENTION` switch on.  `Q is KV` is allowed."""
    def table(t, n):
        return _dev_table(t, EMB_DIM) and t.shape[0] == n
    return bool(EDGE_ATTENTION and table(Q, dyn.n_rows) and table(KV, dyn.n_cols))


def _spmm_with(g, vals, X):
    g.vals = vals
    return spmm_raw(g, X, Y=torch.empty(g.n_rows, X.shape[1], dtype=torch.float32, device=X.device))


class _EdgeAttention(torch.autograd.Function):
    """forward(Q, KV or None for `Q is KV`, dyn, eps, fused_backward) -> (Y, alpha)"""

    @staticmethod
    def forward(ctx, Q, KV, dyn, eps, fused_backward=False):
        ctx.same = KV is None
        if ctx.same:
            KV = Q
        n_edges = dyn.rows.numel()
        g, perm, long_rows, n_long = dyn.side("row")
        # every row of Y is the kernel's to write -- unless there is no edge, and then no launch
        Y = (torch.empty if n_edges else torch.zeros)(dyn.n_rows, EMB_DIM, dtype=torch.float32, device=Q.device)
        alpha = torch.empty(n_edges, dtype=torch.float32, device=Q.device)
        _lib.check(_lib.load().mmrec_edge_attention_f32(_p(g.rowptr), g.n_rows, _p(g.colidx), _p(perm), _p(long_rows), n_long,
                                                        _p(Q), Q.shape[0], _p(KV), KV.shape[0], EMB_DIM, n_edges, eps, _p(Y),
                                                        _p(alpha), _stream()), "edge_attention")
        ctx.dyn = dyn
        ctx.fused_backward = bool(fused_backward and EDGE_ATTENTION_BWD)
        ctx.set_materialize_grads(False)
        if ctx.fused_backward:
            dyn.side("col")                                     # the column side's list: host work, so here and not in backward
            ctx.save_for_backward(Q, KV, alpha, Y)
        else:
            ctx.save_for_backward(Q, KV, alpha)
        return Y, alpha

    @staticmethod
    def backward(ctx, dY, dA):
        Q, KV, alpha = ctx.saved_tensors[:3]
        dyn, same = ctx.dyn, ctx.same
        want_q, want_kv = ctx.needs_input_grad[0], (ctx.needs_input_grad[0] if same else ctx.needs_input_grad[1])
        if (dY is None and dA is None) or not (want_q or want_kv) or not alpha.numel():
            zq = torch.zeros_like(Q) if want_q else None
            return zq, (None if same or not want_kv else torch.zeros_like(KV)), None, None, None
        if ctx.fused_backward:                                  # one call: ds, dQ and dKV with every row gathered once
            fwd, perm, long_rows, n_long = dyn.side("row")      # (both lists are cached since the forward)
            bwd, perm_t, long_cols, n_long_t = dyn.side("col")
            dY = None if dY is None else dY.contiguous()
            dA = None if dA is None else dA.contiguous()
            ds = torch.empty_like(alpha)
            dQ = torch.empty_like(Q) if want_q else None
            dKV = torch.empty_like(KV) if want_kv else None
            _lib.check(_lib.load().mmrec_edge_attention_bwd_f32(
                _p(fwd.rowptr), fwd.n_rows, _p(fwd.colidx), _p(perm), _p(long_rows), n_long,
                _p(bwd.rowptr), _p(bwd.colidx), _p(perm_t), _p(long_cols), n_long_t,
                _p(Q), Q.shape[0], _p(KV), KV.shape[0], _p(ctx.saved_tensors[3]), _p(alpha), _p(dY), _p(dA), EMB_DIM,
                alpha.numel(), _p(ds), _p(dQ), _p(dKV), _p(dQ) if same else None, _stream()), "edge_attention_bwd")
            return (dKV if same else dQ), (None if same else dKV), None, None, None
        # d alpha_e = <dY[row_e], KV[col_e]> (+ what arrives at alpha itself); through the softmax from the saved alpha
        g = None
        if dY is not None:
            dY = dY.contiguous()
            g = _edge_dot_fwd(dY, KV, dyn.rows, dyn.cols)
        if dA is not None:
            g = dA.contiguous() if g is None else g + dA
        fwd, perm, long_rows, n_long = dyn.side("row")
        ds = torch.empty_like(alpha)
        _lib.check(_lib.load().mmrec_segment_softmax_bwd_f32(_p(fwd.rowptr), fwd.n_rows, _p(perm), _p(long_rows), n_long,
                                                             _p(alpha), _p(g), alpha.numel(), _p(ds), _stream()),
                   "segment_softmax_bwd")
        dQ = dKV = None
        if want_q:                                              # d s_e reaches Q[row_e] ...
            dQ = _spmm_with(dyn.fwd, ds[dyn.perm].contiguous(), KV)
        if want_kv:                                             # ... and KV[col_e], which the weighted sum reads as well
            dKV = _spmm_with(dyn.bwd, ds[dyn.perm_t].contiguous(), Q)
            if dY is not None:
                dKV = _spmm_with(dyn.bwd, alpha[dyn.perm_t].contiguous(), dY) + dKV
        if same:
            return dQ + dKV, None, None, None, None
        return dQ, dKV, None, None, None


def edge_attention(Q, KV, dyn, eps=1e-16, fused_backward=False):
    """Attention over the edges of `dyn` ("GAT aggregation"): for every edge e = (row, col) the score s_e = <Q[row], KV[col]>,
    alpha = the softmax of the scores over the edges that share a row (eps in the denominator), Y[row] = sum_e alpha_e KV[col];
    -> (Y [n_rows, 64], alpha [n_edges] in the order of dyn's edge list).  GRCN's content GCN (grcn.py:63-72).
    Served by the kernel (`edge_attention_served`): ONE launch (+ one for the rows longer than `edge_attention_group_max()`)
    that gathers every KV[col] once for both the score and the sum, instead of `edge_dot` -> `edge_softmax` -> `spmm_vals`,
    which gather it twice and write and re-read the scores and the weights; no atomics, so Y and alpha repeat bit for bit.  A
    row that holds a NaN, a +inf or nothing but -inf among its scores is NaN in its alphas and in Y.  Backward, from the saved
    Q, KV and alpha (no [n_edges] score is kept), composed of the existing kernels: g = <dY[row], KV[col]> per edge (+ the
    gradient arriving at alpha), ds = the segment softmax's backward, dQ = SpMM(dyn.fwd, ds) KV, dKV = SpMM(dyn.bwd, alpha) dY +
    SpMM(dyn.bwd, ds) Q; `Q is KV`: the two are summed.  The long-row list is built on the host at the first call on a DynGraph:
    call once before capturing a step.
    `fused_backward=True` (and the `EDGE_ATTENTION_BWD` switch on; ignored where the kernel does not serve): Y is saved as well
    and the backward is ONE call, mmrec_edge_attention_bwd_f32 -- the row's sum of alpha g is <dY[r], Y[r]> (+ sum alpha dAlpha),
    known before the row is walked, so a row pass gathers each KV[col] once for ds and dQ and a column pass over dyn.bwd gathers
    dY[row] and Q[row] once each for dKV, reading alpha and ds through perm_t: three row gathers per edge instead of five, one
    [n_edges] intermediate instead of six, no atomics (fixed bits); `Q is KV`: dQ enters the column pass as its first term.  Both
    long lists are built in the FORWARD, so the backward does no host work.
    EVERY OTHER CASE (CPU tensors, other widths or dtypes, non-contiguous tables, table lengths that are not dyn's, the switch
    off) is exactly `edge_dot` -> `edge_softmax` -> `spmm_vals` with stock autograd."""
    if edge_attention_served(Q, KV, dyn):
        return _EdgeAttention.apply(Q, None if Q is KV else KV, dyn, float(eps), bool(fused_backward))
    alpha = edge_softmax(edge_dot(Q, KV, dyn.rows, dyn.cols, dyn=dyn), dyn, eps=eps)
    return spmm_vals(dyn, KV, alpha), alpha


# ------------------------------------------------------------------------------------------------
# Max over a node's neighbours (mmrec_neighbor_max_f32): PyG's aggr='max' without the [n_edges, 64] message tensor
# ------------------------------------------------------------------------------------------------
NEIGHBOR_MAX = True   # False: every neighbor_max call is `neighbor_max_torch` (A/B runs)


def neighbor_max_group_max():
    """rows longer than this go to one workgroup each (the library's constant; equal to `segment_softmax_group_max()`)"""
    return int(_lib.load().mmrec_neighbor_max_group_max())


def neighbor_max_torch(X, rows, cols, n_rows):
    """Y[r][c] = max over the edges e with rows[e] == r of X[cols[e]][c], and arg [n_rows, d] (int32) = the edge chosen, by the
    kernel's SELECTION RULE: the first edge (lowest position among the row's edges) whose value is NaN; without a NaN the
    first that attains the maximum (-0 and +0 tied); a row without edges: Y = 0, arg = -1.  Stock autograd: an explicit
    first-maximal-edge argmin over positions, then ONE gather of X at the chosen (source, column) pairs, so the whole
    gradient of Y[r][c] goes to the chosen edge's source -- not `scatter_reduce('amax')`'s even split among ties.  This is
    the composition `neighbor_max` falls back to; its temporaries are [n_edges, d]."""
    ne, d = rows.numel(), X.shape[1]
    if ne == 0:
        return X.new_zeros(n_rows, d), torch.full((n_rows, d), -1, dtype=torch.int32, device=X.device)
    with torch.no_grad():
        msg = X.detach()[cols]
        isn = msg.isnan()
        idx = rows.unsqueeze(1).expand(ne, d)
        top = torch.full((n_rows, d), float('-inf'), dtype=X.dtype, device=X.device)
        top = top.scatter_reduce(0, idx, torch.where(isn, torch.full_like(msg, float('inf')), msg), 'amax', include_self=True)
        has_nan = torch.zeros(n_rows, d, dtype=torch.int32, device=X.device).scatter_reduce(0, idx, isn.to(torch.int32), 'amax')
        cand = torch.where(has_nan[rows] > 0, isn, ~isn & (msg == top[rows]))
        pos = torch.arange(ne, device=X.device).unsqueeze(1).expand(ne, d)
        first = torch.full((n_rows, d), ne, dtype=torch.int64, device=X.device)
        first = first.scatter_reduce(0, idx, torch.where(cand, pos, torch.full_like(pos, ne)), 'amin', include_self=True)
        some = first < ne
        src = cols[first.clamp(max=ne - 1)]
        column = torch.arange(d, device=X.device).unsqueeze(0).expand(n_rows, d)
    Y = torch.where(some, X[src, column], torch.zeros((), dtype=X.dtype, device=X.device))
    return Y, torch.where(some, first, torch.full_like(first, -1)).to(torch.int32)


def neighbor_max_served(X, dyn):
    """True where `neighbor_max` runs the kernels: a device fp32 contiguous [dyn.n_cols, 64] table over a `DynGraph` that
    holds both CSR forms, and the `NEIGHBOR_MAX` switch on."""
    return bool(NEIGHBOR_MAX and _dev_table(X, EMB_DIM) and X.shape[0] == dyn.n_cols and hasattr(dyn, "side"))


class _NeighborMax(torch.autograd.Function):
    @staticmethod
    def forward(ctx, X, dyn):
        g, perm, long_rows, n_long = dyn.side("row")
        dyn.side("col")                                         # the column side's list: host work, so here and not in backward
        n_edges = dyn.rows.numel()
        Y = torch.empty(dyn.n_rows, EMB_DIM, dtype=torch.float32, device=X.device)
        arg = torch.empty(dyn.n_rows, EMB_DIM, dtype=torch.int32, device=X.device)
        _lib.check(_lib.load().mmrec_neighbor_max_f32(_p(g.rowptr), g.n_rows, _p(g.colidx), _p(perm), _p(long_rows),
                                                      n_long, _p(X), X.shape[0], EMB_DIM, n_edges, _p(Y), _p(arg), _stream()),
                   "neighbor_max")
        ctx.dyn = dyn
        ctx.set_materialize_grads(False)
        ctx.mark_non_differentiable(arg)
        ctx.save_for_backward(arg)
        return Y, arg

    @staticmethod
    def backward(ctx, dY, _):
        if dY is None or not ctx.needs_input_grad[0]:
            return None, None
        (arg,) = ctx.saved_tensors
        dyn = ctx.dyn
        g, perm_t, long_cols, n_long_t = dyn.side("col")        # (cached since the forward)
        dY = dY.contiguous()
        dX = torch.empty(dyn.n_cols, EMB_DIM, dtype=torch.float32, device=dY.device)
        _lib.check(_lib.load().mmrec_neighbor_max_bwd_f32(_p(g.rowptr), g.n_rows, _p(g.colidx), _p(perm_t), _p(long_cols),
                                                          n_long_t, _p(arg), dyn.n_rows, _p(dY), EMB_DIM, dyn.rows.numel(), _p(dX),
                                                          None, _stream()),
                   "neighbor_max_bwd")
        return dX, None


def neighbor_max(X, dyn):
    """Max over the neighbours of every row of `dyn` (PyG's `aggr='max'`, Base_gcn of dualgnn.py:318-345 / dragon.py:387-410):
    -> (Y [n_rows, d], arg [n_rows, d] int32) with Y[r][c] = max over the edges e = (r, col) of X[col][c] and arg[r][c] the
    position in dyn's edge list of the edge chosen -- the first NaN of the row's edges, else the first that attains the
    maximum (-0 = +0); a row without edges: Y = 0, arg = -1.  Differentiable in X (the whole gradient of Y[r][c] goes to the
    chosen edge's source); `arg` is not differentiable.
    Served by the kernels (`neighbor_max_served`): one launch (+ one for the rows longer than `neighbor_max_group_max()`)
    forward over dyn.fwd / dyn.perm, one (+ one) backward -- a pull over dyn.bwd / dyn.perm_t that adds dY[r][c] where arg[r][c]
    names the slot; no [n_edges, d] tensor in either direction, no atomics: both directions repeat bit for bit.  Both long lists
    are built on the host at the first call on a DynGraph: call once before capturing a step.
    EVERY OTHER CASE (CPU tensors, other widths or dtypes, non-contiguous tables, a graph object that holds only rows / cols,
    the switch off) is `neighbor_max_torch` with stock autograd: the same rule, so the same Y bits and the same arg."""
    if neighbor_max_served(X, dyn):
        return _NeighborMax.apply(X, dyn)
    return neighbor_max_torch(X, dyn.rows, dyn.cols, dyn.n_rows)


# ------------------------------------------------------------------------------------------------
# Contrastive log-sum-exp against a whole table (mmrec_score_lse_f32): lse[i] = log sum_j exp(scale <Q[i], K[j]>)
# ------------------------------------------------------------------------------------------------
SCORE_LSE_WIDTHS = (64, 128)


def score_lse_split_cols(B, N, mode=0):
    """columns of K one workgroup of the forward sweeps (the library's plan for the shape; 0 for an empty K); mode 1: the same
    for the dQ sweep, mode 2: the rows of Q one workgroup of the dK sweep walks"""
    return int(_lib.load().mmrec_score_lse_split_cols(int(B), int(N), int(mode)))


def score_lse_served(Q, K):
    """True where `score_lse` runs the kernel: device fp32 contiguous [B, d] and [N, d] with d 64 or 128.  `Q is K` is allowed."""
    def table(t):
        return _dev_table(t, max_rows=1 << 30) and t.shape[1] in SCORE_LSE_WIDTHS
    return bool(table(Q) and table(K) and Q.shape[1] == K.shape[1])


class _ScoreLse(torch.autograd.Function):
    """forward(Q, K or None for `Q is K`, scale) -> lse [B]"""

    @staticmethod
    def forward(ctx, Q, K, scale):
        ctx.same = K is None
        if ctx.same:
            K = Q
        lib = _lib.load()
        B, N, d = Q.shape[0], K.shape[0], Q.shape[1]
        lse = torch.empty(B, dtype=torch.float32, device=Q.device)
        ws = _ws(lib.mmrec_score_lse_workspace_bytes(B, N, d), Q.device)
        _lib.check(lib.mmrec_score_lse_f32(_p(Q), _p(K), B, N, d, scale, _p(lse), _p(ws), _stream()), "score_lse")
        ctx.scale = scale
        ctx.save_for_backward(Q, K, lse)
        return lse

    @staticmethod
    def backward(ctx, g):
        Q, K, lse = ctx.saved_tensors
        same = ctx.same
        want_q, want_k = ctx.needs_input_grad[0], (ctx.needs_input_grad[0] if same else ctx.needs_input_grad[1])
        if not (want_q or want_k):
            return None, None, None
        lib = _lib.load()
        B, N, d = Q.shape[0], K.shape[0], Q.shape[1]
        g = g.contiguous()
        dQ = torch.empty_like(Q) if want_q else None
        dK = torch.empty_like(K) if want_k else None
        if B and N:
            ws = _ws(lib.mmrec_score_lse_workspace_bytes(B, N, d), Q.device)
            _lib.check(lib.mmrec_score_lse_bwd_f32(_p(Q), _p(K), B, N, d, ctx.scale, _p(lse), _p(g), _p(dQ), _p(dK), _p(ws),
                                                   _stream()), "score_lse_bwd")
        else:
            for t in (dQ, dK):
                if t is not None:
                    t.zero_()
        if same:
            return dQ + dK, None, None
        return dQ, dK, None


def score_lse(Q, K, scale=1.0):
    """lse[i] = log sum_j exp(scale <Q[i], K[j]>) -> [B], with autograd to Q and K, never holding the [B, N] logits: the
    contrastive denominator of LGMRec's hypergraph term (lgmrec.py:157-164, the batch against EVERY user / item) and of PGL's
    two-view InfoNCE (pgl.py:226-231).  Served by the kernel (`score_lse_served`: device fp32 contiguous tables of width 64 or
    128): fp32-MFMA scores with a running maximum (logits of any finite size give a finite result), 128-row tiles x column
    splits combined in a fixed order; the backward recomputes the scores from Q, K and the saved lse -- dQ[i] = scale g[i]
    sum_j p_ij K[j], dK[j] = scale sum_i g[i] p_ij Q[i], p = exp(scale s - lse) -- with both products on the MFMA.  No atomics:
    the same bits every call, so `DETERMINISTIC` changes nothing.  `Q is K`: the two gradients are added.  An empty K gives
    -inf and zero gradients, as torch.logsumexp does.
    EVERY OTHER CASE (CPU tensors, other widths or dtypes, non-contiguous operands) is exactly
    `torch.logsumexp(scale * (Q @ K.T), dim=1)` with stock autograd."""
    if score_lse_served(Q, K):
        return _ScoreLse.apply(Q, None if Q is K else K, float(scale))
    return torch.logsumexp(scale * (Q @ K.T), dim=1)


# ------------------------------------------------------------------------------------------------
# DAMRS's pseudo-labels (csrc/tri_topk.hip): top-k of a mix of three row softmaxes against three whole tables
# ------------------------------------------------------------------------------------------------
TRI_TOPK = True       # False: every tri_softmax_topk call is `tri_softmax_topk_torch`, pseudo_labels the dense composition (A/B runs)
TRI_TOPK_KMAX = 16
_DAMRS_W = {}         # device -> ones(3, 3) + eye(3)


def tri_topk_split_cols(B, N):
    """columns of the tables one workgroup of the sweep walks (the library's plan for the shape; 0 for empty tables)"""
    return int(_lib.load().mmrec_tri_topk_split_cols(int(B), int(N)))


def _tri_tables_served(tables, k):
    if not (isinstance(tables, (tuple, list)) and len(tables) == 3 and isinstance(tables[0], torch.Tensor) and tables[0].dim() == 2):
        return False
    N = tables[0].shape[0]
    return bool(all(_dev_table(t, EMB_DIM) and t.shape[0] == N for t in tables) and 1 <= k <= TRI_TOPK_KMAX and k <= N <= (1 << 30))


def tri_softmax_topk_served(tables, ids, lse, W, k):
    """True where `tri_softmax_topk` runs the kernel: three device fp32 contiguous [N, 64] tables, N >= k, 1 <= k <= 16, ids None
    or int64 [B] on the device, lse fp32 contiguous [3, B], W fp32 contiguous [3, 3], and the `TRI_TOPK` switch on."""
    if not (TRI_TOPK and _tri_tables_served(tables, k) and isinstance(lse, torch.Tensor) and lse.dim() == 2):
        return False
    B = lse.shape[1]
    dev_ids = ids is None or (isinstance(ids, torch.Tensor) and ids.is_cuda and ids.dtype == torch.int64 and
                              ids.is_contiguous() and tuple(ids.shape) == (B,))
    return bool(B <= (1 << 30) and dev_ids and _dev_table(lse, B) and lse.shape[0] == 3 and _dev_table(W, 3) and W.shape[0] == 3)


def tri_softmax_topk_torch(tables, ids, lse, W, k, return_values=False):
    """the materialised composition of `tri_softmax_topk`: S_t = sum_m W[t][m] exp(T_m[ids] T_m^T - lse[m][:, None]) as [B, N]
    blocks, sorted score descending with ties by the lower column; an id outside [0, N) gives -1 (values -inf)."""
    N, B = tables[0].shape[0], lse.shape[1]
    rows = torch.arange(B, device=lse.device) if ids is None else ids
    ok = (rows >= 0) & (rows < N)
    safe = torch.where(ok, rows, torch.zeros_like(rows))
    p = [torch.exp(T[safe] @ T.t() - lse[m][:, None]) for m, T in enumerate(tables)]
    idx, val = [], []
    for t in range(3):
        S = (W[t, 0] * p[0] + W[t, 1] * p[1]) + W[t, 2] * p[2]
        v, i = torch.sort(S, dim=1, descending=True, stable=True)
        idx.append(torch.where(ok[:, None], i[:, :k], torch.full_like(i[:, :k], -1)))
        val.append(torch.where(ok[:, None], v[:, :k], torch.full_like(v[:, :k], float("-inf"))))
    idx = torch.stack(idx)
    return (idx, torch.stack(val)) if return_values else idx


def _tri_topk_raw(tables, ids, lse, W, k, return_values):
    lib = _lib.load()
    N, B = tables[0].shape[0], lse.shape[1]
    idx = torch.empty(3, B, k, dtype=torch.int32, device=lse.device)
    val = torch.empty(3, B, k, dtype=torch.float32, device=lse.device) if return_values else None
    ws = _ws(lib.mmrec_tri_topk_workspace_bytes(B, N, k), lse.device)
    _lib.check(lib.mmrec_tri_topk_f32(_p(tables[0]), _p(tables[1]), _p(tables[2]), N, _p(ids), B, _p(lse), _p(W), k, _p(idx),
                                      _p(val), _p(ws), _stream()), "tri_topk")
    return idx, val


def tri_softmax_topk(tables, ids, lse, W, k, return_values=False):
    """For three tables T_m [N, 64] and query rows ids [B] (None: rows 0 .. B-1): list t of row r = the k columns j with the
    largest S_t[r, j] = sum_m W[t][m] exp(<T_m[ids[r]], T_m[j]> - lse[m][r]) -> int64 [3, B, k] (and the scores), score
    descending, ties by the lower column; lse [3, B] is the caller's log-sum-exp (`score_lse(T_m[ids], T_m, 1.0)`: S is then a
    mix of the three row softmaxes).  DAMRS's mm_pos lists (damrs.py:141-150) with W = ones(3, 3) + eye(3), k = 10.
    Served by the kernel (`tri_softmax_topk_served`): one sweep that never stores a [B, N] block, the same bits every call.
    No autograd: the labels carry no gradient in the reference.
    EVERY OTHER CASE (CPU tensors, other widths or dtypes, k > 16, the switch off) is `tri_softmax_topk_torch`, the materialised
    composition with the same tie rule: a fallback, not a CPU path of the kernel."""
    with torch.no_grad():
        if tri_softmax_topk_served(tables, ids, lse, W, k):
            idx, val = _tri_topk_raw(tables, ids, lse, W, k, return_values)
            return (idx.long(), val) if return_values else idx.long()
        return tri_softmax_topk_torch(tables, ids, lse, W, k, return_values)


def list_exclude(cand, excl, k):
    """row r of the result [R, k]: the first k entries of cand[r] that do not occur in excl[r], in cand's order (int32 device
    lists, cand [R, kc], excl [R, ke], kc - ke >= k: mmrec_list_exclude_i32)"""
    lib = _lib.load()
    cand, excl = _chk(cand, torch.int32, "cand", 2), _chk(excl, torch.int32, "excl", 2)
    if cand.shape[0] != excl.shape[0]:
        raise _lib.MMRecHipError("list_exclude: one row of excl per row of cand")
    out = torch.empty(cand.shape[0], k, dtype=torch.int32, device=cand.device)
    _lib.check(lib.mmrec_list_exclude_i32(_p(cand), _p(excl), cand.shape[0], cand.shape[1], excl.shape[1], k, _p(out), _stream()),
               "list_exclude")
    return out


def pseudo_labels_torch(tables, ids, k=10):
    """DAMRS's labels as its dense path computes them (damrs.py:141-150 on [b, N] blocks): p_m = softmax(T_m[ids] T_m^T), for
    target m with the others a, b: mm_pos = topk(p_a + p_b + p_m + p_m, k), single_pos = topk(p_m with mm_pos zeroed, k)."""
    with torch.no_grad():
        p = [torch.softmax(torch.mm(T[ids], T.t()), dim=1) for T in tables]
        mm, single = [], []
        for a, b, m in ((1, 2, 0), (0, 2, 1), (0, 1, 2)):      # the operand order of DAMRS.calculate_loss
            mm_pos = torch.topk(p[a] + p[b] + p[m] + p[m], k, dim=-1).indices
            mm.append(mm_pos)
            single.append(torch.topk(p[m].scatter(1, mm_pos, 0.0), k, dim=-1).indices)
        return torch.stack(mm), torch.stack(single)


PSEUDO_TOPK_BLOCK_BYTES = 64 << 20    # score_topk sizes a [queries, N] fp32 score block inside its workspace


def _top_cosines(Q, T, k2):
    """score_topk(Q, T, k2) in blocks of query rows (a multiple of 128, at least 128) whose score block stays within
    PSEUDO_TOPK_BLOCK_BYTES, the candidate side prepared once: the workspace never holds b x N scores"""
    rows = max(128, PSEUDO_TOPK_BLOCK_BYTES // (4 * (-(-T.shape[0] // 256) * 256)) // 128 * 128)
    if Q.shape[0] <= rows:
        return score_topk(Q, T, k2)
    cand = TopkCandidates(T)
    return torch.cat([score_topk(Q[r0:r0 + rows], cand, k2) for r0 in range(0, Q.shape[0], rows)])


def pseudo_labels(tables, ids, k=10):
    """DAMRS's pseudo-labels for item rows ids [b] of three ROW-NORMALISED tables (text, image, session) [N, 64] ->
    (mm_pos, single_pos), int64 [3, b, k] each, list t for target modality t -- without a [b, N] block.  Served (device fp32
    contiguous tables of width 64, int64 device ids, N >= 2 k, k <= 16, `TRI_TOPK` on), under no_grad:
      lse_m = score_lse(T_m[ids], T_m, 1.0)                       the three softmax denominators
      mm_pos = tri_softmax_topk(tables, ids, lse, ones + eye, k)  top-k of p_a + p_b + 2 p_m
      single_pos = the first k of score_topk(T_m[ids], T_m, 2 k) that are not in mm_pos[m]   (`_top_cosines`: in blocks of rows)
    -- p_m is positive and monotone in the cosine within a row, so the top-k of p_m with k entries zeroed lies inside the
    top-2k of the cosines.  Where N < 2 k or anything is unserved: `pseudo_labels_torch`, the dense composition."""
    with torch.no_grad():
        N = tables[0].shape[0] if isinstance(tables[0], torch.Tensor) and tables[0].dim() == 2 else 0
        dev_ids = isinstance(ids, torch.Tensor) and ids.is_cuda and ids.dtype == torch.int64 and ids.dim() == 1 and ids.is_contiguous()
        if not (dev_ids and N >= 2 * k and ids.numel() > 0):
            return pseudo_labels_torch(tables, ids, k)
        if not (TRI_TOPK and _tri_tables_served(tables, k) and ids.numel() <= (1 << 30)):
            return pseudo_labels_torch(tables, ids, k)
        dev = ids.device
        W = _DAMRS_W.get(dev)
        if W is None:
            W = _DAMRS_W[dev] = torch.ones(3, 3, device=dev) + torch.eye(3, device=dev)
        Q = [T[ids] for T in tables]
        lse = torch.stack([score_lse(q, T, 1.0) for q, T in zip(Q, tables)])
        mm, _ = _tri_topk_raw(tables, ids, lse, W, k, False)
        cand = torch.stack([_top_cosines(q, T, 2 * k) for q, T in zip(Q, tables)]).to(torch.int32)
        single = list_exclude(cand.view(-1, 2 * k), mm.view(-1, k), k).view(3, -1, k)
        return mm.long(), single.long()


# ------------------------------------------------------------------------------------------------
# Hypergraph message passing of LGMRec (csrc/hypergraph.hip): the Gumbel-softmax assignment with its dropout, the HGNN layer
# ------------------------------------------------------------------------------------------------
HYPER = True          # False: every hyper_* call is its `*_torch` composition (A/B runs)
HYPER_H_MAX = 8       # hyperedges the narrow kernels serve; exactly 64 (Clothing's hyper_num) is the hyper64_* family below


def hyper_rows_per_block(n):
    """rows of a side of n rows that one workgroup of the layer's reduction walks (the library's plan)"""
    return int(_lib.load().mmrec_hyper_rows_per_block(int(n)))


def _hyper_table(t, width=None):
    return _dev_table(t, width, 1 << 30) and (width is not None or 1 <= t.shape[1] <= HYPER_H_MAX)


def hyper_assign_torch(logits, noise, keep_mask=None, tau=1.0, keep_rate=1.0):
    """softmax((logits + noise) / tau) over dim 1, then `* keep_mask / keep_rate` where a mask is given: F.gumbel_softmax with
    the noise supplied, F.dropout with the mask supplied.  The composition `hyper_assign` falls back to."""
    p = ((logits + noise) / tau).softmax(1)
    return p if keep_mask is None else p * keep_mask / keep_rate


def hyper_assign_served(logits, noise, keep_mask=None):
    """True where `hyper_assign` runs the kernels: device fp32 contiguous [n, H] operands of one shape, 1 <= H <= 8, the
    `HYPER` switch on."""
    return bool(HYPER and _hyper_table(logits) and _hyper_table(noise) and noise.shape == logits.shape and
                (keep_mask is None or (_hyper_table(keep_mask) and keep_mask.shape == logits.shape)))


class _HyperAssign(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, noise, keep, tau, keep_rate):
        n, H = logits.shape
        P = torch.empty_like(logits)
        p = None if keep is None else torch.empty_like(logits)       # with a mask P has lost p at the dropped entries
        _lib.check(_lib.load().mmrec_hyper_assign_fwd_f32(_p(logits), _p(noise), _p(keep), n, H, tau, keep_rate, _p(P), _p(p),
                                                          _stream()), "hyper_assign_fwd")
        ctx.tau, ctx.keep_rate, ctx.masked = tau, keep_rate, keep is not None
        ctx.save_for_backward(*((p, keep) if ctx.masked else (P,)))
        return P

    @staticmethod
    def backward(ctx, dP):
        if not ctx.needs_input_grad[0]:
            return None, None, None, None, None
        p, keep = ctx.saved_tensors if ctx.masked else (ctx.saved_tensors[0], None)
        n, H = p.shape
        da = torch.empty_like(p)
        _lib.check(_lib.load().mmrec_hyper_assign_bwd_f32(_p(p), _p(keep), _p(dP.contiguous()), n, H, ctx.tau, ctx.keep_rate,
                                                          _p(da), _stream()), "hyper_assign_bwd")
        return da, None, None, None, None


def hyper_assign(logits, noise, keep_mask=None, tau=1.0, keep_rate=1.0):
    """The hyperedge assignment of LGMRec (lgmrec.py:196-200 and the dropout of :208-209) -> P [n, H]:
    p = softmax((logits + noise) / tau) over a row, P = p * keep_mask / keep_rate (no mask: P = p).  `noise` is the caller's
    Gumbel draw and `keep_mask` its 0 / 1 dropout mask: nothing is drawn here.  Differentiable in `logits` only.
    Served by the kernels (`hyper_assign_served`): one launch forward, one backward, the row maximum subtracted as torch does.
    The state kept for the backward is p: without a mask that is the result itself; with a mask a second [n, H] tensor, because
    the dropped entries of P are zero while their logits still get a gradient.
    EVERY OTHER CASE (CPU tensors, H above 8, other dtypes, non-contiguous operands, the switch off) is `hyper_assign_torch`
    with stock autograd.  H = 64 (Clothing) has kernels of its own under `hyper64_assign`; 9 ... 63 have none."""
    if hyper_assign_served(logits, noise, keep_mask):
        return _HyperAssign.apply(logits, noise, keep_mask, float(tau), float(keep_rate))
    return hyper_assign_torch(logits, noise, keep_mask, tau, keep_rate)


def hyper_layer_torch(P_i, P_u, X):
    """lat = P_i^T X;  X_out = P_i lat;  U_out = P_u lat -> (U_out, X_out): HGNNLayer's three torch.mm in its order"""
    lat = torch.mm(P_i.T, X)
    X_out = torch.mm(P_i, lat)
    U_out = torch.mm(P_u, lat)
    return U_out, X_out


def hyper_layer_served(P_i, P_u, X):
    """True where `hyper_layer` runs the kernels: device fp32 contiguous P_i [I, H], P_u [U, H], X [I, 64] with 1 <= H <= 8
    and the `HYPER` switch on"""
    return bool(HYPER and _hyper_table(P_i) and _hyper_table(P_u) and _hyper_table(X, EMB_DIM) and P_i.shape[1] == P_u.shape[1]
                and P_i.shape[0] == X.shape[0])


class _HyperLayer(torch.autograd.Function):
    """forward(P_i, P_u or None where U_out is not wanted, X) -> (U_out or None, X_out)"""

    @staticmethod
    def forward(ctx, P_i, P_u, X):
        lib = _lib.load()
        (I, H), U = P_i.shape, 0 if P_u is None else P_u.shape[0]
        lat = torch.empty(H, EMB_DIM, dtype=torch.float32, device=X.device)
        X_out = torch.empty_like(X)
        U_out = None if P_u is None else torch.empty(U, EMB_DIM, dtype=torch.float32, device=X.device)
        ws = _ws(lib.mmrec_hyper_workspace_bytes(I, U, H), X.device)
        _lib.check(lib.mmrec_hyper_layer_fwd_f32(_p(P_i), _p(P_u), _p(X), I, U, H, EMB_DIM, _p(U_out), _p(X_out), _p(lat), _p(ws),
                                                 _stream()), "hyper_layer_fwd")
        ctx.has_u = P_u is not None
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(*((P_i, X, lat, P_u) if ctx.has_u else (P_i, X, lat)))
        return U_out, X_out

    @staticmethod
    def backward(ctx, dU, dX):
        P_i, X, lat = ctx.saved_tensors[:3]
        P_u = ctx.saved_tensors[3] if ctx.has_u else None
        want_pi, want_pu, want_x = ctx.needs_input_grad[0], ctx.has_u and ctx.needs_input_grad[1], ctx.needs_input_grad[2]
        if not (want_pi or want_pu or want_x):
            return None, None, None
        lib = _lib.load()
        (I, H), U = P_i.shape, 0 if P_u is None else P_u.shape[0]
        dU = None if (dU is None or P_u is None) else dU.contiguous()
        dX = None if dX is None else dX.contiguous()
        dP_i = torch.empty_like(P_i) if want_pi else None
        dP_u = torch.empty_like(P_u) if want_pu else None
        dX_prev = torch.empty_like(X) if want_x else None
        ws = _ws(lib.mmrec_hyper_workspace_bytes(I, U, H), X.device)
        _lib.check(lib.mmrec_hyper_layer_bwd_f32(_p(P_i), _p(P_u), _p(X), _p(lat), _p(dU), _p(dX), I, U, H, EMB_DIM, _p(dP_i),
                                                 _p(dP_u), _p(dX_prev), _p(ws), _stream()), "hyper_layer_bwd")
        return dP_i, dP_u, dX_prev


def hyper_layer(P_i, P_u, X):
    """One HGNN layer of LGMRec (lgmrec.py:23-36) -> (U_out [U, 64], X_out [I, 64]):
    lat = P_i^T X [H, 64];  X_out = P_i lat;  U_out = P_u lat, differentiable in all three operands.
    Served by the kernels (`hyper_layer_served`): three launches each way (reduce over blocks of `hyper_rows_per_block` rows,
    a finish that adds the blocks' partials in a fixed order, one row pass), X read once and each output written once, lat
    [H, 64] the only state besides the operands.  No atomics: the same bits every call, so `DETERMINISTIC` changes nothing.
    EVERY OTHER CASE (CPU tensors, H above 8, a width other than 64, other dtypes, non-contiguous operands, the switch off) is
    `hyper_layer_torch` with stock autograd.  H = 64 (Clothing) has kernels of its own under `hyper64_layer`; 9 ... 63 have none."""
    if hyper_layer_served(P_i, P_u, X):
        return _HyperLayer.apply(P_i, P_u, X)
    return hyper_layer_torch(P_i, P_u, X)


def hyper_propagate(P_i, P_u, E, n_layers):
    """`n_layers` HGNN layers from X_0 = E -> (U_L, X_L): HGNNLayer.forward.  Only the last layer's U is a result, so the
    served path asks the earlier layers for X alone (their user rows are neither computed nor written)."""
    if n_layers < 1:
        raise _lib.MMRecHipError("hyper_propagate: n_layers must be at least 1, got %r" % (n_layers,))
    if not hyper_layer_served(P_i, P_u, E):
        X = E
        for _ in range(n_layers):
            U_out, X = hyper_layer_torch(P_i, P_u, X)
        return U_out, X
    X = E
    for _ in range(n_layers - 1):
        _, X = _HyperLayer.apply(P_i, None, X)
    return _HyperLayer.apply(P_i, P_u, X)


# ------------------------------------------------------------------------------------------------
# ... at 64 hyperedges (csrc/hypergraph64.hip): Clothing's hyper_num, every product a [64 rows] x [64, 64] stage of csrc/tile64.h
# ------------------------------------------------------------------------------------------------
HYPER64_H = 64        # the one width this family serves; 9 ... 63 stay on the torch compositions (no shipped setting uses them)


def hyper64_rows_per_block(n):
    """rows of a side of n rows that one workgroup of the 64-hyperedge layer's reduction walks (the library's plan)"""
    return int(_lib.load().mmrec_hyper64_rows_per_block(int(n)))


def _hyper64_table(t):
    return _dev_table(t, HYPER64_H, 1 << 30)


def hyper64_assign_served(logits, noise, keep_mask=None):
    """True where `hyper64_assign` runs the kernels: device fp32 contiguous [n, 64] operands of one shape, the `HYPER` switch on"""
    return bool(HYPER and _hyper64_table(logits) and _hyper64_table(noise) and noise.shape == logits.shape and
                (keep_mask is None or (_hyper64_table(keep_mask) and keep_mask.shape == logits.shape)))


class _Hyper64Assign(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, noise, keep, tau, keep_rate):
        n = logits.shape[0]
        P = torch.empty_like(logits)
        p = None if keep is None else torch.empty_like(logits)       # with a mask P has lost p at the dropped entries
        _lib.check(_lib.load().mmrec_hyper64_assign_fwd_f32(_p(logits), _p(noise), _p(keep), n, tau, keep_rate, _p(P), _p(p),
                                                            _stream()), "hyper64_assign_fwd")
        ctx.tau, ctx.keep_rate, ctx.masked = tau, keep_rate, keep is not None
        ctx.save_for_backward(*((p, keep) if ctx.masked else (P,)))
        return P

    @staticmethod
    def backward(ctx, dP):
        if not ctx.needs_input_grad[0]:
            return None, None, None, None, None
        p, keep = ctx.saved_tensors if ctx.masked else (ctx.saved_tensors[0], None)
        da = torch.empty_like(p)
        _lib.check(_lib.load().mmrec_hyper64_assign_bwd_f32(_p(p), _p(keep), _p(dP.contiguous()), p.shape[0], ctx.tau,
                                                            ctx.keep_rate, _p(da), _stream()), "hyper64_assign_bwd")
        return da, None, None, None, None


def hyper64_assign(logits, noise, keep_mask=None, tau=1.0, keep_rate=1.0):
    """`hyper_assign` at 64 hyperedges -> P [n, 64]: p = softmax((logits + noise) / tau) over a row, P = p * keep_mask /
    keep_rate (no mask: P = p); nothing is drawn here; differentiable in `logits` only.
    Served by the kernels (`hyper64_assign_served`): one launch each way, 16 lanes per row, the row maximum subtracted.  The state
    kept for the backward is what `hyper_assign` keeps: P alone without a mask, p and the mask with one.
    EVERY OTHER CASE (CPU tensors, any other width, other dtypes, non-contiguous operands, the switch off) is
    `hyper_assign_torch` with stock autograd."""
    if hyper64_assign_served(logits, noise, keep_mask):
        return _Hyper64Assign.apply(logits, noise, keep_mask, float(tau), float(keep_rate))
    return hyper_assign_torch(logits, noise, keep_mask, tau, keep_rate)


def hyper64_layer_served(P_i, P_u, X):
    """True where `hyper64_layer` runs the kernels: device fp32 contiguous P_i [I, 64], P_u [U, 64], X [I, 64], the `HYPER`
    switch on"""
    return bool(HYPER and _hyper64_table(P_i) and _hyper64_table(P_u) and _dev_table(X, EMB_DIM, 1 << 30)
                and P_i.shape[0] == X.shape[0])


class _Hyper64Layer(torch.autograd.Function):
    """forward(P_i, P_u or None where U_out is not wanted, X) -> (U_out or None, X_out)"""

    @staticmethod
    def forward(ctx, P_i, P_u, X):
        lib = _lib.load()
        I, U = P_i.shape[0], 0 if P_u is None else P_u.shape[0]
        lat = torch.empty(HYPER64_H, EMB_DIM, dtype=torch.float32, device=X.device)
        X_out = torch.empty_like(X)
        U_out = None if P_u is None else torch.empty(U, EMB_DIM, dtype=torch.float32, device=X.device)
        ws = _ws(lib.mmrec_hyper64_workspace_bytes(I, U), X.device)
        _lib.check(lib.mmrec_hyper64_layer_fwd_f32(_p(P_i), _p(P_u), _p(X), I, U, _p(U_out), _p(X_out), _p(lat), _p(ws), _stream()),
                   "hyper64_layer_fwd")
        ctx.has_u = P_u is not None
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(*((P_i, X, lat, P_u) if ctx.has_u else (P_i, X, lat)))
        return U_out, X_out

    @staticmethod
    def backward(ctx, dU, dX):
        P_i, X, lat = ctx.saved_tensors[:3]
        P_u = ctx.saved_tensors[3] if ctx.has_u else None
        want_pi, want_pu, want_x = ctx.needs_input_grad[0], ctx.has_u and ctx.needs_input_grad[1], ctx.needs_input_grad[2]
        if not (want_pi or want_pu or want_x):
            return None, None, None
        lib = _lib.load()
        I, U = P_i.shape[0], 0 if P_u is None else P_u.shape[0]
        dU = None if (dU is None or P_u is None) else dU.contiguous()
        dX = None if dX is None else dX.contiguous()
        dP_i = torch.empty_like(P_i) if want_pi else None
        dP_u = torch.empty_like(P_u) if want_pu else None
        dX_prev = torch.empty_like(X) if want_x else None
        ws = _ws(lib.mmrec_hyper64_workspace_bytes(I, U), X.device)
        _lib.check(lib.mmrec_hyper64_layer_bwd_f32(_p(P_i), _p(P_u), _p(X), _p(lat), _p(dU), _p(dX), I, U, _p(dP_i), _p(dP_u),
                                                   _p(dX_prev), _p(ws), _stream()), "hyper64_layer_bwd")
        return dP_i, dP_u, dX_prev


def hyper64_layer(P_i, P_u, X):
    """`hyper_layer` at 64 hyperedges -> (U_out [U, 64], X_out [I, 64]): lat = P_i^T X [64, 64];  X_out = P_i lat;  U_out = P_u lat,
    differentiable in all three operands.
    Served by the kernels (`hyper64_layer_served`): three launches each way -- a reduce over blocks of `hyper64_rows_per_block`
    rows (one fma chain per block, in row order), a finish that adds the blocks' partials in a fixed order, one row pass over
    items and users with lat in LDS.  The state is what `hyper_layer` keeps: P_i, X, lat [64, 64] and P_u where it was given.  No
    atomics: the same bits every call.
    EVERY OTHER CASE (CPU tensors, any other width, other dtypes, non-contiguous operands, the switch off) is `hyper_layer_torch`
    with stock autograd."""
    if hyper64_layer_served(P_i, P_u, X):
        return _Hyper64Layer.apply(P_i, P_u, X)
    return hyper_layer_torch(P_i, P_u, X)


def hyper64_propagate(P_i, P_u, E, n_layers):
    """`hyper_propagate` at 64 hyperedges: `n_layers` HGNN layers from X_0 = E -> (U_L, X_L).  The served path asks the inner
    layers for X alone (their user rows are neither computed nor written)."""
    if n_layers < 1:
        raise _lib.MMRecHipError("hyper64_propagate: n_layers must be at least 1, got %r" % (n_layers,))
    if not hyper64_layer_served(P_i, P_u, E):
        X = E
        for _ in range(n_layers):
            U_out, X = hyper_layer_torch(P_i, P_u, X)
        return U_out, X
    X = E
    for _ in range(n_layers - 1):
        _, X = _Hyper64Layer.apply(P_i, None, X)
    return _Hyper64Layer.apply(P_i, P_u, X)


# ------------------------------------------------------------------------------------------------
# SMORE's spectrum step (csrc/spectrum.hip): rfft of two tables, three complex filters, three irfft
# ------------------------------------------------------------------------------------------------
SPECTRUM = True       # False: every spectrum_fusion call is `spectrum_fusion_torch` (A/B runs)
SPECTRUM_BINS = EMB_DIM // 2 + 1
_RDFT = {}            # (width, device) -> the four real DFT matrices of spectrum_fusion_torch


def spectrum_rows_per_block(n):
    """rows of a table of n rows that one workgroup of the spectrum kernels walks (the library's plan)"""
    return int(_lib.load().mmrec_spectrum_rows_per_block(int(n)))


def rdft_matrices(d, device):
    """rfft(x) = x @ C + i x @ S, irfft(Re, Im) = Re @ Ci + Im @ Si for norm='ortho', n = d (even);
    the DC / Nyquist imaginary parts do not contribute to the inverse, as in a C2R transform."""
    n = torch.arange(d, dtype=torch.float64).unsqueeze(1)
    k = torch.arange(d // 2 + 1, dtype=torch.float64).unsqueeze(0)
    ang = 2.0 * math.pi * n * k / d
    s = 1.0 / math.sqrt(d)
    wk = torch.full((d // 2 + 1, 1), 2.0, dtype=torch.float64)
    wk[0, 0] = wk[-1, 0] = 1.0
    Si = -wk * torch.sin(ang).t() * s
    Si[0, :] = 0.0
    Si[-1, :] = 0.0
    mats = (torch.cos(ang) * s, -torch.sin(ang) * s, wk * torch.cos(ang).t() * s, Si)
    return tuple(m.to(torch.float32).to(device) for m in mats)


def spectrum_fusion_torch(image, text, w_img, w_txt, w_fus):
    """SMORE.spectrum_convolution as a function of its five operands: the same operations in the same order.  The
    composition `spectrum_fusion` falls back to."""
    key = (image.shape[1], image.device)
    if key not in _RDFT:
        _RDFT[key] = rdft_matrices(*key)
    C, S, Ci, Si = _RDFT[key]
    ir, ii = image @ C, image @ S
    tr, ti = text @ C, text @ S

    def filt(re, im, w):
        wr, wi = w[0, :, 0], w[0, :, 1]
        return (re * wr - im * wi) @ Ci + (re * wi + im * wr) @ Si
    fr, fi = tr * ir - ti * ii, tr * ii + ti * ir
    return filt(ir, ii, w_img), filt(tr, ti, w_txt), filt(fr, fi, w_fus)


def spectrum_fusion_served(image, text, w_img, w_txt, w_fus):
    """True where `spectrum_fusion` runs the kernels: device fp32 contiguous [I, 64] tables of one shape, 1 <= I <= 2^30,
    device fp32 contiguous [1, 33, 2] weights, the `SPECTRUM` switch on."""
    return bool(SPECTRUM and _fuser_table(image) and _fuser_table(text) and image.shape == text.shape
                and image.device == text.device
                and all(_dev_tensor(w, (1, SPECTRUM_BINS, 2)) and w.device == image.device for w in (w_img, w_txt, w_fus)))


class _SpectrumFusion(torch.autograd.Function):
    @staticmethod
    def forward(ctx, image, text, w_img, w_txt, w_fus):
        n = image.shape[0]
        outs = tuple(torch.empty_like(image) for _ in range(3))
        _lib.check(_lib.load().mmrec_spectrum_fwd_f32(_p(image), _p(text), _p(w_img), _p(w_txt), _p(w_fus), n, EMB_DIM,
                                                      _p(outs[0]), _p(outs[1]), _p(outs[2]), _stream()), "spectrum_fwd")
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(image, text, w_img, w_txt, w_fus)      # the spectra are recomputed: nothing else is kept
        return outs

    @staticmethod
    def backward(ctx, g_img, g_txt, g_fus):
        image, text, w_img, w_txt, w_fus = ctx.saved_tensors
        want = ctx.needs_input_grad
        if not any(want) or (g_img is None and g_txt is None and g_fus is None):
            return None, None, None, None, None
        lib = _lib.load()
        n = image.shape[0]
        gs = [None if g is None else g.contiguous() for g in (g_img, g_txt, g_fus)]
        dx = torch.empty_like(image) if want[0] else None
        dy = torch.empty_like(text) if want[1] else None
        dws = [torch.empty_like(w) if want[2 + i] else None for i, w in enumerate((w_img, w_txt, w_fus))]
        ws = _ws(lib.mmrec_spectrum_workspace_bytes(n), image.device) if any(want[2:]) else None
        _lib.check(lib.mmrec_spectrum_bwd_f32(_p(image), _p(text), _p(w_img), _p(w_txt), _p(w_fus), _p(gs[0]), _p(gs[1]),
                                              _p(gs[2]), n, EMB_DIM, _p(dx), _p(dy), _p(dws[0]), _p(dws[1]), _p(dws[2]), _p(ws),
                                              _stream()), "spectrum_bwd")
        return dx, dy, dws[0], dws[1], dws[2]


def spectrum_fusion(image, text, w_img, w_txt, w_fus):
    """SMORE's spectrum step (smore.py:188-206) -> (image_conv, text_conv, fusion_conv), each [I, 64]:
    irfft(rfft(image) * w_img), irfft(rfft(text) * w_txt), irfft(rfft(text) * rfft(image) * w_fus) along dim 1 with
    norm='ortho', the weights [1, 33, 2] as (re, im) pairs.  Differentiable in all five operands.
    Served by the kernels (`spectrum_fusion_served`): one launch forward, two backward (the main pass and the finish that adds
    the blocks' weight-gradient partials in a fixed order); both tables read once, each output written once, the spectra kept
    in LDS and RECOMPUTED in the backward, so the state between the calls is the five operands.  An output that receives no
    gradient costs no transform; an operand that needs none is not computed.  No atomics: the same bits every call, so
    `DETERMINISTIC` changes nothing.  The imaginary weights of bins 0 and 32 are never read and get the gradient 0.0.
    EVERY OTHER CASE (CPU tensors, a width other than 64, other dtypes, non-contiguous operands, an empty table, the switch
    off) is `spectrum_fusion_torch` with stock autograd."""
    if spectrum_fusion_served(image, text, w_img, w_txt, w_fus):
        return _SpectrumFusion.apply(image, text, w_img, w_txt, w_fus)
    return spectrum_fusion_torch(image, text, w_img, w_txt, w_fus)


# ------------------------------------------------------------------------------------------------
# MGCN's behaviour-aware fuser (csrc/modal_fusion.hip): modality attention, two preference gates, the mix
# ------------------------------------------------------------------------------------------------
MODAL_FUSION = True   # False: every modal_fusion call is `modal_fusion_torch` (A/B runs)


def modal_fusion_rows_per_block(n):
    """rows of a table of n rows that one workgroup of the modal fusion kernels walks (the library's plan)"""
    return int(_lib.load().mmrec_modal_fusion_rows_per_block(int(n)))


def modal_fusion_torch(V, T, C, Wq, bq, q, Wv, bv, Wt, bt):
    """MGCN.forward's fuser (models/mgcn.py, the `fused_fusion` key off) as a function of its ten operands: the same operations
    in the same order -> (side, out).  The composition `modal_fusion` falls back to."""
    def query(x):
        return torch.nn.functional.linear(torch.tanh(linear(x.contiguous(), Wq, bq)), q)

    def gate(W, b):
        return torch.sigmoid(linear(C.contiguous(), W, b))
    w = torch.softmax(torch.cat([query(V), query(T)], dim=-1), dim=-1)
    common = w[:, 0].unsqueeze(1) * V + w[:, 1].unsqueeze(1) * T
    sep_image = gate(Wv, bv) * (V - common)
    sep_text = gate(Wt, bt) * (T - common)
    side = (sep_image + sep_text + common) / 3
    return side, C + side


def modal_fusion_served(V, T, C, Wq, bq, q, Wv, bv, Wt, bt):
    """True where `modal_fusion` runs the kernels: device fp32 contiguous [n, 64] tables of one shape, 1 <= n <= 2^30, device
    fp32 contiguous [64, 64] matrices, [64] biases and a [1, 64] q, the `MODAL_FUSION` switch on."""
    ok, table = _dev_tensor, _fuser_table
    if not (MODAL_FUSION and table(V) and table(T) and table(C) and V.shape == T.shape == C.shape):
        return False
    return bool(all(ok(w, (EMB_DIM, EMB_DIM)) for w in (Wq, Wv, Wt)) and all(ok(b, (EMB_DIM,)) for b in (bq, bv, bt)) and
                ok(q, (1, EMB_DIM)) and all(t.device == V.device for t in (T, C, Wq, bq, q, Wv, bv, Wt, bt)))


class _ModalFusion(torch.autograd.Function):
    @staticmethod
    def forward(ctx, *ops):
        V = ops[0]
        side, out = torch.empty_like(V), torch.empty_like(V)
        _lib.check(_lib.load().mmrec_modal_fusion_fwd_f32(*[_p(t) for t in ops], V.shape[0], EMB_DIM, _p(side), _p(out),
                                                          _stream()), "modal_fusion_fwd")
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(*ops)                                  # every intermediate is recomputed: nothing else is kept
        return side, out

    @staticmethod
    def backward(ctx, g_side, g_out):
        ops = ctx.saved_tensors
        want = ctx.needs_input_grad
        if not any(want) or (g_side is None and g_out is None):
            return (None,) * 10
        lib = _lib.load()
        n = ops[0].shape[0]
        gs = [None if g is None else g.contiguous() for g in (g_side, g_out)]
        grads = [torch.empty_like(t) if w else None for t, w in zip(ops, want)]
        ws = _ws(lib.mmrec_modal_fusion_workspace_bytes(n), ops[0].device) if any(want[3:]) else None
        _lib.check(lib.mmrec_modal_fusion_bwd_f32(*[_p(t) for t in ops], _p(gs[0]), _p(gs[1]), n, EMB_DIM,
                                                  *[_p(g) for g in grads], _p(ws), _stream()), "modal_fusion_bwd")
        return tuple(grads)


def modal_fusion(V, T, C, Wq, bq, q, Wv, bv, Wt, bt):
    """MGCN's behaviour-aware fuser (mgcn.py:188-203) -> (side, out), each [n, 64]:
    a = softmax(<tanh(V Wq^T + bq), q>, <tanh(T Wq^T + bq), q>), m = a_0 V + a_1 T, side = (sigmoid(C Wv^T + bv) (V - m) +
    sigmoid(C Wt^T + bt) (T - m) + m) / 3, out = C + side; V, T, C [n, 64] (image, text, content), the matrices [64, 64] as
    nn.Linear keeps them, q = query_common[2].weight [1, 64].  Differentiable in all ten operands.
    Served by the kernels (`modal_fusion_served`): one launch forward, two backward (the main pass and the finish that adds the
    blocks' weight-gradient partials in a fixed order); the three tables read once, the two outputs written once, every
    intermediate kept in LDS and RECOMPUTED in the backward, so the state between the calls is the ten operands.  An operand
    that needs no gradient is not computed.  No atomics: the same bits every call, so `DETERMINISTIC` changes nothing.
    EVERY OTHER CASE (CPU tensors, a width other than 64, other dtypes, non-contiguous operands, an empty table, the switch
    off) is `modal_fusion_torch` with stock autograd."""
    if modal_fusion_served(V, T, C, Wq, bq, q, Wv, bv, Wt, bt):
        return _ModalFusion.apply(V, T, C, Wq, bq, q, Wv, bv, Wt, bt)
    return modal_fusion_torch(V, T, C, Wq, bq, q, Wv, bv, Wt, bt)


# ------------------------------------------------------------------------------------------------
# MVGAE's posterior tail (csrc/posterior.hip): two products of experts, four reparametrisations, four KL terms, sigmoid(mu)
# ------------------------------------------------------------------------------------------------
POSTERIOR_FUSION = True   # False: every posterior_fusion call is `posterior_fusion_torch` (A/B runs)
POSTERIOR_MAX_LOGVAR = 10


def posterior_fusion_rows_per_block(n):
    """rows of a table of n rows that one workgroup of the posterior fusion kernels walks (the library's plan)"""
    return int(_lib.load().mmrec_posterior_fusion_rows_per_block(int(n)))


def posterior_fusion_torch(mu_v, lv_v, mu_t, lv_t, mu_c, lv_c, noise=None):
    """MVGAE.forward / calculate_loss's posterior tail (models/mvgae.py, the `fused_posterior` key off) as a function of the six
    encoder outputs and the four noise tables (pd, v, t, c; None: z = mu): the operations of `product_of_experts`, `reparametrize`
    and `kl_loss` in the model's order -> (Z [4, n, d], kl [4], score [n, d]).  The composition `posterior_fusion` falls back to."""
    def poe(mu, logvar, eps=1e-8):
        T = 1.0 / (torch.exp(logvar) + eps)
        pd_var = 1.0 / torch.sum(T, dim=0)
        return torch.sum(mu * T, dim=0) * pd_var, torch.log(pd_var)

    def reparametrize(mu, logvar, e):
        logvar = logvar.clamp(max=POSTERIOR_MAX_LOGVAR)
        return mu if e is None else mu + e * 0.1 * torch.exp(logvar.mul(0.5))

    def kl(mu, logvar):
        logvar = logvar.clamp(max=POSTERIOR_MAX_LOGVAR)
        return -0.5 * torch.mean(torch.sum(1 + logvar - mu ** 2 - logvar.exp(), dim=1))
    pd_mu, pd_lv = poe(torch.stack([mu_v, mu_t]), torch.stack([lv_v, lv_t]))
    pd_mu, pd_lv = poe(torch.stack([pd_mu, mu_c]), torch.stack([pd_lv, lv_c]))
    pairs = ((pd_mu, pd_lv), (mu_v, lv_v), (mu_t, lv_t), (mu_c, lv_c))
    es = (None,) * 4 if noise is None else noise
    Z = torch.stack([reparametrize(m, l, e) for (m, l), e in zip(pairs, es)])
    return Z, torch.stack([kl(m, l) for m, l in pairs]), torch.sigmoid(pd_mu).detach()


def posterior_fusion_served(mu_v, lv_v, mu_t, lv_t, mu_c, lv_c, noise=None):
    """True where `posterior_fusion` runs the kernels: six device fp32 contiguous [n, 64] tables of one shape on one device,
    1 <= n <= 2^30, the noise None or four more such tables, the `POSTERIOR_FUSION` switch on."""
    tabs = (mu_v, lv_v, mu_t, lv_t, mu_c, lv_c)
    if noise is not None:
        if not isinstance(noise, (tuple, list)) or len(noise) != 4:
            return False
        tabs = tabs + tuple(noise)
    if not (POSTERIOR_FUSION and all(_fuser_table(t) for t in tabs)):
        return False
    return bool(all(t.shape == mu_v.shape and t.device == mu_v.device for t in tabs))


class _PosteriorFusion(torch.autograd.Function):
    @staticmethod
    def forward(ctx, *ops):
        lib = _lib.load()
        mu_v = ops[0]
        n = mu_v.shape[0]
        Z = torch.empty((4,) + tuple(mu_v.shape), dtype=mu_v.dtype, device=mu_v.device)
        score = torch.empty_like(mu_v)
        kl = torch.empty(4, dtype=mu_v.dtype, device=mu_v.device)
        ptrs = [_p(t) for t in ops] + [None] * (10 - len(ops))
        ws = _ws(lib.mmrec_posterior_fusion_workspace_bytes(n), mu_v.device)
        _lib.check(lib.mmrec_posterior_fusion_fwd_f32(*ptrs, n, EMB_DIM, _p(Z), _p(score), _p(kl), _p(ws), _stream()),
                   "posterior_fusion_fwd")
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(*ops)                                  # every intermediate is recomputed: nothing else is kept
        ctx.mark_non_differentiable(score)
        return Z, kl, score

    @staticmethod
    def backward(ctx, gZ, g_kl, _g_score):
        ops = ctx.saved_tensors
        want = ctx.needs_input_grad[:6]
        if not any(want) or (gZ is None and g_kl is None):
            return (None,) * len(ops)
        n = ops[0].shape[0]
        gZ = None if gZ is None else gZ.contiguous()
        g_kl = None if g_kl is None else g_kl.contiguous()
        grads = [torch.empty_like(t) if w else None for t, w in zip(ops[:6], want)]
        ptrs = [_p(t) for t in ops] + [None] * (10 - len(ops))
        _lib.check(_lib.load().mmrec_posterior_fusion_bwd_f32(*ptrs, _p(gZ), _p(g_kl), n, EMB_DIM, *[_p(g) for g in grads],
                                                              _stream()), "posterior_fusion_bwd")
        return tuple(grads) + (None,) * (len(ops) - 6)


def posterior_fusion(mu_v, lv_v, mu_t, lv_t, mu_c, lv_c, noise=None):
    """MVGAE's posterior tail (mvgae.py, forward / calculate_loss) -> (Z [4, n, 64], kl [4], score [n, 64]):
    (m1, l1) = PoE(v, t), (mu_p, l_p) = PoE((m1, l1), c) with PoE's T = 1 / (exp(l) + 1e-8), var = 1 / sum T, m = var sum mu T,
    l = log var;  for k in (p, v, t, c): Z[k] = mu_k + 0.1 noise[k] exp(0.5 min(l_k, 10)) (noise None: Z[k] = mu_k),
    kl[k] = -0.5 mean_rows sum_cols (1 + lh_k - mu_k^2 - exp(lh_k));  score = sigmoid(mu_p), without a gradient.  Differentiable
    in the six encoder outputs; the noise gets none.
    Served by the kernels (`posterior_fusion_served`): two launches forward (the main pass and the finish that adds the blocks'
    KL partials in a fixed order), one backward; the ten tables read once, every output written once, every intermediate
    RECOMPUTED in the backward, so the state between the calls is the inputs.  An operand that needs no gradient is not
    computed.  No atomics: the same bits every call, so `DETERMINISTIC` changes nothing.  Supported domain: finite inputs with
    |log-variance| <= 30 (include/mmrec_hip.h).
    EVERY OTHER CASE (CPU tensors, a width other than 64, other dtypes, non-contiguous operands, an empty table, the switch
    off) is `posterior_fusion_torch` with stock autograd."""
    if posterior_fusion_served(mu_v, lv_v, mu_t, lv_t, mu_c, lv_c, noise):
        return _PosteriorFusion.apply(mu_v, lv_v, mu_t, lv_t, mu_c, lv_c, *(noise or ()))
    return posterior_fusion_torch(mu_v, lv_v, mu_t, lv_t, mu_c, lv_c, noise)


# ------------------------------------------------------------------------------------------------
# MVGAE's reconstruction term (csrc/hardest_neg.hip): every batch user against the hardest of the batch's negatives
# ------------------------------------------------------------------------------------------------
HARDEST_NEGATIVE = True   # False: every hardest_negative_loss call is `hardest_negative_loss_torch` (A/B runs)
HARDEST_NEGATIVE_L_MAX = 8
HARDEST_NEGATIVE_B_MAX = 65536


def hardest_negative_split_cols(B, L):
    """negative positions one workgroup of the sweep walks (the library's plan for the shape; 0 outside the served range)"""
    return int(_lib.load().mmrec_hardest_neg_split_cols(int(B), int(L)))


def hardest_negative_loss_torch(Z, users, pos, neg, squash=True, return_arg=False):
    """MVGAE.recon_loss (models/mvgae.py) line for line, for each of the L latents of Z [L, N, d] -> loss [L] (and arg [L, B]
    int32): S = sigmoid(Z[l]) or Z[l]; a = sigmoid(<S[users], S[pos]>); the [B, B] product of the batch's users against the
    batch's negatives by torch.mm, its row maximum with the argmax RESOLVED TO THE LOWEST POSITION that attains it (torch.max
    leaves the choice among ties open: the value is the same, the gradient goes to that one negative and the user, the rule
    the kernels state); -sum log2(sigmoid(a - sigmoid(h))).  Stock autograd.  The composition `hardest_negative_loss` falls
    back to; its temporaries are the squashed table and [B, B]."""
    losses, args = [], []
    for l in range(Z.shape[0]):
        z = torch.sigmoid(Z[l]) if squash else Z[l]
        zu = z[users]
        a = torch.sigmoid((zu * z[pos]).sum(dim=1))
        scores = torch.mm(zu, z[neg].t())
        with torch.no_grad():
            top = scores.max(dim=-1).values
            where = torch.arange(scores.shape[1], device=scores.device).expand_as(scores)
            arg = torch.where(scores == top.unsqueeze(1), where, torch.full_like(where, scores.shape[1])).min(dim=1).values
        hardest = scores.gather(1, arg.unsqueeze(1)).squeeze(1)
        losses.append(-torch.sum(torch.log2(torch.sigmoid(a - torch.sigmoid(hardest)))))
        args.append(arg.to(torch.int32))
    loss = torch.stack(losses)
    return (loss, torch.stack(args)) if return_arg else loss


def hardest_negative_loss_served(Z, users, pos, neg):
    """True where `hardest_negative_loss` runs the kernels: Z device fp32 contiguous [L, N, 64] with 1 <= L <= 8 and
    1 <= N <= 2^30, three device int64 contiguous 1-D id tensors of one length 1 <= B <= 65,536, the `HARDEST_NEGATIVE`
    switch on."""
    def ids(t):
        return bool(isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.int64 and t.dim() == 1 and t.is_contiguous())
    if not (HARDEST_NEGATIVE and isinstance(Z, torch.Tensor) and Z.is_cuda and Z.dtype == torch.float32 and Z.dim() == 3
            and Z.is_contiguous() and Z.shape[2] == EMB_DIM and 1 <= Z.shape[0] <= HARDEST_NEGATIVE_L_MAX
            and 1 <= Z.shape[1] <= 1 << 30):
        return False
    return bool(ids(users) and ids(pos) and ids(neg) and users.shape == pos.shape == neg.shape
                and 1 <= users.shape[0] <= HARDEST_NEGATIVE_B_MAX)


class _HardestNegative(torch.autograd.Function):
    @staticmethod
    def forward(ctx, Z, users, pos, neg, squash):
        lib = _lib.load()
        L, N, B = Z.shape[0], Z.shape[1], users.shape[0]
        loss = torch.empty(L, dtype=torch.float32, device=Z.device)
        arg = torch.empty(L, B, dtype=torch.int32, device=Z.device)
        coef = torch.empty(L, B, 2, dtype=torch.float32, device=Z.device)
        su = torch.empty(L, B, EMB_DIM, dtype=torch.float32, device=Z.device)       # the squashed user rows, for the backward
        ws = _ws(lib.mmrec_hardest_neg_workspace_bytes(B, L), Z.device)
        _lib.check(lib.mmrec_hardest_neg_fwd_f32(_p(Z), N, L, EMB_DIM, _p(users), _p(pos), _p(neg), B, int(squash), _p(loss),
                                                 _p(arg), _p(coef), _p(su), _p(ws), _stream()), "hardest_neg_fwd")
        ctx.squash = int(squash)
        ctx.set_materialize_grads(False)
        ctx.mark_non_differentiable(arg)
        ctx.save_for_backward(Z, users, pos, neg, arg, coef, su)
        return loss, arg

    @staticmethod
    def backward(ctx, g, _):
        if g is None or not ctx.needs_input_grad[0]:
            return None, None, None, None, None
        lib = _lib.load()
        Z, users, pos, neg, arg, coef, su = ctx.saved_tensors
        L, N, B = Z.shape[0], Z.shape[1], users.shape[0]
        g = g.contiguous()
        G = torch.empty(L, 3 * B, EMB_DIM, dtype=torch.float32, device=Z.device)
        _lib.check(lib.mmrec_hardest_neg_bwd_f32(_p(Z), N, L, EMB_DIM, _p(users), _p(pos), _p(neg), B, ctx.squash, _p(arg),
                                                 _p(coef), _p(su), _p(g), _p(G), _stream()), "hardest_neg_bwd")
        ids = torch.cat((users, pos, neg))
        order = torch.sort(ids, stable=True)[1]                        # one sort, shared by the L scatters
        dZ = torch.zeros_like(Z)
        for l in range(L):
            _lib.check(lib.mmrec_scatter_add_rows_sorted_f32(_p(order), _p(ids), _p(G[l]), 3 * B, EMB_DIM, _p(dZ[l]), _stream()),
                       "scatter_add_rows_sorted")
        return dZ, None, None, None, None


def hardest_negative_loss(Z, users, pos, neg, squash=True, return_arg=False):
    """MVGAE's reconstruction term (mvgae.py, recon_loss) for L latents over the same rows -> loss [L] (and, with `return_arg`,
    the detached arg [L, B] int32): with S = sigmoid(Z[l]) (`squash`) or Z[l], u_b = S[users[b]], p_b = S[pos[b]],
    n_j = S[neg[j]]:  a_b = sigmoid(<u_b, p_b>), h_b = max_j <u_b, n_j> over ALL B negatives of the batch, arg_b the LOWEST
    position that attains it, loss[l] = -sum_b log2(sigmoid(a_b - sigmoid(h_b))).  The ids are row ids into Z, used as given.
    Differentiable in Z only; through the maximum the gradient reaches n_arg_b and u_b only.
    Served by the kernels (`hardest_negative_loss_served`): three launches forward (the fp32-MFMA sweep of 128 users against
    64-negative tiles, both sides gathered and squashed on the way, a running (score, position) per lane; the terms with the
    positive dot products and the coefficients; the sum in a fixed tree), one backward that writes the gradients of the 3 B
    gathered rows, then one stable sort and L calls of the sorted row scatter into a zeroed dZ.  No squashed table, no
    gathered block, no [B, B] block; no float atomics: the same bits every call, so `DETERMINISTIC` changes nothing;
    capturable.
    EVERY OTHER CASE (CPU tensors, a width other than 64, other dtypes, non-contiguous operands, more than 8 latents, more
    than 65,536 samples, the switch off) is `hardest_negative_loss_torch` with stock autograd: the same rule."""
    if hardest_negative_loss_served(Z, users, pos, neg):
        loss, arg = _HardestNegative.apply(Z, users, pos, neg, bool(squash))
        return (loss, arg) if return_arg else loss
    return hardest_negative_loss_torch(Z, users, pos, neg, squash, return_arg)


# ------------------------------------------------------------------------------------------------
# DAMRS's symmetric KL term (csrc/mutual_kl.hip): mean over users x items of KL(p || q) + KL(q || p), no [users, items] block
# ------------------------------------------------------------------------------------------------
def mutual_kl_split_cols(m, n, mode=0):
    """rows of A and B one workgroup of the forward walks (the library's plan for the shape); mode 1: the same for the dU
    sweep, mode 2: the rows of U one workgroup of the dA / dB sweep walks"""
    return int(_lib.load().mmrec_mutual_kl_split_cols(int(m), int(n), int(mode)))


def _bernoulli_kl(p1, p2):
    """DAMRS._kl (models/damrs.py), term for term"""
    return p1 * torch.log(p1) - p1 * torch.log(p2) + (1 - p1) * torch.log(1 - p1) - (1 - p1) * torch.log(1 - p2)


def mutual_kl_torch(U, A, B):
    """exactly DAMRS's composition: p_g = sigmoid(U @ A.T), p_m = sigmoid(U @ B.T), mean(_kl(p_g, p_m) + _kl(p_m, p_g)); stock
    autograd, about twenty [m, n] blocks kept.  NaN (0 * log 0) once a logit saturates fp32's sigmoid, |logit| >~ 17."""
    p_g = torch.sigmoid(torch.mm(U, A.t()))
    p_m = torch.sigmoid(torch.mm(U, B.t()))
    return torch.mean(_bernoulli_kl(p_g, p_m) + _bernoulli_kl(p_m, p_g))


def mutual_kl_served(U, A, B):
    """True where `mutual_kl` runs the kernels: device fp32 contiguous U [m, 64], A [n, 64], B [n, 64] with m, n >= 1"""
    return bool(_fuser_table(U) and _fuser_table(A) and _fuser_table(B) and A.shape[0] == B.shape[0])


class _MutualKL(torch.autograd.Function):
    @staticmethod
    def forward(ctx, U, A, B):
        lib = _lib.load()
        m, n = U.shape[0], A.shape[0]
        scale = 1.0 / (float(m) * float(n))                  # in double on the host, rounded once to fp32 by the call
        out = torch.empty((), dtype=torch.float32, device=U.device)
        ws = _ws(lib.mmrec_mutual_kl_workspace_bytes(m, n, EMB_DIM), U.device)
        _lib.check(lib.mmrec_mutual_kl_f32(_p(U), _p(A), _p(B), m, n, EMB_DIM, scale, _p(out), _p(ws), _stream()), "mutual_kl")
        ctx.scale = scale
        ctx.save_for_backward(U, A, B)
        return out

    @staticmethod
    def backward(ctx, g):
        want = ctx.needs_input_grad[:3]
        if not any(want):
            return None, None, None
        lib = _lib.load()
        U, A, B = ctx.saved_tensors
        m, n = U.shape[0], A.shape[0]
        g = g.contiguous()
        dU, dA, dB = (torch.empty_like(t) if w else None for t, w in zip((U, A, B), want))
        ws = _ws(lib.mmrec_mutual_kl_workspace_bytes(m, n, EMB_DIM), U.device)
        _lib.check(lib.mmrec_mutual_kl_bwd_f32(_p(U), _p(A), _p(B), m, n, EMB_DIM, ctx.scale, _p(g), _p(dU), _p(dA), _p(dB),
                                               _p(ws), _stream()), "mutual_kl_bwd")
        return dU, dA, dB


def mutual_kl(U, A, B):
    """DAMRS's KL term -> the scalar mean over r < m, i < n of KL(p || q) + KL(q || p) of the Bernoulli pairs
    p = sigmoid(<U[r], A[i]>), q = sigmoid(<U[r], B[i]>), with autograd to all three operands, never holding an [m, n] block.
    The two divergences collapse: with a, b the two logits, KL(p || q) + KL(q || p) = (p - q)(a - b) =: J(a, b) -- no
    logarithm.  Served by the kernels (`mutual_kl_served`: device fp32 contiguous [m, 64], [n, 64], [n, 64], m, n >= 1): one
    fp32-MFMA sweep of 128 rows of U against 64-row tiles of A and B staged together plus a fixed-order finish; the backward
    recomputes the logits, one sweep for dU = Ga A + Gb B and one, owning the rows of A and B together, for dA = Ga^T U and
    dB = Gb^T U, a sweep whose gradients nobody wants skipped.  The scale 1 / (m n) is computed on the host in double.  No
    atomics: the same bits every call, so `DETERMINISTIC` changes nothing; the plan depends on (m, n) alone: capturable.
    SATURATION: the composition below returns NaN once a logit saturates fp32's sigmoid (|logit| >~ 17: 0 * log 0); J, and
    so the kernels, stay finite for any finite logits.  Below that the two agree within fp32 rounding.
    EVERY OTHER CASE (CPU tensors, a width other than 64, other dtypes, non-contiguous or empty operands) is exactly
    `mutual_kl_torch`, the model's composition with stock autograd."""
    if mutual_kl_served(U, A, B):
        return _MutualKL.apply(U, A, B)
    return mutual_kl_torch(U, A, B)


# ------------------------------------------------------------------------------------------------
# MVGAE's encoder heads (csrc/encoder_heads.hip): H normalised convolutions of one aggregated table, output and skip Linears
# ------------------------------------------------------------------------------------------------
ENCODER_HEADS = True   # False: every encoder_heads call is `encoder_heads_torch` (A/B runs)
ENCODER_HEADS_MAX = 4  # heads one call serves


def encoder_heads_rows_per_block(n):
    """rows of a table of n rows that one workgroup of the encoder heads kernels walks (the library's plan)"""
    return int(_lib.load().mmrec_encoder_heads_rows_per_block(int(n)))


def encoder_heads_torch(AX, X, W, b, G, bg, L, bl, scale=None, slope=0.01):
    """The end of MVGAE's GCN.forward (models/mvgae.py, the `fused_heads` key off) as a function of AX = spmm(graph, x), x and
    the stacked parameters of H heads, in stock torch -> out [H, n, d]: a = AX W_h + b_h, u = normalize(a), d = u scale_h,
    out_h = leaky(d) G_h^T + bg_h + leaky(X L_h^T + bl_h).  The composition `encoder_heads` falls back to."""
    fn = torch.nn.functional
    u = fn.normalize(torch.matmul(AX, W) + b.unsqueeze(1), p=2, dim=-1)
    hh = fn.leaky_relu(u if scale is None else u * scale, slope)
    p = torch.matmul(X, L.transpose(1, 2)) + bl.unsqueeze(1)
    return torch.matmul(hh, G.transpose(1, 2)) + bg.unsqueeze(1) + fn.leaky_relu(p, slope)


def encoder_heads_served(AX, X, W, b, G, bg, L, bl, scale=None, slope=0.01):
    """True where `encoder_heads` runs the kernels: device fp32 contiguous [n, 64] tables AX and X of one shape, 1 <= n <= 2^30,
    device fp32 contiguous [H, 64, 64] matrices and [H, 64] biases with H in 1 .. 4, `scale` None or such a [H, n, 64] tensor,
    all on one device, the `ENCODER_HEADS` switch on."""
    ok, table = _dev_tensor, _fuser_table
    if not (ENCODER_HEADS and table(AX) and table(X) and AX.shape == X.shape and isinstance(W, torch.Tensor) and W.dim() == 3):
        return False
    H, n = W.shape[0], AX.shape[0]
    if not 1 <= H <= ENCODER_HEADS_MAX:
        return False
    if scale is not None and not ok(scale, (H, n, EMB_DIM)):
        return False
    others = (X, W, b, G, bg, L, bl) + (() if scale is None else (scale,))
    return bool(all(ok(w, (H, EMB_DIM, EMB_DIM)) for w in (W, G, L)) and all(ok(v, (H, EMB_DIM)) for v in (b, bg, bl)) and
                all(t.device == AX.device for t in others))


class _EncoderHeads(torch.autograd.Function):
    @staticmethod
    def forward(ctx, AX, X, W, b, G, bg, L, bl, scale, slope):
        ops = (AX, X, W, b, G, bg, L, bl)
        n, H = AX.shape[0], W.shape[0]
        out = torch.empty((H, n, EMB_DIM), dtype=AX.dtype, device=AX.device)
        _lib.check(_lib.load().mmrec_encoder_heads_fwd_f32(*[_p(t) for t in ops], _p(scale), n, EMB_DIM, H, float(slope), _p(out),
                                                           _stream()), "encoder_heads_fwd")
        ctx.set_materialize_grads(False)
        ctx.slope = float(slope)
        ctx.save_for_backward(*ops, scale)                           # every intermediate is recomputed: nothing else is kept
        return out

    @staticmethod
    def backward(ctx, g):
        *ops, scale = ctx.saved_tensors
        want = ctx.needs_input_grad[:8]
        if not any(want) or g is None:
            return (None,) * 10
        lib = _lib.load()
        n, H = ops[0].shape[0], ops[2].shape[0]
        g = g.contiguous()
        grads = [torch.empty_like(t) if w else None for t, w in zip(ops, want)]
        ws = _ws(lib.mmrec_encoder_heads_workspace_bytes(n, H), ops[0].device) if any(want[2:]) else None
        _lib.check(lib.mmrec_encoder_heads_bwd_f32(*[_p(t) for t in ops], _p(scale), _p(g), n, EMB_DIM, H, ctx.slope,
                                                   *[_p(t) for t in grads], _p(ws), _stream()), "encoder_heads_bwd")
        return tuple(grads) + (None, None)


def encoder_heads(AX, X, W, b, G, bg, L, bl, scale=None, slope=0.01):
    """MVGAE's encoder heads (mvgae.py, the end of GCN.forward) -> out [H, n, 64], one table per head (mean, log-variance):
    a = AX W_h + b_h, u = a / max(||a||, 1e-12), d = u scale_h, out_h = leaky(d) G_h^T + bg_h + leaky(X L_h^T + bl_h);  AX =
    spmm(graph, x) and X = x [n, 64]; W [H, 64, 64] the stacked BaseModel.weight ([in][out]), G and L [H, 64, 64] the stacked
    g_layer and linear_layer weights as nn.Linear keeps them, b, bg, bl [H, 64]; `scale` [H, n, 64] the dropout masks already
    divided by the keep rate (None: no dropout).  Differentiable in the first eight operands; `scale` gets no gradient.
    Served by the kernels (`encoder_heads_served`): one launch forward, two backward (the main pass and the finish that adds the
    blocks' weight-gradient partials in a fixed order); the heads are walked one after another inside each workgroup, every
    intermediate kept in LDS and RECOMPUTED in the backward, so the state between the calls is the operands and `scale`.  An
    operand that needs no gradient is not computed.  No atomics: the same bits every call, so `DETERMINISTIC` changes nothing.
    EVERY OTHER CASE (CPU tensors, a width other than 64, other dtypes, non-contiguous operands, an empty table, more than four
    heads, the switch off) is `encoder_heads_torch` with stock autograd."""
    if encoder_heads_served(AX, X, W, b, G, bg, L, bl, scale, slope):
        return _EncoderHeads.apply(AX, X, W, b, G, bg, L, bl, scale, slope)
    return encoder_heads_torch(AX, X, W, b, G, bg, L, bl, scale, slope)


# ------------------------------------------------------------------------------------------------
# MMGCN's 64-wide layer (csrc/gcn_layer.hip): convolution, skip Linear + id embedding and the 128 -> 64 Linear over their cat
# ------------------------------------------------------------------------------------------------
GCN_LAYER = True   # False: every gcn_layer call is `gcn_layer_torch` (A/B runs)


def gcn_layer_rows_per_block(n):
    """rows of a table of n rows that one workgroup of the GCN layer kernels walks (the library's plan)"""
    return int(_lib.load().mmrec_gcn_layer_rows_per_block(int(n)))


def gcn_layer_torch(AX, X, R, Wc, Wl, bl, Wg, bg, slope=0.01):
    """One layer of MMGCN's GCN.forward (models/mmgcn.py, the `fused_layers` key off) as a function of AX = spmm(graph, x), x,
    the id embedding R (or None) and the layer's parameters, in stock torch -> [n, d]: h = leaky(AX Wc), xh = leaky(X Wl^T + bl)
    + R, out = leaky(cat(h, xh) Wg^T + bg).  The composition `gcn_layer` falls back to."""
    fn = torch.nn.functional
    h = fn.leaky_relu(torch.matmul(AX, Wc), slope)
    xh = fn.leaky_relu(fn.linear(X, Wl, bl), slope)
    if R is not None:
        xh = xh + R
    return fn.leaky_relu(fn.linear(torch.cat((h, xh), dim=1), Wg, bg), slope)


def gcn_layer_served(AX, X, R, Wc, Wl, bl, Wg, bg, slope=0.01):
    """True where `gcn_layer` runs the kernels: device fp32 contiguous [n, 64] tables AX, X and R (or R None) of one shape,
    1 <= n <= 2^30, device fp32 contiguous Wc, Wl [64, 64], Wg [64, 128] and bl, bg [64], all on one device, slope > 0, the
    `GCN_LAYER` switch on."""
    def ok(t, shape):
        return _dev_tensor(t, shape) and t.device == AX.device
    table = _fuser_table
    if not (GCN_LAYER and table(AX) and table(X) and AX.shape == X.shape and float(slope) > 0.0):
        return False
    if X.device != AX.device or (R is not None and not ok(R, tuple(AX.shape))):
        return False
    return bool(ok(Wc, (EMB_DIM, EMB_DIM)) and ok(Wl, (EMB_DIM, EMB_DIM)) and ok(Wg, (EMB_DIM, 2 * EMB_DIM)) and
                ok(bl, (EMB_DIM,)) and ok(bg, (EMB_DIM,)))


class _GcnLayer(torch.autograd.Function):
    @staticmethod
    def forward(ctx, AX, X, R, Wc, Wl, bl, Wg, bg, slope):
        ops = (AX, X, R, Wc, Wl, bl, Wg, bg)
        n = AX.shape[0]
        out = torch.empty((n, EMB_DIM), dtype=AX.dtype, device=AX.device)
        _lib.check(_lib.load().mmrec_gcn_layer_fwd_f32(*[_p(t) for t in ops], n, EMB_DIM, float(slope), _p(out), _stream()),
                   "gcn_layer_fwd")
        ctx.set_materialize_grads(False)
        ctx.slope = float(slope)
        ctx.save_for_backward(*ops, out)                             # a, h, p, xh are recomputed; q's sign is out's
        return out

    @staticmethod
    def backward(ctx, g):
        *ops, out = ctx.saved_tensors
        want = ctx.needs_input_grad[:8]
        if not any(want) or g is None:
            return (None,) * 9
        lib = _lib.load()
        n = ops[0].shape[0]
        g = g.contiguous()
        grads = [torch.empty_like(t) if w and t is not None else None for t, w in zip(ops, want)]
        ws = _ws(lib.mmrec_gcn_layer_workspace_bytes(n), ops[0].device) if any(x is not None for x in grads[3:]) else None
        _lib.check(lib.mmrec_gcn_layer_bwd_f32(*[_p(t) for t in ops], _p(out), _p(g), n, EMB_DIM, ctx.slope,
                                               *[_p(t) for t in grads], _p(ws), _stream()), "gcn_layer_bwd")
        return tuple(grads) + (None,)


def gcn_layer(AX, X, R, Wc, Wl, bl, Wg, bg, slope=0.01):
    """One 64-wide layer of MMGCN's GCN.forward (mmgcn.py) -> [n, 64]: h = leaky(AX Wc), xh = leaky(X Wl^T + bl) + R,
    out = leaky(h Gh^T + xh Gx^T + bg) with Wg = [Gh | Gx];  AX = spmm(graph, x) and X = x [n, 64]; R [n, 64] the id embedding
    (None: zeros); Wc [64, 64] the BaseModel.weight ([in][out]), Wl [64, 64] and Wg [64, 128] the linear_layer and g_layer
    weights as nn.Linear keeps them, bl, bg [64].  Differentiable in all eight operands.
    Served by the kernels (`gcn_layer_served`): one launch forward, two backward (the main pass and the finish that adds the
    blocks' weight-gradient partials in a fixed order); every intermediate is kept in LDS and RECOMPUTED in the backward, so the
    state between the calls is the operands and the result.  An operand that needs no gradient is not computed.  No atomics: the
    same bits every call, so `DETERMINISTIC` changes nothing.
    EVERY OTHER CASE (CPU tensors, a width other than 64, other dtypes, non-contiguous operands, an empty table, a slope that
    is not positive, the switch off) is `gcn_layer_torch` with stock autograd."""
    if gcn_layer_served(AX, X, R, Wc, Wl, bl, Wg, bg, slope):
        return _GcnLayer.apply(AX, X, R, Wc, Wl, bl, Wg, bg, slope)
    return gcn_layer_torch(AX, X, R, Wc, Wl, bl, Wg, bg, slope)


# ------------------------------------------------------------------------------------------------
# Rows next to the hot path: device negative sampler, device ranking metrics
# ------------------------------------------------------------------------------------------------
def flat_to_csr(flat, lens, device):
    """row lists given as one concatenated id array + per-row lengths -> (rowptr int32, ids int32 sorted inside each row)
    on `device`; one global sort of (row, id) keys instead of a Python loop over the rows (1M evaluation users: 0.5 s)."""
    lens = np.asarray(lens, dtype=np.int64)
    flat = np.asarray(flat, dtype=np.int64)
    rowptr = np.zeros(lens.shape[0] + 1, dtype=np.int64)
    np.cumsum(lens, out=rowptr[1:])
    if flat.size:
        stride = np.int64(flat.max()) + 1
        key = np.repeat(np.arange(lens.shape[0], dtype=np.int64), lens) * stride + flat
        key.sort()
        flat = key % stride
    else:
        flat = np.zeros(1, np.int64)
    return (torch.from_numpy(rowptr.astype(np.int32)).to(device),
            torch.from_numpy(flat.astype(np.int32)).to(device))


def lists_to_csr(lists, device):
    """list of per-row id arrays -> (rowptr int32, ids int32 sorted inside each row) on `device`."""
    lens = np.fromiter((len(x) for x in lists), dtype=np.int64, count=len(lists))
    flat = np.concatenate([np.asarray(x, dtype=np.int64) for x in lists]) if len(lists) else np.zeros(0, np.int64)
    return flat_to_csr(flat, lens, device)


def sample_negatives(users, hist_rowptr, hist_col, cand_items, seed, counter):
    """One uniform negative per user id from `cand_items`, outside the user's history (f1)."""
    lib = _lib.load()
    _chk(users, torch.int64, "users", 1), _chk(hist_rowptr, torch.int32, "hist_rowptr", 1)
    _chk(hist_col, torch.int32, "hist_col", 1), _chk(cand_items, torch.int32, "cand_items", 1)
    out = torch.empty_like(users)
    _lib.check(lib.mmrec_sample_negatives_i64(_p(users), users.numel(), _p(hist_rowptr), _p(hist_col),
                                              _p(cand_items), cand_items.numel(), int(seed) & (2 ** 64 - 1),
                                              int(counter) & (2 ** 64 - 1), _p(out), _stream()),
               "sample_negatives")
    return out


def topk_metrics_per_user(topk_idx, gt_rowptr, gt_col, ks, want_hits=False):
    """Per-user Recall/NDCG/Precision/MAP at cut-offs `ks` -> float64 [n_users, 4, len(ks)] (f2)."""
    lib = _lib.load()
    topk_idx = _chk(topk_idx.contiguous(), torch.int64, "topk_idx", 2)
    _chk(gt_rowptr, torch.int32, "gt_rowptr", 1), _chk(gt_col, torch.int32, "gt_col", 1)
    n, k = topk_idx.shape
    dev = topk_idx.device
    ks = sorted(int(x) for x in ks)
    if ks[-1] > k or ks[0] < 1:
        raise _lib.MMRecHipError("cut-offs must lie in [1, k]")
    disc = 1.0 / np.log2(np.arange(1, k + 1, dtype=np.float64) + 1)
    d_disc = torch.from_numpy(disc).to(dev)
    d_idcg = torch.from_numpy(np.cumsum(disc)).to(dev)
    d_ks = torch.tensor(ks, dtype=torch.int32, device=dev)
    out = torch.empty(n, 4, len(ks), dtype=torch.float64, device=dev)
    hits = torch.empty(n, k, dtype=torch.uint8, device=dev) if want_hits else None
    _lib.check(lib.mmrec_topk_metrics_f64(_p(topk_idx), n, k, _p(gt_rowptr), _p(gt_col), _p(d_disc),
                                          _p(d_idcg), _p(d_ks), len(ks), _p(hits), _p(out), _stream()),
               "topk_metrics")
    return (out, hits) if want_hits else out
