// Max over a node's neighbours, with the argmax, and its backward (include/mmrec_hip.h, additive to ABI 16): PyG's
// `aggr='max'` of Base_gcn (dualgnn.py:318-345, dragon.py:387-410) without the gathered [n_edges, 64] message tensor.
// For row r of a CSR (rowptr, colidx), slot j at position p = perm ? perm[j] : j of the caller's (COO) edge list:
//     Y[r][c] = max over the row's slots j of X[colidx[j]][c]          arg[r][c] = the position p of the slot chosen
// THE SELECTION RULE, per (row, column), is part of the contract: the chosen slot is the first in CSR order whose value is
// NaN; without a NaN, the first in CSR order that attains the maximum under IEEE `>` (-0 and +0 are tied: the first wins).
// Y holds the chosen value's bits: the forward is exact.  A row without (present) entries: Y = 0, arg = -1 (PyG's
// semantics for a node without messages).
//
// The access shape is edge_attention.hip's: one 16-lane group owns a row, lane t holds the float4 of columns 4 t ... 4 t + 3
// of the running maximum and the int4 of the CSR slots that gave them; lane t loads the column id of slot base + t (one step
// ahead of its use), the ids go round the group by shuffle and NMAX_NB gathers are in flight per step (NMAX_NB_BLOCK in the
// workgroup of a listed row).  Every lane sees every entry of its span in CSR order, so inside a group "first" needs no
// exchange: an entry replaces the state only if it is NaN where the state is not, or strictly greater (nmax_take).
//   group  four rows per wave, 16 per workgroup; rows of at most rg::GROUP_MAX entries, or every row when no list is given.
//   block  one 256-thread workgroup per LISTED row (the list of mmrec_spmm_plan_fill at rg::GROUP_MAX, row_groups.h's one
//          threshold: the list a DynGraph caches serves every op): group g takes the slots 16 g ... 16 g + 15 of every 256;
//          the 16 (value, slot) states go through LDS and the first wave, one column per lane, combines them by (is NaN,
//          value, CSR slot) -- nmax_better -- so the result is the rule above and not "whichever group held it".
// A colidx outside [0, n_x) or a position outside [0, n_edges) is an absent edge: never an address, never chosen.  EVERY
// row of Y and of arg is written.  No atomics: the bits are a function of the inputs alone (not even of the launch shape).
//
// Backward (mmrec_neighbor_max_bwd_f32): dX[s][c] = base[s][c] + sum of dY[r][c] over the slots jt of COLUMN s in the
// transposed CSR (rowptr_t, rowidx_t, perm_t) with arg[r][c] == p, r = rowidx_t[jt], p = perm_t ? perm_t[jt] : jt.  A PULL:
// every dX row has one owner that walks its column, gathers arg[r] next to dY[r] (256 bytes each) and adds where the
// position matches -- no atomics, a fixed order (slots ascending in a group; a listed column's 16 partial sums in the order
// g = 0 ... 15 after the base), every row of dX written.  The comparison is on POSITIONS, so of duplicate (r, s) edges only
// the chosen copy contributes.  A row id outside [0, n_rows) or a position outside [0, n_edges) is an absent edge.  A term
// that does not match is not added (not "added as 0"): a NaN in dY[r][c] reaches the one dX element its arg names.
// Known and accepted, as in edge_attention.hip: a hub of tens of thousands of edges is ONE workgroup in each direction.
#include "row_groups.h"

namespace {

using rg::slot_pos;

constexpr int NMAX_NB = 4;                       // gathers in flight per group and step
constexpr int NMAX_NB_BLOCK = 16;                // ... in the workgroup that owns a listed row: its latency is the call's tail
constexpr int NMAX_NB_BLOCK_BWD = 8;             // ... of (arg, dY) row pairs in the backward's

struct MaxState {
    float4 v;                                    // the chosen values
    int4 s;                                      // their CSR slots, -1: nothing yet
};

// An entry x of slot j that comes AFTER everything in (b, bs) in CSR order: it wins only if nothing was there, or if the
// state is not NaN and x is NaN or strictly greater (!(x <= b) is both; -0 <= +0 and +0 <= -0: a tie keeps the first).
__device__ __forceinline__ void nmax_take(float x, int j, float& b, int& bs) {
    if (bs < 0 || (b == b && !(x <= b))) {
        b = x;
        bs = j;
    }
}

// (x, xs) before (b, bs) under the rule, for states met in ANY order: present beats absent; among NaNs, and among equal
// values, the lower CSR slot; a NaN beats every number; otherwise the greater value.
__device__ __forceinline__ bool nmax_better(float x, int xs, float b, int bs) {
    if (xs < 0) return false;
    if (bs < 0) return true;
    const bool xn = x != x, bn = b != b;
    if (xn || bn) return (xn && bn) ? xs < bs : xn;
    return x > b || (x == b && xs < bs);
}

// the column id of slot j, -1 for a slot beyond the row or an absent edge
__device__ __forceinline__ int nmax_col(int j, int end, const int32_t* __restrict__ colidx, const int64_t* __restrict__ perm,
                                        int n_edges, int n_x) {
    if (j < 0 || j >= end) return -1;                           // (j < 0: base + stride + t beyond int)
    const int c = colidx[j];
    return (c < 0 || c >= n_x || slot_pos(perm, j, n_edges) < 0) ? -1 : c;
}

// The slots first ... first + 15, first + stride ..., below end, of one row for one 16-lane group, in CSR order, NB gathers in
// flight; the ids of the next step are loaded before this step's rows are waited for.
template <int NB>
__device__ __forceinline__ void max_span(int first, int end, int stride, int t, const int32_t* __restrict__ colidx,
                                         const int64_t* __restrict__ perm, int n_edges, const float4* __restrict__ X4, int n_x,
                                         MaxState& st) {
    int c = first < end ? nmax_col(first + t, end, colidx, perm, n_edges, n_x) : -1;
    for (int base = first; base < end; base += stride) {
        const int c_next = end - base > stride ? nmax_col(base + stride + t, end, colidx, perm, n_edges, n_x) : -1;
        const int cnt = min(rg::LANES, end - base);
        for (int k0 = 0; k0 < cnt; k0 += NB) {
            float4 x[NB];
            int cs[NB];
#pragma unroll
            for (int u = 0; u < NB; ++u) {
                cs[u] = __shfl(c, k0 + u, rg::LANES);          // (-1 beyond cnt: those lanes hold -1)
                x[u] = cs[u] >= 0 ? X4[(size_t)cs[u] * rg::LANES + t] : f4_zero();
            }
#pragma unroll
            for (int u = 0; u < NB; ++u) {
                if (cs[u] < 0) continue;
                const int jj = base + k0 + u;
                nmax_take(x[u].x, jj, st.v.x, st.s.x);
                nmax_take(x[u].y, jj, st.v.y, st.s.y);
                nmax_take(x[u].z, jj, st.v.z, st.s.z);
                nmax_take(x[u].w, jj, st.v.w, st.s.w);
            }
        }
        c = c_next;
        if (end - base <= stride) break;                        // (base + stride may not be representable)
    }
}

// the chosen slot's position in the caller's order (-1: none; a chosen slot's position was checked when it was admitted)
__device__ __forceinline__ int nmax_arg(const int64_t* __restrict__ perm, int slot) {
    return (slot < 0 || !perm) ? slot : (int)perm[slot];
}

__global__ __launch_bounds__(rg::BLOCK) void neighbor_max_group_kernel(
    const int32_t* __restrict__ rowptr, int n_rows, const int32_t* __restrict__ colidx, const int64_t* __restrict__ perm,
    bool skip_long, const float4* __restrict__ X4, int n_x, int n_edges, float4* __restrict__ Y4, int4* __restrict__ arg4) {
    // (the loops of this file are written out, not rg::for_short_rows: row_groups.h says why)
    const int t = threadIdx.x % rg::LANES;
    const int stride = gridDim.x * rg::GROUPS;
    for (long r = (long)blockIdx.x * rg::GROUPS + threadIdx.x / rg::LANES; r < n_rows; r += stride) {
        int start, end;
        rg::row_span(rowptr, (int)r, n_edges, start, end);
        if (skip_long && end - start > rg::GROUP_MAX) continue;           // the block kernel's
        MaxState st{f4_zero(), make_int4(-1, -1, -1, -1)};
        if (end > start) max_span<NMAX_NB>(start, end, rg::LANES, t, colidx, perm, n_edges, X4, n_x, st);
        Y4[(size_t)r * rg::LANES + t] = st.v;                             // (zeros where nothing was chosen)
        arg4[(size_t)r * rg::LANES + t] =
            make_int4(nmax_arg(perm, st.s.x), nmax_arg(perm, st.s.y), nmax_arg(perm, st.s.z), nmax_arg(perm, st.s.w));
    }
}

__global__ __launch_bounds__(rg::BLOCK) void neighbor_max_block_kernel(
    const int32_t* __restrict__ rowptr, int n_rows, const int32_t* __restrict__ colidx, const int64_t* __restrict__ perm,
    const int32_t* __restrict__ long_rows, const float4* __restrict__ X4, int n_x, int n_edges, float* __restrict__ Y,
    int32_t* __restrict__ arg) {
    __shared__ float4 s_v[rg::GROUPS][rg::LANES];
    __shared__ int4 s_s[rg::GROUPS][rg::LANES];
    const int r = long_rows[blockIdx.x];
    if (r < 0 || r >= n_rows) return;                                      // (the whole workgroup)
    int start, end;
    rg::row_span(rowptr, r, n_edges, start, end);
    const int t = threadIdx.x % rg::LANES, g = threadIdx.x / rg::LANES;
    MaxState st{f4_zero(), make_int4(-1, -1, -1, -1)};
    max_span<NMAX_NB_BLOCK>(start + g * rg::LANES, end, rg::BLOCK, t, colidx, perm, n_edges, X4, n_x, st);
    s_v[g][t] = st.v;
    s_s[g][t] = st.s;
    __syncthreads();
    if (threadIdx.x < 4 * rg::LANES) {                                    // the first wave: one column of the row per lane
        const float* cv = reinterpret_cast<const float*>(&s_v[0][0]) + threadIdx.x;
        const int* cs = reinterpret_cast<const int*>(&s_s[0][0]) + threadIdx.x;
        float b = 0.f;
        int bs = -1;
#pragma unroll
        for (int k = 0; k < rg::GROUPS; ++k) {
            const float x = cv[k * 4 * rg::LANES];
            const int xs = cs[k * 4 * rg::LANES];
            if (nmax_better(x, xs, b, bs)) {
                b = x;
                bs = xs;
            }
        }
        Y[(size_t)r * (4 * rg::LANES) + threadIdx.x] = b;
        arg[(size_t)r * (4 * rg::LANES) + threadIdx.x] = nmax_arg(perm, bs);
    }
}

// ------------------------------------------------------------------------------------------------ backward
// the row id and the position of transposed slot j; r = -1 for a slot beyond the column or an absent edge
__device__ __forceinline__ void nmax_row(int j, int end, const int32_t* __restrict__ rowidx_t, const int64_t* __restrict__ perm_t,
                                         int n_edges, int n_rows, int& r, int& p) {
    r = p = -1;
    if (j < 0 || j >= end) return;                              // (j < 0: base + stride + t beyond int)
    r = rowidx_t[j];
    p = slot_pos(perm_t, j, n_edges);
    if (r < 0 || r >= n_rows || p < 0) r = -1;
}

// The slots of one column for one 16-lane group: acc[c] += dY[r][c] where arg[r][c] is this slot's position.
template <int NB>
__device__ __forceinline__ void max_bwd_span(int first, int end, int stride, int t, const int32_t* __restrict__ rowidx_t,
                                             const int64_t* __restrict__ perm_t, int n_edges, int n_rows,
                                             const int4* __restrict__ arg4, const float4* __restrict__ dY4, float4& acc) {
    int r = -1, p = -1;
    if (first < end) nmax_row(first + t, end, rowidx_t, perm_t, n_edges, n_rows, r, p);
    for (int base = first; base < end; base += stride) {
        int r_next = -1, p_next = -1;
        if (end - base > stride) nmax_row(base + stride + t, end, rowidx_t, perm_t, n_edges, n_rows, r_next, p_next);
        const int cnt = min(rg::LANES, end - base);
        for (int k0 = 0; k0 < cnt; k0 += NB) {
            float4 gd[NB];
            int4 a[NB];
            int rs[NB], ps[NB];
#pragma unroll
            for (int u = 0; u < NB; ++u) {
                rs[u] = __shfl(r, k0 + u, rg::LANES);
                ps[u] = __shfl(p, k0 + u, rg::LANES);
                a[u] = rs[u] >= 0 ? arg4[(size_t)rs[u] * rg::LANES + t] : make_int4(-1, -1, -1, -1);
                gd[u] = rs[u] >= 0 ? dY4[(size_t)rs[u] * rg::LANES + t] : f4_zero();
            }
#pragma unroll
            for (int u = 0; u < NB; ++u) {
                if (rs[u] < 0) continue;
                if (a[u].x == ps[u]) acc.x += gd[u].x;
                if (a[u].y == ps[u]) acc.y += gd[u].y;
                if (a[u].z == ps[u]) acc.z += gd[u].z;
                if (a[u].w == ps[u]) acc.w += gd[u].w;
            }
        }
        r = r_next;
        p = p_next;
        if (end - base <= stride) break;                        // (base + stride may not be representable)
    }
}

__global__ __launch_bounds__(rg::BLOCK) void neighbor_max_bwd_group_kernel(
    const int32_t* __restrict__ rowptr_t, int n_cols, const int32_t* __restrict__ rowidx_t, const int64_t* __restrict__ perm_t,
    bool skip_long, int n_rows, int n_edges, const int4* __restrict__ arg4, const float4* __restrict__ dY4,
    const float4* __restrict__ base4, float4* __restrict__ dX4) {
    const int t = threadIdx.x % rg::LANES;
    const int stride = gridDim.x * rg::GROUPS;
    for (long c = (long)blockIdx.x * rg::GROUPS + threadIdx.x / rg::LANES; c < n_cols; c += stride) {
        int start, end;
        rg::row_span(rowptr_t, (int)c, n_edges, start, end);
        if (skip_long && end - start > rg::GROUP_MAX) continue;           // the block kernel's
        float4 acc = base4 ? base4[(size_t)c * rg::LANES + t] : f4_zero();
        if (end > start) max_bwd_span<NMAX_NB>(start, end, rg::LANES, t, rowidx_t, perm_t, n_edges, n_rows, arg4, dY4, acc);
        dX4[(size_t)c * rg::LANES + t] = acc;
    }
}

__global__ __launch_bounds__(rg::BLOCK) void neighbor_max_bwd_block_kernel(
    const int32_t* __restrict__ rowptr_t, int n_cols, const int32_t* __restrict__ rowidx_t, const int64_t* __restrict__ perm_t,
    const int32_t* __restrict__ long_cols, int n_rows, int n_edges, const int4* __restrict__ arg4,
    const float4* __restrict__ dY4, const float* __restrict__ base, float* __restrict__ dX) {
    __shared__ float4 s_acc[rg::GROUPS][rg::LANES];
    const int c = long_cols[blockIdx.x];
    if (c < 0 || c >= n_cols) return;                                      // (the whole workgroup)
    int start, end;
    rg::row_span(rowptr_t, c, n_edges, start, end);
    const int t = threadIdx.x % rg::LANES, g = threadIdx.x / rg::LANES;
    float4 acc = f4_zero();
    max_bwd_span<NMAX_NB_BLOCK_BWD>(start + g * rg::LANES, end, rg::BLOCK, t, rowidx_t, perm_t, n_edges, n_rows, arg4, dY4, acc);
    rg::store_column_sums(s_acc, g, t, acc, base, dX, c);
}

}  // namespace

extern "C" int32_t mmrec_neighbor_max_group_max(void) { return rg::GROUP_MAX; }

extern "C" int mmrec_neighbor_max_f32(const int32_t* rowptr, int32_t n_rows, const int32_t* colidx, const int64_t* perm,
                                      const int32_t* long_rows, int32_t n_long, const float* X, int64_t n_x, int32_t d,
                                      int64_t n_edges, float* Y, int32_t* arg, mmrec_stream_t stream) {
    if (d != 4 * rg::LANES) return MMREC_ERR_UNSUPPORTED;
    if (n_rows < 0 || n_edges < 0 || n_long < 0 || n_x < 0) return MMREC_ERR_BAD_ARG;
    if (n_rows == 0) return 0;                                             // nothing to write
    if (n_edges > INT32_MAX || n_x > INT32_MAX) return MMREC_ERR_UNSUPPORTED;
    if (!rowptr || !Y || !arg) return MMREC_ERR_BAD_ARG;
    if (n_edges > 0 && (!colidx || !X)) return MMREC_ERR_BAD_ARG;
    if (n_long > 0 && !long_rows) return MMREC_ERR_BAD_ARG;
    hipStream_t s = mmrec_stream(stream);
    const float4* X4 = reinterpret_cast<const float4*>(X);
    rg::launch_pair(
        n_rows, n_long,
        [&](dim3 grid) {
            hipLaunchKernelGGL(neighbor_max_group_kernel, grid, dim3(rg::BLOCK), 0, s, rowptr, (int)n_rows, colidx, perm, n_long > 0,
                               X4, (int)n_x, (int)n_edges, reinterpret_cast<float4*>(Y), reinterpret_cast<int4*>(arg));
        },
        [&](dim3 grid) {
            hipLaunchKernelGGL(neighbor_max_block_kernel, grid, dim3(rg::BLOCK), 0, s, rowptr, (int)n_rows, colidx, perm, long_rows,
                               X4, (int)n_x, (int)n_edges, Y, arg);
        });
    MMREC_RETURN_LAUNCH_STATUS();
}

extern "C" int mmrec_neighbor_max_bwd_f32(const int32_t* rowptr_t, int32_t n_cols, const int32_t* rowidx_t,
                                          const int64_t* perm_t, const int32_t* long_cols, int32_t n_long_t,
                                          const int32_t* arg, int64_t n_rows, const float* dY, int32_t d, int64_t n_edges,
                                          float* dX, const float* dX_base, mmrec_stream_t stream) {
    if (d != 4 * rg::LANES) return MMREC_ERR_UNSUPPORTED;
    if (n_cols < 0 || n_edges < 0 || n_long_t < 0 || n_rows < 0) return MMREC_ERR_BAD_ARG;
    if (n_cols == 0) return 0;                                             // nothing to write
    if (n_edges > INT32_MAX || n_rows > INT32_MAX) return MMREC_ERR_UNSUPPORTED;
    if (!rowptr_t || !dX || dX_base == dX) return MMREC_ERR_BAD_ARG;
    if (n_edges > 0 && (!rowidx_t || !arg || !dY)) return MMREC_ERR_BAD_ARG;
    if (n_long_t > 0 && !long_cols) return MMREC_ERR_BAD_ARG;
    hipStream_t s = mmrec_stream(stream);
    const int4* arg4 = reinterpret_cast<const int4*>(arg);
    const float4* dY4 = reinterpret_cast<const float4*>(dY);
    rg::launch_pair(
        n_cols, n_long_t,
        [&](dim3 grid) {
            hipLaunchKernelGGL(neighbor_max_bwd_group_kernel, grid, dim3(rg::BLOCK), 0, s, rowptr_t, (int)n_cols, rowidx_t, perm_t,
                               n_long_t > 0, (int)n_rows, (int)n_edges, arg4, dY4, reinterpret_cast<const float4*>(dX_base),
                               reinterpret_cast<float4*>(dX));
        },
        [&](dim3 grid) {
            hipLaunchKernelGGL(neighbor_max_bwd_block_kernel, grid, dim3(rg::BLOCK), 0, s, rowptr_t, (int)n_cols, rowidx_t, perm_t,
                               long_cols, (int)n_rows, (int)n_edges, arg4, dY4, dX_base, dX);
        });
    MMREC_RETURN_LAUNCH_STATUS();
}
