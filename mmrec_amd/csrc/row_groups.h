// The row-group skeleton of the per-row edge ops (edge_softmax.hip, edge_attention.hip, neighbor_max.hip): what they share,
// written once.  Each walks the rows of a CSR in a "group" kernel, one 16-lane group per row (four rows per wave, 16 per
// workgroup), and hands the rows longer than GROUP_MAX to a "block" kernel, one 256-thread workgroup per LISTED row (the
// list of mmrec_spmm_plan_fill at that threshold).  Slot j of a row lives at position p = perm ? perm[j] : j of the caller's
// (COO) arrays; row spans are clamped to the arrays and a position outside them is an absent edge.  The per-op inner spans,
// reduction structs and tuning constants stay in their files.
#pragma once
#include "common.h"

namespace rg {

constexpr int BLOCK = 256;
constexpr int LANES = 16;                       // lanes per short row (64 columns as float4)
constexpr int GROUPS = BLOCK / LANES;           // rows per workgroup in a group kernel, partial states per listed row
constexpr int GROUP_MAX = 256;                  // longer rows go to the block kernel (when the caller lists them): ONE constant,
                                                // so one long-row list per CSR serves every op (the three *_group_max() exports)
constexpr int MAX_BLOCKS = 2048;                // 8 resident 256-thread workgroups on each of 256 CUs; the loop strides the rest

// position of CSR slot j in the caller's arrays; a slot whose position is outside them is skipped, never used as an address
__device__ __forceinline__ int slot_pos(const int64_t* __restrict__ perm, int j, int n_edges) {
    if (!perm) return j;
    const int64_t p = perm[j];
    return (p >= 0 && p < n_edges) ? (int)p : -1;
}

// [start, end) of row r, clamped to the arrays
__device__ __forceinline__ void row_span(const int32_t* __restrict__ rowptr, int r, int n_edges, int& start, int& end) {
    start = rowptr[r];
    end = rowptr[r + 1];
    if (start < 0) start = 0;
    if (end > n_edges) end = n_edges;
}

// The group kernels' loop: body(r, start, end, t) for every row this 16-lane group owns, t the lane within the group; with
// skip_long the rows of more than GROUP_MAX entries are left to the block kernel.  The row -- and with it every branch
// around a shuffle or butterfly, a `return` from the body included -- is the same for the 16 lanes of a group.
// (Not in neighbor_max.hip: see below.)
template <class Body>
__device__ __forceinline__ void for_short_rows(const int32_t* __restrict__ rowptr, int n_rows, int n_edges, bool skip_long,
                                               const Body& body) {
    const int t = threadIdx.x % LANES;
    const int stride = gridDim.x * GROUPS;
    for (long r = (long)blockIdx.x * GROUPS + threadIdx.x / LANES; r < n_rows; r += stride) {
        int start, end;
        row_span(rowptr, (int)r, n_edges, start, end);
        if (skip_long && end - start > GROUP_MAX) continue;                // the block kernel's
        body(r, start, end, t);
    }
}

// The block kernels' preamble (r = long_rows[blockIdx.x], the bounds check by which the WHOLE workgroup leaves before any
// __syncthreads(), row_span, the t / g split) is NOT a helper here: as a function that reports "no row" it made the compiler
// emit other code for every block kernel (160 - 670 instruction lines of each), and the workgroup of a hub row is a call's
// tail.  The same holds for for_short_rows in neighbor_max.hip, whose loops are written out.

// The block kernels' plain epilogue (every thread of the workgroup calls it): the 16 groups' float4 partial sums go through
// LDS and the first wave, one column of the row per lane, stores out[r] = base[r] (0 without a base) + the partials added
// in the order g = 0 ... 15.
__device__ __forceinline__ void store_column_sums(float4 (&s_acc)[GROUPS][LANES], int g, int t, float4 acc,
                                                  const float* __restrict__ base, float* __restrict__ out, int r) {
    s_acc[g][t] = acc;
    __syncthreads();
    if (threadIdx.x < 4 * LANES) {
        const float* col = reinterpret_cast<const float*>(&s_acc[0][0]) + threadIdx.x;
        float y = base ? base[(size_t)r * (4 * LANES) + threadIdx.x] : 0.f;
#pragma unroll
        for (int k = 0; k < GROUPS; ++k) y += col[k * 4 * LANES];
        out[(size_t)r * (4 * LANES) + threadIdx.x] = y;
    }
}

// The host's launch pair: group(grid) over n rows -- 16 rows per workgroup, at most MAX_BLOCKS workgroups -- and, when rows
// are listed, block(grid) with one workgroup per listed row.  Both launch BLOCK threads.
template <class Group, class Block>
inline void launch_pair(int64_t n, int32_t n_long, const Group& group, const Block& block) {
    const int64_t blocks = (n + GROUPS - 1) / GROUPS;
    group(dim3((unsigned)(blocks < MAX_BLOCKS ? blocks : MAX_BLOCKS)));
    if (n_long > 0) block(dim3((unsigned)n_long));
}

}  // namespace rg
