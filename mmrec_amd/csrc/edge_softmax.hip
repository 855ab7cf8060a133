// Segment softmax over the edges of a graph and its backward (include/mmrec_hip.h, additive to ABI 16).
//
// Segments are the rows of a CSR rowptr; entry j of row r lives at position p = perm ? perm[j] : j of the caller's (COO)
// arrays.  Forward  out[p] = exp(s[p] - m_r) / (sum_q exp(s[q] - m_r) + eps),  m_r = max s over the row;
// backward ds[p] = alpha[p] * (g[p] - sum_q alpha[q] g[q]).
//
// Two kernels share one row routine (row_softmax / row_softmax_bwd), which differs only in how many lanes own a row and how
// they reduce:
//   group  16 lanes per row (four rows per wave, 16 per workgroup), lanes stride over the row's entries, maximum and sum by the
//          DPP / ds_swizzle butterfly of common.h (xor 8, 4, 2, 1).  A term of the sum meets ceil(len / 16) roundings in its
//          lane's chain and 4 in the butterfly.
//   block  one 256-thread workgroup per LISTED row (rows longer than rg::GROUP_MAX: the list of mmrec_spmm_plan_fill at that
//          threshold): the wave butterfly (xor 32 ... 1), then the four wave partials through LDS, added as (w0 + w1) + (w2 +
//          w3).  ceil(len / 256) + 8 roundings.
// The first KEEP entries of a lane stay in registers between the passes (rows of <= 64 entries at 16 lanes, <= 1024 at 256
// never re-read a score); a longer row's further entries park exp(s - m) in `out` -- written and read back by the same lane, so
// no fence -- and are divided in place.  No atomics: the summation order is a function of the row's length alone, so the bits
// of both directions repeat run after run.  Empty rows write nothing.  Non-finite scores follow the arithmetic: the maximum
// skips NaN (v_max_f32), the NaN then enters the sum through exp; +inf or an all -inf row give inf - inf = NaN; so such a
// row is NaN in every entry and no other row is touched, and a -inf next to a finite maximum is exp(-inf) = 0 exactly.
#include "row_groups.h"

#include <math.h>

namespace {

using rg::slot_pos;

constexpr int SEG_KEEP = 4;                     // entries per lane kept in registers between the passes

struct GroupReduce {
    __device__ __forceinline__ float max(float v) const {
        v = fmaxf(v, lane_xor_f<8>(v));
        v = fmaxf(v, lane_xor_f<4>(v));
        v = fmaxf(v, lane_xor_f<2>(v));
        return fmaxf(v, lane_xor_f<1>(v));
    }
    __device__ __forceinline__ float sum(float v) const { return row16_sum(v); }
};

// every thread of the workgroup calls these (the row is the workgroup's)
struct BlockReduce {
    float* lds;                                  // rg::BLOCK / 64 floats
    __device__ __forceinline__ float max(float v) const {
        v = fmaxf(v, lane_xor_f<32>(v));
        v = fmaxf(v, lane_xor_f<16>(v));
        v = GroupReduce().max(v);
        __syncthreads();                         // the previous reduction's readers are done with lds
        if (threadIdx.x % MMREC_WAVE == 0) lds[threadIdx.x / MMREC_WAVE] = v;
        __syncthreads();
        return fmaxf(fmaxf(lds[0], lds[1]), fmaxf(lds[2], lds[3]));
    }
    __device__ __forceinline__ float sum(float v) const {
        v = wave_sum(v);
        __syncthreads();
        if (threadIdx.x % MMREC_WAVE == 0) lds[threadIdx.x / MMREC_WAVE] = v;
        __syncthreads();
        return (lds[0] + lds[1]) + (lds[2] + lds[3]);
    }
};

// the row's slots are [start, end); lane t of LANES owns the slots start + t, start + t + LANES, ...
template <int LANES, class Reduce>
__device__ __forceinline__ void row_softmax(int start, int end, int t, const int64_t* __restrict__ perm,
                                            const float* __restrict__ score, int n_edges, float eps, float* __restrict__ out,
                                            const Reduce& red) {
    int pk[SEG_KEEP];
    float vk[SEG_KEEP];
    float m = -INFINITY;
#pragma unroll
    for (int k = 0; k < SEG_KEEP; ++k) {
        const int j = start + t + k * LANES;
        pk[k] = j < end ? slot_pos(perm, j, n_edges) : -1;
        vk[k] = pk[k] >= 0 ? score[pk[k]] : -INFINITY;
        m = fmaxf(m, vk[k]);
    }
    for (int j = start + t + SEG_KEEP * LANES; j < end; j += LANES) {
        const int p = slot_pos(perm, j, n_edges);
        if (p >= 0) m = fmaxf(m, score[p]);
    }
    m = red.max(m);
    float acc = 0.f;
#pragma unroll
    for (int k = 0; k < SEG_KEEP; ++k) {
        vk[k] = pk[k] >= 0 ? expf(vk[k] - m) : 0.f;
        acc += vk[k];
    }
    for (int j = start + t + SEG_KEEP * LANES; j < end; j += LANES) {
        const int p = slot_pos(perm, j, n_edges);
        if (p >= 0) {
            const float e = expf(score[p] - m);
            out[p] = e;                                       // parked: this lane reads it back below
            acc += e;
        }
    }
    const float den = red.sum(acc) + eps;
#pragma unroll
    for (int k = 0; k < SEG_KEEP; ++k)
        if (pk[k] >= 0) out[pk[k]] = vk[k] / den;
    for (int j = start + t + SEG_KEEP * LANES; j < end; j += LANES) {
        const int p = slot_pos(perm, j, n_edges);
        if (p >= 0) out[p] = out[p] / den;
    }
}

template <int LANES, class Reduce>
__device__ __forceinline__ void row_softmax_bwd(int start, int end, int t, const int64_t* __restrict__ perm,
                                                const float* __restrict__ alpha, const float* __restrict__ g, int n_edges,
                                                float* __restrict__ ds, const Reduce& red) {
    int pk[SEG_KEEP];
    float ak[SEG_KEEP], gk[SEG_KEEP];
    float acc = 0.f;
#pragma unroll
    for (int k = 0; k < SEG_KEEP; ++k) {
        const int j = start + t + k * LANES;
        pk[k] = j < end ? slot_pos(perm, j, n_edges) : -1;
        ak[k] = pk[k] >= 0 ? alpha[pk[k]] : 0.f;
        gk[k] = pk[k] >= 0 ? g[pk[k]] : 0.f;
        acc = fmaf(ak[k], gk[k], acc);
    }
    for (int j = start + t + SEG_KEEP * LANES; j < end; j += LANES) {
        const int p = slot_pos(perm, j, n_edges);
        if (p >= 0) acc = fmaf(alpha[p], g[p], acc);
    }
    const float dot = red.sum(acc);
#pragma unroll
    for (int k = 0; k < SEG_KEEP; ++k)
        if (pk[k] >= 0) ds[pk[k]] = ak[k] * (gk[k] - dot);
    for (int j = start + t + SEG_KEEP * LANES; j < end; j += LANES) {
        const int p = slot_pos(perm, j, n_edges);
        if (p >= 0) ds[p] = alpha[p] * (g[p] - dot);
    }
}

// BWD = false: a = score, b unused, c = eps; BWD = true: a = alpha, b = g
template <bool BWD>
__global__ __launch_bounds__(rg::BLOCK) void segment_softmax_group_kernel(const int32_t* __restrict__ rowptr, int n_rows,
                                                                          const int64_t* __restrict__ perm, bool skip_long,
                                                                          const float* __restrict__ a,
                                                                          const float* __restrict__ b, int n_edges, float eps,
                                                                          float* __restrict__ out) {
    rg::for_short_rows(rowptr, n_rows, n_edges, skip_long, [&](long, int start, int end, int t) {
        if (end <= start) return;
        if (BWD)
            row_softmax_bwd<rg::LANES>(start, end, t, perm, a, b, n_edges, out, GroupReduce());
        else
            row_softmax<rg::LANES>(start, end, t, perm, a, n_edges, eps, out, GroupReduce());
    });
}

template <bool BWD>
__global__ __launch_bounds__(rg::BLOCK) void segment_softmax_block_kernel(const int32_t* __restrict__ rowptr, int n_rows,
                                                                          const int64_t* __restrict__ perm,
                                                                          const int32_t* __restrict__ long_rows,
                                                                          const float* __restrict__ a,
                                                                          const float* __restrict__ b, int n_edges, float eps,
                                                                          float* __restrict__ out) {
    __shared__ float lds[rg::BLOCK / MMREC_WAVE];
    const int r = long_rows[blockIdx.x];
    if (r < 0 || r >= n_rows) return;                        // (the whole workgroup)
    int start, end;
    rg::row_span(rowptr, r, n_edges, start, end);
    if (end <= start) return;
    const BlockReduce red{lds};
    if (BWD)
        row_softmax_bwd<rg::BLOCK>(start, end, threadIdx.x, perm, a, b, n_edges, out, red);
    else
        row_softmax<rg::BLOCK>(start, end, threadIdx.x, perm, a, n_edges, eps, out, red);
}

inline int seg_check(const int32_t* rowptr, int32_t n_rows, const int32_t* long_rows, int32_t n_long, const float* a,
                     const float* b, int64_t n_edges, const float* out) {
    if (n_rows < 0 || n_edges < 0 || n_long < 0) return MMREC_ERR_BAD_ARG;
    if (n_edges == 0 || n_rows == 0) return -1;              // nothing to launch
    if (n_edges > INT32_MAX) return MMREC_ERR_UNSUPPORTED;
    if (!rowptr || !a || !b || !out) return MMREC_ERR_BAD_ARG;
    if (n_long > 0 && !long_rows) return MMREC_ERR_BAD_ARG;
    return 0;
}

template <bool BWD>
int seg_launch(const int32_t* rowptr, int32_t n_rows, const int64_t* perm, const int32_t* long_rows, int32_t n_long,
               const float* a, const float* b, int64_t n_edges, float eps, float* out, mmrec_stream_t stream) {
    hipStream_t s = mmrec_stream(stream);
    rg::launch_pair(
        n_rows, n_long,
        [&](dim3 grid) {
            hipLaunchKernelGGL(segment_softmax_group_kernel<BWD>, grid, dim3(rg::BLOCK), 0, s, rowptr, (int)n_rows, perm,
                               n_long > 0, a, b, (int)n_edges, eps, out);
        },
        [&](dim3 grid) {
            hipLaunchKernelGGL(segment_softmax_block_kernel<BWD>, grid, dim3(rg::BLOCK), 0, s, rowptr, (int)n_rows, perm,
                               long_rows, a, b, (int)n_edges, eps, out);
        });
    MMREC_RETURN_LAUNCH_STATUS();
}

}  // namespace

extern "C" int32_t mmrec_segment_softmax_group_max(void) { return rg::GROUP_MAX; }

extern "C" int mmrec_segment_softmax_f32(const int32_t* rowptr, int32_t n_rows, const int64_t* perm, const int32_t* long_rows,
                                         int32_t n_long, const float* score, int64_t n_edges, float eps, float* out,
                                         mmrec_stream_t stream) {
    const int rc = seg_check(rowptr, n_rows, long_rows, n_long, score, score, n_edges, out);
    if (rc) return rc < 0 ? 0 : rc;
    return seg_launch<false>(rowptr, n_rows, perm, long_rows, n_long, score, nullptr, n_edges, eps, out, stream);
}

extern "C" int mmrec_segment_softmax_bwd_f32(const int32_t* rowptr, int32_t n_rows, const int64_t* perm,
                                             const int32_t* long_rows, int32_t n_long, const float* alpha, const float* g,
                                             int64_t n_edges, float* ds, mmrec_stream_t stream) {
    const int rc = seg_check(rowptr, n_rows, long_rows, n_long, alpha, g, n_edges, ds);
    if (rc) return rc < 0 ? 0 : rc;
    return seg_launch<true>(rowptr, n_rows, perm, long_rows, n_long, alpha, g, n_edges, 0.f, ds, stream);
}
