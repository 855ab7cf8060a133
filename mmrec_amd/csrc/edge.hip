// Per-edge dot products (SDDMM) and their backward: out[e] = <A[rows[e]], B[cols[e]]>  (include/mmrec_hip.h, ABI 16).
//
// One group of L = min(d, 64) / 4 lanes per edge (16 lanes at d >= 64: four edges per wave).  Forward: lane t of the group
// loads ONE float4 of each row per 64 columns -- a 256-byte coalesced row read per group, the access shape of spmm.hip --
// and runs one fma chain over its own d / 16 (4 for the slices) columns; the group sum is the DPP / ds_swizzle butterfly of
// common.h (row16_sum at 16 lanes, its lower stages for the narrower groups), so the summation order is fixed and the bits
// repeat run after run.  A term meets d / 16 (or 4) roundings in its lane's chain and log2(L) in the butterfly.
// Backward: the same edge -> group mapping; lane t owns the columns t, t + L, t + 2L, ... of the row, so ONE atomic
// wave-instruction adds a contiguous 4 L-byte segment per edge (64 B at d >= 64) instead of every fourth dword of 256 B.
// Nothing is staged in LDS: the node tables are a few MB and sit in L2, and consecutive edges of a CSR-ordered list read the
// same A row.
#include "common.h"

namespace {

constexpr int EDGE_BLOCK = 256;
constexpr int EDGE_MAX_BLOCKS = 2048;        // 8 resident 256-thread workgroups on each of 256 CUs; the loop strides the rest

template <int L>
__device__ __forceinline__ float group_sum(float v) {
    if (L >= 16) v += lane_xor_f<8>(v);
    if (L >= 8) v += lane_xor_f<4>(v);
    if (L >= 4) v += lane_xor_f<2>(v);
    v += lane_xor_f<1>(v);
    return v;
}

// acc + <a, b> as ONE chain: w, z, y, x
__device__ __forceinline__ float f4_dot_acc(float4 a, float4 b, float acc) {
    return fmaf(a.x, b.x, fmaf(a.y, b.y, fmaf(a.z, b.z, fmaf(a.w, b.w, acc))));
}

// D: row width; L lanes per edge; NB = max(D / 64, 1) float4 per lane and row
template <int D>
__global__ __launch_bounds__(EDGE_BLOCK) void edge_dot_kernel(const float* __restrict__ A, long n_a, const float* __restrict__ B,
                                                              long n_b, const int64_t* __restrict__ rows,
                                                              const int64_t* __restrict__ cols, int n_edges,
                                                              float* __restrict__ out) {
    constexpr int L = (D < 64 ? D : 64) / 4;
    constexpr int NB = D < 64 ? 1 : D / 64;
    constexpr int GROUPS = EDGE_BLOCK / L;
    const int t = threadIdx.x % L;
    const long stride = (long)gridDim.x * GROUPS;
    for (long e = (long)blockIdx.x * GROUPS + threadIdx.x / L; e < n_edges; e += stride) {
        const int64_t r = rows[e], c = cols[e];
        // an id outside its table reads as a row of zeros and is never used as an address; the whole group takes one side
        const bool ok = r >= 0 && r < n_a && c >= 0 && c < n_b;
        float acc = 0.f;
        if (ok) {
            const float4* a = reinterpret_cast<const float4*>(A + (size_t)r * D) + t;
            const float4* b = reinterpret_cast<const float4*>(B + (size_t)c * D) + t;
            float4 av[NB], bv[NB];
#pragma unroll
            for (int k = 0; k < NB; ++k) {
                av[k] = a[k * 16];
                bv[k] = b[k * 16];
            }
#pragma unroll
            for (int k = 0; k < NB; ++k) acc = f4_dot_acc(av[k], bv[k], acc);
        }
        acc = group_sum<L>(acc);
        if (t == 0) out[e] = acc;
    }
}

template <int D>
__global__ __launch_bounds__(EDGE_BLOCK) void edge_dot_bwd_kernel(const float* __restrict__ g, const float* __restrict__ A, long n_a,
                                                                  const float* __restrict__ B, long n_b,
                                                                  const int64_t* __restrict__ rows,
                                                                  const int64_t* __restrict__ cols, int n_edges, float* dA,
                                                                  float* dB) {
    constexpr int L = (D < 64 ? D : 64) / 4;
    constexpr int NC = D / L;                 // columns per lane: t, t + L, ...
    constexpr int GROUPS = EDGE_BLOCK / L;
    const int t = threadIdx.x % L;
    const long stride = (long)gridDim.x * GROUPS;
    for (long e = (long)blockIdx.x * GROUPS + threadIdx.x / L; e < n_edges; e += stride) {
        const int64_t r = rows[e], c = cols[e];
        if (!(r >= 0 && r < n_a && c >= 0 && c < n_b)) continue;      // adds nothing
        const float ge = g[e];
        const size_t ra = (size_t)r * D + t, cb = (size_t)c * D + t;
        if (dA) {
            float v[NC];
#pragma unroll
            for (int k = 0; k < NC; ++k) v[k] = ge * B[cb + k * L];
#pragma unroll
            for (int k = 0; k < NC; ++k) unsafeAtomicAdd(dA + ra + k * L, v[k]);
        }
        if (dB) {
            float v[NC];
#pragma unroll
            for (int k = 0; k < NC; ++k) v[k] = ge * A[ra + k * L];
#pragma unroll
            for (int k = 0; k < NC; ++k) unsafeAtomicAdd(dB + cb + k * L, v[k]);
        }
    }
}

inline bool width_served(int d) { return d == 8 || d == 16 || d == 32 || (d > 0 && d % 64 == 0 && d <= 384); }

inline int edge_grid(int64_t n_edges, int d) {
    const int groups = EDGE_BLOCK / ((d < 64 ? d : 64) / 4);
    const int64_t blocks = (n_edges + groups - 1) / groups;
    return (int)(blocks < EDGE_MAX_BLOCKS ? blocks : EDGE_MAX_BLOCKS);
}

}  // namespace

#define MMREC_EDGE_WIDTHS(X) X(8) X(16) X(32) X(64) X(128) X(192) X(256) X(320) X(384)

extern "C" int mmrec_edge_dot_f32(const float* A, int64_t n_a, const float* B, int64_t n_b, const int64_t* rows,
                                  const int64_t* cols, int64_t n_edges, int32_t d, float* out, mmrec_stream_t stream) {
    if (!width_served(d)) return MMREC_ERR_UNSUPPORTED;
    if (n_a < 0 || n_b < 0 || n_edges < 0) return MMREC_ERR_BAD_ARG;
    if (n_edges == 0) return 0;
    if (n_edges > INT32_MAX) return MMREC_ERR_UNSUPPORTED;
    if (!A || !B || !rows || !cols || !out) return MMREC_ERR_BAD_ARG;
    const dim3 grid(edge_grid(n_edges, d)), block(EDGE_BLOCK);
    hipStream_t s = mmrec_stream(stream);
    switch (d) {
#define MMREC_EDGE_CASE(D)                                                                                              \
    case D:                                                                                                             \
        hipLaunchKernelGGL(edge_dot_kernel<D>, grid, block, 0, s, A, (long)n_a, B, (long)n_b, rows, cols, (int)n_edges, out); \
        break;
        MMREC_EDGE_WIDTHS(MMREC_EDGE_CASE)
#undef MMREC_EDGE_CASE
    }
    MMREC_RETURN_LAUNCH_STATUS();
}

extern "C" int mmrec_edge_dot_bwd_f32(const float* g, const float* A, int64_t n_a, const float* B, int64_t n_b,
                                      const int64_t* rows, const int64_t* cols, int64_t n_edges, int32_t d, float* dA,
                                      float* dB, mmrec_stream_t stream) {
    if (!width_served(d)) return MMREC_ERR_UNSUPPORTED;
    if (n_a < 0 || n_b < 0 || n_edges < 0) return MMREC_ERR_BAD_ARG;
    if (n_edges == 0) return 0;
    if (n_edges > INT32_MAX) return MMREC_ERR_UNSUPPORTED;
    if (!g || !A || !B || !rows || !cols) return MMREC_ERR_BAD_ARG;
    if (!dA && !dB) return 0;
    if (dA && dA == dB && (A != B || n_a != n_b)) return MMREC_ERR_BAD_ARG;      // one buffer for both sums: one table
    const dim3 grid(edge_grid(n_edges, d)), block(EDGE_BLOCK);
    hipStream_t s = mmrec_stream(stream);
    switch (d) {
#define MMREC_EDGE_CASE(D)                                                                                              \
    case D:                                                                                                             \
        hipLaunchKernelGGL(edge_dot_bwd_kernel<D>, grid, block, 0, s, g, A, (long)n_a, B, (long)n_b, rows, cols,        \
                           (int)n_edges, dA, dB);                                                                       \
        break;
        MMREC_EDGE_WIDTHS(MMREC_EDGE_CASE)
#undef MMREC_EDGE_CASE
    }
    MMREC_RETURN_LAUNCH_STATUS();
}
