// Hypergraph message passing of LGMRec (include/mmrec_hip.h, additive to ABI 16): the Gumbel-softmax hyperedge assignment with
// its dropout, and the HGNN layer  lat = P_i^T X,  X' = P_i lat,  U' = P_u lat  (lgmrec.py:23-36, 196-216), each with its
// backward.  The operands are [n, H] with H hyperedges (4 in every shipped setting but Clothing's 64) against a 64-wide table:
// a 4-row GEMM reduced over tens of thousands of rows, the shape a library GEMM serves worst.  Served: d = 64, 1 <= H <= 8.
//
// THE ASSIGNMENT (one launch each way, one thread per row, H values in registers)
//     x = (a + g) / tau;  p = exp(x - max x) / sum exp(x - max x);  P = keep ? p * keep / q : p
// The row maximum is subtracted, so finite logits of any spread give a finite P.  The kernels draw nothing: g (the Gumbel
// noise) and keep (a 0 / 1 mask) are the caller's.  STATE BETWEEN THE TWO CALLS: p.  Without a mask P is p and the forward
// writes nothing else; with a mask P has lost p at the dropped entries, which the backward needs (a dropped entry's logit
// still gets -p_h sum_k p_k s_k / tau), so the forward also writes p where the caller gives it a second buffer.
//     s = dP * keep / q  (no mask: dP);   d a = p * (s - sum_h p_h s_h) / tau
// A row whose mask is all zero: P = 0 and s = 0, so d a = 0.
//
// THE LAYER.  Reduce, finish, expand -- three launches forward, three backward, X read once and every output written once.
//   reduce  one 256-thread workgroup per block of R = mmrec_hyper_rows_per_block(n) consecutive rows.  Wave w of the four walks
//           the rows [w R / 4, (w + 1) R / 4) of the block in order, one column per lane and H accumulators:
//           acc[h] = fma(P[r][h], V[r][lane], acc[h]); P[r][h] is the same for the whole wave (a scalar load).  The four
//           waves' partials are added through LDS as ((w0 + w1) + w2) + w3 and stored: part[block][h][c].
//   finish  one 1024-thread workgroup per hyperedge: wave k of the sixteen adds the blocks k, k + 16, ... in order, the sixteen
//           sums are added in the order k = 0 ... 15.  A fixed order, no atomics: the same bits every call.
//           A term of lat[h][c] therefore meets at most R / 4 + 3 + ceil(blocks / 16) + 15 additions.
//   expand  16 lanes per output row, a float4 of columns each, lat in registers: out[r] = P[r][0] lat[0], then one fma per
//           further hyperedge, in order.  Items and users in one launch.
// Backward of a layer, given dU and dX (either may be NULL: zeros):
//     dlat = P_i^T dX + P_u^T dU           the same reduce over the item blocks, then the user blocks; the same finish
//     dP_i[r][h] = <dX[r], lat[h]> + <X[r], dlat[h]>      per lane an fma chain over its four columns of dX then of X, then
//     dP_u[r][h] = <dU[r], lat[h]>                        the butterfly over the row's 16 lanes (row16_sum)
//     dX_prev[r] = sum_h P_i[r][h] dlat[h]                as the expand
// Workspace: 512 floats (dlat) + one H x 64 partial per block of either side.  Nothing is allocated, nothing synchronises.
#include "common.h"

namespace {

constexpr int HYP_D = 64;
constexpr int HYP_HMAX = 8;
constexpr int HYP_BLOCK = 256;
constexpr int HYP_WAVES = HYP_BLOCK / MMREC_WAVE;
constexpr int HYP_GROUP = 16;                    // lanes per row in the expand and the row pass: 64 columns as float4
constexpr int HYP_GROUPS = HYP_BLOCK / HYP_GROUP;
constexpr int HYP_SLICES = 16;                   // waves of the finish workgroup
constexpr int HYP_MIN_ROWS = 64;                 // rows per reduce block: 16 per wave at least
constexpr int HYP_MAX_PARTS = 2048;              // ... and more of them where the table has more than 131,072 rows
constexpr int HYP_MAX_BLOCKS = 2048;             // grid cap of the row kernels; the loop strides the rest
constexpr int HYP_NB = 4;                        // rows in flight per wave of the reduce
constexpr int64_t HYP_MAX_ROWS = (int64_t)1 << 30;

inline int hyp_rows_per_block(int64_t n) {
    int64_t r = (n + HYP_MAX_PARTS - 1) / HYP_MAX_PARTS;
    r = (r + HYP_MIN_ROWS - 1) / HYP_MIN_ROWS * HYP_MIN_ROWS;
    return (int)(r < HYP_MIN_ROWS ? HYP_MIN_ROWS : r);
}
inline int hyp_blocks(int64_t n) { return n <= 0 ? 0 : (int)((n + hyp_rows_per_block(n) - 1) / hyp_rows_per_block(n)); }

// ------------------------------------------------------------------------------------------------ the assignment
template <int H>
__global__ __launch_bounds__(HYP_BLOCK) void hyper_assign_fwd_kernel(
    const float* __restrict__ logits, const float* __restrict__ noise, const float* __restrict__ keep, long n, float tau,
    float q, float* __restrict__ P, float* __restrict__ p_soft) {
    const long stride = (long)gridDim.x * HYP_BLOCK;
    for (long r = (long)blockIdx.x * HYP_BLOCK + threadIdx.x; r < n; r += stride) {
        const size_t o = (size_t)r * H;
        float x[H];
#pragma unroll
        for (int h = 0; h < H; ++h) x[h] = (logits[o + h] + noise[o + h]) / tau;
        float m = x[0];
#pragma unroll
        for (int h = 1; h < H; ++h) m = fmaxf(m, x[h]);
        float sum = 0.f;
#pragma unroll
        for (int h = 0; h < H; ++h) {
            x[h] = expf(x[h] - m);
            sum += x[h];
        }
#pragma unroll
        for (int h = 0; h < H; ++h) {
            const float p = x[h] / sum;
            if (p_soft) p_soft[o + h] = p;
            P[o + h] = keep ? p * keep[o + h] / q : p;
        }
    }
}

template <int H>
__global__ __launch_bounds__(HYP_BLOCK) void hyper_assign_bwd_kernel(
    const float* __restrict__ p_soft, const float* __restrict__ keep, const float* __restrict__ dP, long n, float tau, float q,
    float* __restrict__ dlogits) {
    const long stride = (long)gridDim.x * HYP_BLOCK;
    for (long r = (long)blockIdx.x * HYP_BLOCK + threadIdx.x; r < n; r += stride) {
        const size_t o = (size_t)r * H;
        float p[H], s[H];
        float dot = 0.f;
#pragma unroll
        for (int h = 0; h < H; ++h) {
            p[h] = p_soft[o + h];
            s[h] = keep ? dP[o + h] * keep[o + h] / q : dP[o + h];
            dot = fmaf(p[h], s[h], dot);
        }
#pragma unroll
        for (int h = 0; h < H; ++h) dlogits[o + h] = p[h] * (s[h] - dot) / tau;
    }
}

// ------------------------------------------------------------------------------------------------ reduce, finish
// part[block][h][c] = sum over the block's rows r of P[r][h] V[r][c]; blocks [0, nb_a) walk side a, the rest side b
template <int H>
__global__ __launch_bounds__(HYP_BLOCK) void hyper_reduce_kernel(
    const float* __restrict__ P_a, const float* __restrict__ V_a, long n_a, int R_a, int nb_a, const float* __restrict__ P_b,
    const float* __restrict__ V_b, long n_b, int R_b, float* __restrict__ part) {
    __shared__ float s_part[HYP_WAVES][H * HYP_D];
    const bool a = (int)blockIdx.x < nb_a;
    const float* __restrict__ P = a ? P_a : P_b;
    const float* __restrict__ V = a ? V_a : V_b;
    const long n = a ? n_a : n_b;
    const int R = a ? R_a : R_b;
    const long blk = a ? blockIdx.x : blockIdx.x - nb_a;
    const int lane = threadIdx.x % MMREC_WAVE;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x / MMREC_WAVE);    // the wave's rows are the same for every lane
    const int per_wave = R / HYP_WAVES;
    const long r0 = blk * R + (long)w * per_wave;
    const long r1 = r0 + per_wave < n ? r0 + per_wave : n;
    float acc[H];
#pragma unroll
    for (int h = 0; h < H; ++h) acc[h] = 0.f;
    for (long r = r0; r < r1; r += HYP_NB) {
        float x[HYP_NB];
#pragma unroll
        for (int u = 0; u < HYP_NB; ++u) x[u] = r + u < r1 ? V[(size_t)(r + u) * HYP_D + lane] : 0.f;
#pragma unroll
        for (int u = 0; u < HYP_NB; ++u) {
            if (r + u >= r1) break;
            const float* __restrict__ pr = P + (size_t)(r + u) * H;
#pragma unroll
            for (int h = 0; h < H; ++h) acc[h] = fmaf(pr[h], x[u], acc[h]);
        }
    }
#pragma unroll
    for (int h = 0; h < H; ++h) s_part[w][h * HYP_D + lane] = acc[h];
    __syncthreads();
    for (int e = threadIdx.x; e < H * HYP_D; e += HYP_BLOCK)
        part[(size_t)blockIdx.x * (H * HYP_D) + e] = ((s_part[0][e] + s_part[1][e]) + s_part[2][e]) + s_part[3][e];
}

// out[h][c] = the nb partials added: wave k takes k, k + 16, ... in order, then the sixteen sums in order
__global__ __launch_bounds__(HYP_SLICES * MMREC_WAVE) void hyper_finish_kernel(const float* __restrict__ part, int nb, int H,
                                                                              float* __restrict__ out) {
    __shared__ float s_sum[HYP_SLICES][HYP_D];
    const int h = blockIdx.x;
    const int lane = threadIdx.x % MMREC_WAVE, k = threadIdx.x / MMREC_WAVE;
    float a = 0.f;
#pragma unroll 4
    for (int b = k; b < nb; b += HYP_SLICES) a += part[((size_t)b * H + h) * HYP_D + lane];
    s_sum[k][lane] = a;
    __syncthreads();
    if (k == 0) {
        float v = s_sum[0][lane];
#pragma unroll
        for (int j = 1; j < HYP_SLICES; ++j) v += s_sum[j][lane];
        out[h * HYP_D + lane] = v;
    }
}

// ------------------------------------------------------------------------------------------------ expand, row pass
template <int H>
__device__ __forceinline__ float4 hyp_mix(const float* __restrict__ p, const float4 (&L)[H]) {
    float4 o = f4_scale(p[0], L[0]);
#pragma unroll
    for (int h = 1; h < H; ++h) o = f4_fma(p[h], L[h], o);
    return o;
}

// rows [0, I): X_out[r] = P_i[r] lat; rows [I, I + U): U_out[r - I] = P_u[r - I] lat (U = 0 where U_out is not wanted)
template <int H>
__global__ __launch_bounds__(HYP_BLOCK) void hyper_expand_kernel(
    const float* __restrict__ P_i, long I, float4* __restrict__ X_out, const float* __restrict__ P_u, long U,
    float4* __restrict__ U_out, const float4* __restrict__ lat4) {
    const int t = threadIdx.x % HYP_GROUP;
    float4 L[H];
#pragma unroll
    for (int h = 0; h < H; ++h) L[h] = lat4[h * HYP_GROUP + t];
    const long stride = (long)gridDim.x * HYP_GROUPS;
    for (long r = (long)blockIdx.x * HYP_GROUPS + threadIdx.x / HYP_GROUP; r < I + U; r += stride) {
        if (r < I)
            X_out[(size_t)r * HYP_GROUP + t] = hyp_mix<H>(P_i + (size_t)r * H, L);
        else
            U_out[(size_t)(r - I) * HYP_GROUP + t] = hyp_mix<H>(P_u + (size_t)(r - I) * H, L);
    }
}

__device__ __forceinline__ float hyp_dot_onto(float4 a, float4 b, float acc) {
    return fmaf(a.w, b.w, fmaf(a.z, b.z, fmaf(a.y, b.y, fmaf(a.x, b.x, acc))));
}

// rows [0, I): dP_i and dX_prev; rows [I, I + U): dP_u.  A NULL dX / dU reads as zeros, a NULL output is not written.
template <int H>
__global__ __launch_bounds__(HYP_BLOCK) void hyper_rows_bwd_kernel(
    const float* __restrict__ P_i, const float4* __restrict__ X4, const float4* __restrict__ dX4, long I,
    float* __restrict__ dP_i, float4* __restrict__ dXprev4, const float4* __restrict__ dU4, long U, float* __restrict__ dP_u,
    const float4* __restrict__ lat4, const float4* __restrict__ dlat4) {
    const int t = threadIdx.x % HYP_GROUP;
    float4 L[H], D[H];
#pragma unroll
    for (int h = 0; h < H; ++h) {
        L[h] = lat4[h * HYP_GROUP + t];
        D[h] = dlat4[h * HYP_GROUP + t];
    }
    const long stride = (long)gridDim.x * HYP_GROUPS;
    for (long r = (long)blockIdx.x * HYP_GROUPS + threadIdx.x / HYP_GROUP; r < I + U; r += stride) {
        if (r < I) {
            if (dP_i) {
                const float4 g = dX4 ? dX4[(size_t)r * HYP_GROUP + t] : f4_zero();
                const float4 x = X4[(size_t)r * HYP_GROUP + t];
                float mine = 0.f;
#pragma unroll
                for (int h = 0; h < H; ++h) {
                    const float v = row16_sum(hyp_dot_onto(x, D[h], hyp_dot_onto(g, L[h], 0.f)));
                    if (t == h) mine = v;
                }
                if (t < H) dP_i[(size_t)r * H + t] = mine;
            }
            if (dXprev4) dXprev4[(size_t)r * HYP_GROUP + t] = hyp_mix<H>(P_i + (size_t)r * H, D);
        } else if (dP_u) {
            const long ru = r - I;
            const float4 g = dU4 ? dU4[(size_t)ru * HYP_GROUP + t] : f4_zero();
            float mine = 0.f;
#pragma unroll
            for (int h = 0; h < H; ++h) {
                const float v = row16_sum(hyp_dot_onto(g, L[h], 0.f));
                if (t == h) mine = v;
            }
            if (t < H) dP_u[(size_t)ru * H + t] = mine;
        }
    }
}

// ------------------------------------------------------------------------------------------------ launches
inline int hyp_grid(long items, int per_block) {
    const long b = (items + per_block - 1) / per_block;
    return (int)(b < HYP_MAX_BLOCKS ? b : HYP_MAX_BLOCKS);
}

template <int H>
void hyp_launch_assign_fwd(hipStream_t s, const float* logits, const float* noise, const float* keep, long n, float tau, float q,
                           float* P, float* p_soft) {
    hipLaunchKernelGGL(hyper_assign_fwd_kernel<H>, dim3(hyp_grid(n, HYP_BLOCK)), dim3(HYP_BLOCK), 0, s, logits, noise, keep, n,
                       tau, q, P, p_soft);
}
template <int H>
void hyp_launch_assign_bwd(hipStream_t s, const float* p_soft, const float* keep, const float* dP, long n, float tau, float q,
                           float* dlogits) {
    hipLaunchKernelGGL(hyper_assign_bwd_kernel<H>, dim3(hyp_grid(n, HYP_BLOCK)), dim3(HYP_BLOCK), 0, s, p_soft, keep, dP, n, tau,
                       q, dlogits);
}
template <int H>
void hyp_launch_reduce(hipStream_t s, const float* P_a, const float* V_a, long n_a, const float* P_b, const float* V_b, long n_b,
                       float* part) {
    const int nb_a = hyp_blocks(n_a), nb_b = hyp_blocks(n_b);
    if (nb_a + nb_b == 0) return;
    hipLaunchKernelGGL(hyper_reduce_kernel<H>, dim3(nb_a + nb_b), dim3(HYP_BLOCK), 0, s, P_a, V_a, n_a, hyp_rows_per_block(n_a),
                       nb_a, P_b, V_b, n_b, hyp_rows_per_block(n_b), part);
}
template <int H>
void hyp_launch_expand(hipStream_t s, const float* P_i, long I, float* X_out, const float* P_u, long U, float* U_out,
                       const float* lat) {
    hipLaunchKernelGGL(hyper_expand_kernel<H>, dim3(hyp_grid(I + U, HYP_GROUPS)), dim3(HYP_BLOCK), 0, s, P_i, I,
                       reinterpret_cast<float4*>(X_out), P_u, U, reinterpret_cast<float4*>(U_out),
                       reinterpret_cast<const float4*>(lat));
}
template <int H>
void hyp_launch_rows_bwd(hipStream_t s, const float* P_i, const float* X, const float* dX, long I, float* dP_i, float* dX_prev,
                         const float* dU, long U, float* dP_u, const float* lat, const float* dlat) {
    hipLaunchKernelGGL(hyper_rows_bwd_kernel<H>, dim3(hyp_grid(I + U, HYP_GROUPS)), dim3(HYP_BLOCK), 0, s, P_i,
                       reinterpret_cast<const float4*>(X), reinterpret_cast<const float4*>(dX), I, dP_i,
                       reinterpret_cast<float4*>(dX_prev), reinterpret_cast<const float4*>(dU), U, dP_u,
                       reinterpret_cast<const float4*>(lat), reinterpret_cast<const float4*>(dlat));
}

#define HYP_SWITCH(H, FN, ...)            \
    switch (H) {                          \
        case 1: FN<1>(__VA_ARGS__); break; \
        case 2: FN<2>(__VA_ARGS__); break; \
        case 3: FN<3>(__VA_ARGS__); break; \
        case 4: FN<4>(__VA_ARGS__); break; \
        case 5: FN<5>(__VA_ARGS__); break; \
        case 6: FN<6>(__VA_ARGS__); break; \
        case 7: FN<7>(__VA_ARGS__); break; \
        default: FN<8>(__VA_ARGS__); break; \
    }

inline bool hyp_served(int32_t H, int32_t d) { return d == HYP_D && H >= 1 && H <= HYP_HMAX; }

}  // namespace

extern "C" int32_t mmrec_hyper_rows_per_block(int64_t n) { return n < 0 ? 0 : hyp_rows_per_block(n); }

extern "C" size_t mmrec_hyper_workspace_bytes(int64_t I, int64_t U, int32_t H) {
    if (I < 0 || U < 0 || I > HYP_MAX_ROWS || U > HYP_MAX_ROWS || H < 1 || H > HYP_HMAX) return 0;
    return sizeof(float) * ((size_t)HYP_HMAX * HYP_D + (size_t)(hyp_blocks(I) + hyp_blocks(U)) * H * HYP_D);
}

extern "C" int mmrec_hyper_assign_fwd_f32(const float* logits, const float* noise, const float* keep, int64_t n, int32_t H,
                                          float tau, float keep_rate, float* P, float* p_soft, mmrec_stream_t stream) {
    if (H < 1 || H > HYP_HMAX) return MMREC_ERR_UNSUPPORTED;
    if (n < 0) return MMREC_ERR_BAD_ARG;
    if (n > HYP_MAX_ROWS) return MMREC_ERR_UNSUPPORTED;
    if (n == 0) return 0;
    if (!logits || !noise || !P || P == p_soft) return MMREC_ERR_BAD_ARG;
    HYP_SWITCH(H, hyp_launch_assign_fwd, mmrec_stream(stream), logits, noise, keep, (long)n, tau, keep_rate, P, p_soft);
    MMREC_RETURN_LAUNCH_STATUS();
}

extern "C" int mmrec_hyper_assign_bwd_f32(const float* p_soft, const float* keep, const float* dP, int64_t n, int32_t H,
                                          float tau, float keep_rate, float* dlogits, mmrec_stream_t stream) {
    if (H < 1 || H > HYP_HMAX) return MMREC_ERR_UNSUPPORTED;
    if (n < 0) return MMREC_ERR_BAD_ARG;
    if (n > HYP_MAX_ROWS) return MMREC_ERR_UNSUPPORTED;
    if (n == 0) return 0;
    if (!p_soft || !dP || !dlogits) return MMREC_ERR_BAD_ARG;
    HYP_SWITCH(H, hyp_launch_assign_bwd, mmrec_stream(stream), p_soft, keep, dP, (long)n, tau, keep_rate, dlogits);
    MMREC_RETURN_LAUNCH_STATUS();
}

extern "C" int mmrec_hyper_layer_fwd_f32(const float* P_i, const float* P_u, const float* X_prev, int64_t I, int64_t U,
                                         int32_t H, int32_t d, float* U_out, float* X_out, float* lat, void* workspace,
                                         mmrec_stream_t stream) {
    if (!hyp_served(H, d)) return MMREC_ERR_UNSUPPORTED;
    if (I < 0 || U < 0) return MMREC_ERR_BAD_ARG;
    if (I > HYP_MAX_ROWS || U > HYP_MAX_ROWS) return MMREC_ERR_UNSUPPORTED;
    if (!lat || !workspace) return MMREC_ERR_BAD_ARG;
    if (I > 0 && (!P_i || !X_prev || !X_out)) return MMREC_ERR_BAD_ARG;
    if (U_out && U > 0 && !P_u) return MMREC_ERR_BAD_ARG;
    hipStream_t s = mmrec_stream(stream);
    float* part = static_cast<float*>(workspace) + HYP_HMAX * HYP_D;
    HYP_SWITCH(H, hyp_launch_reduce, s, P_i, X_prev, (long)I, nullptr, nullptr, 0L, part);
    hipLaunchKernelGGL(hyper_finish_kernel, dim3(H), dim3(HYP_SLICES * MMREC_WAVE), 0, s, part, hyp_blocks(I), (int)H, lat);
    const long rows_u = U_out ? (long)U : 0L;
    if (I + rows_u > 0) HYP_SWITCH(H, hyp_launch_expand, s, P_i, (long)I, X_out, P_u, rows_u, U_out, lat);
    MMREC_RETURN_LAUNCH_STATUS();
}

extern "C" int mmrec_hyper_layer_bwd_f32(const float* P_i, const float* P_u, const float* X_prev, const float* lat,
                                         const float* dU, const float* dX, int64_t I, int64_t U, int32_t H, int32_t d,
                                         float* dP_i, float* dP_u, float* dX_prev, void* workspace, mmrec_stream_t stream) {
    if (!hyp_served(H, d)) return MMREC_ERR_UNSUPPORTED;
    if (I < 0 || U < 0) return MMREC_ERR_BAD_ARG;
    if (I > HYP_MAX_ROWS || U > HYP_MAX_ROWS) return MMREC_ERR_UNSUPPORTED;
    if (!lat || !workspace) return MMREC_ERR_BAD_ARG;
    if (I > 0 && (!P_i || ((dP_i) && !X_prev))) return MMREC_ERR_BAD_ARG;
    if (U > 0 && dU && !P_u) return MMREC_ERR_BAD_ARG;
    hipStream_t s = mmrec_stream(stream);
    float* dlat = static_cast<float*>(workspace);
    float* part = dlat + HYP_HMAX * HYP_D;
    const long n_i = dX ? (long)I : 0L, n_u = dU ? (long)U : 0L;             // a NULL gradient adds no blocks: zeros
    HYP_SWITCH(H, hyp_launch_reduce, s, P_i, dX, n_i, P_u, dU, n_u, part);
    hipLaunchKernelGGL(hyper_finish_kernel, dim3(H), dim3(HYP_SLICES * MMREC_WAVE), 0, s, part, hyp_blocks(n_i) + hyp_blocks(n_u),
                       (int)H, dlat);
    const long rows_i = (dP_i || dX_prev) ? (long)I : 0L, rows_u = dP_u ? (long)U : 0L;
    if (rows_i + rows_u > 0)
        HYP_SWITCH(H, hyp_launch_rows_bwd, s, P_i, X_prev, dX, rows_i, dP_i, dX_prev, dU, rows_u, dP_u, lat, dlat);
    MMREC_RETURN_LAUNCH_STATUS();
}
