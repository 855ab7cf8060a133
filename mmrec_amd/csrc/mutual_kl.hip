// DAMRS's symmetric KL term between two views of the same user-item probabilities (damrs.py: kl = mean(_kl(p_g, p_m) +
// _kl(p_m, p_g)), p_g = sigmoid(U A^T), p_m = sigmoid(U B^T)) without the [m, n] blocks.  The sum of the two divergences of two
// Bernoulli variables collapses:  with a = <U[r], A[i]>, b = <U[r], B[i]>, p = sigmoid(a), q = sigmoid(b)
//   KL(p || q) + KL(q || p) = (p - q)(logit p - logit q) = (sigmoid(a) - sigmoid(b)) (a - b)  =: J(a, b)
// no logarithm, two exponentials a pair, finite for every finite a and b (the composition is 0 * log 0 = NaN once a sigmoid
// saturates in fp32).
//   out   = scale * sum_{r < m, i < n} J(a_ri, b_ri)                       U [m, 64], A, B [n, 64]; scale = 1 / (m n), the caller's
//   ga_ri = g scale [s'(a)(a - b) + (p - q)],  gb_ri = -g scale [s'(b)(a - b) + (p - q)]           s'(x) = sigmoid(x)(1 - sigmoid(x))
//   dU = Ga A + Gb B,   dA = Ga^T U,   dB = Gb^T U
// All three kernels are the sweep of mfma_sweep.h (as score_lse.hip): a workgroup (4 waves) OWNS 128 rows, their fragments in
// registers, and walks a range of 64-row tiles of the other side through LDS; a score is the fma chain over k = 0 .. 63 of
// other[o][k] * own[i][k] (v_mfma_f32_32x32x2_f32), the same bits in the forward and in both backward sweeps.
//   mk_fwd_kernel      own = U, the tiles of A and B staged together: both scores of a pair from the same walk, J added per lane
//                      in the lane's order (r, sub-tile, tile), the wave's lanes by a butterfly, the four waves in order: one
//                      partial per workgroup;  mk_finish_kernel adds the partials in a fixed tree and multiplies by scale.
//   mk_bwd_kernel<1>   own = U, walks A and B: dU[own] += Ga A_tile, then += Gb B_tile, per 32-row sub-tile
//   mk_bwd_kernel<2>   own = the item rows of A AND B, walks U: dA[own] += Ga^T U_tile, dB[own] += Gb^T U_tile
// The gradient products run on the same MFMA through a per-wave 32 x 32 LDS tile (score_lse.hip's re-layout).  Grid (own tiles x
// splits of the walked side); per-split partial gradients are added in split order by mk_reduce_kernel.  Rows past the end are
// zero rows: J(0, 0) = 0 and both coefficients are 0 exactly, so no edge needs a mask.  No atomics, every order fixed by (m, n)
// alone: the same bits on every call, and the plan is capturable.
#include "mfma_sweep.h"

namespace {

constexpr int MK_LD = 64 + 4;          // tile pitch (mfma_sweep.h)
constexpr int MK_FWD_WGS = 512;        // workgroups the forward grid aims at (2 per CU)
constexpr int MK_BWD_WGS = 256;
constexpr int MK_FWD_SPLITS_MAX = 64;
constexpr int MK_BWD_SPLITS_MAX = 16;
constexpr int MK_ROWS_MAX = 1 << 30;   // row indices (+ a tile) stay in int32

inline SweepPlan mk_plan_fwd(long m, long n) { return sweep_plan(m, n, MK_FWD_WGS, MK_FWD_SPLITS_MAX); }
// backward: the partial results are [splits][n_own][64]; they never exceed 4 (m + n) 64 floats per gradient
inline SweepPlan mk_plan_bwd(long n_own, long n_oth) {
    long cap = n_own > 0 ? 4 * (n_own + n_oth) / n_own : 1;
    if (cap > MK_BWD_SPLITS_MAX) cap = MK_BWD_SPLITS_MAX;
    return sweep_plan(n_own, n_oth, MK_BWD_WGS, (int)cap);
}

__device__ __forceinline__ float mk_j(float a, float b) { return (stable_sigmoid(a) - stable_sigmoid(b)) * (a - b); }

// the two coefficients of a pair; gs = g * scale
__device__ __forceinline__ void mk_coef(float a, float b, float gs, float& ga, float& gb) {
    const float p = stable_sigmoid(a), q = stable_sigmoid(b);
    const float d = a - b, pq = p - q;
    ga = gs * (p * (1.f - p) * d + pq);
    gb = -gs * (q * (1.f - q) * d + pq);
}

__global__ __launch_bounds__(256) void mk_fwd_kernel(const float* __restrict__ U, int m, const float* __restrict__ A,
                                                     const float* __restrict__ B, int n, int per, float* __restrict__ part) {
    __shared__ __attribute__((aligned(16))) float TA[SWEEP_TILE * MK_LD], TB[SWEEP_TILE * MK_LD];
    __shared__ float wsum[4];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int i = lane & 31, h = lane >> 5;
    const int own0 = blockIdx.x * SWEEP_OWN + wave * 32;
    const int oth_tiles = (n + SWEEP_TILE - 1) / SWEEP_TILE;
    const int t_begin = blockIdx.y * per, t_end = min(t_begin + per, oth_tiles);

    float uf[32];                       // U[own0 + i][2 s + h]; rows past the end are zero
    sweep_own<64>(uf, U + (size_t)(own0 + i < m ? own0 + i : 0) * 64, own0 + i < m, h);

    float4 pa[4], pb[4];
    auto fetch = [&](int t) {
        sweep_fetch<64>(pa, A, t * SWEEP_TILE, n, tid);
        sweep_fetch<64>(pb, B, t * SWEEP_TILE, n, tid);
    };
    float jsum = 0.f;
    if (t_begin < t_end) fetch(t_begin);
    for (int t = t_begin; t < t_end; ++t) {
        __syncthreads();                           // the previous tiles are consumed
        sweep_stage<64>(TA, pa, tid);
        sweep_stage<64>(TB, pb, tid);
        __syncthreads();
        if (t + 1 < t_end) fetch(t + 1);           // in flight under this tile's MFMAs
        const int o0 = t * SWEEP_TILE;
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            if (o0 + 32 * u >= n) break;           // uniform: nothing but padding in this sub-tile
            const f32x16 sa = sweep_scores<64>(TA, u, i, h, uf);
            const f32x16 sb = sweep_scores<64>(TB, u, i, h, uf);
#pragma unroll
            for (int r = 0; r < 16; ++r) jsum += mk_j(sa[r], sb[r]);       // a padding row: J(0, 0) = 0
        }
    }
    jsum = wave_sum(jsum);
    if (lane == 0) wsum[wave] = jsum;
    __syncthreads();
    if (tid == 0) part[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = ((wsum[0] + wsum[1]) + wsum[2]) + wsum[3];
}

// out = scale * the sum of the partials in a fixed tree: thread t adds the partials t, t + 256, ... in order, the wave's 64
// lanes by a butterfly, the four waves in order
__global__ __launch_bounds__(256) void mk_finish_kernel(const float* __restrict__ part, size_t n_part, float scale,
                                                        float* __restrict__ out) {
    __shared__ float wsum[4];
    const int tid = threadIdx.x;
    float sum = 0.f;
    for (size_t e = tid; e < n_part; e += 256) sum += part[e];
    sum = wave_sum(sum);
    if ((tid & 63) == 0) wsum[tid >> 6] = sum;
    __syncthreads();
    if (tid == 0) out[0] = scale * (((wsum[0] + wsum[1]) + wsum[2]) + wsum[3]);
}

// acc[own d_row(r, lane)][32 c + i] += sum over the sub-tile's 32 rows o of w(own, o) T[o][32 c + i]: the lane's sixteen
// w(own = i, other = d_row(r, lane)) go through the wave's private tile P ([own][other], pitch 33) into the A operand, the B
// operand is the tile already in LDS, the contraction runs over the sub-tile's rows in order (score_lse.hip)
__device__ __forceinline__ void mk_outer(float* __restrict__ pw, const float* __restrict__ T, int u, int i, int h, int lane,
                                         const float (&w)[16], f32x16 (&acc)[2]) {
#pragma unroll
    for (int r = 0; r < 16; ++r) pw[i * 33 + d_row(r, lane)] = w[r];
    wave_lds_order();                              // P is private to the wave
    const int bpos = (i & 1) * 32 + (i >> 1);      // mfma_sweep.h's position of column k = 32 c + i: + 16 c
#pragma unroll
    for (int s = 0; s < 16; ++s) {
        const float a = pw[i * 33 + 2 * s + h];
        const float* brow = T + (32 * u + 2 * s + h) * MK_LD + bpos;
        acc[0] = mfma32(a, brow[0], acc[0]);
        acc[1] = mfma32(a, brow[16], acc[1]);
    }
    wave_lds_order();
}

__device__ __forceinline__ void mk_store(float* __restrict__ dst, int own0, int n_own, int i, int lane, const f32x16 (&acc)[2]) {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int row = own0 + d_row(r, lane);
        if (row < n_own) {
            dst[(size_t)row * 64 + i] = acc[0][r];
            dst[(size_t)row * 64 + 32 + i] = acc[1][r];
        }
    }
}

// MODE 1: own = U (n_own = m), Oa = A, Ob = B (n_oth = n), out0 = dU (or its partials).
// MODE 2: own = A and B (n_own = n), Oa = U (n_oth = m), out0 = dA, out1 = dB (or their partials; NULL: not wanted).
template <int MODE>
__global__ __launch_bounds__(256) void mk_bwd_kernel(const float* __restrict__ OwnA, const float* __restrict__ OwnB, int n_own,
                                                     const float* __restrict__ Oa, const float* __restrict__ Ob, int n_oth,
                                                     int per, const float* __restrict__ g, float scale,
                                                     float* __restrict__ out0, float* __restrict__ out1) {
    __shared__ __attribute__((aligned(16))) float Ta[SWEEP_TILE * MK_LD];
    __shared__ __attribute__((aligned(16))) float Tb[MODE == 1 ? SWEEP_TILE * MK_LD : 4];
    __shared__ float P[4][32 * 33];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int i = lane & 31, h = lane >> 5;
    const int own0 = blockIdx.x * SWEEP_OWN + wave * 32;
    const int oth_tiles = (n_oth + SWEEP_TILE - 1) / SWEEP_TILE;
    const int t_begin = blockIdx.y * per, t_end = min(t_begin + per, oth_tiles);
    const float gs = g[0] * scale;
    const bool want0 = out0 != nullptr, want1 = MODE == 2 && out1 != nullptr;      // uniform

    const bool present = own0 + i < n_own;
    const size_t own_off = (size_t)(present ? own0 + i : 0) * 64;
    float fa[32], fb[32];                // (MODE 1 never touches fb, MODE 2 never pb)
    sweep_own<64>(fa, OwnA + own_off, present, h);
    if (MODE == 2) sweep_own<64>(fb, OwnB + own_off, present, h);

    float4 pa[4], pb[4];
    auto fetch = [&](int t) {
        sweep_fetch<64>(pa, Oa, t * SWEEP_TILE, n_oth, tid);
        if (MODE == 1) sweep_fetch<64>(pb, Ob, t * SWEEP_TILE, n_oth, tid);
    };
    f32x16 acc0[2] = {{0}, {0}}, acc1[2] = {{0}, {0}};
    float* pw = P[wave];

    if (t_begin < t_end) fetch(t_begin);
    for (int t = t_begin; t < t_end; ++t) {
        __syncthreads();                           // the previous tiles are consumed
        sweep_stage<64>(Ta, pa, tid);
        if (MODE == 1) sweep_stage<64>(Tb, pb, tid);
        __syncthreads();
        if (t + 1 < t_end) fetch(t + 1);           // in flight under this tile's MFMAs
        const int o0 = t * SWEEP_TILE;
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            if (o0 + 32 * u >= n_oth) break;       // uniform: nothing but padding in this sub-tile
            // a = <U, A>, b = <U, B>: the forward's chains (the products commute)
            const f32x16 sa = sweep_scores<64>(Ta, u, i, h, fa);
            const f32x16 sb = MODE == 1 ? sweep_scores<64>(Tb, u, i, h, fa) : sweep_scores<64>(Ta, u, i, h, fb);
            float wa[16], wb[16];
#pragma unroll
            for (int r = 0; r < 16; ++r) mk_coef(sa[r], sb[r], gs, wa[r], wb[r]);   // a padding row: both 0
            if (MODE == 1) {
                mk_outer(pw, Ta, u, i, h, lane, wa, acc0);
                mk_outer(pw, Tb, u, i, h, lane, wb, acc0);
            } else {
                if (want0) mk_outer(pw, Ta, u, i, h, lane, wa, acc0);
                if (want1) mk_outer(pw, Ta, u, i, h, lane, wb, acc1);
            }
        }
    }
    const size_t split_off = (size_t)blockIdx.y * (size_t)n_own * 64;
    if (want0) mk_store(out0 + split_off, own0, n_own, i, lane, acc0);
    if (want1) mk_store(out1 + split_off, own0, n_own, i, lane, acc1);
}

// out[e] = sum_s part[s][e] in split order (n4 float4 per split)
__global__ __launch_bounds__(256) void mk_reduce_kernel(const float4* __restrict__ part, size_t n4, int splits,
                                                        float4* __restrict__ out) {
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= n4) return;
    float4 a = part[e];
    for (int s = 1; s < splits; ++s) a = f4_add(a, part[(size_t)s * n4 + e]);
    out[e] = a;
}

inline size_t mk_bwd_floats(long n_own, long n_oth) {
    if (n_own <= 0 || n_oth <= 0) return 0;
    const SweepPlan p = mk_plan_bwd(n_own, n_oth);
    return p.splits > 1 ? (size_t)p.splits * (size_t)n_own * 64 : 0;
}

inline void mk_reduce(const float* part, float* out, int n_own, int splits, hipStream_t s) {
    const size_t n4 = (size_t)n_own * 16;
    hipLaunchKernelGGL(mk_reduce_kernel, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, s,
                       reinterpret_cast<const float4*>(part), n4, splits, reinterpret_cast<float4*>(out));
}

inline bool mk_shape_ok(int32_t m, int32_t n, int32_t d) { return d == 64 && m >= 0 && n >= 0; }

}  // namespace

// rows of the walked side per split: mode 0 the forward (rows of A and B), 1 the dU sweep (rows of A and B), 2 the dA / dB sweep
// (rows of U).  A function of (m, n) alone; 0 where there is no pair.
extern "C" int32_t mmrec_mutual_kl_split_cols(int32_t m, int32_t n, int32_t mode) {
    if (m <= 0 || n <= 0 || mode < 0 || mode > 2) return 0;
    const SweepPlan p = mode == 0 ? mk_plan_fwd(m, n) : mode == 1 ? mk_plan_bwd(m, n) : mk_plan_bwd(n, m);
    return p.per * SWEEP_TILE;
}

extern "C" size_t mmrec_mutual_kl_workspace_bytes(int32_t m, int32_t n, int32_t d) {
    if (m <= 0 || n <= 0 || d != 64) return 0;
    const SweepPlan p = mk_plan_fwd(m, n);
    const size_t fwd = (size_t)p.own_tiles * (size_t)p.splits;
    const size_t bwd = mk_bwd_floats(m, n) + 2 * mk_bwd_floats(n, m);
    return (fwd > bwd ? fwd : bwd) * sizeof(float);
}

extern "C" int mmrec_mutual_kl_f32(const float* U, const float* A, const float* B, int32_t m, int32_t n, int32_t d, float scale,
                                   float* out, void* workspace, mmrec_stream_t stream) {
    if (!mk_shape_ok(m, n, d)) return MMREC_ERR_BAD_ARG;
    if (m > MK_ROWS_MAX || n > MK_ROWS_MAX) return MMREC_ERR_UNSUPPORTED;
    if (!out) return MMREC_ERR_BAD_ARG;
    hipStream_t s = mmrec_stream(stream);
    if (m == 0 || n == 0) {             // no pair: the empty sum
        (void)hipMemsetAsync(out, 0, sizeof(float), s);
        MMREC_RETURN_LAUNCH_STATUS();
    }
    if (!U || !A || !B || !workspace) return MMREC_ERR_BAD_ARG;
    const SweepPlan p = mk_plan_fwd(m, n);
    float* part = static_cast<float*>(workspace);
    hipLaunchKernelGGL(mk_fwd_kernel, dim3(p.own_tiles, p.splits), dim3(256), 0, s, U, m, A, B, n, p.per, part);
    hipLaunchKernelGGL(mk_finish_kernel, dim3(1), dim3(256), 0, s, part, (size_t)p.own_tiles * (size_t)p.splits, scale, out);
    MMREC_RETURN_LAUNCH_STATUS();
}

extern "C" int mmrec_mutual_kl_bwd_f32(const float* U, const float* A, const float* B, int32_t m, int32_t n, int32_t d,
                                       float scale, const float* g, float* dU, float* dA, float* dB, void* workspace,
                                       mmrec_stream_t stream) {
    if (!mk_shape_ok(m, n, d)) return MMREC_ERR_BAD_ARG;
    if (m > MK_ROWS_MAX || n > MK_ROWS_MAX) return MMREC_ERR_UNSUPPORTED;
    if (m == 0 && n == 0) return 0;
    if (!dU && !dA && !dB) return MMREC_ERR_BAD_ARG;
    hipStream_t s = mmrec_stream(stream);
    if (m == 0 || n == 0) {             // no pair: zero gradients
        if (dU && m > 0) (void)hipMemsetAsync(dU, 0, (size_t)m * 64 * sizeof(float), s);
        if (dA && n > 0) (void)hipMemsetAsync(dA, 0, (size_t)n * 64 * sizeof(float), s);
        if (dB && n > 0) (void)hipMemsetAsync(dB, 0, (size_t)n * 64 * sizeof(float), s);
        MMREC_RETURN_LAUNCH_STATUS();
    }
    if (!U || !A || !B || !g) return MMREC_ERR_BAD_ARG;
    const size_t fu = mk_bwd_floats(m, n), fi = mk_bwd_floats(n, m);
    if (!workspace && ((fu && dU) || (fi && (dA || dB)))) return MMREC_ERR_BAD_ARG;
    float* part_u = static_cast<float*>(workspace);
    if (dU) {                           // own = U, walks A and B
        const SweepPlan p = mk_plan_bwd(m, n);
        hipLaunchKernelGGL(mk_bwd_kernel<1>, dim3(p.own_tiles, p.splits), dim3(256), 0, s, U, (const float*)nullptr, m, A, B, n,
                           p.per, g, scale, p.splits > 1 ? part_u : dU, (float*)nullptr);
        if (p.splits > 1) mk_reduce(part_u, dU, m, p.splits, s);
    }
    if (dA || dB) {                     // own = the item rows of A and B together, walks U
        const SweepPlan p = mk_plan_bwd(n, m);
        float* part_a = part_u ? part_u + fu : nullptr;
        float* part_b = part_a ? part_a + fi : nullptr;
        const bool split = p.splits > 1;
        hipLaunchKernelGGL(mk_bwd_kernel<2>, dim3(p.own_tiles, p.splits), dim3(256), 0, s, A, B, n, U, (const float*)nullptr, m,
                           p.per, g, scale, dA ? (split ? part_a : dA) : (float*)nullptr,
                           dB ? (split ? part_b : dB) : (float*)nullptr);
        if (split && dA) mk_reduce(part_a, dA, n, p.splits, s);
        if (split && dB) mk_reduce(part_b, dB, n, p.splits, s);
    }
    MMREC_RETURN_LAUNCH_STATUS();
}
