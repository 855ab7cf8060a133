// Row-wise log-sum-exp of scale * Q K^T against a whole table, and its gradients, without the [B, N] matrix:
//   lse[i] = log sum_{j<N} exp(scale <Q[i], K[j]>)                                   Q [B, d], K [N, d], d = 64 / 128
//   dQ[i]  = scale g[i] sum_j p_ij K[j],   dK[j] = scale sum_i g[i] p_ij Q[i],       p_ij = exp(scale s_ij - lse[i])
// (LGMRec's hypergraph contrastive term, lgmrec.py:157-164: the batch against EVERY user / item; PGL's two-view InfoNCE,
// pgl.py:226-231, at width 128.)  infonce.hip is the square, 64-wide, plain-FMA kernel of a B x B problem; a B x N sweep is
// 10-100 times that work and runs on the fp32-input MFMA.
//
// One kernel, three modes, all the sweep of mfma_sweep.h: a workgroup (4 waves) OWNS 128 rows of one operand, their fragments
// in registers, and walks a range of 64-row tiles of the OTHER operand, which reach the waves through LDS, de-interleaved:
//   s(other o, own i) = fma chain over k = 0 .. d-1 of other[o][k] * own[i][k]       (v_mfma_f32_32x32x2_f32, bitwise that chain)
// A lane holds 16 others of ONE own row: D[other = d_row(r, lane)][own = lane & 31].
//   MODE 0  own = Q, other = K: per lane a running (max, rescaled sum) over its 16 scores per sub-tile, the two lanes of a row
//           combined once at the end (h = 0 first), one (m, sum) per (column split, row); `sl_finish_kernel` combines the
//           splits in split order:  M = max m_s,  L = sum_s l_s exp(m_s - M),  lse = M + log L.
//   MODE 1  own = Q, other = K: w = exp(x - lse[own]) * scale g[own] -> dQ[own] += W K_tile      (lse, g: one per lane)
//   MODE 2  own = K, other = Q: w = exp(x - lse[oth]) * scale g[oth] -> dK[own] += W^T Q_tile    (lse, g: staged with the tile)
// The gradient products run on the same MFMA: W is re-laid-out through a per-wave 32 x 32 LDS tile ([own][other], pitch 33)
// into the A operand, the B operand is the tile already in LDS, the contraction runs over the tile's rows in order.
// Grid (own tiles x splits of the other operand): partial sums per split, added in split order by `sl_reduce_kernel` (one
// split: straight into the result).  No atomics; every sum has one fixed order, so two calls give the same bits.
#include "mfma_sweep.h"

namespace {

constexpr int SL_FWD_WGS = 512;        // workgroups the forward grid aims at (2 per CU)
constexpr int SL_BWD_WGS = 256;
constexpr int SL_FWD_SPLITS_MAX = 64;
constexpr int SL_BWD_SPLITS_MAX = 16;
constexpr int SL_ROWS_MAX = 1 << 30;   // row indices (+ a tile) stay in int32

inline SweepPlan sl_plan_fwd(long B, long N) { return sweep_plan(B, N, SL_FWD_WGS, SL_FWD_SPLITS_MAX); }
// backward: the partial results are [splits][n_own][d]; they never exceed 4 (B + N) d floats
inline SweepPlan sl_plan_bwd(long n_own, long n_oth) {
    long cap = n_own > 0 ? 4 * (n_own + n_oth) / n_own : 1;
    if (cap > SL_BWD_SPLITS_MAX) cap = SL_BWD_SPLITS_MAX;
    return sweep_plan(n_own, n_oth, SL_BWD_WGS, (int)cap);
}

__device__ __forceinline__ float sl_max16(const float (&a)[16]) {
    float m = a[0];
#pragma unroll
    for (int r = 1; r < 16; ++r) m = fmaxf(m, a[r]);
    return m;
}

template <int D, int MODE>
__global__ __launch_bounds__(256) void sl_sweep_kernel(const float* __restrict__ Own, int n_own,
                                                       const float* __restrict__ Oth, int n_oth, float scale,
                                                       int per, const float* __restrict__ lse,
                                                       const float* __restrict__ g, float* __restrict__ out0,
                                                       float* __restrict__ out1) {
    constexpr int LD = D + 4;           // tile pitch (mfma_sweep.h)
    constexpr int NC = D / 32;          // 32-column chunks of a gradient row
    __shared__ __attribute__((aligned(16))) float T[SWEEP_TILE * LD];
    __shared__ float P[MODE ? 4 : 1][MODE ? 32 * 33 : 1];
    __shared__ float Tl[MODE == 2 ? SWEEP_TILE : 1], Tg[MODE == 2 ? SWEEP_TILE : 1];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int i = lane & 31, h = lane >> 5;
    const int own0 = blockIdx.x * SWEEP_OWN + wave * 32;
    const int oth_tiles = (n_oth + SWEEP_TILE - 1) / SWEEP_TILE;
    const int t_begin = blockIdx.y * per, t_end = min(t_begin + per, oth_tiles);

    float qf[D / 2];                    // own[own0 + i][2 s + h]; rows past the end are zero
    sweep_own<D>(qf, Own + (size_t)(own0 + i < n_own ? own0 + i : 0) * D, own0 + i < n_own, h);
    float own_l = 0.f, own_g = 0.f;
    if (MODE == 1 && own0 + i < n_own) {
        own_l = lse[own0 + i];
        own_g = scale * g[own0 + i];
    }

    float4 pre[D / 16];
    float pre_l = 0.f, pre_g = 0.f;
    auto fetch = [&](int t) {
        const int o0 = t * SWEEP_TILE;
        sweep_fetch<D>(pre, Oth, o0, n_oth, tid);
        if (MODE == 2 && tid < SWEEP_TILE) {
            const bool ok = o0 + tid < n_oth;
            pre_l = ok ? lse[o0 + tid] : 0.f;
            pre_g = ok ? scale * g[o0 + tid] : 0.f;
        }
    };
    auto stage = [&]() {
        sweep_stage<D>(T, pre, tid);
        if (MODE == 2 && tid < SWEEP_TILE) { Tl[tid] = pre_l; Tg[tid] = pre_g; }
    };

    float m_run = -INFINITY, l_run = 0.f;          // MODE 0
    f32x16 dacc[NC];                               // MODE 1, 2: [own d_row(r, lane)][32 c + i]
#pragma unroll
    for (int c = 0; c < NC; ++c) dacc[c] = f32x16{0};

    if (t_begin < t_end) fetch(t_begin);
    for (int t = t_begin; t < t_end; ++t) {
        __syncthreads();                           // the previous tile is consumed
        stage();
        __syncthreads();
        if (t + 1 < t_end) fetch(t + 1);           // in flight under this tile's MFMAs
        const int o0 = t * SWEEP_TILE;
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            if (o0 + 32 * u >= n_oth) break;       // uniform: nothing but padding in this sub-tile
            const f32x16 acc = sweep_scores<D>(T, u, i, h, qf);
            const bool partial = o0 + 32 * u + 32 > n_oth;      // uniform
            float x[16];
#pragma unroll
            for (int r = 0; r < 16; ++r) x[r] = scale * acc[r];
            if (MODE == 0) {
                if (partial) {
#pragma unroll
                    for (int r = 0; r < 16; ++r) x[r] = o0 + 32 * u + d_row(r, lane) < n_oth ? x[r] : -INFINITY;
                }
                const float m_new = fmaxf(m_run, sl_max16(x));
                const float ms = m_new == -INFINITY ? 0.f : m_new;
                l_run *= expf(m_run - ms);                      // exp(0) = 1 while the maximum stands: no rounding
#pragma unroll
                for (int r = 0; r < 16; ++r) l_run += expf(x[r] - ms);
                m_run = m_new;
            } else {
                float* pw = P[wave];
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int oo = 32 * u + d_row(r, lane);
                    const float lv = MODE == 1 ? own_l : Tl[oo];
                    const float gv = MODE == 1 ? own_g : Tg[oo];
                    float w = expf(x[r] - lv) * gv;
                    if (partial) w = o0 + oo < n_oth ? w : 0.f;
                    pw[i * 33 + d_row(r, lane)] = w;            // [own][other]
                }
                wave_lds_order();                               // P is private to the wave
                // out[own i'][dim] += sum_c W[i'][c] tile[c][dim]: A = W[own = i][c = 2 s + h], B = tile[c = 2 s + h][32 nc + i]
                const int bpos = (i & 1) * (D / 2) + (i >> 1);  // mfma_sweep.h's position of column k = 32 nc + i: + 16 nc
#pragma unroll
                for (int s = 0; s < 16; ++s) {
                    const float a = pw[i * 33 + 2 * s + h];
                    const float* brow = T + (32 * u + 2 * s + h) * LD + bpos;
#pragma unroll
                    for (int c = 0; c < NC; ++c) dacc[c] = mfma32(a, brow[16 * c], dacc[c]);
                }
                wave_lds_order();
            }
        }
    }

    if (MODE == 0) {
        // the two lanes of a row, h = 0 first
        const float m_o = lane_xor_f<32>(m_run), l_o = lane_xor_f<32>(l_run);
        const float m0 = h ? m_o : m_run, l0 = h ? l_o : l_run, m1 = h ? m_run : m_o, l1 = h ? l_run : l_o;
        const float M = fmaxf(m0, m1), ms = M == -INFINITY ? 0.f : M;
        const float L = l0 * expf(m0 - ms) + l1 * expf(m1 - ms);
        if (h == 0 && own0 + i < n_own) {
            out0[(size_t)blockIdx.y * n_own + own0 + i] = M;
            out1[(size_t)blockIdx.y * n_own + own0 + i] = L;
        }
    } else {
        float* dst = out0 + (size_t)blockIdx.y * n_own * D;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = own0 + d_row(r, lane);
            if (row < n_own) {
#pragma unroll
                for (int c = 0; c < NC; ++c) dst[(size_t)row * D + 32 * c + i] = dacc[c][r];
            }
        }
    }
}

// lse[i] from the per-split (m, l), in split order; no split (N == 0): -inf
__global__ __launch_bounds__(256) void sl_finish_kernel(const float* __restrict__ pm, const float* __restrict__ pl,
                                                        int B, int splits, float* __restrict__ lse) {
    const int b = blockIdx.x * 256 + threadIdx.x;
    if (b >= B) return;
    float M = -INFINITY;
    for (int s = 0; s < splits; ++s) M = fmaxf(M, pm[(size_t)s * B + b]);
    const float ms = M == -INFINITY ? 0.f : M;
    float L = 0.f;
    for (int s = 0; s < splits; ++s) L += pl[(size_t)s * B + b] * expf(pm[(size_t)s * B + b] - ms);
    lse[b] = M + logf(L);
}

// out[e] = sum_s part[s][e] in split order (n4 float4 per split)
__global__ __launch_bounds__(256) void sl_reduce_kernel(const float4* __restrict__ part, size_t n4, int splits,
                                                        float4* __restrict__ out) {
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= n4) return;
    float4 a = part[e];
    for (int s = 1; s < splits; ++s) a = f4_add(a, part[(size_t)s * n4 + e]);
    out[e] = a;
}

inline size_t sl_bwd_floats(long n_own, long n_oth, int d) {
    if (n_own <= 0 || n_oth <= 0) return 0;
    const SweepPlan p = sl_plan_bwd(n_own, n_oth);
    return p.splits > 1 ? (size_t)p.splits * (size_t)n_own * d : 0;
}

template <int MODE>
inline void sl_launch(int d, dim3 grid, hipStream_t s, const float* own, int n_own, const float* oth, int n_oth,
                      float scale, int per, const float* lse, const float* g, float* o0, float* o1) {
    if (d == 64)
        hipLaunchKernelGGL((sl_sweep_kernel<64, MODE>), grid, dim3(256), 0, s, own, n_own, oth, n_oth, scale, per, lse, g, o0, o1);
    else
        hipLaunchKernelGGL((sl_sweep_kernel<128, MODE>), grid, dim3(256), 0, s, own, n_own, oth, n_oth, scale, per, lse, g, o0, o1);
}

// one gradient: own rows x splits of the other operand, then the splits in order
inline void sl_grad(int mode, const float* own, int n_own, const float* oth, int n_oth, int d, float scale,
                    const float* lse, const float* g, float* out, float* part, hipStream_t s) {
    const SweepPlan p = sl_plan_bwd(n_own, n_oth);
    float* dst = p.splits > 1 ? part : out;
    const dim3 grid(p.own_tiles, p.splits);
    if (mode == 1) sl_launch<1>(d, grid, s, own, n_own, oth, n_oth, scale, p.per, lse, g, dst, nullptr);
    else sl_launch<2>(d, grid, s, own, n_own, oth, n_oth, scale, p.per, lse, g, dst, nullptr);
    if (p.splits > 1) {
        const size_t n4 = (size_t)n_own * d / 4;
        hipLaunchKernelGGL(sl_reduce_kernel, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, s,
                           reinterpret_cast<const float4*>(part), n4, p.splits, reinterpret_cast<float4*>(out));
    }
}

}  // namespace

// rows of the walked operand per split: mode 0 the forward (columns of K), 1 the dQ sweep (columns of K), 2 the dK sweep (rows of Q)
extern "C" int32_t mmrec_score_lse_split_cols(int32_t B, int32_t N, int32_t mode) {
    if (B < 0 || N < 0 || mode < 0 || mode > 2) return 0;
    if ((mode == 2 ? B : N) == 0) return 0;
    const SweepPlan p = mode == 0 ? sl_plan_fwd(B, N) : mode == 1 ? sl_plan_bwd(B, N) : sl_plan_bwd(N, B);
    return p.per * SWEEP_TILE;
}

extern "C" size_t mmrec_score_lse_workspace_bytes(int32_t B, int32_t N, int32_t d) {
    if (B <= 0 || N < 0 || (d != 64 && d != 128)) return 0;
    const size_t fwd = N > 0 ? (size_t)2 * sl_plan_fwd(B, N).splits * (size_t)B : 0;
    const size_t bwd = sl_bwd_floats(B, N, d) + sl_bwd_floats(N, B, d);
    return (fwd > bwd ? fwd : bwd) * sizeof(float);
}

extern "C" int mmrec_score_lse_f32(const float* Q, const float* K, int32_t B, int32_t N, int32_t d, float scale,
                                   float* lse, void* workspace, mmrec_stream_t stream) {
    if ((d != 64 && d != 128) || B < 0 || N < 0) return MMREC_ERR_BAD_ARG;
    if (B > SL_ROWS_MAX || N > SL_ROWS_MAX) return MMREC_ERR_UNSUPPORTED;
    if (B == 0) return 0;
    if (!lse || (N > 0 && (!Q || !K || !workspace))) return MMREC_ERR_BAD_ARG;
    hipStream_t s = mmrec_stream(stream);
    int splits = 0;
    float* pm = static_cast<float*>(workspace);
    float* pl = pm;
    if (N > 0) {
        const SweepPlan p = sl_plan_fwd(B, N);
        splits = p.splits;
        pl = pm + (size_t)splits * B;
        sl_launch<0>(d, dim3(p.own_tiles, p.splits), s, Q, B, K, N, scale, p.per, nullptr, nullptr, pm, pl);
    }
    hipLaunchKernelGGL(sl_finish_kernel, dim3((B + 255) / 256), dim3(256), 0, s, pm, pl, B, splits, lse);
    MMREC_RETURN_LAUNCH_STATUS();
}

extern "C" int mmrec_score_lse_bwd_f32(const float* Q, const float* K, int32_t B, int32_t N, int32_t d, float scale,
                                       const float* lse, const float* g, float* dQ, float* dK, void* workspace,
                                       mmrec_stream_t stream) {
    if ((d != 64 && d != 128) || B < 0 || N < 0) return MMREC_ERR_BAD_ARG;
    if (B > SL_ROWS_MAX || N > SL_ROWS_MAX) return MMREC_ERR_UNSUPPORTED;
    if (B == 0 && N == 0) return 0;
    if ((B > 0 && !dQ && !dK) || (B > 0 && N > 0 && (!Q || !K || !lse || !g))) return MMREC_ERR_BAD_ARG;
    hipStream_t s = mmrec_stream(stream);
    if (B == 0 || N == 0) {             // no pair: zero gradients
        if (dQ && B > 0) hipMemsetAsync(dQ, 0, (size_t)B * d * sizeof(float), s);
        if (dK && N > 0) hipMemsetAsync(dK, 0, (size_t)N * d * sizeof(float), s);
        MMREC_RETURN_LAUNCH_STATUS();
    }
    const size_t fq = sl_bwd_floats(B, N, d), fk = sl_bwd_floats(N, B, d);
    if ((fq && dQ && !workspace) || (fk && dK && !workspace)) return MMREC_ERR_BAD_ARG;
    float* part_q = static_cast<float*>(workspace);
    float* part_k = part_q ? part_q + fq : nullptr;
    if (dQ) sl_grad(1, Q, B, K, N, d, scale, lse, g, dQ, part_q, s);
    if (dK) sl_grad(2, K, N, Q, B, d, scale, lse, g, dK, part_k, s);
    MMREC_RETURN_LAUNCH_STATUS();
}
