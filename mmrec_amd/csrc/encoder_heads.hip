// MVGAE's mean / log-variance heads (include/mmrec_hip.h, additive to ABI 16): everything mvgae.py's GCN.forward does after the
// trunk, given AX = spmm(graph, x) once for all heads -- H heads over all n = users + items rows in ONE launch, and the backward
// in two (the main pass + the weight gradients' finish).  fp32 throughout, VALU fma (tile64.h), one head's three matrices in LDS.
//
// Per head h and row (W_h [64][64] as [in][out]; G_h, L_h [64][64] as [out][in]; scale_h the dropout mask / keep rate or NULL):
//     a = AX W_h + b_h, nrm = max(||a||, 1e-12), u = a / nrm, d = u scale_h, hh = leaky(d)
//     p = X L_h^T + bl_h                                          out_h = hh G_h^T + bg_h + leaky(p)
//
// THE PLAN (what the fuzz's error bound counts) is tile64.h's: blocks of R = mmrec_encoder_heads_rows_per_block(n) rows, stage,
// weight partials, column sums, finish.  The HEAD LOOP IS OUTERMOST: W_h, G_h, L_h are staged in LDS as they lie in memory
// (68-float rows), the block's tiles are walked, then the next head.  This op's own:
//   stage   a: over the input column from b;  p: from bl;  out: over hh's column from bg, then ONE addition of leaky(p).
//   norm    the thread's columns c = 4 sg .. 4 sg + 3: ss = fma(a_c, a_c, ss) from 0 in this order, then the butterfly over the 16
//           lanes of the row (xor 8, 4, 2, 1); raw = sqrtf(ss), nrm = fmaxf(raw, 1e-12f), u = a / nrm, d = u * scale (scale NULL:
//           d = u), leaky(z) = z > 0 ? z : slope * z.
// Backward from g [H, n, 64], everything RECOMPUTED as above (state between the calls: the operands and scale), then per head
//   dhh = the stage of g G_h over the output column from 0;  du = (dhh * (d > 0 ? 1 : slope)) * scale (scale NULL: no second product);
//   dot = fma(u_c, du_c, dot) over the thread's columns from 0, then the same butterfly;
//   da = (raw >= 1e-12f ? fma(-u, dot, du) : du) / nrm;                dp = g * (p > 0 ? 1 : slope);
//   dAX = the stage of da W_h^T over the output column, started at 0 for head 0 and at the rows' dAX after head h - 1 for head h:
//   one chain of 64 H terms, the heads in order;  dX = the stage of dp L_h over the output column, started and continued alike.
//   dW_h[k][o] = one fma chain over the block's rows in order (AX^T da), dG_h[o][k] alike (g^T hh), dL_h[o][k] alike (dp^T X).
//   The column sums: db_h (da), dbg_h (g), dbl_h (dp).
// Every order is fixed by n and H alone.  The scale of a row past n is never read.  The rows of dAX / dX that a later head adds
// onto were stored by the SAME thread.
// Workspace: per block and head 3 (64 64 + 64) = 12,480 floats: [dW][dG][dL][db][dbg][dbl].
// LDS: 3 matrices + 3 tiles (forward) or + 6 tiles (backward) of 17,408 B, + 768 B of biases: 105,216 B and 157,440 B.
#include "tile64.h"

namespace {

constexpr int EH_D = 64;
constexpr int EH_MAX_HEADS = 4;
constexpr int EH_W = EH_D * EH_D;
constexpr int EH_PART = 3 * (EH_W + EH_D);                  // floats of one block's partial of one head
constexpr int EH_VEC = 3 * EH_D;                            // b, bg, bl in LDS
constexpr int EH_FWD_TILES = 3, EH_BWD_TILES = 6;
constexpr float EH_EPS = 1e-12f;

constexpr size_t eh_lds_bytes(int tiles) { return sizeof(float) * ((size_t)(3 + tiles) * T64_FLOATS + EH_VEC); }

// head h's three matrices and three biases into LDS (visible after the caller's next barrier)
__device__ __forceinline__ void eh_setup(float* __restrict__ LW, float* __restrict__ LG, float* __restrict__ LL,
                                         float* __restrict__ vec, const float* __restrict__ W, const float* __restrict__ b,
                                         const float* __restrict__ G, const float* __restrict__ bg, const float* __restrict__ L,
                                         const float* __restrict__ bl, int h) {
    t64_matrix(LW, W + (size_t)h * EH_W);
    t64_matrix(LG, G + (size_t)h * EH_W);
    t64_matrix(LL, L + (size_t)h * EH_W);
    if (threadIdx.x < EH_VEC) {
        const int c = threadIdx.x % EH_D;
        const float* __restrict__ src = threadIdx.x < EH_D ? b : threadIdx.x < 2 * EH_D ? bg : bl;
        vec[threadIdx.x] = src[h * EH_D + c];
    }
}

// the normalised convolution of the thread's rows at its columns 4 sg + j (layout L0), from the transposed AX tile
struct EhRows {
    float u[4][4], d[4][4], sc[4][4];
    float nrm[4], raw[4];
};

__device__ __forceinline__ void eh_recompute(const float* __restrict__ At, const float* __restrict__ LW,
                                             const float* __restrict__ vec, const float* __restrict__ scale, long row0, long n,
                                             int rg, int sg, EhRows& f) {
    float4 a[4];
    t64_start0(a, vec, sg);
    t64_stage_nn(At, LW, rg, sg, a);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const long r = row0 + 4 * rg + i;
        const float av[4] = {a[i].x, a[i].y, a[i].z, a[i].w};
        float4 s4 = make_float4(1.f, 1.f, 1.f, 1.f);
        if (scale && r < n) s4 = *reinterpret_cast<const float4*>(scale + (size_t)r * EH_D + 4 * sg);
        f.sc[i][0] = s4.x, f.sc[i][1] = s4.y, f.sc[i][2] = s4.z, f.sc[i][3] = s4.w;
        float ss = 0.f;
#pragma unroll
        for (int j = 0; j < 4; ++j) ss = fmaf(av[j], av[j], ss);
        f.raw[i] = sqrtf(row16_sum(ss));
        f.nrm[i] = fmaxf(f.raw[i], EH_EPS);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            f.u[i][j] = av[j] / f.nrm[i];
            f.d[i][j] = scale ? f.u[i][j] * f.sc[i][j] : f.u[i][j];
        }
    }
}

__global__ __launch_bounds__(T64_BLOCK) void encoder_heads_fwd_kernel(
    const float* __restrict__ AX, const float* __restrict__ X, const float* __restrict__ W, const float* __restrict__ b,
    const float* __restrict__ G, const float* __restrict__ bg, const float* __restrict__ L, const float* __restrict__ bl,
    const float* __restrict__ scale, long n, int tiles, int H, float slope, float* __restrict__ out) {
    extern __shared__ float4 s_eh[];
    float* LW = reinterpret_cast<float*>(s_eh);
    float* LG = LW + T64_FLOATS;
    float* LL = LG + T64_FLOATS;
    float* vec = LL + T64_FLOATS;
    float* At = vec + EH_VEC;                // AX transposed
    float* Xr = At + T64_FLOATS;
    float* Hr = Xr + T64_FLOATS;             // hh row-major
    const int rg = threadIdx.x / 16, sg = threadIdx.x % 16;
    for (int h = 0; h < H; ++h) {
        if (h) __syncthreads();              // every read of the previous head's matrices is done
        eh_setup(LW, LG, LL, vec, W, b, G, bg, L, bl, h);
        const float* __restrict__ scale_h = scale ? scale + (size_t)h * n * EH_D : nullptr;
        float* __restrict__ out_h = out + (size_t)h * n * EH_D;
        for (int t = 0; t < tiles; ++t) {
            const long row0 = t64_row0(t, tiles);
            if (row0 >= n) break;
            float4 v[4];
            t64_rows(v, AX, row0, n, rg, sg);
            t64_put_t(At, rg, sg, v);
            t64_load(Xr, X, row0, n, rg, sg);
            __syncthreads();
            EhRows f;
            eh_recompute(At, LW, vec, scale_h, row0, n, rg, sg, f);
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) f.d[i][j] = t64_leaky(f.d[i][j], slope);
            t64_put0(Hr, rg, sg, f.d);
            __syncthreads();
            float o[4][4], p[4][4];
            t64_start1(o, vec + EH_D, sg);
            t64_start1(p, vec + 2 * EH_D, sg);
            t64_stage_nt(Hr, LG, rg, sg, o);
            t64_stage_nt(Xr, LL, rg, sg, p);
#pragma unroll
            for (int i = 0; i < 4; ++i) {                                    // not t64_store1: the sum is formed in the guard
                const long r = row0 + 4 * rg + i;
                if (r < n) {
#pragma unroll
                    for (int j = 0; j < 4; ++j) out_h[(size_t)r * EH_D + sg + 16 * j] = o[i][j] + t64_leaky(p[i][j], slope);
                }
            }
            __syncthreads();
        }
    }
}

__global__ __launch_bounds__(T64_BLOCK) void encoder_heads_bwd_kernel(
    const float* __restrict__ AX, const float* __restrict__ X, const float* __restrict__ W, const float* __restrict__ b,
    const float* __restrict__ G, const float* __restrict__ bg, const float* __restrict__ L, const float* __restrict__ bl,
    const float* __restrict__ scale, const float* __restrict__ g, long n, int tiles, int H, float slope, float* dAX, float* dX,
    float* __restrict__ part) {
    extern __shared__ float4 s_eh[];
    float* LW = reinterpret_cast<float*>(s_eh);
    float* LG = LW + T64_FLOATS;
    float* LL = LG + T64_FLOATS;
    float* vec = LL + T64_FLOATS;
    float* Ar = vec + EH_VEC;                // AX row-major; at a head's end the column sums of the 16 row groups
    float* At = Ar + T64_FLOATS;             // AX transposed, then dp row-major
    float* Xr = At + T64_FLOATS;
    float* Gr = Xr + T64_FLOATS;             // g row-major
    float* Gt = Gr + T64_FLOATS;             // g transposed, then da row-major
    float* Pt = Gt + T64_FLOATS;             // dp transposed, then hh row-major
    const int rg = threadIdx.x / 16, sg = threadIdx.x % 16;
    for (int h = 0; h < H; ++h) {
        if (h) __syncthreads();              // every read of the previous head's matrices and column sums is done
        eh_setup(LW, LG, LL, vec, W, b, G, bg, L, bl, h);
        const float* __restrict__ scale_h = scale ? scale + (size_t)h * n * EH_D : nullptr;
        const float* __restrict__ g_h = g + (size_t)h * n * EH_D;
        float4 ww[4], wg[4], wl[4];          // dW, dG, dL at [4 rg + i][4 sg .. + 3]
        float cs[3][4];                      // db at the columns 4 sg + j; dbg, dbl at the columns sg + 16 j
        t64_zero(ww), t64_zero(wg), t64_zero(wl);
#pragma unroll
        for (int j = 0; j < 4; ++j) cs[0][j] = cs[1][j] = cs[2][j] = 0.f;
        for (int t = 0; t < tiles; ++t) {
            const long row0 = t64_row0(t, tiles);
            if (row0 >= n) break;
            {
                float4 v[4];
                t64_rows(v, AX, row0, n, rg, sg);
                t64_put_t(At, rg, sg, v);
                t64_put0(Ar, rg, sg, v);
                t64_rows(v, g_h, row0, n, rg, sg);
                t64_put_t(Gt, rg, sg, v);
                t64_put0(Gr, rg, sg, v);
            }
            t64_load(Xr, X, row0, n, rg, sg);
            __syncthreads();
            EhRows f;
            eh_recompute(At, LW, vec, scale_h, row0, n, rg, sg, f);
            float da[4][4];
            {
                float4 dh[4];
                t64_zero(dh);
                t64_stage_nn(Gt, LG, rg, sg, dh);
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const float dv[4] = {dh[i].x, dh[i].y, dh[i].z, dh[i].w};
                    float du[4];
                    float dot = 0.f;
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const float lk = dv[j] * t64_dleaky(f.d[i][j], slope);
                        du[j] = scale_h ? lk * f.sc[i][j] : lk;
                        dot = fmaf(f.u[i][j], du[j], dot);
                    }
                    dot = row16_sum(dot);
                    const bool live = f.raw[i] >= EH_EPS;
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        da[i][j] = (live ? fmaf(-f.u[i][j], dot, du[j]) : du[j]) / f.nrm[i];
                        cs[0][j] += da[i][j];
                        f.d[i][j] = t64_leaky(f.d[i][j], slope);             // hh
                    }
                }
            }
            float dp[4][4];
            t64_start1(dp, vec + 2 * EH_D, sg);
            t64_stage_nt(Xr, LL, rg, sg, dp);
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const float gv = Gr[(4 * rg + i) * T64_LD + sg + 16 * j];
                    dp[i][j] = gv * t64_dleaky(dp[i][j], slope);
                    cs[1][j] += gv;
                    cs[2][j] += dp[i][j];
                }
            __syncthreads();                                                 // every read of AX and g transposed is done
            t64_put0(Gt, rg, sg, da);
            t64_put(At, Pt, rg, sg, dp);
            __syncthreads();
            if (part) {
                t64_stage_nn(Ar, Gt, rg, sg, ww);
                t64_stage_nn(At, Xr, rg, sg, wl);
            }
            if (dX) {
                float4 acc[4];
                if (h) t64_rows(acc, dX, row0, n, rg, sg);
                else t64_zero(acc);
                t64_stage_nn(Pt, LL, rg, sg, acc);
                t64_store(dX, row0, n, rg, sg, acc);
            }
            if (dAX) {
                float acc[4][4];
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const long r = row0 + 4 * rg + i;
#pragma unroll
                    for (int j = 0; j < 4; ++j) acc[i][j] = (h && r < n) ? dAX[(size_t)r * EH_D + sg + 16 * j] : 0.f;
                }
                t64_stage_nt(Gt, LW, rg, sg, acc);
                t64_store1(dAX, row0, n, rg, sg, acc);
            }
            if (part) {
                __syncthreads();                                             // every read of dp transposed is done
                t64_put0(Pt, rg, sg, f.d);
                __syncthreads();
                t64_stage_nn(Gr, Pt, rg, sg, wg);
            }
            __syncthreads();
        }
        if (part) {
            float* __restrict__ p = part + ((size_t)blockIdx.x * H + h) * EH_PART;
            t64_part_store(p, rg, sg, ww);
            t64_part_store(p + EH_W, rg, sg, wg);
            t64_part_store(p + 2 * EH_W, rg, sg, wl);
            const T64Layout lay[3] = {T64_L0, T64_L1, T64_L1};
            t64_colsum(Ar, rg, sg, lay, cs, p + 3 * EH_W);                   // through the AX tile, which is dead
        }
    }
}

// t64_finish_sum over the H partials of a block, and where head h's float e goes
__global__ __launch_bounds__(T64_BLOCK) void encoder_heads_finish_kernel(const float* __restrict__ part, int nb, int H,
                                                                         float* __restrict__ dW, float* __restrict__ db,
                                                                         float* __restrict__ dG, float* __restrict__ dbg,
                                                                         float* __restrict__ dL, float* __restrict__ dbl) {
    int o;                                                     // EH_PART is a multiple of 64: o < H EH_PART
    float a;
    if (!t64_finish_sum(part, nb, (size_t)H * EH_PART, o, a)) return;
    const int h = o / EH_PART, e = o % EH_PART;
    float* dst = nullptr;
    if (e < EH_W) dst = dW ? dW + h * EH_W + e : nullptr;
    else if (e < 2 * EH_W) dst = dG ? dG + h * EH_W + (e - EH_W) : nullptr;
    else if (e < 3 * EH_W) dst = dL ? dL + h * EH_W + (e - 2 * EH_W) : nullptr;
    else if (e < 3 * EH_W + EH_D) dst = db ? db + h * EH_D + (e - 3 * EH_W) : nullptr;
    else if (e < 3 * EH_W + 2 * EH_D) dst = dbg ? dbg + h * EH_D + (e - 3 * EH_W - EH_D) : nullptr;
    else dst = dbl ? dbl + h * EH_D + (e - 3 * EH_W - 2 * EH_D) : nullptr;
    if (dst) *dst = a;
}

inline bool eh_served(int64_t n, int32_t d, int32_t H) { return d == EH_D && H >= 1 && H <= EH_MAX_HEADS && n <= T64_MAX_ROWS; }

}  // namespace

extern "C" int32_t mmrec_encoder_heads_rows_per_block(int64_t n) { return n < 0 || n > T64_MAX_ROWS ? 0 : t64_fuser_rows(n); }

extern "C" size_t mmrec_encoder_heads_workspace_bytes(int64_t n, int32_t H) {
    if (n < 0 || n > T64_MAX_ROWS || H < 1 || H > EH_MAX_HEADS) return 0;
    return sizeof(float) * (size_t)t64_fuser_blocks(n) * H * EH_PART;
}

extern "C" int mmrec_encoder_heads_fwd_f32(const float* AX, const float* X, const float* W, const float* b, const float* G,
                                           const float* bg, const float* L, const float* bl, const float* scale, int64_t n,
                                           int32_t d, int32_t H, float slope, float* out, mmrec_stream_t stream) {
    if (!eh_served(n, d, H)) return MMREC_ERR_UNSUPPORTED;
    if (n < 0) return MMREC_ERR_BAD_ARG;
    if (n == 0) return 0;
    if (!AX || !X || !W || !b || !G || !bg || !L || !bl || !out) return MMREC_ERR_BAD_ARG;
    const int rc = t64_launch<encoder_heads_fwd_kernel>(t64_fuser_blocks(n), eh_lds_bytes(EH_FWD_TILES), mmrec_stream(stream), AX, X,
                                                        W, b, G, bg, L, bl, scale, (long)n, t64_fuser_rows(n) / T64, (int)H, slope,
                                                        out);
    if (rc) return rc;
    MMREC_RETURN_LAUNCH_STATUS();
}

extern "C" int mmrec_encoder_heads_bwd_f32(const float* AX, const float* X, const float* W, const float* b, const float* G,
                                           const float* bg, const float* L, const float* bl, const float* scale, const float* g,
                                           int64_t n, int32_t d, int32_t H, float slope, float* dAX, float* dX, float* dW, float* db,
                                           float* dG, float* dbg, float* dL, float* dbl, void* workspace, mmrec_stream_t stream) {
    if (!eh_served(n, d, H)) return MMREC_ERR_UNSUPPORTED;
    if (n < 0) return MMREC_ERR_BAD_ARG;
    if (n == 0) return 0;
    const bool want_w = dW || db || dG || dbg || dL || dbl;
    if (!AX || !X || !W || !b || !G || !bg || !L || !bl || !g || (want_w && !workspace)) return MMREC_ERR_BAD_ARG;
    if (!want_w && !dAX && !dX) return 0;
    hipStream_t s = mmrec_stream(stream);
    float* part = want_w ? static_cast<float*>(workspace) : nullptr;
    const int nb = t64_fuser_blocks(n);
    const int rc = t64_launch<encoder_heads_bwd_kernel>(nb, eh_lds_bytes(EH_BWD_TILES), s, AX, X, W, b, G, bg, L, bl, scale, g, (long)n,
                                                        t64_fuser_rows(n) / T64, (int)H, slope, dAX, dX, part);
    if (rc) return rc;
    if (want_w)
        hipLaunchKernelGGL(encoder_heads_finish_kernel, dim3(H * EH_PART / EH_D), dim3(T64_BLOCK), 0, s, part, nb, (int)H, dW, db,
                           dG, dbg, dL, dbl);
    MMREC_RETURN_LAUNCH_STATUS();
}
