// MGCN's behaviour-aware fuser (include/mmrec_hip.h, additive to ABI 16): the attention over the two modalities, the two
// preference gates and the mix -- mgcn.py:188-203 -- over all n = users + items rows in ONE launch, and its backward in two (the
// main pass + the weight gradients' finish).  fp32 throughout, VALU fma (tile64.h) with the three weight matrices in LDS.
//
// Per row (V image, T text, C content; Wq, Wv, Wt [64][64] as [out][in]):
//     zV = V Wq^T + bq, hV = tanh(zV), sV = <hV, q>   (zT, hT, sT alike)      (aV, aT) = softmax(sV, sT)      m = aV V + aT T
//     pV = sigmoid(C Wv^T + bv), pT = sigmoid(C Wt^T + bt)       side = (pV (V - m) + pT (T - m) + m) / 3       out = C + side
//
// THE PLAN (what the fuzz's error bound counts) is tile64.h's: blocks of R = mmrec_modal_fusion_rows_per_block(n) rows, stage,
// weight partials, column sums, finish.  Wq, Wv, Wt stay in LDS for the block's life, as they lie in memory ([out][in], 68-float
// rows).  This op's own:
//   stage   z / u: the chain over the input column k starts at the bias.
//   tanh    q = expf(-2 |z|), h = copysign((1 - q) / (1 + q), z);  sigmoid: q = expf(-|z|), p = (z >= 0 ? 1 : q) / (1 + q).
//           Exactly +-1 and 1 / 0 once q underflows to 0; the argument of expf is exact and never positive.
//   score   the thread's columns c = sg, sg + 16, sg + 32, sg + 48: s = fma(h_c, q_c, s) from 0 in this order, then the butterfly
//           over the 16 lanes of the row (xor 8, 4, 2, 1).
//   mix     mx = max(sV, sT), eV = expf(sV - mx), eT = expf(sT - mx), den = eV + eT, aV = eV / den, aT = eT / den;
//           m = fma(aT, T, aV V), xV = V - m, xT = T - m, side = fma(pT, xT, fma(pV, xV, m)) / 3, out = C + side.
// Backward, everything RECOMPUTED from V, T, C and the weights as above (state between the calls: the operands), then
//   G = g_side + g_out (a NULL one is zeros), G3 = G / 3, dm = G3 ((1 - pV) - pT), dpV = G3 xV, dpT = G3 xT,
//   dot = fma(dm_c, V_c - T_c, dot) over the thread's columns from 0, then the same butterfly;  dsV = (aV aT) dot, dsT = -dsV,
//   dzV = (dsV q) fma(-hV, hV, 1), dzT alike;  duV = dpV (pV (1 - pV)), duT alike;
//   dV = the stage over the output column o of dzV Wq, started at fma(aV, dm, G3 pV);  dT alike;
//   dC = the stage of duV Wv started at g_out (or 0), continued by the stage of duT Wt.
//   dWq[o][k] = one fma chain over the block's rows: per tile the 64 rows of dzV^T V, then the 64 of dzT^T T;  dWv, dWt: duV^T C,
//   duT^T C.   The column sums: dbq (terms dzV + dzT), dbv (duV), dbt (duT), dq (fma(dsT, hT, dsV hV)).
// Rows past n get G = 0.
// Workspace: 3 (64 64 + 64) + 64 = 12,544 floats per block: [dWq][dWv][dWt][dbq][dbv][dbt][dq].
#include "tile64.h"

namespace {

constexpr int MF_D = 64;
constexpr int MF_W = MF_D * MF_D;
constexpr int MF_PART = 3 * (MF_W + MF_D) + MF_D;           // floats of one block's partial
constexpr int MF_VEC = 4 * MF_D;                            // bq, q, bv, bt in LDS
constexpr int MF_FWD_TILES = 3, MF_BWD_TILES = 5;

constexpr size_t mf_lds_bytes(int tiles) { return sizeof(float) * ((size_t)(3 + tiles) * T64_FLOATS + MF_VEC); }

__device__ __forceinline__ float mf_tanh(float z) {
    const float q = expf(-2.f * fabsf(z));
    return copysignf((1.f - q) / (1.f + q), z);
}

__device__ __forceinline__ void mf_setup(float* __restrict__ LWq, float* __restrict__ LWv, float* __restrict__ LWt,
                                         float* __restrict__ vec, const float* __restrict__ Wq, const float* __restrict__ bq,
                                         const float* __restrict__ q, const float* __restrict__ Wv, const float* __restrict__ bv,
                                         const float* __restrict__ Wt, const float* __restrict__ bt) {
    t64_matrix(LWq, Wq);
    t64_matrix(LWv, Wv);
    t64_matrix(LWt, Wt);
    const int c = threadIdx.x % MF_D;
    const float* __restrict__ src = threadIdx.x < MF_D ? bq : threadIdx.x < 2 * MF_D ? q : threadIdx.x < 3 * MF_D ? bv : bt;
    vec[threadIdx.x] = src[c];
}

// the forward's intermediates of the thread's rows 4 rg + i at its columns sg + 16 j (layout L1), from the tiles in LDS
struct MfRows {
    float hV[4][4], hT[4][4], pV[4][4], pT[4][4];
    float aV[4], aT[4];
};

__device__ __forceinline__ void mf_recompute(const float* __restrict__ Vr, const float* __restrict__ Tr,
                                             const float* __restrict__ Cr, const float* __restrict__ LWq,
                                             const float* __restrict__ LWv, const float* __restrict__ LWt,
                                             const float* __restrict__ vec, int rg, int sg, MfRows& f) {
    float sV[4], sT[4];
#pragma unroll
    for (int pass = 0; pass < 2; ++pass) {
        float (&h)[4][4] = pass ? f.hT : f.hV;
        float (&s)[4] = pass ? sT : sV;
        t64_start1(h, vec, sg);
        t64_stage_nt(pass ? Tr : Vr, LWq, rg, sg, h);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            float a = 0.f;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                h[i][j] = mf_tanh(h[i][j]);
                a = fmaf(h[i][j], vec[MF_D + sg + 16 * j], a);
            }
            s[i] = row16_sum(a);
        }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const float mx = fmaxf(sV[i], sT[i]);
        const float eV = expf(sV[i] - mx), eT = expf(sT[i] - mx);
        const float den = eV + eT;
        f.aV[i] = eV / den;
        f.aT[i] = eT / den;
    }
#pragma unroll
    for (int pass = 0; pass < 2; ++pass) {
        float (&p)[4][4] = pass ? f.pT : f.pV;
        t64_start1(p, vec + (pass ? 3 : 2) * MF_D, sg);
        t64_stage_nt(Cr, pass ? LWt : LWv, rg, sg, p);
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) p[i][j] = stable_sigmoid(p[i][j]);
    }
}

__global__ __launch_bounds__(T64_BLOCK) void modal_fusion_fwd_kernel(
    const float* __restrict__ V, const float* __restrict__ T, const float* __restrict__ C, const float* __restrict__ Wq,
    const float* __restrict__ bq, const float* __restrict__ q, const float* __restrict__ Wv, const float* __restrict__ bv,
    const float* __restrict__ Wt, const float* __restrict__ bt, long n, int tiles, float* __restrict__ side,
    float* __restrict__ out) {
    extern __shared__ float4 s_mf[];
    float* LWq = reinterpret_cast<float*>(s_mf);
    float* LWv = LWq + T64_FLOATS;
    float* LWt = LWv + T64_FLOATS;
    float* vec = LWt + T64_FLOATS;
    float* Vr = vec + MF_VEC;
    float* Tr = Vr + T64_FLOATS;
    float* Cr = Tr + T64_FLOATS;
    const int rg = threadIdx.x / 16, sg = threadIdx.x % 16;
    mf_setup(LWq, LWv, LWt, vec, Wq, bq, q, Wv, bv, Wt, bt);
    for (int t = 0; t < tiles; ++t) {
        const long row0 = t64_row0(t, tiles);
        if (row0 >= n) break;
        t64_load(Vr, V, row0, n, rg, sg);
        t64_load(Tr, T, row0, n, rg, sg);
        t64_load(Cr, C, row0, n, rg, sg);
        __syncthreads();
        MfRows f;
        mf_recompute(Vr, Tr, Cr, LWq, LWv, LWt, vec, rg, sg, f);
        float s[4][4], o[4][4];
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int at = (4 * rg + i) * T64_LD + sg + 16 * j;
                const float v = Vr[at], x = Tr[at];
                const float m = fmaf(f.aT[i], x, f.aV[i] * v);
                s[i][j] = fmaf(f.pT[i][j], x - m, fmaf(f.pV[i][j], v - m, m)) / 3.f;
                o[i][j] = Cr[at] + s[i][j];
            }
        t64_store1(side, row0, n, rg, sg, s);
        t64_store1(out, row0, n, rg, sg, o);
        __syncthreads();
    }
}

__global__ __launch_bounds__(T64_BLOCK) void modal_fusion_bwd_kernel(
    const float* __restrict__ V, const float* __restrict__ T, const float* __restrict__ C, const float* __restrict__ Wq,
    const float* __restrict__ bq, const float* __restrict__ q, const float* __restrict__ Wv, const float* __restrict__ bv,
    const float* __restrict__ Wt, const float* __restrict__ bt, const float* __restrict__ g_side,
    const float* __restrict__ g_out, long n, int tiles, float* __restrict__ dV, float* __restrict__ dT, float* __restrict__ dC,
    float* __restrict__ part) {
    extern __shared__ float4 s_mf[];
    float* LWq = reinterpret_cast<float*>(s_mf);
    float* LWv = LWq + T64_FLOATS;
    float* LWt = LWv + T64_FLOATS;
    float* vec = LWt + T64_FLOATS;
    float* Vr = vec + MF_VEC;
    float* Tr = Vr + T64_FLOATS;
    float* Cr = Tr + T64_FLOATS;             // C, then the starts of dV and dT
    float* Xr = Cr + T64_FLOATS;             // g_side, then du / dz row-major
    float* Xt = Xr + T64_FLOATS;             // g_out, then du / dz transposed
    const int rg = threadIdx.x / 16, sg = threadIdx.x % 16;
    float4 wq[4], wv[4], wt[4];              // dWq, dWv, dWt at [4 rg + i][4 sg .. + 3]
    float cs[4][4];                          // the column sums dbq, dbv, dbt, dq at the columns sg + 16 j
    t64_zero(wq), t64_zero(wv), t64_zero(wt), t64_zero(cs);
    mf_setup(LWq, LWv, LWt, vec, Wq, bq, q, Wv, bv, Wt, bt);
    for (int t = 0; t < tiles; ++t) {
        const long row0 = t64_row0(t, tiles);
        if (row0 >= n) break;
        t64_load(Vr, V, row0, n, rg, sg);
        t64_load(Tr, T, row0, n, rg, sg);
        t64_load(Cr, C, row0, n, rg, sg);
        t64_load(Xr, g_side, row0, n, rg, sg);
        t64_load(Xt, g_out, row0, n, rg, sg);
        __syncthreads();
        MfRows f;
        mf_recompute(Vr, Tr, Cr, LWq, LWv, LWt, vec, rg, sg, f);
        float4 dc[4];                        // dC starts at g_out
        t64_get0(dc, Xt, rg, sg);
        float duV[4][4], duT[4][4], sV_[4][4], sT_[4][4];      // sV_, sT_: the starts of dV and dT
        float dsV[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            float dot = 0.f;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int at = (4 * rg + i) * T64_LD + sg + 16 * j;
                const float v = Vr[at], x = Tr[at];
                const float G3 = (Xr[at] + Xt[at]) / 3.f;
                const float m = fmaf(f.aT[i], x, f.aV[i] * v);
                const float pv = f.pV[i][j], pt = f.pT[i][j];
                const float dm = G3 * ((1.f - pv) - pt);
                dot = fmaf(dm, v - x, dot);
                duV[i][j] = (G3 * (v - m)) * (pv * (1.f - pv));
                duT[i][j] = (G3 * (x - m)) * (pt * (1.f - pt));
                sV_[i][j] = fmaf(f.aV[i], dm, G3 * pv);
                sT_[i][j] = fmaf(f.aT[i], dm, G3 * pt);
            }
            dsV[i] = (f.aV[i] * f.aT[i]) * row16_sum(dot);
        }
        // dz over h, in place; the four column sums
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float qc = vec[MF_D + sg + 16 * j];
                const float hv = f.hV[i][j], ht = f.hT[i][j];
                const float dsT = -dsV[i];
                const float e = fmaf(dsT, ht, dsV[i] * hv);
                const float zv = (dsV[i] * qc) * fmaf(-hv, hv, 1.f), zt = (dsT * qc) * fmaf(-ht, ht, 1.f);
                f.hV[i][j] = zv;
                f.hT[i][j] = zt;
                cs[0][j] += zv + zt;
                cs[1][j] += duV[i][j];
                cs[2][j] += duT[i][j];
                cs[3][j] += e;
            }
        __syncthreads();                                       // every read of g_side, g_out in Xr, Xt is done
        t64_put(Xr, Xt, rg, sg, duV);
        __syncthreads();
        if (part) t64_stage_nn(Xr, Cr, rg, sg, wv);
        if (dC) t64_stage_nn(Xt, LWv, rg, sg, dc);
        __syncthreads();
        t64_put(Xr, Xt, rg, sg, duT);
        __syncthreads();
        if (part) t64_stage_nn(Xr, Cr, rg, sg, wt);
        if (dC) {
            t64_stage_nn(Xt, LWt, rg, sg, dc);
            t64_store(dC, row0, n, rg, sg, dc);
        }
        __syncthreads();                                       // C is dead: its tile holds the starts of dV, then of dT
        t64_put(Cr, nullptr, rg, sg, sV_);
        t64_put(Xr, Xt, rg, sg, f.hV);
        __syncthreads();
        if (part) t64_stage_nn(Xr, Vr, rg, sg, wq);
        if (dV) {
            t64_get0(dc, Cr, rg, sg);
            t64_stage_nn(Xt, LWq, rg, sg, dc);
            t64_store(dV, row0, n, rg, sg, dc);
        }
        __syncthreads();
        t64_put(Cr, nullptr, rg, sg, sT_);
        t64_put(Xr, Xt, rg, sg, f.hT);
        __syncthreads();
        if (part) t64_stage_nn(Xr, Tr, rg, sg, wq);
        if (dT) {
            t64_get0(dc, Cr, rg, sg);
            t64_stage_nn(Xt, LWq, rg, sg, dc);
            t64_store(dT, row0, n, rg, sg, dc);
        }
        __syncthreads();
    }
    if (part) {
        float* __restrict__ p = part + (size_t)blockIdx.x * MF_PART;
        t64_part_store(p, rg, sg, wq);
        t64_part_store(p + MF_W, rg, sg, wv);
        t64_part_store(p + 2 * MF_W, rg, sg, wt);
        const T64Layout lay[4] = {T64_L1, T64_L1, T64_L1, T64_L1};
        t64_colsum(Vr, rg, sg, lay, cs, p + 3 * MF_W);      // through the V tile, which is dead
    }
}

// t64_finish_sum, and where a partial's float o goes
__global__ __launch_bounds__(T64_BLOCK) void modal_fusion_finish_kernel(const float* __restrict__ part, int nb,
                                                                        float* __restrict__ dWq, float* __restrict__ dbq,
                                                                        float* __restrict__ dq, float* __restrict__ dWv,
                                                                        float* __restrict__ dbv, float* __restrict__ dWt,
                                                                        float* __restrict__ dbt) {
    int o;                                                     // MF_PART is a multiple of 64: o < MF_PART
    float a;
    if (!t64_finish_sum(part, nb, MF_PART, o, a)) return;
    constexpr int W = MF_W;
    float* dst = nullptr;
    if (o < W) dst = dWq ? dWq + o : nullptr;
    else if (o < 2 * W) dst = dWv ? dWv + (o - W) : nullptr;
    else if (o < 3 * W) dst = dWt ? dWt + (o - 2 * W) : nullptr;
    else if (o < 3 * W + MF_D) dst = dbq ? dbq + (o - 3 * W) : nullptr;
    else if (o < 3 * W + 2 * MF_D) dst = dbv ? dbv + (o - 3 * W - MF_D) : nullptr;
    else if (o < 3 * W + 3 * MF_D) dst = dbt ? dbt + (o - 3 * W - 2 * MF_D) : nullptr;
    else dst = dq ? dq + (o - 3 * W - 3 * MF_D) : nullptr;
    if (dst) *dst = a;
}

}  // namespace

extern "C" int32_t mmrec_modal_fusion_rows_per_block(int64_t n) { return n < 0 || n > T64_MAX_ROWS ? 0 : t64_fuser_rows(n); }

extern "C" size_t mmrec_modal_fusion_workspace_bytes(int64_t n) {
    if (n < 0 || n > T64_MAX_ROWS) return 0;
    return sizeof(float) * (size_t)t64_fuser_blocks(n) * MF_PART;
}

extern "C" int mmrec_modal_fusion_fwd_f32(const float* V, const float* T, const float* C, const float* Wq, const float* bq,
                                          const float* q, const float* Wv, const float* bv, const float* Wt, const float* bt,
                                          int64_t n, int32_t d, float* side, float* out, mmrec_stream_t stream) {
    if (d != MF_D || n > T64_MAX_ROWS) return MMREC_ERR_UNSUPPORTED;
    if (n < 0) return MMREC_ERR_BAD_ARG;
    if (n == 0) return 0;
    if (!V || !T || !C || !Wq || !bq || !q || !Wv || !bv || !Wt || !bt || !side || !out) return MMREC_ERR_BAD_ARG;
    const int rc = t64_launch<modal_fusion_fwd_kernel>(t64_fuser_blocks(n), mf_lds_bytes(MF_FWD_TILES), mmrec_stream(stream), V, T,
                                                       C, Wq, bq, q, Wv, bv, Wt, bt, (long)n, t64_fuser_rows(n) / T64, side, out);
    if (rc) return rc;
    MMREC_RETURN_LAUNCH_STATUS();
}

extern "C" int mmrec_modal_fusion_bwd_f32(const float* V, const float* T, const float* C, const float* Wq, const float* bq,
                                          const float* q, const float* Wv, const float* bv, const float* Wt, const float* bt,
                                          const float* g_side, const float* g_out, int64_t n, int32_t d, float* dV, float* dT,
                                          float* dC, float* dWq, float* dbq, float* dq, float* dWv, float* dbv, float* dWt,
                                          float* dbt, void* workspace, mmrec_stream_t stream) {
    if (d != MF_D || n > T64_MAX_ROWS) return MMREC_ERR_UNSUPPORTED;
    if (n < 0) return MMREC_ERR_BAD_ARG;
    if (n == 0) return 0;
    const bool want_w = dWq || dbq || dq || dWv || dbv || dWt || dbt;
    if (!V || !T || !C || !Wq || !bq || !q || !Wv || !bv || !Wt || !bt || (want_w && !workspace)) return MMREC_ERR_BAD_ARG;
    if (!want_w && !dV && !dT && !dC) return 0;
    hipStream_t s = mmrec_stream(stream);
    float* part = want_w ? static_cast<float*>(workspace) : nullptr;
    const int nb = t64_fuser_blocks(n);
    const int rc = t64_launch<modal_fusion_bwd_kernel>(nb, mf_lds_bytes(MF_BWD_TILES), s, V, T, C, Wq, bq, q, Wv, bv, Wt, bt, g_side,
                                                       g_out, (long)n, t64_fuser_rows(n) / T64, dV, dT, dC, part);
    if (rc) return rc;
    if (want_w)
        hipLaunchKernelGGL(modal_fusion_finish_kernel, dim3(MF_PART / MF_D), dim3(T64_BLOCK), 0, s, part, nb, dWq, dbq, dq, dWv,
                           dbv, dWt, dbt);
    MMREC_RETURN_LAUNCH_STATUS();
}
