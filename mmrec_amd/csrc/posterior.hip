// MVGAE's posterior tail (include/mmrec_hip.h, additive to ABI 16): the two products of experts, the four reparametrisations,
// the four KL terms and sigmoid(mu_p) -- mvgae.py, forward / calculate_loss -- over all n = users + items rows in ONE launch and
// a finish of one workgroup, and its backward in ONE launch.  fp32 throughout, element-wise but for the four KL sums.
//
// Per element (v image, t text, c collaborative; eps = 1e-8):
//     PoE((mu_a, l_a), (mu_b, l_b)):  T_x = 1 / (exp(l_x) + eps),  S = T_a + T_b,  var = 1 / S,  m = (mu_a T_a + mu_b T_b) var,
//                                     l = log(var)
//     (m1, l1) = PoE(v, t);   (mu_p, l_p) = PoE((m1, l1), c)            l1 goes into stage 2 as it is: no clamp
//     k in (p, v, t, c):  lh_k = min(l_k, 10),  Z[k] = mu_k + 0.1 E_k exp(0.5 lh_k),  kl[k] = -0.5 / n sum (1 + lh_k - mu_k^2 - exp(lh_k))
//     score = sigmoid(mu_p)
//
// THE PLAN (what the fuzz's error bound counts).  A 16-lane group per row, one float4 per lane and table.  One 256-thread
// workgroup per block of R = mmrec_posterior_fusion_rows_per_block(n) consecutive rows, walked in R / 16 passes of 16 rows: group g
// of pass p has the row  block R + 16 p + g.  Every operation below is one rounding (an fma is one), in this order:
//   expert   E = expf(l), T = 1 / (E + eps)
//   PoE      S = T_a + T_b, var = 1 / S, m = fma(mu_b, T_b, mu_a T_a) var, l = logf(var)
//   tail     lh = fminf(l, 10), sd = expf(0.5 lh), el = expf(lh), Z = fma(0.1 E_k, sd, mu)  (noise NULL: Z = mu, a copy)
//   KL term  t = fma(-mu, mu, 1 + lh) - el;  a lane adds its four columns in order, t_0 + t_1 + t_2 + t_3 (3 additions), the 16
//            lanes by the butterfly xor 8, 4, 2, 1 (4), the group adds its rows pass after pass onto one sum from 0 (R / 16), the
//            16 groups are added in order from 0 (16): one partial per block and k, four floats per block in the workspace.
//   finish   ONE workgroup, wave k for kl[k]: lane j adds the blocks j, j + 64, ... in order from 0 (ceil(blocks / 64)), the 64
//            lanes by the butterfly xor 32, 16, 8, 4, 2, 1 (6);  kl[k] = (-0.5 inv_n) sum,  inv_n = 1 / (float)n  rounded once.
//   sigmoid  q = expf(-|z|), score = (z >= 0 ? 1 : q) / (1 + q): exactly 1 / 0 once q underflows; the argument of expf is exact.
// Backward, everything RECOMPUTED from the ten inputs as above (state between the calls: the inputs), then per element
//   ck = g_kl[k] inv_n  (0 where g_kl is NULL),  gz = gZ[k]  (0 where gZ is NULL)
//   up_k     gm_k = fma(ck, mu_k, gz);   gl_k = l_k <= 10 ? fma(gz, (0.05 E_k) sd_k, -((0.5 ck) (1 - el_k))) : 0
//            (noise NULL: E_k = 0)
//   PoE backward of (gm, gl) into expert a (b alike):   w_a = ((T_a T_a) E_a) var
//            d mu_a = (gm T_a) var,   d l_a = -(w_a fma(gm, mu_a - m, -gl))
//   stage 2 from up_p gives (g m1, g l1) and c's share; stage 1 from (g m1, g l1) gives v's and t's shares;
//   d_mu_k = share + gm_k,  d_lv_k = share + gl_k  for k in (v, t, c).
// NO ATOMICS, every order fixed by n alone.  Rows past n are never read and never stored; they add 0 to the sums.
#include "common.h"

namespace {

constexpr int PF_D = 64;
constexpr int PF_BLOCK = 256;
constexpr int PF_ROWS = 16;                                 // rows of a pass: 16 groups of 16 lanes
constexpr int PF_MAX_BLOCKS = 1024;
constexpr int64_t PF_MAX_ROWS = (int64_t)1 << 30;
constexpr float PF_EPS = 1e-8f;
constexpr float PF_MAX_LOGVAR = 10.f;

inline int pf_rows_per_block(int64_t n) {
    const int64_t p = (n + (int64_t)PF_ROWS * PF_MAX_BLOCKS - 1) / ((int64_t)PF_ROWS * PF_MAX_BLOCKS);
    return (int)(p < 1 ? 1 : p) * PF_ROWS;
}
inline int pf_blocks(int64_t n) { return n <= 0 ? 0 : (int)((n + pf_rows_per_block(n) - 1) / pf_rows_per_block(n)); }

struct PfExpert {
    float E, T;
};
struct PfPoE {
    float var, m, l;
};

__device__ __forceinline__ PfExpert pf_expert(float l) {
    PfExpert x;
    x.E = expf(l);
    x.T = 1.f / (x.E + PF_EPS);
    return x;
}
__device__ __forceinline__ PfPoE pf_poe(float mu_a, PfExpert a, float mu_b, PfExpert b) {
    PfPoE r;
    r.var = 1.f / (a.T + b.T);
    r.m = fmaf(mu_b, b.T, mu_a * a.T) * r.var;
    r.l = logf(r.var);
    return r;
}
__device__ __forceinline__ float pf_get(const float4& v, int j) { return j == 0 ? v.x : j == 1 ? v.y : j == 2 ? v.z : v.w; }
__device__ __forceinline__ void pf_set(float4& v, int j, float x) {
    if (j == 0) v.x = x;
    else if (j == 1) v.y = x;
    else if (j == 2) v.z = x;
    else v.w = x;
}
__device__ __forceinline__ float4 pf_load(const float* __restrict__ g, size_t at) {
    return *reinterpret_cast<const float4*>(g + at);
}

// Z and the KL term of one (mu, l): the tail of the plan
__device__ __forceinline__ float pf_tail(float mu, float l, bool noisy, float e, float& z) {
    const float lh = fminf(l, PF_MAX_LOGVAR);
    const float sd = expf(0.5f * lh), el = expf(lh);
    z = noisy ? fmaf(0.1f * e, sd, mu) : mu;
    return fmaf(-mu, mu, 1.f + lh) - el;
}

__global__ __launch_bounds__(PF_BLOCK) void posterior_fwd_kernel(
    const float* __restrict__ mu_v, const float* __restrict__ lv_v, const float* __restrict__ mu_t,
    const float* __restrict__ lv_t, const float* __restrict__ mu_c, const float* __restrict__ lv_c,
    const float* __restrict__ E_p, const float* __restrict__ E_v, const float* __restrict__ E_t, const float* __restrict__ E_c,
    long n, int passes, float* __restrict__ Z, float* __restrict__ score, float* __restrict__ part) {
    __shared__ float red[PF_ROWS][4];
    const int g = threadIdx.x / 16, lane = threadIdx.x % 16;
    const bool noisy = E_p != nullptr;
    const size_t plane = (size_t)n * PF_D;
    float acc[4] = {0.f, 0.f, 0.f, 0.f};                     // the group's KL sums, order p, v, t, c
    for (int p = 0; p < passes; ++p) {
        const long r = ((long)blockIdx.x * passes + p) * PF_ROWS + g;
        const bool live = r < n;
        const size_t at = (size_t)(live ? r : 0) * PF_D + 4 * lane;
        float4 mv, lv, mt, lt, mc, lc, ep, ev, et, ec;
        mv = lv = mt = lt = mc = lc = ep = ev = et = ec = f4_zero();
        if (live) {
            mv = pf_load(mu_v, at), lv = pf_load(lv_v, at), mt = pf_load(mu_t, at);
            lt = pf_load(lv_t, at), mc = pf_load(mu_c, at), lc = pf_load(lv_c, at);
            if (noisy) ep = pf_load(E_p, at), ev = pf_load(E_v, at), et = pf_load(E_t, at), ec = pf_load(E_c, at);
        }
        float4 zp, zv, zt, zc, sc;
        float row[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float muv = pf_get(mv, j), lvv = pf_get(lv, j), mut = pf_get(mt, j), lvt = pf_get(lt, j);
            const float muc = pf_get(mc, j), lvc = pf_get(lc, j);
            const PfPoE s1 = pf_poe(muv, pf_expert(lvv), mut, pf_expert(lvt));
            const PfPoE s2 = pf_poe(s1.m, pf_expert(s1.l), muc, pf_expert(lvc));
            float z;
            const float tp = pf_tail(s2.m, s2.l, noisy, pf_get(ep, j), z);
            pf_set(zp, j, z);
            const float tv = pf_tail(muv, lvv, noisy, pf_get(ev, j), z);
            pf_set(zv, j, z);
            const float tt = pf_tail(mut, lvt, noisy, pf_get(et, j), z);
            pf_set(zt, j, z);
            const float tc = pf_tail(muc, lvc, noisy, pf_get(ec, j), z);
            pf_set(zc, j, z);
            pf_set(sc, j, stable_sigmoid(s2.m));
            row[0] = j ? row[0] + tp : tp;
            row[1] = j ? row[1] + tv : tv;
            row[2] = j ? row[2] + tt : tt;
            row[3] = j ? row[3] + tc : tc;
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float s = row16_sum(row[k]);
            acc[k] += live ? s : 0.f;
        }
        if (live) {
            *reinterpret_cast<float4*>(Z + at) = zp;
            *reinterpret_cast<float4*>(Z + plane + at) = zv;
            *reinterpret_cast<float4*>(Z + 2 * plane + at) = zt;
            *reinterpret_cast<float4*>(Z + 3 * plane + at) = zc;
            *reinterpret_cast<float4*>(score + at) = sc;
        }
    }
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < 4; ++k) red[g][k] = acc[k];
    }
    __syncthreads();
    if (threadIdx.x < 4) {
        float a = 0.f;
        for (int i = 0; i < PF_ROWS; ++i) a += red[i][threadIdx.x];
        part[(size_t)blockIdx.x * 4 + threadIdx.x] = a;
    }
}

// wave k for kl[k]: lane j adds the blocks j, j + 64, ... in order from 0, then the butterfly over the 64 lanes
__global__ __launch_bounds__(PF_BLOCK) void posterior_finish_kernel(const float* __restrict__ part, int nb, float inv_n,
                                                                    float* __restrict__ kl) {
    const int k = threadIdx.x / MMREC_WAVE, j = threadIdx.x % MMREC_WAVE;
    float a = 0.f;
    for (int b = j; b < nb; b += MMREC_WAVE) a += part[(size_t)b * 4 + k];
    a = wave_sum(a);
    if (j == 0) kl[k] = (-0.5f * inv_n) * a;
}

// up_k of the plan: the gradient of Z[k] and kl[k] in (mu_k, l_k)
__device__ __forceinline__ void pf_up(float mu, float l, float e, float gz, float ck, float& gm, float& gl) {
    const float lh = fminf(l, PF_MAX_LOGVAR);
    const float sd = expf(0.5f * lh), el = expf(lh);
    gm = fmaf(ck, mu, gz);
    gl = l <= PF_MAX_LOGVAR ? fmaf(gz, (0.05f * e) * sd, -((0.5f * ck) * (1.f - el))) : 0.f;
}
// the PoE's backward into one expert
__device__ __forceinline__ void pf_poe_bwd(float mu_a, PfExpert a, PfPoE r, float gm, float gl, float& d_mu, float& d_l) {
    const float w = ((a.T * a.T) * a.E) * r.var;
    d_mu = (gm * a.T) * r.var;
    d_l = -(w * fmaf(gm, mu_a - r.m, -gl));
}

__global__ __launch_bounds__(PF_BLOCK) void posterior_bwd_kernel(
    const float* __restrict__ mu_v, const float* __restrict__ lv_v, const float* __restrict__ mu_t,
    const float* __restrict__ lv_t, const float* __restrict__ mu_c, const float* __restrict__ lv_c,
    const float* __restrict__ E_p, const float* __restrict__ E_v, const float* __restrict__ E_t, const float* __restrict__ E_c,
    const float* __restrict__ gZ, const float* __restrict__ g_kl, long n, int passes, float inv_n, float* __restrict__ d_mu_v,
    float* __restrict__ d_lv_v, float* __restrict__ d_mu_t, float* __restrict__ d_lv_t, float* __restrict__ d_mu_c,
    float* __restrict__ d_lv_c) {
    const int g = threadIdx.x / 16, lane = threadIdx.x % 16;
    const bool noisy = E_p != nullptr;
    const size_t plane = (size_t)n * PF_D;
    float ck[4] = {0.f, 0.f, 0.f, 0.f};
    if (g_kl) {
#pragma unroll
        for (int k = 0; k < 4; ++k) ck[k] = g_kl[k] * inv_n;
    }
    for (int p = 0; p < passes; ++p) {
        const long r = ((long)blockIdx.x * passes + p) * PF_ROWS + g;
        if (r >= n) break;                                   // no cross-lane step below
        const size_t at = (size_t)r * PF_D + 4 * lane;
        const float4 mv = pf_load(mu_v, at), lv = pf_load(lv_v, at), mt = pf_load(mu_t, at);
        const float4 lt = pf_load(lv_t, at), mc = pf_load(mu_c, at), lc = pf_load(lv_c, at);
        float4 ep, ev, et, ec, gp, gv, gt, gc;
        ep = ev = et = ec = gp = gv = gt = gc = f4_zero();
        if (noisy) ep = pf_load(E_p, at), ev = pf_load(E_v, at), et = pf_load(E_t, at), ec = pf_load(E_c, at);
        if (gZ) {
            gp = pf_load(gZ, at), gv = pf_load(gZ, plane + at);
            gt = pf_load(gZ, 2 * plane + at), gc = pf_load(gZ, 3 * plane + at);
        }
        float4 dmv, dlv, dmt, dlt, dmc, dlc;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float muv = pf_get(mv, j), lvv = pf_get(lv, j), mut = pf_get(mt, j), lvt = pf_get(lt, j);
            const float muc = pf_get(mc, j), lvc = pf_get(lc, j);
            const PfExpert xv = pf_expert(lvv), xt = pf_expert(lvt), xc = pf_expert(lvc);
            const PfPoE s1 = pf_poe(muv, xv, mut, xt);
            const PfExpert x1 = pf_expert(s1.l);
            const PfPoE s2 = pf_poe(s1.m, x1, muc, xc);
            float gm, gl, gm1, gl1, a, b;
            pf_up(s2.m, s2.l, pf_get(ep, j), pf_get(gp, j), ck[0], gm, gl);
            pf_poe_bwd(s1.m, x1, s2, gm, gl, gm1, gl1);
            pf_poe_bwd(muc, xc, s2, gm, gl, a, b);
            pf_up(muc, lvc, pf_get(ec, j), pf_get(gc, j), ck[3], gm, gl);
            pf_set(dmc, j, a + gm);
            pf_set(dlc, j, b + gl);
            pf_poe_bwd(muv, xv, s1, gm1, gl1, a, b);
            pf_up(muv, lvv, pf_get(ev, j), pf_get(gv, j), ck[1], gm, gl);
            pf_set(dmv, j, a + gm);
            pf_set(dlv, j, b + gl);
            pf_poe_bwd(mut, xt, s1, gm1, gl1, a, b);
            pf_up(mut, lvt, pf_get(et, j), pf_get(gt, j), ck[2], gm, gl);
            pf_set(dmt, j, a + gm);
            pf_set(dlt, j, b + gl);
        }
        if (d_mu_v) *reinterpret_cast<float4*>(d_mu_v + at) = dmv;
        if (d_lv_v) *reinterpret_cast<float4*>(d_lv_v + at) = dlv;
        if (d_mu_t) *reinterpret_cast<float4*>(d_mu_t + at) = dmt;
        if (d_lv_t) *reinterpret_cast<float4*>(d_lv_t + at) = dlt;
        if (d_mu_c) *reinterpret_cast<float4*>(d_mu_c + at) = dmc;
        if (d_lv_c) *reinterpret_cast<float4*>(d_lv_c + at) = dlc;
    }
}

// 0: go on;  1: nothing to do;  otherwise the error
inline int pf_check(int64_t n, int32_t d, const float* const* in, const float* const* noise) {
    if (d != PF_D || n < 0 || n > PF_MAX_ROWS) return MMREC_ERR_BAD_ARG;
    if (n == 0) return 1;
    for (int i = 0; i < 6; ++i)
        if (!in[i]) return MMREC_ERR_BAD_ARG;
    const int given = (noise[0] != nullptr) + (noise[1] != nullptr) + (noise[2] != nullptr) + (noise[3] != nullptr);
    return given == 0 || given == 4 ? 0 : MMREC_ERR_BAD_ARG;
}

}  // namespace

extern "C" int32_t mmrec_posterior_fusion_rows_per_block(int64_t n) { return n < 0 || n > PF_MAX_ROWS ? 0 : pf_rows_per_block(n); }

extern "C" size_t mmrec_posterior_fusion_workspace_bytes(int64_t n) {
    if (n < 0 || n > PF_MAX_ROWS) return 0;
    return sizeof(float) * 4 * (size_t)pf_blocks(n);
}

extern "C" int mmrec_posterior_fusion_fwd_f32(const float* mu_v, const float* lv_v, const float* mu_t, const float* lv_t,
                                              const float* mu_c, const float* lv_c, const float* E_p, const float* E_v,
                                              const float* E_t, const float* E_c, int64_t n, int32_t d, float* Z, float* score,
                                              float* kl, void* workspace, mmrec_stream_t stream) {
    const float* in[6] = {mu_v, lv_v, mu_t, lv_t, mu_c, lv_c};
    const float* noise[4] = {E_p, E_v, E_t, E_c};
    const int rc = pf_check(n, d, in, noise);
    if (rc) return rc == 1 ? 0 : rc;
    if (!Z || !score || !kl || !workspace) return MMREC_ERR_BAD_ARG;
    hipStream_t s = mmrec_stream(stream);
    const int nb = pf_blocks(n);
    float* part = static_cast<float*>(workspace);
    hipLaunchKernelGGL(posterior_fwd_kernel, dim3(nb), dim3(PF_BLOCK), 0, s, mu_v, lv_v, mu_t, lv_t, mu_c, lv_c, E_p, E_v, E_t, E_c,
                       (long)n, pf_rows_per_block(n) / PF_ROWS, Z, score, part);
    hipLaunchKernelGGL(posterior_finish_kernel, dim3(1), dim3(PF_BLOCK), 0, s, part, nb, 1.f / (float)n, kl);
    MMREC_RETURN_LAUNCH_STATUS();
}

extern "C" int mmrec_posterior_fusion_bwd_f32(const float* mu_v, const float* lv_v, const float* mu_t, const float* lv_t,
                                              const float* mu_c, const float* lv_c, const float* E_p, const float* E_v,
                                              const float* E_t, const float* E_c, const float* gZ, const float* g_kl, int64_t n,
                                              int32_t d, float* d_mu_v, float* d_lv_v, float* d_mu_t, float* d_lv_t,
                                              float* d_mu_c, float* d_lv_c, mmrec_stream_t stream) {
    const float* in[6] = {mu_v, lv_v, mu_t, lv_t, mu_c, lv_c};
    const float* noise[4] = {E_p, E_v, E_t, E_c};
    const int rc = pf_check(n, d, in, noise);
    if (rc) return rc == 1 ? 0 : rc;
    if (!d_mu_v && !d_lv_v && !d_mu_t && !d_lv_t && !d_mu_c && !d_lv_c) return 0;
    hipLaunchKernelGGL(posterior_bwd_kernel, dim3(pf_blocks(n)), dim3(PF_BLOCK), 0, mmrec_stream(stream), mu_v, lv_v, mu_t, lv_t,
                       mu_c, lv_c, E_p, E_v, E_t, E_c, gZ, g_kl, (long)n, pf_rows_per_block(n) / PF_ROWS, 1.f / (float)n, d_mu_v,
                       d_lv_v, d_mu_t, d_lv_t, d_mu_c, d_lv_c);
    MMREC_RETURN_LAUNCH_STATUS();
}
