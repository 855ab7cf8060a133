// Fused in-batch InfoNCE (reference: MGCN.InfoNCE, mgcn.py:224-231):
//   v1 = normalize(E1[ids]); v2 = normalize(E2[ids])                      (F.normalize, eps 1e-12)
//   loss = mean_i( -log( exp(<v1_i, v2_i>/tau) / sum_j exp(<v1_i, v2_j>/tau) ) )
// without ever materialising the [B, B] logits, forward or backward.
//
// B = 2048, d = 64: 0.27 GFMA per logits sweep -- a launch/latency-sized problem, so plain fp32 FMA
// tiles (64 x 64 logits per workgroup step, 4 x 4 per thread, operands in LDS), no MFMA.  exp() is
// taken without max-subtraction exactly like the reference (|logit| <= 1/tau).
// Everything is summed in a fixed order except the final scatter into the embedding-table gradients
// (duplicate ids -> atomics, as in bpr.hip).
//   prep     : gather + normalise both views, keep 1/norm
//   sweep<0> : per row block, partial row sums  ttl_part[split][i]          (forward)
//   finish   : ttl_i, loss_i, loss
//   sweep<1> : dV1n_i = sum_j g_ij v2_j ; sweep<2> : dV2n_j = sum_i g_ij v1_i ,  g_ij = (p_ij - [i=j]) / (tau B)
//   scatter  : through the normalisation, atomically into dE1 / dE2
#include "common.h"

namespace {

constexpr int NCE_T = 64;        // rows / columns per tile
constexpr int NCE_LD = 65;       // padded LDS pitch (conflict-free column walks)
constexpr int NCE_SPLIT = 4;     // column (other-index) splits per row block: fills 4x more CUs

// workspace layout (floats): V1n[B*64] V2n[B*64] inv1[B] inv2[B] ttl_part[SPLIT*B] ttl[B] lossi[B]
//                            dV1n_part[SPLIT*B*64] dV2n_part[SPLIT*B*64]
struct NceWs {
    float *v1, *v2, *inv1, *inv2, *ttl_part, *ttl, *lossi, *d1, *d2;
};
inline size_t nce_ws_floats(int B) {
    return (size_t)B * 64 * 2 + (size_t)B * 2 + (size_t)NCE_SPLIT * B + (size_t)B * 2 +
           (size_t)NCE_SPLIT * B * 64 * 2;
}
inline NceWs nce_ws(void* ws, int B) {
    NceWs w;
    float* p = static_cast<float*>(ws);
    w.v1 = p; p += (size_t)B * 64;
    w.v2 = p; p += (size_t)B * 64;
    w.inv1 = p; p += B;
    w.inv2 = p; p += B;
    w.ttl_part = p; p += (size_t)NCE_SPLIT * B;
    w.ttl = p; p += B;
    w.lossi = p; p += B;
    w.d1 = p; p += (size_t)NCE_SPLIT * B * 64;
    w.d2 = p;
    return w;
}

// one 16-lane group per batch row: gather, L2-normalise (x / max(||x||, 1e-12))
__global__ __launch_bounds__(256) void nce_prep_kernel(const float* __restrict__ E1,
                                                       const float* __restrict__ E2,
                                                       const int64_t* __restrict__ ids, int B,
                                                       float* __restrict__ v1, float* __restrict__ v2,
                                                       float* __restrict__ inv1, float* __restrict__ inv2) {
    const int lane16 = threadIdx.x & 15;
    const int b = blockIdx.x * 16 + (threadIdx.x >> 4);
    if (b >= B) return;
    const size_t r = (size_t)ids[b] * 16 + lane16;
    const float4 a = reinterpret_cast<const float4*>(E1)[r], c = reinterpret_cast<const float4*>(E2)[r];
    const float na = sqrtf(row16_sum(f4_dot(a, a))), nc = sqrtf(row16_sum(f4_dot(c, c)));
    const float ia = 1.0f / fmaxf(na, 1e-12f), ic = 1.0f / fmaxf(nc, 1e-12f);
    reinterpret_cast<float4*>(v1)[(size_t)b * 16 + lane16] = f4_scale(ia, a);
    reinterpret_cast<float4*>(v2)[(size_t)b * 16 + lane16] = f4_scale(ic, c);
    // sign bit: the clamp was active -- the norm is then a constant of the backward, as in row_normalize_fwd_kernel
    if (lane16 == 0) { inv1[b] = na > 1e-12f ? ia : -ia; inv2[b] = nc > 1e-12f ? ic : -ic; }
}

// MODE 0: own = rows i of view 1, other = columns j of view 2; output ttl_part[split][i]
// MODE 1: own = rows i (view 1), other = j (view 2);          output dOwn_part = sum_j g_ij v2_j
// MODE 2: own = columns j (view 2), other = rows i (view 1);  output dOwn_part = sum_i g_ij v1_i
// grid (ceil(B/64), NCE_SPLIT).  Thread (ty = tid>>4, tx = tid&15) owns own-rows 4ty..+3 and, per
// tile, other-rows 4tx..+3 (logits) / dims 4tx..+3 (gradient accumulation).
template <int MODE>
__global__ __launch_bounds__(256) void nce_sweep_kernel(const float* __restrict__ Vown,
                                                        const float* __restrict__ Voth, int B,
                                                        float inv_tau, const float* __restrict__ ttl,
                                                        const float* __restrict__ gout,
                                                        float* __restrict__ out) {
    __shared__ float A[NCE_T][NCE_LD];   // own rows
    __shared__ float O[NCE_T][NCE_LD];   // other rows of the current tile
    __shared__ float G[NCE_T][NCE_LD];   // g tile (MODE 1, 2)
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    const int a0 = blockIdx.x * NCE_T;
    const int tiles = (B + NCE_T - 1) / NCE_T;
    const int per = (tiles + NCE_SPLIT - 1) / NCE_SPLIT;
    const int t_begin = blockIdx.y * per, t_end = min(t_begin + per, tiles);
    // stage own rows (zero past B)
    for (int e = tid; e < NCE_T * 16; e += 256) {
        const int r = e >> 4, c4 = e & 15;
        const float4 v = a0 + r < B ? reinterpret_cast<const float4*>(Vown)[(size_t)(a0 + r) * 16 + c4] : f4_zero();
        A[r][c4 * 4 + 0] = v.x; A[r][c4 * 4 + 1] = v.y; A[r][c4 * 4 + 2] = v.z; A[r][c4 * 4 + 3] = v.w;
    }
    float rsum[4] = {0.f, 0.f, 0.f, 0.f};
    float dacc[4][4] = {};
    float own_ttl[4] = {1.f, 1.f, 1.f, 1.f};
    if (MODE == 1) {
#pragma unroll
        for (int u = 0; u < 4; ++u) own_ttl[u] = a0 + 4 * ty + u < B ? ttl[a0 + 4 * ty + u] : 1.f;
    }
    const float gscale = MODE == 0 ? 0.f : gout[0] * inv_tau / (float)B;
    for (int t = t_begin; t < t_end; ++t) {
        const int b0 = t * NCE_T;
        __syncthreads();   // previous tile fully consumed (also orders the A staging the first time)
        for (int e = tid; e < NCE_T * 16; e += 256) {
            const int r = e >> 4, c4 = e & 15;
            const float4 v = b0 + r < B ? reinterpret_cast<const float4*>(Voth)[(size_t)(b0 + r) * 16 + c4] : f4_zero();
            O[r][c4 * 4 + 0] = v.x; O[r][c4 * 4 + 1] = v.y; O[r][c4 * 4 + 2] = v.z; O[r][c4 * 4 + 3] = v.w;
        }
        __syncthreads();
        float s[4][4] = {};
#pragma unroll 8
        for (int k = 0; k < 64; ++k) {
            float av[4], ov[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) { av[u] = A[4 * ty + u][k]; ov[u] = O[4 * tx + u][k]; }
#pragma unroll
            for (int u = 0; u < 4; ++u)
#pragma unroll
                for (int w = 0; w < 4; ++w) s[u][w] = fmaf(av[u], ov[w], s[u][w]);
        }
        // e = exp(s / tau) for valid (own, other) pairs
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int ga = a0 + 4 * ty + u;
#pragma unroll
            for (int w = 0; w < 4; ++w) {
                const int gb = b0 + 4 * tx + w;
                const bool ok = ga < B && gb < B;
                const float e = ok ? expf(s[u][w] * inv_tau) : 0.f;
                if (MODE == 0) {
                    rsum[u] += e;
                } else {
                    // row index of the softmax: the view-1 index (own in MODE 1, other in MODE 2)
                    const float tt = MODE == 1 ? own_ttl[u] : (gb < B ? ttl[gb] : 1.f);
                    const float g = ok ? gscale * (e / tt - (ga == gb ? 1.f : 0.f)) : 0.f;
                    G[4 * ty + u][4 * tx + w] = g;
                }
            }
        }
        if (MODE != 0) {
            __syncthreads();
            // dOwn[4ty+u][4tx+w] += sum_b G[4ty+u][b] * O[b][4tx+w]
#pragma unroll 8
            for (int b = 0; b < NCE_T; ++b) {
                float gv[4], ov[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) { gv[u] = G[4 * ty + u][b]; ov[u] = O[b][4 * tx + u]; }
#pragma unroll
                for (int u = 0; u < 4; ++u)
#pragma unroll
                    for (int w = 0; w < 4; ++w) dacc[u][w] = fmaf(gv[u], ov[w], dacc[u][w]);
            }
        }
    }
    if (MODE == 0) {
        // row sums over this split: reduce the 16 tx lanes of each ty group (lanes are consecutive)
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const float r = row16_sum(rsum[u]);
            const int ga = a0 + 4 * ty + u;
            if (tx == 0 && ga < B) out[(size_t)blockIdx.y * B + ga] = r;
        }
    } else {
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int ga = a0 + 4 * ty + u;
            if (ga < B)
                reinterpret_cast<float4*>(out + ((size_t)blockIdx.y * B + ga) * 64)[tx] =
                    make_float4(dacc[u][0], dacc[u][1], dacc[u][2], dacc[u][3]);
        }
    }
}

// ttl_i = sum of the split partials (fixed order); loss_i = log(ttl_i) - <v1_i, v2_i> / tau
__global__ __launch_bounds__(256) void nce_finish_kernel(const float* __restrict__ v1,
                                                         const float* __restrict__ v2, int B,
                                                         float inv_tau, const float* __restrict__ ttl_part,
                                                         float* __restrict__ ttl, float* __restrict__ lossi) {
    const int lane16 = threadIdx.x & 15;
    const int b = blockIdx.x * 16 + (threadIdx.x >> 4);
    if (b >= B) return;
    const float4 a = reinterpret_cast<const float4*>(v1)[(size_t)b * 16 + lane16];
    const float4 c = reinterpret_cast<const float4*>(v2)[(size_t)b * 16 + lane16];
    const float dot = row16_sum(f4_dot(a, c));
    if (lane16 == 0) {
        float t = 0.f;
        for (int s = 0; s < NCE_SPLIT; ++s) t += ttl_part[(size_t)s * B + b];
        ttl[b] = t;
        // -log(exp(dot/tau) / t), evaluated the way the reference does (exp, divide, log)
        lossi[b] = -logf(expf(dot * inv_tau) / t);
    }
}

__global__ __launch_bounds__(256) void nce_reduce_kernel(const float* __restrict__ v, int n, float scale,
                                                         float* __restrict__ out) {
    __shared__ float red[256];
    float t = 0.f;
    for (int i = threadIdx.x; i < n; i += 256) t += v[i];
    red[threadIdx.x] = t;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x == 0) out[0] = scale * red[0];
}

// dE[id] += (dvn - vn <vn, dvn>) * inv_norm   with dvn = sum of the split partials (fixed order); a row below F.normalize's
// clamp (0 < ||x|| <= 1e-12) was divided by the constant 1e-12: dE[id] += dvn * 1e12, as autograd of F.normalize gives
__global__ __launch_bounds__(256) void nce_scatter_kernel(const float* __restrict__ vn,
                                                          const float* __restrict__ inv,
                                                          const float* __restrict__ dpart,
                                                          const int64_t* __restrict__ ids, int B,
                                                          float* __restrict__ dE) {
    const int lane16 = threadIdx.x & 15;
    const int b = blockIdx.x * 16 + (threadIdx.x >> 4);
    if (b >= B) return;
    const float4 x = reinterpret_cast<const float4*>(vn)[(size_t)b * 16 + lane16];
    float4 d = f4_zero();
    for (int s = 0; s < NCE_SPLIT; ++s)
        d = f4_add(d, reinterpret_cast<const float4*>(dpart + ((size_t)s * B + b) * 64)[lane16]);
    const float dot = row16_sum(f4_dot(x, d));
    const float proj = inv[b] > 0.f ? dot : 0.f;       // clamp active (sign bit, nce_prep_kernel): x / 1e-12, nothing to project out
    const float iv = fabsf(inv[b]);
    float* dst = dE + (size_t)ids[b] * 64 + lane16 * 4;
    unsafeAtomicAdd(dst + 0, (d.x - x.x * proj) * iv);
    unsafeAtomicAdd(dst + 1, (d.y - x.y * proj) * iv);
    unsafeAtomicAdd(dst + 2, (d.z - x.z * proj) * iv);
    unsafeAtomicAdd(dst + 3, (d.w - x.w * proj) * iv);
}

}  // namespace

extern "C" size_t mmrec_infonce_workspace_bytes(int32_t batch) {
    return batch > 0 ? nce_ws_floats(batch) * sizeof(float) : 0;
}

extern "C" int mmrec_infonce_fwd_f32(const float* E1, const float* E2, const int64_t* ids,
                                     int32_t batch, int32_t d, float tau, float* loss, void* workspace,
                                     mmrec_stream_t stream) {
    if (d != 64) return MMREC_ERR_UNSUPPORTED;
    if (batch <= 0 || !(tau > 0.f)) return MMREC_ERR_BAD_ARG;
    if (!E1 || !E2 || !ids || !loss || !workspace) return MMREC_ERR_BAD_ARG;
    hipStream_t s = mmrec_stream(stream);
    const NceWs w = nce_ws(workspace, batch);
    const int g16 = (batch + 15) / 16, gt = (batch + NCE_T - 1) / NCE_T;
    hipLaunchKernelGGL(nce_prep_kernel, dim3(g16), dim3(256), 0, s, E1, E2, ids, batch, w.v1, w.v2, w.inv1,
                       w.inv2);
    hipLaunchKernelGGL(nce_sweep_kernel<0>, dim3(gt, NCE_SPLIT), dim3(256), 0, s, w.v1, w.v2, batch,
                       1.0f / tau, (const float*)nullptr, (const float*)nullptr, w.ttl_part);
    hipLaunchKernelGGL(nce_finish_kernel, dim3(g16), dim3(256), 0, s, w.v1, w.v2, batch, 1.0f / tau,
                       w.ttl_part, w.ttl, w.lossi);
    hipLaunchKernelGGL(nce_reduce_kernel, dim3(1), dim3(256), 0, s, w.lossi, batch, 1.0f / batch, loss);
    MMREC_RETURN_LAUNCH_STATUS();
}

// `workspace` must be the buffer the forward call filled.  dE1 / dE2 are accumulated into (zero or
// pre-filled by the caller); either may be null.
extern "C" int mmrec_infonce_bwd_f32(const int64_t* ids, int32_t batch, int32_t d, float tau,
                                     const float* grad_loss, float* dE1, float* dE2, void* workspace,
                                     mmrec_stream_t stream) {
    if (d != 64) return MMREC_ERR_UNSUPPORTED;
    if (batch <= 0 || !(tau > 0.f)) return MMREC_ERR_BAD_ARG;
    if (!ids || !grad_loss || !workspace) return MMREC_ERR_BAD_ARG;
    hipStream_t s = mmrec_stream(stream);
    const NceWs w = nce_ws(workspace, batch);
    const int g16 = (batch + 15) / 16, gt = (batch + NCE_T - 1) / NCE_T;
    if (dE1) {
        hipLaunchKernelGGL(nce_sweep_kernel<1>, dim3(gt, NCE_SPLIT), dim3(256), 0, s, w.v1, w.v2, batch,
                           1.0f / tau, w.ttl, grad_loss, w.d1);
        hipLaunchKernelGGL(nce_scatter_kernel, dim3(g16), dim3(256), 0, s, w.v1, w.inv1, w.d1, ids, batch, dE1);
    }
    if (dE2) {
        hipLaunchKernelGGL(nce_sweep_kernel<2>, dim3(gt, NCE_SPLIT), dim3(256), 0, s, w.v2, w.v1, batch,
                           1.0f / tau, w.ttl, grad_loss, w.d2);
        hipLaunchKernelGGL(nce_scatter_kernel, dim3(g16), dim3(256), 0, s, w.v2, w.inv2, w.d2, ids, batch, dE2);
    }
    MMREC_RETURN_LAUNCH_STATUS();
}
