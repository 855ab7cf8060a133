// MMGCN's 64-wide layer (include/mmrec_hip.h, additive to ABI 16): everything one layer of mmgcn.py's GCN.forward does, given
// AX = spmm(graph, x) -- the aggregation is linear, spmm(graph, x Wc) = AX Wc -- over all n = users + items rows in ONE launch, and
// the backward in two (the main pass + the weight gradients' finish).  fp32 throughout, VALU fma (tile64.h).
//
// Per row (Wc [64][64] as [in][out]; Wl [64][64] and Wg = [Gh | Gx] [64][128] as torch's [out][in]; R the id embedding or NULL):
//     a = AX Wc, h = leaky(a);   p = X Wl^T + bl, xh = leaky(p) + R;   q = h Gh^T + xh Gx^T + bg;   out = leaky(q)
//
// THE PLAN (what the fuzz's error bound counts) is tile64.h's: blocks of R = mmrec_gcn_layer_rows_per_block(n) rows, stage,
// weight partials, column sums, finish.  This op's own:
//   stage   a: over the input column from 0;  p: from bl;  q: over h's column from bg and ON, over xh's column: 128 roundings.
//   leaky(z) = z > 0 ? z : slope * z;  xh = leaky(p) + R is one addition (R NULL: none).
// Backward from g [n, 64] and the saved out, a, h, p, xh RECOMPUTED as above; dq = g * (out > 0 ? 1 : slope): the sign of out is
// the sign of q.  The PHASE LOOP IS OUTERMOST inside the workgroup, as the head loop of encoder_heads.hip: two matrices in LDS,
// the block's tiles walked, then the other two.
//   conv    Wc, Gh:  dh = the stage of dq Gh over the output column from 0;  da = dh * (a > 0 ? 1 : slope);
//           dAX = the stage of da Wc^T over the output column from 0;  dWc[k][o] = one fma chain over the block's rows in order
//           (AX^T da), dGh[o][k] alike (dq^T h);  dbg: the column sums of dq.
//   skip    Wl, Gx:  dxh = the stage of dq Gx over the output column from 0 = dR;  dp = dxh * (p > 0 ? 1 : slope);
//           dX = the stage of dp Wl over the output column from 0;  dWl[o][k] alike (dp^T X), dGx[o][k] alike (dq^T xh);
//           dbl: the column sums of dp.
// Rows past n are zero in every tile of AX, X, g (so dq, and every term they add to a sum, is an exact zero).
// Workspace: per block 4 (64 64) + 2 (64) = 16,512 floats: [dWc][dGh][dWl][dGx][dbg][dbl].
// LDS: forward 4 matrices + 4 tiles, backward 2 matrices + 6 tiles of 17,408 B, + 512 B of biases: 139,776 B both.
#include "tile64.h"

namespace {

constexpr int GL_D = 64;
constexpr int GL_W = GL_D * GL_D;
constexpr int GL_PART = 4 * GL_W + 2 * GL_D;                // floats of one block's partial
constexpr int GL_VEC = 2 * GL_D;                            // bl, bg in LDS
constexpr int GL_IMAGES = 8;                                // matrices + tiles, forward and backward alike
constexpr size_t GL_LDS = sizeof(float) * ((size_t)GL_IMAGES * T64_FLOATS + GL_VEC);

__device__ __forceinline__ float4 gl_leaky4(const float4 z, float slope) {
    return make_float4(t64_leaky(z.x, slope), t64_leaky(z.y, slope), t64_leaky(z.z, slope), t64_leaky(z.w, slope));
}
// dz = dy * (z > 0 ? 1 : slope)
__device__ __forceinline__ void gl_dleaky4(float4& dy, const float4 z, float slope) {
    dy.x *= t64_dleaky(z.x, slope);
    dy.y *= t64_dleaky(z.y, slope);
    dy.z *= t64_dleaky(z.z, slope);
    dy.w *= t64_dleaky(z.w, slope);
}

// dq of the thread's rows in layout L0: g * (out > 0 ? 1 : slope); rows past n are zeros
__device__ __forceinline__ void gl_dq(float4 (&dq)[4], const float* __restrict__ g, const float* __restrict__ out, long row0,
                                      long n, int rg, int sg, float slope) {
    float4 o[4];
    t64_rows(dq, g, row0, n, rg, sg);
    t64_rows(o, out, row0, n, rg, sg);
#pragma unroll
    for (int i = 0; i < 4; ++i) gl_dleaky4(dq[i], o[i], slope);
}

// p (layout L1: rows 4 rg + i, columns sg + 16 j) from the X tile, and xh = leaky(p) + R.  A row past n gets NO addition:
// adding a zero in R's place would turn a -0 into +0
__device__ __forceinline__ void gl_skip(const float* __restrict__ Xr, const float* __restrict__ LWl, const float* __restrict__ vec,
                                        const float* __restrict__ R, long row0, long n, int rg, int sg, float slope,
                                        float (&p)[4][4], float (&xh)[4][4]) {
    t64_start1(p, vec, sg);
    t64_stage_nt(Xr, LWl, rg, sg, p);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const long r = row0 + 4 * rg + i;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            xh[i][j] = t64_leaky(p[i][j], slope);
            if (R && r < n) xh[i][j] += R[(size_t)r * GL_D + sg + 16 * j];
        }
    }
}

__global__ __launch_bounds__(T64_BLOCK) void gcn_layer_fwd_kernel(
    const float* __restrict__ AX, const float* __restrict__ X, const float* __restrict__ R, const float* __restrict__ Wc,
    const float* __restrict__ Wl, const float* __restrict__ bl, const float* __restrict__ Wg, const float* __restrict__ bg, long n,
    int tiles, float slope, float* __restrict__ out) {
    extern __shared__ float4 s_gl[];
    float* LWc = reinterpret_cast<float*>(s_gl);
    float* LWl = LWc + T64_FLOATS;
    float* LGh = LWl + T64_FLOATS;
    float* LGx = LGh + T64_FLOATS;
    float* vec = LGx + T64_FLOATS;           // bl, bg
    float* At = vec + GL_VEC;                // AX transposed
    float* Xr = At + T64_FLOATS;
    float* Hr = Xr + T64_FLOATS;             // h row-major
    float* XHr = Hr + T64_FLOATS;            // xh row-major
    const int rg = threadIdx.x / 16, sg = threadIdx.x % 16;
    t64_matrix(LWc, Wc);
    t64_matrix(LWl, Wl);
    t64_matrix_ld(LGh, Wg, 2 * GL_D);
    t64_matrix_ld(LGx, Wg + GL_D, 2 * GL_D);
    if (threadIdx.x < GL_VEC) vec[threadIdx.x] = threadIdx.x < GL_D ? bl[threadIdx.x] : bg[threadIdx.x - GL_D];
    for (int t = 0; t < tiles; ++t) {
        const long row0 = t64_row0(t, tiles);
        if (row0 >= n) break;
        {
            float4 v[4];
            t64_rows(v, AX, row0, n, rg, sg);
            t64_put_t(At, rg, sg, v);
        }
        t64_load(Xr, X, row0, n, rg, sg);
        __syncthreads();
        {
            float4 a[4];
            t64_zero(a);
            t64_stage_nn(At, LWc, rg, sg, a);
#pragma unroll
            for (int i = 0; i < 4; ++i) a[i] = gl_leaky4(a[i], slope);
            t64_put0(Hr, rg, sg, a);
            float p[4][4], xh[4][4];
            gl_skip(Xr, LWl, vec, R, row0, n, rg, sg, slope, p, xh);
            t64_put(XHr, nullptr, rg, sg, xh);
        }
        __syncthreads();
        float q[4][4];
#pragma unroll
        for (int i = 0; i < 4; ++i)                                          // not t64_start1: 2 more VGPRs, 0.5 % slower
#pragma unroll
            for (int j = 0; j < 4; ++j) q[i][j] = vec[GL_D + sg + 16 * j];
        t64_stage_nt(Hr, LGh, rg, sg, q);
        t64_stage_nt(XHr, LGx, rg, sg, q);
#pragma unroll
        for (int i = 0; i < 4; ++i) {                                        // not t64_store1: leaky is applied in the guard
            const long r = row0 + 4 * rg + i;
            if (r < n) {
#pragma unroll
                for (int j = 0; j < 4; ++j) out[(size_t)r * GL_D + sg + 16 * j] = t64_leaky(q[i][j], slope);
            }
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(T64_BLOCK) void gcn_layer_bwd_kernel(
    const float* __restrict__ AX, const float* __restrict__ X, const float* __restrict__ R, const float* __restrict__ Wc,
    const float* __restrict__ Wl, const float* __restrict__ bl, const float* __restrict__ Wg, const float* __restrict__ out,
    const float* __restrict__ g, long n, int tiles, float slope, float* __restrict__ dAX, float* __restrict__ dX,
    float* __restrict__ dR, float* __restrict__ part) {
    extern __shared__ float4 s_gl[];
    float* M0 = reinterpret_cast<float*>(s_gl);          // Wc, then Wl
    float* M1 = M0 + T64_FLOATS;                         // Gh, then Gx TRANSPOSED
    float* vec = M1 + T64_FLOATS;                        // bl
    float* T0 = vec + GL_VEC;
    float* T1 = T0 + T64_FLOATS;
    float* T2 = T1 + T64_FLOATS;
    float* T3 = T2 + T64_FLOATS;
    float* T4 = T3 + T64_FLOATS;
    float* T5 = T4 + T64_FLOATS;
    const int rg = threadIdx.x / 16, sg = threadIdx.x % 16;
    float* __restrict__ mine = part ? part + (size_t)blockIdx.x * GL_PART : nullptr;

    if (dAX || part) {                                   // ---- the conv phase
        float* At = T0;                                  // AX transposed
        float* Ar = T1;                                  // AX row-major; at the end the column sums of the 16 row groups
        float* Qt = T2;                                  // dq transposed
        float* Qr = T3;                                  // dq row-major
        float* Dr = T4;                                  // da row-major
        float* Hr = T5;                                  // h row-major
        t64_matrix(M0, Wc);
        t64_matrix_ld(M1, Wg, 2 * GL_D);
        float4 ww[4], wg[4];                             // dWc, dGh at [4 rg + i][4 sg .. + 3]
        float cs[1][4] = {{0.f, 0.f, 0.f, 0.f}};         // dbg at the columns 4 sg + j
        t64_zero(ww), t64_zero(wg);
        for (int t = 0; t < tiles; ++t) {
            const long row0 = t64_row0(t, tiles);
            if (row0 >= n) break;
            {
                float4 v[4];
                t64_rows(v, AX, row0, n, rg, sg);
                t64_put_t(At, rg, sg, v);
                t64_put0(Ar, rg, sg, v);
                gl_dq(v, g, out, row0, n, rg, sg, slope);
                t64_put_t(Qt, rg, sg, v);
                t64_put0(Qr, rg, sg, v);
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    cs[0][0] += v[i].x;
                    cs[0][1] += v[i].y;
                    cs[0][2] += v[i].z;
                    cs[0][3] += v[i].w;
                }
            }
            __syncthreads();
            {
                float4 a[4], dh[4];
                t64_zero(a), t64_zero(dh);
                t64_stage_nn(At, M0, rg, sg, a);
                t64_stage_nn(Qt, M1, rg, sg, dh);
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    gl_dleaky4(dh[i], a[i], slope);      // da
                    a[i] = gl_leaky4(a[i], slope);
                }
                t64_put0(Dr, rg, sg, dh);
                t64_put0(Hr, rg, sg, a);
            }
            __syncthreads();
            if (part) {
                t64_stage_nn(Ar, Dr, rg, sg, ww);
                t64_stage_nn(Qr, Hr, rg, sg, wg);
            }
            if (dAX) {
                float acc[4][4];
                t64_zero(acc);
                t64_stage_nt(Dr, M0, rg, sg, acc);
                t64_store1(dAX, row0, n, rg, sg, acc);
            }
            __syncthreads();
        }
        if (part) {
            t64_part_store(mine, rg, sg, ww);
            t64_part_store(mine + GL_W, rg, sg, wg);
            const T64Layout lay[1] = {T64_L0};
            t64_colsum(Ar, rg, sg, lay, cs, mine + 4 * GL_W);
        }
        __syncthreads();                                 // every read of the phase's matrices and column sums is done
    }

    if (dX || dR || part) {                              // ---- the skip phase
        float* Xr = T0;                                  // at the end the column sums of the 16 row groups
        float* Qr = T1;                                  // dq row-major
        float* Pr = T2;                                  // dp row-major
        float* Pt = T3;                                  // dp transposed
        float* XHr = T4;                                 // xh row-major
        t64_matrix(M0, Wl);
        t64_matrix_ld_t(M1, Wg + GL_D, 2 * GL_D);
        if (threadIdx.x < GL_D) vec[threadIdx.x] = bl[threadIdx.x];
        float4 wl[4], wx[4];                             // dWl, dGx at [4 rg + i][4 sg .. + 3]
        float cs[1][4] = {{0.f, 0.f, 0.f, 0.f}};         // dbl at the columns sg + 16 j
        t64_zero(wl), t64_zero(wx);
        for (int t = 0; t < tiles; ++t) {
            const long row0 = t64_row0(t, tiles);
            if (row0 >= n) break;
            t64_load(Xr, X, row0, n, rg, sg);
            {
                float4 v[4];
                gl_dq(v, g, out, row0, n, rg, sg, slope);
                t64_put0(Qr, rg, sg, v);
            }
            __syncthreads();
            {
                float p[4][4], xh[4][4], dxh[4][4];
                gl_skip(Xr, M0, vec, R, row0, n, rg, sg, slope, p, xh);
                t64_zero(dxh);
                t64_stage_nt(Qr, M1, rg, sg, dxh);
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const long r = row0 + 4 * rg + i;
#pragma unroll
                    for (int j = 0; j < 4; ++j) {                            // dR not through t64_store1: 32 more VGPRs
                        if (dR && r < n) dR[(size_t)r * GL_D + sg + 16 * j] = dxh[i][j];
                        dxh[i][j] *= t64_dleaky(p[i][j], slope);             // dp
                        cs[0][j] += dxh[i][j];
                    }
                }
                t64_put(Pr, Pt, rg, sg, dxh);
                t64_put(XHr, nullptr, rg, sg, xh);
            }
            __syncthreads();
            if (part) {
                t64_stage_nn(Pr, Xr, rg, sg, wl);
                t64_stage_nn(Qr, XHr, rg, sg, wx);
            }
            if (dX) {
                float4 acc[4];
                t64_zero(acc);
                t64_stage_nn(Pt, M0, rg, sg, acc);
                t64_store(dX, row0, n, rg, sg, acc);
            }
            __syncthreads();
        }
        if (part) {
            t64_part_store(mine + 2 * GL_W, rg, sg, wl);
            t64_part_store(mine + 3 * GL_W, rg, sg, wx);
            const T64Layout lay[1] = {T64_L1};
            t64_colsum(Xr, rg, sg, lay, cs, mine + 4 * GL_W + GL_D);
        }
    }
}

// t64_finish_sum, and where a partial's float e goes
__global__ __launch_bounds__(T64_BLOCK) void gcn_layer_finish_kernel(const float* __restrict__ part, int nb, float* __restrict__ dWc,
                                                                     float* __restrict__ dWl, float* __restrict__ dbl,
                                                                     float* __restrict__ dWg, float* __restrict__ dbg) {
    int e;                                                     // GL_PART is a multiple of 64: e < GL_PART
    float a;
    if (!t64_finish_sum(part, nb, GL_PART, e, a)) return;
    const int row = (e % GL_W) / GL_D, c = e % GL_D;           // of a matrix partial
    float* dst = nullptr;
    if (e < GL_W) dst = dWc ? dWc + e : nullptr;
    else if (e < 2 * GL_W) dst = dWg ? dWg + row * 2 * GL_D + c : nullptr;
    else if (e < 3 * GL_W) dst = dWl ? dWl + (e - 2 * GL_W) : nullptr;
    else if (e < 4 * GL_W) dst = dWg ? dWg + row * 2 * GL_D + GL_D + c : nullptr;
    else if (e < 4 * GL_W + GL_D) dst = dbg ? dbg + c : nullptr;
    else dst = dbl ? dbl + c : nullptr;
    if (dst) *dst = a;
}

inline bool gl_served(int64_t n, int32_t d, float slope) { return d == GL_D && slope > 0.f && n <= T64_MAX_ROWS; }

}  // namespace

extern "C" int32_t mmrec_gcn_layer_rows_per_block(int64_t n) { return n < 0 || n > T64_MAX_ROWS ? 0 : t64_fuser_rows(n); }

extern "C" size_t mmrec_gcn_layer_workspace_bytes(int64_t n) {
    if (n < 0 || n > T64_MAX_ROWS) return 0;
    return sizeof(float) * (size_t)t64_fuser_blocks(n) * GL_PART;
}

extern "C" int mmrec_gcn_layer_fwd_f32(const float* AX, const float* X, const float* R, const float* Wc, const float* Wl,
                                       const float* bl, const float* Wg, const float* bg, int64_t n, int32_t d, float slope,
                                       float* out, mmrec_stream_t stream) {
    if (!gl_served(n, d, slope)) return MMREC_ERR_UNSUPPORTED;
    if (n < 0) return MMREC_ERR_BAD_ARG;
    if (n == 0) return 0;
    if (!AX || !X || !Wc || !Wl || !bl || !Wg || !bg || !out) return MMREC_ERR_BAD_ARG;
    const int rc = t64_launch<gcn_layer_fwd_kernel>(t64_fuser_blocks(n), GL_LDS, mmrec_stream(stream), AX, X, R, Wc, Wl, bl, Wg, bg,
                                                    (long)n, t64_fuser_rows(n) / T64, slope, out);
    if (rc) return rc;
    MMREC_RETURN_LAUNCH_STATUS();
}

extern "C" int mmrec_gcn_layer_bwd_f32(const float* AX, const float* X, const float* R, const float* Wc, const float* Wl,
                                       const float* bl, const float* Wg, const float* bg, const float* out, const float* g,
                                       int64_t n, int32_t d, float slope, float* dAX, float* dX, float* dR, float* dWc, float* dWl,
                                       float* dbl, float* dWg, float* dbg, void* workspace, mmrec_stream_t stream) {
    if (!gl_served(n, d, slope)) return MMREC_ERR_UNSUPPORTED;
    if (n < 0) return MMREC_ERR_BAD_ARG;
    if (n == 0) return 0;
    const bool want_w = dWc || dWl || dbl || dWg || dbg;
    if (!AX || !X || !Wc || !Wl || !bl || !Wg || !bg || !out || !g || (want_w && !workspace)) return MMREC_ERR_BAD_ARG;
    if (!want_w && !dAX && !dX && !dR) return 0;
    hipStream_t s = mmrec_stream(stream);
    float* part = want_w ? static_cast<float*>(workspace) : nullptr;
    const int nb = t64_fuser_blocks(n);
    const int rc = t64_launch<gcn_layer_bwd_kernel>(nb, GL_LDS, s, AX, X, R, Wc, Wl, bl, Wg, out, g, (long)n, t64_fuser_rows(n) / T64,
                                                    slope, dAX, dX, dR, part);
    if (rc) return rc;
    if (want_w)
        hipLaunchKernelGGL(gcn_layer_finish_kernel, dim3(GL_PART / GL_D), dim3(T64_BLOCK), 0, s, part, nb, dWc, dWl, dbl, dWg, dbg);
    MMREC_RETURN_LAUNCH_STATUS();
}
