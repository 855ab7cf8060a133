// SMORE's spectrum step (include/mmrec_hip.h, additive to ABI 16): rfft of the projected image and text rows, the three
// complex filters (image, text, text x image) and the three irfft -- smore.py:188-206, norm='ortho', d = 64 -- in ONE launch,
// and its backward in two (main pass + the weight gradients' finish).  fp32 throughout, VALU fma with both DFT matrices in LDS.
//
// PACKING.  Bins 0 and 32 of a 64-point real transform are real, so a row's spectrum is exactly 64 floats:
//     slot k (0 <= k <= 32) = re_k,   slot 32 + k (1 <= k <= 31) = im_k.
// Both directions are then [rows, 64] x [64, 64] products with ONE matrix
//     F[n][slot k] = cos(2 pi n k / 64) / 8,   F[n][slot 32 + k] = -sin(2 pi n k / 64) / 8
// (rfft = x F) and its transpose: irfft(P, Q) = (wk * (P, Q)) F^T with wk = 1 for bins 0 and 32 and 2 for the others -- the factor
// is applied in the filter, exactly.  The twiddles come from one 64-entry table of cos(2 pi j / 64) rounded from float64, exact 0
// and +-1 at the quarter points, indexed (n k) & 63; 1 / 8 is a power of two, so an entry of F is the table's entry, scaled exactly.
// The imaginary parts of bins 0 and 32 do not exist in this layout: the two weights that would multiply them are never read, and
// their gradients are written as 0.0.
//
// THE PLAN (what the fuzz's error bound counts).  One 256-thread workgroup per block of R = mmrec_spectrum_rows_per_block(n)
// consecutive rows, walked as R / 64 tiles of 64 rows.  A tile in LDS is TRANSPOSED, T[slot or column][row] with 68-float rows.
//   stage   a [64 rows] x [64, 64] product, tile64.h's t64_stage_nn (F and F^T lie at the tiles' pitch): thread (rg, sg) of
//           16 x 16 owns rows 4 rg .. + 3 and outputs 4 sg .. + 3; per summed
//           index one float4 of the tile, one float4 of the matrix and 16 fma onto accumulators that start at 0, the summed
//           index ascending.  An output therefore meets 64 roundings; the matrix entry's own rounding is counted as 2: S = 66.
//   filter  lane = row, wave w takes the bins w, w + 4, ...; with (a, b) the image and (c, e) the text spectrum of the bin:
//           p3 = fma(-e, b, c a), q3 = fma(e, a, c b);  P = wk fma(-q, wi, p wr), Q = wk fma(p, wi, q wr): two roundings each.
// Forward: stage x F and y F -> filter (in place, the fusion pair over the dead x tile) -> three stages with F^T -> the outputs.
//     ROUNDINGS a term of an output meets: image / text S + 2 + S = 134; fusion (S + S) + 2 + 2 + S = 202 (p3 is a product of
//     two spectra).
// Backward, the spectra RECOMPUTED from x and y (state between the calls: x, y and the weights, nothing else):
//     stage x F, y F;  per given g_k: stage g_k F and wk -> (dP, dQ);  one filter-like pass per (row, bin):
//         dwr += fma(dQ, q, dP p), dwi += fma(dQ, p, -(dP q))           per lane, over the block's tiles in order
//         dp = fma(dQ, wi, dP wr), dq = fma(dQ, wr, -(dP wi))
//         da = fma(dq3, e, fma(dp3, c, dp1)), db = fma(dq3, c, fma(-dp3, e, dq1)), dc, de alike with (a, b) and filter 2
//     then stage (da, db) F^T -> dx and (dc, de) F^T -> dy.
//     ROUNDINGS: dx / dy: the longest term is dp3 c: (S + 2) + S + 2, then the last stage: 3 S + 4 = 202.  A weight gradient's
//     term: image / text S + S + 2 = 134, fusion S + (2 S + 2) + 2 = 202; then R / 64 additions over the block's tiles, 6 of the
//     wave's butterfly, and in the finish ceil(blocks / 64) + 6: the finish gives every one of the 198 sums a wave, lane l adds
//     the blocks l, l + 64, ... in order, then the same butterfly.  NO ATOMICS, every order fixed by n alone.
// A NULL g_k reads as zeros (its stage is skipped), a NULL output is not computed.  Rows past n are zero in every tile and are
// never stored.  Workspace: 198 floats per block.  Nothing is allocated, nothing synchronises.
#include "tile64.h"

namespace {

constexpr int SPC_D = 64;
constexpr int SPC_BINS = SPC_D / 2 + 1;
constexpr int SPC_W = 2 * SPC_BINS;              // floats of one filter's weight: [33][2]
constexpr int SPC_NW = 3 * SPC_W;                // ... and of the three: the partial of a block
constexpr int SPC_MAX_BLOCKS = 1024;             // more rows than 65,536: more tiles per block
constexpr int SPC_W_LDS = 208;                   // the weights in LDS, padded to a float4 multiple
constexpr int SPC_FWD_TILES = 4, SPC_BWD_TILES = 6;
constexpr int SPC_BINS_PER_WAVE = 9;             // wave w of four takes the bins w, w + 4, ...: nine at most

// F, F^T and the tiles, all at the T64_LD pitch, and the weights
constexpr size_t spc_lds_bytes(int tiles) { return sizeof(float) * ((size_t)(2 + tiles) * T64_FLOATS + SPC_W_LDS); }

inline int spc_rows_per_block(int64_t n) { return t64_rows_per_block(n, SPC_MAX_BLOCKS); }
inline int spc_blocks(int64_t n) { return t64_blocks(n, SPC_MAX_BLOCKS); }

// cos(2 pi j / 64) rounded from float64; sin(2 pi j / 64) = cos(2 pi (j - 16) / 64)
__device__ const float SPC_COS[64] = {
    1.f, 0.99518472f, 0.980785251f, 0.956940353f, 0.923879504f, 0.881921291f, 0.831469595f, 0.773010433f,
    0.707106769f, 0.634393275f, 0.555570245f, 0.471396744f, 0.382683426f, 0.290284663f, 0.195090324f, 0.0980171412f,
    0.f, -0.0980171412f, -0.195090324f, -0.290284663f, -0.382683426f, -0.471396744f, -0.555570245f, -0.634393275f,
    -0.707106769f, -0.773010433f, -0.831469595f, -0.881921291f, -0.923879504f, -0.956940353f, -0.980785251f, -0.99518472f,
    -1.f, -0.99518472f, -0.980785251f, -0.956940353f, -0.923879504f, -0.881921291f, -0.831469595f, -0.773010433f,
    -0.707106769f, -0.634393275f, -0.555570245f, -0.471396744f, -0.382683426f, -0.290284663f, -0.195090324f, -0.0980171412f,
    0.f, 0.0980171412f, 0.195090324f, 0.290284663f, 0.382683426f, 0.471396744f, 0.555570245f, 0.634393275f,
    0.707106769f, 0.773010433f, 0.831469595f, 0.881921291f, 0.923879504f, 0.956940353f, 0.980785251f, 0.99518472f};

// F and F^T, and the three weights, into LDS (made visible by the caller's next barrier)
__device__ __forceinline__ void spc_setup(float* __restrict__ F, float* __restrict__ FT, float* __restrict__ W,
                                          const float* __restrict__ w_img, const float* __restrict__ w_txt,
                                          const float* __restrict__ w_fus) {
    for (int e = threadIdx.x; e < SPC_D * SPC_D; e += T64_BLOCK) {
        const int n = e / SPC_D, s = e % SPC_D;
        const int j = (n * (s <= 32 ? s : s - 32)) & 63;
        const float v = s <= 32 ? SPC_COS[j] * 0.125f : -SPC_COS[(j - 16) & 63] * 0.125f;
        F[n * T64_LD + s] = v;
        FT[s * T64_LD + n] = v;
    }
    for (int e = threadIdx.x; e < SPC_NW; e += T64_BLOCK)
        W[e] = e < SPC_W ? w_img[e] : e < 2 * SPC_W ? w_txt[e - SPC_W] : w_fus[e - 2 * SPC_W];
}

// the spectrum's stages all start at zero (t64_stage_nn): into a transposed tile, or to a table
__device__ __forceinline__ void spc_to_tile(float* __restrict__ dst, const float* __restrict__ T, const float* __restrict__ M,
                                            int rg, int sg) {
    float4 acc[4] = {f4_zero(), f4_zero(), f4_zero(), f4_zero()};
    t64_stage_nn(T, M, rg, sg, acc);
    t64_put_t(dst, rg, sg, acc);
}
__device__ __forceinline__ void spc_to_table(float* __restrict__ g, long row0, long n, const float* __restrict__ T,
                                             const float* __restrict__ M, int rg, int sg) {
    float4 acc[4] = {f4_zero(), f4_zero(), f4_zero(), f4_zero()};
    t64_stage_nn(T, M, rg, sg, acc);
    t64_store(g, row0, n, rg, sg, acc);
}

// rows row0 .. + 63 of a [n, 64] table into a transposed tile; rows past n are zeros
__device__ __forceinline__ void spc_rows_to_tile(float* __restrict__ dst, const float* __restrict__ g, long row0, long n, int rg,
                                                 int sg) {
    float4 v[4];
    t64_rows(v, g, row0, n, rg, sg);
    t64_put_t(dst, rg, sg, v);
}

__global__ __launch_bounds__(T64_BLOCK) void spectrum_fwd_kernel(
    const float* __restrict__ x, const float* __restrict__ y, const float* __restrict__ w_img, const float* __restrict__ w_txt,
    const float* __restrict__ w_fus, long n, int tiles, float* __restrict__ out_img, float* __restrict__ out_txt,
    float* __restrict__ out_fus) {
    extern __shared__ float4 s_spc[];
    float* F = reinterpret_cast<float*>(s_spc);
    float* FT = F + T64_FLOATS;
    float* W = FT + T64_FLOATS;
    float* T0 = W + SPC_W_LDS;
    float* T1 = T0 + T64_FLOATS;
    float* T2 = T1 + T64_FLOATS;
    float* T3 = T2 + T64_FLOATS;
    const int rg = threadIdx.x / 16, sg = threadIdx.x % 16;
    const int lane = threadIdx.x % MMREC_WAVE, w = threadIdx.x / MMREC_WAVE;
    spc_setup(F, FT, W, w_img, w_txt, w_fus);
    for (int t = 0; t < tiles; ++t) {
        const long row0 = ((long)blockIdx.x * tiles + t) * T64;
        if (row0 >= n) break;
        spc_rows_to_tile(T0, x, row0, n, rg, sg);
        spc_rows_to_tile(T1, y, row0, n, rg, sg);
        __syncthreads();
        spc_to_tile(T2, T0, F, rg, sg);
        spc_to_tile(T3, T1, F, rg, sg);
        __syncthreads();
        for (int k = w; k < SPC_BINS; k += 4) {
            const bool edge = k == 0 || k == SPC_BINS - 1;
            const int re = k * T64_LD + lane, im = (32 + k) * T64_LD + lane;
            const float wk = edge ? 1.f : 2.f;
            const float a = T2[re], c = T3[re];
            const float b = edge ? 0.f : T2[im], e = edge ? 0.f : T3[im];
            const float wr1 = W[2 * k], wr2 = W[SPC_W + 2 * k], wr3 = W[2 * SPC_W + 2 * k];
            const float wi1 = edge ? 0.f : W[2 * k + 1], wi2 = edge ? 0.f : W[SPC_W + 2 * k + 1];
            const float wi3 = edge ? 0.f : W[2 * SPC_W + 2 * k + 1];
            const float p3 = fmaf(-e, b, c * a), q3 = fmaf(e, a, c * b);
            T2[re] = wk * fmaf(-b, wi1, a * wr1);
            T3[re] = wk * fmaf(-e, wi2, c * wr2);
            T0[re] = wk * fmaf(-q3, wi3, p3 * wr3);
            if (!edge) {
                T2[im] = wk * fmaf(a, wi1, b * wr1);
                T3[im] = wk * fmaf(c, wi2, e * wr2);
                T0[im] = wk * fmaf(p3, wi3, q3 * wr3);
            }
        }
        __syncthreads();
        spc_to_table(out_img, row0, n, T2, FT, rg, sg);
        spc_to_table(out_txt, row0, n, T3, FT, rg, sg);
        spc_to_table(out_fus, row0, n, T0, FT, rg, sg);
        __syncthreads();
    }
}

__global__ __launch_bounds__(T64_BLOCK) void spectrum_bwd_kernel(
    const float* __restrict__ x, const float* __restrict__ y, const float* __restrict__ w_img, const float* __restrict__ w_txt,
    const float* __restrict__ w_fus, const float* __restrict__ g_img, const float* __restrict__ g_txt,
    const float* __restrict__ g_fus, long n, int tiles, float* __restrict__ dx, float* __restrict__ dy,
    float* __restrict__ part) {
    extern __shared__ float4 s_spc[];
    float* F = reinterpret_cast<float*>(s_spc);
    float* FT = F + T64_FLOATS;
    float* W = FT + T64_FLOATS;
    float* T0 = W + SPC_W_LDS;               // x, then g_img, then g_fus
    float* T1 = T0 + T64_FLOATS;             // y, then g_txt, then the fusion filter's (dP, dQ)
    float* T2 = T1 + T64_FLOATS;             // (a, b), then (da, db)
    float* T3 = T2 + T64_FLOATS;             // (c, e), then (dc, de)
    float* T4 = T3 + T64_FLOATS;             // the image filter's (dP, dQ)
    float* T5 = T4 + T64_FLOATS;             // the text filter's
    const int rg = threadIdx.x / 16, sg = threadIdx.x % 16;
    const int lane = threadIdx.x % MMREC_WAVE, w = threadIdx.x / MMREC_WAVE;
    float wacc[SPC_BINS_PER_WAVE][6];
#pragma unroll
    for (int i = 0; i < SPC_BINS_PER_WAVE; ++i)
#pragma unroll
        for (int j = 0; j < 6; ++j) wacc[i][j] = 0.f;
    spc_setup(F, FT, W, w_img, w_txt, w_fus);
    for (int t = 0; t < tiles; ++t) {
        const long row0 = ((long)blockIdx.x * tiles + t) * T64;
        if (row0 >= n) break;
        spc_rows_to_tile(T0, x, row0, n, rg, sg);
        spc_rows_to_tile(T1, y, row0, n, rg, sg);
        __syncthreads();
        spc_to_tile(T2, T0, F, rg, sg);
        spc_to_tile(T3, T1, F, rg, sg);
        __syncthreads();                                  // every read of the x and y tiles is done
        if (g_img) spc_rows_to_tile(T0, g_img, row0, n, rg, sg);
        if (g_txt) spc_rows_to_tile(T1, g_txt, row0, n, rg, sg);
        __syncthreads();
        if (g_img) spc_to_tile(T4, T0, F, rg, sg);
        if (g_txt) spc_to_tile(T5, T1, F, rg, sg);
        __syncthreads();
        if (g_fus) {
            spc_rows_to_tile(T0, g_fus, row0, n, rg, sg);
            __syncthreads();
            spc_to_tile(T1, T0, F, rg, sg);
            __syncthreads();
        }
#pragma unroll
        for (int i = 0; i < SPC_BINS_PER_WAVE; ++i) {
            const int k = w + 4 * i;
            if (k < SPC_BINS) {
                const bool edge = k == 0 || k == SPC_BINS - 1;
                const int re = k * T64_LD + lane, im = (32 + k) * T64_LD + lane;
                const float wk = edge ? 1.f : 2.f;
                const float a = T2[re], c = T3[re];
                const float b = edge ? 0.f : T2[im], e = edge ? 0.f : T3[im];
                const float wr1 = W[2 * k], wr2 = W[SPC_W + 2 * k], wr3 = W[2 * SPC_W + 2 * k];
                const float wi1 = edge ? 0.f : W[2 * k + 1], wi2 = edge ? 0.f : W[SPC_W + 2 * k + 1];
                const float wi3 = edge ? 0.f : W[2 * SPC_W + 2 * k + 1];
                const float dP1 = g_img ? wk * T4[re] : 0.f, dQ1 = g_img && !edge ? wk * T4[im] : 0.f;
                const float dP2 = g_txt ? wk * T5[re] : 0.f, dQ2 = g_txt && !edge ? wk * T5[im] : 0.f;
                const float dP3 = g_fus ? wk * T1[re] : 0.f, dQ3 = g_fus && !edge ? wk * T1[im] : 0.f;
                const float p3 = fmaf(-e, b, c * a), q3 = fmaf(e, a, c * b);
                wacc[i][0] += fmaf(dQ1, b, dP1 * a);
                wacc[i][1] += fmaf(dQ1, a, -(dP1 * b));
                wacc[i][2] += fmaf(dQ2, e, dP2 * c);
                wacc[i][3] += fmaf(dQ2, c, -(dP2 * e));
                wacc[i][4] += fmaf(dQ3, q3, dP3 * p3);
                wacc[i][5] += fmaf(dQ3, p3, -(dP3 * q3));
                const float dp1 = fmaf(dQ1, wi1, dP1 * wr1), dq1 = fmaf(dQ1, wr1, -(dP1 * wi1));
                const float dp2 = fmaf(dQ2, wi2, dP2 * wr2), dq2 = fmaf(dQ2, wr2, -(dP2 * wi2));
                const float dp3 = fmaf(dQ3, wi3, dP3 * wr3), dq3 = fmaf(dQ3, wr3, -(dP3 * wi3));
                T2[re] = fmaf(dq3, e, fmaf(dp3, c, dp1));
                T3[re] = fmaf(dq3, b, fmaf(dp3, a, dp2));
                if (!edge) {
                    T2[im] = fmaf(dq3, c, fmaf(-dp3, e, dq1));
                    T3[im] = fmaf(dq3, a, fmaf(-dp3, b, dq2));
                }
            }
        }
        __syncthreads();
        if (dx) spc_to_table(dx, row0, n, T2, FT, rg, sg);
        if (dy) spc_to_table(dy, row0, n, T3, FT, rg, sg);
        __syncthreads();
    }
    if (part) {
#pragma unroll
        for (int i = 0; i < SPC_BINS_PER_WAVE; ++i) {
            const int k = w + 4 * i;
            if (k < SPC_BINS) {                           // wave uniform
                const bool edge = k == 0 || k == SPC_BINS - 1;
#pragma unroll
                for (int j = 0; j < 6; ++j) {
                    const float v = wave_sum(wacc[i][j]);
                    if (lane == 0)
                        part[(size_t)blockIdx.x * SPC_NW + (j / 2) * SPC_W + 2 * k + (j & 1)] = (edge && (j & 1)) ? 0.f : v;
                }
            }
        }
    }
}

// every one of the 198 sums a wave: lane l adds the blocks l, l + 64, ... in order, then the butterfly
__global__ __launch_bounds__(T64_BLOCK) void spectrum_finish_kernel(const float* __restrict__ part, int nb,
                                                                    float* __restrict__ dw_img, float* __restrict__ dw_txt,
                                                                    float* __restrict__ dw_fus) {
    const int lane = threadIdx.x % MMREC_WAVE;
    const int o = blockIdx.x * (T64_BLOCK / MMREC_WAVE) + threadIdx.x / MMREC_WAVE;
    if (o >= SPC_NW) return;
    float a = 0.f;
    for (int b = lane; b < nb; b += MMREC_WAVE) a += part[(size_t)b * SPC_NW + o];
    a = wave_sum(a);
    float* __restrict__ dw = o < SPC_W ? dw_img : o < 2 * SPC_W ? dw_txt : dw_fus;
    if (lane == 0 && dw) dw[o % SPC_W] = a;
}

}  // namespace

extern "C" int32_t mmrec_spectrum_rows_per_block(int64_t n) { return n < 0 || n > T64_MAX_ROWS ? 0 : spc_rows_per_block(n); }

extern "C" size_t mmrec_spectrum_workspace_bytes(int64_t n) {
    if (n < 0 || n > T64_MAX_ROWS) return 0;
    return sizeof(float) * (size_t)spc_blocks(n) * SPC_NW;
}

extern "C" int mmrec_spectrum_fwd_f32(const float* x, const float* y, const float* w_img, const float* w_txt,
                                      const float* w_fus, int64_t n, int32_t d, float* out_img, float* out_txt, float* out_fus,
                                      mmrec_stream_t stream) {
    if (d != SPC_D || n > T64_MAX_ROWS) return MMREC_ERR_UNSUPPORTED;
    if (n < 0) return MMREC_ERR_BAD_ARG;
    if (n == 0) return 0;
    if (!x || !y || !w_img || !w_txt || !w_fus || !out_img || !out_txt || !out_fus) return MMREC_ERR_BAD_ARG;
    const int rc = t64_launch<spectrum_fwd_kernel>(spc_blocks(n), spc_lds_bytes(SPC_FWD_TILES), mmrec_stream(stream), x, y, w_img,
                                                   w_txt, w_fus, (long)n, spc_rows_per_block(n) / T64, out_img, out_txt, out_fus);
    if (rc) return rc;
    MMREC_RETURN_LAUNCH_STATUS();
}

extern "C" int mmrec_spectrum_bwd_f32(const float* x, const float* y, const float* w_img, const float* w_txt,
                                      const float* w_fus, const float* g_img, const float* g_txt, const float* g_fus, int64_t n,
                                      int32_t d, float* dx, float* dy, float* dw_img, float* dw_txt, float* dw_fus,
                                      void* workspace, mmrec_stream_t stream) {
    if (d != SPC_D || n > T64_MAX_ROWS) return MMREC_ERR_UNSUPPORTED;
    if (n < 0) return MMREC_ERR_BAD_ARG;
    if (n == 0) return 0;
    const bool want_w = dw_img || dw_txt || dw_fus;
    if (!x || !y || !w_img || !w_txt || !w_fus || (want_w && !workspace)) return MMREC_ERR_BAD_ARG;
    if (!want_w && !dx && !dy) return 0;
    hipStream_t s = mmrec_stream(stream);
    float* part = want_w ? static_cast<float*>(workspace) : nullptr;
    const int nb = spc_blocks(n);
    const int rc = t64_launch<spectrum_bwd_kernel>(nb, spc_lds_bytes(SPC_BWD_TILES), s, x, y, w_img, w_txt, w_fus, g_img, g_txt,
                                                   g_fus, (long)n, spc_rows_per_block(n) / T64, dx, dy, part);
    if (rc) return rc;
    if (want_w)
        hipLaunchKernelGGL(spectrum_finish_kernel, dim3((SPC_NW + T64_BLOCK / MMREC_WAVE - 1) / (T64_BLOCK / MMREC_WAVE)),
                           dim3(T64_BLOCK), 0, s, part, nb, dw_img, dw_txt, dw_fus);
    MMREC_RETURN_LAUNCH_STATUS();
}
