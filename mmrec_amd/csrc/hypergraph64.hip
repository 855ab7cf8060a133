// Hypergraph message passing of LGMRec at 64 hyperedges (include/mmrec_hip.h, additive to ABI 16): Clothing's setting, the one
// csrc/hypergraph.hip (1 <= H <= 8, H values in registers) does not serve.  The same assignment and the same HGNN layer
//     lat = P_i^T X,  X' = P_i lat,  U' = P_u lat                                   (lgmrec.py:23-36, 196-216)
// with d = 64 and H = 64 fixed at compile time: every product is a [64 rows] x [64, 64] stage of tile64.h.  fp32 throughout.
//
// THE ASSIGNMENT (one launch each way, 16 lanes per row, a float4 of the row's 64 entries each: lane t holds 4 t .. 4 t + 3)
//     x = (a + g) / tau;  p = exp(x - max x) / sum exp(x - max x);  P = keep ? p * keep / q : p
// The maximum is the lane's four in order, then the butterfly over the row's 16 lanes (distances 8, 4, 2, 1); the sum is
// ((e0 + e1) + e2) + e3 per lane, then the same butterfly (row16_sum).  The contract is hypergraph.hip's word for word: the row
// maximum is subtracted, nothing is drawn here, with a mask the forward also writes p where a second buffer is given (the
// backward needs it: P has lost p at the dropped entries), P == p_soft is refused.
//     s = keep ? dP * keep / q : dP;   d a = p * (s - sum_h p_h s_h) / tau
// The dot product is an fma chain over the lane's four entries from 0, then the butterfly.  All-zero mask row: P = 0, d a = 0.
//
// THE LAYER.  Reduce, finish, row pass -- three launches each way -- on tile64.h's plan for a weight gradient:
//   reduce    one workgroup per block of R = t64_fuser_rows(n) consecutive rows (64 while 256 workgroups cover the side, then
//             more 64-row tiles per workgroup).  Tile after tile, the P tile as T and the V tile as M:
//             acc[h][c] = fma(P[r][h], V[r][c], acc[h][c]) for r ascending over the whole block -- ONE chain of R fmas
//             (t64_stage_nn carried across tiles; rows past n are zeros) -- stored as the block's [64][64] partial.
//   finish    64 workgroups, 64 floats each (t64_finish_sum): thread (quarter, c) adds the blocks quarter, quarter + 4, ... in
//             order from 0, then the four quarters in order: ceil(blocks / 4) + 3 additions.
//             A term of lat[h][c] therefore meets at most  R + ceil(blocks / 4) + 3  roundings.
//   row pass  forward: per 64-row tile, items then users in one launch, lat in LDS for the workgroup's whole walk; the P tile is
//             put transposed and out[r][c] = sum_h P[r][h] lat[h][c] is one chain of 64 fmas from 0, h ascending.
//             backward: lat and dlat in LDS.  dP_i[r][h] is ONE chain of 128 fmas from 0: dX[r][c] lat[h][c] for c ascending,
//             then X[r][c] dlat[h][c] for c ascending (a NULL dX: the second 64 alone).  dP_u[r][h]: 64 fmas over dU lat.
//             dX_prev[r][c] = sum_h P_i[r][h] dlat[h][c] as the forward.
// Backward of a layer: dlat = P_i^T dX + P_u^T dU is the same reduce over the item blocks, then the user blocks, in one launch
// (a NULL gradient adds no blocks) and the same finish over all of them.
// NO ATOMICS; every order is a function of the row counts alone.  Workspace: 4096 floats (dlat) + one 4096-float partial per
// block of either side.  Nothing is allocated, nothing synchronises.
#include "tile64.h"

namespace {

constexpr int H64_MAT = T64 * T64;               // floats of lat, dlat and of a block's partial
constexpr int H64_GROUP = 16;                    // lanes per row of the assignment
constexpr int H64_GROUPS = T64_BLOCK / H64_GROUP;
constexpr int H64_ASSIGN_BLOCKS = 2048;          // grid caps; the loops stride the rest
constexpr int H64_ROW_BLOCKS = 512;
constexpr size_t H64_BWD_LDS = sizeof(float) * 4 * T64_FLOATS;

// ------------------------------------------------------------------------------------------------ the assignment
__device__ __forceinline__ float row16_max(float v) {
    v = fmaxf(v, lane_xor_f<8>(v));
    v = fmaxf(v, lane_xor_f<4>(v));
    v = fmaxf(v, lane_xor_f<2>(v));
    v = fmaxf(v, lane_xor_f<1>(v));
    return v;
}

__global__ __launch_bounds__(T64_BLOCK) void hyper64_assign_fwd_kernel(
    const float4* __restrict__ logits, const float4* __restrict__ noise, const float4* __restrict__ keep, long n, float tau,
    float q, float4* __restrict__ P, float4* __restrict__ p_soft) {
    const int t = threadIdx.x % H64_GROUP;
    const long stride = (long)gridDim.x * H64_GROUPS;
    for (long r = (long)blockIdx.x * H64_GROUPS + threadIdx.x / H64_GROUP; r < n; r += stride) {
        const size_t o = (size_t)r * H64_GROUP + t;
        const float4 a = logits[o], g = noise[o];
        float4 x = make_float4((a.x + g.x) / tau, (a.y + g.y) / tau, (a.z + g.z) / tau, (a.w + g.w) / tau);
        const float m = row16_max(fmaxf(fmaxf(fmaxf(x.x, x.y), x.z), x.w));
        x = make_float4(expf(x.x - m), expf(x.y - m), expf(x.z - m), expf(x.w - m));
        const float sum = row16_sum(((x.x + x.y) + x.z) + x.w);
        const float4 p = make_float4(x.x / sum, x.y / sum, x.z / sum, x.w / sum);
        if (p_soft) p_soft[o] = p;
        if (keep) {
            const float4 k = keep[o];
            P[o] = make_float4(p.x * k.x / q, p.y * k.y / q, p.z * k.z / q, p.w * k.w / q);
        } else {
            P[o] = p;
        }
    }
}

__global__ __launch_bounds__(T64_BLOCK) void hyper64_assign_bwd_kernel(
    const float4* __restrict__ p_soft, const float4* __restrict__ keep, const float4* __restrict__ dP, long n, float tau, float q,
    float4* __restrict__ dlogits) {
    const int t = threadIdx.x % H64_GROUP;
    const long stride = (long)gridDim.x * H64_GROUPS;
    for (long r = (long)blockIdx.x * H64_GROUPS + threadIdx.x / H64_GROUP; r < n; r += stride) {
        const size_t o = (size_t)r * H64_GROUP + t;
        const float4 p = p_soft[o];
        float4 s = dP[o];
        if (keep) {
            const float4 k = keep[o];
            s = make_float4(s.x * k.x / q, s.y * k.y / q, s.z * k.z / q, s.w * k.w / q);
        }
        const float dot = row16_sum(fmaf(p.w, s.w, fmaf(p.z, s.z, fmaf(p.y, s.y, fmaf(p.x, s.x, 0.f)))));
        dlogits[o] = make_float4(p.x * (s.x - dot) / tau, p.y * (s.y - dot) / tau, p.z * (s.z - dot) / tau, p.w * (s.w - dot) / tau);
    }
}

// ------------------------------------------------------------------------------------------------ reduce, finish
// part[block][h][c] = sum over the block's rows r, in order, of P[r][h] V[r][c]; blocks [0, nb_a) walk side a, the rest side b
__global__ __launch_bounds__(T64_BLOCK) void hyper64_reduce_kernel(
    const float* __restrict__ P_a, const float* __restrict__ V_a, long n_a, int tiles_a, int nb_a, const float* __restrict__ P_b,
    const float* __restrict__ V_b, long n_b, int tiles_b, float* __restrict__ part) {
    __shared__ float4 s_tiles[2 * T64_FLOATS / 4];
    float* T = reinterpret_cast<float*>(s_tiles);
    float* M = T + T64_FLOATS;
    const bool a = (int)blockIdx.x < nb_a;
    const float* __restrict__ P = a ? P_a : P_b;
    const float* __restrict__ V = a ? V_a : V_b;
    const long n = a ? n_a : n_b;
    const int tiles = a ? tiles_a : tiles_b;
    const long first = (long)(a ? blockIdx.x : blockIdx.x - nb_a) * tiles * T64;
    const int rg = threadIdx.x / 16, sg = threadIdx.x % 16;
    float4 acc[4], pv[4], vv[4];
    t64_zero(acc);
    t64_rows(pv, P, first, n, rg, sg);
    t64_rows(vv, V, first, n, rg, sg);
    for (int t = 0; t < tiles && first + (long)t * T64 < n; ++t) {
        __syncthreads();                                     // the previous stage has read the tiles
        t64_put0(T, rg, sg, pv);
        t64_put0(M, rg, sg, vv);
        __syncthreads();
        if (t + 1 < tiles) {                                 // the next tile's rows are in flight during the stage
            t64_rows(pv, P, first + (long)(t + 1) * T64, n, rg, sg);
            t64_rows(vv, V, first + (long)(t + 1) * T64, n, rg, sg);
        }
        t64_stage_nn(T, M, rg, sg, acc);
    }
    t64_part_store(part + (size_t)blockIdx.x * H64_MAT, rg, sg, acc);
}

__global__ __launch_bounds__(T64_BLOCK) void hyper64_finish_kernel(const float* __restrict__ part, int nb, float* __restrict__ out) {
    int o;
    float a;
    if (t64_finish_sum(part, nb, H64_MAT, o, a)) out[o] = a;
}

// ------------------------------------------------------------------------------------------------ the row passes
// tiles [0, ceil(I / 64)): X_out = P_i lat; the rest: U_out = P_u lat (U = 0 where U_out is not wanted)
__global__ __launch_bounds__(T64_BLOCK) void hyper64_rows_fwd_kernel(
    const float* __restrict__ P_i, long I, float* __restrict__ X_out, const float* __restrict__ P_u, long U,
    float* __restrict__ U_out, const float* __restrict__ lat) {
    __shared__ float4 s_tiles[2 * T64_FLOATS / 4];
    float* LAT = reinterpret_cast<float*>(s_tiles);
    float* T = LAT + T64_FLOATS;
    const int rg = threadIdx.x / 16, sg = threadIdx.x % 16;
    t64_matrix(LAT, lat);
    const long ti = (I + T64 - 1) / T64, tu = (U + T64 - 1) / T64;
    for (long t = blockIdx.x; t < ti + tu; t += gridDim.x) {
        const bool item = t < ti;
        const float* __restrict__ P = item ? P_i : P_u;
        float* __restrict__ out = item ? X_out : U_out;
        const long n = item ? I : U, row0 = (item ? t : t - ti) * T64;
        float4 v[4], acc[4];
        t64_rows(v, P, row0, n, rg, sg);
        __syncthreads();                                     // lat is in LDS; the previous stage has read T
        t64_put_t(T, rg, sg, v);
        __syncthreads();
        t64_zero(acc);
        t64_stage_nn(T, LAT, rg, sg, acc);
        t64_store(out, row0, n, rg, sg, acc);
    }
}

// item tiles: dP_i and dX_prev; user tiles: dP_u.  A NULL dX / dU reads as zeros (its stage is skipped: it would add exact zeros),
// a NULL output is not written and its work is skipped.
__global__ __launch_bounds__(T64_BLOCK) void hyper64_rows_bwd_kernel(
    const float* __restrict__ P_i, const float* __restrict__ X, const float* __restrict__ dX, long I, float* dP_i,
    float* __restrict__ dX_prev, const float* __restrict__ dU, long U, float* dP_u, const float* __restrict__ lat,
    const float* __restrict__ dlat) {
    extern __shared__ float4 s_h64[];
    float* LAT = reinterpret_cast<float*>(s_h64);
    float* DLAT = LAT + T64_FLOATS;
    float* TA = DLAT + T64_FLOATS;
    float* TB = TA + T64_FLOATS;
    const int rg = threadIdx.x / 16, sg = threadIdx.x % 16;
    t64_matrix(LAT, lat);
    t64_matrix(DLAT, dlat);
    const long ti = (I + T64 - 1) / T64, tu = (U + T64 - 1) / T64;
    for (long t = blockIdx.x; t < ti + tu; t += gridDim.x) {
        const bool item = t < ti;
        const long n = item ? I : U, row0 = (item ? t : t - ti) * T64;
        const float* __restrict__ g = item ? dX : dU;
        float* dP = item ? dP_i : dP_u;
        __syncthreads();                                     // lat and dlat are in LDS; the previous stages have read TA and TB
        if (dP) {
            if (g) t64_load(TA, g, row0, n, rg, sg);
            if (item) t64_load(TB, X, row0, n, rg, sg);
            __syncthreads();
            float acc[4][4];
            t64_zero(acc);
            if (g) t64_stage_nt(TA, LAT, rg, sg, acc);
            if (item) t64_stage_nt(TB, DLAT, rg, sg, acc);
            t64_store1(dP, row0, n, rg, sg, acc);
        }
        if (item && dX_prev) {
            float4 v[4], acc[4];
            t64_rows(v, P_i, row0, n, rg, sg);
            __syncthreads();                                 // the dot products have read TA
            t64_put_t(TA, rg, sg, v);
            __syncthreads();
            t64_zero(acc);
            t64_stage_nn(TA, DLAT, rg, sg, acc);
            t64_store(dX_prev, row0, n, rg, sg, acc);
        }
    }
}

// ------------------------------------------------------------------------------------------------ launches
inline int h64_grid(long items, int per_block, int cap) {
    const long b = (items + per_block - 1) / per_block;
    return (int)(b < cap ? b : cap);
}
inline int h64_row_grid(long I, long U) {                     // one workgroup per 64-row tile of either side up to the cap
    const long t = (I + T64 - 1) / T64 + (U + T64 - 1) / T64;
    return (int)(t < H64_ROW_BLOCKS ? t : H64_ROW_BLOCKS);
}

inline void h64_launch_reduce(hipStream_t s, const float* P_a, const float* V_a, long n_a, const float* P_b, const float* V_b,
                              long n_b, float* part) {
    const int nb_a = t64_fuser_blocks(n_a), nb_b = t64_fuser_blocks(n_b);
    if (nb_a + nb_b == 0) return;
    hipLaunchKernelGGL(hyper64_reduce_kernel, dim3(nb_a + nb_b), dim3(T64_BLOCK), 0, s, P_a, V_a, n_a, t64_fuser_rows(n_a) / T64, nb_a,
                       P_b, V_b, n_b, t64_fuser_rows(n_b) / T64, part);
}

inline bool h64_rows_ok(int64_t n) { return n <= T64_MAX_ROWS; }

}  // namespace

extern "C" int32_t mmrec_hyper64_rows_per_block(int64_t n) { return n < 0 || !h64_rows_ok(n) ? 0 : t64_fuser_rows(n); }

extern "C" size_t mmrec_hyper64_workspace_bytes(int64_t I, int64_t U) {
    if (I < 0 || U < 0 || !h64_rows_ok(I) || !h64_rows_ok(U)) return 0;
    return sizeof(float) * H64_MAT * ((size_t)1 + t64_fuser_blocks(I) + t64_fuser_blocks(U));
}

extern "C" int mmrec_hyper64_assign_fwd_f32(const float* logits, const float* noise, const float* keep, int64_t n, float tau,
                                            float keep_rate, float* P, float* p_soft, mmrec_stream_t stream) {
    if (n < 0) return MMREC_ERR_BAD_ARG;
    if (!h64_rows_ok(n)) return MMREC_ERR_UNSUPPORTED;
    if (n == 0) return 0;
    if (!logits || !noise || !P || P == p_soft) return MMREC_ERR_BAD_ARG;
    hipLaunchKernelGGL(hyper64_assign_fwd_kernel, dim3(h64_grid(n, H64_GROUPS, H64_ASSIGN_BLOCKS)), dim3(T64_BLOCK), 0,
                       mmrec_stream(stream), reinterpret_cast<const float4*>(logits), reinterpret_cast<const float4*>(noise),
                       reinterpret_cast<const float4*>(keep), (long)n, tau, keep_rate, reinterpret_cast<float4*>(P),
                       reinterpret_cast<float4*>(p_soft));
    MMREC_RETURN_LAUNCH_STATUS();
}

extern "C" int mmrec_hyper64_assign_bwd_f32(const float* p_soft, const float* keep, const float* dP, int64_t n, float tau,
                                            float keep_rate, float* dlogits, mmrec_stream_t stream) {
    if (n < 0) return MMREC_ERR_BAD_ARG;
    if (!h64_rows_ok(n)) return MMREC_ERR_UNSUPPORTED;
    if (n == 0) return 0;
    if (!p_soft || !dP || !dlogits) return MMREC_ERR_BAD_ARG;
    hipLaunchKernelGGL(hyper64_assign_bwd_kernel, dim3(h64_grid(n, H64_GROUPS, H64_ASSIGN_BLOCKS)), dim3(T64_BLOCK), 0,
                       mmrec_stream(stream), reinterpret_cast<const float4*>(p_soft), reinterpret_cast<const float4*>(keep),
                       reinterpret_cast<const float4*>(dP), (long)n, tau, keep_rate, reinterpret_cast<float4*>(dlogits));
    MMREC_RETURN_LAUNCH_STATUS();
}

extern "C" int mmrec_hyper64_layer_fwd_f32(const float* P_i, const float* P_u, const float* X_prev, int64_t I, int64_t U,
                                           float* U_out, float* X_out, float* lat, void* workspace, mmrec_stream_t stream) {
    if (I < 0 || U < 0) return MMREC_ERR_BAD_ARG;
    if (!h64_rows_ok(I) || !h64_rows_ok(U)) return MMREC_ERR_UNSUPPORTED;
    if (!lat || !workspace) return MMREC_ERR_BAD_ARG;
    if (I > 0 && (!P_i || !X_prev || !X_out)) return MMREC_ERR_BAD_ARG;
    if (U_out && U > 0 && !P_u) return MMREC_ERR_BAD_ARG;
    hipStream_t s = mmrec_stream(stream);
    float* part = static_cast<float*>(workspace) + H64_MAT;
    h64_launch_reduce(s, P_i, X_prev, (long)I, nullptr, nullptr, 0L, part);
    hipLaunchKernelGGL(hyper64_finish_kernel, dim3(T64), dim3(T64_BLOCK), 0, s, part, t64_fuser_blocks(I), lat);
    const long rows_u = U_out ? (long)U : 0L;
    if (I + rows_u > 0)
        hipLaunchKernelGGL(hyper64_rows_fwd_kernel, dim3(h64_row_grid(I, rows_u)), dim3(T64_BLOCK), 0, s, P_i, (long)I, X_out, P_u,
                           rows_u, U_out, lat);
    MMREC_RETURN_LAUNCH_STATUS();
}

extern "C" int mmrec_hyper64_layer_bwd_f32(const float* P_i, const float* P_u, const float* X_prev, const float* lat,
                                           const float* dU, const float* dX, int64_t I, int64_t U, float* dP_i, float* dP_u,
                                           float* dX_prev, void* workspace, mmrec_stream_t stream) {
    if (I < 0 || U < 0) return MMREC_ERR_BAD_ARG;
    if (!h64_rows_ok(I) || !h64_rows_ok(U)) return MMREC_ERR_UNSUPPORTED;
    if (!lat || !workspace) return MMREC_ERR_BAD_ARG;
    if (I > 0 && (!P_i || (dP_i && !X_prev))) return MMREC_ERR_BAD_ARG;
    if (U > 0 && dU && !P_u) return MMREC_ERR_BAD_ARG;
    hipStream_t s = mmrec_stream(stream);
    float* dlat = static_cast<float*>(workspace);
    float* part = dlat + H64_MAT;
    const long n_i = dX ? (long)I : 0L, n_u = dU ? (long)U : 0L;             // a NULL gradient adds no blocks: zeros
    h64_launch_reduce(s, P_i, dX, n_i, P_u, dU, n_u, part);
    hipLaunchKernelGGL(hyper64_finish_kernel, dim3(T64), dim3(T64_BLOCK), 0, s, part, t64_fuser_blocks(n_i) + t64_fuser_blocks(n_u),
                       dlat);
    const long rows_i = (dP_i || dX_prev) ? (long)I : 0L, rows_u = dP_u ? (long)U : 0L;
    if (rows_i + rows_u > 0) {
        const int rc = t64_launch<hyper64_rows_bwd_kernel>(
            h64_row_grid(rows_i, rows_u), H64_BWD_LDS, s, P_i, X_prev, dX, rows_i, dP_i, dX_prev, dU, rows_u, dP_u, lat, dlat);
        if (rc) return rc;
    }
    MMREC_RETURN_LAUNCH_STATUS();
}
