// Fused edge attention: scores, softmax over a target's incoming edges and the weighted sum in ONE pass over the edges
// (include/mmrec_hip.h, additive to ABI 16).  For row r of a CSR (rowptr, colidx), slot j at position p = perm ? perm[j] : j of the
// caller's (COO) arrays, exactly as in edge_softmax.hip:
//     s_p = <Q[r], KV[colidx[j]]>,   alpha_p = exp(s_p - m_r) / (sum_q exp(s_q - m_r) + eps),   Y[r] = sum_p alpha_p KV[colidx[j]]
// which was edge_dot -> segment softmax -> SpMM with values: KV[colidx[j]] gathered twice, the scores and the weights each
// written and read back.  Here every source row is gathered ONCE and serves the dot product and the sum.
//
// One 16-lane group owns a row (the access shape of spmm.hip: lane t holds the float4 of columns 4 t ... 4 t + 3 of q, of the
// gathered row and of the accumulator).  A score is 4 roundings in the lane's chain (f4_dot) and 4 in the row16_sum butterfly.
// The softmax is online: the group keeps (m, den, acc); a score above m first multiplies den and acc by exp(m - s), then every
// score adds e = exp(s - m) to den and e * row to acc; a score of -inf has e = 0.
//   group  four rows per wave, 16 per workgroup; rows of at most rg::GROUP_MAX entries, or every row when no list is given.
//   block  one 256-thread workgroup per LISTED row (the list of mmrec_spmm_plan_fill at rg::GROUP_MAX, row_groups.h's one
//          threshold: one list serves every op): group g takes the slots 16 g ... 16 g + 15 of every 256, with its own
//          state; the 16 states go through LDS and are combined in the order g = 0 ... 15 by weights exp(m_g - max m).
// alpha in the caller's order: lane t of the group that handles slots base ... base + 15 PARKS the raw score of slot base + t in
// alpha[p]; after the row the same lane reads it back and writes exp(s - m) / (den + eps) -- written and re-read by one lane,
// so no fence (edge_softmax.hip's rule).  No atomics: the bits of Y and alpha are a function of the inputs and the row lengths.
// A colidx outside [0, n_kv) or a position outside [0, n_edges) is an absent edge: never an address, adds nothing, its alpha
// stays unwritten.  EVERY row of Y is written: zeros for a row without (present) edges.  Non-finite scores follow the
// arithmetic: fmaxf skips a NaN, which then enters den and acc through exp; +inf gives exp(inf - inf) = NaN; a row of nothing
// but -inf has no maximum and is set to NaN (exp(-inf + inf) in its alphas): such a row is NaN in every alpha and in Y[r], no
// other row is touched, and a -inf next to a finite maximum is exactly 0.
//
// Backward (mmrec_edge_attention_bwd_f32), from the forward's alpha and Y, in two passes without atomics:
//     g_p = <dY[r], KV[c]> + dAlpha[p]     t_r = <dY[r], Y[r]> + sum_p alpha_p dAlpha[p]     ds_p = alpha_p (g_p - t_r)
//     dQ[r] = sum_p ds_p KV[c]             dKV[c] = base[c] + sum over the edges of column c of (alpha_p dY[r] + ds_p Q[r])
// t_r = sum_p alpha_p g_p is known BEFORE the row is walked, because sum_p alpha_p <dY[r], KV[c_p]> = <dY[r], Y[r]> (Y was built
// from the same alpha, whatever eps): the dAlpha part is one pass over the row's scalars, never over its 256-byte rows.
//   row pass     the forward's CSR and access shape: one walk gathers each KV[c] once for g and for dQ; lane t of the group that
//                handles slots base ... base + 15 writes ds[p] of slot base + t (0 for an absent edge whose position is valid).
//                A listed row: the 16 groups' dQ states go through LDS and are added in the order g = 0 ... 15, and so are
//                their parts of sum alpha dAlpha.
//   column pass  the transposed CSR (rowptr_t, rowidx_t, perm_t): per slot alpha[p] and ds[p] through perm_t, dY[r] and Q[r]
//                gathered once each; the same group / workgroup split, driven by the column side's list.  base[c] is the first
//                term of the sum.
// Every row of dQ and of dKV is written.  A row id outside [0, n_rows) on the transposed side is an absent edge as well.  A row
// whose alpha is NaN is NaN in its ds, in dQ[r] and in the dKV rows of its columns: the arithmetic's pattern.  Known and
// accepted, as in the forward: a hub of tens of thousands of edges is ONE workgroup in each pass (no chunk plan here).
#include "row_groups.h"

#include <math.h>

namespace {

using rg::slot_pos;

constexpr int ATT_NB = 4;                       // gathers in flight per group and step

struct RowState {
    float m, den;
    float4 acc;
    bool any;                                   // a present edge was seen (uniform over the group)
};

// The slots first ... first + 15, first + stride ..., below end, of one row for one 16-lane group: raw scores parked in alpha,
// the online state updated.  Trip counts and branches are uniform over the group (the shuffles and butterflies need that).
__device__ __forceinline__ void attend_span(int first, int end, int stride, int t, const int32_t* __restrict__ colidx,
                                            const int64_t* __restrict__ perm, int n_edges, float4 q,
                                            const float4* __restrict__ KV4, int n_kv, float* __restrict__ alpha, RowState& st) {
    for (int base = first; base < end; base += stride) {
        const int j = base + t;
        int c = -1, p = -1;
        if (j < end) {
            c = colidx[j];
            p = slot_pos(perm, j, n_edges);
            if (c < 0 || c >= n_kv || p < 0) c = -1;          // an absent edge
        }
        const int cnt = min(rg::LANES, end - base);
        float mine = 0.f;
        for (int k0 = 0; k0 < cnt; k0 += ATT_NB) {
            float4 x[ATT_NB];
            int cs[ATT_NB];
#pragma unroll
            for (int u = 0; u < ATT_NB; ++u) {
                cs[u] = __shfl(c, k0 + u, rg::LANES);           // (-1 beyond cnt: those lanes hold -1)
                x[u] = cs[u] >= 0 ? KV4[(size_t)cs[u] * rg::LANES + t] : f4_zero();
            }
#pragma unroll
            for (int u = 0; u < ATT_NB; ++u) {
                const float s = row16_sum(f4_dot(q, x[u]));
                if (cs[u] < 0) continue;
                st.any = true;
                if (t == k0 + u) mine = s;
                if (s > st.m) {                                 // a new maximum: rescale what was summed under the old one
                    const float sc = expf(st.m - s);            // (m = -inf: 0, and den = acc = 0)
                    st.den *= sc;
                    st.acc = f4_scale(sc, st.acc);
                    st.m = s;
                }
                const float e = s == -INFINITY ? 0.f : expf(s - st.m);     // (-inf before any maximum: not exp(-inf + inf))
                st.den += e;
                st.acc = f4_fma(e, x[u], st.acc);
            }
        }
        if (c >= 0) alpha[p] = mine;                            // parked: this lane reads it back in write_alpha
    }
}

// the lane that parked a slot's score turns it into the weight
__device__ __forceinline__ void write_alpha(int first, int end, int stride, const int32_t* __restrict__ colidx,
                                            const int64_t* __restrict__ perm, int n_edges, int n_kv, float m, float dn,
                                            float* __restrict__ alpha) {
    for (int j = first; j < end; j += stride) {
        const int c = colidx[j];
        const int p = slot_pos(perm, j, n_edges);
        if (c >= 0 && c < n_kv && p >= 0) alpha[p] = expf(alpha[p] - m) / dn;
    }
}

// den + eps; NaN for a row whose present scores are all -inf (no maximum)
__device__ __forceinline__ float att_denominator(float m, float den, float eps) {
    return m == -INFINITY ? __int_as_float(0x7fc00000) : den + eps;
}

__global__ __launch_bounds__(rg::BLOCK) void edge_attention_group_kernel(
    const int32_t* __restrict__ rowptr, int n_rows, const int32_t* __restrict__ colidx, const int64_t* __restrict__ perm,
    bool skip_long, const float4* __restrict__ Q4, const float4* __restrict__ KV4, int n_kv, int n_edges, float eps,
    float4* __restrict__ Y4, float* __restrict__ alpha) {
    rg::for_short_rows(rowptr, n_rows, n_edges, skip_long, [&](long r, int start, int end, int t) {
        RowState st{-INFINITY, 0.f, f4_zero(), false};
        if (end > start)
            attend_span(start, end, rg::LANES, t, colidx, perm, n_edges, Q4[(size_t)r * rg::LANES + t], KV4, n_kv, alpha, st);
        if (!st.any) {
            Y4[(size_t)r * rg::LANES + t] = f4_zero();
            return;
        }
        const float dn = att_denominator(st.m, st.den, eps);
        Y4[(size_t)r * rg::LANES + t] = make_float4(st.acc.x / dn, st.acc.y / dn, st.acc.z / dn, st.acc.w / dn);
        write_alpha(start + t, end, rg::LANES, colidx, perm, n_edges, n_kv, st.m, dn, alpha);
    });
}

__global__ __launch_bounds__(rg::BLOCK) void edge_attention_block_kernel(
    const int32_t* __restrict__ rowptr, int n_rows, const int32_t* __restrict__ colidx, const int64_t* __restrict__ perm,
    const int32_t* __restrict__ long_rows, const float4* __restrict__ Q4, const float4* __restrict__ KV4, int n_kv, int n_edges,
    float eps, float* __restrict__ Y, float* __restrict__ alpha) {
    __shared__ float s_m[rg::GROUPS], s_den[rg::GROUPS], s_any[rg::GROUPS];
    __shared__ float4 s_acc[rg::GROUPS][rg::LANES];
    const int r = long_rows[blockIdx.x];
    if (r < 0 || r >= n_rows) return;                                      // (the whole workgroup)
    int start, end;
    rg::row_span(rowptr, r, n_edges, start, end);
    const int t = threadIdx.x % rg::LANES, g = threadIdx.x / rg::LANES;
    RowState st{-INFINITY, 0.f, f4_zero(), false};
    attend_span(start + g * rg::LANES, end, rg::BLOCK, t, colidx, perm, n_edges, Q4[(size_t)r * rg::LANES + t], KV4, n_kv, alpha, st);
    if (t == 0) {
        s_m[g] = st.m;
        s_den[g] = st.den;
        s_any[g] = st.any ? 1.f : 0.f;
    }
    s_acc[g][t] = st.acc;
    __syncthreads();
    // every thread: the row's maximum, and the 16 denominators under it, added in the order g = 0 ... 15
    float m = -INFINITY, den = 0.f;
    bool any = false;
#pragma unroll
    for (int k = 0; k < rg::GROUPS; ++k) {
        m = fmaxf(m, s_m[k]);
        any = any || s_any[k] != 0.f;
    }
    float w[rg::GROUPS];
#pragma unroll
    for (int k = 0; k < rg::GROUPS; ++k) {
        w[k] = s_m[k] == m ? 1.f : expf(s_m[k] - m);                       // (equal infinities: 1, not exp(inf - inf))
        den = fmaf(s_den[k], w[k], den);
    }
    const float dn = att_denominator(m, den, eps);
    if (threadIdx.x < 4 * rg::LANES) {                                     // the first wave: one column of Y[r] per lane
        const float* col = reinterpret_cast<const float*>(&s_acc[0][0]) + threadIdx.x;
        float y = 0.f;
#pragma unroll
        for (int k = 0; k < rg::GROUPS; ++k) y = fmaf(col[k * 4 * rg::LANES], w[k], y);
        Y[(size_t)r * (4 * rg::LANES) + threadIdx.x] = any ? y / dn : 0.f;
    }
    if (any) write_alpha(start + threadIdx.x, end, rg::BLOCK, colidx, perm, n_edges, n_kv, m, dn, alpha);
}

// ------------------------------------------------------------------------------------------------ backward
// this lane's part of sum_p alpha_p dAlpha_p over the slots first, first + stride, ... of a row (present edges only)
__device__ __forceinline__ float bwd_alpha_dot(int first, int end, int stride, const int32_t* __restrict__ colidx,
                                               const int64_t* __restrict__ perm, int n_edges, int n_kv,
                                               const float* __restrict__ alpha, const float* __restrict__ dAlpha) {
    float acc = 0.f;
    for (int j = first; j < end; j += stride) {
        const int c = colidx[j];
        const int p = slot_pos(perm, j, n_edges);
        if (c >= 0 && c < n_kv && p >= 0) acc = fmaf(alpha[p], dAlpha[p], acc);
    }
    return acc;
}

// The slots first ... first + 15, first + stride ..., below end, of one row for one 16-lane group, with the row's t known:
// ds written, ds_p KV[c] added to acc.  gather: dY or dQ is there (without both no source row is needed).
__device__ __forceinline__ void bwd_row_span(int first, int end, int stride, int t, const int32_t* __restrict__ colidx,
                                             const int64_t* __restrict__ perm, int n_edges, bool has_dy, float4 dy, float tr,
                                             const float4* __restrict__ KV4, int n_kv, bool gather,
                                             const float* __restrict__ alpha, const float* __restrict__ dAlpha,
                                             float* __restrict__ ds, float4& acc) {
    for (int base = first; base < end; base += stride) {
        const int j = base + t;
        int c = -1, p = -1;
        float a = 0.f, da = 0.f;
        if (j < end) {
            c = colidx[j];
            p = slot_pos(perm, j, n_edges);
            if (c < 0 || c >= n_kv || p < 0) c = -1;          // an absent edge
            if (c >= 0) {
                a = alpha[p];
                if (dAlpha) da = dAlpha[p];
            }
        }
        const int cnt = min(rg::LANES, end - base);
        float mine = 0.f;
        for (int k0 = 0; k0 < cnt; k0 += ATT_NB) {
            float4 x[ATT_NB];
            int cs[ATT_NB];
#pragma unroll
            for (int u = 0; u < ATT_NB; ++u) {
                cs[u] = __shfl(c, k0 + u, rg::LANES);
                x[u] = (cs[u] >= 0 && gather) ? KV4[(size_t)cs[u] * rg::LANES + t] : f4_zero();
            }
#pragma unroll
            for (int u = 0; u < ATT_NB; ++u) {
                const float gd = has_dy ? row16_sum(f4_dot(dy, x[u])) : 0.f;
                const float ak = __shfl(a, k0 + u, rg::LANES), dak = __shfl(da, k0 + u, rg::LANES);
                if (cs[u] < 0) continue;
                const float d = ak * ((gd + dak) - tr);
                acc = f4_fma(d, x[u], acc);
                if (t == k0 + u) mine = d;
            }
        }
        if (p >= 0) ds[p] = mine;                              // (0 for an absent edge whose position is valid)
    }
}

__global__ __launch_bounds__(rg::BLOCK) void edge_attention_bwd_rows_group_kernel(
    const int32_t* __restrict__ rowptr, int n_rows, const int32_t* __restrict__ colidx, const int64_t* __restrict__ perm,
    bool skip_long, const float4* __restrict__ KV4, int n_kv, int n_edges, const float4* __restrict__ Y4,
    const float* __restrict__ alpha, const float4* __restrict__ dY4, const float* __restrict__ dAlpha, float* __restrict__ ds,
    float4* __restrict__ dQ4) {
    rg::for_short_rows(rowptr, n_rows, n_edges, skip_long, [&](long r, int start, int end, int t) {
        float4 dy = f4_zero(), acc = f4_zero();
        float tr = 0.f;
        if (dY4) {
            dy = dY4[(size_t)r * rg::LANES + t];
            tr = row16_sum(f4_dot(dy, Y4[(size_t)r * rg::LANES + t]));
        }
        if (end > start) {
            if (dAlpha) tr += row16_sum(bwd_alpha_dot(start + t, end, rg::LANES, colidx, perm, n_edges, n_kv, alpha, dAlpha));
            bwd_row_span(start, end, rg::LANES, t, colidx, perm, n_edges, dY4 != nullptr, dy, tr, KV4, n_kv,
                         dY4 != nullptr || dQ4 != nullptr, alpha, dAlpha, ds, acc);
        }
        if (dQ4) dQ4[(size_t)r * rg::LANES + t] = acc;
    });
}

__global__ __launch_bounds__(rg::BLOCK) void edge_attention_bwd_rows_block_kernel(
    const int32_t* __restrict__ rowptr, int n_rows, const int32_t* __restrict__ colidx, const int64_t* __restrict__ perm,
    const int32_t* __restrict__ long_rows, const float4* __restrict__ KV4, int n_kv, int n_edges, const float4* __restrict__ Y4,
    const float* __restrict__ alpha, const float4* __restrict__ dY4, const float* __restrict__ dAlpha, float* __restrict__ ds,
    float* __restrict__ dQ) {
    __shared__ float s_t[rg::GROUPS];
    __shared__ float4 s_acc[rg::GROUPS][rg::LANES];
    const int r = long_rows[blockIdx.x];
    if (r < 0 || r >= n_rows) return;                                      // (the whole workgroup)
    int start, end;
    rg::row_span(rowptr, r, n_edges, start, end);
    const int t = threadIdx.x % rg::LANES, g = threadIdx.x / rg::LANES;
    float4 dy = f4_zero(), acc = f4_zero();
    float tr = 0.f;
    if (dY4) {                                                             // every group: the same bits
        dy = dY4[(size_t)r * rg::LANES + t];
        tr = row16_sum(f4_dot(dy, Y4[(size_t)r * rg::LANES + t]));
    }
    if (dAlpha) {                                                          // (a kernel argument: the whole workgroup)
        const float part = row16_sum(bwd_alpha_dot(start + threadIdx.x, end, rg::BLOCK, colidx, perm, n_edges, n_kv, alpha, dAlpha));
        if (t == 0) s_t[g] = part;
        __syncthreads();
        float ta = 0.f;
#pragma unroll
        for (int k = 0; k < rg::GROUPS; ++k) ta += s_t[k];                 // in the order g = 0 ... 15
        tr += ta;
    }
    bwd_row_span(start + g * rg::LANES, end, rg::BLOCK, t, colidx, perm, n_edges, dY4 != nullptr, dy, tr, KV4, n_kv,
                 dY4 != nullptr || dQ != nullptr, alpha, dAlpha, ds, acc);
    if (!dQ) return;                                                       // (a kernel argument: the whole workgroup)
    rg::store_column_sums(s_acc, g, t, acc, nullptr, dQ, r);
}

// The slots of one column for one 16-lane group: acc += alpha_p dY[r] + ds_p Q[r], each row gathered once.
__device__ __forceinline__ void bwd_col_span(int first, int end, int stride, int t, const int32_t* __restrict__ rowidx_t,
                                             const int64_t* __restrict__ perm_t, int n_edges, int n_rows,
                                             const float* __restrict__ alpha, const float* __restrict__ ds,
                                             const float4* __restrict__ dY4, const float4* __restrict__ Q4, float4& acc) {
    for (int base = first; base < end; base += stride) {
        const int j = base + t;
        int r = -1;
        float a = 0.f, s = 0.f;
        if (j < end) {
            r = rowidx_t[j];
            const int p = slot_pos(perm_t, j, n_edges);
            if (r < 0 || r >= n_rows || p < 0) {
                r = -1;                                        // an absent edge
            } else {
                a = alpha[p];
                s = ds[p];
            }
        }
        const int cnt = min(rg::LANES, end - base);
        for (int k0 = 0; k0 < cnt; k0 += ATT_NB) {
            float4 xd[ATT_NB], xq[ATT_NB];
            int rs[ATT_NB];
#pragma unroll
            for (int u = 0; u < ATT_NB; ++u) {
                rs[u] = __shfl(r, k0 + u, rg::LANES);
                xd[u] = (rs[u] >= 0 && dY4) ? dY4[(size_t)rs[u] * rg::LANES + t] : f4_zero();
                xq[u] = rs[u] >= 0 ? Q4[(size_t)rs[u] * rg::LANES + t] : f4_zero();
            }
#pragma unroll
            for (int u = 0; u < ATT_NB; ++u) {
                const float ak = __shfl(a, k0 + u, rg::LANES), sk = __shfl(s, k0 + u, rg::LANES);
                if (rs[u] < 0) continue;
                if (dY4) acc = f4_fma(ak, xd[u], acc);
                acc = f4_fma(sk, xq[u], acc);
            }
        }
    }
}

__global__ __launch_bounds__(rg::BLOCK) void edge_attention_bwd_cols_group_kernel(
    const int32_t* __restrict__ rowptr_t, int n_kv, const int32_t* __restrict__ rowidx_t, const int64_t* __restrict__ perm_t,
    bool skip_long, int n_rows, int n_edges, const float* __restrict__ alpha, const float* __restrict__ ds,
    const float4* __restrict__ dY4, const float4* __restrict__ Q4, const float4* __restrict__ base4, float4* __restrict__ dKV4) {
    rg::for_short_rows(rowptr_t, n_kv, n_edges, skip_long, [&](long c, int start, int end, int t) {
        float4 acc = base4 ? base4[(size_t)c * rg::LANES + t] : f4_zero();
        if (end > start) bwd_col_span(start, end, rg::LANES, t, rowidx_t, perm_t, n_edges, n_rows, alpha, ds, dY4, Q4, acc);
        dKV4[(size_t)c * rg::LANES + t] = acc;
    });
}

__global__ __launch_bounds__(rg::BLOCK) void edge_attention_bwd_cols_block_kernel(
    const int32_t* __restrict__ rowptr_t, int n_kv, const int32_t* __restrict__ rowidx_t, const int64_t* __restrict__ perm_t,
    const int32_t* __restrict__ long_cols, int n_rows, int n_edges, const float* __restrict__ alpha,
    const float* __restrict__ ds, const float4* __restrict__ dY4, const float4* __restrict__ Q4, const float* __restrict__ base,
    float* __restrict__ dKV) {
    __shared__ float4 s_acc[rg::GROUPS][rg::LANES];
    const int c = long_cols[blockIdx.x];
    if (c < 0 || c >= n_kv) return;                                        // (the whole workgroup)
    int start, end;
    rg::row_span(rowptr_t, c, n_edges, start, end);
    const int t = threadIdx.x % rg::LANES, g = threadIdx.x / rg::LANES;
    float4 acc = f4_zero();
    bwd_col_span(start + g * rg::LANES, end, rg::BLOCK, t, rowidx_t, perm_t, n_edges, n_rows, alpha, ds, dY4, Q4, acc);
    rg::store_column_sums(s_acc, g, t, acc, base, dKV, c);
}

}  // namespace

extern "C" int32_t mmrec_edge_attention_group_max(void) { return rg::GROUP_MAX; }

extern "C" int mmrec_edge_attention_f32(const int32_t* rowptr, int32_t n_rows, const int32_t* colidx, const int64_t* perm,
                                        const int32_t* long_rows, int32_t n_long, const float* Q, int64_t n_q, const float* KV,
                                        int64_t n_kv, int32_t d, int64_t n_edges, float eps, float* Y, float* alpha,
                                        mmrec_stream_t stream) {
    if (d != 4 * rg::LANES) return MMREC_ERR_UNSUPPORTED;
    if (n_rows < 0 || n_edges < 0 || n_long < 0 || n_q < 0 || n_kv < 0) return MMREC_ERR_BAD_ARG;
    if (n_rows == 0 || n_edges == 0) return 0;                             // nothing to launch (the caller's Y is all zeros)
    if (n_edges > INT32_MAX || n_kv > INT32_MAX) return MMREC_ERR_UNSUPPORTED;
    if (n_q < n_rows) return MMREC_ERR_BAD_ARG;                            // one row of Q per row of the CSR
    if (!rowptr || !colidx || !Q || !KV || !Y || !alpha) return MMREC_ERR_BAD_ARG;
    if (n_long > 0 && !long_rows) return MMREC_ERR_BAD_ARG;
    hipStream_t s = mmrec_stream(stream);
    const float4 *Q4 = reinterpret_cast<const float4*>(Q), *KV4 = reinterpret_cast<const float4*>(KV);
    rg::launch_pair(
        n_rows, n_long,
        [&](dim3 grid) {
            hipLaunchKernelGGL(edge_attention_group_kernel, grid, dim3(rg::BLOCK), 0, s, rowptr, (int)n_rows, colidx, perm,
                               n_long > 0, Q4, KV4, (int)n_kv, (int)n_edges, eps, reinterpret_cast<float4*>(Y), alpha);
        },
        [&](dim3 grid) {
            hipLaunchKernelGGL(edge_attention_block_kernel, grid, dim3(rg::BLOCK), 0, s, rowptr, (int)n_rows, colidx, perm,
                               long_rows, Q4, KV4, (int)n_kv, (int)n_edges, eps, Y, alpha);
        });
    MMREC_RETURN_LAUNCH_STATUS();
}

extern "C" int mmrec_edge_attention_bwd_f32(const int32_t* rowptr, int32_t n_rows, const int32_t* colidx, const int64_t* perm,
                                            const int32_t* long_rows, int32_t n_long, const int32_t* rowptr_t,
                                            const int32_t* rowidx_t, const int64_t* perm_t, const int32_t* long_cols,
                                            int32_t n_long_t, const float* Q, int64_t n_q, const float* KV, int64_t n_kv,
                                            const float* Y, const float* alpha, const float* dY, const float* dAlpha, int32_t d,
                                            int64_t n_edges, float* ds, float* dQ, float* dKV, const float* dKV_base,
                                            mmrec_stream_t stream) {
    if (d != 4 * rg::LANES) return MMREC_ERR_UNSUPPORTED;
    if (n_rows < 0 || n_edges < 0 || n_long < 0 || n_long_t < 0 || n_q < 0 || n_kv < 0) return MMREC_ERR_BAD_ARG;
    if (n_rows == 0 || n_edges == 0) return 0;                             // nothing to launch (the caller's zeros stand)
    if (n_edges > INT32_MAX || n_kv > INT32_MAX) return MMREC_ERR_UNSUPPORTED;
    if (n_q < n_rows) return MMREC_ERR_BAD_ARG;
    if (!rowptr || !colidx || !KV || !alpha || !ds) return MMREC_ERR_BAD_ARG;
    if ((!dY && !dAlpha) || (dY && !Y) || (!dQ && !dKV)) return MMREC_ERR_BAD_ARG;
    if (dKV && (!rowptr_t || !rowidx_t || !Q || dKV_base == dKV)) return MMREC_ERR_BAD_ARG;
    if ((n_long > 0 && !long_rows) || (dKV && n_long_t > 0 && !long_cols)) return MMREC_ERR_BAD_ARG;
    hipStream_t s = mmrec_stream(stream);
    const float4 *Q4 = reinterpret_cast<const float4*>(Q), *KV4 = reinterpret_cast<const float4*>(KV),
                 *Y4 = reinterpret_cast<const float4*>(Y), *dY4 = reinterpret_cast<const float4*>(dY);
    rg::launch_pair(
        n_rows, n_long,
        [&](dim3 grid) {
            hipLaunchKernelGGL(edge_attention_bwd_rows_group_kernel, grid, dim3(rg::BLOCK), 0, s, rowptr, (int)n_rows, colidx,
                               perm, n_long > 0, KV4, (int)n_kv, (int)n_edges, Y4, alpha, dY4, dAlpha, ds,
                               reinterpret_cast<float4*>(dQ));
        },
        [&](dim3 grid) {
            hipLaunchKernelGGL(edge_attention_bwd_rows_block_kernel, grid, dim3(rg::BLOCK), 0, s, rowptr, (int)n_rows, colidx,
                               perm, long_rows, KV4, (int)n_kv, (int)n_edges, Y4, alpha, dY4, dAlpha, ds, dQ);
        });
    if (dKV && n_kv > 0)
        rg::launch_pair(
            n_kv, n_long_t,
            [&](dim3 grid) {
                hipLaunchKernelGGL(edge_attention_bwd_cols_group_kernel, grid, dim3(rg::BLOCK), 0, s, rowptr_t, (int)n_kv,
                                   rowidx_t, perm_t, n_long_t > 0, (int)n_rows, (int)n_edges, alpha, ds, dY4, Q4,
                                   reinterpret_cast<const float4*>(dKV_base), reinterpret_cast<float4*>(dKV));
            },
            [&](dim3 grid) {
                hipLaunchKernelGGL(edge_attention_bwd_cols_block_kernel, grid, dim3(rg::BLOCK), 0, s, rowptr_t, (int)n_kv,
                                   rowidx_t, perm_t, long_cols, (int)n_rows, (int)n_edges, alpha, ds, dY4, Q4, dKV_base, dKV);
            });
    MMREC_RETURN_LAUNCH_STATUS();
}
