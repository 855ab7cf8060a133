// Top-k of a MIX of three row softmaxes against three whole tables, without any [B, N] block (DAMRS's pseudo-labels,
// damrs.py:141-180: top10_j(p_a + p_b + 2 p_m) for each target modality m):
//   c_m[r, j] = <T_m[ids[r]], T_m[j]>,   p_m[r, j] = exp(c_m[r, j] - lse[m][r]),   S_t[r, j] = sum_m W[t][m] p_m[r, j]
//   list t of row r = the k columns with the largest S_t[r, .], score descending, ties by the lower column (cand_before).
// A list needs all three modalities' scores of a (row, column) pair at once, so no two-operand top-k serves it.
//
// One sweep of mfma_sweep.h (as score_lse.hip MODE 0) and the FUSED form of topk.hip.  A workgroup (4 waves) owns 128 query
// rows, a wave 32 of them: the three gathered query fragments stay in registers (lane (i, h) holds T_m[ids[q0 + i]][2 s + h],
// 3 x 32 VGPRs).  64-row tiles of the three tables reach the waves through LDS, fetched one tile ahead and stored de-interleaved
// (mfma_sweep.h).  Per 32-row sub-tile three v_mfma_f32_32x32x2_f32 chains in the swapped orientation: a lane holds ONE query
// and 16 candidates, so a list's running threshold is one register.  Per candidate three exp and three mixes; the common
// path of a list is 16 compares.
// Survivors go to lists in LDS, PRIVATE to a lane (one query x one half of the candidate rows) and to one of the three targets:
// TT_CAP slots and a write-only dump slot, appended branch-free (topk.hip).  A sub-tile is offered in two rounds of 8
// candidates; after a round every query whose half list holds more than TT_CAP - 8 entries is sorted by its wave (<= 32
// entries: bitonic64), cut to k, split back over the two halves (<= 8 each) and its threshold raised to the k-th score, strict
// from then on: every later column is higher, so a tie loses.  Nothing that can be in the top-k is ever dropped.
// LDS: tiles 3 x 64 x 68 x 4 = 52,224 B, lists 256 lanes x 3 x 17 x 8 = 104,448 B; 156,672 B of the 163,840 B a gfx950 workgroup
// may declare -- four waves, one per SIMD, is what fits; a fifth list slot per lane would not.
// Columns are split over gridDim.y by a plan of (B, N) alone; every split hands its sorted, cut lists to `tt_finish_kernel`,
// which ranks the <= 32 k entries of a (target, row) by counting.  No atomics; a call always gives the same bits; no
// allocation, no synchronisation: capturable.
#include "mfma_sweep.h"
#include "topk_sort.h"

namespace {

constexpr int TT_LD = 64 + 4;        // tile pitch (mfma_sweep.h)
constexpr int TT_CAP = 16;           // list slots per (lane, target); slot TT_CAP is the dump
constexpr int TT_KMAX = 16;
constexpr int TT_WGS = 512;          // workgroups the grid aims at
constexpr int TT_SPLITS_MAX = 32;    // 32 * 16 = 512 merge slots
constexpr int TT_ROWS_MAX = 1 << 30;

inline SweepPlan tt_plan(long B, long N) { return sweep_plan(B, N, TT_WGS, TT_SPLITS_MAX); }

__device__ __forceinline__ float tt_max8(const float* a) {
    return fmaxf(fmaxf(fmaxf(a[0], a[1]), fmaxf(a[2], a[3])), fmaxf(fmaxf(a[4], a[5]), fmaxf(a[6], a[7])));
}

__global__ __launch_bounds__(256) void tt_sweep_kernel(const float* __restrict__ T0, const float* __restrict__ T1,
                                                       const float* __restrict__ T2, int N,
                                                       const int64_t* __restrict__ ids, int B,
                                                       const float* __restrict__ lse, const float* __restrict__ W, int k,
                                                       int per, int* __restrict__ tmp_idx, float* __restrict__ tmp_val) {
    __shared__ __attribute__((aligned(16))) float T[3][SWEEP_TILE * TT_LD];
    __shared__ unsigned long long L[256 * 3][TT_CAP + 1];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int i = lane & 31, h = lane >> 5;
    const int q0 = blockIdx.x * SWEEP_OWN + wave * 32;
    const int col_tiles = (N + SWEEP_TILE - 1) / SWEEP_TILE;
    const int t_begin = blockIdx.y * per, t_end = min(t_begin + per, col_tiles);
    const float* const tabs[3] = {T0, T1, T2};
    unsigned long long (*Lw)[TT_CAP + 1] = L + wave * 64 * 3;     // this wave's lists: [(lane_in_wave * 3 + target)][slot]

    // the lane's query: a row past the end or an id outside [0, N) is never used as an address and takes no candidate
    const int row = q0 + i;
    long long id = -1;
    if (row < B) id = ids ? (long long)ids[row] : (long long)row;
    const bool q_ok = id >= 0 && id < (long long)N;
    float qf[3][32];
    float own_l[3];
#pragma unroll
    for (int m = 0; m < 3; ++m) {
        sweep_own<64>(qf[m], tabs[m] + (size_t)(q_ok ? id : 0) * 64, q_ok, h);
        own_l[m] = q_ok ? lse[(size_t)m * B + row] : 0.f;
    }
    float w[3][3];
#pragma unroll
    for (int t = 0; t < 3; ++t)
#pragma unroll
        for (int m = 0; m < 3; ++m) w[t][m] = W[3 * t + m];

    float4 pre[3][4];
    auto fetch = [&](int t) {
#pragma unroll
        for (int m = 0; m < 3; ++m) sweep_fetch<64>(pre[m], tabs[m], t * SWEEP_TILE, N, tid);
    };
    auto stage = [&]() {
#pragma unroll
        for (int m = 0; m < 3; ++m) sweep_stage<64>(T[m], pre[m], tid);
    };

    // keep a score iff s > teff: -inf until the list's first cut, the strict k-th score after it
    float teff0 = -INFINITY, teff1 = -INFINITY, teff2 = -INFINITY;
    int cnt0 = 0, cnt1 = 0, cnt2 = 0;

    // sort target t's entries of query qq (both half lists, n0 + n1 <= 64), keep the best min(n, k) split back over the halves;
    // returns the k-th score or -inf when fewer than k entries exist.  The lists are private to the wave and a wave's LDS
    // operations complete in order: only the compiler must keep the order.
    auto gather = [&](int t, int qq, int n0, int n1) -> Cand {
        Cand x{-INFINITY, INT_MAX};
        if (lane < n0) x = unpack_cand(Lw[qq * 3 + t][lane]);
        else if (lane < n0 + n1) x = unpack_cand(Lw[(qq + 32) * 3 + t][lane - n0]);
        return x;
    };
    auto compact = [&](int t, int qq, int& my_cnt) -> float {
        const int n0 = __shfl(my_cnt, qq, 64), n1 = __shfl(my_cnt, qq + 32, 64);
        const int n = n0 + n1;
        wave_lds_order();
        Cand x = gather(t, qq, n0, n1);
        bitonic64(x, lane);
        const int keep = min(n, k), h0 = (keep + 1) >> 1;
        wave_lds_order();
        if (lane < h0) Lw[qq * 3 + t][lane] = pack_cand(x.v, x.i);
        else if (lane < keep) Lw[(qq + 32) * 3 + t][lane - h0] = pack_cand(x.v, x.i);
        wave_lds_order();
        if (lane == qq) my_cnt = h0;
        if (lane == qq + 32) my_cnt = keep - h0;
        return n >= k ? __shfl(x.v, k - 1, 64) : -INFINITY;
    };

    if (t_begin < t_end) fetch(t_begin);
    for (int tl = t_begin; tl < t_end; ++tl) {
        __syncthreads();                           // the previous tile is consumed
        stage();
        __syncthreads();
        if (tl + 1 < t_end) fetch(tl + 1);         // in flight under this tile's MFMAs
        const int o0 = tl * SWEEP_TILE;
#pragma unroll 1
        for (int u = 0; u < 2; ++u) {
            if (o0 + 32 * u >= N) break;           // uniform: nothing but padding in this sub-tile
            f32x16 acc[3];
#pragma unroll
            for (int m = 0; m < 3; ++m) acc[m] = sweep_scores<64>(T[m], u, i, h, qf[m]);
            float p[3][16];
#pragma unroll
            for (int m = 0; m < 3; ++m)
#pragma unroll
                for (int r = 0; r < 16; ++r) p[m][r] = expf(acc[m][r] - own_l[m]);
            const bool partial = o0 + 32 * u + 32 > N;          // uniform
            const int c0 = o0 + 32 * u + 4 * h;
#pragma unroll
            for (int t = 0; t < 3; ++t) {
                float s[16];
#pragma unroll
                // explicit fma: left to the compiler, some register pairs were contracted and others were not, and two
                // bit-identical table rows no longer scored the same bits
                for (int r = 0; r < 16; ++r) s[r] = fmaf(w[t][2], p[2][r], fmaf(w[t][1], p[1][r], w[t][0] * p[0][r]));
                if (partial) {
#pragma unroll
                    for (int r = 0; r < 16; ++r) s[r] = c0 + (r & 3) + 8 * (r >> 2) < N ? s[r] : -INFINITY;
                }
                float& teff = t == 0 ? teff0 : t == 1 ? teff1 : teff2;
                int& my_cnt = t == 0 ? cnt0 : t == 1 ? cnt1 : cnt2;
#pragma unroll
                for (int half = 0; half < 2; ++half) {
                    const bool hit = q_ok && tt_max8(s + 8 * half) > teff;
                    if (!__any(hit)) continue;     // nothing of this round can enter any list of this target
                    const float thr = hit ? teff : INFINITY;
                    unsigned long long* mine = Lw[lane * 3 + t];
                    int cnt = my_cnt;
#pragma unroll
                    for (int r = 8 * half; r < 8 * half + 8; ++r) {
                        const bool pass = s[r] > thr;
                        mine[pass ? cnt : TT_CAP] = pack_cand(s[r], c0 + (r & 3) + 8 * (r >> 2));
                        cnt += pass ? 1 : 0;
                    }
                    my_cnt = cnt;
                    // a round adds at most 8 entries per lane: cut the queries that might overflow in the next one
                    unsigned long long mm = __ballot(my_cnt > TT_CAP - 8);
                    mm = (mm | (mm >> 32)) & 0xffffffffull;
                    while (mm) {
                        const int qq = __ffsll((long long)mm) - 1;
                        mm &= mm - 1;
                        const float kth = compact(t, qq, my_cnt);
                        if (i == qq && kth > teff) teff = kth;
                    }
                }
            }
        }
    }

    // this split's lists, sorted and cut to k, for the finish kernel; missing entries: INT_MAX
#pragma unroll 1
    for (int t = 0; t < 3; ++t) {
        int my_cnt = t == 0 ? cnt0 : t == 1 ? cnt1 : cnt2;
#pragma unroll 1
        for (int qq = 0; qq < 32; ++qq) {
            if (q0 + qq >= B) break;               // uniform
            const int n0 = __shfl(my_cnt, qq, 64), n1 = __shfl(my_cnt, qq + 32, 64);
            wave_lds_order();
            Cand x = gather(t, qq, n0, n1);
            bitonic64(x, lane);
            if (lane < k) {
                const size_t o = (((size_t)blockIdx.y * 3 + t) * B + (q0 + qq)) * k + lane;
                tmp_idx[o] = lane < n0 + n1 ? x.i : INT_MAX;
                tmp_val[o] = lane < n0 + n1 ? x.v : -INFINITY;
            }
        }
    }
}

// Final top-k of the per-split lists of one (target, row): valid entries are packed in split order with a ballot prefix, then
// rank counting writes every survivor straight to its sorted position; ranks nobody takes (a row without a usable id) get -1.
__global__ __launch_bounds__(64) void tt_finish_kernel(const int* __restrict__ tmp_idx, const float* __restrict__ tmp_val,
                                                       int B, int k, int splits, int32_t* __restrict__ out_idx,
                                                       float* __restrict__ out_val) {
    __shared__ float v[TT_SPLITS_MAX * TT_KMAX];
    __shared__ int id[TT_SPLITS_MAX * TT_KMAX];
    const int r = blockIdx.x, t = blockIdx.y, lane = threadIdx.x;
    const int n = splits * k;
    int n_valid = 0;
    for (int e0 = 0; e0 < n; e0 += 64) {
        const int e = e0 + lane;
        int my_id = INT_MAX;
        float my_v = -INFINITY;
        if (e < n) {
            const int s = e / k, j = e - s * k;
            const size_t o = (((size_t)s * 3 + t) * B + r) * k + j;
            my_id = tmp_idx[o];
            my_v = tmp_val[o];
        }
        const unsigned long long ok = __ballot(my_id != INT_MAX);
        if (my_id != INT_MAX) {
            const int pos = n_valid + __popcll(ok & ((1ull << lane) - 1ull));
            v[pos] = my_v;
            id[pos] = my_id;
        }
        n_valid += __popcll(ok);
    }
    __syncthreads();
    const size_t o = ((size_t)t * B + r) * k;
    if (lane < k && lane >= n_valid) {
        out_idx[o + lane] = -1;
        if (out_val) out_val[o + lane] = -INFINITY;
    }
    for (int e = lane; e < n_valid; e += 64) {
        const Cand me{v[e], id[e]};
        int rank = 0;
        for (int j = 0; j < n_valid; ++j) rank += cand_before(Cand{v[j], id[j]}, me);
        if (rank < k) {
            out_idx[o + rank] = me.i;
            if (out_val) out_val[o + rank] = me.v;
        }
    }
}

// out[r] = the first k entries of cand[r] that do not occur in excl[r], in cand's order; one thread per row
__global__ __launch_bounds__(256) void list_exclude_kernel(const int32_t* __restrict__ cand, const int32_t* __restrict__ excl,
                                                           int R, int kc, int ke, int k, int32_t* __restrict__ out) {
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r >= R) return;
    const int32_t* c = cand + (size_t)r * kc;
    const int32_t* x = excl + (size_t)r * ke;
    int32_t* o = out + (size_t)r * k;
    int n = 0;
    for (int j = 0; j < kc && n < k; ++j) {
        const int32_t cj = c[j];
        bool hit = false;
        for (int e = 0; e < ke; ++e) hit |= x[e] == cj;
        if (!hit) o[n++] = cj;
    }
    for (; n < k; ++n) o[n] = -1;       // (duplicates inside excl never make this happen: kc - ke >= k)
}

}  // namespace

extern "C" int32_t mmrec_tri_topk_split_cols(int32_t B, int32_t N) {
    if (B < 0 || N <= 0 || B > TT_ROWS_MAX || N > TT_ROWS_MAX) return 0;
    return tt_plan(B, N).per * SWEEP_TILE;      // <= 2^30 + 63
}

extern "C" size_t mmrec_tri_topk_workspace_bytes(int32_t B, int32_t N, int32_t k) {
    if (B <= 0 || N <= 0 || k < 1 || k > TT_KMAX || B > TT_ROWS_MAX || N > TT_ROWS_MAX) return 0;
    return (size_t)2 * tt_plan(B, N).splits * 3 * (size_t)B * k * sizeof(float);
}

extern "C" int mmrec_tri_topk_f32(const float* T0, const float* T1, const float* T2, int32_t N, const int64_t* ids, int32_t B,
                                  const float* lse, const float* W, int32_t k, int32_t* out_idx, float* out_val, void* ws,
                                  mmrec_stream_t stream) {
    if (B < 0 || N < 0 || k < 1 || k > TT_KMAX || N < k) return MMREC_ERR_BAD_ARG;
    if (!T0 || !T1 || !T2 || !lse) return MMREC_ERR_BAD_ARG;
    if (B > TT_ROWS_MAX || N > TT_ROWS_MAX) return MMREC_ERR_UNSUPPORTED;
    if (B == 0) return 0;
    if (!W || !out_idx || !ws) return MMREC_ERR_BAD_ARG;
    const SweepPlan p = tt_plan(B, N);
    hipStream_t s = mmrec_stream(stream);
    int* tmp_idx = static_cast<int*>(ws);
    float* tmp_val = reinterpret_cast<float*>(tmp_idx + (size_t)p.splits * 3 * (size_t)B * k);
    hipLaunchKernelGGL(tt_sweep_kernel, dim3(p.own_tiles, p.splits), dim3(256), 0, s, T0, T1, T2, N, ids, B, lse, W, k, p.per,
                       tmp_idx, tmp_val);
    hipLaunchKernelGGL(tt_finish_kernel, dim3(B, 3), dim3(64), 0, s, tmp_idx, tmp_val, B, k, p.splits, out_idx, out_val);
    MMREC_RETURN_LAUNCH_STATUS();
}

extern "C" int mmrec_list_exclude_i32(const int32_t* cand, const int32_t* excl, int32_t R, int32_t kc, int32_t ke, int32_t k,
                                      int32_t* out, mmrec_stream_t stream) {
    if (R < 0 || kc < 0 || ke < 0 || k < 1 || kc - ke < k) return MMREC_ERR_BAD_ARG;
    if (R == 0) return 0;
    if (!cand || !out || (ke > 0 && !excl)) return MMREC_ERR_BAD_ARG;
    hipLaunchKernelGGL(list_exclude_kernel, dim3((R + 255) / 256), dim3(256), 0, mmrec_stream(stream), cand, excl, R, kc, ke, k,
                       out);
    MMREC_RETURN_LAUNCH_STATUS();
}
