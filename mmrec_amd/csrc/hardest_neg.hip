// MVGAE's reconstruction term (mvgae.py:73-85, recon_loss): every batch user against the HARDEST of the batch's negatives,
//   S = sigmoid(Z[l]) (squash) or Z[l];  u_b = S[users[b]], p_b = S[pos[b]], n_j = S[neg[j]]
//   a_b = sigmoid(<u_b, p_b>),  h_b = max_j <u_b, n_j>,  arg_b = the LOWEST j that attains it
//   loss[l] = - sum_b log2(sigmoid(a_b - sigmoid(h_b)))
// for L latents over the same rows, without the sigmoid of the whole table, the three gathered blocks or the [B, B] scores.
//
// hn_sweep_kernel: the sweep of mfma_sweep.h (as score_lse.hip MODE 0) with both operands GATHERED and squashed on the way: a
// workgroup (4 waves) owns 128 batch users, a wave 32 of them, their squashed rows in registers (`sweep_own`); the negatives'
// rows are gathered from Z[l], squashed and staged de-interleaved into one of TWO tiles in LDS, the next tile while this one is
// scored (one barrier a tile).  A lane holds 16 scores of ONE user and keeps a running (score, position): its positions come in
// ascending order, so `>` keeps the lowest position of equal scores; the two lanes of a user and the splits compare (score, then
// lower position).  Which rows of a tile are candidates -- position < B and id in [0, N) -- is a 64-bit mask staged with the
// tile: a row that is no candidate is EXCLUDED, not zeroed (without the squash every real score may be negative).
// hn_term_kernel: a thread per sample: the splits in order, the positive dot product as one fma chain, the term and the two
// coefficients dloss/d<u, p> and dloss/dh; hn_loss_kernel: one workgroup per latent adds the B terms in a fixed tree.
// hn_bwd_kernel: slot gradients G [L, 3 B, 64] (users, pos, neg); a negative's owner scans arg[l, :] for its position and adds
// its users' kept rows in ascending order.  The caller scatters G with mmrec_scatter_add_rows_sorted_f32.
// No float atomics, every order fixed by (B, L) alone: the same bits on every call.  No address depends on an id out of range.
#include "mfma_sweep.h"

namespace {

constexpr int HN_LD = 64 + 4;          // tile pitch (mfma_sweep.h)
constexpr int HN_WGS = 512;            // workgroups the sweep's grid aims at (2 per CU), over all latents
constexpr int HN_SPLITS_MAX = 16;
constexpr int HN_L_MAX = 8;
constexpr int HN_B_MAX = 65536;
constexpr long long HN_N_MAX = 1ll << 30;
constexpr int HN_TERM_THREADS = 64;      // a wave of samples a workgroup: B / 64 x L workgroups
constexpr int HN_LOSS_THREADS = 1024;
constexpr float HN_INV_LN2 = 1.44269504088896340736f;

inline SweepPlan hn_plan(long B, long L) { return sweep_plan(B, B, (int)((HN_WGS + L - 1) / L), HN_SPLITS_MAX); }

template <bool SQ>
__device__ __forceinline__ float hn_squash(float v) { return SQ ? stable_sigmoid(v) : v; }
template <bool SQ>
__device__ __forceinline__ float4 hn_squash4(float4 v) {
    return make_float4(hn_squash<SQ>(v.x), hn_squash<SQ>(v.y), hn_squash<SQ>(v.z), hn_squash<SQ>(v.w));
}
__device__ __forceinline__ bool hn_in_range(long long id, long long N) { return id >= 0 && id < N; }

// (s1, p1) beats (s0, p0): a candidate beats none, a higher score beats a lower, of equal scores the lower position wins
__device__ __forceinline__ bool hn_beats(float s1, int p1, float s0, int p0) {
    return p1 >= 0 && (p0 < 0 || s1 > s0 || (s1 == s0 && p1 < p0));
}

template <bool SQ>
__global__ __launch_bounds__(256) void hn_sweep_kernel(const float* __restrict__ Z, long long N,
                                                       const int64_t* __restrict__ users, const int64_t* __restrict__ neg,
                                                       int B, int per, float* __restrict__ ws_max, int* __restrict__ ws_arg) {
    __shared__ __attribute__((aligned(16))) float T[2][SWEEP_TILE * HN_LD];
    __shared__ unsigned long long Tm[2];               // the tile's candidate rows
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int i = lane & 31, h = lane >> 5;
    const int l = blockIdx.z, L = gridDim.z;
    const float* __restrict__ Zl = Z + (size_t)l * (size_t)N * 64;
    const int own0 = blockIdx.x * SWEEP_OWN + wave * 32;
    const int oth_tiles = (B + SWEEP_TILE - 1) / SWEEP_TILE;
    const int t_begin = blockIdx.y * per, t_end = min(t_begin + per, oth_tiles);

    // the lane's user: a row past the end or an id outside [0, N) is never an address; its scores are those of a zero row and
    // the finish drops the sample
    long long uid = -1;
    if (own0 + i < B) uid = (long long)users[own0 + i];
    const bool u_ok = hn_in_range(uid, N);
    float qf[32];
    sweep_own<64>(qf, Zl + (size_t)(u_ok ? uid : 0) * 64, u_ok, h);
    if (SQ) {
#pragma unroll
        for (int s = 0; s < 32; ++s) qf[s] = u_ok ? stable_sigmoid(qf[s]) : 0.f;
    }

    // a thread stages the 16-byte piece c4 of the tile rows r0 + 16 j; wave 0 also knows which of the 64 rows are candidates
    const int r0 = tid >> 4, c4 = tid & 15;
    long long nid[4];
    float4 pre[4];
    unsigned long long pre_mask = 0;
    long long nxt[4];                              // the ids of the tile after the one in `pre`: one level of the chain less
    auto fetch_ids = [&](int t) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int p = t * SWEEP_TILE + r0 + 16 * j;
            const long long v = p < B ? (long long)neg[p] : -1;
            nxt[j] = hn_in_range(v, N) ? v : -1;
        }
    };
    auto fetch = [&](int t) {                      // (after fetch_ids(t))
        const int o0 = t * SWEEP_TILE;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            nid[j] = nxt[j];
            pre[j] = ld4_guard(Zl + (size_t)(nid[j] >= 0 ? nid[j] : 0) * 64 + 4 * c4, nid[j] >= 0);
        }
        if (wave == 0) {
            const long long v = o0 + lane < B ? (long long)neg[o0 + lane] : -1;
            pre_mask = __ballot(hn_in_range(v, N));
        }
        if (t + 1 < t_end) fetch_ids(t + 1);
    };
    auto stage = [&](int buf) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float4 v = nid[j] >= 0 ? hn_squash4<SQ>(pre[j]) : f4_zero();
            float* row = T[buf] + (r0 + 16 * j) * HN_LD;
            *reinterpret_cast<float2*>(row + 2 * c4) = make_float2(v.x, v.z);             // k = 4 c4, 4 c4 + 2 (mfma_sweep.h)
            *reinterpret_cast<float2*>(row + 32 + 2 * c4) = make_float2(v.y, v.w);        // k = 4 c4 + 1, + 3
        }
        if (tid == 0) Tm[buf] = pre_mask;
    };

    float best = -INFINITY;
    int bpos = -1;
    if (t_begin < t_end) {
        fetch_ids(t_begin);
        fetch(t_begin);
        stage(0);
    }
    __syncthreads();
    for (int t = t_begin; t < t_end; ++t) {
        const int buf = (t - t_begin) & 1;
        if (t + 1 < t_end) fetch(t + 1);           // in flight under this tile's MFMAs
        const int o0 = t * SWEEP_TILE;
        const unsigned long long mask = Tm[buf];
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            if (o0 + 32 * u >= B) break;           // uniform: no candidate in this sub-tile
            const f32x16 acc = sweep_scores<64>(T[buf], u, i, h, qf);
            const unsigned m32 = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(mask >> (32 * u)));
#pragma unroll
            for (int r = 0; r < 16; ++r) {         // the lane's positions ascend with r, u and t
                const int row = d_row(r, lane);
                const float x = acc[r];
                const bool take = ((m32 >> row) & 1u) && (bpos < 0 || x > best);
                best = take ? x : best;
                bpos = take ? o0 + 32 * u + row : bpos;
            }
        }
        if (t + 1 < t_end) stage(buf ^ 1);
        __syncthreads();                           // tile t is consumed, tile t + 1 is staged
    }

    // the two lanes of a user
    const float o_s = lane_xor_f<32>(best);
    const int o_p = lane_xor_i<32>(bpos);
    if (hn_beats(o_s, o_p, best, bpos)) {
        best = o_s;
        bpos = o_p;
    }
    if (h == 0 && own0 + i < B) {
        const size_t o = ((size_t)blockIdx.y * L + l) * (size_t)B + own0 + i;
        ws_max[o] = best;
        ws_arg[o] = bpos;
    }
}

// softplus(y) = log(1 + exp(y)) = max(y, 0) + log1p(exp(-|y|)), finite for every finite y
__device__ __forceinline__ float hn_softplus(float y) { return fmaxf(y, 0.f) + log1pf(expf(-fabsf(y))); }

// a thread per sample: the splits in order, the positive dot product, the term and the two coefficients; the squashed user row
// is kept for the backward (its neg slots add user rows by the thousand)
template <bool SQ>
__global__ __launch_bounds__(HN_TERM_THREADS) void hn_term_kernel(const float* __restrict__ Z, long long N,
                                                                  const int64_t* __restrict__ users,
                                                                  const int64_t* __restrict__ pos, int B, int splits,
                                                                  const float* __restrict__ ws_max, const int* __restrict__ ws_arg,
                                                                  float* __restrict__ ws_term, int32_t* __restrict__ arg,
                                                                  float* __restrict__ coef, float* __restrict__ su) {
    const int b = blockIdx.x * HN_TERM_THREADS + threadIdx.x, l = blockIdx.y, L = gridDim.y;
    if (b >= B) return;
    const float* __restrict__ Zl = Z + (size_t)l * (size_t)N * 64;
    float hmax = -INFINITY;
    int a = -1;
    for (int s = 0; s < splits; ++s) {             // the splits in order, the sweep's rule
        const size_t o = ((size_t)s * L + l) * (size_t)B + b;
        const float sv = ws_max[o];
        const int sa = ws_arg[o];
        if (hn_beats(sv, sa, hmax, a)) {
            hmax = sv;
            a = sa;
        }
    }
    const long long uid = (long long)users[b], pid = (long long)pos[b];
    const bool ok = a >= 0 && hn_in_range(uid, N) && hn_in_range(pid, N);
    const float4* ur = reinterpret_cast<const float4*>(Zl + (size_t)(ok ? uid : 0) * 64);
    const float4* pr = reinterpret_cast<const float4*>(Zl + (size_t)(ok ? pid : 0) * 64);
    const size_t o = (size_t)l * B + b;
    float4* sur = reinterpret_cast<float4*>(su + o * 64);
    float dp = 0.f;
#pragma unroll 4
    for (int q = 0; q < 16; ++q) {                 // one fma chain in natural k order
        const float4 u4 = hn_squash4<SQ>(ur[q]), p4 = hn_squash4<SQ>(pr[q]);
        sur[q] = ok ? u4 : f4_zero();
        dp = fmaf(u4.x, p4.x, dp);
        dp = fmaf(u4.y, p4.y, dp);
        dp = fmaf(u4.z, p4.z, dp);
        dp = fmaf(u4.w, p4.w, dp);
    }
    const float av = stable_sigmoid(dp), sh = stable_sigmoid(ok ? hmax : 0.f);
    const float x = av - sh;
    const float term = hn_softplus(-x) * HN_INV_LN2;                     // -log2(sigmoid(x))
    const float sg = stable_sigmoid(-x) * HN_INV_LN2;                    // -d term / dx
    const float c1 = -(sg * (av * (1.f - av))), c2 = sg * (sh * (1.f - sh));
    arg[o] = ok ? a : -1;
    coef[2 * o] = ok ? c1 : 0.f;
    coef[2 * o + 1] = ok ? c2 : 0.f;
    ws_term[o] = ok ? term : 0.f;
}

// loss[l] = the B terms in a fixed tree: thread t adds the samples t, t + 1024, ... in order, the wave's 64 lanes by a
// butterfly, the 16 waves in order
__global__ __launch_bounds__(HN_LOSS_THREADS) void hn_loss_kernel(const float* __restrict__ ws_term, int B,
                                                                  float* __restrict__ loss) {
    __shared__ float part[HN_LOSS_THREADS / 64];
    const int tid = threadIdx.x, l = blockIdx.x;
    float sum = 0.f;
    for (int b = tid; b < B; b += HN_LOSS_THREADS) sum += ws_term[(size_t)l * B + b];
    sum = wave_sum(sum);
    if ((tid & 63) == 0) part[tid >> 6] = sum;
    __syncthreads();
    if (tid == 0) {
        float total = 0.f;
        for (int w = 0; w < HN_LOSS_THREADS / 64; ++w) total += part[w];
        loss[l] = total;
    }
}

// Slot gradients.  The first ceil(2 B / 16) workgroups have the user and positive slots, a 16-lane group per slot and a float4
// per lane.  The others have the negative slots, a WAVE per slot and a column per lane: the hardest negative of a batch is the
// same for most of its users, so one slot's chain can be B long -- its owner reads the kept user rows 16 at a time (all loads
// in flight), then adds them in ascending order.
template <bool SQ>
__global__ __launch_bounds__(256) void hn_bwd_kernel(const float* __restrict__ Z, long long N, const int64_t* __restrict__ users,
                                                     const int64_t* __restrict__ pos, const int64_t* __restrict__ neg, int B,
                                                     const int32_t* __restrict__ arg, const float* __restrict__ coef,
                                                     const float* __restrict__ su, const float* __restrict__ g,
                                                     float* __restrict__ G, int row_blocks) {
    const int tid = threadIdx.x, lane = tid & 63;
    const int l = blockIdx.y;
    const float* __restrict__ Zl = Z + (size_t)l * (size_t)N * 64;
    const int32_t* __restrict__ argl = arg + (size_t)l * B;
    const float* __restrict__ coefl = coef + (size_t)l * B * 2;
    const float* __restrict__ sul = su + (size_t)l * B * 64;
    float* __restrict__ Gl = G + (size_t)l * 3 * B * 64;
    const float gl = g[l];
    if ((int)blockIdx.x < row_blocks) {
        const int l16 = tid & 15, slot = blockIdx.x * 16 + (tid >> 4);
        if (slot >= 2 * B) return;
        const int kind = slot / B, b = slot - kind * B;        // 0 users, 1 pos
        auto row4 = [&](long long id) { return hn_squash4<SQ>(*reinterpret_cast<const float4*>(Zl + (size_t)id * 64 + 4 * l16)); };
        const int a = argl[b];
        // a sample that contributes has its user, positive and chosen negative in range (the forward's arg); an arg that is
        // not the forward's is still never an address
        const long long uid = (long long)users[b], pid = (long long)pos[b], cid = a >= 0 && a < B ? (long long)neg[a] : -1;
        float4 t = f4_zero();
        if (hn_in_range(uid, N) && hn_in_range(pid, N) && hn_in_range(cid, N)) {
            const float w1 = gl * coefl[2 * b], w2 = gl * coefl[2 * b + 1];
            const float4 u4 = *reinterpret_cast<const float4*>(sul + (size_t)b * 64 + 4 * l16), p4 = row4(pid);
            t = kind == 0 ? f4_fma(w2, row4(cid), f4_scale(w1, p4)) : f4_scale(w1, u4);
            if (SQ) {
                const float4 s = kind == 0 ? u4 : p4;          // the slot's own squashed row
                t = make_float4(t.x * (s.x * (1.f - s.x)), t.y * (s.y * (1.f - s.y)), t.z * (s.z * (1.f - s.z)),
                                t.w * (s.w * (1.f - s.w)));
            }
        }
        *reinterpret_cast<float4*>(Gl + (size_t)slot * 64 + 4 * l16) = t;
        return;
    }
    const int j = ((int)blockIdx.x - row_blocks) * 4 + __builtin_amdgcn_readfirstlane(tid >> 6);       // the wave's negative
    if (j >= B) return;
    const long long nid = (long long)neg[j];
    float t = 0.f;
    if (hn_in_range(nid, N)) {                     // uniform
        for (int c0 = 0; c0 < B; c0 += 64) {
            const int bb = c0 + lane;
            const int a = bb < B ? argl[bb] : -1;
            unsigned long long bal = __ballot(a == j);
            if (!bal) continue;
            const int wl = __float_as_int(a == j ? gl * coefl[2 * bb + 1] : 0.f);      // the lane's sample, if it chose j
            while (bal) {                          // its samples in ascending order, 16 rows in flight
                float v[16], w[16];
#pragma unroll
                for (int q = 0; q < 16; ++q) {
                    v[q] = 0.f;
                    w[q] = 0.f;
                    if (bal) {                     // uniform
                        const int k = __builtin_amdgcn_readfirstlane(__ffsll((long long)bal) - 1);
                        bal &= bal - 1;
                        w[q] = __int_as_float(__builtin_amdgcn_readlane(wl, k));
                        v[q] = sul[(size_t)(c0 + k) * 64 + lane];
                    }
                }
#pragma unroll
                for (int q = 0; q < 16; ++q) t = fmaf(w[q], v[q], t);   // (a slot past the last sample adds 0 * 0: t unchanged)
            }
        }
        if (SQ) {
            const float s = stable_sigmoid(Zl[(size_t)nid * 64 + lane]);
            t *= s * (1.f - s);
        }
    }
    Gl[(size_t)(2 * B + j) * 64 + lane] = t;
}

inline bool hn_shape_ok(long long N, int L, int d, int B) {
    return d == 64 && L >= 1 && L <= HN_L_MAX && B >= 0 && B <= HN_B_MAX && N >= 1 && N <= HN_N_MAX;
}

}  // namespace

// negatives one workgroup of the sweep walks (a function of B and L alone; 0 outside the served range)
extern "C" int32_t mmrec_hardest_neg_split_cols(int32_t B, int32_t L) {
    if (B < 1 || B > HN_B_MAX || L < 1 || L > HN_L_MAX) return 0;
    return hn_plan(B, L).per * SWEEP_TILE;
}

// per (split, l, b) a maximum and its position, per (l, b) a term
extern "C" size_t mmrec_hardest_neg_workspace_bytes(int32_t B, int32_t L) {
    if (B < 1 || B > HN_B_MAX || L < 1 || L > HN_L_MAX) return 0;
    return ((size_t)hn_plan(B, L).splits * 2 + 1) * (size_t)L * (size_t)B * sizeof(float);
}

extern "C" int mmrec_hardest_neg_fwd_f32(const float* Z, int64_t N, int32_t L, int32_t d, const int64_t* users,
                                         const int64_t* pos, const int64_t* neg, int32_t B, int32_t squash, float* loss,
                                         int32_t* arg, float* coef, float* su, void* workspace, mmrec_stream_t stream) {
    if (!hn_shape_ok(N, L, d, B)) return MMREC_ERR_BAD_ARG;
    if (B == 0) return 0;
    if (!Z || !users || !pos || !neg || !loss || !arg || !coef || !su || !workspace) return MMREC_ERR_BAD_ARG;
    const SweepPlan p = hn_plan(B, L);
    hipStream_t s = mmrec_stream(stream);
    float* ws_max = static_cast<float*>(workspace);
    int* ws_arg = reinterpret_cast<int*>(ws_max + (size_t)p.splits * L * B);
    float* ws_term = ws_max + (size_t)2 * p.splits * L * B;
    const dim3 grid(p.own_tiles, p.splits, L), tgrid((B + HN_TERM_THREADS - 1) / HN_TERM_THREADS, L);
    if (squash) {
        hipLaunchKernelGGL(hn_sweep_kernel<true>, grid, dim3(256), 0, s, Z, (long long)N, users, neg, B, p.per, ws_max, ws_arg);
        hipLaunchKernelGGL(hn_term_kernel<true>, tgrid, dim3(HN_TERM_THREADS), 0, s, Z, (long long)N, users, pos, B, p.splits,
                           ws_max, ws_arg, ws_term, arg, coef, su);
    } else {
        hipLaunchKernelGGL(hn_sweep_kernel<false>, grid, dim3(256), 0, s, Z, (long long)N, users, neg, B, p.per, ws_max, ws_arg);
        hipLaunchKernelGGL(hn_term_kernel<false>, tgrid, dim3(HN_TERM_THREADS), 0, s, Z, (long long)N, users, pos, B, p.splits,
                           ws_max, ws_arg, ws_term, arg, coef, su);
    }
    hipLaunchKernelGGL(hn_loss_kernel, dim3(L), dim3(HN_LOSS_THREADS), 0, s, ws_term, B, loss);
    MMREC_RETURN_LAUNCH_STATUS();
}

extern "C" int mmrec_hardest_neg_bwd_f32(const float* Z, int64_t N, int32_t L, int32_t d, const int64_t* users,
                                         const int64_t* pos, const int64_t* neg, int32_t B, int32_t squash, const int32_t* arg,
                                         const float* coef, const float* su, const float* g, float* G, mmrec_stream_t stream) {
    if (!hn_shape_ok(N, L, d, B)) return MMREC_ERR_BAD_ARG;
    if (B == 0 || !G) return 0;                    // nothing wanted: no launch
    if (!Z || !users || !pos || !neg || !arg || !coef || !su || !g) return MMREC_ERR_BAD_ARG;
    hipStream_t s = mmrec_stream(stream);
    const int row_blocks = (2 * B + 15) / 16;
    const dim3 grid(row_blocks + (B + 3) / 4, L);
    if (squash)
        hipLaunchKernelGGL(hn_bwd_kernel<true>, grid, dim3(256), 0, s, Z, (long long)N, users, pos, neg, B, arg, coef, su, g, G,
                           row_blocks);
    else
        hipLaunchKernelGGL(hn_bwd_kernel<false>, grid, dim3(256), 0, s, Z, (long long)N, users, pos, neg, B, arg, coef, su, g, G,
                           row_blocks);
    MMREC_RETURN_LAUNCH_STATUS();
}
