// Rows SURVEY.md 8(f) marks "next" on either side of the hot path.
//  f1  negative sampler  (replaces the Python rejection loop TrainDataLoader._sample_neg_ids,
//      utils/dataloader.py:267-275: uniform over train-seen items, rejected while in the user's history)
//  f2  hit matrix + per-user ranking metrics (replaces the Python double loop
//      topk_evaluator.py:88-93 and the per-user part of metrics.py:12-105)
// Integer / index work: exact.  The sampler uses its own counter-based RNG (splitmix64), so ids match
// the host sampler statistically, not stream for stream (the host sampler stays the parity mode).
// A sample's first state is mix64 applied three times, to the seed, then with the counter, then with the
// sample index added (include/mmrec_hip.h): adding b times splitmix64's own increment to the state, as
// this file once did, made sample b + 1's draw t equal sample b's draw t + 1 whenever the seed was 0.
#include "common.h"

namespace {

__device__ __forceinline__ uint64_t mix64(uint64_t z) {   // splitmix64's output function: a bijection
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

__device__ __forceinline__ uint64_t splitmix64(uint64_t& s) {
    return mix64(s += 0x9E3779B97F4A7C15ull);
}

__device__ __forceinline__ bool row_contains(const int32_t* __restrict__ col, int lo, int hi, int x) {
    int l = lo, h = hi;
    while (l < h) {
        const int mid = (l + h) >> 1;
        if (col[mid] < x) l = mid + 1; else h = mid;
    }
    return l < hi && col[l] == x;
}

__global__ __launch_bounds__(256) void sample_negatives_kernel(
    const int64_t* __restrict__ users, int batch, const int32_t* __restrict__ hist_rowptr,
    const int32_t* __restrict__ hist_col, const int32_t* __restrict__ cand, int n_cand, uint64_t seed,
    uint64_t counter, int64_t* __restrict__ out) {
    const int b = blockIdx.x * 256 + threadIdx.x;
    if (b >= batch) return;
    // one mixing round per argument: neither a seed, nor a counter, nor b shifts one sample's stream along another's
    uint64_t s = mix64(mix64(mix64(seed + 0x9E3779B97F4A7C15ull) + counter) + (uint64_t)b);
    const int u = (int)users[b];
    const int lo = hist_rowptr[u], hi = hist_rowptr[u + 1];
    int item = cand[0];
    for (int tries = 0; tries < 4096; ++tries) {   // the reference loops forever; bounded here
        const uint32_t r = (uint32_t)(splitmix64(s) >> 32);
        item = cand[(uint32_t)(((uint64_t)r * (uint64_t)n_cand) >> 32)];
        if (!row_contains(hist_col, lo, hi, item)) break;
    }
    out[b] = item;
}

// One thread per evaluated user, sequential over its K recommendations so that every running sum
// has exactly the order of numpy's cumsum in the reference (bit-identical doubles).
// out[u][m][t]: m = 0 recall, 1 ndcg, 2 precision, 3 map ; t indexes the requested cut-offs ks[t].
__global__ __launch_bounds__(256) void topk_metrics_kernel(
    const int64_t* __restrict__ topk_idx, int n_users, int k, const int32_t* __restrict__ gt_rowptr,
    const int32_t* __restrict__ gt_col, const double* __restrict__ discount,
    const double* __restrict__ idcg_cum, const int32_t* __restrict__ ks, int n_ks,
    uint8_t* __restrict__ hit_out, double* __restrict__ out) {
    const int u = blockIdx.x * 256 + threadIdx.x;
    if (u >= n_users) return;
    const int lo = gt_rowptr[u], hi = gt_rowptr[u + 1];
    const int pos_len = hi - lo;
    double cum = 0.0, dcg = 0.0, sum_pre = 0.0;
    int t = 0;
    for (int j = 0; j < k; ++j) {
        const bool hit = row_contains(gt_col, lo, hi, (int)topk_idx[(size_t)u * k + j]);
        if (hit_out) hit_out[(size_t)u * k + j] = hit ? 1 : 0;
        cum += hit ? 1.0 : 0.0;
        dcg += hit ? discount[j] : 0.0;
        sum_pre += (cum / (double)(j + 1)) * (hit ? 1.0 : 0.0);
        while (t < n_ks && ks[t] == j + 1) {
            const int cap = min(pos_len, k);                    // metrics.py:45-48,83-84
            // no ground truth (cap == 0): the reference's slices idcg[row, 0:] = idcg[row, -1] and ranges[0:] = ranges[-1]
            // hold the LAST entry, so ndcg and map are 0 / idcg_cum[k-1] and 0 / k, and recall is 0 / 0
            const int held = cap > 0 ? min(j, cap - 1) : k - 1;
            const int map_div = cap > 0 ? min(j + 1, cap) : k;
            double* o = out + ((size_t)u * 4) * n_ks + t;
            o[0 * n_ks] = cum / (double)pos_len;
            o[1 * n_ks] = dcg / idcg_cum[held];
            o[2 * n_ks] = cum / (double)(j + 1);
            o[3 * n_ks] = sum_pre / (double)map_div;
            ++t;
        }
    }
}

}  // namespace

extern "C" int mmrec_sample_negatives_i64(const int64_t* users, int32_t batch,
                                          const int32_t* hist_rowptr, const int32_t* hist_col,
                                          const int32_t* cand_items, int32_t n_cand, uint64_t seed,
                                          uint64_t counter, int64_t* out_neg, mmrec_stream_t stream) {
    if (batch < 0 || n_cand <= 0) return MMREC_ERR_BAD_ARG;
    if (batch == 0) return 0;
    if (!users || !hist_rowptr || !hist_col || !cand_items || !out_neg) return MMREC_ERR_BAD_ARG;
    hipLaunchKernelGGL(sample_negatives_kernel, dim3((batch + 255) / 256), dim3(256), 0,
                       mmrec_stream(stream), users, batch, hist_rowptr, hist_col, cand_items, n_cand, seed,
                       counter, out_neg);
    MMREC_RETURN_LAUNCH_STATUS();
}

extern "C" int mmrec_topk_metrics_f64(const int64_t* topk_idx, int32_t n_users, int32_t k,
                                      const int32_t* gt_rowptr, const int32_t* gt_col,
                                      const double* discount, const double* idcg_cum,
                                      const int32_t* ks, int32_t n_ks, uint8_t* hit_out,
                                      double* out_per_user, mmrec_stream_t stream) {
    if (n_users < 0 || k <= 0 || n_ks <= 0) return MMREC_ERR_BAD_ARG;
    if (n_users == 0) return 0;
    if (!topk_idx || !gt_rowptr || !gt_col || !discount || !idcg_cum || !ks || !out_per_user)
        return MMREC_ERR_BAD_ARG;
    hipLaunchKernelGGL(topk_metrics_kernel, dim3((n_users + 255) / 256), dim3(256), 0,
                       mmrec_stream(stream), topk_idx, n_users, k, gt_rowptr, gt_col, discount, idcg_cum, ks,
                       n_ks, hit_out, out_per_user);
    MMREC_RETURN_LAUNCH_STATUS();
}


// ---- host-side batch assembly: the reference's negative sampler, bit for bit, without the interpreter ------------
// `_sample_neg_ids` (dataloader.py:267-275) draws `random.sample(all_items, 1)[0]` per user and redraws while the item
// is in the user's history.  That call is one `_randbelow(n)`: `getrandbits(k)`, k = n.bit_length(), redrawn while
// >= n; and `getrandbits(k <= 32)` is one tempered 32-bit output of CPython's Mersenne Twister shifted right by
// 32 - k.  This function continues CPython's generator from its exported state (`random.getstate()`: 624 words + the
// index), consumes exactly the outputs the reference's loop would, and hands the state back -- same ids, same
// stream position for everything the run draws afterwards (shuffles, dropout seeds), ~10 us per 2048-user batch
// instead of ~0.75 ms of Python loop, which was most of an eager training step on the small datasets.
static inline uint32_t mt_next(uint32_t* mt, int32_t* idx) {
    if (*idx >= 624) {   // regenerate the block (MT19937 reference recurrence)
        int kk = 0;
        for (; kk < 624 - 397; ++kk) {
            const uint32_t y = (mt[kk] & 0x80000000u) | (mt[kk + 1] & 0x7fffffffu);
            mt[kk] = mt[kk + 397] ^ (y >> 1) ^ ((y & 1u) ? 0x9908b0dfu : 0u);
        }
        for (; kk < 623; ++kk) {
            const uint32_t y = (mt[kk] & 0x80000000u) | (mt[kk + 1] & 0x7fffffffu);
            mt[kk] = mt[kk + (397 - 624)] ^ (y >> 1) ^ ((y & 1u) ? 0x9908b0dfu : 0u);
        }
        const uint32_t y = (mt[623] & 0x80000000u) | (mt[0] & 0x7fffffffu);
        mt[623] = mt[396] ^ (y >> 1) ^ ((y & 1u) ? 0x9908b0dfu : 0u);
        *idx = 0;
    }
    uint32_t y = mt[(*idx)++];
    y ^= y >> 11;
    y ^= (y << 7) & 0x9d2c5680u;
    y ^= (y << 15) & 0xefc60000u;
    y ^= y >> 18;
    return y;
}

extern "C" int mmrec_host_sample_negatives(uint32_t* mt_state, int32_t* mt_index, const int64_t* users, int32_t batch,
                                           const int64_t* hist_rowptr, const int64_t* hist_items,
                                           const int64_t* all_items, int32_t n_all_items, int64_t* out) {
    if (batch < 0 || n_all_items <= 0) return MMREC_ERR_BAD_ARG;
    if (batch == 0) return 0;
    if (!mt_state || !mt_index || !users || !hist_rowptr || !hist_items || !all_items || !out) return MMREC_ERR_BAD_ARG;
    int k = 0;
    while ((n_all_items >> k) != 0) ++k;          // n.bit_length()
    const int shift = 32 - k;
    for (int32_t b = 0; b < batch; ++b) {
        const int64_t lo0 = hist_rowptr[users[b]], hi0 = hist_rowptr[users[b] + 1];
        for (;;) {
            uint32_t r = mt_next(mt_state, mt_index) >> shift;
            while (r >= (uint32_t)n_all_items) r = mt_next(mt_state, mt_index) >> shift;
            const int64_t cand = all_items[r];
            int64_t lo = lo0, hi = hi0;           // sorted history of the user
            while (lo < hi) {
                const int64_t mid = (lo + hi) >> 1;
                if (hist_items[mid] < cand) lo = mid + 1; else hi = mid;
            }
            if (!(lo < hi0 && hist_items[lo] == cand)) { out[b] = cand; break; }
        }
    }
    return 0;
}


// `random.sample(range(n), k)` of CPython 3.10 (LayerGCN's uniform edge pruning, layergcn.py:56-58), bit for bit and
// with the same consumption of the generator: for n <= 21 + 4^ceil(log4(3k)) (k > 5) the pool algorithm -- j =
// _randbelow(n - i), result = pool[j], pool[j] = pool[n - i - 1] -- otherwise rejection against the set of chosen
// indices.  0.025 s of Python per call at 118 k edges, every other epoch of a LayerGCN run.
static inline uint32_t mt_randbelow(uint32_t* mt, int32_t* idx, uint32_t n) {   // n >= 1
    int k = 0;
    while ((n >> k) != 0) ++k;
    uint32_t r = mt_next(mt, idx) >> (32 - k);
    while (r >= n) r = mt_next(mt, idx) >> (32 - k);
    return r;
}

extern "C" int mmrec_host_random_sample_range(uint32_t* mt_state, int32_t* mt_index, int32_t n, int32_t k,
                                              int64_t* out, int32_t* scratch) {
    if (n < 0 || k < 0 || k > n) return MMREC_ERR_BAD_ARG;
    if (k == 0) return 0;
    if (!mt_state || !mt_index || !out || !scratch) return MMREC_ERR_BAD_ARG;   // scratch: n int32
    double setsize = 21.0;
    if (k > 5) setsize += pow(4.0, ceil(log((double)k * 3.0) / log(4.0)));
    if ((double)n <= setsize) {
        for (int32_t i = 0; i < n; ++i) scratch[i] = i;                  // pool = list(population)
        for (int32_t i = 0; i < k; ++i) {
            const uint32_t j = mt_randbelow(mt_state, mt_index, (uint32_t)(n - i));
            out[i] = scratch[j];
            scratch[j] = scratch[n - i - 1];
        }
    } else {
        for (int32_t i = 0; i < n; ++i) scratch[i] = 0;                  // selected = set()
        for (int32_t i = 0; i < k; ++i) {
            uint32_t j = mt_randbelow(mt_state, mt_index, (uint32_t)n);
            while (scratch[j]) j = mt_randbelow(mt_state, mt_index, (uint32_t)n);
            scratch[j] = 1;
            out[i] = j;
        }
    }
    return 0;
}
