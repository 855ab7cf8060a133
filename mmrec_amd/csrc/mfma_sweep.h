// The fp32-MFMA sweep of an operand's rows against a whole table (score_lse.hip, tri_topk.hip), D = 64 or 128 wide.
// A 256-thread workgroup (4 waves) OWNS SWEEP_OWN = 128 rows, a wave 32 of them, their fragment in registers for the whole
// walk: lane (i, h) = (lane & 31, lane >> 5) holds own[i][2 s + h].  The OTHER operand reaches the waves through LDS in tiles
// of SWEEP_TILE = 64 rows, fetched one tile ahead (sweep_fetch under the previous tile's MFMAs, sweep_stage between two
// barriers).
//
// THE TILE LAYOUT (defined here and nowhere else).  A row has the pitch D + 4 floats (16 B aligned; 16 consecutive rows lie on
// 64 different banks) and is stored DE-INTERLEAVED: column k at position (k & 1) * (D / 2) + (k >> 1), the even k in the first
// half of the row, the odd k in the second.  Lane (i, h) then reads its MFMA operands of four consecutive steps,
// tile[i][2 s + h] for s = 4 q .. 4 q + 3, as ONE conflict-free 16-byte LDS read, and the contraction still runs in natural k
// order:  score(other o, own i) = the fma chain over k = 0 .. D - 1 of other[o][k] * own[i][k]  (v_mfma_f32_32x32x2_f32, bitwise
// that chain).  With the tile as the A operand a lane holds 16 others of ONE own row: D[other = d_row(r, lane)][own = lane & 31].
#pragma once
#include "mfma_stream.h"

namespace {

constexpr int SWEEP_OWN = 128;
constexpr int SWEEP_TILE = 64;

struct SweepPlan {
    int own_tiles, oth_tiles, per, splits;     // per: tiles of the other operand per split
};
// own tiles x splits of the other operand: about `target` workgroups, at most `cap` splits.  A function of the two sizes only
// (never of data): capturable, and the same call always has the same plan.
inline SweepPlan sweep_plan(long n_own, long n_oth, int target, int cap) {
    SweepPlan p;
    p.own_tiles = (int)((n_own + SWEEP_OWN - 1) / SWEEP_OWN);
    p.oth_tiles = (int)((n_oth + SWEEP_TILE - 1) / SWEEP_TILE);
    const long own = p.own_tiles > 0 ? p.own_tiles : 1;
    long want = (target + own - 1) / own;
    if (want > cap) want = cap;
    if (want > p.oth_tiles) want = p.oth_tiles;
    if (want < 1) want = 1;
    p.per = (int)((p.oth_tiles + want - 1) / want);
    if (p.per < 1) p.per = 1;
    p.splits = (p.oth_tiles + p.per - 1) / p.per;
    return p;
}

// the lane's own fragment own[2 s + h] of the row at `row`; zeros where the caller says the row is absent.  `row` is read
// either way (the caller points an absent row at row 0 of the table): 32 or 64 loads in flight and a select, no branch.
template <int D>
__device__ __forceinline__ void sweep_own(float (&own)[D / 2], const float* row, bool present, int h) {
#pragma unroll
    for (int s = 0; s < D / 2; ++s) {
        const float v = row[2 * s + h];
        own[s] = present ? v : 0.f;
    }
}

// rows o0 .. o0 + 63 of a [n, D] table into registers, coalesced 16-byte loads; rows past n read as zeros
template <int D>
__device__ __forceinline__ void sweep_fetch(float4 (&pre)[D / 16], const float* __restrict__ tab, int o0, int n, int tid) {
#pragma unroll
    for (int j = 0; j < D / 16; ++j) {
        const int e = tid + 256 * j, r = e / (D / 4), c4 = e % (D / 4);
        pre[j] = ld4_guard(tab + (size_t)(o0 + r < n ? o0 + r : 0) * D + 4 * c4, o0 + r < n);
    }
}

// ... and from the registers into the tile, de-interleaved
template <int D>
__device__ __forceinline__ void sweep_stage(float* __restrict__ T, const float4 (&pre)[D / 16], int tid) {
#pragma unroll
    for (int j = 0; j < D / 16; ++j) {
        const int e = tid + 256 * j, r = e / (D / 4), c4 = e % (D / 4);
        float* row = T + r * (D + 4);
        *reinterpret_cast<float2*>(row + 2 * c4) = make_float2(pre[j].x, pre[j].z);             // k = 4 c4, 4 c4 + 2
        *reinterpret_cast<float2*>(row + D / 2 + 2 * c4) = make_float2(pre[j].y, pre[j].w);     // k = 4 c4 + 1, + 3
    }
}

// the scores of the 32-row sub-tile u of the tile against the wave's 32 own rows: D / 8 LDS reads, four MFMAs each
template <int D>
__device__ __forceinline__ f32x16 sweep_scores(const float* __restrict__ T, int u, int i, int h, const float (&own)[D / 2]) {
    f32x16 acc = {0};
    const float* tr = T + (32 * u + i) * (D + 4) + h * (D / 2);
#pragma unroll
    for (int q4 = 0; q4 < D / 8; ++q4) {
        const float4 a = *reinterpret_cast<const float4*>(tr + 4 * q4);
        acc = mfma32(a.x, own[4 * q4 + 0], acc);
        acc = mfma32(a.y, own[4 * q4 + 1], acc);
        acc = mfma32(a.z, own[4 * q4 + 2], acc);
        acc = mfma32(a.w, own[4 * q4 + 3], acc);
    }
    return acc;
}

// orders a wave's accesses to LDS that is private to it: a wave's LDS operations complete in order, so no barrier, only the
// compiler must keep the order
__device__ __forceinline__ void wave_lds_order() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

}  // namespace
