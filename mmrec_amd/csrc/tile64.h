// [64 rows] x [64, 64] products on a 256-thread workgroup, fp32 VALU fma, both operands in LDS: the stage of the row-wise fusers
// (modal_fusion.hip, encoder_heads.hip, gcn_layer.hip: the whole plan below; spectrum.hip: transposed tiles filled from
// registers, t64_stage_nn, its own finish).
//
// Every tile and every matrix is 64 x 64 floats with rows of T64_LD = 68 floats (float4 aligned, and 17 sixteen-byte slots: the
// 16 lanes of a read that walk 16 rows hit 16 different slots).  Thread (rg, sg) = (tid / 16, tid % 16) always owns the tile
// rows 4 rg .. 4 rg + 3.  Two forms, named after the BLAS letters of their second operand:
//   t64_stage_nt  out[r][c] += sum over s of A[r][s] B[c][s]     the thread's columns are c = sg + 16 j  (j = 0 .. 3): layout L1
//   t64_stage_nn  out[r][c] += sum over s of T[s][r] M[s][c]     the thread's columns are c = 4 sg + j   (j = 0 .. 3): layout L0
//
// THE PLAN OF A FUSER (what the fuzz tests' error bounds count; each file adds its own formulas, LDS and workspace sizes).
//   blocks       one workgroup per block of R = t64_fuser_rows(n) consecutive rows, walked as R / 64 tiles of 64 rows: 64 rows
//                while T64_FUSER_BLOCKS = 256 workgroups cover the table, then more tiles per workgroup.  Rows past n are zero in
//                every tile and are never stored.
//   stage        the summed index s ASCENDS and every term is one fmaf onto the accumulator the caller passes in (a bias, another
//                stage's result, a table's rows, or zeros): an output meets 64 roundings per stage, nothing else.
//   weight       dW = one fma chain over the block's rows in order (t64_stage_nn over tile after tile onto one accumulator),
//   partials     stored per block (t64_part_store) into the workspace.
//   column sums  a thread adds its four rows in order, tile after tile, from 0: R / 16 additions; then the 16 row groups are added
//                in order from 0 (t64_colsum): 16 more; the result is the block's partial.
//   finish       a second launch, 64 partial floats per workgroup: thread (quarter, c) adds the blocks quarter, quarter + 4, ...
//                in order from 0, then the four quarters are added in order (t64_finish_sum): F = ceil(blocks / 4) + 3 additions.
//                So a column sum is R / 16 + 16 + F additions, a weight gradient a chain of R fmas and F additions.
//   NO ATOMICS, every order fixed by n (and the op's own counts) alone.
#pragma once
#include "common.h"

constexpr int T64 = 64;
constexpr int T64_LD = 68;
constexpr int T64_FLOATS = T64 * T64_LD;
constexpr int T64_BLOCK = 256;
constexpr int T64_FUSER_BLOCKS = 256;
constexpr int64_t T64_MAX_ROWS = (int64_t)1 << 30;
enum T64Layout { T64_L0, T64_L1 };

// the plan of a fuser: 64 rows per workgroup while max_blocks workgroups cover the n rows, then more tiles per workgroup
static inline int t64_rows_per_block(int64_t n, int max_blocks) {
    const int64_t t = (n + (int64_t)T64 * max_blocks - 1) / ((int64_t)T64 * max_blocks);
    return (int)(t < 1 ? 1 : t) * T64;
}
static inline int t64_blocks(int64_t n, int max_blocks) {
    return n <= 0 ? 0 : (int)((n + t64_rows_per_block(n, max_blocks) - 1) / t64_rows_per_block(n, max_blocks));
}
static inline int t64_fuser_rows(int64_t n) { return t64_rows_per_block(n, T64_FUSER_BLOCKS); }
static inline int t64_fuser_blocks(int64_t n) { return t64_blocks(n, T64_FUSER_BLOCKS); }

// the first row of the workgroup's t-th tile (the walk ends at the first row0 >= n)
__device__ __forceinline__ long t64_row0(int t, int tiles) { return ((long)blockIdx.x * tiles + t) * T64; }

__device__ __forceinline__ float t64_leaky(float z, float slope) { return z > 0.f ? z : slope * z; }
__device__ __forceinline__ float t64_dleaky(float z, float slope) { return z > 0.f ? 1.f : slope; }

// a row-major [64][64] matrix of global memory into an LDS image with T64_LD rows (visible after the caller's next barrier)
__device__ __forceinline__ void t64_matrix(float* __restrict__ L, const float* __restrict__ g) {
    for (int e = threadIdx.x; e < T64 * T64 / 4; e += T64_BLOCK) {
        const int r = e / 16, c = 4 * (e % 16);
        *reinterpret_cast<float4*>(L + r * T64_LD + c) = *reinterpret_cast<const float4*>(g + r * T64 + c);
    }
}

// the same of a [64][64] block whose rows lie ld floats apart (ld a multiple of 4: one half of a [64][128] matrix)
__device__ __forceinline__ void t64_matrix_ld(float* __restrict__ L, const float* __restrict__ g, int ld) {
    for (int e = threadIdx.x; e < T64 * T64 / 4; e += T64_BLOCK) {
        const int r = e / 16, c = 4 * (e % 16);
        *reinterpret_cast<float4*>(L + r * T64_LD + c) = *reinterpret_cast<const float4*>(g + (size_t)r * ld + c);
    }
}

// ... and TRANSPOSED: L[c][r] = g[r ld + c]
__device__ __forceinline__ void t64_matrix_ld_t(float* __restrict__ L, const float* __restrict__ g, int ld) {
    for (int e = threadIdx.x; e < T64 * T64 / 4; e += T64_BLOCK) {
        const int r = e / 16, c = 4 * (e % 16);
        const float4 v = *reinterpret_cast<const float4*>(g + (size_t)r * ld + c);
        L[c * T64_LD + r] = v.x;
        L[(c + 1) * T64_LD + r] = v.y;
        L[(c + 2) * T64_LD + r] = v.z;
        L[(c + 3) * T64_LD + r] = v.w;
    }
}

// rows row0 .. row0 + 63 of a [n, 64] table into a row-major tile; rows past n, and a NULL table, read as zeros
__device__ __forceinline__ void t64_load(float* __restrict__ R, const float* __restrict__ g, long row0, long n, int rg, int sg) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const long r = row0 + 4 * rg + i;
        *reinterpret_cast<float4*>(R + (4 * rg + i) * T64_LD + 4 * sg) =
            (g && r < n) ? *reinterpret_cast<const float4*>(g + (size_t)r * T64 + 4 * sg) : f4_zero();
    }
}

// rows row0 + 4 rg + i of a [n, 64] table at the columns 4 sg .. + 3 into registers (layout L0); rows past n read as zeros
__device__ __forceinline__ void t64_rows(float4 (&v)[4], const float* __restrict__ g, long row0, long n, int rg, int sg) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const long r = row0 + 4 * rg + i;
        v[i] = r < n ? *reinterpret_cast<const float4*>(g + (size_t)r * T64 + 4 * sg) : f4_zero();
    }
}

// layout L0 (rows 4 rg + i, columns 4 sg .. + 3) to a [n, 64] table; rows past n are not stored
__device__ __forceinline__ void t64_store(float* __restrict__ g, long row0, long n, int rg, int sg, const float4 (&v)[4]) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const long r = row0 + 4 * rg + i;
        if (r < n) *reinterpret_cast<float4*>(g + (size_t)r * T64 + 4 * sg) = v[i];
    }
}

// layout L1 (rows 4 rg + i, columns sg + 16 j) to a [n, 64] table; rows past n are not stored
__device__ __forceinline__ void t64_store1(float* g, long row0, long n, int rg, int sg, const float (&v)[4][4]) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const long r = row0 + 4 * rg + i;
        if (r < n) {
#pragma unroll
            for (int j = 0; j < 4; ++j) g[(size_t)r * T64 + sg + 16 * j] = v[i][j];
        }
    }
}

// where a stage's accumulators start: at vec (64 floats, one per column) in layout L1 or L0, or at zero
__device__ __forceinline__ void t64_start1(float (&acc)[4][4], const float* __restrict__ vec, int sg) {
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = vec[sg + 16 * j];
}
__device__ __forceinline__ void t64_start0(float4 (&acc)[4], const float* __restrict__ vec, int sg) {
    acc[0] = acc[1] = acc[2] = acc[3] = *reinterpret_cast<const float4*>(vec + 4 * sg);
}
__device__ __forceinline__ void t64_zero(float (&acc)[4][4]) {
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = 0.f;
}
__device__ __forceinline__ void t64_zero(float4 (&acc)[4]) {
#pragma unroll
    for (int i = 0; i < 4; ++i) acc[i] = f4_zero();
}

// acc[i][j] += sum_s A[4 rg + i][s] B[sg + 16 j][s], s ascending
__device__ __forceinline__ void t64_stage_nt(const float* __restrict__ A, const float* __restrict__ B, int rg, int sg,
                                             float (&acc)[4][4]) {
    const float* __restrict__ a = A + 4 * rg * T64_LD;
    const float* __restrict__ b = B + sg * T64_LD;
#pragma unroll 2
    for (int s = 0; s < T64; s += 4) {
        float4 av[4], bv[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) av[i] = *reinterpret_cast<const float4*>(a + i * T64_LD + s);
#pragma unroll
        for (int j = 0; j < 4; ++j) bv[j] = *reinterpret_cast<const float4*>(b + 16 * j * T64_LD + s);
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                float c = acc[i][j];
                c = fmaf(av[i].x, bv[j].x, c);
                c = fmaf(av[i].y, bv[j].y, c);
                c = fmaf(av[i].z, bv[j].z, c);
                c = fmaf(av[i].w, bv[j].w, c);
                acc[i][j] = c;
            }
    }
}

// acc[i] (columns 4 sg .. + 3) += sum_s T[s][4 rg + i] M[s][4 sg .. + 3], s ascending
__device__ __forceinline__ void t64_stage_nn(const float* __restrict__ T, const float* __restrict__ M, int rg, int sg,
                                             float4 (&acc)[4]) {
#pragma unroll 8
    for (int s = 0; s < T64; ++s) {
        const float4 t = *reinterpret_cast<const float4*>(T + s * T64_LD + 4 * rg);
        const float4 m = *reinterpret_cast<const float4*>(M + s * T64_LD + 4 * sg);
        acc[0] = f4_fma(t.x, m, acc[0]);
        acc[1] = f4_fma(t.y, m, acc[1]);
        acc[2] = f4_fma(t.z, m, acc[2]);
        acc[3] = f4_fma(t.w, m, acc[3]);
    }
}

// layout L1 values (rows 4 rg + i, columns sg + 16 j) into a row-major tile R and, where Tt is given, its transpose
__device__ __forceinline__ void t64_put(float* __restrict__ R, float* __restrict__ Tt, int rg, int sg, const float (&v)[4][4]) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int c = sg + 16 * j;
#pragma unroll
        for (int i = 0; i < 4; ++i) R[(4 * rg + i) * T64_LD + c] = v[i][j];
        if (Tt) *reinterpret_cast<float4*>(Tt + c * T64_LD + 4 * rg) = make_float4(v[0][j], v[1][j], v[2][j], v[3][j]);
    }
}

// layout L0 values (rows 4 rg + i, columns 4 sg .. + 3) into a row-major tile, as float4s or as v[i][j] at the column 4 sg + j
__device__ __forceinline__ void t64_put0(float* __restrict__ R, int rg, int sg, const float4 (&v)[4]) {
#pragma unroll
    for (int i = 0; i < 4; ++i) *reinterpret_cast<float4*>(R + (4 * rg + i) * T64_LD + 4 * sg) = v[i];
}
__device__ __forceinline__ void t64_put0(float* __restrict__ R, int rg, int sg, const float (&v)[4][4]) {
#pragma unroll
    for (int i = 0; i < 4; ++i)
        *reinterpret_cast<float4*>(R + (4 * rg + i) * T64_LD + 4 * sg) = make_float4(v[i][0], v[i][1], v[i][2], v[i][3]);
}

// ... and back
__device__ __forceinline__ void t64_get0(float4 (&v)[4], const float* __restrict__ R, int rg, int sg) {
#pragma unroll
    for (int i = 0; i < 4; ++i) v[i] = *reinterpret_cast<const float4*>(R + (4 * rg + i) * T64_LD + 4 * sg);
}

// layout L0 values into a TRANSPOSED tile: Tt[4 sg + j][4 rg .. + 3]
__device__ __forceinline__ void t64_put_t(float* __restrict__ Tt, int rg, int sg, const float4 (&v)[4]) {
    float* __restrict__ p = Tt + 4 * sg * T64_LD + 4 * rg;
    *reinterpret_cast<float4*>(p) = make_float4(v[0].x, v[1].x, v[2].x, v[3].x);
    *reinterpret_cast<float4*>(p + T64_LD) = make_float4(v[0].y, v[1].y, v[2].y, v[3].y);
    *reinterpret_cast<float4*>(p + 2 * T64_LD) = make_float4(v[0].z, v[1].z, v[2].z, v[3].z);
    *reinterpret_cast<float4*>(p + 3 * T64_LD) = make_float4(v[0].w, v[1].w, v[2].w, v[3].w);
}

// a block's [64][64] weight partial from the L0 accumulators of a t64_stage_nn chain
__device__ __forceinline__ void t64_part_store(float* __restrict__ p, int rg, int sg, const float4 (&w)[4]) {
#pragma unroll
    for (int i = 0; i < 4; ++i) *reinterpret_cast<float4*>(p + (4 * rg + i) * T64 + 4 * sg) = w[i];
}

// K column sums at once: the 16 row groups' cs[k] (of the columns of layout lay[k]) through a dead tile red, one barrier, then
// thread c + 64 k adds the 16 in order from 0 into dst[c + 64 k].  The caller's next barrier frees red.
template <int K>
__device__ __forceinline__ void t64_colsum(float* __restrict__ red, int rg, int sg, const T64Layout (&lay)[K],
                                           const float (&cs)[K][4], float* __restrict__ dst) {
#pragma unroll
    for (int k = 0; k < K; ++k)
#pragma unroll
        for (int j = 0; j < 4; ++j) red[(rg * K + k) * T64 + (lay[k] == T64_L1 ? sg + 16 * j : 4 * sg + j)] = cs[k][j];
    __syncthreads();
    if (threadIdx.x < K * T64) {
        float a = 0.f;
        for (int q = 0; q < 16; ++q) a += red[q * K * T64 + threadIdx.x];
        dst[threadIdx.x] = a;
    }
}

// the finish of the partials: this workgroup's 64 floats o = 64 blockIdx.x + c of a partial, the blocks' partials stride floats
// apart.  Thread (quarter, c) adds the blocks quarter, quarter + 4, ... in order from 0, then the four quarters are added in
// order; true for the 64 threads that hold a sum
__device__ __forceinline__ bool t64_finish_sum(const float* __restrict__ part, int nb, size_t stride, int& o, float& a) {
    __shared__ float s[4][T64];
    const int quarter = threadIdx.x / T64, c = threadIdx.x % T64;
    o = blockIdx.x * T64 + c;
    a = 0.f;
    for (int blk = quarter; blk < nb; blk += 4) a += part[blk * stride + o];
    s[quarter][c] = a;
    __syncthreads();
    if (quarter) return false;
    a = s[0][c];
    a += s[1][c];
    a += s[2][c];
    a += s[3][c];
    return true;
}

// a launch of T64_BLOCK threads with more dynamic LDS than a kernel gets by default: the attribute is asked for once per device
// and kernel, outside any launch.  Nonzero: the runtime's error, nothing launched; the launch's own status is the caller's to read
template <auto Kernel, typename... Args>
static inline int t64_launch(int blocks, size_t lds_bytes, hipStream_t stream, Args... args) {
    static bool done[64];
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return (int)e;
    if (dev < 0 || dev >= 64 || !done[dev]) {
        e = hipFuncSetAttribute(reinterpret_cast<const void*>(Kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
        if (e != hipSuccess) return (int)e;
        if (dev >= 0 && dev < 64) done[dev] = true;
    }
    hipLaunchKernelGGL(Kernel, dim3(blocks), dim3(T64_BLOCK), lds_bytes, stream, args...);
    return 0;
}
