// Ablation probe for the fp32 dX kernel (gemm64_stream_kernel, mfma_stream.h), built with the mask on the command line:
//   for m in 0 256 512; do hipcc --offload-arch=gfx950 -O3 -std=c++17 -DBX_PROBE_MASK=$m tools/gemm_bx_probe.hip \
//       -o tools/gemm_bx_probe_$m.bin; done
// 256: no stores, 512: 1/8 of the MFMAs
#ifndef BX_PROBE_MASK
#define BX_PROBE_MASK 0
#endif
#define MMREC_STREAM_PROBE BX_PROBE_MASK      // (read by mfma_stream.h, which gemm.hip includes)
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include "../mmrec_amd/csrc/gemm.hip"
int main(int argc, char** argv) {
    const int n = argc > 1 ? atoi(argv[1]) : 7050, F = 4096;
    float *G, *W, *dX;
    hipMalloc(&G, (size_t)n * 64 * 4); hipMalloc(&W, 64 * F * 4); hipMalloc(&dX, (size_t)n * F * 4);
    hipMemset(G, 0x3c, (size_t)n * 64 * 4); hipMemset(W, 0x3c, 64 * F * 4);
    hipEvent_t e0, e1; hipEventCreate(&e0); hipEventCreate(&e1);
    for (int i = 0; i < 3; ++i) mmrec_linear_bwd_x_f32(G, W, dX, n, F, 64, nullptr);
    hipDeviceSynchronize();
    hipEventRecord(e0);
    const int reps = 20;
    for (int i = 0; i < reps; ++i) mmrec_linear_bwd_x_f32(G, W, dX, n, F, 64, nullptr);
    hipEventRecord(e1); hipEventSynchronize(e1);
    float ms; hipEventElapsedTime(&ms, e0, e1);
    printf("dX n %d mask %3d : %.1f us / call  %.1f TF  %.2f TB/s written\n", n, BX_PROBE_MASK, ms / reps * 1e3,
           2.0 * n * F * 64 / (ms / reps * 1e-3) / 1e12, (double)n * F * 4 / (ms / reps * 1e-3) / 1e12);
    return 0;
}
