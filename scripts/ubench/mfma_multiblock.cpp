// Micro-benchmark: the rate of the multi-block fp32 MFMA (v_mfma_f32_16x16x1_4b_f32, what conv_grouped_kernel issues)
// beside v_mfma_f32_16x16x4_f32 and v_mfma_f32_32x32x2_f32, registers only, four independent accumulators per wave,
// one and two workgroups of four waves per CU.  Build: hipcc --offload-arch=gfx950 -O3
#include <hip/hip_runtime.h>
#include <cstdio>
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

// FORM 0: 16x16x1_4b (2048 FLOP), 1: 16x16x4 (2048 FLOP), 2: 32x32x2 (4096 FLOP)
template <int FORM>
__global__ __launch_bounds__(256) void k(float* out, int iters) {
    const int lane = threadIdx.x & 63;
    const float a = 1.0f + lane * 1e-3f, b = 0.5f - lane * 1e-3f;
    float s = 0.f;
    if (FORM == 1) {
        f32x4 acc[4];
        for (int t = 0; t < 4; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
        for (int it = 0; it < iters; ++it) {
#pragma unroll
            for (int u = 0; u < 16; ++u) {
                acc[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, acc[0], 0, 0, 0);
                acc[1] = __builtin_amdgcn_mfma_f32_16x16x4f32(b, a, acc[1], 0, 0, 0);
                acc[2] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, a, acc[2], 0, 0, 0);
                acc[3] = __builtin_amdgcn_mfma_f32_16x16x4f32(b, b, acc[3], 0, 0, 0);
            }
        }
        for (int t = 0; t < 4; ++t) for (int r = 0; r < 4; ++r) s += acc[t][r];
    } else {
        f32x16 acc[4];
        for (int t = 0; t < 4; ++t) for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;
        for (int it = 0; it < iters; ++it) {
#pragma unroll
            for (int u = 0; u < 16; ++u) {
                if (FORM == 0) {
                    acc[0] = __builtin_amdgcn_mfma_f32_16x16x1f32(a, b, acc[0], 0, 0, 0);
                    acc[1] = __builtin_amdgcn_mfma_f32_16x16x1f32(b, a, acc[1], 0, 0, 0);
                    acc[2] = __builtin_amdgcn_mfma_f32_16x16x1f32(a, a, acc[2], 0, 0, 0);
                    acc[3] = __builtin_amdgcn_mfma_f32_16x16x1f32(b, b, acc[3], 0, 0, 0);
                } else {
                    acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, acc[0], 0, 0, 0);
                    acc[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(b, a, acc[1], 0, 0, 0);
                    acc[2] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, a, acc[2], 0, 0, 0);
                    acc[3] = __builtin_amdgcn_mfma_f32_32x32x2f32(b, b, acc[3], 0, 0, 0);
                }
            }
        }
        for (int t = 0; t < 4; ++t) for (int r = 0; r < 16; ++r) s += acc[t][r];
    }
    out[blockIdx.x * 256 + threadIdx.x] = s;
}

template <int FORM>
void run(const char* name, int blocks_per_cu, int iters, double flop_per_mfma) {
    float* out;
    const int blocks = 256 * blocks_per_cu;
    if (hipMalloc(&out, sizeof(float) * blocks * 256) != hipSuccess) { printf("hipMalloc failed\n"); return; }
    hipEvent_t s, e;
    hipEventCreate(&s); hipEventCreate(&e);
    hipLaunchKernelGGL(k<FORM>, dim3(blocks), dim3(256), 0, 0, out, iters);
    hipDeviceSynchronize();
    float best = 1e9f;
    for (int r = 0; r < 5; ++r) {
        hipEventRecord(s);
        hipLaunchKernelGGL(k<FORM>, dim3(blocks), dim3(256), 0, 0, out, iters);
        hipEventRecord(e);
        hipEventSynchronize(e);
        float ms; hipEventElapsedTime(&ms, s, e);
        if (ms < best) best = ms;
    }
    const double flops = (double)blocks * 4 /*waves*/ * iters * 64.0 * flop_per_mfma;
    printf("%-28s blocks/CU %d: %8.3f ms  %7.1f TFLOP/s\n", name, blocks_per_cu, best, flops / best / 1e9);
    hipFree(out);
}

int main() {
    for (int bpc = 1; bpc <= 2; ++bpc) {
        run<0>("v_mfma_f32_16x16x1_4b_f32", bpc, 4000, 2048.0);
        run<1>("v_mfma_f32_16x16x4_f32", bpc, 4000, 2048.0);
        run<2>("v_mfma_f32_32x32x2_f32", bpc, 4000, 4096.0);
    }
    return 0;
}
