// Shared declarations for the gfx950 BTS hot-path kernels.
#pragma once
#include <hip/hip_runtime.h>
#include <atomic>
#include "../../include/bts_hip.h"

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

// v_mfma_f32_32x32x2_f32: D[32x32] += A[32x2] * B[2x32], exact f32 (fmaf chain).
// lane l supplies A[i = l&31][k = l>>5] and B[k = l>>5][j = l&31];
// D register r of lane l is D[row = (r&3) + 8*(r>>2) + 4*(l>>5)][col = l&31].
__device__ __forceinline__ f32x16 mfma32x2(float a, float b, f32x16 c) {
    return __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c, 0, 0, 0);
}

// nn.ELU(alpha=1) and nn.Sigmoid on the hardware exponential (v_exp_f32 behind one multiply) and reciprocal: ~3 and ~5 VALU
// instructions where expm1f / expf + an IEEE division cost ~35 / ~30.  The decoder applies ELU to every output of every
// convolution (860 M elements per B=16 step) and 32 times per pixel group inside the reduction chains, so the accurate
// forms were a measurable share of those kernels' issue slots.  exp(x) - 1 is ATen's own ELU formula; its absolute error
// (<= 1e-7, relative to an O(1) activation scale) is what matters downstream -- the relative error near x = 0, where
// expm1f differs, does not survive the next layer's sum.  Parity: the oracle / golden tolerances are unchanged (tests).
__device__ __forceinline__ float elu1(float x) { return x > 0.f ? x : __expf(x) - 1.f; }
__device__ __forceinline__ float sigmoid1(float x) { return __frcp_rn(1.f + __expf(-x)); }

// Table-driven launches (weight packs, batched weight gradients, AdamW): a device table holds one record per problem with
// a prefix sum of workgroups in the member `first`; the record whose range holds this workgroup is the last one with
// first <= blockIdx.x.  Uniform per workgroup: integer code on scalar registers.
template <typename T>
__device__ __forceinline__ int bts_table_find(const T* __restrict__ table, int n, long T::*first) {
    int lo = 0, hi = n - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (table[mid].*first <= (long)blockIdx.x) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// The fixed-order sum of split partials shared by the weight-gradient reduce kernels (wgrad.hip, conv_grouped_wgrad.inc): 16
// lanes walk the splits of one float4 element -- lane j adds splits j, j + 16, ... in ascending order, four independent loads
// in flight added as (a0 + a1) + (a2 + a3), then one at a time -- and lane 0 adds the 16 lane sums in lane order.
// p = split 0's float4, step = float4s from one split to the next.
__device__ __forceinline__ f32x4 sum_splits(const f32x4* __restrict__ p, size_t step, int ksplit, int lane) {
    f32x4 v = (f32x4)(0.f);
    int s = lane;
    for (; s + 48 < ksplit; s += 64) {
        const f32x4 a0 = p[(size_t)s * step], a1 = p[(size_t)(s + 16) * step];
        const f32x4 a2 = p[(size_t)(s + 32) * step], a3 = p[(size_t)(s + 48) * step];
        v += (a0 + a1) + (a2 + a3);
    }
    for (; s < ksplit; s += 16) v += p[(size_t)s * step];
    return v;
}

__device__ __forceinline__ f32x4 sum_lanes(const f32x4 (&red)[16][16], int el) {
    f32x4 r = red[0][el];
#pragma unroll
    for (int j = 1; j < 16; ++j) r += red[j][el];
    return r;
}

// Raise a kernel's dynamic-LDS limit above the 64 KB default.  hipFuncAttributeMaxDynamicSharedMemorySize is a property
// of (function, DEVICE): a process that drives several GPUs (nn.DataParallel: one Python thread per device,
// bts_test.py:91) must set it on each of them.  `done` is one bit per device ordinal, one word per kernel (lds_set
// below); the only library state that is ever written after load, idempotent (setting the attribute twice is harmless)
// and lock-free, so concurrent callers on any mix of devices and streams are safe.
inline hipError_t bts_ensure_dynamic_lds(const void* kern, size_t bytes, std::atomic<unsigned long long>& done) {
    if (bytes < 64 * 1024) return hipSuccess;
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    const unsigned long long bit = (dev >= 0 && dev < 64) ? 1ull << dev : 0ull;      // ordinals >= 64: set every time
    if (bit && (done.load(std::memory_order_acquire) & bit)) return hipSuccess;
    e = hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
    if (e != hipSuccess) return e;
    if (bit) done.fetch_or(bit, std::memory_order_release);
    return hipSuccess;
}

// The one way the library enqueues a kernel that may need more than 64 KB of dynamic LDS: raise Kern's limit on the current
// device if `lds_bytes` asks for it, then launch.  Returns the attribute step's error, or 0 with the kernel enqueued; the
// caller reads hipGetLastError after its last launch.
template <auto Kern> inline std::atomic<unsigned long long> lds_set{0};      // per kernel: one bit per device
template <auto Kern, typename... Args>
int bts_launch(dim3 grid, dim3 block, size_t lds_bytes, hipStream_t s, const Args&... args) {
    if (hipError_t e = bts_ensure_dynamic_lds((const void*)Kern, lds_bytes, lds_set<Kern>); e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(Kern, grid, block, lds_bytes, s, args...);
    return 0;
}
