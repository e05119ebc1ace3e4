// The dense layer of the reduction_1x1 chains on v_mfma_f32_32x32x2_f32, shared by the forward kernel (reduc.hip) and
// the backward-data kernel (reduc_bwd.hip).  See reduc.hip's header for the mapping: weights are the A operand, the
// 32-pixel activation tile the B operand, and the D tile of one layer (channel in register, pixel on lane) is the B
// operand of the next.
#pragma once
#include <hip/hip_runtime.h>
#include "common.h"

// One dense layer: acc[mt] (32 out-rows each) = W * x, K real input channels (multiple of 8).
// wf points at this layer's fragments: float4 index ((mt*(K/8) + g)*64 + lane).
template <int K, int MT, int NX>
__device__ __forceinline__ void dense_layer(const float4* __restrict__ wf, int lane, const float (&x)[NX],
                                            f32x16 (&acc)[MT]) {
    static_assert(NX >= K / 2, "activation registers");
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[mt][r] = 0.f;
    // software-prefetch one g-step of weight fragments; the sched_barrier keeps hipcc from
    // hoisting every ds_read of the layer to its top (which spills: 64 x b128 for 128->128)
    float4 wn[MT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) wn[mt] = wf[(mt * (K / 8)) * 64 + lane];
#pragma unroll
    for (int g = 0; g < K / 8; ++g) {
        float4 w[MT];
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) w[mt] = wn[mt];
        if (g + 1 < K / 8) {
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) wn[mt] = wf[(mt * (K / 8) + g + 1) * 64 + lane];
        }
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) {
            acc[mt] = mfma32x2(w[mt].x, x[4 * g + 0], acc[mt]);
            acc[mt] = mfma32x2(w[mt].y, x[4 * g + 1], acc[mt]);
            acc[mt] = mfma32x2(w[mt].z, x[4 * g + 2], acc[mt]);
            acc[mt] = mfma32x2(w[mt].w, x[4 * g + 3], acc[mt]);
        }
        __builtin_amdgcn_sched_barrier(0);
    }
}

// float4s of one layer's fragments: `rows` outputs padded to 32-row tiles, `k` inputs (multiple of 8)
constexpr long layer_frag_float4s(int rows, int k) { return (long)((rows + 31) / 32) * (k / 8) * 64; }

// float4s of a whole chain's forward fragments (num_in_filters = c0, num_out_filters = m0, bts.py:105-122)
constexpr long chain_frag_float4s_of(int c0, int m0) {
    long n = 0;
    int k = c0, m = m0;
    while (m >= 8) { n += layer_frag_float4s(m, k); k = m; m = m / 2; }
    return n + layer_frag_float4s(1, k);
}

template <int C0, int M0>
constexpr long chain_frag_float4s() { return chain_frag_float4s_of(C0, M0); }
