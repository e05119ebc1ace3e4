// reduction_1x1 (+ F.normalize + LPG + /max_depth) BACKWARD-DATA for gfx950: what autograd through reference
// pytorch/bts.py:124-136, 249-256 (263-270, 277-283) computes for the chain's input, in one launch per scale.
//
// One wave owns a tile of 32 pixels (cells), as in the forward kernel (reduc.hip), and does three things:
//   1. recompute the chain: y_l = ELU(W_l y_{l-1}) on v_mfma_f32_32x32x2_f32, layers transposed (channel in register,
//      pixel on lane), each hidden y_l written to the row buffer Y on its way down;
//   2. differentiate the epilogue on the lanes that hold the last layer's outputs: LPG (each cell sums its k x k block
//      of the incoming gradient) <- F.normalize with its 1e-12 clamp <- sin / cos <- the three sigmoids; the final chain
//      has the one sigmoid;
//   3. walk back up: dpre_l = dy_l * ELU'(y_l), ELU' = y + 1 for y < 0, written to the row buffer G, and
//      dy_{l-1} = W_l^T dpre_l.  The D tile of that product is again the B operand of the next one, so the walk is the
//      forward chain mirrored, on fragments the host packed from W_l^T in reverse layer order.
// The weight gradients are not computed here: dW_l = dpre_l^T y_{l-1} is one bts_conv_wgrad_f32 call per layer on column
// slices of G and Y (x for the first layer).
//
// Decisions.
//   LDS        The forward fragments always sit in LDS (<= 114 KB, the 8x8 chain).  The transposed fragments join them
//              when both fit in 160 KB: 4x4 (47 + 44 KB), 2x2 (15 + 12 KB), final (5 + 4 KB).  The 8x8 chain's 108 KB of
//              transposed fragments are read from global memory: every wave reads the same bytes, so they stay in L2.
//   Registers  A layer's y_l is NOT held across the deeper layers: the lane re-reads its own values from the Y row it
//              has just written (same thread, same address: program order).  Live at the widest point are one layer's
//              input (64) and accumulators (64), as in the forward kernel.  hipcc -O3, gfx950: 222 VGPRs for <128,128,8>, 154 for
//              <128,64,4> (128 / 84 for the narrow chains), 0 AGPRs and no scratch in any; 2 waves per SIMD for the 8x8 chain
//              (its LDS allows one 8-wave workgroup per CU anyway).
//   Sums       No atomics.  A cell's k x k gradients are summed by its two lanes over fixed halves of the block in a
//              fixed order and the two partial sums added once; everything else is the MFMA's own fixed order.  Two
//              runs on the same inputs give the same bits in dx, G and Y.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "common.h"
#include "lpg_math.h"
#include "reduc_chain.h"

namespace {

// ---- fragment and column bookkeeping ------------------------------------------------------------------------------
// transposed fragments of layer (k -> m): W^T is [k rows][max(m, 8) columns]
constexpr long layer_t_float4s(int k, int m) { return layer_frag_float4s(k, m < 8 ? 8 : m); }
// ... of the sub-chain that starts with layer (k -> m): the offset of the layer ABOVE it in the reversed buffer
constexpr long chain_t_float4s(int k, int m) {
    long n = 0;
    while (m >= 8) { n += layer_t_float4s(k, m); k = m; m = m / 2; }
    return n + layer_t_float4s(k, m);
}
// hidden widths summed: the columns of Y; G has 4 more (the last layer's 3 or 1 pre-activation gradients, zero-padded)
constexpr int chain_y_cols(int m0) { int n = 0; for (int m = m0; m >= 8; m /= 2) n += m; return n; }

struct Tile {
    long p;              // this lane's pixel (both lane halves hold the same pixel)
    bool live;           // p < npix
    int h;               // lane half
    float* yrow;         // Y + p * YC + 4h
    float* grow;         // G + p * GC + 4h, or NULL
    // epilogue
    const float* gout;   // incoming gradient
    float max_depth;
    int ch, cw;          // cells per column / row (LPG)
    bool want_dx;
};

// d(depth_scaled block)/d(o0, o1, o2) for one cell: both lane halves return the same values
template <int LPGK>
__device__ __forceinline__ void lpg_epilogue_bwd(const Tile& t, const float (&o)[3], float (&d)[3]) {
    const float PI = 3.14159265358979323846f;
    const float s0 = sigmoid1(o[0]), s1 = sigmoid1(o[1]), s2 = sigmoid1(o[2]);
    const float theta = s0 * PI / 3.f, phi = s1 * PI * 2.f, dist = s2 * t.max_depth;      // bts.py:127-129
    const float st = sinf(theta), ct = cosf(theta), sp = sinf(phi), cp = cosf(phi);
    const float m1 = st * cp, m2 = st * sp, m3 = ct;                                      // bts.py:130-132
    const float nrm = sqrtf(m1 * m1 + m2 * m2 + m3 * m3);
    const float nn = fmaxf(nrm, 1e-12f);                                                  // F.normalize, bts.py:251
    const float n1 = m1 / nn, n2 = m2 / nn, n3 = m3 / nn;
    // the cell's K x K block of the incoming gradient: lane half h takes a fixed half of it
    float g1 = 0.f, g2 = 0.f, g3 = 0.f, g4 = 0.f;
    if (t.live) {
        const int cx = (int)(t.p % t.cw);
        const long rowi = t.p / t.cw;
        const int cy = (int)(rowi % t.ch);
        const long b = rowi / t.ch;
        const long W = (long)t.cw * LPGK, H = (long)t.ch * LPGK;
        const float* gc = t.gout + (b * H + (long)cy * LPGK) * W + (long)cx * LPGK;
        if constexpr (LPGK == 8) {                          // half h: columns 4h .. 4h+3 of all eight rows
#pragma unroll
            for (int r = 0; r < 8; ++r) {
                const float4 v = *reinterpret_cast<const float4*>(gc + (long)r * W + 4 * t.h);
                const float g[4] = {v.x, v.y, v.z, v.w};
                lpg_cell_grads<8, 4>(n1, n2, n3, dist, r, 4 * t.h, t.max_depth, g, g1, g2, g3, g4);
            }
        } else if constexpr (LPGK == 4) {                   // half h: rows 2h, 2h+1
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const int r = 2 * t.h + i;
                const float4 v = *reinterpret_cast<const float4*>(gc + (long)r * W);
                const float g[4] = {v.x, v.y, v.z, v.w};
                lpg_cell_grads<4, 4>(n1, n2, n3, dist, r, 0, t.max_depth, g, g1, g2, g3, g4);
            }
        } else {                                            // half h: row h
            static_assert(LPGK == 2, "upratio 8, 4 or 2");
            const float2 v = *reinterpret_cast<const float2*>(gc + (long)t.h * W);
            const float g[2] = {v.x, v.y};
            lpg_cell_grads<2, 2>(n1, n2, n3, dist, t.h, 0, t.max_depth, g, g1, g2, g3, g4);
        }
    }
    g1 += __shfl_xor(g1, 32, 64); g2 += __shfl_xor(g2, 32, 64);       // a + b on one half, b + a on the other: same bits
    g3 += __shfl_xor(g3, 32, 64); g4 += __shfl_xor(g4, 32, 64);
    // F.normalize: n = m / max(|m|, eps); the norm takes a gradient only where the clamp is not active
    float q1, q2, q3;
    if (nrm > 1e-12f) {
        const float dot = n1 * g1 + n2 * g2 + n3 * g3;
        q1 = (g1 - n1 * dot) / nn; q2 = (g2 - n2 * dot) / nn; q3 = (g3 - n3 * dot) / nn;
    } else {
        q1 = g1 / nn; q2 = g2 / nn; q3 = g3 / nn;
    }
    const float dtheta = q1 * ct * cp + q2 * ct * sp - q3 * st;
    const float dphi = st * (q2 * cp - q1 * sp);
    d[0] = dtheta * (PI / 3.f) * s0 * (1.f - s0);
    d[1] = dphi * (PI * 2.f) * s1 * (1.f - s1);
    d[2] = g4 * t.max_depth * s2 * (1.f - s2);             // n4 = sigmoid * max_depth
}

// Forward down, backward on the way back up.  x: the layer's input (K real channels); dxo <- gradient w.r.t. x.
// COL: first Y / G column of this layer's output.  wf: this layer's forward fragments; wt: the transposed buffer's base.
template <int K, int M, int NX, bool FINAL, int LPGK, int COL>
__device__ __forceinline__ void chain_bwd(const float4* __restrict__ wf, const float4* __restrict__ wt, int lane,
                                          const float (&x)[NX], const Tile& t, float (&dxo)[NX]) {
    constexpr int MTT = (K + 31) / 32;                    // row tiles of W^T
    if constexpr (M < 8) {                                // plane_params (3 outs) or final (1 out)
        float o[3];
        {
            f32x16 acc[1];
            dense_layer<K, 1, NX>(wf, lane, x, acc);
            o[0] = acc[0][0]; o[1] = acc[0][1]; o[2] = acc[0][2];
        }
        float d[3] = {0.f, 0.f, 0.f};
        if constexpr (FINAL) {
            const float s = sigmoid1(o[0]);                                               // bts.py:108-110
            d[0] = (t.live ? t.gout[t.p] : 0.f) * s * (1.f - s);
        } else {
            // rows 0..2 of the D tile live on lane half 0 only; half 1 works on the same cell and needs the same values
#pragma unroll
            for (int i = 0; i < 3; ++i) o[i] = __shfl(o[i], lane & 31, 64);
            lpg_epilogue_bwd<LPGK>(t, o, d);
        }
        // channels 0..3 of the (padded) last layer sit on lane half 0, channels 4..7 (zeros) on half 1
        const bool lo = t.h == 0;
        const float dp[4] = {lo ? d[0] : 0.f, lo ? d[1] : 0.f, lo ? d[2] : 0.f, 0.f};
        if (t.grow != nullptr && t.live && lo)
            *reinterpret_cast<float4*>(t.grow + COL) = make_float4(dp[0], dp[1], dp[2], 0.f);
        f32x16 acc[MTT];
        dense_layer<8, MTT, 4>(wt, lane, dp, acc);
#pragma unroll
        for (int i = 0; i < NX; ++i) dxo[i] = acc[i / 16][i % 16];
    } else {
        constexpr int MT = (M + 31) / 32;
        constexpr int NY = (M / 2 < 4) ? 4 : M / 2;
        float dy[NY];
        {
            float y[NY];
            {
                f32x16 acc[MT];
                dense_layer<K, MT, NX>(wf, lane, x, acc);
#pragma unroll
                for (int i = 0; i < NY; ++i) y[i] = elu1(acc[i / 16][i % 16]);          // conv + ELU, bts.py:116-119
            }
            if (t.live) {
#pragma unroll
                for (int g = 0; g < M / 8; ++g)          // lane (j,h): channels 8g + 4h .. +3
                    *reinterpret_cast<float4*>(t.yrow + COL + 8 * g) = make_float4(y[4 * g], y[4 * g + 1], y[4 * g + 2], y[4 * g + 3]);
            }
            chain_bwd<M, M / 2, NY, FINAL, LPGK, COL + M>(wf + layer_frag_float4s(M, K), wt, lane, y, t, dy);
        }
        float dp[NY];
#pragma unroll
        for (int g = 0; g < M / 8; ++g) {
            const float4 v = t.live ? *reinterpret_cast<const float4*>(t.yrow + COL + 8 * g) : make_float4(0.f, 0.f, 0.f, 0.f);
            dp[4 * g + 0] = dy[4 * g + 0] * (v.x < 0.f ? v.x + 1.f : 1.f);               // ELU'(pre) from y = ELU(pre)
            dp[4 * g + 1] = dy[4 * g + 1] * (v.y < 0.f ? v.y + 1.f : 1.f);
            dp[4 * g + 2] = dy[4 * g + 2] * (v.z < 0.f ? v.z + 1.f : 1.f);
            dp[4 * g + 3] = dy[4 * g + 3] * (v.w < 0.f ? v.w + 1.f : 1.f);
            if (t.grow != nullptr && t.live)
                *reinterpret_cast<float4*>(t.grow + COL + 8 * g) = make_float4(dp[4 * g], dp[4 * g + 1], dp[4 * g + 2], dp[4 * g + 3]);
        }
        if (COL == 0 && !t.want_dx) return;              // first layer and nobody wants dx
        f32x16 acc[MTT];
        dense_layer<M, MTT, NY>(wt + chain_t_float4s(M, M / 2), lane, dp, acc);
#pragma unroll
        for (int i = 0; i < NX; ++i) dxo[i] = acc[i / 16][i % 16];
    }
}

template <int C0, int M0>
struct ChainSizes {
    static constexpr long NWF = chain_frag_float4s_of(C0, M0);       // forward fragments, float4s
    static constexpr long NWT = chain_t_float4s(C0, M0);             // transposed fragments
    static constexpr int YC = chain_y_cols(M0), GC = YC + 4;
    static constexpr bool WT_LDS = (NWF + NWT) * 16 <= 160 * 1024;
    static constexpr size_t LDS = (size_t)(WT_LDS ? NWF + NWT : NWF) * 16;
    static constexpr int PER_CU = LDS > 80 * 1024 ? 1 : 2;
    static constexpr long MAX_BLOCKS = 256L * PER_CU;
};

template <int C0, int M0, bool FINAL, int LPGK>
__global__ __launch_bounds__(512, 2) void reduc_bwd_kernel(const float* __restrict__ x, long x_pix_stride, long npix,
                                                           const float4* __restrict__ w_frag, const float4* __restrict__ wt_frag,
                                                           float max_depth, int ch, int cw, const float* __restrict__ gout,
                                                           float* __restrict__ dx, long dx_pix_stride, float* G, float* Y) {
    using S = ChainSizes<C0, M0>;
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    float4* wl = reinterpret_cast<float4*>(smem_raw);
    for (long i = threadIdx.x; i < S::NWF; i += blockDim.x) wl[i] = w_frag[i];
    if constexpr (S::WT_LDS)
        for (long i = threadIdx.x; i < S::NWT; i += blockDim.x) wl[S::NWF + i] = wt_frag[i];
    __syncthreads();

    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int waves_per_block = blockDim.x >> 6;
    const int j = lane & 31, h = lane >> 5;
    const long ntiles = (npix + 31) / 32;
    for (long tile = (long)blockIdx.x * waves_per_block + wave; tile < ntiles;
         tile += (long)gridDim.x * waves_per_block) {
        Tile t;
        t.p = tile * 32 + j;
        t.live = t.p < npix;
        t.h = h;
        const long pr = t.live ? t.p : 0;
        t.yrow = Y + pr * S::YC + 4 * h;
        t.grow = G != nullptr ? G + pr * S::GC + 4 * h : nullptr;
        t.gout = gout;
        t.max_depth = max_depth;
        t.ch = ch; t.cw = cw;
        t.want_dx = dx != nullptr;
        float xr[C0 / 2], dxr[C0 / 2];
        const float* xp = x + pr * x_pix_stride + 4 * h;
#pragma unroll
        for (int q = 0; q < C0 / 8; ++q) {         // lane (j,h): channels 4*(2q+h) .. +3
            float4 v = t.live ? *reinterpret_cast<const float4*>(xp + 8 * q) : make_float4(0.f, 0.f, 0.f, 0.f);
            xr[4 * q + 0] = v.x; xr[4 * q + 1] = v.y; xr[4 * q + 2] = v.z; xr[4 * q + 3] = v.w;
        }
        if constexpr (S::WT_LDS) chain_bwd<C0, M0, C0 / 2, FINAL, LPGK, 0>(wl, wl + S::NWF, lane, xr, t, dxr);
        else {
            // the fragments are the same for every tile: without this the compiler hoists all 108 KB / 8 waves of loads
            // out of the tile loop and spills them
            const float4* wt = wt_frag;
            asm volatile("" : "+s"(wt));
            chain_bwd<C0, M0, C0 / 2, FINAL, LPGK, 0>(wl, wt, lane, xr, t, dxr);
        }
        if (dx != nullptr && t.live) {
            float* dp = dx + t.p * dx_pix_stride + 4 * h;
#pragma unroll
            for (int q = 0; q < C0 / 8; ++q)
                *reinterpret_cast<float4*>(dp + 8 * q) = make_float4(dxr[4 * q], dxr[4 * q + 1], dxr[4 * q + 2], dxr[4 * q + 3]);
        }
    }
}

template <int C0, int M0, bool FINAL, int LPGK>
int launch_reduc_bwd(const float* x, long stride, long npix, int ch, int cw, const float* w_frag, long w_frag_floats,
                     const float* wt_frag, long wt_frag_floats, float max_depth, const float* gout, float* dx,
                     long dx_stride, float* G, float* Y, hipStream_t s) {
    using S = ChainSizes<C0, M0>;
    if (w_frag_floats != S::NWF * 4 || wt_frag_floats != S::NWT * 4) return BTS_ERR_INVALID;
    const long ntiles = (npix + 31) / 32;
    long blocks = (ntiles + 7) / 8;
    if (blocks > S::MAX_BLOCKS) blocks = S::MAX_BLOCKS;
    if (const int rc = bts_launch<reduc_bwd_kernel<C0, M0, FINAL, LPGK>>(
            dim3((unsigned)blocks), dim3(512), S::LDS, s, x, stride, npix, reinterpret_cast<const float4*>(w_frag),
            reinterpret_cast<const float4*>(wt_frag), max_depth, ch, cw, gout, dx, dx_stride, G, Y); rc != 0) return rc;
    return (int)hipGetLastError();
}

}  // namespace

extern "C" long bts_reduc_bwd_max_waves(int c_in, int c_first_out, int upratio) {
    if (c_in == 128 && c_first_out == 128 && upratio == 8) return ChainSizes<128, 128>::MAX_BLOCKS * 8;
    if (c_in == 128 && c_first_out == 64 && upratio == 4) return ChainSizes<128, 64>::MAX_BLOCKS * 8;
    if (c_in == 64 && c_first_out == 32 && upratio == 2) return ChainSizes<64, 32>::MAX_BLOCKS * 8;
    if (c_in == 32 && c_first_out == 16 && upratio == 0) return ChainSizes<32, 16>::MAX_BLOCKS * 8;
    return BTS_ERR_UNSUPPORTED;
}

extern "C" int bts_reduc_bwd_f32(const float* x, long x_pix_stride, int B, int h, int w, int c_in, int c_first_out,
                                 const float* w_frag, long w_frag_floats, const float* wt_frag, long wt_frag_floats,
                                 float max_depth, int upratio, const float* grad_out, float* dx, long dx_pix_stride,
                                 float* G, float* Y, bts_stream_t stream) {
    if (!x || !w_frag || !wt_frag || !grad_out || !Y || B <= 0 || h <= 0 || w <= 0) return BTS_ERR_INVALID;
    if ((x_pix_stride & 3) || ((uintptr_t)x & 15) || ((uintptr_t)w_frag & 15) || ((uintptr_t)wt_frag & 15) ||
        ((uintptr_t)grad_out & 15) || ((uintptr_t)G & 15) || ((uintptr_t)Y & 15) || ((uintptr_t)dx & 15))
        return BTS_ERR_INVALID;
    if (x_pix_stride < c_in || !(max_depth > 0.f)) return BTS_ERR_INVALID;
    if (dx != nullptr && ((dx_pix_stride & 3) || dx_pix_stride < c_in)) return BTS_ERR_INVALID;
    const long npix = (long)B * h * w;
    if ((double)npix * (upratio > 0 ? upratio * upratio : 1) >= 9.0e18) return BTS_ERR_UNSUPPORTED;
    hipStream_t s = (hipStream_t)stream;
#define BTS_REDUC_BWD(C0, M0, FIN, KK)                                                                                   \
    return launch_reduc_bwd<C0, M0, FIN, KK>(x, x_pix_stride, npix, h, w, w_frag, w_frag_floats, wt_frag, wt_frag_floats, \
                                             max_depth, grad_out, dx, dx_pix_stride, G, Y, s)
    if (c_in == 128 && c_first_out == 128 && upratio == 8) BTS_REDUC_BWD(128, 128, false, 8);
    if (c_in == 128 && c_first_out == 64 && upratio == 4) BTS_REDUC_BWD(128, 64, false, 4);
    if (c_in == 64 && c_first_out == 32 && upratio == 2) BTS_REDUC_BWD(64, 32, false, 2);
    if (c_in == 32 && c_first_out == 16 && upratio == 0) BTS_REDUC_BWD(32, 16, true, 0);
#undef BTS_REDUC_BWD
    return BTS_ERR_UNSUPPORTED;
}
