// Weight packs of the training step and of the Winograd forward kernel on gfx950 (bts_pack_weights_*, bts_pack_wino_*,
// bts_upconv_train_pack_*; include/bts_hip.h).  Every step the optimiser rewrites the OIHW parameters, and the kernels
// that consume them read other layouts; each pack here is ONE launch from a device table (one record per weight with a
// `first_block` prefix sum, found by bts_table_find) or, for the Winograd form, one launch per weight.
#include "common.h"
#include <stdint.h>

// ---------------------------------------------------------------------------------------------------------------
// Batched weight packing for the training step: both the forward kernel ([c_out_pad][k_pad], K = tap*c_in_ld + c) and
// the input-gradient pass (the same layout of the flipped, transposed kernel) need the parameters re-laid.  One launch
// re-packs every registered weight from a device table.
namespace {

struct PackEntry {          // 14 x int64, filled by the host (bts_amd/train.py)
    const float* src;       // OIHW parameter
    float* dst;             // [rows_pad][k_pad]
    long rows, inner;       // packed rows (c_out, or c_in for the transposed layout) and real inner channels
    long k, c_in_ld, rows_pad, k_pad;
    long s_row, s_c;        // element strides in src for the packed row / inner channel
    long flip;              // 0: taps as stored, 1: spatially flipped (input gradient)
    long first_block;       // prefix sum of blocks over the table
    long cg, gmode;         // grouped weight [C][cg][k][k] packed block-diagonally into a bundle (src points at the
                            // bundle's first output channel): cg = channels per group; gmode 1 = forward (row = output
                            // channel, inner = bundle-local input channel), 2 = input gradient (row = bundle-local input
                            // channel, inner = output channel); entries outside a row's own group are zero.  0 = dense.
                            // gmode 3 / 4: the whole [c][cg][3][3] weight (src) in the 144 c-float layout of
                            // bts_conv_grouped_fwd_f32 (rows_pad * k_pad = 144 c; only cg and the two pointers are read):
                            // 3 = the forward weight, 4 = the flipped, group-transposed weight of the input gradient
};
static_assert(sizeof(PackEntry) == 14 * 8, "train.py builds these rows as 14 int64 columns");

constexpr int PACK_PER_BLOCK = 256 * 4 * 4;

__global__ __launch_bounds__(256) void pack_weights_kernel(const PackEntry* __restrict__ table, int n) {
    const PackEntry e = table[bts_table_find(table, n, &PackEntry::first_block)];
    const long total = e.rows_pad * e.k_pad;
    const long base = ((long)blockIdx.x - e.first_block) * PACK_PER_BLOCK;
    const long kk2 = e.k * e.k;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const long i0 = base + ((long)u * 256 + threadIdx.x) * 4;
        if (i0 >= total) continue;
        const long row = i0 / e.k_pad, col0 = i0 - row * e.k_pad;
        f32x4 v = (f32x4)(0.f);
        if (e.gmode >= 3) {                                              // native grouped layout: four lanes of one (s, tap, k)
            const long lane0 = i0 & 63, kb = (i0 >> 6) & 15, tap = (i0 >> 10) % 9, s = i0 / 9216;
            const long ci = 64 * s + 16 * (lane0 >> 4) + kb;            // input channel of the product; lanes = output channels
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const long n = 64 * s + lane0 + j;
                if (n / e.cg == ci / e.cg)
                    v[j] = e.gmode == 3 ? e.src[(n * e.cg + ci % e.cg) * 9 + tap] : e.src[(ci * e.cg + n % e.cg) * 9 + 8 - tap];
            }
        } else if (row < e.rows) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const long col = col0 + j;
                const long tap = col / e.c_in_ld, c = col - tap * e.c_in_ld;
                if (tap < kk2 && c < e.inner) {
                    const long t = e.flip ? kk2 - 1 - tap : tap;
                    if (e.gmode == 0) {
                        v[j] = e.src[row * e.s_row + c * e.s_c + t];
                    } else if (row / e.cg == c / e.cg) {                 // same group: the only non-zero block
                        const long g0 = (row / e.cg) * e.cg;
                        const long r = e.gmode == 2 ? row - g0 : row, cc = e.gmode == 1 ? c - g0 : c;
                        v[j] = e.src[r * e.s_row + cc * e.s_c + t];
                    }
                }
            }
        }
        *reinterpret_cast<f32x4*>(e.dst + i0) = v;
    }
}

// Winograd F(2x2,3x3) form of a packed 3x3 weight, in conv_wino_kernel's B-fragment order (include/bts_hip.h,
// bts_pack_wino_f32).  One thread = one output f32x4 (four consecutive k of one (xi, n)): U = G g G^T in fp64, rounded once.
__global__ __launch_bounds__(256) void pack_wino_kernel(const float* __restrict__ w, long k_pad, int c_in_ld, int c_main, int n_ct,
                                                        int mf16, float* __restrict__ out, long total4) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total4) return;
    const int lane = (int)(i & 63);
    long r = i >> 6;
    const int gpc = mf16 ? 2 : 4;
    const int g = (int)(r % gpc); r /= gpc;
    const int ct = (int)(r % n_ct); r /= n_ct;
    const int nchunks = c_main / 32;
    const int chunk = (int)(r % nchunks);
    const int xi = (int)(r / nchunks);
    const int n = mf16 ? 16 * ct + (lane & 15) : 32 * ct + (lane & 31);
    const int k0 = mf16 ? 32 * chunk + 16 * g + 4 * (lane >> 4) : 32 * chunk + 8 * g + 4 * (lane >> 5);
    const int wi = xi >> 2, wj = xi & 3;
    // rows of G: {1,0,0}, {.5,.5,.5}, {.5,-.5,.5}, {0,0,1}
    const double Gi[3] = {wi == 0 ? 1.0 : (wi == 3 ? 0.0 : 0.5), wi == 1 ? 0.5 : (wi == 2 ? -0.5 : 0.0), wi == 3 ? 1.0 : (wi == 0 ? 0.0 : 0.5)};
    const double Gj[3] = {wj == 0 ? 1.0 : (wj == 3 ? 0.0 : 0.5), wj == 1 ? 0.5 : (wj == 2 ? -0.5 : 0.0), wj == 3 ? 1.0 : (wj == 0 ? 0.0 : 0.5)};
    f32x4 o;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const float* src = w + (long)n * k_pad + (k0 + q);
        double acc = 0.0;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            double row = 0.0;
#pragma unroll
            for (int b = 0; b < 3; ++b) row += (double)src[(long)(3 * a + b) * c_in_ld] * Gj[b];
            acc += Gi[a] * row;
        }
        o[q] = (float)acc;
    }
    *reinterpret_cast<f32x4*>(out + 4 * i) = o;
}

}  // namespace

extern "C" long bts_pack_wino_floats(int c_out_pad, int c_in_ld, int n_tail, int c_out16) {
    const int c_main = c_in_ld - (n_tail > 0 ? 4 : 0);
    if (c_out_pad <= 0 || (c_out_pad & 31) || c_main <= 0 || (c_main & 31) || c_out16 < 0 || (c_out16 & 15) || c_out16 > c_out_pad) return -1;
    return 16L * c_main * (c_out16 > 0 ? c_out16 : c_out_pad);
}

extern "C" int bts_pack_wino_f32(const float* w_packed, int c_out_pad, long k_pad, int c_in_ld, int n_tail, int c_out16,
                                 float* out, bts_stream_t stream) {
    const long total = bts_pack_wino_floats(c_out_pad, c_in_ld, n_tail, c_out16);
    if (!w_packed || !out || total <= 0 || k_pad < 9L * c_in_ld || ((uintptr_t)out & 15)) return BTS_ERR_INVALID;
    const int c_main = c_in_ld - (n_tail > 0 ? 4 : 0);
    const int mf16 = c_out16 > 0 ? 1 : 0;
    const int n_ct = mf16 ? c_out16 / 16 : c_out_pad / 32;
    const long total4 = total / 4, blocks = (total4 + 255) / 256;
    if (blocks > 2147483647L) return BTS_ERR_INVALID;
    hipLaunchKernelGGL(pack_wino_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, w_packed, k_pad, c_in_ld, c_main,
                       n_ct, mf16, out, total4);
    return (int)hipGetLastError();
}

extern "C" long bts_pack_weights_blocks(long rows_pad, long k_pad) {
    return (rows_pad * k_pad + PACK_PER_BLOCK - 1) / PACK_PER_BLOCK;
}

extern "C" int bts_pack_weights_f32(const void* table, int n_entries, long total_blocks, bts_stream_t stream) {
    if (!table || n_entries <= 0 || total_blocks <= 0 || total_blocks > 2147483647L) return BTS_ERR_INVALID;
    hipLaunchKernelGGL(pack_weights_kernel, dim3((unsigned)total_blocks), dim3(256), 0, (hipStream_t)stream,
                       (const PackEntry*)table, n_entries);
    return (int)hipGetLastError();
}

// ---------------------------------------------------------------------------------------------------------------
// Per-step packs of the sub-pixel upconv weights (bts_upconv_train_pack_f32): the forward pack of the four 2x2 class
// filters and the input-gradient pack of the 4x4 / stride-2 kernel, both from the OIHW 3x3 parameter.
namespace {

struct UpconvPackEntry {    // 12 x int64, filled by the host (ops.upconv_train_pack)
    const float* src;       // OIHW [c_out][c_in][3][3]
    float* fwd;             // [4][c_out_pad][k_pad_f], k = (2*ty+tx)*c_in_ld + c   (ops.pack_upconv_subpixel)
    float* dgrad;           // [c_in_pad][k_pad_d], k = (4*r+s)*c_out_ld + n         (bts_upconv_dgrad_f32)
    long c_out, c_in, c_in_ld, c_out_ld, c_out_pad, k_pad_f, c_in_pad, k_pad_d;
    long first_block;       // prefix sum of blocks over the table
};
static_assert(sizeof(UpconvPackEntry) == 12 * 8, "ops.upconv_train_pack builds these rows as 12 int64 columns");

// g_(py,px)[ty][tx] of one (output, input) channel pair: the 3x3 taps the class tap covers, added in fp32 in the order
// ky outer, kx inner (pack_upconv_subpixel's order); w9 = the pair's nine taps.  Additions only: nothing to contract.
__device__ __forceinline__ float subpix_class_tap(const float* __restrict__ w9, int py, int ty, int px, int tx) {
    const int ky0 = ty == 0 ? 0 : (py == 0 ? 1 : 2), nky = py != ty ? 2 : 1;     // (0,0):{0} (0,1):{1,2} (1,0):{0,1} (1,1):{2}
    const int kx0 = tx == 0 ? 0 : (px == 0 ? 1 : 2), nkx = px != tx ? 2 : 1;
    float acc = w9[ky0 * 3 + kx0];
    if (nkx == 2) acc = __fadd_rn(acc, w9[ky0 * 3 + kx0 + 1]);
    if (nky == 2) {
        acc = __fadd_rn(acc, w9[(ky0 + 1) * 3 + kx0]);
        if (nkx == 2) acc = __fadd_rn(acc, w9[(ky0 + 1) * 3 + kx0 + 1]);
    }
    return acc;
}

__global__ __launch_bounds__(256) void upconv_train_pack_kernel(const UpconvPackEntry* __restrict__ table, int n) {
    const UpconvPackEntry e = table[bts_table_find(table, n, &UpconvPackEntry::first_block)];
    const long n_fwd = 4 * e.c_out_pad * e.k_pad_f, total = n_fwd + e.c_in_pad * e.k_pad_d;     // both multiples of 4
    const long base = ((long)blockIdx.x - e.first_block) * PACK_PER_BLOCK;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const long i0 = base + ((long)u * 256 + threadIdx.x) * 4;
        if (i0 >= total) continue;
        f32x4 v = (f32x4)(0.f);
        if (i0 < n_fwd) {
            const long cls = i0 / (e.c_out_pad * e.k_pad_f), r0 = i0 - cls * e.c_out_pad * e.k_pad_f;
            const long row = r0 / e.k_pad_f, col0 = r0 - row * e.k_pad_f;
            if (row < e.c_out) {
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const long col = col0 + j, tap = col / e.c_in_ld, c = col - tap * e.c_in_ld;
                    if (tap < 4 && c < e.c_in)
                        v[j] = subpix_class_tap(e.src + (row * e.c_in + c) * 9, (int)(cls >> 1), (int)(tap >> 1), (int)(cls & 1), (int)(tap & 1));
                }
            }
            *reinterpret_cast<f32x4*>(e.fwd + i0) = v;
        } else {
            const long i1 = i0 - n_fwd;
            const long row = i1 / e.k_pad_d, col0 = i1 - row * e.k_pad_d;      // row = input channel
            if (row < e.c_in) {
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const long col = col0 + j, rs = col / e.c_out_ld, nn = col - rs * e.c_out_ld;
                    if (rs < 16 && nn < e.c_out) {
                        const int r = (int)(rs >> 2), sx = (int)(rs & 3);      // K[r][s]: 3 - r = py + 2 ty, 3 - s = px + 2 tx
                        v[j] = subpix_class_tap(e.src + (nn * e.c_in + row) * 9, (3 - r) & 1, (3 - r) >> 1, (3 - sx) & 1, (3 - sx) >> 1);
                    }
                }
            }
            *reinterpret_cast<f32x4*>(e.dgrad + i1) = v;
        }
    }
}

}  // namespace

extern "C" long bts_upconv_train_pack_blocks(long c_out_pad, long k_pad_f, long c_in_pad, long k_pad_d) {
    return (4 * c_out_pad * k_pad_f + c_in_pad * k_pad_d + PACK_PER_BLOCK - 1) / PACK_PER_BLOCK;
}

extern "C" int bts_upconv_train_pack_f32(const void* table, int n_entries, long total_blocks, bts_stream_t stream) {
    if (!table || ((uintptr_t)table & 7) || n_entries <= 0 || total_blocks <= 0 || total_blocks > 2147483647L) return BTS_ERR_INVALID;
    hipLaunchKernelGGL(upconv_train_pack_kernel, dim3((unsigned)total_blocks), dim3(256), 0, (hipStream_t)stream,
                       (const UpconvPackEntry*)table, n_entries);
    return (int)hipGetLastError();
}
