// AdamW for the training step as ONE launch over every parameter of the model (reference: torch.optim.AdamW with two
// parameter groups, pytorch/bts_main.py:354-356, stepped at bts_main.py:606), which also re-lays the updated convolution
// weights out as the forward and input-gradient kernels read them (bts_pack_weights_f32's layouts) while the new values
// are still on the chip.
//
// Launch shape (the idiom of pack_weights_kernel / conv_wgrad_batch_kernel): a device table holds one record per parameter
// with a `first_block` prefix sum; a workgroup finds its record with bts_table_find (common.h) and derives its chunk or
// tile from its rank inside the record.  Hyper-parameters come BY VALUE, up to 8 records, every table record names one.
// Nothing is read from the host during the launch; no allocation, no synchronisation; hipGraph-capturable.
//
// Update (torch.optim.AdamW, amsgrad=False, maximize=False), fp32, in this order:
//     p <- p * (1 - lr*wd)
//     m <- m + (g - m) * (1 - beta1)                                   fmaf(g - m, 1 - beta1, m)
//     v <- beta2 * v + (1 - beta2) * g * g                             fmaf((1 - beta2) * g, g, beta2 * v)
//     p <- p - step_size * m / (sqrt(v) * inv_sqrt_bc2 + eps)          (step_size * m) / (...), then the subtraction
// with step_size = lr / (1 - beta1^t), inv_sqrt_bc2 = 1 / sqrt(1 - beta2^t), and the three factors (1 - lr*wd),
// (1 - beta1), (1 - beta2) all computed in double on the host and rounded to fp32 once.  The two fused multiply-adds are
// written out (one rounding fewer each; they are also what ATen's CPU lerp_ / addcmul_ round like); everything else
// rounds on its own -- the file is compiled with -ffp-contract=off -- and sqrtf and '/' are the correctly rounded IEEE
// forms, no fast intrinsics.  Elementwise: the result does not depend on the launch shape and is bit-reproducible.
//
// FLAT records (anything without packs): one block covers a fixed span of AW_SPAN elements; 16 bytes per lane where p, g,
// m, v share their offset to a 16-byte line, with a scalar head and tail per block (as loss.hip splits its pixels), one
// element per lane otherwise.
//
// TILE records (dense OIHW weight, ksize 1 or 3, one or two pack destinations): a workgroup owns T output channels x T
// input channels x all k*k taps (T = 32 for 3x3: 36 KB of LDS, four workgroups per CU; T = 64 for 1x1: 16 KB).  For one
// output channel the tile's part of the weight is ONE contiguous run of T*k*k floats (1152 B / 256 B), so p, g, m, v are
// read and p, m, v written back a whole run per wave instruction.  The new p is staged in LDS as lds[o][c*kk + t] with a
// row stride of T*kk + 1 floats -- PADDED, not swizzled: the run write is consecutive addresses; the forward-layout read
// (lanes along c) has stride kk = 9 or 1, the input-gradient read (lanes along o) has stride T*kk + 1 = 289 or 65, all odd,
// so the 32 lanes of a ds_read_b32 group fall on 32 different banks.  The packs are written in runs of T floats
// (128 B / 256 B): dst[row][tap*c_in_ld + c], forward row = c_out, input gradient row = c_in with the taps flipped and
// c_out as the inner index.  Only real elements of a destination are written: its padding is zero from the weight's
// first ordinary pack and stays untouched.
//
// `skip`: optional device scalar; non-zero or NaN -> every workgroup returns before its first access (a non-finite loss
// skips the step without the host ever looking at it).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include "common.h"

namespace {

constexpr int AW_THREADS = 256;
constexpr int AW_SPAN = 4096;                       // floats of a flat record per block: 4 x 16 B per lane
constexpr int AW_T3 = 32, AW_T1 = 64;               // channel tile (both ways) of a 3x3 / 1x1 tile record
constexpr int AW_LDS_FLOATS = AW_T3 * (AW_T3 * 9 + 1);   // 9248 floats = 36992 B (the 1x1 tile needs 64 * 65 = 4160)
constexpr int AW_MAX_HYPER = 8;

struct AdamwHyperDev {       // 12 floats
    float lr, beta1, beta2, eps, weight_decay, step_size, inv_sqrt_bc2;
    float decay, omb1, omb2;                        // 1 - lr*wd, 1 - beta1, 1 - beta2
    float pad0, pad1;
};
struct AdamwHyperTable { AdamwHyperDev h[AW_MAX_HYPER]; };

struct AdamwRec {            // 136 bytes, 8-byte aligned
    float* p; const float* g; float* m; float* v;
    float* dst[2];           // pack destinations (tile records), NULL = none
    long k_pad[2];
    long numel, first_block, n_blocks;
    int ld[2];               // c_in_ld of each pack
    int mode[2];             // 0 = forward layout, 1 = input-gradient layout
    int kind;                // 0 = flat, 1 = tile
    int hyper;
    int c_out, c_in, ksize, tiles_c;
    int head, vec;           // flat: floats up to p's next 16-byte line; 1 = g, m, v share that offset
};
static_assert(sizeof(AdamwRec) == 136, "AdamwRec layout");

__device__ __forceinline__ void adamw_update(const AdamwHyperDev& h, float& p, float g, float& m, float& v) {
    p = p * h.decay;
    m = fmaf(g - m, h.omb1, m);
    v = fmaf(h.omb2 * g, g, h.beta2 * v);
    p = p - (h.step_size * m) / (sqrtf(v) * h.inv_sqrt_bc2 + h.eps);
}

__device__ __forceinline__ void flat_block(const AdamwRec& e, const AdamwHyperDev& h, long rank) {
    const long s = rank * AW_SPAN;
    const long left = e.numel - s;
    const int len = left < AW_SPAN ? (int)left : AW_SPAN;
    float* __restrict__ p = e.p + s;
    const float* __restrict__ g = e.g + s;
    float* __restrict__ m = e.m + s;
    float* __restrict__ v = e.v + s;
    // AW_SPAN * 4 is a multiple of 16: every block of the record sees the same offset to a 16-byte line
    int head = 0, nv = 0;
    if (e.vec && len >= e.head + 4) { head = e.head; nv = (len - head) >> 2; }
    float4* __restrict__ p4 = reinterpret_cast<float4*>(p + head);
    const float4* __restrict__ g4 = reinterpret_cast<const float4*>(g + head);
    float4* __restrict__ m4 = reinterpret_cast<float4*>(m + head);
    float4* __restrict__ v4 = reinterpret_cast<float4*>(v + head);
#pragma unroll
    for (int u = 0; u < AW_SPAN / 4 / AW_THREADS; ++u) {
        const int i = u * AW_THREADS + (int)threadIdx.x;
        if (i < nv) {
            float4 pp = p4[i], mm = m4[i], vv = v4[i];
            const float4 gg = g4[i];
            adamw_update(h, pp.x, gg.x, mm.x, vv.x);
            adamw_update(h, pp.y, gg.y, mm.y, vv.y);
            adamw_update(h, pp.z, gg.z, mm.z, vv.z);
            adamw_update(h, pp.w, gg.w, mm.w, vv.w);
            p4[i] = pp; m4[i] = mm; v4[i] = vv;
        }
    }
    // the head and the tail -- or, without a shared alignment, the whole span -- one element per lane
    const int nscalar = len - 4 * nv;
    for (int j = (int)threadIdx.x; j < nscalar; j += AW_THREADS) {
        const int i = j < head ? j : j + 4 * nv;
        float pp = p[i], mm = m[i], vv = v[i];
        adamw_update(h, pp, g[i], mm, vv);
        p[i] = pp; m[i] = mm; v[i] = vv;
    }
}

template <int KK, int T>
__device__ __forceinline__ void tile_block(const AdamwRec& e, const AdamwHyperDev& h, long rank, float* lds) {
    constexpr int SO = T * KK + 1;                  // LDS row stride (floats): odd, see the header
    static_assert(T * SO <= AW_LDS_FLOATS, "tile does not fit the LDS buffer");
    const int to = (int)(rank / e.tiles_c), tc = (int)(rank - (long)to * e.tiles_c);
    const int o0 = to * T, c0 = tc * T;
    const int no = e.c_out - o0 < T ? e.c_out - o0 : T;
    const int nc = e.c_in - c0 < T ? e.c_in - c0 : T;
    const int run = nc * KK;                        // contiguous floats of one output channel inside the tile
    const long row_stride = (long)e.c_in * KK;
    const int wave = (int)threadIdx.x >> 6, lane = (int)threadIdx.x & 63;
#pragma unroll 2
    for (int o = wave; o < no; o += AW_THREADS / 64) {
        const long base = (long)(o0 + o) * row_stride + (long)c0 * KK;
        float* __restrict__ p = e.p + base;
        const float* __restrict__ g = e.g + base;
        float* __restrict__ m = e.m + base;
        float* __restrict__ v = e.v + base;
#pragma unroll
        for (int u = 0; u < (T * KK + 63) / 64; ++u) {
            const int j = u * 64 + lane;
            if (j < run) {
                float pp = p[j], mm = m[j], vv = v[j];
                adamw_update(h, pp, g[j], mm, vv);
                p[j] = pp; m[j] = mm; v[j] = vv;
                lds[o * SO + j] = pp;
            }
        }
    }
    __syncthreads();
    constexpr int NG = AW_THREADS / T;              // lane groups of T lanes, each writes one run of T floats at a time
    const int gl = (int)threadIdx.x % T, gi = (int)threadIdx.x / T;
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        float* __restrict__ dst = e.dst[k];
        if (dst == nullptr) continue;
        const long kp = e.k_pad[k];
        const long ld = e.ld[k];
        if (e.mode[k] == 0) {                       // forward: dst[c_out][tap*ld + c_in], lanes along c_in
            if (gl < nc) {
                for (int q = gi; q < no * KK; q += NG) {
                    const int o = q / KK, t = q - o * KK;
                    dst[(long)(o0 + o) * kp + t * ld + (c0 + gl)] = lds[o * SO + gl * KK + t];
                }
            }
        } else {                                    // input gradient: dst[c_in][(kk-1-tap)*ld + c_out], lanes along c_out
            if (gl < no) {
                for (int q = gi; q < nc * KK; q += NG) {
                    const int c = q / KK, t = q - c * KK;
                    dst[(long)(c0 + c) * kp + (KK - 1 - t) * ld + (o0 + gl)] = lds[gl * SO + c * KK + t];
                }
            }
        }
    }
}

__global__ __launch_bounds__(AW_THREADS) void adamw_step_kernel(const AdamwRec* __restrict__ table, int n,
                                                                const AdamwHyperTable hy, const float* __restrict__ skip) {
    __shared__ float lds[AW_LDS_FLOATS];
    if (skip != nullptr) {
        const float s = *skip;
        if (!(s == 0.f)) return;                    // non-zero or NaN: leave every byte untouched
    }
    const AdamwRec e = table[bts_table_find(table, n, &AdamwRec::first_block)];
    const long rank = (long)blockIdx.x - e.first_block;
    if (rank < 0 || rank >= e.n_blocks) return;     // a grid larger than the plan's: nothing to do (uniform per block)
    const AdamwHyperDev h = hy.h[e.hyper & (AW_MAX_HYPER - 1)];
    if (e.kind == 0) flat_block(e, h, rank);
    else if (e.ksize == 3) tile_block<9, AW_T3>(e, h, rank, lds);
    else tile_block<1, AW_T1>(e, h, rank, lds);
}

}  // namespace

extern "C" long bts_adamw_table_bytes(int n) { return n <= 0 ? 0 : (long)n * (long)sizeof(AdamwRec); }

extern "C" long bts_adamw_flat_span(void) { return AW_SPAN; }

extern "C" int bts_adamw_plan_f32(const bts_adamw_item* items, int n, void* table_host, long* total_blocks,
                                  bts_adamw_plan_item* plan) {
    if (n < 0 || !total_blocks) return BTS_ERR_INVALID;
    if (n == 0) { *total_blocks = 0; return 0; }
    if (!items || !table_host) return BTS_ERR_INVALID;
    AdamwRec* table = (AdamwRec*)table_host;
    long first = 0;
    for (int i = 0; i < n; ++i) {
        const bts_adamw_item& it = items[i];
        if (!it.p || !it.g || !it.m || !it.v || it.numel <= 0) return BTS_ERR_INVALID;
        if (((uintptr_t)it.p & 3) || ((uintptr_t)it.g & 3) || ((uintptr_t)it.m & 3) || ((uintptr_t)it.v & 3)) return BTS_ERR_INVALID;
        if (it.hyper < 0 || it.hyper >= AW_MAX_HYPER) return BTS_ERR_INVALID;
        if (it.n_packs < 0 || it.n_packs > 2) return BTS_ERR_INVALID;
        const bool geom = it.c_out != 0 || it.c_in != 0 || it.ksize != 0 || it.n_packs > 0;
        if (geom) {
            if (it.c_out <= 0 || it.c_in <= 0 || it.ksize <= 0) return BTS_ERR_INVALID;
            if (it.n_packs > 0 && it.ksize != 1 && it.ksize != 3) return BTS_ERR_INVALID;
            if (it.ksize > 46340) return BTS_ERR_INVALID;
            // exact in 128 bits: c_out, c_in < 2^31 and k*k < 2^31
            if ((__int128)it.c_out * it.c_in * (it.ksize * it.ksize) != (__int128)it.numel) return BTS_ERR_INVALID;
        }
        AdamwRec r;
        r.p = it.p; r.g = it.g; r.m = it.m; r.v = it.v;
        r.numel = it.numel; r.hyper = it.hyper;
        r.c_out = it.c_out; r.c_in = it.c_in; r.ksize = it.ksize;
        r.tiles_c = 0; r.head = 0; r.vec = 0;
        for (int k = 0; k < 2; ++k) { r.dst[k] = nullptr; r.k_pad[k] = 0; r.ld[k] = 0; r.mode[k] = 0; }
        const long kk = (long)it.ksize * it.ksize;
        for (int k = 0; k < it.n_packs; ++k) {
            const bts_adamw_pack& pk = it.packs[k];
            if (!pk.dst || ((uintptr_t)pk.dst & 15) || (pk.mode != 0 && pk.mode != 1)) return BTS_ERR_INVALID;
            const int inner = pk.mode == 0 ? it.c_in : it.c_out;
            if (pk.c_in_ld < inner || pk.k_pad < kk * (long)pk.c_in_ld) return BTS_ERR_INVALID;
            r.dst[k] = pk.dst; r.k_pad[k] = pk.k_pad; r.ld[k] = pk.c_in_ld; r.mode[k] = pk.mode;
        }
        long blocks;
        if (it.n_packs > 0) {
            const int T = it.ksize == 3 ? AW_T3 : AW_T1;
            const long t_o = ((long)it.c_out + T - 1) / T, t_c = ((long)it.c_in + T - 1) / T;
            r.kind = 1;
            r.tiles_c = (int)t_c;
            blocks = t_o * t_c;                     // < 2^52
        } else {
            r.kind = 0;
            blocks = it.numel / AW_SPAN + (it.numel % AW_SPAN != 0);
            const uintptr_t a = (uintptr_t)it.p;
            const int head = (int)(((16 - (a & 15)) & 15) >> 2);
            r.head = head;
            r.vec = ((((uintptr_t)it.g + 4 * head) & 15) == 0 && (((uintptr_t)it.m + 4 * head) & 15) == 0 &&
                     (((uintptr_t)it.v + 4 * head) & 15) == 0) ? 1 : 0;
        }
        r.first_block = first;
        r.n_blocks = blocks;
        if (blocks > 2147483647L - first) return BTS_ERR_INVALID;       // the grid's x extent
        table[i] = r;
        if (plan) { plan[i].kind = r.kind; plan[i].reserved = 0; plan[i].first_block = first; plan[i].n_blocks = blocks; }
        first += blocks;
    }
    *total_blocks = first;
    return 0;
}

extern "C" int bts_adamw_step_f32(const void* table_dev, int n, long total_blocks, const bts_adamw_hyper* hyper, int n_hyper,
                                  const float* skip, bts_stream_t stream) {
    if (n < 0) return BTS_ERR_INVALID;
    if (n == 0) return 0;
    if (!table_dev || ((uintptr_t)table_dev & 15) || total_blocks <= 0 || total_blocks > 2147483647L) return BTS_ERR_INVALID;
    if (!hyper || n_hyper <= 0 || n_hyper > AW_MAX_HYPER || ((uintptr_t)skip & 3)) return BTS_ERR_INVALID;
    AdamwHyperTable hy;
    for (int i = 0; i < AW_MAX_HYPER; ++i) {
        const bts_adamw_hyper& s = hyper[i < n_hyper ? i : 0];
        if (!(s.step >= 1.0) || !(s.beta1 >= 0.0 && s.beta1 < 1.0) || !(s.beta2 >= 0.0 && s.beta2 < 1.0)) return BTS_ERR_INVALID;
        AdamwHyperDev& d = hy.h[i];
        const double bc1 = 1.0 - pow(s.beta1, s.step), bc2 = 1.0 - pow(s.beta2, s.step);
        d.lr = (float)s.lr; d.beta1 = (float)s.beta1; d.beta2 = (float)s.beta2; d.eps = (float)s.eps;
        d.weight_decay = (float)s.weight_decay;
        d.step_size = (float)(s.lr / bc1);
        d.inv_sqrt_bc2 = (float)(1.0 / sqrt(bc2));
        d.decay = (float)(1.0 - s.lr * s.weight_decay);
        d.omb1 = (float)(1.0 - s.beta1);
        d.omb2 = (float)(1.0 - s.beta2);
        d.pad0 = d.pad1 = 0.f;
    }
    hipLaunchKernelGGL(adamw_step_kernel, dim3((unsigned)total_blocks), dim3(AW_THREADS), 0, (hipStream_t)stream,
                       (const AdamwRec*)table_dev, n, hy, skip);
    return (int)hipGetLastError();
}
