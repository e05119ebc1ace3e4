// Training losses as GPU reductions: the masked scale-invariant log loss and the asymmetric L1 depth loss, forward and
// backward (silog_loss / depth_l1_loss).
//
// Restates silog_loss.forward (reference pytorch/bts.py:41-48) and depth_l1_loss.forward (pytorch/bts.py:50-63) as they
// are used by the training step (pytorch/bts_main.py:551-565): ONE reduction over all B*H*W pixels of the batch (the
// reference reduces over the whole batch, not per frame).  The reference gathers `depth_est[mask]` first -- a boolean
// index, i.e. a `nonzero` that waits for the device, a dozen small kernels and an index_put scatter in backward.  Here
// the forward is one pass over est / gt / mask (HBM-bound: 9 B per pixel) that leaves three sums per block, plus a
// one-block kernel that adds the partials in block order; the backward is one elementwise pass that reads the saved
// statistics and the upstream gradient FROM THE DEVICE.  Nothing waits for the host and no shape depends on the data.
// Everything is accumulated in fp64 (d = log(est) - log(gt) in fp64 from the fp32 inputs, as eval.hip does) and in a
// fixed order (no atomics, block count a function of npix only): two runs on the same buffers give the same bits, and
// the result is rounded to fp32 once.  (The order depends on where the 16-byte boundaries of the inputs fall, so the
// same values at a differently aligned address may differ in the last bits of the fp64 sums.)
//
// A pixel is valid when mask[p] != 0, or -- without a mask -- when gt[p] > gt_min (bts_main.py:551-553).  Invalid pixels
// contribute nothing: their est / gt may be 0, negative, inf or NaN and never reach a log whose result is used.
//
// Deliberate deviations from the reference (all three are cases where torch returns NaN or inf):
//   * no valid pixel (n == 0): loss = 0 and the gradient is zero everywhere (torch: mean of an empty tensor, NaN);
//   * silog with v = E[d^2] - vf * E[d]^2 <= 0 (one valid pixel with vf = 1, a constant scale error, or rounding a few
//     ulp below zero): loss = 0 and the gradient is zero everywhere (torch: sqrt of a negative number is NaN, and the
//     derivative of sqrt at 0 is inf);
//   * everything else propagates as IEEE arithmetic does, as in torch: a NaN or non-positive est at a VALID pixel makes
//     the loss NaN (or inf).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "common.h"

namespace {

constexpr int LS_NS = 3;                 // n, sum d, sum d^2  (L1: n, sum of the weighted |e|, unused)
constexpr int LS_THREADS = 256;
constexpr int LS_MAX_BLOCKS = 512;
constexpr int LS_PIX_PER_THREAD = 16;    // four 16-byte loads of est and gt per lane before the grid wraps

struct LossArgs {
    const float* est; const float* gt; const unsigned char* mask;
    float gt_min;
    int kind;                            // 0 = silog, 1 = asymmetric L1
    double param;                        // variance_focus | inbalance_to_closer
    long npix;
    // pixels [head, head + 4 * nvec) are read 16 bytes per lane (est + head and gt + head 16-byte aligned, mask + head
    // 4-byte aligned); the head and the tail -- or everything, nvec = 0, when the pointers do not share an alignment --
    // one element per lane
    long head, nvec;
};

// the split of LossArgs: `p4`, an optional fourth fp32 array (grad_est), must share the alignment too
void split_pixels(LossArgs& a, const float* p4) {
    const uintptr_t e = (uintptr_t)a.est, g = (uintptr_t)a.gt, m = (uintptr_t)a.mask;
    const long head = (long)(((16 - (e & 15)) & 15) >> 2);                         // floats up to est's next 16-byte line
    bool share = ((g + 4 * head) & 15) == 0 && (a.mask == nullptr || ((m + head) & 3) == 0);
    if (p4 != nullptr && (((uintptr_t)p4 + 4 * head) & 15) != 0) share = false;
    a.head = 0; a.nvec = 0;
    if (share && a.npix >= head + 4) { a.head = head; a.nvec = (a.npix - head) / 4; }
}

// index of the j-th pixel that is NOT covered by a 16-byte group
__device__ __forceinline__ long scalar_pixel(const LossArgs& a, long j) { return j < a.head ? j : j + 4 * a.nvec; }

__device__ __forceinline__ bool is_valid(const LossArgs& a, unsigned m, float g) { return a.mask != nullptr ? m != 0u : g > a.gt_min; }

struct LossSums { double n, s1, s2; };

__device__ __forceinline__ void accumulate(const LossArgs& a, float est, float gt, LossSums& s) {
    double c1, c2 = 0.0;
    if (a.kind == 0) {
        c1 = log((double)est) - log((double)gt);                                    // bts.py:45
        c2 = c1 * c1;
    } else {
        const double e = (double)est - (double)gt;                                  // bts.py:57
        c1 = a.param == 1.0 ? fabs(e) : (e > 0.0 ? a.param * e : -e);               // bts.py:58-62 (NaN -> -NaN: still NaN)
    }
    s.n += 1.0;
    s.s1 += c1;
    s.s2 += c2;
}

__global__ __launch_bounds__(LS_THREADS) void loss_partial_kernel(const LossArgs a, double* __restrict__ ws) {
    LossSums s = {0.0, 0.0, 0.0};
    const long stride = (long)gridDim.x * LS_THREADS;
    const long t0 = (long)blockIdx.x * LS_THREADS + threadIdx.x;
    const float4* __restrict__ e4 = reinterpret_cast<const float4*>(a.est + a.head);
    const float4* __restrict__ g4 = reinterpret_cast<const float4*>(a.gt + a.head);
    const uint32_t* __restrict__ m4 = reinterpret_cast<const uint32_t*>(a.mask != nullptr ? a.mask + a.head : nullptr);
    for (long v = t0; v < a.nvec; v += stride) {
        const float4 e = e4[v], g = g4[v];
        const uint32_t m = m4 != nullptr ? m4[v] : 0u;
        if (is_valid(a, m & 0xffu, g.x)) accumulate(a, e.x, g.x, s);
        if (is_valid(a, (m >> 8) & 0xffu, g.y)) accumulate(a, e.y, g.y, s);
        if (is_valid(a, (m >> 16) & 0xffu, g.z)) accumulate(a, e.z, g.z, s);
        if (is_valid(a, m >> 24, g.w)) accumulate(a, e.w, g.w, s);
    }
    const long nscalar = a.npix - 4 * a.nvec;
    for (long j = t0; j < nscalar; j += stride) {
        const long p = scalar_pixel(a, j);
        const float g = a.gt[p];
        if (is_valid(a, a.mask != nullptr ? a.mask[p] : 0u, g)) accumulate(a, a.est[p], g, s);
    }
    // fixed-order block reduction: lanes (shuffle tree), then waves (LDS)
    __shared__ double red[LS_THREADS / 64][LS_NS];
#pragma unroll
    for (int i = 0; i < LS_NS; ++i) {
        double v = i == 0 ? s.n : (i == 1 ? s.s1 : s.s2);
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
        if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6][i] = v;
    }
    __syncthreads();
    if (threadIdx.x < LS_NS) {
        double v = 0.0;
        for (int w = 0; w < LS_THREADS / 64; ++w) v += red[w][threadIdx.x];
        ws[(long)blockIdx.x * LS_NS + threadIdx.x] = v;
    }
}

// one block: sum the partials in block order, derive the loss
__global__ __launch_bounds__(64) void loss_finalize_kernel(const double* __restrict__ ws, int nblk, int kind, double param,
                                                           double* __restrict__ stats, float* __restrict__ loss) {
    __shared__ double tot[LS_NS];
    if (threadIdx.x < LS_NS) {
        double v = 0.0;
        for (int k = 0; k < nblk; ++k) v += ws[(long)k * LS_NS + threadIdx.x];
        tot[threadIdx.x] = v;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        const double n = tot[0];
        double mu = 0.0, m2 = 0.0, l = 0.0;
        if (n > 0.0) {                                                              // n == 0: loss 0 (header, deviation 1)
            if (kind == 0) {
                mu = tot[1] / n;
                m2 = tot[2] / n;
                const double v = m2 - param * mu * mu;                              // bts.py:47
                l = v <= 0.0 ? 0.0 : 10.0 * sqrt(v);                                // v <= 0: loss 0 (deviation 2); NaN stays NaN
            } else {
                l = tot[1] / n;
            }
        }
        stats[0] = n; stats[1] = mu; stats[2] = m2; stats[3] = l;
        *loss = (float)l;
    }
}

__device__ __forceinline__ float loss_grad(const LossArgs& a, float est, float gt, double c, double shift) {
    if (a.kind == 0) {
        const double d = log((double)est) - log((double)gt);
        return (float)(c * (d - shift) / (double)est);                              // c = grad * 100 / (n * loss), shift = vf * mean d
    }
    const double e = (double)est - (double)gt;
    if (a.param == 1.0) return (float)(e > 0.0 ? c : (e < 0.0 ? -c : (e == 0.0 ? 0.0 : e)));   // sign(e) as abs has; NaN stays NaN
    return (float)(e > 0.0 ? a.param * c : -c);                                     // torch.where(err > 0, k * err, -err)
}

__global__ __launch_bounds__(LS_THREADS) void loss_bwd_kernel(const LossArgs a, const double* __restrict__ stats,
                                                              const float* __restrict__ grad_loss, float* __restrict__ grad_est) {
    const double n = stats[0], l = stats[3];
    // silog: d loss / d est_p = 100 (d_p - vf mu) / (n loss est_p); L1: (k | -1 | sign) / n.  Degenerate cases: all zero.
    const bool zero = !(n > 0.0) || (a.kind == 0 && l == 0.0);
    const double c = zero ? 0.0 : (a.kind == 0 ? (double)*grad_loss * 100.0 / (n * l) : (double)*grad_loss / n);
    const double shift = a.param * stats[1];
    const long stride = (long)gridDim.x * LS_THREADS;
    const long t0 = (long)blockIdx.x * LS_THREADS + threadIdx.x;
    const float4* __restrict__ e4 = reinterpret_cast<const float4*>(a.est + a.head);
    const float4* __restrict__ g4 = reinterpret_cast<const float4*>(a.gt + a.head);
    const uint32_t* __restrict__ m4 = reinterpret_cast<const uint32_t*>(a.mask != nullptr ? a.mask + a.head : nullptr);
    float4* __restrict__ o4 = reinterpret_cast<float4*>(grad_est + a.head);
    for (long v = t0; v < a.nvec; v += stride) {
        const float4 e = e4[v], g = g4[v];
        const uint32_t m = m4 != nullptr ? m4[v] : 0u;
        float4 o;
        o.x = !zero && is_valid(a, m & 0xffu, g.x) ? loss_grad(a, e.x, g.x, c, shift) : 0.f;
        o.y = !zero && is_valid(a, (m >> 8) & 0xffu, g.y) ? loss_grad(a, e.y, g.y, c, shift) : 0.f;
        o.z = !zero && is_valid(a, (m >> 16) & 0xffu, g.z) ? loss_grad(a, e.z, g.z, c, shift) : 0.f;
        o.w = !zero && is_valid(a, m >> 24, g.w) ? loss_grad(a, e.w, g.w, c, shift) : 0.f;
        o4[v] = o;
    }
    const long nscalar = a.npix - 4 * a.nvec;
    for (long j = t0; j < nscalar; j += stride) {
        const long p = scalar_pixel(a, j);
        const float g = a.gt[p];
        grad_est[p] = !zero && is_valid(a, a.mask != nullptr ? a.mask[p] : 0u, g) ? loss_grad(a, a.est[p], g, c, shift) : 0.f;
    }
}

bool bad_args(const float* est, const float* gt, long npix, int kind) {
    return !est || !gt || npix <= 0 || (kind != 0 && kind != 1) || ((uintptr_t)est & 3) || ((uintptr_t)gt & 3);
}

}  // namespace

extern "C" long bts_depth_loss_ws_doubles(long npix) {
    if (npix <= 0) return 0;
    long nblk = (npix + (long)LS_THREADS * LS_PIX_PER_THREAD - 1) / ((long)LS_THREADS * LS_PIX_PER_THREAD);
    if (nblk > LS_MAX_BLOCKS) nblk = LS_MAX_BLOCKS;
    return nblk * LS_NS;
}

extern "C" int bts_depth_loss_fwd_f32(const float* est, const float* gt, const unsigned char* mask, float gt_min, long npix,
                                      int kind, float param, double* ws, long ws_doubles, double* stats, float* loss,
                                      bts_stream_t stream) {
    if (bad_args(est, gt, npix, kind) || !ws || !stats || !loss) return BTS_ERR_INVALID;
    const long need = bts_depth_loss_ws_doubles(npix);
    if (ws_doubles < need || ((uintptr_t)ws & 7) || ((uintptr_t)stats & 7) || ((uintptr_t)loss & 3)) return BTS_ERR_INVALID;
    LossArgs a;
    a.est = est; a.gt = gt; a.mask = mask; a.gt_min = gt_min; a.kind = kind; a.param = (double)param; a.npix = npix;
    split_pixels(a, nullptr);
    const int nblk = (int)(need / LS_NS);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(loss_partial_kernel, dim3((unsigned)nblk), dim3(LS_THREADS), 0, s, a, ws);
    hipLaunchKernelGGL(loss_finalize_kernel, dim3(1), dim3(64), 0, s, ws, nblk, kind, a.param, stats, loss);
    return (int)hipGetLastError();
}

extern "C" int bts_depth_loss_bwd_f32(const float* est, const float* gt, const unsigned char* mask, float gt_min, long npix,
                                      int kind, float param, const double* stats, const float* grad_loss, float* grad_est,
                                      bts_stream_t stream) {
    if (bad_args(est, gt, npix, kind) || !stats || !grad_loss || !grad_est) return BTS_ERR_INVALID;
    if (((uintptr_t)stats & 7) || ((uintptr_t)grad_loss & 3) || ((uintptr_t)grad_est & 3)) return BTS_ERR_INVALID;
    LossArgs a;
    a.est = est; a.gt = gt; a.mask = mask; a.gt_min = gt_min; a.kind = kind; a.param = (double)param; a.npix = npix;
    split_pixels(a, grad_est);
    // one 16-byte group (or one head / tail pixel) per lane; the grid wraps only beyond 2^21 groups
    long work = a.nvec > a.npix - 4 * a.nvec ? a.nvec : a.npix - 4 * a.nvec;
    long nblk = (work + LS_THREADS - 1) / LS_THREADS;
    if (nblk > 8192) nblk = 8192;
    hipLaunchKernelGGL(loss_bwd_kernel, dim3((unsigned)nblk), dim3(LS_THREADS), 0, (hipStream_t)stream, a, stats, grad_loss, grad_est);
    return (int)hipGetLastError();
}
