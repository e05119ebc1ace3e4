// Convolution weight gradient for the BTS training step (reference: autograd of every nn.Conv2d on the path,
// pytorch/bts.py:70-77, 87-93, 108-119, 180-221; training caller bts_main.py:476-500) on gfx950.
//
//   dw[co][tap][ci] = sum over output pixels p of  dy[p][co] * x[q(p,tap)][ci]
//
// As a GEMM:  C[M = c_out][N = taps*c_in] = A^T[K = pixels][M] (dy, NHWC)  x  B[K = pixels][N] (gathered x, NHWC).
// Both operands are K-major with their M/N index contiguous in memory -- exactly how NHWC stores them -- so a
// tile row (one pixel) is loaded with coalesced 16-byte reads and lands in LDS as [k][m] / [k][n]; an MFMA operand
// is then one conflict-free ds_read_b32 (lane l reads row 2*kk + (l>>5), column base + (l&31)).
// K is the long axis (B*H*W up to 6.8 M pixels) and the output is small, so the launch splits K over gridDim.y;
// partials go to a workspace and are summed in a fixed order (sum_splits: deterministic, no atomics); plan_wgrad picks
// the tile (WGRAD_TILES: 128x128 / 64x128 / 32x128 / 64x64) and the split together.
//
// Three entry points share the tile body (wgrad_tile), the tile table, the split rules and the split sum:
// bts_conv_wgrad_f32 (one problem), bts_upconv_wgrad_f32 (the sub-pixel upconv's four class gradients, folded) and
// bts_conv_wgrad_batch_f32; bts_conv_wgrad_bf16_f32 / bts_conv_wgrad_batch_bf16_f32 are the first and the last with the
// tile body's BF16 form (bf16 operands, fp32 accumulation; same plan, same split sum).
// bts_conv_wgrad_batch_f32 runs many problems (a DenseNet block's 2*L weight gradients) in one launch per tile
// shape plus one reduction launch; its planner sees the whole batch.  The weight packs live in pack.hip.
// Batch planner, the rule kept:
//   tile   per problem, by the single planner's shape terms alone: useful fraction of the padded tile grid x per-tile
//          efficiency.  Its chip-fill and partial-traffic terms are properties of the whole batch here, not of a tile.
//   split  one pixel quantum q (a multiple of 32 pixels, at least 4 K-steps) for the whole batch: split_i =
//          ceil(M_i / q), within the single planner's limits (>= 4 K-steps per split unless M is smaller, <= 1024), then
//          settled as there (pix_per_split rounded up to 32, no empty split).  q is the LARGEST quantum at which the batch
//          still has >= max(768, T / 128) workgroups, T = sum of tiles_i x K-steps_i: 768 is the single planner's target
//          (three per CU, two resident); T / 128 asks for workgroups of about 128 K-steps (4096 pixels) once the batch
//          has work for more than 768 of them.  A batch that has that many workgroups unsplit is not split at all.  One
//          quantum rather than one split count makes every workgroup of the batch walk about the same number of pixels
//          whatever its problem's M; the largest such q is the least partial traffic that fills the chip.  Why not a
//          flat 768: all workgroups of a batch take about equally long, so the grid runs in rounds of the 512 resident
//          ones and a batch of 800 pays for two rounds.  Measured so (MI355X, DenseNet161 at 4x352x704): block 1 as 810
//          workgroups of 323 K-steps and block 2 as 990 of 162 ran at 0.76x / 0.79x the speed of their single launches;
//          at ~128 K-steps a long batch runs several rounds and the last, partly filled one costs less (0.97x / 0.93x), while
//          blocks 3 and 4 (121 / 31 K-steps unsplit, 3078 / 2484 tiles) stay unsplit (DESIGN.md 3a has the tables).
//   ws     if the partials at that q exceed the workspace, q grows to the smallest quantum whose partials fit (none
//          at all in the limit): lack of workspace lowers splits, it never fails.
//   order  inside a tile shape's grid, problems whose workgroups walk the most K-steps come first (dispatched first);
//          ties are broken by shape, then by position.  Tile, split and pix_per_split of a problem therefore do not depend
//          on the batch order at all; ws_offset is handed out in that order, so among problems of EQUAL shape it goes by
//          position: permuting a batch permutes the offsets of equal-shape problems among themselves, and the set of
//          workspace regions stays the same.
// Everything above reads shapes and ws_floats only.
#include "common.h"
#include <stdint.h>
#include <algorithm>
#include <vector>

namespace {

constexpr int WBK = 32;   // pixels per K-step

// What wgrad_tile reads besides pointers; a batch table entry (WgradBatchEntry) stores the same struct.
struct WgradGeom {
    long x_pix_stride, dy_pix_stride;
    int c_in, c_out, N;          // N = taps * c_in
    int B, h_in, w_in, Hs, Ws, ups, H, W, ksize, dil, stride, pad;
    unsigned M;                  // B*H*W output pixels
    unsigned pix_per_split;      // multiple of WBK
    int n_ntiles;
};

struct WgradArgs {
    const float* __restrict__ x;
    const float* __restrict__ dy;
    float* __restrict__ out;     // dw (ksplit == 1) or the partial-sum workspace [ksplit][c_out][N]
    WgradGeom g;
    const float* pre_scale; const float* pre_shift; int pre_relu;   // optional per-input-channel affine (+ReLU) applied to x
                                 // in the gather: the forward convolution saw relu(x*scale + shift) (a folded norm layer)
    int n_bundles;               // grouped convolution as channel bundles (blockIdx.z): bundle j uses input channels
                                 // [j*c_in, ..), gradient channels [j*c_out, ..) and writes dense block j of [c_out][N]
};

typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

// Four channels of two pixels as four dwords of bf16 pairs, rounded to nearest even (a plain conversion: hipcc emits
// v_cvt_pk_bf16_f32, two values per instruction); low half = the even pixel.
__device__ __forceinline__ u32x4 pack_pairs(const f32x4 even, const f32x4 odd) {
    u32x4 r;
#pragma unroll
    for (int c = 0; c < 4; ++c) r[c] = __builtin_bit_cast(unsigned, __builtin_convertvector(f32x2{even[c], odd[c]}, bf16x2));
    return r;
}

// One workgroup = 4 waves arranged WM x WN over a BM x BN tile of dw; each wave owns (BM/WM) x (BN/WN).  The body is
// shared by the single-problem launch (tile / split / bundle = blockIdx.x / .y / .z) and the batched launch (all three
// derived from the workgroup's rank inside its problem).
//
// SUBPIX (bts_upconv_wgrad_f32): the sub-pixel upconv's class gradients.  `bundle` is then the parity class 2*py + px, the
// K axis walks the B*h*w SOURCE pixels (g.H x g.W = g.Hs x g.Ws = the source map), the A operand of pixel (b, Y, X) is
// dy at (b, 2Y+py, 2X+px) of the [B, 2h, 2w] gradient, and the 2x2 taps gather x at (Y-1+py+ty, X-1+px+tx); neither
// operand is offset by the class, and the class results land in dense blocks [split][class][c_out][4*c_in] of a.out.
//
// BF16 (bts_conv_wgrad_bf16_f32): both operands are rounded to the nearest bf16 (ties to even) on their way to LDS -- x
// after its prologue and zero padding -- and a 32x32 block takes one v_mfma_f32_32x32x16_bf16 per 16 pixels, accumulated in
// fp32.  That instruction wants 8 consecutive k per lane while both operands are K-major in memory, so the K-step is staged
// as pixel PAIRS: a loader thread owns pixels 2r and 2r+1 of the step for its four channels and writes one 16-byte store of
// four dwords (pixel 2r in the low half, 2r+1 in the high half) into an image [16 pair-rows][BM or BN] of dwords -- half the
// LDS of the fp32 body.  Lane l's fragment of the 16-k block kb is then four ds_read_b32: pair-rows 8 kb + 4 (l >> 5) + 0..3,
// column l & 31 (k = 8 (l >> 5) + j in element j, the map of both operands).  The order of k inside a block is free as long
// as A and B agree, and they are staged by the same rule.  A pixel past the split's end is a zero partner.  Tile, split,
// guards, epilogue and the registers' double staging are the fp32 body's.
template <int BM, int BN, int WM, int WN, bool SUBPIX = false, bool BF16 = false>
__device__ __forceinline__ void wgrad_tile(const WgradArgs& a, const unsigned tile, const unsigned split_idx,
                                           const unsigned bundle) {
    static_assert(WM * WN == 4, "4 waves");
    constexpr int TM = BM / WM / 32, TN = BN / WN / 32;
    static_assert(TM >= 1 && TN >= 1, "wave tile must be at least 32x32");
    constexpr int ACOLS = BM / 4, BCOLS = BN / 4;          // float4 columns per tile row
    // fp32: rows covered per pass, register p of a thread is row a_row + p * AROWS.  BF16: pair-rows covered per pass (at
    // most the 16 of a K-step: a 32-wide operand is loaded by the first 128 threads), registers 2q and 2q+1 are the two
    // pixels of pair-row a_row + q * AROWS.
    constexpr int AROWS = BF16 ? (256 / ACOLS < WBK / 2 ? 256 / ACOLS : WBK / 2) : 256 / ACOLS;
    constexpr int BROWS = BF16 ? (256 / BCOLS < WBK / 2 ? 256 / BCOLS : WBK / 2) : 256 / BCOLS;
    constexpr int PA = WBK / AROWS, PB = WBK / BROWS;
    static_assert(PA >= 1 && PB >= 1, "tile too wide for 256 loader threads");
    static_assert(!BF16 || (PA % 2 == 0 && PB % 2 == 0), "pixel pairs");
    const WgradGeom& g = a.g;

    extern __shared__ __attribute__((aligned(16))) float lds[];
    float* As = lds;                       // [2][WBK][BM]
    float* Bs = lds + 2 * WBK * BM;        // [2][WBK][BN]
    [[maybe_unused]] unsigned* Au = reinterpret_cast<unsigned*>(lds);     // BF16: [2][WBK / 2][BM] pixel pairs
    [[maybe_unused]] unsigned* Bu = Au + WBK * BM;                        //       [2][WBK / 2][BN]

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm0 = (wave / WN) * (BM / WM), wn0 = (wave % WN) * (BN / WN);
    const int l31 = lane & 31, khalf = lane >> 5;
    const int tile_n = tile % g.n_ntiles, tile_m = tile / g.n_ntiles;
    const int m0 = tile_m * BM, n0 = tile_n * BN;
    const float* __restrict__ xg = a.x + (SUBPIX ? (size_t)0 : (size_t)bundle * g.c_in);      // this bundle's channel slice
    const float* __restrict__ dyg = a.dy + (SUBPIX ? (size_t)0 : (size_t)bundle * g.c_out);
    [[maybe_unused]] const int cpy = (int)(bundle >> 1), cpx = (int)(bundle & 1);             // SUBPIX: the class parities

    // ---- loader roles (fixed for the whole K walk) ----
    const int a_col = (tid % ACOLS) * 4, a_row = tid / ACOLS;
    const int b_col = (tid % BCOLS) * 4, b_row = tid / BCOLS;
    const bool a_act = !BF16 || a_row < AROWS, b_act = !BF16 || b_row < BROWS;
    auto a_rowof = [&](int p) __attribute__((always_inline)) { return BF16 ? 2 * (a_row + (p >> 1) * AROWS) + (p & 1) : a_row + p * AROWS; };
    auto b_rowof = [&](int p) __attribute__((always_inline)) { return BF16 ? 2 * (b_row + (p >> 1) * BROWS) + (p & 1) : b_row + p * BROWS; };
    const bool a_ok = m0 + a_col < g.c_out && a_act;        // c_out % 4 == 0: a float4 is all real or all padding
    const int a_m = a_ok ? m0 + a_col : 0;
    const int n4 = n0 + b_col;
    const bool b_ok = n4 < g.N && b_act;
    const int nn = b_ok ? n4 : 0;
    const int tap = nn / g.c_in, ci = nn - tap * g.c_in;    // c_in % 4 == 0: a float4 never straddles a tap
    const int ky = tap / g.ksize, kx = tap - ky * g.ksize;
    const int off_y = SUBPIX ? ky - 1 + cpy : ky * g.dil - g.pad, off_x = SUBPIX ? kx - 1 + cpx : kx * g.dil - g.pad;

    const unsigned k_begin = split_idx * g.pix_per_split;
    const unsigned k_end = min(g.M, k_begin + g.pix_per_split);
    const int n_it = k_begin < k_end ? (int)((k_end - k_begin + WBK - 1) / WBK) : 0;
    const unsigned HW = (unsigned)g.H * (unsigned)g.W;

    // Two staging register sets: the loads of tile it+2 are issued at the top of step it and consumed (written to LDS)
    // at the bottom of step it+1, so every global load has two full MFMA steps to land.
    f32x4 ra0[PA], rb0[PB], ra1[PA], rb1[PB];
    f32x4 psc = {1.f, 1.f, 1.f, 1.f}, psh = {0.f, 0.f, 0.f, 0.f};          // this thread's four input channels never change
    const bool has_pre = a.pre_scale != nullptr;
    if (has_pre) {
        const int cpre = (SUBPIX ? 0 : (int)bundle * g.c_in) + ci;
        psc = *reinterpret_cast<const f32x4*>(a.pre_scale + cpre);
        psh = *reinterpret_cast<const f32x4*>(a.pre_shift + cpre);
    }
    int pb[PB], py[PB], px[PB];             // (frame, row, column) of each gathered row's output pixel at the next step
#pragma unroll
    for (int p = 0; p < PB; ++p) {
        const unsigned pix = k_begin + b_rowof(p);
        const unsigned b = pix / HW, rem = pix - b * HW;
        pb[p] = (int)b;
        py[p] = (int)(rem / (unsigned)g.W);
        px[p] = (int)(rem - (unsigned)py[p] * (unsigned)g.W);
    }
    [[maybe_unused]] int qb[PA], qy[PA], qx[PA];   // SUBPIX: (frame, row, column) of each A row's source pixel at the next step
    if constexpr (SUBPIX) {
#pragma unroll
        for (int p = 0; p < PA; ++p) {
            const unsigned pix = k_begin + a_rowof(p);
            const unsigned b = pix / HW, rem = pix - b * HW;
            qb[p] = (int)b;
            qy[p] = (int)(rem / (unsigned)g.W);
            qx[p] = (int)(rem - (unsigned)qy[p] * (unsigned)g.W);
        }
    }
    auto issue = [&](int it, f32x4 (&ra)[PA], f32x4 (&rb)[PB]) __attribute__((always_inline)) {
        const unsigned base = k_begin + (unsigned)it * WBK;
        if (!BF16 || a_act)                                              // BF16 32-wide A: threads 128.. load nothing
#pragma unroll
        for (int p = 0; p < PA; ++p) {
            const unsigned pix = base + a_rowof(p);
            const bool ok = a_ok && pix < k_end;
            size_t row = ok ? pix : 0u;
            if constexpr (SUBPIX) {                                      // dy lives at (2Y+py, 2X+px) of the [B,2h,2w] map
                row = ok ? ((size_t)qb[p] * (2 * g.H) + (size_t)(2 * qy[p] + cpy)) * (size_t)(2 * g.W) + (size_t)(2 * qx[p] + cpx) : 0;
                qx[p] += WBK;
                while (qx[p] >= g.W) { qx[p] -= g.W; ++qy[p]; }
                while (qy[p] >= g.H) { qy[p] -= g.H; ++qb[p]; }
            }
            const float* src = dyg + row * g.dy_pix_stride + a_m;
            f32x4 v = *reinterpret_cast<const f32x4*>(src);
            ra[p] = ok ? v : (f32x4)(0.f);
        }
#pragma unroll
        for (int p = 0; p < PB; ++p) {
            const unsigned pix = base + b_rowof(p);
            const int iy = py[p] * g.stride + off_y, ix = px[p] * g.stride + off_x;
            const bool ok = b_ok && pix < k_end && iy >= 0 && iy < g.Hs && ix >= 0 && ix < g.Ws;
            const int sb = ok ? pb[p] : 0, sy = ok ? (iy >> g.ups) : 0, sx = ok ? (ix >> g.ups) : 0;
            const float* src = xg + ((size_t)(sb * g.h_in + sy) * g.w_in + sx) * g.x_pix_stride + ci;
            f32x4 v = *reinterpret_cast<const f32x4*>(src);
            if (has_pre) {
                v = v * psc + psh;
                if (a.pre_relu) v = __builtin_elementwise_max(v, (f32x4)(0.f));
            }
            rb[p] = ok ? v : (f32x4)(0.f);                               // zero padding AFTER the prologue
            // advance this row's output pixel by one K-step without dividing (issue() is called for it = 0, 1, 2, ...)
            px[p] += WBK;
            while (px[p] >= g.W) { px[p] -= g.W; ++py[p]; }
            while (py[p] >= g.H) { py[p] -= g.H; ++pb[p]; }
        }
    };
    auto stage = [&](int buf, const f32x4 (&ra)[PA], const f32x4 (&rb)[PB]) __attribute__((always_inline)) {
        if constexpr (BF16) {
            if (a_act) {
#pragma unroll
                for (int q = 0; q < PA / 2; ++q)
                    *reinterpret_cast<u32x4*>(&Au[(buf * (WBK / 2) + a_row + q * AROWS) * BM + a_col]) = pack_pairs(ra[2 * q], ra[2 * q + 1]);
            }
            if (b_act) {
#pragma unroll
                for (int q = 0; q < PB / 2; ++q)
                    *reinterpret_cast<u32x4*>(&Bu[(buf * (WBK / 2) + b_row + q * BROWS) * BN + b_col]) = pack_pairs(rb[2 * q], rb[2 * q + 1]);
            }
            return;
        }
#pragma unroll
        for (int p = 0; p < PA; ++p)
            *reinterpret_cast<f32x4*>(&As[(buf * WBK + a_row + p * AROWS) * BM + a_col]) = ra[p];
#pragma unroll
        for (int p = 0; p < PB; ++p)
            *reinterpret_cast<f32x4*>(&Bs[(buf * WBK + b_row + p * BROWS) * BN + b_col]) = rb[p];
    };

    f32x16 acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j) acc[i][j] = (f32x16)(0.f);

    auto mfma_step = [&](int cur) __attribute__((always_inline)) {
        if constexpr (BF16) {
            const unsigned* Ac = Au + cur * (WBK / 2) * BM + wm0 + l31;
            const unsigned* Bc = Bu + cur * (WBK / 2) * BN + wn0 + l31;
#pragma unroll
            for (int kb = 0; kb < WBK / 16; ++kb) {
                u32x4 av[TM], bv[TN];
#pragma unroll
                for (int e = 0; e < 4; ++e) {
#pragma unroll
                    for (int i = 0; i < TM; ++i) av[i][e] = Ac[(8 * kb + 4 * khalf + e) * BM + 32 * i];
#pragma unroll
                    for (int j = 0; j < TN; ++j) bv[j][e] = Bc[(8 * kb + 4 * khalf + e) * BN + 32 * j];
                }
#pragma unroll
                for (int i = 0; i < TM; ++i)
#pragma unroll
                    for (int j = 0; j < TN; ++j)
                        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, av[i]), __builtin_bit_cast(bf16x8, bv[j]),
                                                                            acc[i][j], 0, 0, 0);
            }
            return;
        }
        const float* Ac = As + cur * WBK * BM + wm0 + l31;
        const float* Bc = Bs + cur * WBK * BN + wn0 + l31;
#pragma unroll
        for (int kk = 0; kk < WBK / 2; ++kk) {
            float av[TM], bv[TN];
#pragma unroll
            for (int i = 0; i < TM; ++i) av[i] = Ac[(2 * kk + khalf) * BM + 32 * i];
#pragma unroll
            for (int j = 0; j < TN; ++j) bv[j] = Bc[(2 * kk + khalf) * BN + 32 * j];
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int j = 0; j < TN; ++j) acc[i][j] = mfma32x2(av[i], bv[j], acc[i][j]);
        }
    };

    if (n_it > 0) {
        issue(0, ra0, rb0);
        if (n_it > 1) issue(1, ra1, rb1);
        stage(0, ra0, rb0);
    }
    __syncthreads();
    for (int it = 0; it < n_it; it += 2) {
        // even step: LDS[0] holds tile it, set 1 holds tile it+1, set 0 is free
        if (it + 2 < n_it) issue(it + 2, ra0, rb0);
        mfma_step(0);
        if (it + 1 < n_it) stage(1, ra1, rb1);
        __syncthreads();
        if (it + 1 >= n_it) break;
        // odd step: LDS[1] holds tile it+1, set 0 holds tile it+2, set 1 is free
        if (it + 3 < n_it) issue(it + 3, ra1, rb1);
        mfma_step(1);
        if (it + 2 < n_it) stage(0, ra0, rb0);
        __syncthreads();
    }

    // ---- store: D register r of lane l is row (r&3) + 8*(r>>2) + 4*(l>>5), column l&31 ----
    float* out = a.out + ((size_t)split_idx * a.n_bundles + bundle) * g.c_out * g.N;
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j) {
            const int n = n0 + wn0 + 32 * j + l31;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int m = m0 + wm0 + 32 * i + (r & 3) + 8 * (r >> 2) + 4 * khalf;
                if (m < g.c_out && n < g.N) out[(size_t)m * g.N + n] = acc[i][j][r];
            }
        }
}

template <int BM, int BN, int WM, int WN, bool BF16 = false>
__global__ __launch_bounds__(256, 2) void conv_wgrad_kernel(const WgradArgs a) {
    wgrad_tile<BM, BN, WM, WN, false, BF16>(a, blockIdx.x, blockIdx.y, blockIdx.z);
}

template <int BM, int BN, int WM, int WN>
__global__ __launch_bounds__(256, 2) void upconv_wgrad_kernel(const WgradArgs a) {
    wgrad_tile<BM, BN, WM, WN, true>(a, blockIdx.x, blockIdx.y, blockIdx.z);
}

// ---- the fixed-order sum of the ksplit partials, the same code in the three reduce kernels ----
// The output is small and the split count can be in the hundreds, so the walk over splits is itself spread over 16 lanes
// per element (a serial walk is pure load latency): a block owns 16 consecutive float4 elements, lane j adds splits j,
// j+16, ... (sum_splits: four independent loads in flight, added as (a0+a1)+(a2+a3), then one at a time), then lane 0
// adds the 16 lane sums in lane order (sum_lanes).  Both live in common.h: the grouped weight gradient (conv_grouped_wgrad.inc)
// sums its partials with them too.

// dw[0 .. count4) = the split sum of ws [ksplit][count4] float4s; element t = 16 * block + el, lane = split residue.
__device__ __forceinline__ void reduce_block(const float* __restrict__ ws, float* __restrict__ dw, long count4, int ksplit,
                                             long block) {
    const int el = threadIdx.x & 15, lane = threadIdx.x >> 4;
    const long t = block * 16 + el;
    const long tt = t < count4 ? t : count4 - 1;
    __shared__ f32x4 red[16][16];
    red[lane][el] = sum_splits(reinterpret_cast<const f32x4*>(ws) + tt, (size_t)count4, ksplit, lane);
    __syncthreads();
    if (lane == 0 && t < count4) reinterpret_cast<f32x4*>(dw)[t] = sum_lanes(red, el);
}

__global__ __launch_bounds__(256) void wgrad_reduce_kernel(const float* __restrict__ ws, float* __restrict__ dw,
                                                           long count4, int ksplit) {
    reduce_block(ws, dw, count4, ksplit, (long)blockIdx.x);
}

// Sub-pixel upconv (bts_upconv_wgrad_f32): wgrad_tile<SUBPIX> with the class as gridDim.z writes the class gradients
// [c_out] x [4*c_in] as [split][class][c_out][4*c_in] into the caller's workspace (split >= 1: the class results need a
// home even unsplit).  This kernel then produces dw[co][3*ky+kx][ci] in a FIXED order:
//   1. per class cls = 0..3, the split partials of element (co, tau_py(ky)*2 + tau_px(kx), ci) by sum_splits + sum_lanes -> r_cls;
//   2. dw = ((r_0 + r_1) + r_2) + r_3.
// tau_0 = (0,1,1), tau_1 = (0,0,1): the adjoint of the pre-sum in pack_upconv_subpixel.  No atomics; bit-reproducible.
__global__ __launch_bounds__(256) void upconv_wgrad_fold_kernel(const float* __restrict__ ws, float* __restrict__ dw, int c_out,
                                                                int c_in, int ksplit) {
    const long count4 = (long)c_out * 9 * c_in / 4;
    const long per = (long)c_out * 4 * c_in;               // floats of one class block; one split = four of them = per float4s
    const int el = threadIdx.x & 15, lane = threadIdx.x >> 4;
    const long t = (long)blockIdx.x * 16 + el;
    const long tt = t < count4 ? t : count4 - 1;
    const long idx = tt * 4;
    const int co = (int)(idx / (9L * c_in));
    const int rem = (int)(idx - (long)co * 9 * c_in);
    const int tap = rem / c_in, ci = rem - tap * c_in;
    const int ky = tap / 3, kx = tap - 3 * ky;
    __shared__ f32x4 red[4][16][16];
#pragma unroll
    for (int cls = 0; cls < 4; ++cls) {
        const int py = cls >> 1, px = cls & 1;
        const int ty = py == 0 ? (ky >= 1) : (ky >= 2), tx = px == 0 ? (kx >= 1) : (kx >= 2);
        const float* p = ws + (long)cls * per + ((long)co * 4 + (ty * 2 + tx)) * c_in + ci;
        red[cls][lane][el] = sum_splits(reinterpret_cast<const f32x4*>(p), (size_t)per, ksplit, lane);
    }
    __syncthreads();
    if (lane == 0 && t < count4) {
        f32x4 r[4];
#pragma unroll
        for (int cls = 0; cls < 4; ++cls) r[cls] = sum_lanes(red[cls], el);
        reinterpret_cast<f32x4*>(dw)[t] = ((r[0] + r[1]) + r[2]) + r[3];
    }
}

// ---- host: the four tiles, the shape score and the split rules, each stated once ----
struct WgradTileInfo { int bm, bn, wm, wn; double eff; };      // workgroup tile, wave arrangement, measured per-tile efficiency
constexpr WgradTileInfo WGRAD_TILES[4] = {{128, 128, 2, 2, 1.0}, {64, 128, 1, 4, 0.9}, {32, 128, 1, 4, 0.75}, {64, 64, 2, 2, 0.8}};

template <int V> struct WgradTile {                             // WGRAD_TILES[V] as a type: the kernels' template arguments
    static constexpr int BM = WGRAD_TILES[V].bm, BN = WGRAD_TILES[V].bn, WM = WGRAD_TILES[V].wm, WN = WGRAD_TILES[V].wn;
};

// A tile index (WgradPlan::variant) onto its type: f(WgradTile<variant>{}).
template <typename F> inline int for_wgrad_tile(int variant, F f) {
    switch (variant) {
        case 0: return f(WgradTile<0>{});
        case 1: return f(WgradTile<1>{});
        case 2: return f(WgradTile<2>{});
        default: return f(WgradTile<3>{});
    }
}

inline long wgrad_n_tiles(const WgradTileInfo& t, int c_out, int N) {
    return (long)((c_out + t.bm - 1) / t.bm) * ((N + t.bn - 1) / t.bn);
}

// The shape terms of a tile's score: useful fraction of the padded tile grid x per-tile efficiency.
inline double wgrad_shape_score(const WgradTileInfo& t, int c_out, int N) {
    const double useful = (double)c_out * N / ((double)wgrad_n_tiles(t, c_out, N) * t.bm * t.bn);
    return useful * t.eff;
}

// The tile of one problem inside a batch: the best shape score alone, with plan_wgrad's tie rule.
inline int wgrad_best_shape_tile(int c_out, int N) {
    int best = 0;
    double best_score = -1.0;
    for (int v = 0; v < 4; ++v) {
        const double score = wgrad_shape_score(WGRAD_TILES[v], c_out, N);
        if (score > best_score * 1.0001) { best_score = score; best = v; }
    }
    return best;
}

// At least 4 K-steps per split (unless M is smaller), at most 1024 splits.
inline long wgrad_max_split(long M) { return std::min(std::max(M / (4 * WBK), 1L), 1024L); }

// Settle a wanted split: pix_per_split rounded up to whole K-steps, then no empty split.
struct WgradSplit { long split, pps; };
inline WgradSplit wgrad_settle_split(long M, long split) {
    const long pps = ((M + split - 1) / split + WBK - 1) / WBK * WBK;
    return {(M + pps - 1) / pps, pps};
}

// Tile + split plan.  The output (c_out x taps*c_in) is small and the pixel axis long, so parallelism comes from
// splitting pixels; every split costs one partial tile written and re-read.  Candidates are scored by
//   useful fraction of the padded tile grid  x  per-tile efficiency  x  chip fill (workgroups / 512, capped at 1)
//   x  operand bytes / (operand bytes + partial-tile bytes)
// with the split chosen to reach ~768 workgroups within [>= 4 K-steps per split, <= 1024 splits, workspace size].
struct WgradPlan { int variant; long split; };

inline WgradPlan plan_wgrad(int c_out, int N, long M, long ws_floats, bool have_ws, int n_bundles) {
    constexpr long target = 768;                                       // workgroups a split aims for (see above)
    const long per = (long)c_out * N * n_bundles;
    long max_split = wgrad_max_split(M);
    if (!have_ws || ws_floats < 2 * per) max_split = 1;
    else if (max_split * per > ws_floats) max_split = ws_floats / per;
    const double in_bytes = 4.0 * (double)M * (c_out + N);           // operands read once (taps re-read from cache)
    WgradPlan best = {0, 1};
    double best_score = -1.0;
    for (int v = 0; v < 4; ++v) {
        const long tiles = wgrad_n_tiles(WGRAD_TILES[v], c_out, N) * n_bundles;
        const long split = std::min((target + tiles - 1) / tiles, max_split);
        const double fill = std::min((double)(tiles * split) / 512.0, 1.0);
        const double partial_bytes = split > 1 ? 8.0 * (double)split * (double)per : 0.0;   // written once, read once
        const double score = wgrad_shape_score(WGRAD_TILES[v], c_out, N) * fill * in_bytes / (in_bytes + partial_bytes);
        if (score > best_score * 1.0001) { best_score = score; best = {v, split}; }
    }
    return best;
}

// plan_wgrad's tile and its split, settled into a.g.pix_per_split: the end of both prepare_* functions.
inline WgradPlan plan_and_settle(WgradArgs& a, long ws_floats, bool have_ws) {
    WgradPlan p = plan_wgrad(a.g.c_out, a.g.N, (long)a.g.M, ws_floats, have_ws, a.n_bundles);
    const WgradSplit s = wgrad_settle_split((long)a.g.M, p.split);
    p.split = s.split;
    a.g.pix_per_split = (unsigned)s.pps;
    return p;
}

// The answer of both plan queries.
inline int report_plan(const WgradPlan& p, const WgradArgs& a, int* bm, int* bn, long* split, long* pix_per_split) {
    if (bm) *bm = WGRAD_TILES[p.variant].bm;
    if (bn) *bn = WGRAD_TILES[p.variant].bn;
    if (split) *split = p.split;
    if (pix_per_split) *pix_per_split = (long)a.g.pix_per_split;
    return 0;
}

// The tile grid of one problem under tile T: sets g.n_ntiles, returns the tiles.
template <typename T> long wgrad_tile_grid(WgradGeom& g) {
    g.n_ntiles = (g.N + T::BN - 1) / T::BN;
    return (long)((g.c_out + T::BM - 1) / T::BM) * g.n_ntiles;
}

// Enqueue a wgrad_tile kernel of tile T: its LDS (two stages of both operands; BF16: as pixel pairs, half the bytes), raised
// above the default where needed.
// Returns that step's error, or 0 with the kernel enqueued; the caller reads hipGetLastError after its last launch.
template <typename T, auto Kern, bool BF16 = false, typename... Args> int launch_wgrad_tiles(dim3 grid, hipStream_t s, Args... args) {
    return bts_launch<Kern>(grid, dim3(256), (size_t)2 * WBK * (T::BM + T::BN) * (BF16 ? sizeof(unsigned) / 2 : sizeof(float)), s, args...);
}

// `a` and `split` come from prepare_wgrad: a.g.pix_per_split and the split count are final here.
template <typename T, bool BF16 = false> int launch_wgrad(WgradArgs a, long split, float* dw, float* ws, hipStream_t s) {
    const long tiles = wgrad_tile_grid<T>(a.g);
    a.out = split > 1 ? ws : dw;
    if (const int rc = launch_wgrad_tiles<T, conv_wgrad_kernel<T::BM, T::BN, T::WM, T::WN, BF16>, BF16>(
            dim3((unsigned)tiles, (unsigned)split, (unsigned)a.n_bundles), s, a); rc != 0) return rc;
    if (split > 1) {
        const long count4 = (long)a.g.c_out * a.g.N * a.n_bundles / 4;      // N % 4 == 0
        hipLaunchKernelGGL(wgrad_reduce_kernel, dim3((unsigned)((count4 + 15) / 16)), dim3(256), 0, s, ws, dw, count4, (int)split);
    }
    return (int)hipGetLastError();
}

template <typename T> int launch_upconv_wgrad(WgradArgs a, long split, float* dw, float* ws, hipStream_t s) {
    const long tiles = wgrad_tile_grid<T>(a.g);
    a.out = ws;
    if (const int rc = launch_wgrad_tiles<T, upconv_wgrad_kernel<T::BM, T::BN, T::WM, T::WN>>(
            dim3((unsigned)tiles, (unsigned)split, 4u), s, a); rc != 0) return rc;
    const long count4 = (long)a.g.c_out * 9 * a.g.c_in / 4;
    hipLaunchKernelGGL(upconv_wgrad_fold_kernel, dim3((unsigned)((count4 + 15) / 16)), dim3(256), 0, s, (const float*)ws, dw,
                       a.g.c_out, a.g.c_in, (int)split);
    return (int)hipGetLastError();
}

// Everything bts_conv_wgrad_f32 decides on the host, shared with the plan query (no GPU work): validates the
// descriptor, fills the kernel arguments (a.out / g.n_ntiles are the launch's), picks the tile and settles the split.
// Returns 0 or a BTS_ERR_* code.
int prepare_wgrad(const bts_conv_wgrad_desc* d, WgradArgs& a, WgradPlan& p) {
    if (!d || !d->x || !d->dy || !d->dw) return BTS_ERR_INVALID;
    if (d->B <= 0 || d->h_in <= 0 || d->w_in <= 0 || d->c_in <= 0 || d->c_out <= 0) return BTS_ERR_INVALID;
    if (d->up != 1 && d->up != 2) return BTS_ERR_UNSUPPORTED;
    if (d->ksize < 1 || d->ksize > 7 || !(d->ksize & 1)) return BTS_ERR_UNSUPPORTED;
    if (d->dil < 1 || d->stride < 1 || d->pad < 0) return BTS_ERR_INVALID;
    if (d->up == 2 && d->stride != 1) return BTS_ERR_UNSUPPORTED;
    if ((d->c_in & 3) || (d->c_out & 3)) return BTS_ERR_INVALID;
    if ((d->x_pix_stride & 3) || d->x_pix_stride < d->c_in) return BTS_ERR_INVALID;
    if ((d->dy_pix_stride & 3) || d->dy_pix_stride < d->c_out) return BTS_ERR_INVALID;
    if (((uintptr_t)d->x & 15) || ((uintptr_t)d->dy & 15) || ((uintptr_t)d->dw & 15)) return BTS_ERR_INVALID;
    if (d->ws && (((uintptr_t)d->ws & 15) || d->ws_floats < 0)) return BTS_ERR_INVALID;
    WgradGeom& g = a.g;
    a.x = d->x; a.dy = d->dy; a.out = d->dw;
    g.x_pix_stride = d->x_pix_stride; g.dy_pix_stride = d->dy_pix_stride;
    g.c_in = d->c_in; g.c_out = d->c_out;
    g.B = d->B; g.h_in = d->h_in; g.w_in = d->w_in; g.ups = d->up == 2 ? 1 : 0;
    g.Hs = d->h_in * d->up; g.Ws = d->w_in * d->up;
    g.ksize = d->ksize; g.dil = d->dil; g.stride = d->stride; g.pad = d->pad;
    g.H = (g.Hs + 2 * d->pad - d->dil * (d->ksize - 1) - 1) / d->stride + 1;
    g.W = (g.Ws + 2 * d->pad - d->dil * (d->ksize - 1) - 1) / d->stride + 1;
    if (g.H <= 0 || g.W <= 0) return BTS_ERR_INVALID;
    const double mpix = (double)d->B * g.H * g.W;
    if (mpix >= 4294967296.0 - 65536.0) return BTS_ERR_UNSUPPORTED;
    const double nflat = (double)d->ksize * d->ksize * d->c_in;
    if (nflat >= 2147483648.0) return BTS_ERR_UNSUPPORTED;
    g.M = (unsigned)mpix;
    g.N = d->ksize * d->ksize * d->c_in;
    g.pix_per_split = 0; g.n_ntiles = 0;
    a.pre_scale = d->pre_scale; a.pre_shift = d->pre_shift; a.pre_relu = d->pre_relu;
    if (d->pre_scale && (!d->pre_shift || ((uintptr_t)d->pre_scale & 15) || ((uintptr_t)d->pre_shift & 15))) return BTS_ERR_INVALID;
    a.n_bundles = d->n_bundles > 1 ? d->n_bundles : 1;
    if (d->n_bundles < 0 || a.n_bundles > 65535) return BTS_ERR_INVALID;
    if (d->x_pix_stride < (long)a.n_bundles * d->c_in || d->dy_pix_stride < (long)a.n_bundles * d->c_out) return BTS_ERR_INVALID;
    p = plan_and_settle(a, d->ws_floats, d->ws != nullptr);
    return 0;
}

// Host side of bts_upconv_wgrad_f32, shared with its plan query: validation, kernel arguments, plan_wgrad's tile and
// split for M = B*h*w source pixels, N = 4*c_in, four "bundles" (the classes).  Returns 0 or a BTS_ERR_* code.
int prepare_upconv_wgrad(const float* x, long x_pix_stride, int B, int h, int w, int c_in, const float* dy, long dy_pix_stride,
                         int c_out, const float* dw, const float* ws, long ws_floats, WgradArgs& a, WgradPlan& p) {
    if (!x || !dy || !dw || !ws) return BTS_ERR_INVALID;
    if (B <= 0 || h <= 0 || w <= 0 || c_in <= 0 || c_out <= 0) return BTS_ERR_INVALID;
    if ((c_in & 3) || (c_out & 3)) return BTS_ERR_INVALID;
    if ((x_pix_stride & 3) || x_pix_stride < c_in || (dy_pix_stride & 3) || dy_pix_stride < c_out) return BTS_ERR_INVALID;
    if (((uintptr_t)x & 15) || ((uintptr_t)dy & 15) || ((uintptr_t)dw & 15) || ((uintptr_t)ws & 15) || ws_floats < 0) return BTS_ERR_INVALID;
    const double mpix = (double)B * h * w;
    if (4.0 * mpix >= 2147483648.0 || (double)h * w >= 1073741824.0) return BTS_ERR_UNSUPPORTED;   // 32-bit pixel decode, 2h x 2w rows
    if (36.0 * c_in * (double)c_out >= 2147483648.0) return BTS_ERR_UNSUPPORTED;
    WgradGeom& g = a.g;
    a.x = x; a.dy = dy; a.out = nullptr;
    g.x_pix_stride = x_pix_stride; g.dy_pix_stride = dy_pix_stride;
    g.c_in = c_in; g.c_out = c_out; g.N = 4 * c_in;
    g.B = B; g.h_in = h; g.w_in = w; g.Hs = h; g.Ws = w; g.ups = 0; g.H = h; g.W = w;
    g.ksize = 2; g.dil = 1; g.stride = 1; g.pad = 0;
    g.M = (unsigned)mpix;
    g.pix_per_split = 0; g.n_ntiles = 0;
    a.pre_scale = nullptr; a.pre_shift = nullptr; a.pre_relu = 0;
    a.n_bundles = 4;
    const long per = 16L * c_out * c_in;                   // floats of the four class blocks of one split
    if (ws_floats < per) return BTS_ERR_INVALID;
    p = plan_and_settle(a, ws_floats, true);
    if (p.split * per > ws_floats) return BTS_ERR_INVALID;
    return 0;
}

}  // namespace

extern "C" int bts_conv_wgrad_f32(const bts_conv_wgrad_desc* d, bts_stream_t stream) {
    WgradArgs a;
    WgradPlan p;
    if (const int rc = prepare_wgrad(d, a, p); rc != 0) return rc;
    return for_wgrad_tile(p.variant, [&](auto t) { return launch_wgrad<decltype(t)>(a, p.split, d->dw, d->ws, (hipStream_t)stream); });
}

extern "C" int bts_conv_wgrad_plan_f32(const bts_conv_wgrad_desc* d, int* bm, int* bn, long* split, long* pix_per_split) {
    WgradArgs a;
    WgradPlan p;
    if (const int rc = prepare_wgrad(d, a, p); rc != 0) return rc;
    return report_plan(p, a, bm, bn, split, pix_per_split);
}

// bf16 operands, fp32 accumulation: the descriptor, the checks, the tile, the split and the split sum of bts_conv_wgrad_f32.
extern "C" int bts_conv_wgrad_bf16_f32(const bts_conv_wgrad_desc* d, bts_stream_t stream) {
    WgradArgs a;
    WgradPlan p;
    if (const int rc = prepare_wgrad(d, a, p); rc != 0) return rc;
    return for_wgrad_tile(p.variant, [&](auto t) { return launch_wgrad<decltype(t), true>(a, p.split, d->dw, d->ws, (hipStream_t)stream); });
}

extern "C" int bts_conv_wgrad_bf16_plan_f32(const bts_conv_wgrad_desc* d, int* bm, int* bn, long* split, long* pix_per_split) {
    return bts_conv_wgrad_plan_f32(d, bm, bn, split, pix_per_split);      // no shape class is declined
}

extern "C" int bts_upconv_wgrad_f32(const float* x, long x_pix_stride, int B, int h, int w, int c_in, const float* dy,
                                    long dy_pix_stride, int c_out, float* dw, float* ws, long ws_floats, bts_stream_t stream) {
    WgradArgs a;
    WgradPlan p;
    if (const int rc = prepare_upconv_wgrad(x, x_pix_stride, B, h, w, c_in, dy, dy_pix_stride, c_out, dw, ws, ws_floats, a, p); rc != 0) return rc;
    return for_wgrad_tile(p.variant, [&](auto t) { return launch_upconv_wgrad<decltype(t)>(a, p.split, dw, ws, (hipStream_t)stream); });
}

extern "C" int bts_upconv_wgrad_plan_f32(int B, int h, int w, int c_in, int c_out, long ws_floats, int* bm, int* bn, long* split,
                                         long* pix_per_split) {
    WgradArgs a;
    WgradPlan p;
    const float* dummy = (const float*)(uintptr_t)(1 << 20);      // pointers are checked, never followed
    if (const int rc = prepare_upconv_wgrad(dummy, c_in, B, h, w, c_in, dummy, c_out, c_out, dummy, dummy, ws_floats, a, p); rc != 0) return rc;
    return report_plan(p, a, bm, bn, split, pix_per_split);
}

// ---------------------------------------------------------------------------------------------------------------
// Many problems in one launch (bts_conv_wgrad_batch_*, include/bts_hip.h).  One grid per tile shape covers every problem
// of the batch that uses that tile; a workgroup finds its problem in a device table by its prefix sum of workgroups
// (bts_table_find), derives (tile, split, bundle) from its rank inside the problem and runs wgrad_tile.  The table stores
// (base index, byte offset) for every pointer, the launch receives the base pointers by value: one upload per geometry
// serves every later step.
//
// The batch planner's rule is in this file's header comment.
namespace {

struct WgradBatchEntry {
    long x_off, dy_off, dw_off, sc_off, sh_off;   // byte offsets into their base ranges
    long ws_off;                                   // floats into the batch workspace (split > 1)
    long first_wg;                                 // prefix sum of workgroups over the entries of this tile shape
    long first_red;                                // prefix sum of reduction blocks over the whole table
    int x_base, dy_base, dw_base, sc_base, sh_base;   // sc_base < 0: no prologue
    int tiles, split, n_bundles, pre_relu, variant;
    WgradGeom g;
};

constexpr long WGRAD_BATCH_MAGIC = 0x4254535747424131L;
constexpr int WGRAD_MAX_BASES = 8;

struct WgradBatchHeader {
    long magic;
    int n, n_bases;
    int first[5];          // entries [first[v], first[v+1]) use tile shape v
    int reserved;
    long wgs[4];           // workgroups of each tile shape's grid
    long red_blocks;       // blocks of the reduction launch (0: no problem is split)
    long ws_used;          // floats of the workspace the launch writes
    long reserved2;
};
static_assert(sizeof(WgradBatchHeader) % 16 == 0 && sizeof(WgradBatchEntry) % 8 == 0, "table layout");

struct WgradBases { const char* p[WGRAD_MAX_BASES]; };

__device__ __forceinline__ const char* wgrad_base(const WgradBases& b, int i) {   // uniform selects, no indexed kernarg
    const char* p = b.p[0];
#pragma unroll
    for (int j = 1; j < WGRAD_MAX_BASES; ++j) p = i == j ? b.p[j] : p;
    return p;
}

template <int BM, int BN, int WM, int WN, bool BF16 = false>
__global__ __launch_bounds__(256, 2) void conv_wgrad_batch_kernel(const WgradBatchEntry* __restrict__ table, int n,
                                                                  const WgradBases bases, float* __restrict__ ws) {
    // uniform: read once, into scalar registers
    const WgradBatchEntry& e = table[bts_table_find(table, n, &WgradBatchEntry::first_wg)];
    WgradArgs a;
    a.x = reinterpret_cast<const float*>(wgrad_base(bases, e.x_base) + e.x_off);
    a.dy = reinterpret_cast<const float*>(wgrad_base(bases, e.dy_base) + e.dy_off);
    a.out = e.split > 1 ? ws + e.ws_off
                        : reinterpret_cast<float*>(const_cast<char*>(wgrad_base(bases, e.dw_base)) + e.dw_off);
    a.g = e.g;
    const bool has_pre = e.sc_base >= 0;
    a.pre_scale = has_pre ? reinterpret_cast<const float*>(wgrad_base(bases, e.sc_base) + e.sc_off) : nullptr;
    a.pre_shift = has_pre ? reinterpret_cast<const float*>(wgrad_base(bases, e.sh_base) + e.sh_off) : nullptr;
    a.pre_relu = e.pre_relu;
    a.n_bundles = e.n_bundles;
    const unsigned rank = (unsigned)((long)blockIdx.x - e.first_wg);      // < tiles * split * n_bundles
    const unsigned tile = rank % (unsigned)e.tiles, rest = rank / (unsigned)e.tiles;
    wgrad_tile<BM, BN, WM, WN, false, BF16>(a, tile, rest % (unsigned)e.split, rest / (unsigned)e.split);
}

// wgrad_reduce_kernel for every split problem of a batch in one launch: the block finds its problem in the table
// (unsplit problems own no blocks: the last entry at or below blockIdx.x is never one), then runs the same reduce_block.
__global__ __launch_bounds__(256) void wgrad_reduce_batch_kernel(const WgradBatchEntry* __restrict__ table, int n,
                                                                 const WgradBases bases, const float* __restrict__ ws_all) {
    const WgradBatchEntry& e = table[bts_table_find(table, n, &WgradBatchEntry::first_red)];
    float* dw = reinterpret_cast<float*>(const_cast<char*>(wgrad_base(bases, e.dw_base)) + e.dw_off);
    reduce_block(ws_all + e.ws_off, dw, (long)e.g.c_out * e.g.N * e.n_bundles / 4, e.split, (long)blockIdx.x - e.first_red);
}

// Split of an M-pixel problem at a quantum of qs K-steps, within the single planner's limits and settled as there.
inline WgradSplit wgrad_batch_split(long M, long qs) {
    return wgrad_settle_split(M, std::min((M + qs * WBK - 1) / (qs * WBK), wgrad_max_split(M)));
}

// Byte range [p, p + bytes) inside one of the declared bases: its index and offset.
inline bool wgrad_resolve(const void* p, double bytes, const void* const* bases, const long* base_bytes, int n_bases, int& idx,
                          long& off) {
    const uintptr_t u = (uintptr_t)p;
    for (int j = 0; j < n_bases; ++j) {
        const uintptr_t b = (uintptr_t)bases[j];
        if (u >= b && (double)(u - b) + bytes <= (double)base_bytes[j]) { idx = j; off = (long)(u - b); return true; }
    }
    return false;
}

struct WgradBatchItem { WgradBatchEntry e; int src; long n_it; };      // src: position in the caller's batch; n_it: K-steps a workgroup walks

// Planner step 1: one entry per descriptor -- validated as a single problem, its pointers resolved against the bases, its
// tile chosen by the shape score.  Split, offsets and prefix sums are the later steps'.
int wgrad_batch_describe(const bts_conv_wgrad_desc* descs, int n, const void* const* bases, const long* base_bytes, int n_bases,
                         std::vector<WgradBatchItem>& items) {
    for (int i = 0; i < n; ++i) {
        const bts_conv_wgrad_desc* d = descs + i;
        WgradArgs a;
        WgradPlan p;
        if (const int rc = prepare_wgrad(d, a, p); rc != 0) return rc;
        if (d->ws || d->ws_floats) return BTS_ERR_INVALID;       // the batch has one workspace
        const WgradGeom& g = a.g;
        WgradBatchEntry& e = items[i].e;
        items[i].src = i;
        const double nbx = 4.0 * a.n_bundles * g.c_in, nby = 4.0 * a.n_bundles * g.c_out;
        const double x_bytes = 4.0 * ((double)g.B * g.h_in * g.w_in - 1.0) * (double)g.x_pix_stride + nbx;
        const double dy_bytes = 4.0 * ((double)g.M - 1.0) * (double)g.dy_pix_stride + nby;
        const double dw_bytes = 4.0 * (double)g.c_out * g.N * a.n_bundles;
        if (!wgrad_resolve(d->x, x_bytes, bases, base_bytes, n_bases, e.x_base, e.x_off)) return BTS_ERR_INVALID;
        if (!wgrad_resolve(d->dy, dy_bytes, bases, base_bytes, n_bases, e.dy_base, e.dy_off)) return BTS_ERR_INVALID;
        if (!wgrad_resolve(d->dw, dw_bytes, bases, base_bytes, n_bases, e.dw_base, e.dw_off)) return BTS_ERR_INVALID;
        e.sc_base = e.sh_base = -1; e.sc_off = e.sh_off = 0;
        if (d->pre_scale) {
            if (!wgrad_resolve(d->pre_scale, nbx, bases, base_bytes, n_bases, e.sc_base, e.sc_off)) return BTS_ERR_INVALID;
            if (!wgrad_resolve(d->pre_shift, nbx, bases, base_bytes, n_bases, e.sh_base, e.sh_off)) return BTS_ERR_INVALID;
        }
        e.ws_off = 0; e.first_wg = 0; e.first_red = 0;
        e.g = g;
        e.n_bundles = a.n_bundles; e.pre_relu = d->pre_scale ? a.pre_relu : 0;
        e.variant = wgrad_best_shape_tile(g.c_out, g.N);
        const WgradTileInfo& t = WGRAD_TILES[e.variant];
        e.g.n_ntiles = (g.N + t.bn - 1) / t.bn;
        const long tiles = wgrad_n_tiles(t, g.c_out, g.N);
        if (tiles > 2147483647L) return BTS_ERR_UNSUPPORTED;
        e.tiles = (int)tiles;
    }
    return 0;
}

// Planner step 2: the quantum (in K-steps) of the header comment's `split` and `ws` rules.  Workgroups and partial floats
// of the batch are both non-increasing in qs.
long wgrad_batch_quantum(const std::vector<WgradBatchItem>& items, long ws_floats) {
    long target = 768;                                     // workgroups the batch aims for: plan_wgrad's own target, or
    double tile_ksteps = 0.0;                              // workgroups of ~128 K-steps if the batch has work for more
    long max_m = 1;
    for (const WgradBatchItem& it : items) {
        const WgradBatchEntry& e = it.e;
        max_m = std::max(max_m, (long)e.g.M);
        tile_ksteps += (double)e.tiles * e.n_bundles * (double)(((long)e.g.M + WBK - 1) / WBK);
    }
    if (tile_ksteps / 128.0 > (double)target) target = tile_ksteps / 128.0 < 2147483647.0 ? (long)(tile_ksteps / 128.0) : 2147483647L;

    auto totals = [&](long qs, long& wgs, double& part) {
        wgs = 0; part = 0.0;
        for (const WgradBatchItem& it : items) {
            const WgradBatchEntry& e = it.e;
            const long split = wgrad_batch_split((long)e.g.M, qs).split;
            wgs += (long)e.tiles * e.n_bundles * split;
            if (split > 1) part += (double)split * e.g.c_out * e.g.N * e.n_bundles;
        }
    };
    const long q_all = std::max((max_m + WBK - 1) / WBK, 4L);      // every split is 1 from here on
    long wgs; double part;
    long qs = q_all;
    totals(q_all, wgs, part);
    if (wgs < target) {                                  // the largest quantum that still reaches the target, or 4
        long lo = 4, hi = q_all;                         // invariant: answer in [lo, hi)
        totals(lo, wgs, part);
        if (wgs < target) qs = 4;
        else {
            while (hi - lo > 1) {
                const long mid = lo + (hi - lo) / 2;
                totals(mid, wgs, part);
                if (wgs >= target) lo = mid; else hi = mid;
            }
            qs = lo;
        }
    }
    totals(qs, wgs, part);
    if (part > (double)ws_floats) {                      // the smallest quantum whose partials fit (q_all: none)
        long lo = qs, hi = q_all;                        // part(lo) too large, part(hi) = 0
        while (hi - lo > 1) {
            const long mid = lo + (hi - lo) / 2;
            totals(mid, wgs, part);
            if (part > (double)ws_floats) lo = mid; else hi = mid;
        }
        qs = hi;
    }
    return qs;
}

// Planner step 3: every problem's split at the quantum, the `order` rule, then prefix sums and workspace offsets in that
// order into the table (and the caller's plan, by source position).
int wgrad_batch_layout(std::vector<WgradBatchItem>& items, long qs, int n_bases, long ws_floats, WgradBatchHeader* hdr,
                       WgradBatchEntry* out, bts_conv_wgrad_batch_item* plan) {
    const int n = (int)items.size();
    for (WgradBatchItem& it : items) {
        const WgradSplit s = wgrad_batch_split((long)it.e.g.M, qs);
        it.e.split = (int)s.split; it.e.g.pix_per_split = (unsigned)s.pps;
        it.n_it = (std::min((long)it.e.g.M, s.pps) + WBK - 1) / WBK;
    }
    // tile shape, then longest workgroups first, then shape, then position: a strict total order
    std::sort(items.begin(), items.end(), [](const WgradBatchItem& p, const WgradBatchItem& q) {
        const WgradBatchEntry &a = p.e, &b = q.e;
        if (a.variant != b.variant) return a.variant < b.variant;
        if (p.n_it != q.n_it) return p.n_it > q.n_it;
        if (a.g.M != b.g.M) return a.g.M > b.g.M;
        if (a.g.N != b.g.N) return a.g.N > b.g.N;
        if (a.g.c_out != b.g.c_out) return a.g.c_out > b.g.c_out;
        if (a.n_bundles != b.n_bundles) return a.n_bundles > b.n_bundles;
        return p.src < q.src;
    });

    hdr->magic = WGRAD_BATCH_MAGIC; hdr->n = n; hdr->n_bases = n_bases; hdr->reserved = 0; hdr->reserved2 = 0;
    for (int v = 0; v < 5; ++v) hdr->first[v] = n;
    for (int v = 0; v < 4; ++v) hdr->wgs[v] = 0;
    long red = 0, ws_used = 0;
    for (int r = 0; r < n; ++r) {
        WgradBatchEntry& e = items[r].e;
        if (r < hdr->first[e.variant]) hdr->first[e.variant] = r;
        const long per = (long)e.g.c_out * e.g.N * e.n_bundles;
        e.first_wg = hdr->wgs[e.variant];
        hdr->wgs[e.variant] += (long)e.tiles * e.n_bundles * e.split;
        e.first_red = red;
        if (e.split > 1) {
            e.ws_off = ws_used;
            ws_used += per * e.split;
            red += (per / 4 + 15) / 16;
        }
        out[r] = e;
        if (plan) {
            bts_conv_wgrad_batch_item& it = plan[items[r].src];
            it.bm = WGRAD_TILES[e.variant].bm; it.bn = WGRAD_TILES[e.variant].bn;
            it.split = e.split; it.pix_per_split = (long)e.g.pix_per_split;
            it.ws_offset = e.split > 1 ? e.ws_off : -1;
        }
    }
    for (int v = 3; v >= 0; --v)                          // a shape with no entries starts where the next one does
        if (hdr->first[v] > hdr->first[v + 1]) hdr->first[v] = hdr->first[v + 1];
    hdr->red_blocks = red; hdr->ws_used = ws_used;
    for (int v = 0; v < 4; ++v)
        if (hdr->wgs[v] > 2147483647L) return BTS_ERR_UNSUPPORTED;
    if (red > 2147483647L || ws_used > ws_floats) return BTS_ERR_UNSUPPORTED;
    return 0;
}

}  // namespace

extern "C" long bts_conv_wgrad_batch_table_bytes(int n) {
    if (n < 0) return -1;
    return (long)sizeof(WgradBatchHeader) + (long)n * (long)sizeof(WgradBatchEntry);
}

extern "C" int bts_conv_wgrad_batch_plan_f32(const bts_conv_wgrad_desc* descs, int n, const void* const* bases,
                                             const long* base_bytes, int n_bases, long ws_floats, void* table_host,
                                             bts_conv_wgrad_batch_item* plan) {
    if (n < 0 || n_bases < 0 || n_bases > WGRAD_MAX_BASES || ws_floats < 0 || !table_host) return BTS_ERR_INVALID;
    if (n > 0 && (!descs || n_bases == 0)) return BTS_ERR_INVALID;
    if (n_bases > 0 && (!bases || !base_bytes)) return BTS_ERR_INVALID;
    for (int j = 0; j < n_bases; ++j)
        if (!bases[j] || ((uintptr_t)bases[j] & 15) || base_bytes[j] <= 0) return BTS_ERR_INVALID;
    WgradBatchHeader* hdr = (WgradBatchHeader*)table_host;
    std::vector<WgradBatchItem> items(n);
    if (const int rc = wgrad_batch_describe(descs, n, bases, base_bytes, n_bases, items); rc != 0) return rc;
    return wgrad_batch_layout(items, wgrad_batch_quantum(items, ws_floats), n_bases, ws_floats, hdr, (WgradBatchEntry*)(hdr + 1), plan);
}

namespace {

// Both batch launches: the table's grids with the fp32 or the bf16 tile body, then the one reduction launch.
template <bool BF16>
int launch_wgrad_batch(const void* table_host, const void* table_dev, int n, const void* const* bases, int n_bases, float* ws,
                       bts_stream_t stream) {
    const WgradBatchHeader* hdr = (const WgradBatchHeader*)table_host;
    if (!hdr || hdr->magic != WGRAD_BATCH_MAGIC || hdr->n != n || hdr->n_bases != n_bases || n < 0) return BTS_ERR_INVALID;
    if (n == 0) return 0;
    if (!table_dev || ((uintptr_t)table_dev & 15) || !bases) return BTS_ERR_INVALID;
    if (hdr->ws_used > 0 && (!ws || ((uintptr_t)ws & 15))) return BTS_ERR_INVALID;
    WgradBases b;
    for (int j = 0; j < WGRAD_MAX_BASES; ++j) {
        b.p[j] = j < n_bases ? (const char*)bases[j] : nullptr;
        if (j < n_bases && (!bases[j] || ((uintptr_t)bases[j] & 15))) return BTS_ERR_INVALID;
    }
    const WgradBatchEntry* entries = (const WgradBatchEntry*)((const char*)table_dev + sizeof(WgradBatchHeader));
    hipStream_t s = (hipStream_t)stream;
    for (int v = 0; v < 4; ++v) {
        const int cnt = hdr->first[v + 1] - hdr->first[v];
        if (cnt <= 0 || hdr->wgs[v] <= 0) continue;
        const int rc = for_wgrad_tile(v, [&](auto t) {
            using T = decltype(t);
            const int e = launch_wgrad_tiles<T, conv_wgrad_batch_kernel<T::BM, T::BN, T::WM, T::WN, BF16>, BF16>(
                dim3((unsigned)hdr->wgs[v]), s, entries + hdr->first[v], cnt, b, ws);
            return e != 0 ? e : (int)hipGetLastError();
        });
        if (rc != 0) return rc;
    }
    if (hdr->red_blocks > 0) {
        hipLaunchKernelGGL(wgrad_reduce_batch_kernel, dim3((unsigned)hdr->red_blocks), dim3(256), 0, s, entries, n, b,
                           (const float*)ws);
        return (int)hipGetLastError();
    }
    return 0;
}

}  // namespace

extern "C" int bts_conv_wgrad_batch_f32(const void* table_host, const void* table_dev, int n, const void* const* bases,
                                        int n_bases, float* ws, bts_stream_t stream) {
    return launch_wgrad_batch<false>(table_host, table_dev, n, bases, n_bases, ws, stream);
}

// The same table (bts_conv_wgrad_batch_plan_f32) and the same reduction launch, the tiles with bf16 operands.
extern "C" int bts_conv_wgrad_batch_bf16_f32(const void* table_host, const void* table_dev, int n, const void* const* bases,
                                             int n_bases, float* ws, bts_stream_t stream) {
    return launch_wgrad_batch<true>(table_host, table_dev, n, bases, n_bases, ws, stream);
}
