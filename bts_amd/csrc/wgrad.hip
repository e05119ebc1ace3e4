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
// partials go to a workspace and are summed in a fixed order (deterministic, no atomics); plan_wgrad picks the tile
// (128x128 / 64x128 / 32x128 / 64x64) and the split together.
//
// bts_conv_wgrad_batch_f32 runs many such problems (a DenseNet block's 2*L weight gradients) in one launch per tile
// shape plus one reduction launch; its planner sees the whole batch.
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

namespace {

constexpr int WBK = 32;   // pixels per K-step

struct WgradArgs {
    const float* __restrict__ x;
    const float* __restrict__ dy;
    float* __restrict__ out;     // dw (ksplit == 1) or the partial-sum workspace [ksplit][c_out][N]
    long x_pix_stride, dy_pix_stride;
    int c_in, c_out, N;          // N = taps * c_in
    int B, h_in, w_in, Hs, Ws, ups, H, W, ksize, dil, stride, pad;
    unsigned M;                  // B*H*W output pixels
    unsigned pix_per_split;      // multiple of WBK
    int n_ntiles;
    const float* pre_scale; const float* pre_shift; int pre_relu;   // optional per-input-channel affine (+ReLU) applied to x
                                 // in the gather: the forward convolution saw relu(x*scale + shift) (a folded norm layer)
    int n_bundles;               // grouped convolution as channel bundles (blockIdx.z): bundle j uses input channels
                                 // [j*c_in, ..), gradient channels [j*c_out, ..) and writes dense block j of [c_out][N]
};

// One workgroup = 4 waves arranged WM x WN over a BM x BN tile of dw; each wave owns (BM/WM) x (BN/WN).  The body is
// shared by the single-problem launch (tile / split / bundle = blockIdx.x / .y / .z) and the batched launch (all three
// derived from the workgroup's rank inside its problem).
//
// SUBPIX (bts_upconv_wgrad_f32): the sub-pixel upconv's class gradients.  `bundle` is then the parity class 2*py + px, the
// K axis walks the B*h*w SOURCE pixels (a.H x a.W = a.Hs x a.Ws = the source map), the A operand of pixel (b, Y, X) is
// dy at (b, 2Y+py, 2X+px) of the [B, 2h, 2w] gradient, and the 2x2 taps gather x at (Y-1+py+ty, X-1+px+tx); neither
// operand is offset by the class, and the class results land in dense blocks [split][class][c_out][4*c_in] of a.out.
template <int BM, int BN, int WM, int WN, bool SUBPIX = false>
__device__ __forceinline__ void wgrad_tile(const WgradArgs& a, const unsigned tile, const unsigned split_idx,
                                           const unsigned bundle) {
    static_assert(WM * WN == 4, "4 waves");
    constexpr int TM = BM / WM / 32, TN = BN / WN / 32;
    static_assert(TM >= 1 && TN >= 1, "wave tile must be at least 32x32");
    constexpr int ACOLS = BM / 4, BCOLS = BN / 4;          // float4 columns per tile row
    constexpr int AROWS = 256 / ACOLS, BROWS = 256 / BCOLS;  // rows covered per pass
    constexpr int PA = WBK / AROWS, PB = WBK / BROWS;
    static_assert(PA >= 1 && PB >= 1, "tile too wide for 256 loader threads");

    extern __shared__ __attribute__((aligned(16))) float lds[];
    float* As = lds;                       // [2][WBK][BM]
    float* Bs = lds + 2 * WBK * BM;        // [2][WBK][BN]

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm0 = (wave / WN) * (BM / WM), wn0 = (wave % WN) * (BN / WN);
    const int l31 = lane & 31, khalf = lane >> 5;
    const int tile_n = tile % a.n_ntiles, tile_m = tile / a.n_ntiles;
    const int m0 = tile_m * BM, n0 = tile_n * BN;
    const float* __restrict__ xg = a.x + (SUBPIX ? (size_t)0 : (size_t)bundle * a.c_in);      // this bundle's channel slice
    const float* __restrict__ dyg = a.dy + (SUBPIX ? (size_t)0 : (size_t)bundle * a.c_out);
    [[maybe_unused]] const int cpy = (int)(bundle >> 1), cpx = (int)(bundle & 1);             // SUBPIX: the class parities

    // ---- loader roles (fixed for the whole K walk) ----
    const int a_col = (tid % ACOLS) * 4, a_row = tid / ACOLS;
    const int b_col = (tid % BCOLS) * 4, b_row = tid / BCOLS;
    const bool a_ok = m0 + a_col < a.c_out;                 // c_out % 4 == 0: a float4 is all real or all padding
    const int a_m = a_ok ? m0 + a_col : 0;
    const int n4 = n0 + b_col;
    const bool b_ok = n4 < a.N;
    const int nn = b_ok ? n4 : 0;
    const int tap = nn / a.c_in, ci = nn - tap * a.c_in;    // c_in % 4 == 0: a float4 never straddles a tap
    const int ky = tap / a.ksize, kx = tap - ky * a.ksize;
    const int off_y = SUBPIX ? ky - 1 + cpy : ky * a.dil - a.pad, off_x = SUBPIX ? kx - 1 + cpx : kx * a.dil - a.pad;

    const unsigned k_begin = split_idx * a.pix_per_split;
    const unsigned k_end = min(a.M, k_begin + a.pix_per_split);
    const int n_it = k_begin < k_end ? (int)((k_end - k_begin + WBK - 1) / WBK) : 0;
    const unsigned HW = (unsigned)a.H * (unsigned)a.W;

    // Two staging register sets: the loads of tile it+2 are issued at the top of step it and consumed (written to LDS)
    // at the bottom of step it+1, so every global load has two full MFMA steps to land.
    f32x4 ra0[PA], rb0[PB], ra1[PA], rb1[PB];
    f32x4 psc = {1.f, 1.f, 1.f, 1.f}, psh = {0.f, 0.f, 0.f, 0.f};          // this thread's four input channels never change
    const bool has_pre = a.pre_scale != nullptr;
    if (has_pre) {
        const int cpre = (SUBPIX ? 0 : (int)bundle * a.c_in) + ci;
        psc = *reinterpret_cast<const f32x4*>(a.pre_scale + cpre);
        psh = *reinterpret_cast<const f32x4*>(a.pre_shift + cpre);
    }
    int pb[PB], py[PB], px[PB];             // (frame, row, column) of each gathered row's output pixel at the next step
#pragma unroll
    for (int p = 0; p < PB; ++p) {
        const unsigned pix = k_begin + b_row + p * BROWS;
        const unsigned b = pix / HW, rem = pix - b * HW;
        pb[p] = (int)b;
        py[p] = (int)(rem / (unsigned)a.W);
        px[p] = (int)(rem - (unsigned)py[p] * (unsigned)a.W);
    }
    [[maybe_unused]] int qb[PA], qy[PA], qx[PA];   // SUBPIX: (frame, row, column) of each A row's source pixel at the next step
    if constexpr (SUBPIX) {
#pragma unroll
        for (int p = 0; p < PA; ++p) {
            const unsigned pix = k_begin + a_row + p * AROWS;
            const unsigned b = pix / HW, rem = pix - b * HW;
            qb[p] = (int)b;
            qy[p] = (int)(rem / (unsigned)a.W);
            qx[p] = (int)(rem - (unsigned)qy[p] * (unsigned)a.W);
        }
    }
    auto issue = [&](int it, f32x4 (&ra)[PA], f32x4 (&rb)[PB]) __attribute__((always_inline)) {
        const unsigned base = k_begin + (unsigned)it * WBK;
#pragma unroll
        for (int p = 0; p < PA; ++p) {
            const unsigned pix = base + a_row + p * AROWS;
            const bool ok = a_ok && pix < k_end;
            size_t row = ok ? pix : 0u;
            if constexpr (SUBPIX) {                                      // dy lives at (2Y+py, 2X+px) of the [B,2h,2w] map
                row = ok ? ((size_t)qb[p] * (2 * a.H) + (size_t)(2 * qy[p] + cpy)) * (size_t)(2 * a.W) + (size_t)(2 * qx[p] + cpx) : 0;
                qx[p] += WBK;
                while (qx[p] >= a.W) { qx[p] -= a.W; ++qy[p]; }
                while (qy[p] >= a.H) { qy[p] -= a.H; ++qb[p]; }
            }
            const float* src = dyg + row * a.dy_pix_stride + a_m;
            f32x4 v = *reinterpret_cast<const f32x4*>(src);
            ra[p] = ok ? v : (f32x4)(0.f);
        }
#pragma unroll
        for (int p = 0; p < PB; ++p) {
            const unsigned pix = base + b_row + p * BROWS;
            const int iy = py[p] * a.stride + off_y, ix = px[p] * a.stride + off_x;
            const bool ok = b_ok && pix < k_end && iy >= 0 && iy < a.Hs && ix >= 0 && ix < a.Ws;
            const int sb = ok ? pb[p] : 0, sy = ok ? (iy >> a.ups) : 0, sx = ok ? (ix >> a.ups) : 0;
            const float* src = xg + ((size_t)(sb * a.h_in + sy) * a.w_in + sx) * a.x_pix_stride + ci;
            f32x4 v = *reinterpret_cast<const f32x4*>(src);
            if (has_pre) {
                v = v * psc + psh;
                if (a.pre_relu) v = __builtin_elementwise_max(v, (f32x4)(0.f));
            }
            rb[p] = ok ? v : (f32x4)(0.f);                               // zero padding AFTER the prologue
            // advance this row's output pixel by one K-step without dividing (issue() is called for it = 0, 1, 2, ...)
            px[p] += WBK;
            while (px[p] >= a.W) { px[p] -= a.W; ++py[p]; }
            while (py[p] >= a.H) { py[p] -= a.H; ++pb[p]; }
        }
    };
    auto stage = [&](int buf, const f32x4 (&ra)[PA], const f32x4 (&rb)[PB]) __attribute__((always_inline)) {
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
    float* out = a.out + ((size_t)split_idx * a.n_bundles + bundle) * a.c_out * a.N;
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j) {
            const int n = n0 + wn0 + 32 * j + l31;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int m = m0 + wm0 + 32 * i + (r & 3) + 8 * (r >> 2) + 4 * khalf;
                if (m < a.c_out && n < a.N) out[(size_t)m * a.N + n] = acc[i][j][r];
            }
        }
}

template <int BM, int BN, int WM, int WN>
__global__ __launch_bounds__(256, 2) void conv_wgrad_kernel(const WgradArgs a) {
    wgrad_tile<BM, BN, WM, WN>(a, blockIdx.x, blockIdx.y, blockIdx.z);
}

// Sum the ksplit partial tiles in a fixed order.  The output is small and the split count can be in the hundreds, so
// the walk over splits is itself spread over 16 lanes per element (a serial walk is pure load latency): a block owns
// 16 consecutive float4 elements, lane j adds splits j, j+16, ... (four independent loads in flight), then lane 0 adds
// the 16 lane sums in order.
__global__ __launch_bounds__(256) void wgrad_reduce_kernel(const float* __restrict__ ws, float* __restrict__ dw,
                                                           long count4, int ksplit) {
    const int el = threadIdx.x & 15, lane = threadIdx.x >> 4;
    const long t = (long)blockIdx.x * 16 + el;
    const long tt = t < count4 ? t : count4 - 1;
    const f32x4* p = reinterpret_cast<const f32x4*>(ws) + tt;
    f32x4 v = (f32x4)(0.f);
    int s = lane;
    for (; s + 48 < ksplit; s += 64) {
        const f32x4 a0 = p[(size_t)s * count4], a1 = p[(size_t)(s + 16) * count4];
        const f32x4 a2 = p[(size_t)(s + 32) * count4], a3 = p[(size_t)(s + 48) * count4];
        v += (a0 + a1) + (a2 + a3);
    }
    for (; s < ksplit; s += 16) v += p[(size_t)s * count4];
    __shared__ f32x4 red[16][16];
    red[lane][el] = v;
    __syncthreads();
    if (lane == 0 && t < count4) {
        f32x4 r = red[0][el];
#pragma unroll
        for (int j = 1; j < 16; ++j) r += red[j][el];
        reinterpret_cast<f32x4*>(dw)[t] = r;
    }
}

// `a` and `split` come from prepare_wgrad: a.pix_per_split and the split count are final here.
template <int BM, int BN, int WM, int WN>
int launch_wgrad(WgradArgs a, long split, float* dw, float* ws, hipStream_t s) {
    const int m_tiles = (a.c_out + BM - 1) / BM;
    a.n_ntiles = (a.N + BN - 1) / BN;
    const long tiles = (long)m_tiles * a.n_ntiles;
    const long per = (long)a.c_out * a.N * a.n_bundles;
    a.out = split > 1 ? ws : dw;
    const size_t lds_bytes = (size_t)2 * WBK * (BM + BN) * sizeof(float);
    auto kern = conv_wgrad_kernel<BM, BN, WM, WN>;
    static std::atomic<unsigned long long> lds_set{0};     // per instantiation: one bit per device (common.h)
    if (hipError_t e = bts_ensure_dynamic_lds((const void*)kern, lds_bytes, lds_set); e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(kern, dim3((unsigned)tiles, (unsigned)split, (unsigned)a.n_bundles), dim3(256), lds_bytes, s, a);
    if (split > 1) {
        const long count4 = per / 4;      // N % 4 == 0
        hipLaunchKernelGGL(wgrad_reduce_kernel, dim3((unsigned)((count4 + 15) / 16)), dim3(256), 0, s, ws, dw, count4,
                           (int)split);
    }
    return (int)hipGetLastError();
}

// Tile + split plan.  The output (c_out x taps*c_in) is small and the pixel axis long, so parallelism comes from
// splitting pixels; every split costs one partial tile written and re-read.  Candidates are scored by
//   useful fraction of the padded tile grid  x  per-tile efficiency  x  chip fill (workgroups / 512, capped at 1)
//   x  operand bytes / (operand bytes + partial-tile bytes)
// with the split chosen to reach ~768 workgroups within [>= 4 K-steps per split, <= 1024 splits, workspace size].
struct WgradPlan { int variant; long split; };
constexpr int WGRAD_BM[4] = {128, 64, 32, 64}, WGRAD_BN[4] = {128, 128, 128, 64};   // tile of WgradPlan::variant

inline WgradPlan plan_wgrad(int c_out, int N, long M, long ws_floats, bool have_ws, int n_bundles) {
    const int* bm = WGRAD_BM;
    const int* bn = WGRAD_BN;
    static const double eff[4] = {1.0, 0.9, 0.75, 0.8};
    constexpr long target = 768;                                       // workgroups a split aims for (see above)
    const long per = (long)c_out * N * n_bundles;
    long max_split = M / (4 * WBK);
    if (max_split > 1024) max_split = 1024;
    if (!have_ws || ws_floats < 2 * per) max_split = 1;
    else if (max_split * per > ws_floats) max_split = ws_floats / per;
    if (max_split < 1) max_split = 1;
    const double in_bytes = 4.0 * (double)M * (c_out + N);           // operands read once (taps re-read from cache)
    WgradPlan best = {0, 1};
    double best_score = -1.0;
    for (int v = 0; v < 4; ++v) {
        const long mt = (c_out + bm[v] - 1) / bm[v], nt = (N + bn[v] - 1) / bn[v];
        const long tiles = mt * nt * n_bundles;
        long split = (target + tiles - 1) / tiles;
        if (split > max_split) split = max_split;
        const double useful = (double)c_out * N / ((double)mt * bm[v] * nt * bn[v]);
        double fill = (double)(tiles * split) / 512.0;
        if (fill > 1.0) fill = 1.0;
        const double partial_bytes = split > 1 ? 8.0 * (double)split * (double)per : 0.0;   // written once, read once
        const double score = useful * eff[v] * fill * in_bytes / (in_bytes + partial_bytes);
        if (score > best_score * 1.0001) { best_score = score; best = {v, split}; }
    }
    return best;
}

// Everything bts_conv_wgrad_f32 decides on the host, shared with the plan query (no GPU work): validates the
// descriptor, fills the kernel arguments (a.out / a.n_ntiles are the launch's), picks the tile and settles the split.
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
    a.x = d->x; a.dy = d->dy; a.out = d->dw;
    a.x_pix_stride = d->x_pix_stride; a.dy_pix_stride = d->dy_pix_stride;
    a.c_in = d->c_in; a.c_out = d->c_out;
    a.B = d->B; a.h_in = d->h_in; a.w_in = d->w_in; a.ups = d->up == 2 ? 1 : 0;
    a.Hs = d->h_in * d->up; a.Ws = d->w_in * d->up;
    a.ksize = d->ksize; a.dil = d->dil; a.stride = d->stride; a.pad = d->pad;
    a.H = (a.Hs + 2 * d->pad - d->dil * (d->ksize - 1) - 1) / d->stride + 1;
    a.W = (a.Ws + 2 * d->pad - d->dil * (d->ksize - 1) - 1) / d->stride + 1;
    if (a.H <= 0 || a.W <= 0) return BTS_ERR_INVALID;
    const double mpix = (double)d->B * a.H * a.W;
    if (mpix >= 4294967296.0 - 65536.0) return BTS_ERR_UNSUPPORTED;
    const double nflat = (double)d->ksize * d->ksize * d->c_in;
    if (nflat >= 2147483648.0) return BTS_ERR_UNSUPPORTED;
    a.M = (unsigned)mpix;
    a.N = d->ksize * d->ksize * d->c_in;
    a.pix_per_split = 0; a.n_ntiles = 0;
    a.pre_scale = d->pre_scale; a.pre_shift = d->pre_shift; a.pre_relu = d->pre_relu;
    if (d->pre_scale && (!d->pre_shift || ((uintptr_t)d->pre_scale & 15) || ((uintptr_t)d->pre_shift & 15))) return BTS_ERR_INVALID;
    a.n_bundles = d->n_bundles > 1 ? d->n_bundles : 1;
    if (d->n_bundles < 0 || a.n_bundles > 65535) return BTS_ERR_INVALID;
    if (d->x_pix_stride < (long)a.n_bundles * d->c_in || d->dy_pix_stride < (long)a.n_bundles * d->c_out) return BTS_ERR_INVALID;
    p = plan_wgrad(d->c_out, a.N, (long)a.M, d->ws_floats, d->ws != nullptr, a.n_bundles);
    const long pps = (((long)a.M + p.split - 1) / p.split + WBK - 1) / WBK * WBK;
    p.split = ((long)a.M + pps - 1) / pps;                       // no empty splits
    a.pix_per_split = (unsigned)pps;
    return 0;
}

}  // namespace

extern "C" int bts_conv_wgrad_f32(const bts_conv_wgrad_desc* d, bts_stream_t stream) {
    WgradArgs a;
    WgradPlan p;
    if (const int rc = prepare_wgrad(d, a, p); rc != 0) return rc;
    hipStream_t s = (hipStream_t)stream;
    switch (p.variant) {
        case 0: return launch_wgrad<128, 128, 2, 2>(a, p.split, d->dw, d->ws, s);
        case 1: return launch_wgrad<64, 128, 1, 4>(a, p.split, d->dw, d->ws, s);
        case 2: return launch_wgrad<32, 128, 1, 4>(a, p.split, d->dw, d->ws, s);
        default: return launch_wgrad<64, 64, 2, 2>(a, p.split, d->dw, d->ws, s);
    }
}

extern "C" int bts_conv_wgrad_plan_f32(const bts_conv_wgrad_desc* d, int* bm, int* bn, long* split, long* pix_per_split) {
    WgradArgs a;
    WgradPlan p;
    if (const int rc = prepare_wgrad(d, a, p); rc != 0) return rc;
    if (bm) *bm = WGRAD_BM[p.variant];
    if (bn) *bn = WGRAD_BN[p.variant];
    if (split) *split = p.split;
    if (pix_per_split) *pix_per_split = (long)a.pix_per_split;
    return 0;
}

// ---------------------------------------------------------------------------------------------------------------
// Many problems in one launch (bts_conv_wgrad_batch_*, include/bts_hip.h).  One grid per tile shape covers every problem
// of the batch that uses that tile; a workgroup finds its problem by binary search over a prefix sum of workgroups in a
// device table (the way pack_weights_kernel finds its entry), derives (tile, split, bundle) from its rank inside the
// problem and runs wgrad_tile.  The table stores (base index, byte offset) for every pointer, the launch receives the
// base pointers by value: one upload per geometry serves every later step.
//
// The batch planner's rule is in this file's header comment.
namespace {

struct WgradBatchEntry {
    long x_off, dy_off, dw_off, sc_off, sh_off;   // byte offsets into their base ranges
    long ws_off;                                   // floats into the batch workspace (split > 1)
    long x_pix_stride, dy_pix_stride;
    long first_wg;                                 // prefix sum of workgroups over the entries of this tile shape
    long first_red;                                // prefix sum of reduction blocks over the whole table
    int x_base, dy_base, dw_base, sc_base, sh_base;   // sc_base < 0: no prologue
    int c_in, c_out, N, B, h_in, w_in, Hs, Ws, ups, H, W, ksize, dil, stride, pad;
    unsigned M, pix_per_split;
    int n_ntiles, tiles, split, n_bundles, pre_relu, variant;
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

template <int BM, int BN, int WM, int WN>
__global__ __launch_bounds__(256, 2) void conv_wgrad_batch_kernel(const WgradBatchEntry* __restrict__ table, int n,
                                                                  const WgradBases bases, float* __restrict__ ws) {
    int lo = 0, hi = n - 1;                       // the entry whose workgroup range holds blockIdx.x
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (table[mid].first_wg <= (long)blockIdx.x) lo = mid; else hi = mid - 1;
    }
    const WgradBatchEntry& e = table[lo];         // uniform: read once, into scalar registers
    WgradArgs a;
    a.x = reinterpret_cast<const float*>(wgrad_base(bases, e.x_base) + e.x_off);
    a.dy = reinterpret_cast<const float*>(wgrad_base(bases, e.dy_base) + e.dy_off);
    a.out = e.split > 1 ? ws + e.ws_off
                        : reinterpret_cast<float*>(const_cast<char*>(wgrad_base(bases, e.dw_base)) + e.dw_off);
    a.x_pix_stride = e.x_pix_stride; a.dy_pix_stride = e.dy_pix_stride;
    a.c_in = e.c_in; a.c_out = e.c_out; a.N = e.N;
    a.B = e.B; a.h_in = e.h_in; a.w_in = e.w_in; a.Hs = e.Hs; a.Ws = e.Ws; a.ups = e.ups; a.H = e.H; a.W = e.W;
    a.ksize = e.ksize; a.dil = e.dil; a.stride = e.stride; a.pad = e.pad;
    a.M = e.M; a.pix_per_split = e.pix_per_split; a.n_ntiles = e.n_ntiles;
    const bool has_pre = e.sc_base >= 0;
    a.pre_scale = has_pre ? reinterpret_cast<const float*>(wgrad_base(bases, e.sc_base) + e.sc_off) : nullptr;
    a.pre_shift = has_pre ? reinterpret_cast<const float*>(wgrad_base(bases, e.sh_base) + e.sh_off) : nullptr;
    a.pre_relu = e.pre_relu;
    a.n_bundles = e.n_bundles;
    const unsigned rank = (unsigned)((long)blockIdx.x - e.first_wg);      // < tiles * split * n_bundles
    const unsigned tile = rank % (unsigned)e.tiles, rest = rank / (unsigned)e.tiles;
    wgrad_tile<BM, BN, WM, WN>(a, tile, rest % (unsigned)e.split, rest / (unsigned)e.split);
}

// wgrad_reduce_kernel for every split problem of a batch in one launch: the block finds its problem in the table, then
// sums exactly as wgrad_reduce_kernel does (lane j adds splits j, j+16, ..., then the 16 lane sums in order).
__global__ __launch_bounds__(256) void wgrad_reduce_batch_kernel(const WgradBatchEntry* __restrict__ table, int n,
                                                                 const WgradBases bases, const float* __restrict__ ws_all) {
    int lo = 0, hi = n - 1;      // unsplit problems own no blocks: the last entry at or below blockIdx.x is never one
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (table[mid].first_red <= (long)blockIdx.x) lo = mid; else hi = mid - 1;
    }
    const WgradBatchEntry& e = table[lo];
    const long count4 = (long)e.c_out * e.N * e.n_bundles / 4;
    const int ksplit = e.split;
    const float* ws = ws_all + e.ws_off;
    float* dw = reinterpret_cast<float*>(const_cast<char*>(wgrad_base(bases, e.dw_base)) + e.dw_off);
    const int el = threadIdx.x & 15, lane = threadIdx.x >> 4;
    const long t = ((long)blockIdx.x - e.first_red) * 16 + el;
    const long tt = t < count4 ? t : count4 - 1;
    const f32x4* p = reinterpret_cast<const f32x4*>(ws) + tt;
    f32x4 v = (f32x4)(0.f);
    int s = lane;
    for (; s + 48 < ksplit; s += 64) {
        const f32x4 a0 = p[(size_t)s * count4], a1 = p[(size_t)(s + 16) * count4];
        const f32x4 a2 = p[(size_t)(s + 32) * count4], a3 = p[(size_t)(s + 48) * count4];
        v += (a0 + a1) + (a2 + a3);
    }
    for (; s < ksplit; s += 16) v += p[(size_t)s * count4];
    __shared__ f32x4 red[16][16];
    red[lane][el] = v;
    __syncthreads();
    if (lane == 0 && t < count4) {
        f32x4 r = red[0][el];
#pragma unroll
        for (int j = 1; j < 16; ++j) r += red[j][el];
        reinterpret_cast<f32x4*>(dw)[t] = r;
    }
}

template <int BM, int BN, int WM, int WN>
int launch_wgrad_batch(const WgradBatchEntry* entries, int n, long wgs, const WgradBases& bases, float* ws, hipStream_t s) {
    const size_t lds_bytes = (size_t)2 * WBK * (BM + BN) * sizeof(float);
    auto kern = conv_wgrad_batch_kernel<BM, BN, WM, WN>;
    static std::atomic<unsigned long long> lds_set{0};     // per instantiation: one bit per device (common.h)
    if (hipError_t e = bts_ensure_dynamic_lds((const void*)kern, lds_bytes, lds_set); e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(kern, dim3((unsigned)wgs), dim3(256), lds_bytes, s, entries, n, bases, ws);
    return (int)hipGetLastError();
}

// The tile of one problem inside a batch: the single planner's shape terms (see the rule above).
inline int wgrad_batch_variant(int c_out, int N) {
    static const double eff[4] = {1.0, 0.9, 0.75, 0.8};
    int best = 0;
    double best_score = -1.0;
    for (int v = 0; v < 4; ++v) {
        const long mt = (c_out + WGRAD_BM[v] - 1) / WGRAD_BM[v], nt = (N + WGRAD_BN[v] - 1) / WGRAD_BN[v];
        const double useful = (double)c_out * N / ((double)mt * WGRAD_BM[v] * nt * WGRAD_BN[v]);
        const double score = useful * eff[v];
        if (score > best_score * 1.0001) { best_score = score; best = v; }
    }
    return best;
}

// Split of an M-pixel problem at a quantum of qs K-steps, settled as prepare_wgrad settles it.
inline void wgrad_batch_split(long M, long qs, long& split, long& pps) {
    long max_split = M / (4 * WBK);
    if (max_split > 1024) max_split = 1024;
    if (max_split < 1) max_split = 1;
    split = (M + qs * WBK - 1) / (qs * WBK);
    if (split > max_split) split = max_split;
    pps = ((M + split - 1) / split + WBK - 1) / WBK * WBK;
    split = (M + pps - 1) / pps;
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
    WgradBatchEntry* out = (WgradBatchEntry*)(hdr + 1);
    long target = 768;                                     // workgroups the batch aims for: plan_wgrad's own target, or
    double tile_ksteps = 0.0;                              // workgroups of ~128 K-steps if the batch has work for more

    struct Item { WgradBatchEntry e; int src; long n_it; };
    Item* items = n > 0 ? new Item[n] : nullptr;
    struct Free { Item* p; ~Free() { delete[] p; } } free_items{items};
    long max_m = 1;
    for (int i = 0; i < n; ++i) {
        const bts_conv_wgrad_desc* d = descs + i;
        WgradArgs a;
        WgradPlan p;
        if (const int rc = prepare_wgrad(d, a, p); rc != 0) return rc;
        if (d->ws || d->ws_floats) return BTS_ERR_INVALID;       // the batch has one workspace
        WgradBatchEntry& e = items[i].e;
        items[i].src = i;
        const double nbx = 4.0 * a.n_bundles * a.c_in, nby = 4.0 * a.n_bundles * a.c_out;
        const double x_bytes = 4.0 * ((double)a.B * a.h_in * a.w_in - 1.0) * (double)a.x_pix_stride + nbx;
        const double dy_bytes = 4.0 * ((double)a.M - 1.0) * (double)a.dy_pix_stride + nby;
        const double dw_bytes = 4.0 * (double)a.c_out * a.N * a.n_bundles;
        if (!wgrad_resolve(d->x, x_bytes, bases, base_bytes, n_bases, e.x_base, e.x_off)) return BTS_ERR_INVALID;
        if (!wgrad_resolve(d->dy, dy_bytes, bases, base_bytes, n_bases, e.dy_base, e.dy_off)) return BTS_ERR_INVALID;
        if (!wgrad_resolve(d->dw, dw_bytes, bases, base_bytes, n_bases, e.dw_base, e.dw_off)) return BTS_ERR_INVALID;
        e.sc_base = e.sh_base = -1; e.sc_off = e.sh_off = 0;
        if (d->pre_scale) {
            if (!wgrad_resolve(d->pre_scale, nbx, bases, base_bytes, n_bases, e.sc_base, e.sc_off)) return BTS_ERR_INVALID;
            if (!wgrad_resolve(d->pre_shift, nbx, bases, base_bytes, n_bases, e.sh_base, e.sh_off)) return BTS_ERR_INVALID;
        }
        e.ws_off = 0; e.first_wg = 0; e.first_red = 0;
        e.x_pix_stride = a.x_pix_stride; e.dy_pix_stride = a.dy_pix_stride;
        e.c_in = a.c_in; e.c_out = a.c_out; e.N = a.N; e.B = a.B; e.h_in = a.h_in; e.w_in = a.w_in; e.Hs = a.Hs; e.Ws = a.Ws;
        e.ups = a.ups; e.H = a.H; e.W = a.W; e.ksize = a.ksize; e.dil = a.dil; e.stride = a.stride; e.pad = a.pad;
        e.M = a.M; e.n_bundles = a.n_bundles; e.pre_relu = d->pre_scale ? a.pre_relu : 0;
        e.variant = wgrad_batch_variant(a.c_out, a.N);
        e.n_ntiles = (a.N + WGRAD_BN[e.variant] - 1) / WGRAD_BN[e.variant];
        const long tiles = (long)((a.c_out + WGRAD_BM[e.variant] - 1) / WGRAD_BM[e.variant]) * e.n_ntiles;
        if (tiles > 2147483647L) return BTS_ERR_UNSUPPORTED;
        e.tiles = (int)tiles;
        if ((long)a.M > max_m) max_m = (long)a.M;
        tile_ksteps += (double)tiles * a.n_bundles * (double)(((long)a.M + WBK - 1) / WBK);
    }
    if (tile_ksteps / 128.0 > (double)target) target = tile_ksteps / 128.0 < 2147483647.0 ? (long)(tile_ksteps / 128.0) : 2147483647L;

    // ---- the quantum: workgroups and partial floats of the batch are both non-increasing in qs ----
    auto totals = [&](long qs, long& wgs, double& part) {
        wgs = 0; part = 0.0;
        for (int i = 0; i < n; ++i) {
            const WgradBatchEntry& e = items[i].e;
            long split, pps;
            wgrad_batch_split((long)e.M, qs, split, pps);
            wgs += (long)e.tiles * e.n_bundles * split;
            if (split > 1) part += (double)split * e.c_out * e.N * e.n_bundles;
        }
    };
    const long q_all = (max_m + WBK - 1) / WBK < 4 ? 4 : (max_m + WBK - 1) / WBK;      // every split is 1 from here on
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

    for (int i = 0; i < n; ++i) {
        WgradBatchEntry& e = items[i].e;
        long split, pps;
        wgrad_batch_split((long)e.M, qs, split, pps);
        e.split = (int)split; e.pix_per_split = (unsigned)pps;
        const long own = (long)e.M < pps ? (long)e.M : pps;
        items[i].n_it = (own + WBK - 1) / WBK;
    }
    // tile shape, then longest workgroups first, then shape, then position (stable: std::sort is not needed for n this small)
    auto before = [](const Item& p, const Item& q) {
        const WgradBatchEntry &a = p.e, &b = q.e;
        if (a.variant != b.variant) return a.variant < b.variant;
        if (p.n_it != q.n_it) return p.n_it > q.n_it;
        if (a.M != b.M) return a.M > b.M;
        if (a.N != b.N) return a.N > b.N;
        if (a.c_out != b.c_out) return a.c_out > b.c_out;
        if (a.n_bundles != b.n_bundles) return a.n_bundles > b.n_bundles;
        return p.src < q.src;
    };
    int* order = n > 0 ? new int[n] : nullptr;
    struct FreeI { int* p; ~FreeI() { delete[] p; } } free_order{order};
    for (int i = 0; i < n; ++i) order[i] = i;
    for (int i = 1; i < n; ++i) {                        // insertion sort
        const int k = order[i];
        int j = i - 1;
        while (j >= 0 && before(items[k], items[order[j]])) { order[j + 1] = order[j]; --j; }
        order[j + 1] = k;
    }

    hdr->magic = WGRAD_BATCH_MAGIC; hdr->n = n; hdr->n_bases = n_bases; hdr->reserved = 0; hdr->reserved2 = 0;
    for (int v = 0; v < 5; ++v) hdr->first[v] = n;
    for (int v = 0; v < 4; ++v) hdr->wgs[v] = 0;
    long red = 0, ws_used = 0;
    for (int r = 0; r < n; ++r) {
        WgradBatchEntry& e = items[order[r]].e;
        if (r < hdr->first[e.variant]) hdr->first[e.variant] = r;
        const long per = (long)e.c_out * e.N * e.n_bundles;
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
            bts_conv_wgrad_batch_item& it = plan[order[r]];
            it.bm = WGRAD_BM[e.variant]; it.bn = WGRAD_BN[e.variant];
            it.split = e.split; it.pix_per_split = (long)e.pix_per_split;
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

extern "C" int bts_conv_wgrad_batch_f32(const void* table_host, const void* table_dev, int n, const void* const* bases,
                                        int n_bases, float* ws, bts_stream_t stream) {
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
        const WgradBatchEntry* ev = entries + hdr->first[v];
        int rc;
        switch (v) {
            case 0: rc = launch_wgrad_batch<128, 128, 2, 2>(ev, cnt, hdr->wgs[v], b, ws, s); break;
            case 1: rc = launch_wgrad_batch<64, 128, 1, 4>(ev, cnt, hdr->wgs[v], b, ws, s); break;
            case 2: rc = launch_wgrad_batch<32, 128, 1, 4>(ev, cnt, hdr->wgs[v], b, ws, s); break;
            default: rc = launch_wgrad_batch<64, 64, 2, 2>(ev, cnt, hdr->wgs[v], b, ws, s); break;
        }
        if (rc != 0) return rc;
    }
    if (hdr->red_blocks > 0) {
        hipLaunchKernelGGL(wgrad_reduce_batch_kernel, dim3((unsigned)hdr->red_blocks), dim3(256), 0, s, entries, n, b,
                           (const float*)ws);
        return (int)hipGetLastError();
    }
    return 0;
}

// ---------------------------------------------------------------------------------------------------------------
// Batched weight packing for the training step: every step the optimiser rewrites the OIHW parameters, and both the
// forward kernel ([c_out_pad][k_pad], K = tap*c_in_ld + c) and the input-gradient pass (the same layout of the
// flipped, transposed kernel) need them re-laid.  One launch re-packs every registered weight from a device table.
namespace {

struct PackEntry {          // 12 x int64, filled by the host (bts_amd/train.py)
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
                            // channel, inner = output channel); entries outside a row's own group are zero.  0 = dense
};

constexpr int PACK_PER_BLOCK = 256 * 4 * 4;

__global__ __launch_bounds__(256) void pack_weights_kernel(const PackEntry* __restrict__ table, int n) {
    int lo = 0, hi = n - 1;                       // the entry whose block range holds blockIdx.x
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (table[mid].first_block <= (long)blockIdx.x) lo = mid; else hi = mid - 1;
    }
    const PackEntry e = table[lo];
    const long total = e.rows_pad * e.k_pad;
    const long base = ((long)blockIdx.x - e.first_block) * PACK_PER_BLOCK;
    const long kk2 = e.k * e.k;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const long i0 = base + ((long)u * 256 + threadIdx.x) * 4;
        if (i0 >= total) continue;
        const long row = i0 / e.k_pad, col0 = i0 - row * e.k_pad;
        f32x4 v = (f32x4)(0.f);
        if (row < e.rows) {
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
// Sub-pixel upconv in the training step (bts_upconv_wgrad_f32, bts_upconv_train_pack_f32; include/bts_hip.h).
//
// Weight gradient: per parity class (py, px) the 2x2 class filter's gradient is a [c_out] x [4*c_in] GEMM over the B*h*w
// source pixels -- wgrad_tile<SUBPIX> with the class as gridDim.z -- written as [split][class][c_out][4*c_in] into the
// caller's workspace (split >= 1: the class results need a home even unsplit).  upconv_wgrad_fold_kernel then produces
// dw[co][3*ky+kx][ci] in a FIXED order:
//   1. per class cls = 0..3, the split partials of element (co, tau_py(ky)*2 + tau_px(kx), ci) exactly as
//      wgrad_reduce_kernel sums them (lane j adds splits j, j+16, ..., four at a time as (a0+a1)+(a2+a3); then the 16
//      lane sums are added in lane order) -> r_cls;
//   2. dw = ((r_0 + r_1) + r_2) + r_3.
// tau_0 = (0,1,1), tau_1 = (0,0,1): the adjoint of the pre-sum in pack_upconv_subpixel.  No atomics; bit-reproducible.
namespace {

template <int BM, int BN, int WM, int WN>
__global__ __launch_bounds__(256, 2) void upconv_wgrad_kernel(const WgradArgs a) {
    wgrad_tile<BM, BN, WM, WN, true>(a, blockIdx.x, blockIdx.y, blockIdx.z);
}

__global__ __launch_bounds__(256) void upconv_wgrad_fold_kernel(const float* __restrict__ ws, float* __restrict__ dw, int c_out,
                                                                int c_in, int ksplit) {
    const long count4 = (long)c_out * 9 * c_in / 4;
    const long per = (long)c_out * 4 * c_in;               // floats of one class block
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
        const size_t step = (size_t)4 * per;               // one split = four class blocks
        f32x4 v = (f32x4)(0.f);
        int s = lane;
        for (; s + 48 < ksplit; s += 64) {
            const f32x4 a0 = *reinterpret_cast<const f32x4*>(p + (size_t)s * step), a1 = *reinterpret_cast<const f32x4*>(p + (size_t)(s + 16) * step);
            const f32x4 a2 = *reinterpret_cast<const f32x4*>(p + (size_t)(s + 32) * step), a3 = *reinterpret_cast<const f32x4*>(p + (size_t)(s + 48) * step);
            v += (a0 + a1) + (a2 + a3);
        }
        for (; s < ksplit; s += 16) v += *reinterpret_cast<const f32x4*>(p + (size_t)s * step);
        red[cls][lane][el] = v;
    }
    __syncthreads();
    if (lane == 0 && t < count4) {
        f32x4 r[4];
#pragma unroll
        for (int cls = 0; cls < 4; ++cls) {
            r[cls] = red[cls][0][el];
#pragma unroll
            for (int j = 1; j < 16; ++j) r[cls] += red[cls][j][el];
        }
        reinterpret_cast<f32x4*>(dw)[t] = ((r[0] + r[1]) + r[2]) + r[3];
    }
}

template <int BM, int BN, int WM, int WN>
int launch_upconv_wgrad(WgradArgs a, long split, float* dw, float* ws, hipStream_t s) {
    const int m_tiles = (a.c_out + BM - 1) / BM;
    a.n_ntiles = (a.N + BN - 1) / BN;
    const long tiles = (long)m_tiles * a.n_ntiles;
    a.out = ws;
    const size_t lds_bytes = (size_t)2 * WBK * (BM + BN) * sizeof(float);
    auto kern = upconv_wgrad_kernel<BM, BN, WM, WN>;
    static std::atomic<unsigned long long> lds_set{0};     // per instantiation: one bit per device (common.h)
    if (hipError_t e = bts_ensure_dynamic_lds((const void*)kern, lds_bytes, lds_set); e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(kern, dim3((unsigned)tiles, (unsigned)split, 4u), dim3(256), lds_bytes, s, a);
    const long count4 = (long)a.c_out * 9 * a.c_in / 4;
    hipLaunchKernelGGL(upconv_wgrad_fold_kernel, dim3((unsigned)((count4 + 15) / 16)), dim3(256), 0, s, (const float*)ws, dw,
                       a.c_out, a.c_in, (int)split);
    return (int)hipGetLastError();
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
    a.x = x; a.dy = dy; a.out = nullptr;
    a.x_pix_stride = x_pix_stride; a.dy_pix_stride = dy_pix_stride;
    a.c_in = c_in; a.c_out = c_out; a.N = 4 * c_in;
    a.B = B; a.h_in = h; a.w_in = w; a.Hs = h; a.Ws = w; a.ups = 0; a.H = h; a.W = w;
    a.ksize = 2; a.dil = 1; a.stride = 1; a.pad = 0;
    a.M = (unsigned)mpix;
    a.pix_per_split = 0; a.n_ntiles = 0;
    a.pre_scale = nullptr; a.pre_shift = nullptr; a.pre_relu = 0;
    a.n_bundles = 4;
    const long per = 16L * c_out * c_in;                   // floats of the four class blocks of one split
    if (ws_floats < per) return BTS_ERR_INVALID;
    p = plan_wgrad(c_out, a.N, (long)a.M, ws_floats, true, 4);
    const long pps = (((long)a.M + p.split - 1) / p.split + WBK - 1) / WBK * WBK;
    p.split = ((long)a.M + pps - 1) / pps;                 // no empty splits
    a.pix_per_split = (unsigned)pps;
    if (p.split * per > ws_floats) return BTS_ERR_INVALID;
    return 0;
}

// ---- per-step packs of the upconv weights (bts_upconv_train_pack_f32) ----
struct UpconvPackEntry {    // 12 x int64, filled by the host (bts_amd/train.py)
    const float* src;       // OIHW [c_out][c_in][3][3]
    float* fwd;             // [4][c_out_pad][k_pad_f], k = (2*ty+tx)*c_in_ld + c   (ops.pack_upconv_subpixel)
    float* dgrad;           // [c_in_pad][k_pad_d], k = (4*r+s)*c_out_ld + n         (bts_upconv_dgrad_f32)
    long c_out, c_in, c_in_ld, c_out_ld, c_out_pad, k_pad_f, c_in_pad, k_pad_d;
    long first_block;       // prefix sum of blocks over the table
};

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
    int lo = 0, hi = n - 1;                       // the entry whose block range holds blockIdx.x
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (table[mid].first_block <= (long)blockIdx.x) lo = mid; else hi = mid - 1;
    }
    const UpconvPackEntry e = table[lo];
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

extern "C" int bts_upconv_wgrad_f32(const float* x, long x_pix_stride, int B, int h, int w, int c_in, const float* dy,
                                    long dy_pix_stride, int c_out, float* dw, float* ws, long ws_floats, bts_stream_t stream) {
    WgradArgs a;
    WgradPlan p;
    if (const int rc = prepare_upconv_wgrad(x, x_pix_stride, B, h, w, c_in, dy, dy_pix_stride, c_out, dw, ws, ws_floats, a, p); rc != 0) return rc;
    hipStream_t s = (hipStream_t)stream;
    switch (p.variant) {
        case 0: return launch_upconv_wgrad<128, 128, 2, 2>(a, p.split, dw, ws, s);
        case 1: return launch_upconv_wgrad<64, 128, 1, 4>(a, p.split, dw, ws, s);
        case 2: return launch_upconv_wgrad<32, 128, 1, 4>(a, p.split, dw, ws, s);
        default: return launch_upconv_wgrad<64, 64, 2, 2>(a, p.split, dw, ws, s);
    }
}

extern "C" int bts_upconv_wgrad_plan_f32(int B, int h, int w, int c_in, int c_out, long ws_floats, int* bm, int* bn, long* split,
                                         long* pix_per_split) {
    WgradArgs a;
    WgradPlan p;
    const float* dummy = (const float*)(uintptr_t)(1 << 20);      // pointers are checked, never followed
    if (const int rc = prepare_upconv_wgrad(dummy, c_in, B, h, w, c_in, dummy, c_out, c_out, dummy, dummy, ws_floats, a, p); rc != 0) return rc;
    if (bm) *bm = WGRAD_BM[p.variant];
    if (bn) *bn = WGRAD_BN[p.variant];
    if (split) *split = p.split;
    if (pix_per_split) *pix_per_split = (long)a.pix_per_split;
    return 0;
}

extern "C" long bts_upconv_train_pack_blocks(long c_out_pad, long k_pad_f, long c_in_pad, long k_pad_d) {
    return (4 * c_out_pad * k_pad_f + c_in_pad * k_pad_d + PACK_PER_BLOCK - 1) / PACK_PER_BLOCK;
}

extern "C" int bts_upconv_train_pack_f32(const void* table, int n_entries, long total_blocks, bts_stream_t stream) {
    if (!table || ((uintptr_t)table & 7) || n_entries <= 0 || total_blocks <= 0 || total_blocks > 2147483647L) return BTS_ERR_INVALID;
    hipLaunchKernelGGL(upconv_train_pack_kernel, dim3((unsigned)total_blocks), dim3(256), 0, (hipStream_t)stream,
                       (const UpconvPackEntry*)table, n_entries);
    return (int)hipGetLastError();
}
