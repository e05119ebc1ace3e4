// Weight gradient of ResNeXt's grouped 3x3 convolution (stride 1, padding 1, c channels in `groups` groups of 4 / 8 / 16) on the
// MULTI-BLOCK fp32 MFMA, v_mfma_f32_16x16x1_4b_f32 (included by conv_mfma.hip after conv_grouped.inc, whose tile constants,
// patch staging and D layout it shares).
//
//   dw[n][k][tap] = sum_{b, p} dy[b, p][n] * x[b, q(p, tap)][cg (n / cg) + k],   zero padding, tap = 3 (dy+1) + (dx+1)
//
//   * One instruction accumulates four independent 16 x 16 (output channel x input channel) blocks from ONE dy float and
//     ONE x float per lane: a 64-channel slab's gradient for one tap and one pixel.  Roles: A = dy (row = output channel of
//     the block), B = x (column = input channel of the block), K-step = one pixel; lane l holds channel 64 slab + l of both.
//     D register 4 b + q of lane l is block b, output channel 4 (l >> 4) + q, input channel l & 15 of that block.
//     cg 16: every product is algorithmic; cg 8 / 4: the off-diagonal (out group != in group) quarter-blocks are computed
//     and dropped (2x / 4x the algorithmic products, where the 32-channel bundles spend 4x / 8x).
//   * A workgroup (4 waves) owns a 64-channel slab and a contiguous range of 8 x 16-pixel tiles (blockIdx.x = split).  Nine
//     accumulators -- one per tap, 144 registers -- live in every wave for the life of the workgroup.  Per tile the 10 x 18
//     input patch with halo is staged in LDS in the forward's layout (two passes of six 16-byte loads in flight per
//     thread); wave v walks tile rows 2v and 2v + 1: its 32 dy floats are loaded into registers before the staging (in
//     flight under it), each pixel then reads its nine shifted x floats from LDS (64 consecutive floats per read:
//     conflict-free) and issues nine MFMAs onto nine different accumulators (no back-to-back dependent MFMAs).  A pixel of
//     a ragged tile outside the map has both of its operands replaced by zero (uniform selects: a lane is a channel): it
//     adds exact zeros, never 0 * inf.
//   * At the end the four waves' accumulators are folded through LDS in wave order 0..3 (((w0 + w1) + w2) + w3) into one
//     [9 taps][16 registers][64 lanes] block.  Unsplit, the workgroup writes the in-group entries straight into dw (OIHW);
//     split, it writes the block to ws[split][slab] and conv_grouped_wgrad_reduce_kernel sums the in-group entries in
//     ascending split order (common.h: sum_splits / sum_lanes) and writes OIHW.  Off-diagonal products never reach dw.
//   * Split rule (wgrad.hip's): a function of (B, h, w, c, groups, ws_floats) only -- ceil(512 / slabs) workgroups per slab,
//     one resident round of the chip at two workgroups per CU, all walking the same number of tiles (+-1 for the last) --
//     lowered to what the workspace holds, down to 1 with none; no atomics.
//   * Residency (-O3, gfx950, -Rpass-analysis=kernel-resource-usage): 255 / 255 / 256 VGPRs for CG 16 / 8 / 4 under the
//     launch bound of 256, no AGPRs, no scratch, 48 960 B of LDS -> two workgroups per CU (one stages while the other
//     multiplies).  The register file is full: twelve staging loads in flight at once, or masking dy in a loop of its own,
//     spill.
//
// Numerics: exact-f32 products; a dw entry's sum order is fixed by the shape and the split count alone (pixels of a wave in
// tile order then row-major, waves 0..3, splits ascending).  Non-finite values: an x or dy value reaches only dw entries of
// its own 16-channel block, and since off-diagonal products are dropped, only entries of its own group.
struct GroupedWgradArgs {
    const float* x; long x_pix_stride;
    const float* dy; long dy_pix_stride;
    int B, H, W;
    float* out;                                         // direct: dw [c][cg][3][3]; else ws [split][slab][9][16][64]
    int direct;
    int n_ty, n_tx, tiles, tiles_per_split;             // tiles per frame (rows, columns); tiles of the launch per slab
};

constexpr int GW_BLOCK = 9 * 16 * 64;                   // floats of one slab's folded accumulators

// (tap, register, lane) of dw entry (output channel nl of the slab, input channel k of its group, tap) in a folded block
template <int CG>
__device__ __forceinline__ int grouped_wgrad_slot(int nl, int k, int tap) {
    const int b = nl >> 4, o = nl & 15;
    return (tap * 16 + 4 * b + (o & 3)) * 64 + 16 * (o >> 2) + CG * (o / CG) + k;
}

// A loaded value as the compiler must take it: unconditionally loaded, whatever is selected from it afterwards.  Without
// this, "load from a clamped address, then select 0 outside the map" becomes a branch around the load with a full wait
// behind every single load -- one trip to memory per load instead of one per batch.
__device__ __forceinline__ void grouped_wgrad_landed(float& v) { asm volatile("" : "+v"(v)); }
__device__ __forceinline__ void grouped_wgrad_landed(f32x4& v) { asm volatile("" : "+v"(v)); }

// One tile's 32 pixels of wave wv: rows 2 wv, 2 wv + 1.  A pixel outside the map (ragged tile; uniform: a lane is a channel)
// has BOTH operands replaced by zero here, at their use, so it adds exact zeros and no 0 * inf; the walk itself is
// branch-free.  The nine x floats of pixel i + 1 are read under the MFMAs of pixel i and masked only when they are
// used, one pixel later (a select right behind the read waits out the LDS latency nine times per pixel), and nothing moves
// across a pixel: left to itself the scheduler hoists the LDS reads of the whole unrolled walk onto the 144 accumulator
// registers.
__device__ __forceinline__ void grouped_wgrad_pixels(f32x16 (&acc)[9], const float (&dv)[32], const float* __restrict__ bbase,
                                                     int rows_ok, int cols_ok) {
    auto read9 = [&](float (&bv)[9], int i) __attribute__((always_inline)) {
        const float* const bp = bbase + ((i / GR_TW) * GR_PW + i % GR_TW) * GR_LD;
#pragma unroll
        for (int tap = 0; tap < 9; ++tap) bv[tap] = bp[((tap / 3) * GR_PW + tap % 3) * GR_LD];
    };
    float bv[2][9];
    read9(bv[0], 0);
#pragma unroll
    for (int i = 0; i < 2 * GR_TW; ++i) {
        if (i + 1 < 2 * GR_TW) read9(bv[(i + 1) & 1], i + 1);
        __builtin_amdgcn_sched_barrier(0);              // the reads stay on top of the pixel's MFMAs
        const bool ok = i / GR_TW < rows_ok && i % GR_TW < cols_ok;
        float av = dv[i];
        grouped_wgrad_landed(av);
        av = ok ? av : 0.f;
#pragma unroll
        for (int tap = 0; tap < 9; ++tap)
            acc[tap] = __builtin_amdgcn_mfma_f32_16x16x1f32(av, ok ? bv[i & 1][tap] : 0.f, acc[tap], 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);
    }
}

template <int CG>
__global__ __launch_bounds__(256, 2) void conv_grouped_wgrad_kernel(const GroupedWgradArgs a) {
    static_assert(CG == 4 || CG == 8 || CG == 16, "one 16-channel MFMA block holds whole groups");
    static_assert(GR_PH * GR_PW * GR_LD >= GW_BLOCK, "the fold reuses the patch");
    __shared__ __attribute__((aligned(16))) float patch[GR_PH * GR_PW * GR_LD];

    const int tid = threadIdx.x;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
    const int slab = blockIdx.y, split = blockIdx.x;

    f32x16 acc[9];
#pragma unroll
    for (int tap = 0; tap < 9; ++tap)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[tap][e] = 0.f;

    const int per_frame = a.n_ty * a.n_tx;
    const long HW = (long)a.H * a.W;
    // this lane's first B element: patch row 2 wv (tap row 0 of tile row 2 wv), column 0, channel lane
    const float* const bbase = patch + (2 * wv) * GR_PW * GR_LD + lane;
    const int t_begin = split * a.tiles_per_split;
    const int t_end = min(a.tiles, t_begin + a.tiles_per_split);

    for (int t = t_begin; t < t_end; ++t) {
        const int bfr = t / per_frame;
        const int trem = t - bfr * per_frame;
        const int tyi = trem / a.n_tx;
        const int y0 = tyi * GR_TH, x0 = (trem - tyi * a.n_tx) * GR_TW;
        const float* const xf = a.x + (long)bfr * HW * a.x_pix_stride + 64 * slab;
        const float* const dyf = a.dy + (long)bfr * HW * a.dy_pix_stride + 64 * slab + lane;

        // ---- this wave's 32 dy floats (clamped addresses), in flight under the staging; masked where they are used
        float dv[32];
#pragma unroll
        for (int rr = 0; rr < 2; ++rr) {
            const long rowpix = (long)min(y0 + 2 * wv + rr, a.H - 1) * a.W;
#pragma unroll
            for (int cc = 0; cc < GR_TW; ++cc) dv[rr * GR_TW + cc] = dyf[(rowpix + min(x0 + cc, a.W - 1)) * a.dy_pix_stride];
        }

        __syncthreads();                                // the previous tile's reads are done
        // ---- stage the patch: thread = (patch pixel, channel quad); clamped addresses, zero padding
        // (two passes of six loads in flight per thread: all twelve at once spill beside the accumulators)
        constexpr int N_ST = 6, N_PASS = 2;
        static_assert(N_PASS * N_ST * 256 >= GR_PH * GR_PW * 16, "the passes cover the patch");
#pragma unroll
        for (int half = 0; half < N_PASS; ++half) {
            f32x4 sv[N_ST];
            bool okv[N_ST];
#pragma unroll
            for (int j = 0; j < N_ST; ++j) {
                const int i = min(tid + 256 * (N_ST * half + j), GR_PH * GR_PW * 16 - 1);
                const int pp = i >> 4, cq = i & 15;
                const int py = pp / GR_PW, px = pp - py * GR_PW;
                const int gy = y0 + py - 1, gx = x0 + px - 1;
                const bool ok = (unsigned)gy < (unsigned)a.H && (unsigned)gx < (unsigned)a.W;
                const long pix = (long)min(max(gy, 0), a.H - 1) * a.W + min(max(gx, 0), a.W - 1);
                sv[j] = *reinterpret_cast<const f32x4*>(xf + pix * a.x_pix_stride + 4 * cq);
                okv[j] = ok;
            }
#pragma unroll
            for (int j = 0; j < N_ST; ++j) {
                const int i = tid + 256 * (N_ST * half + j);
                grouped_wgrad_landed(sv[j]);
                if (i < GR_PH * GR_PW * 16)
                    *reinterpret_cast<f32x4*>(patch + (i >> 4) * GR_LD + 4 * (i & 15)) = okv[j] ? sv[j] : (f32x4)(0.f);
            }
        }
        __syncthreads();

        // ---- 32 pixels x 9 taps
        const int rows_ok = a.H - (y0 + 2 * wv), cols_ok = a.W - x0;       // real rows / columns from this wave's first pixel
        grouped_wgrad_pixels(acc, dv, bbase, rows_ok, cols_ok);
    }

    // ---- fold the four waves in wave order, then write
    for (int v = 0; v < 4; ++v) {
        __syncthreads();                                // v = 0: the last tile's reads are done
        if (wv == v) {
#pragma unroll
            for (int tap = 0; tap < 9; ++tap)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    float* const f = patch + (tap * 16 + r) * 64 + lane;
                    *f = v == 0 ? acc[tap][r] : *f + acc[tap][r];
                }
        }
    }
    __syncthreads();
    if (a.direct) {                                     // the slab's [64][CG][9] floats of dw are contiguous
        float* const dw = a.out + (long)slab * (64 * CG * 9);
        for (int i = tid; i < 64 * CG * 9; i += 256) {
            const int nl = i / (CG * 9), rem = i - nl * (CG * 9);
            const int k = rem / 9, tap = rem - 9 * k;
            dw[i] = patch[grouped_wgrad_slot<CG>(nl, k, tap)];
        }
    } else {
        f32x4* const o = reinterpret_cast<f32x4*>(a.out + ((long)split * gridDim.y + slab) * GW_BLOCK);
        for (int i = tid; i < GW_BLOCK / 4; i += 256) o[i] = *reinterpret_cast<const f32x4*>(patch + 4 * i);
    }
}

// dw (OIHW) = the in-group entries of the split partials, summed in ascending split order.  One float4 element = the four
// consecutive input channels 4 k4 .. 4 k4 + 3 of (output channel n, tap): contiguous in a partial block, stride 9 in dw.
template <int CG>
__global__ __launch_bounds__(256) void conv_grouped_wgrad_reduce_kernel(const float* __restrict__ ws, float* __restrict__ dw, int c,
                                                                        int splits) {
    const long count4 = (long)c * 9 * (CG / 4);
    const int el = threadIdx.x & 15, lane = threadIdx.x >> 4;
    const long t = (long)blockIdx.x * 16 + el;
    const long tt = t < count4 ? t : count4 - 1;
    const int k4 = (int)(tt % (CG / 4));
    const int tap = (int)((tt / (CG / 4)) % 9);
    const int n = (int)(tt / (9 * (CG / 4)));
    const float* const p = ws + (long)(n >> 6) * GW_BLOCK + grouped_wgrad_slot<CG>(n & 63, 4 * k4, tap);
    __shared__ f32x4 red[16][16];
    red[lane][el] = sum_splits(reinterpret_cast<const f32x4*>(p), (size_t)(c / 64) * (GW_BLOCK / 4), splits, lane);
    __syncthreads();
    if (lane == 0 && t < count4) {
        const f32x4 r = sum_lanes(red, el);
        float* const o = dw + ((long)n * CG + 4 * k4) * 9 + tap;
        o[0] = r.x; o[9] = r.y; o[18] = r.z; o[27] = r.w;
    }
}

// Host: the split of the tile axis -- (B, h, w, c, groups, ws_floats) only.  have_ws false = no workspace at all.
struct GroupedWgradPlan { long tiles, splits, tiles_per_split, ws_used; };
inline GroupedWgradPlan grouped_wgrad_plan(int B, int H, int W, int c, long ws_floats, bool have_ws) {
    int n_ty, n_tx; double fill;
    grouped_grid(H, W, &n_ty, &n_tx, &fill);
    const long slabs = c / 64, per = (long)GW_BLOCK * slabs;
    GroupedWgradPlan p;
    p.tiles = (long)B * n_ty * n_tx;
    long want = std::min((GR_RESIDENT + slabs - 1) / slabs, p.tiles);
    if (!have_ws || ws_floats < 2 * per) want = 1;
    else want = std::min(want, ws_floats / per);
    p.tiles_per_split = (p.tiles + want - 1) / want;
    p.splits = (p.tiles + p.tiles_per_split - 1) / p.tiles_per_split;      // no empty split
    p.ws_used = p.splits > 1 ? p.splits * per : 0;
    return p;
}
