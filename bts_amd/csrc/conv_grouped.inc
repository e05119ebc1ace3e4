// ResNeXt's grouped 3x3 convolution (stride 1, padding 1, c_in == c_out == c, 4 / 8 / 16 channels per group) on the
// MULTI-BLOCK fp32 MFMA, v_mfma_f32_16x16x1_4b_f32: four independent 16x16 outer products per instruction, one A and one
// B float per lane -- the operand traffic per FLOP of the 16x16x4 form, at the same 64 FLOP/clk/SIMD (included by
// conv_mfma.hip inside its anonymous namespace).
//
//   y[p][n] = act( e1( sum_{tap, k < cg} x[q(p, tap)][cg g(n) + k] * w[n][k][tap] ) ),   zero padding, NHWC in and out
//
//   * One MFMA block = 16 consecutive channels, in AND out: one group at 16 channels per group (no redundant product),
//     two / four groups at 8 / 4 per group (block-diagonal weights with exact zeros off the diagonal: 2x / 4x the
//     algorithmic products, where the 32-channel bundles of bts_conv_desc.n_bundles spend 4x / 8x).
//   * Roles: A = weights (row = output channel of the block), B = pixels (column = one of 16 x-consecutive pixels).  Lane l
//     holds A of block l >> 4, row l & 15 and B of block l >> 4, column l & 15; D register 4 b + q of lane l is block b,
//     row 4 (l >> 4) + q, column l & 15: a lane owns four consecutive channels of each block at its own pixel, one
//     16-byte store per block.
//   * A workgroup (4 waves) owns a 64-channel slab (four blocks) and walks 8 x 16-pixel tiles of it, persistently
//     (tile t = blockIdx.x, + gridDim.x, ...).  The slab's whole weight -- 9 taps x 16 block channels = 144 k-steps, ONE
//     float per lane each -- stays in 144 registers of every wave for the life of the workgroup: no weight traffic per
//     tile, no LDS for weights.
//   * Per tile the 10 x 18-pixel input patch WITH halo of the slab's 64 channels is staged once into LDS (68 floats per
//     pixel: the 16 pixels of a ds_read_b128 lane group fall in 16 distinct 16-byte bank slots; 48 960 B) and all nine
//     taps read it as shifted views.  A lane reads four consecutive channels of its (block, pixel) with one
//     ds_read_b128 and feeds four consecutive MFMAs.  Wave v runs tile rows 2v and 2v + 1 on two independent
//     accumulators: 288 MFMAs and 72 LDS reads per tile and wave.
//   * Residency: launch bound 256 registers and 48 KB of LDS -> TWO workgroups per CU; one stages its patch while the
//     other multiplies.  There is no prefetch of the next patch inside a workgroup.
//   * CG only names the instantiation (profiles tell the layer classes apart): the machine code is the same, the
//     block-diagonal structure lives in the packed weights (ops.pack_grouped_native).
//
// Measured and not kept (B = 16, stand-alone launches, DESIGN 3d): ONE workgroup per CU (512 registers per lane) that loads
// the next tile's patch into 48 registers under the current tile's MFMAs and writes them to LDS afterwards -- 0.247 / 0.151
// ms on ResNeXt-101's layer-1 / layer-2 launches at 416x544 against 0.258 / 0.139 for this form, 0.421 / 0.243 against
// 0.431 / 0.248 at 352x1216: inside the run-to-run spread, so the shorter code stays.
//
// Numerics: exact-f32 products, one k-ordered chain per output (tap-major, block channel ascending), so a frame's bits depend
// neither on B nor on any launch declaration nor on the grid.  Non-finite values: an input value reaches only the outputs
// of its own 16-channel block whose nine taps touch it -- its own group for CG 16; for CG < 16 also the other groups of
// the block (0 * inf), as the bundle path does over 32 channels.
constexpr int GR_TH = 8, GR_TW = 16;                    // output pixels of a workgroup tile (rows, columns)
constexpr int GR_PH = GR_TH + 2, GR_PW = GR_TW + 2;     // its input patch
constexpr int GR_LD = 68;                               // floats per patch pixel in LDS (64 + 4)
constexpr int GR_RESIDENT = 512;                        // workgroups the chip holds: 2 per CU x 256 CUs
constexpr long kGroupedMinTiles = 2 * GR_RESIDENT;      // declared (slab, tile) pairs: two per resident workgroup, so that the
                                                        // 36 KB weight fetch per wave is shared by more than one tile
constexpr double kGroupedMinFill = 0.55;                // the project's 0.70 rule, lowered by measurement: the emptiest grid measured
                                                        // (26 x 34, fill 0.575) still beats the bundle launch 1.6x (DESIGN 3d)

struct GroupedArgs {
    const float* x; long x_pix_stride; int B, H, W;
    const float* w;                                     // [slab][9 taps][16 k][64 lanes]   (ops.pack_grouped_native)
    const float* e1_scale; const float* e1_shift; int act;
    float* y; long y_pix_stride;
    int n_ty, n_tx, tiles;                              // tiles per frame (rows, columns); tiles of the launch per slab
};

template <int ACT>
__device__ __forceinline__ void grouped_store(const GroupedArgs& a, const f32x16& acc, long pix, int ch0) {
    float* const yp = a.y + pix * a.y_pix_stride + ch0;
#pragma unroll
    for (int b = 0; b < 4; ++b) {
        f32x4 v = {acc[4 * b], acc[4 * b + 1], acc[4 * b + 2], acc[4 * b + 3]};
        if (a.e1_scale != nullptr) {                    // uniform
            const f32x4 sc = *reinterpret_cast<const f32x4*>(a.e1_scale + ch0 + 16 * b);
            const f32x4 sh = *reinterpret_cast<const f32x4*>(a.e1_shift + ch0 + 16 * b);
            v = v * sc + sh;
        }
        v.x = act_fn<ACT>(v.x); v.y = act_fn<ACT>(v.y); v.z = act_fn<ACT>(v.z); v.w = act_fn<ACT>(v.w);
        *reinterpret_cast<f32x4*>(yp + 16 * b) = v;
    }
}

template <int CG>
__global__ __launch_bounds__(256, 2) void conv_grouped_kernel(const GroupedArgs a) {
    static_assert(CG == 4 || CG == 8 || CG == 16, "one 16-channel MFMA block holds whole groups");
    __shared__ __attribute__((aligned(16))) float patch[GR_PH * GR_PW * GR_LD];

    const int tid = threadIdx.x;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
    const int lp = lane & 15, lb = lane >> 4;
    const int slab = blockIdx.y;

    // ---- the slab's weights: 144 k-steps, one float per lane each, kept for every tile of this workgroup
    float wr[144];
    {
        const float* const wp = a.w + (long)slab * (144 * 64) + lane;
#pragma unroll
        for (int i = 0; i < 144; ++i) wr[i] = wp[i * 64];
    }
    const int per_frame = a.n_ty * a.n_tx;
    const long HW = (long)a.H * a.W;
    // this lane's first B element: patch row 2 wv (tap row 0 of tile row 2 wv), column lp, block lb
    const float* const bbase = patch + ((2 * wv) * GR_PW + lp) * GR_LD + 16 * lb;

    for (int t = blockIdx.x; t < a.tiles; t += gridDim.x) {
        const int bfr = t / per_frame;
        const int trem = t - bfr * per_frame;
        const int tyi = trem / a.n_tx;
        const int y0 = tyi * GR_TH, x0 = (trem - tyi * a.n_tx) * GR_TW;
        const float* const xf = a.x + (long)bfr * HW * a.x_pix_stride + 64 * slab;

        __syncthreads();                                // the previous tile's reads are done
        // ---- stage the patch: thread = (patch pixel, channel quad); clamped addresses, zero padding
#pragma unroll 4
        for (int i = tid; i < GR_PH * GR_PW * 16; i += 256) {
            const int pp = i >> 4, cq = i & 15;
            const int py = pp / GR_PW, px = pp - py * GR_PW;
            const int gy = y0 + py - 1, gx = x0 + px - 1;
            const bool ok = (unsigned)gy < (unsigned)a.H && (unsigned)gx < (unsigned)a.W;
            const long pix = (long)min(max(gy, 0), a.H - 1) * a.W + min(max(gx, 0), a.W - 1);
            f32x4 v = *reinterpret_cast<const f32x4*>(xf + pix * a.x_pix_stride + 4 * cq);
            v.x = ok ? v.x : 0.f; v.y = ok ? v.y : 0.f; v.z = ok ? v.z : 0.f; v.w = ok ? v.w : 0.f;
            *reinterpret_cast<f32x4*>(patch + pp * GR_LD + 4 * cq) = v;
        }
        __syncthreads();

        // ---- 9 taps x 16 block channels on two tile rows
        f32x16 acc0, acc1;
#pragma unroll
        for (int e = 0; e < 16; ++e) { acc0[e] = 0.f; acc1[e] = 0.f; }
#pragma unroll
        for (int tap = 0; tap < 9; ++tap) {
            const float* const bp = bbase + ((tap / 3) * GR_PW + tap % 3) * GR_LD;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const f32x4 v0 = *reinterpret_cast<const f32x4*>(bp + 4 * j);
                const f32x4 v1 = *reinterpret_cast<const f32x4*>(bp + GR_PW * GR_LD + 4 * j);
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    acc0 = __builtin_amdgcn_mfma_f32_16x16x1f32(wr[tap * 16 + 4 * j + q], v0[q], acc0, 0, 0, 0);
                    acc1 = __builtin_amdgcn_mfma_f32_16x16x1f32(wr[tap * 16 + 4 * j + q], v1[q], acc1, 0, 0, 0);
                }
            }
        }

        // ---- epilogue: lane = pixel lp of its rows, channels 64 slab + 16 b + 4 lb + (0..3)
        const int Y = y0 + 2 * wv, X = x0 + lp;
        const int ch0 = 64 * slab + 4 * lb;
        if (X < a.W) {
            const long pix = (long)bfr * HW + (long)Y * a.W + X;
            dispatch_act(a.act, [&](auto act) {
                if (Y < a.H) grouped_store<decltype(act)::value>(a, acc0, pix, ch0);
                if (Y + 1 < a.H) grouped_store<decltype(act)::value>(a, acc1, pix + a.W, ch0);
            });
        }
    }
}

// Host: tiles of one frame and the share of their pixels that are real (the tile-grid fill)
inline void grouped_grid(int H, int W, int* n_ty, int* n_tx, double* fill) {
    *n_ty = (H + GR_TH - 1) / GR_TH; *n_tx = (W + GR_TW - 1) / GR_TW;
    *fill = (double)H * W / ((double)*n_ty * GR_TH * *n_tx * GR_TW);
}

// What the entry point runs: whole 64-channel slabs of whole groups of 4, 8 or 16 channels
inline bool grouped_supported(int c, int groups) {
    if (c <= 0 || groups <= 0 || (c % groups) || (c % 64)) return false;
    const int cg = c / groups;
    return cg == 4 || cg == 8 || cg == 16;
}

// The layers the encoder hands to this kernel under grouped_conv = "auto" (bts_conv_grouped_plan): fp32 arithmetic, a
// supported shape, a tile grid that is mostly real pixels and a DECLARED launch (fill_frames x tiles x slabs, never B) of at
// least two tiles per resident workgroup.
inline bool grouped_eligible(int H, int W, int c, int groups, int precision, int fill_frames, long* wgs_per_frame) {
    *wgs_per_frame = 0;
    if (H <= 0 || W <= 0 || precision != 0 || !grouped_supported(c, groups)) return false;
    int n_ty, n_tx; double fill;
    grouped_grid(H, W, &n_ty, &n_tx, &fill);
    *wgs_per_frame = (long)n_ty * n_tx * (c / 64);
    return fill >= kGroupedMinFill && (long)fill_frames * *wgs_per_frame >= kGroupedMinTiles;
}
