// ResNeXt's grouped 3x3 convolution (stride 1, padding 1, c_in == c_out == c, 4 / 8 / 16 channels per group) with bf16
// operands on v_mfma_f32_16x16x16_bf16: the bf16 body of conv_grouped.inc (included by conv_mfma.hip inside its anonymous
// namespace, after conv_grouped.inc, whose tile constants and host helpers it shares).
//
//   y[p][n] = act( e1( sum_{tap, k < cg} bf16(x[q(p, tap)][cg g(n) + k]) * bf16(w[n][k][tap]) ) ),   zero padding, NHWC fp32
//
//   * One MFMA = one 16-channel block x one tap: its K = 16 is exactly the block's 16 input channels, so a tile takes
//     9 taps x 4 blocks x 2 rows = 72 MFMAs per wave where the multi-block fp32 form takes 288.  The two-tap form
//     (v_mfma_f32_16x16x32_bf16, five instructions per block with a zero-weighted tenth half-step) was not taken: nine taps
//     do not pair, the weights would grow to 160 c with a structural zero plane, and the 72 MFMAs (16 cycles each, 1152 per
//     tile and wave) already sit far below the tile's memory time (64 KB in and out per tile at ~13 B/clk/CU: ~5000 cycles).
//   * Roles as in the fp32 kernel: A = weights (row = output channel of the block), B = pixels (column = one of 16
//     x-consecutive pixels).  Lane l holds A[row l & 15][k = 4 (l >> 4) + 0..3] and B[k = 4 (l >> 4) + 0..3][column l & 15]:
//     four consecutive input channels of one pixel, one ds_read_b64.  D register q of lane l is row 4 (l >> 4) + q, column
//     l & 15: a lane owns four consecutive channels of each block at its own pixel, one 16-byte store per block.
//   * A workgroup (4 waves) owns a 64-channel slab and walks 8 x 16-pixel tiles of it, persistently (tile t = blockIdx.x,
//     + gridDim.x, ...).  The slab's weights -- 9 taps x 4 blocks, four bf16 per lane each -- stay in 72 registers of every
//     wave for the life of the workgroup.
//   * Per tile the 10 x 18-pixel patch WITH halo of the slab's 64 channels is rounded to bf16 (plain conversion,
//     v_cvt_pk_bf16_f32: nearest, ties to even; padding is an exact zero) and staged once into LDS at a pixel pitch of
//     72 bf16 = 144 bytes (64 + 8): a ds_read_b64 serves lanes 0-31 and 32-63 in turn, each 16 pixels x 2 k-quads = 16
//     bytes per pixel, and 144 p mod 256 runs through the 16 distinct 16-byte slots of the 256-byte bank row for p = 0..15:
//     conflict-free.  25 920 B of LDS.  Wave v runs tile rows 2v and 2v + 1 on two independent sets of accumulators.
//   * Residency: launch bound 256 registers, 25 KB of LDS -> TWO workgroups per CU as in the fp32 kernel (the persistent
//     grid is sized for that); one stages while the other multiplies.  No prefetch of the next patch inside a workgroup.
//   * CG only names the instantiation: the block-diagonal structure lives in the packed weights
//     (ops.pack_grouped_native_bf16), bf16 index (((s*9 + tap)*4 + b)*64 + lane)*4 + j = the weight from input channel
//     64 s + 16 b + 4 (lane >> 4) + j to output channel 64 s + 16 b + (lane & 15), exact zero across groups.
//
// Resources (hipcc -Rpass-analysis=kernel-resource-usage, gfx950, all three instantiations): 144 VGPRs, 0 AGPRs, 71 SGPRs,
// scratch 0, no spill, LDS 25 920 B per workgroup, occupancy 3 waves per SIMD by registers (the persistent grid of
// GR_RESIDENT workgroups puts two on a CU).
//
// Numerics: bf16 x bf16 products are exact in fp32 and accumulate in fp32, one fixed order per output (tap-major; the 16
// channels of a block inside the MFMA), so a frame's bits depend neither on B nor on any launch declaration nor on the
// grid.  Non-finite values: an input value reaches only the outputs of its own 16-channel block whose nine taps touch it.
constexpr int GB_LD = 72;                               // bf16 per patch pixel in LDS (64 + 8): 144 bytes
// "auto" (bts_conv_grouped_bf16_plan).  The thresholds start from the fp32 kernel's and profiles/grouped_bf16_bench.{txt,json}
// (scripts/grouped_bf16_bench.py, kernel sources 95cda26f507b3468, fill_frames 16, bundle launch of precision bf16 against
// this kernel, alternating) moves neither: all ten stride-1 classes with <= 16 channels per group of ResNeXt-101 32x8d and
// ResNeXt-50 32x4d at 416x544 and 352x1216 beat the bundle launch by more than the spread as the B = 16 launch (1.82x ...
// 2.38x by medians) and none loses as the B = 4 sub-batch launch (1.60x ... 2.45x).  The emptiest grid measured (26 x 34,
// fill 0.576, which is also the smallest declared launch: 1536 pairs) wins 0.0644 -> 0.0354 ms at B = 16 and 0.0380 ->
// 0.0215 ms at B = 4; the fullest (88 x 304, 256 channels, 13 376 pairs) 0.572 -> 0.269 ms.  Emptier grids and smaller
// declarations were not measured and stay on bundles.
constexpr long kGroupedBf16MinTiles = 2 * GR_RESIDENT;  // declared (slab, tile) pairs, as kGroupedMinTiles
constexpr double kGroupedBf16MinFill = 0.55;            // real pixels of the tile grid, as kGroupedMinFill

typedef short bf16x4_bits __attribute__((ext_vector_type(4)));      // the operand type of the 16x16x16 bf16 builtin

struct GroupedBf16Args {
    const float* x; long x_pix_stride; int B, H, W;
    const unsigned short* w;                            // [slab][9 taps][4 blocks][64 lanes][4 k]   (ops.pack_grouped_native_bf16)
    const float* e1_scale; const float* e1_shift; int act;
    float* y; long y_pix_stride;
    int n_ty, n_tx, tiles;                              // tiles per frame (rows, columns); tiles of the launch per slab
};

template <int ACT>
__device__ __forceinline__ void grouped_bf16_store(const GroupedBf16Args& a, const f32x4 (&acc)[4], long pix, int ch0) {
    float* const yp = a.y + pix * a.y_pix_stride + ch0;
#pragma unroll
    for (int b = 0; b < 4; ++b) {
        f32x4 v = acc[b];
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
__global__ __launch_bounds__(256, 2) void conv_grouped_bf16_kernel(const GroupedBf16Args a) {
    static_assert(CG == 4 || CG == 8 || CG == 16, "one 16-channel MFMA block holds whole groups");
    __shared__ __attribute__((aligned(16))) unsigned short patch[GR_PH * GR_PW * GB_LD];

    const int tid = threadIdx.x;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
    const int lp = lane & 15, lb = lane >> 4;
    const int slab = blockIdx.y;

    // ---- the slab's weights: 36 (tap, block) steps, four bf16 per lane each, kept for every tile of this workgroup
    bf16x4_bits wr[36];
    {
        const unsigned short* const wp = a.w + (long)slab * (144 * 64) + 4 * lane;
#pragma unroll
        for (int i = 0; i < 36; ++i) wr[i] = *reinterpret_cast<const bf16x4_bits*>(wp + i * 256);
    }
    const int per_frame = a.n_ty * a.n_tx;
    const long HW = (long)a.H * a.W;
    // this lane's first B element: patch row 2 wv (tap row 0 of tile row 2 wv), column lp, k-quad lb of block 0
    const unsigned short* const bbase = patch + ((2 * wv) * GR_PW + lp) * GB_LD + 4 * lb;

    for (int t = blockIdx.x; t < a.tiles; t += gridDim.x) {
        const int bfr = t / per_frame;
        const int trem = t - bfr * per_frame;
        const int tyi = trem / a.n_tx;
        const int y0 = tyi * GR_TH, x0 = (trem - tyi * a.n_tx) * GR_TW;
        const float* const xf = a.x + (long)bfr * HW * a.x_pix_stride + 64 * slab;

        __syncthreads();                                // the previous tile's reads are done
        // ---- stage the patch: thread = (patch pixel, channel quad); clamped addresses, zero padding, one rounding
#pragma unroll 4
        for (int i = tid; i < GR_PH * GR_PW * 16; i += 256) {
            const int pp = i >> 4, cq = i & 15;
            const int py = pp / GR_PW, px = pp - py * GR_PW;
            const int gy = y0 + py - 1, gx = x0 + px - 1;
            const bool ok = (unsigned)gy < (unsigned)a.H && (unsigned)gx < (unsigned)a.W;
            const long pix = (long)min(max(gy, 0), a.H - 1) * a.W + min(max(gx, 0), a.W - 1);
            f32x4 v = *reinterpret_cast<const f32x4*>(xf + pix * a.x_pix_stride + 4 * cq);
            v.x = ok ? v.x : 0.f; v.y = ok ? v.y : 0.f; v.z = ok ? v.z : 0.f; v.w = ok ? v.w : 0.f;
            *reinterpret_cast<u32x2*>(patch + pp * GB_LD + 4 * cq) = u32x2{pack_bf16_rne(v.x, v.y), pack_bf16_rne(v.z, v.w)};
        }
        __syncthreads();

        // ---- 9 taps x 4 blocks on two tile rows: one MFMA per (tap, block, row)
        f32x4 acc0[4], acc1[4];
#pragma unroll
        for (int b = 0; b < 4; ++b) { acc0[b] = f32x4{0.f, 0.f, 0.f, 0.f}; acc1[b] = f32x4{0.f, 0.f, 0.f, 0.f}; }
#pragma unroll
        for (int tap = 0; tap < 9; ++tap) {
            const unsigned short* const bp = bbase + ((tap / 3) * GR_PW + tap % 3) * GB_LD;
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                const bf16x4_bits v0 = *reinterpret_cast<const bf16x4_bits*>(bp + 16 * b);
                const bf16x4_bits v1 = *reinterpret_cast<const bf16x4_bits*>(bp + GR_PW * GB_LD + 16 * b);
                acc0[b] = __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(wr[tap * 4 + b], v0, acc0[b], 0, 0, 0);
                acc1[b] = __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(wr[tap * 4 + b], v1, acc1[b], 0, 0, 0);
            }
        }

        // ---- epilogue: lane = pixel lp of its rows, channels 64 slab + 16 b + 4 lb + (0..3)
        const int Y = y0 + 2 * wv, X = x0 + lp;
        const int ch0 = 64 * slab + 4 * lb;
        if (X < a.W) {
            const long pix = (long)bfr * HW + (long)Y * a.W + X;
            dispatch_act(a.act, [&](auto act) {
                if (Y < a.H) grouped_bf16_store<decltype(act)::value>(a, acc0, pix, ch0);
                if (Y + 1 < a.H) grouped_bf16_store<decltype(act)::value>(a, acc1, pix + a.W, ch0);
            });
        }
    }
}

// The layers the encoder hands to this kernel under grouped_conv_bf16 = "auto" (bts_conv_grouped_bf16_plan): bf16 arithmetic
// (precision 2), a supported shape, a tile grid that is mostly real pixels and a DECLARED launch (fill_frames x tiles x
// slabs, never B) of enough (slab, tile) pairs.
inline bool grouped_bf16_eligible(int H, int W, int c, int groups, int precision, int fill_frames, long* wgs_per_frame) {
    *wgs_per_frame = 0;
    if (H <= 0 || W <= 0 || precision != 2 || !grouped_supported(c, groups)) return false;
    int n_ty, n_tx; double fill;
    grouped_grid(H, W, &n_ty, &n_tx, &fill);
    *wgs_per_frame = (long)n_ty * n_tx * (c / 64);
    return fill >= kGroupedBf16MinFill && (long)fill_frames * *wgs_per_frame >= kGroupedBf16MinTiles;
}
