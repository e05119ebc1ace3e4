// Wide 1x1 convolution with bf16 operands (the precision-2 arithmetic of DESIGN 3c) for c_out % 192 == 0: DenseNet161's
// bottleneck 1x1 layers under conv_precision "bf16".  Included by conv_mfma.hip inside its anonymous namespace, after
// conv_tail_bf16.inc.  Opt-in: its own entry point (bts_conv1x1_bf16_fwd_f32); bts_conv_fwd_f32 keeps these layers on the
// row-tiled kernel (BTS_CONV_KIND_ROW_BF16) whatever this file does.
//
//   y[p][n] = act( e1( sum_{c < c_in} bf16( P(x[p][c]) ) * wb[n][c] ) )                       (fp32 accumulation, ascending k)
//   P(v) = fma(v, pre_scale[c], pre_shift[c]) [then max(., 0)]: ONE fused multiply-add in fp32, then rounded to bf16 (RNE)
//
// What the row-tiled kernel does to such a layer: 64-wide N tiles, so a pixel tile's input is fetched, put through the
// prologue and converted three times for 192 outputs, through LDS each time, and every workgroup rounds its fp32 weight
// tile itself.  Here:
//   * ONE workgroup (4 waves) owns 128 pixels and all BN = 192 channels of an N tile; wave w owns pixels 32 w .. 32 w + 31
//     and holds BN / 32 = 6 accumulators of v_mfma_f32_32x32x16_bf16.
//   * The A operand never touches LDS.  The 32x32x16 lane map gives lane l the 8 consecutive k of row l & 31, k-group
//     l >> 5: 32 contiguous bytes of one NHWC pixel.  Per 16 k a lane issues two 16-byte loads, eight fmas and four
//     conversions (v_cvt_pk_bf16_f32); every input value is fetched, affined and converted exactly ONCE.
//   * The weights are the pre-rounded one-plane copy (ops.round_bf16: [c_out_pad][k_pad] bf16), streamed by LDS-DMA
//     (global_load_lds_dwordx4, 16 rows x 64 B per wave instruction) into a ring of TWO stages of BN unpadded 64-byte rows
//     whose four 16-byte chunks are XOR-swizzled with bits 2-3 of the row -- on the per-lane SOURCE address; the reader
//     applies it again (conv_halo_emu.inc's layout: conflict-free ds_read_b128).
//   * The prologue vectors are staged to LDS once per workgroup (2 x k32 floats) and read back as broadcast ds_read_b128.
//
// One K step = 32 k (two MFMA k-blocks).  At the start of step s every wave issues its share of the DMA for step s+1 into
// the stage step s-1 read (the barrier that ended s-1 protects it) and the loads of its own A values of step s+1; then the
// 12 MFMAs of step s; then s_waitcnt vmcnt(0) and a barrier, after which step s+1's stage may be read (the wait comes
// BEFORE the barrier, the read after it).  Nothing stays in flight across a barrier, so every count is 0 and a partial
// last step (c_in % 32 == 16) may simply skip its second k-block: neither its loads nor its MFMAs are issued, so
// channels >= c_in of x and the K padding of the weights never reach a product.  Latency is hidden by the other
// workgroups of the CU (three per CU by registers), not by a deeper ring: the K loop is 3 .. 66 steps long.
//
// Sum order: ascending k in 16-k MFMA blocks, whatever the grid: a pixel's bits depend neither on npix nor on its
// position in the launch -- nor on BN.
//
// The same body is instantiated at BN = 128 and 256 for the second entry point (bts_conv1x1_bf16_wide_fwd_f32: ResNe(X)t's
// conv1 / conv3 / stride-1 downsample, DenseNet121's 128-wide bottlenecks), which also has the bottleneck epilogue
// (conv1x1_bf16_epi_kernel: y = act(e1(acc) + res), the same values to y2 -- bts_conv_desc.res / .y2).  The epilogue is a
// template flag, so the kernel the first entry point launches is the code it was.  gfx950, registers / waves per SIMD / scratch:
//   BN 128: 120 / 4 / 0     BN 192: 152 / 3 / 0     BN 256: 188 (epilogue: 189) / 2 / 0;   LDS 2 * BN * 64 B + 8 B per channel.
struct Conv1x1Bf16Args {
    const float* x; long x_pix_stride; long npix; int c_in;
    const unsigned short* w; int k_pad;           // bf16 [c_out_pad][k_pad]
    int c_out, c_out_pad;
    const float* pre_scale; const float* pre_shift; int pre_relu;
    const float* e1_scale; const float* e1_shift; int act;
    float* y; long y_pix_stride;
    int n_ntiles;
    const float* res; long res_pix_stride;        // bottleneck epilogue (conv1x1_bf16_epi_kernel only): bts_conv_desc.res / .y2
    float* y2; long y2_pix_stride;
};

constexpr int C1B_BM = 128;                       // pixels per workgroup (4 waves x 32)
template <int BN> constexpr int c1b_stage_bytes() { return BN * EMU_ROW_BYTES; }
// LDS: two weight stages, then the prologue scale and shift of all k32 = roundup(c_in, 32) channels
template <int BN> inline size_t c1b_lds_bytes(int c_in, bool has_pre) {
    return (size_t)2 * c1b_stage_bytes<BN>() + (has_pre ? (size_t)2 * ((c_in + 31) / 32 * 32) * sizeof(float) : 0);
}

// One wave's 32 pixels x BN channels to the NHWC slice: a wave-uniform 64-bit row base plus one per-lane 32-bit offset
// EPI: y = act(e1(acc) + res[p][n]) (one fp32 add, after e1 and before the activation), and the same values to y2; either
// operand may be null.  A residual value is loaded only where its output is stored: rows >= npix are never touched.
template <int ACT, int TN, bool EPI, typename AccT>
__device__ __forceinline__ void c1b_store(const Conv1x1Bf16Args& a, const AccT (&acc)[TN], long pix0, int nvalid, int ncol0, int li, int lh) {
    float* const yb = a.y + pix0 * a.y_pix_stride;                                      // wave-uniform
    const int nv = nvalid - 4 * lh;                                                     // slots this lane's half may write
#pragma unroll
    for (int j = 0; j < TN; ++j) {
        const int n = ncol0 + j * 32 + li;                                              // < c_out: c_out % BN == 0
        float s1 = a.e1_scale != nullptr ? a.e1_scale[n] : 1.f;
        float b1 = a.e1_scale != nullptr ? a.e1_shift[n] : 0.f;
        asm volatile("" : "+v"(s1), "+v"(b1));          // waited for HERE, once (see tail_bf16_store)
        const unsigned lane_y = (unsigned)(4 * lh) * (unsigned)a.y_pix_stride + (unsigned)n;
        if constexpr (!EPI) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int qu = (r & 3) + 8 * (r >> 2);
                const float v = act_fn<ACT>(fmaf(acc[j][r], s1, b1));
                if (qu < nv) (yb + (long)qu * a.y_pix_stride)[lane_y] = v;
            }
        } else {
            float rv[16];
#pragma unroll
            for (int r = 0; r < 16; ++r) {                 // the 16 residual loads of this column in flight together
                const int qu = (r & 3) + 8 * (r >> 2);
                rv[r] = 0.f;
                if (a.res != nullptr && qu < nv) rv[r] = a.res[(pix0 + 4 * lh + qu) * a.res_pix_stride + n];
            }
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int qu = (r & 3) + 8 * (r >> 2);
                float v = fmaf(acc[j][r], s1, b1);
                if (a.res != nullptr) v += rv[r];
                v = act_fn<ACT>(v);
                if (qu < nv) {
                    (yb + (long)qu * a.y_pix_stride)[lane_y] = v;
                    if (a.y2 != nullptr) a.y2[(pix0 + 4 * lh + qu) * a.y2_pix_stride + n] = v;
                }
            }
        }
    }
}

// The same tile to a BF16 destination (bts_conv1x1_bf16_fwd_bf16: the bottleneck intermediate of a dense layer, whose only
// reader -- the 3x3 growth convolution on the bf16 halo tile -- rounds every value to bf16 on its way to LDS anyway).  a.y is
// then a bf16 buffer and a.y_pix_stride counts bf16 elements.  The value stored is c1b_store's act(e1(acc)) put through
// pack_bf16_rne: the routine plane_store<1> rounds the halo tile's patch with, so rounding here and copying there gives the
// consumer's LDS the bits it has today, NaN and infinity included.
// Two store forms were built and measured (the producer alone, DenseNet161 blocks 1-2 at 352x1216, three K each, B = 16 and
// B = 4, three forms alternating in one process, 5 rounds x 300 launches, median us per launch; both forms gave the RNE bits
// of the fp32 kernel's output on every class):
//   plain : every lane stores its own channel, 2 bytes -- sixteen half-width wave stores per column tile.  152 VGPRs, 3 waves
//           per SIMD, no scratch.
//   paired: adjacent lanes (channels n, n + 1; n even) exchange one value per row pair by DPP (quad_perm [1,0,3,2]); the even
//           lane then stores rows 2t, the odd lane rows 2t + 1, both channels in one 4-byte store: eight stores per lane and
//           column tile, each wave store as wide as the fp32 kernel's.  Needs a 4-byte aligned row (host: stride % 4 == 0).
//           154 VGPRs, 3 waves per SIMD, no scratch.
//                        fp32 store   plain   paired                          fp32 store   plain   paired
//   B=16 block1 K  96      100.8      81.7    78.6        B=4 block1 K  96       26.8      23.7    22.0
//               K 240      170.2     148.9   145.5                   K 240       39.9      37.2    35.1
//               K 336      211.7     190.3   187.4                   K 336       48.7      46.5    44.7
//        block2 K 192       37.7      32.7    30.7            block2 K 192       15.6      14.3    13.3
//               K 480       84.8      74.3    74.3                   K 480       28.7      27.8    26.9
//               K 720      122.4     116.8   115.1                   K 720       37.9      36.9    36.0
// Paired is ahead of plain on eleven classes of twelve (+1.5 ... +7.5 %, spreads <= 1.0 %) and level on one: it is the form
// kept; the plain form is not built.
template <int ACT, int TN, typename AccT>
__device__ __forceinline__ void c1b_store_bf16(const Conv1x1Bf16Args& a, const AccT (&acc)[TN], long pix0, int nvalid, int ncol0, int li, int lh) {
    unsigned short* const yb = reinterpret_cast<unsigned short*>(a.y) + pix0 * a.y_pix_stride;      // wave-uniform
    const int nv = nvalid - 4 * lh;
    const bool odd = li & 1;
#pragma unroll
    for (int j = 0; j < TN; ++j) {
        const int n = ncol0 + j * 32 + li;
        float s1 = a.e1_scale != nullptr ? a.e1_scale[n] : 1.f;
        float b1 = a.e1_scale != nullptr ? a.e1_shift[n] : 0.f;
        asm volatile("" : "+v"(s1), "+v"(b1));          // waited for HERE, once (see tail_bf16_store)
        // this lane's row of the pair (rows 2t + odd) and the 4-byte slot of channels n & ~1, n | 1
        const unsigned lane_y = (unsigned)(4 * lh + (odd ? 1 : 0)) * (unsigned)a.y_pix_stride + (unsigned)(n & ~1);
#pragma unroll
        for (int t = 0; t < 8; ++t) {
            const int qu = ((2 * t) & 3) + 8 * ((2 * t) >> 2);                      // row slot of r = 2t; r = 2t + 1 is qu + 1
            const float v0 = act_fn<ACT>(fmaf(acc[j][2 * t], s1, b1)), v1 = act_fn<ACT>(fmaf(acc[j][2 * t + 1], s1, b1));
            const float mine = odd ? v1 : v0, send = odd ? v0 : v1;                 // the partner stores the other row
            const float recv = __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, send), 0xB1, 0xF, 0xF, false));
            const unsigned pk = odd ? pack_bf16_rne(recv, mine) : pack_bf16_rne(mine, recv);      // low half = the even channel
            if (qu + (odd ? 1 : 0) < nv)
                *reinterpret_cast<unsigned*>(yb + (long)qu * a.y_pix_stride + lane_y) = pk;
        }
    }
}

// Workgroups per CU the register file is asked to hold: BN = 128 (64 accumulator registers) four, BN = 192 (96) and
// BN = 256 (128 + 32 for the B fragments) two -- 192 takes 152 registers and gets three by itself, 256 cannot get three.
template <int BN> constexpr int c1b_min_wgs_per_cu() { return BN <= 128 ? 4 : 2; }

// YBF16: the bf16 destination (c1b_store_bf16; no EPI form)
template <int BN, bool EPI, bool YBF16 = false>
__device__ __forceinline__ void c1b_body(const Conv1x1Bf16Args& a) {
    constexpr int TN = BN / 32, STAGE = c1b_stage_bytes<BN>();
    constexpr int NIW = BN / 16 / 4;                      // DMA wave-instructions per stage and wave (16 rows x 64 B each)
    static_assert(BN % 64 == 0, "the four waves share a stage's DMA evenly");
    typedef float acc_t __attribute__((ext_vector_type(16)));
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    char* const Bs = smem_raw;
    float* const Ps = reinterpret_cast<float*>(smem_raw + 2 * STAGE);      // [2][k32]: scale, then shift

    const int tile = xcd_swizzle(blockIdx.x, gridDim.x);
    const int mt = tile / a.n_ntiles, n0 = (tile - mt * a.n_ntiles) * BN;
    const int tid = threadIdx.x;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
    const int li = lane & 31, lh = lane >> 5;
    const int nk16 = a.c_in >> 4;                          // host: c_in % 16 == 0
    const int nsteps = (nk16 + 1) >> 1, k32 = nsteps * 32;
    const bool has_pre = a.pre_scale != nullptr;
    const bool relu = a.pre_relu != 0;

    // this lane's pixel (clamped: rows past npix are loaded from the last pixel and never stored)
    const long pix0 = (long)mt * C1B_BM + wv * 32;
    const long prow = pix0 + li < a.npix ? pix0 + li : a.npix - 1;
    const float* const xp = a.x + prow * a.x_pix_stride + lh * 8;

    // weight DMA: wave wv sends wave-instructions q = wv + 4u: rows [16 q, 16 q + 16) of the stage
    unsigned wsrc[NIW];
#pragma unroll
    for (int u = 0; u < NIW; ++u) {
        const int r = (wv + 4 * u) * 16 + (lane >> 2);
        const int chunk = (lane & 3) ^ ((r >> 2) & 3);    // source-side swizzle (the reader XORs again)
        int n = n0 + r;
        n = n < a.c_out_pad ? n : a.c_out_pad - 1;
        wsrc[u] = (unsigned)n * (unsigned)a.k_pad + (unsigned)(chunk * 8);
    }
    auto dma_b = [&](int step, int stage_idx) {
        const unsigned koff = (unsigned)(step * BK);       // step * 32 + 32 <= k32 <= k_pad
        char* const stage = Bs + stage_idx * STAGE;
#pragma unroll
        for (int u = 0; u < NIW; ++u)
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(a.w + (wsrc[u] + koff)),
                                             (__attribute__((address_space(3))) void*)(stage + (wv + 4 * u) * 1024), 16, 0, 0);
    };
    // A values of one step: k-block ks covers channels step*32 + ks*16 + lh*8 .. +7; a k-block past c_in is not loaded
    auto load_a = [&](int step, f32x4 (&raw)[4]) {
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            if (2 * step + ks < nk16) {
                const float* const p = xp + step * BK + ks * 16;
                raw[2 * ks] = *reinterpret_cast<const f32x4*>(p);
                raw[2 * ks + 1] = *reinterpret_cast<const f32x4*>(p + 4);
            } else {
                raw[2 * ks] = f32x4{0.f, 0.f, 0.f, 0.f};
                raw[2 * ks + 1] = f32x4{0.f, 0.f, 0.f, 0.f};
            }
        }
    };
    // prologue (one fma, optional ReLU) and RNE conversion: 8 fp32 -> one bf16x8 fragment per k-block
    auto convert = [&](int step, const f32x4 (&raw)[4], u32x4 (&fa)[2]) {
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            f32x4 v0 = raw[2 * ks], v1 = raw[2 * ks + 1];
            if (has_pre) {
                const float* const ps = Ps + step * BK + ks * 16 + lh * 8;
                const f32x4 s0 = *reinterpret_cast<const f32x4*>(ps), s1 = *reinterpret_cast<const f32x4*>(ps + 4);
                const f32x4 b0 = *reinterpret_cast<const f32x4*>(ps + k32), b1 = *reinterpret_cast<const f32x4*>(ps + k32 + 4);
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    v0[e] = fmaf(v0[e], s0[e], b0[e]);
                    v1[e] = fmaf(v1[e], s1[e], b1[e]);
                    if (relu) { v0[e] = fmaxf(v0[e], 0.f); v1[e] = fmaxf(v1[e], 0.f); }
                }
            }
            fa[ks] = u32x4{pack_bf16_rne(v0.x, v0.y), pack_bf16_rne(v0.z, v0.w), pack_bf16_rne(v1.x, v1.y), pack_bf16_rne(v1.z, v1.w)};
        }
    };

    acc_t acc[TN];
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[j][r] = 0.f;

    // ---------------------------------------------------------------- prologue: stage 0 in flight, A of step 0, the vectors
    f32x4 raw[4];
    u32x4 fa[2];
    dma_b(0, 0);
    load_a(0, raw);
    if (has_pre)
        for (int c = tid; c < k32; c += 256) {
            const bool in = c < a.c_in;                    // the vectors hold c_in values; the rest is never multiplied
            Ps[c] = in ? a.pre_scale[c] : 1.f;
            Ps[k32 + c] = in ? a.pre_shift[c] : 0.f;
        }
    wait_then_barrier<0>();
    convert(0, raw, fa);

    const int sw = (li >> 2) & 3;
    const int b_row = li * EMU_ROW_BYTES;
    for (int s = 0; s < nsteps; ++s) {
        const char* const cur = Bs + (s & 1) * STAGE;
        const bool more = s + 1 < nsteps;
        if (more) {
            dma_b(s + 1, (s + 1) & 1);
            load_a(s + 1, raw);
        }
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            if (ks == 0 || 2 * s + 1 < nk16) {             // the second k-block of a partial last step does not exist
                u32x4 fb[TN];
#pragma unroll
                for (int j = 0; j < TN; ++j)
                    fb[j] = *reinterpret_cast<const u32x4*>(cur + j * 32 * EMU_ROW_BYTES + b_row + (((2 * ks + lh) ^ sw) << 4));
#pragma unroll
                for (int j = 0; j < TN; ++j)
                    acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, fa[ks]), __builtin_bit_cast(bf16x8, fb[j]),
                                                                     acc[j], 0, 0, 0);
            }
        }
        if (more) {
            wait_then_barrier<0>();                        // every wave's DMA of step s+1 has landed; stage s & 1 is free
            convert(s + 1, raw, fa);
        }
    }

    // ---------------------------------------------------------------- epilogue (NHWC slice)
    const long left = a.npix - pix0;
    const int nvalid = left >= 32 ? 32 : (left > 0 ? (int)left : 0);
    if constexpr (YBF16) {
        static_assert(!EPI, "the bf16 destination has no residual epilogue");
        dispatch_act(a.act, [&](auto act) { c1b_store_bf16<decltype(act)::value, TN>(a, acc, pix0, nvalid, n0, li, lh); });
    } else
    dispatch_act(a.act, [&](auto act) { c1b_store<decltype(act)::value, TN, EPI>(a, acc, pix0, nvalid, n0, li, lh); });
}

template <int BN>
__global__ __launch_bounds__(256, c1b_min_wgs_per_cu<BN>()) void conv1x1_bf16_kernel(const Conv1x1Bf16Args a) { c1b_body<BN, false>(a); }
// the same tile with the bottleneck epilogue (a.res and / or a.y2 set)
template <int BN>
__global__ __launch_bounds__(256, c1b_min_wgs_per_cu<BN>()) void conv1x1_bf16_epi_kernel(const Conv1x1Bf16Args a) { c1b_body<BN, true>(a); }

// the same tile to a bf16 destination (bts_conv1x1_bf16_fwd_bf16)
template <int BN>
__global__ __launch_bounds__(256, c1b_min_wgs_per_cu<BN>()) void conv1x1_bf16_ybf16_kernel(const Conv1x1Bf16Args a) { c1b_body<BN, false, true>(a); }

// The layers the encoder hands to this kernel under BtsModel.bf16_wide_1x1 (bts_conv1x1_bf16_plan).  Structural: whole
// 192-channel N tiles, whole 16-k MFMA blocks.  Measured: a declared launch of at least kC1bMinWgs workgroups.
//
// kC1bMinWgs = 512, two workgroups per CU of the DECLARED launch, from profiles/conv1x1_bf16_bench.txt (isolated launches
// against today's row-tiled bf16 path, DenseNet161 at 352x1216, fill_frames 16; a launch of B = 16 frames, and of the B = 4
// sub-batch BtsModel really enqueues per stream) and profiles/bf16_wide_1x1_bench.json (whole model):
//   block 1, 88x304: 3344 declared workgroups -- x2.05-2.12 at B = 16, x1.65-1.76 at B = 4 (836 real workgroups), every K class
//   block 2, 44x152:  848                     -- x1.62-1.67 at B = 16; at B = 4 (212 real, less than one per CU) +13.5 %, -1.7 %
//                                                (within the spread: the marginal class), +10.0 %
//   block 3, 22x76 :  224                     -- +2.9 % / -3.4 % (both within the spread) / +11.5 % at B = 16, loses 6-28 % at
//                                                B = 4 (56 real workgroups)
//   block 4, 11x38 :   64                     -- loses 45-63 % everywhere
// A 128-pixel tile that owns all 192 channels makes a third of the row-tiled kernel's workgroups: below about one workgroup
// per CU the launch is latency-bound and the narrower tiles fill the chip better.  Whole model, configs[1], four sub-batch
// streams: blocks 1 + 2 on this kernel +6.9 % (+6.7 % in the recorded run), block 1 alone +4.4 %, blocks 1 + 2 + 3 +0.9 %.  The threshold sits between
// block 2 and block 3, at a round number with a meaning rather than at either measured edge.
constexpr long kC1bMinWgs = 512;
inline bool c1b_supported(int c_in, int c_out) { return c_in > 0 && c_out > 0 && (c_out % 192) == 0 && (c_in % 16) == 0; }
inline bool c1b_eligible(int H, int W, int c_in, int c_out, int ff, long* wgs_per_frame) {
    *wgs_per_frame = 0;
    if (H <= 0 || W <= 0 || !c1b_supported(c_in, c_out)) return false;
    *wgs_per_frame = (((long)H * W + C1B_BM - 1) / C1B_BM) * (c_out / 192);
    return (long)ff * *wgs_per_frame >= kC1bMinWgs;
}

// ---- the other widths (bts_conv1x1_bf16_wide_fwd_f32 / _plan; BtsModel.bf16_wide_1x1 = "all")
// Structural: whole 128- or 192-channel N tiles, whole 16-k MFMA blocks.  The tile of bn = 0 is a pure function of c_out: 192
// where it divides c_out (the instantiation measured first), else 128.
//
// Source of everything below: profiles/conv1x1_bf16_wide_bench.txt (scripts/conv1x1_bf16_wide_bench.py: isolated launches
// against the row-tiled bf16 path on the 1x1 layer classes of ResNeXt-101 and ResNet-50 at 416x544 and DenseNet121 at 352x1216,
// fill_frames 16, as the B = 16 launch and as the B = 4 sub-batch launch; a class enters only if it wins by more than the
// run-to-run spread at B = 16 and does not lose at B = 4 -- the rule that set kC1bMinWgs).
//   128 against 256, per width over all of its measured classes: where the tile wins at all, 256 beats 128 at B = 16 on the
//   forms without a residual (+7 ... +45 %), loses 6-22 % on the accepted conv3 classes (residual epilogue at two waves per
//   SIMD), and loses 8-37 % at B = 4 on every 52x68 and 26x34 class but one (half the workgroups).  Every width has classes on
//   which 256 loses at B = 4, so bn = 0 never picks 256; it runs when forced.
//   Tile 128, declared workgroups = fill_frames x ceil(h w / 128) x c_out / 128, and K = c_in (gain at B = 16 / at B = 4):
//     enters: 7104 K256 +17 / +32 %; 3552 K64-256 +9...+53 / +26...+70 % (conv1, conv3, conv3 + skip tap, downsample);
//       3584 K512 +11 / +38 %; 3344 K64-224 +20...+41 / +62...+75 % (DenseNet121 block 1); 1792 K128-512 +15...+28 /
//       -0.2 (within spread) ...+11 %; 1776 K256 +8 / +14 %
//     marginal at B = 4, left out: 896 K512 +36 / +1.0 % (within spread), 896 K256 with residual +38 / -1.7 % (loses), 848
//       K480 +42 / -1.7 % (loses; DenseNet121 block 2) -- although 848 K128 wins +69 / +35 %
//     stays: K >= 992 wherever it was measured -- 1792 K1024 +9 / -5 %, 896 K1024 +23...+26 / -13...-16 %, 512 K2048 -5...-9 /
//       -35...-37 %, 224 K992-1024 -4...-7 / -30...-32 %; and at most 512 declared workgroups -- 512 K512 -2 / -31 %, 448 K512
//       +5 / -8 %, 448 K1024 -5 / -23 %, 128 K2048 -35 / -63 %
//   kC1wMinWgs = 1024 (four workgroups per CU of the declared launch: what the register file holds of this tile) sits between
//   the measured edges 896 (marginal) and 1776 (wins); kC1wMaxK = 512 is the largest K measured to win (the next one measured,
//   992, loses: the K loop is not pipelined deeper than two stages, and nothing else hides a long loop of a small launch).
//   Also left out although it won in isolation: DenseNet121's block 3 at K 256 (224 workgroups, +70 / +52 %) -- the same block
//   loses at K 992 and nothing between was measured.
//   Whole model with these constants (profiles/bf16_wide_1x1_all_bench.json): configs[2] +6.8 %, DenseNet121 +2.5 %, both
//   outside the spread (0.9 %, 0.7 %).
//   Tile 192 with a residual was not measured: refused.
inline bool c1w_supported(int c_in, int c_out) { return c_in > 0 && c_out > 0 && (c_out % 128 == 0 || c_out % 192 == 0) && (c_in % 16) == 0; }
constexpr long kC1wMinWgs = 1024;
constexpr int kC1wMaxK = 512;
inline int c1w_bn(int c_out) { return c_out % 192 == 0 ? 192 : 128; }
inline bool c1w_eligible(int H, int W, int c_in, int c_out, bool has_res, int ff, int* bn, long* wgs_per_frame) {
    *wgs_per_frame = 0; *bn = 0;
    if (H <= 0 || W <= 0 || !c1w_supported(c_in, c_out)) return false;
    const int tile = c1w_bn(c_out);
    const long wgs = (((long)H * W + C1B_BM - 1) / C1B_BM) * (c_out / tile);
    const bool ok = tile == 192 ? (!has_res && (long)ff * wgs >= kC1bMinWgs) : ((long)ff * wgs >= kC1wMinWgs && c_in <= kC1wMaxK);
    if (!ok) return false;
    *bn = tile; *wgs_per_frame = wgs;
    return true;
}

template <int BN>
int launch_conv1x1_bf16(Conv1x1Bf16Args a, const ConvRun& r, bool y_bf16 = false) {
    const long n_mtiles = (a.npix + C1B_BM - 1) / C1B_BM;
    a.n_ntiles = a.c_out / BN;
    const long nwg = n_mtiles * a.n_ntiles;
    const size_t lds = c1b_lds_bytes<BN>(a.c_in, a.pre_scale != nullptr);
    if constexpr (BN == 192) {               // the bf16 destination: a.y holds bf16, a.y_pix_stride counts bf16 elements
        if (y_bf16) return conv_launch<conv1x1_bf16_ybf16_kernel<BN>>(r, ConvChoice{}, BTS_ERR_UNSUPPORTED, nwg, nwg, 256, lds, a);
    }
    if (a.res != nullptr || a.y2 != nullptr)
        return conv_launch<conv1x1_bf16_epi_kernel<BN>>(r, ConvChoice{}, BTS_ERR_UNSUPPORTED, nwg, nwg, 256, lds, a);
    return conv_launch<conv1x1_bf16_kernel<BN>>(r, ConvChoice{}, BTS_ERR_UNSUPPORTED, nwg, nwg, 256, lds, a);
}
