// Planar-tail 3x3 convolution (decoder conv3 / conv2) with bf16 main operands: the one-plane bf16 halo tile of
// conv_halo_emu.inc (halo_emu_produce / halo_emu_consume with KS 3, NP 1: the mechanism is documented there) over the MAIN
// channels, plus the one-plane tail added in fp32 before the epilogue.  Included by conv_mfma.hip inside its anonymous
// namespace, after conv_halo_emu.inc.  Opt-in: its own entry point (bts_conv_tail_bf16_fwd_f32); bts_conv_fwd_f32 keeps these
// layers on conv_halo_kernel<..., tail> whatever `precision` says.
//
//   y[b][y][x][n] = e2(act( sum_{tap,c<c_main} bf16(x[b][y+dy][x+dx][c]) * w_main[n][tap*c_main + c]      (fp32 accumulation)
//                         + sum_tap t[b][y+dy][x+dx] * w_tail[n][tap][0] ))                               (fp32 FMAs, unrounded)
//
// What differs from conv_halo_emu_kernel<BN, 3, 1>:
//   * WEIGHTS are two operands of their own.  The layer's packed K axis is tap * (c_main + 4) + c, which puts the main block
//     of an odd tap at a byte offset that is no multiple of 16 in a bf16 plane; w_main is re-laid as [c_out_pad][9 * c_main]
//     (k = tap * c_main + c), so every tap-step's 64-byte DMA rows are 16-byte aligned.  w_tail is fp32 [c_out_pad][9][4].
//   * NO prologue affine: a patch pass is ONE untracked load, not three, and holds four registers, not twelve.
//   * THE TAIL: the producers stage the tile's 6 x 34 plane values (zero outside the map) into LDS once, before the first
//     barrier.  After the K loop a consumer lane reads, per four adjacent outputs, the 3 x 6 plane values they share (a
//     broadcast read: the address depends on the lane's k-half only) and adds nine fp32 FMAs per output and channel tile.
//   * TWO workgroups per CU (one's prologue, tail and epilogue run under the other's MFMAs): four waves per SIMD, so a
//     128-register budget, which both instantiations meet without scratch (DESIGN 3c), and at most 80 KB of LDS.
struct TailBf16Args {
    const float* x; long x_pix_stride; int B, H, W, c_main;
    const unsigned short* w_main;                 // bf16 [c_out_pad][9 * c_main]
    const float* w_tail;                          // fp32 [c_out_pad][9][4]
    const float* tail;                            // plane [B][H][W]
    int c_out, c_out_pad;
    const float* e2_scale; const float* e2_shift; int act;
    float* y; long y_pix_stride;
    int n_ntiles;
};

template <int BN>
constexpr int tail_bf16_lds_bytes() { return HaloEmuGeom<BN, 3, 1>::LDS_BYTES + HaloEmuGeom<BN, 3, 1>::NPIX * 4; }      // ... then Ts

// One consumer wave's 2 x TN accumulator tiles to the NHWC slice (store_tiles_nhwc's addressing: a wave-uniform 64-bit row
// base plus one per-lane 32-bit offset per column tile)
template <int ACT, int TM, int TN, typename AccT>
__device__ __forceinline__ void tail_bf16_store(const TailBf16Args& a, const AccT (&acc)[TM][TN], const long (&pix0)[TM],
                                                const int (&nvalid)[TM], int ncol0, int li, int lh) {
#pragma unroll
    for (int j = 0; j < TN; ++j) {
        const int n = ncol0 + j * 32 + li;
        const bool nok = n < a.c_out;
        float s2 = (a.e2_scale != nullptr && nok) ? a.e2_scale[n] : 1.f;
        float b2 = (a.e2_scale != nullptr && nok) ? a.e2_shift[n] : 0.f;
        // An unconditional use of the two loaded values: the compiler waits for them HERE, once.  Left to their first use
        // inside a masked store block, every such block gets its own s_waitcnt vmcnt(0) -- which on gfx9 also waits for the
        // previous block's STORE, so the 64 stores of a lane would run one memory round trip after the other.
        asm volatile("" : "+v"(s2), "+v"(b2));
        const unsigned lane_y = (unsigned)(4 * lh) * (unsigned)a.y_pix_stride + (unsigned)n;
#pragma unroll
        for (int i = 0; i < TM; ++i) {
            float* const yb = a.y + pix0[i] * a.y_pix_stride;                           // wave-uniform
            const int nv = nvalid[i] - 4 * lh;                                          // slots this lane's half may write
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int qu = (r & 3) + 8 * (r >> 2);
                float v = act_fn<ACT>(acc[i][j][r]);
                v = fmaf(v, s2, b2);
                if (nok && qu < nv) (yb + (long)qu * a.y_pix_stride)[lane_y] = v;
            }
        }
    }
}

template <int BN>
__global__ __launch_bounds__(512, 4) void conv_tail_bf16_kernel(const TailBf16Args a) {
    using G = HaloEmuGeom<BN, 3, 1>;
    constexpr int KS = 3, MF = 32, TM = 2, TN = BN / 2 / MF, PW = G::PW, NPIX = G::NPIX, T = KS * KS;
    static_assert(TN >= 1, "layout");
    typedef float acc_t __attribute__((ext_vector_type(16)));
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    char* const As = smem_raw;
    char* const Bs = smem_raw + 2 * G::A_BUF;
    float* const Ts = reinterpret_cast<float*>(smem_raw + G::LDS_BYTES);      // [6][34] plane values of the tile

    const Tile4x32 tile = decode_tile_4x32<BN>(xcd_swizzle(blockIdx.x, gridDim.x), a.n_ntiles, a.H, a.W);
    const int n0 = tile.n0, bfr = tile.bfr, y0 = tile.y0, x0 = tile.x0;

    const int tid = threadIdx.x;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
    const int nchunks = a.c_main / BK;                    // host: c_main % 32 == 0

    if (wv >= 4) {
        const HaloEmuSource src = {a.x, (unsigned)a.x_pix_stride, a.H, a.W, bfr, y0, x0, 1, 1, nullptr, nullptr, false, 0,
                                   a.w_main, a.c_out_pad, T * a.c_main, a.c_main, n0, nchunks};
        halo_emu_produce<BN, KS, 1, false>(src, As, Bs, tid, wv, [&] {      // the tile's plane values
            const int ptid = tid - 256;
            if (ptid < NPIX) {
                const int pyy = ptid / PW, pxx = ptid - pyy * PW;
                const int gy = y0 - 1 + pyy, gx = x0 - 1 + pxx;
                const bool ok = (unsigned)gy < (unsigned)a.H && (unsigned)gx < (unsigned)a.W;
                const int yc = min(max(gy, 0), a.H - 1), xc = min(max(gx, 0), a.W - 1);
                const float tv = a.tail[((long)bfr * a.H + yc) * a.W + xc];
                Ts[ptid] = ok ? tv : 0.f;
            }
        });
        return;
    }

    const int cm = wv >> 1, cn = wv & 1;
    const int li = lane & 31, lh = lane >> 5;
    acc_t acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
    halo_emu_consume<1, TM, TN, KS, G::A_PLANE, G::B_PLANE>(As, Bs, nchunks, cm, cn, li, lh, acc);

    // ---------------------------------------------------------------- the tail plane, fp32: acc += sum_tap w_tail[n][tap][0] * t
    // Accumulator register r = 4 g + rl of row tile i is output (row cm*2 + i, column 8 g + 4 lh + rl) of the tile: the four
    // outputs of a group share the 3 x 6 plane values at patch rows row..row+2, columns col..col+5 (Ts was written before the
    // first barrier and is never overwritten).
    {
        float wt[TN][T];
#pragma unroll
        for (int j = 0; j < TN; ++j) {
            int n = n0 + (cn * TN + j) * MF + li;
            n = n < a.c_out_pad ? n : a.c_out_pad - 1;
#pragma unroll
            for (int tap = 0; tap < T; ++tap) wt[j][tap] = a.w_tail[((long)n * T + tap) * 4];
        }
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const float* const tp = Ts + (cm * TM + i) * PW + 8 * g + 4 * lh;
                float tv[KS][6];
#pragma unroll
                for (int dy = 0; dy < KS; ++dy)
#pragma unroll
                    for (int c = 0; c < 6; ++c) tv[dy][c] = tp[dy * PW + c];
#pragma unroll
                for (int rl = 0; rl < 4; ++rl)
#pragma unroll
                    for (int j = 0; j < TN; ++j) {
                        float v = acc[i][j][4 * g + rl];
#pragma unroll
                        for (int tap = 0; tap < T; ++tap) v = fmaf(wt[j][tap], tv[tap / KS][rl + tap % KS], v);
                        acc[i][j][4 * g + rl] = v;
                    }
            }
    }

    // ---------------------------------------------------------------- epilogue (NHWC slice)
    const int cms = __builtin_amdgcn_readfirstlane(cm), cns = __builtin_amdgcn_readfirstlane(cn);
    const int xleft = a.W - x0;
    long pix0[TM];
    int nvalid[TM];
#pragma unroll
    for (int i = 0; i < TM; ++i) {
        const int y = y0 + cms * TM + i;
        pix0[i] = ((long)bfr * a.H + y) * a.W + x0;
        nvalid[i] = y < a.H ? (xleft >= MF ? MF : xleft) : 0;
    }
    const int ncol0 = n0 + cns * TN * MF;
    dispatch_act(a.act, [&](auto act) { tail_bf16_store<decltype(act)::value, TM, TN>(a, acc, pix0, nvalid, ncol0, li, lh); });
}

// The layers the decoder hands to this kernel (bts_conv_tail_bf16_plan).  From the bf16 halo tile: whole 32-channel chunks
// and a 4 x 32 tile grid that is at least 0.80 real pixels (halo_eligible).  NOT from it: the declared-launch minimum
// (kFillWgs) -- there it separates the halo tile from split-K, and a planar-tail layer never splits K: the fp32 kernel it
// would otherwise take walks the same 4 x 32 tile grid, so the launch size does not tell the two apart.  c_out >= 64: the
// narrowest tile is 64 channels wide.
constexpr double kTailBf16MinFill = 0.80;
inline int tail_bf16_bn(int c_out) { return c_out >= 128 ? 128 : 64; }
inline bool tail_bf16_eligible(int H, int W, int c_main, int c_out, int n_tail, long* wgs_per_frame) {
    *wgs_per_frame = 0;
    if (H <= 0 || W <= 0 || c_main <= 0 || (c_main % BK) || c_out < 64 || n_tail != 1) return false;
    const int bn = tail_bf16_bn(c_out);
    double fill;
    *wgs_per_frame = tiles_4x32(H, W, &fill) * ((c_out + bn - 1) / bn);
    return fill >= kTailBf16MinFill;
}

template <int BN>
int launch_tail_bf16(TailBf16Args a, const ConvRun& r) {
    const long n_mtiles = (long)a.B * tiles_4x32(a.H, a.W);
    a.n_ntiles = (a.c_out + BN - 1) / BN;
    const long nwg = n_mtiles * a.n_ntiles;
    constexpr size_t lds = (size_t)tail_bf16_lds_bytes<BN>();
    static_assert(lds <= 80 * 1024, "two workgroups per CU");
    return conv_launch<conv_tail_bf16_kernel<BN>>(r, ConvChoice{}, BTS_ERR_UNSUPPORTED, nwg, nwg, 512, lds, a);
}
