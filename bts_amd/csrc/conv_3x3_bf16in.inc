// 3x3 convolution (stride 1, padding 1) whose INPUT is a bf16 NHWC tensor: the growth convolution of a dense layer reading the
// bottleneck intermediate that bts_conv1x1_bf16_fwd_bf16 stored as bf16 (BtsModel.bf16_mid_storage).  The one-plane bf16 halo
// tile of conv_halo_emu.inc (halo_emu_produce / halo_emu_consume with KS 3, NP 1: the mechanism is documented there), built
// as conv_tail_bf16_kernel is.  Included by conv_mfma.hip inside its anonymous namespace, after conv_tail_bf16.inc.  Opt-in:
// its own entry point (bts_conv3x3_bf16in_fwd_f32); bts_conv_fwd_f32 never launches it.
//
//   y[b][y][x][n] = act( e1( sum_{tap, c < c_in} x[b][y+dy][x+dx][c] * w[n][tap * c_in + c] ) )         (fp32 accumulation)
//
// What differs from conv_halo_emu_kernel<BN, 3, 1>, which runs the same layer from an fp32 tensor:
//   * THE PATCH SOURCE (halo_emu_produce's XBF16): a pass is one untracked 8-byte load of the thread's four channels
//     instead of a 16-byte one plus the two prologue vectors, and store_a copies the 8 bytes (zeroed outside the image) into
//     the swizzled LDS slot plane_store<1> would have rounded them into.  When the tensor holds RNE(v) for the fp32 value v
//     the sibling would have read, LDS holds the same bits in both kernels; consumer, sum order (chunk-major, nine taps per
//     chunk, two 16-k MFMA blocks per tap) and epilogue are the sibling's, so every output bit is.
//   * NO prologue: three loads per pass become one, twelve registers four -- two.
//   * WAIT COUNTS: untouched.  vmcnt counts vector-memory operations, and a pass is still ONE unconditional, clamped
//     operation (LPP = 1, as in conv_tail_bf16_kernel); the weight DMA ring, its NIW operations per step, the counted waits
//     and the raw barriers are halo_emu_produce's own code, shared with both siblings, and not a line of them depends on
//     the source flag.  A clamped load reads channels [32 chunk + lk, + 4) < c_in of a pixel inside the map: never past a
//     channel-prefix view's c_in, never outside the tensor.
//   * The epilogue computes what conv_halo_emu_kernel's NHWC fast path (store_tiles_nhwc) computes -- fma(acc, s1, b1), the
//     activation, then that path's identity e2 as the fma(v, 1, 0) it is there (-0 becomes +0 in both) -- with
//     tail_bf16_store's addressing and its one wait for the two vectors: left to store_tiles_nhwc, every masked store block
//     waits vmcnt(0), which on gfx9 also waits for the previous block's store (253 such waits in the sibling at BN 64).
//
// gfx950 (-Rpass-analysis=kernel-resource-usage), registers / waves per SIMD / scratch / LDS:
//   BN 64: 87 / 5 / 0 / 38400 B        BN 128: 120 / 4 / 0 / 50688 B      (two eight-wave workgroups per CU; the sibling: 124 / 4
//   and 227 / 2 -- its producer holds the prologue's twelve registers per pass)
struct Conv3x3Bf16InArgs {
    const unsigned short* x; long x_pix_stride; int B, H, W, c_in;      // bf16 NHWC, stride in bf16 elements
    const unsigned short* w; int k_pad;           // bf16 [c_out_pad][k_pad], k = tap * c_in + c
    int c_out, c_out_pad;
    const float* e1_scale; const float* e1_shift; int act;
    float* y; long y_pix_stride;
    int n_ntiles;
};

// One consumer wave's 2 x TN accumulator tiles to the NHWC slice (tail_bf16_store's addressing; store_tiles_nhwc's values)
template <int ACT, int TM, int TN, typename AccT>
__device__ __forceinline__ void bf16in_store(const Conv3x3Bf16InArgs& a, const AccT (&acc)[TM][TN], const long (&pix0)[TM],
                                             const int (&nvalid)[TM], int ncol0, int li, int lh) {
#pragma unroll
    for (int j = 0; j < TN; ++j) {
        const int n = ncol0 + j * 32 + li;
        const bool nok = n < a.c_out, in = n < a.c_out_pad;
        float s1 = (a.e1_scale != nullptr && in) ? a.e1_scale[n] : 1.f;
        float b1 = (a.e1_scale != nullptr && in) ? a.e1_shift[n] : 0.f;
        float s2 = 1.f, b2 = 0.f;                       // the sibling's absent e2: an fma all the same
        asm volatile("" : "+v"(s1), "+v"(b1), "+v"(s2), "+v"(b2));      // waited for HERE, once (see tail_bf16_store)
        const unsigned lane_y = (unsigned)(4 * lh) * (unsigned)a.y_pix_stride + (unsigned)n;
#pragma unroll
        for (int i = 0; i < TM; ++i) {
            float* const yb = a.y + pix0[i] * a.y_pix_stride;                           // wave-uniform
            const int nv = nvalid[i] - 4 * lh;                                          // slots this lane's half may write
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int qu = (r & 3) + 8 * (r >> 2);
                float v = fmaf(acc[i][j][r], s1, b1);
                v = act_fn<ACT>(v);
                v = fmaf(v, s2, b2);
                if (nok && qu < nv) (yb + (long)qu * a.y_pix_stride)[lane_y] = v;
            }
        }
    }
}

template <int BN>
__global__ __launch_bounds__(512, 2) void conv3x3_bf16in_kernel(const Conv3x3Bf16InArgs a) {
    using G = HaloEmuGeom<BN, 3, 1>;
    constexpr int KS = 3, MF = 32, TM = 2, TN = BN / 2 / MF;
    static_assert(TN >= 1, "layout");
    typedef float acc_t __attribute__((ext_vector_type(16)));
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    char* const As = smem_raw;
    char* const Bs = smem_raw + 2 * G::A_BUF;

    const Tile4x32 tile = decode_tile_4x32<BN>(xcd_swizzle(blockIdx.x, gridDim.x), a.n_ntiles, a.H, a.W);
    const int n0 = tile.n0, bfr = tile.bfr, y0 = tile.y0, x0 = tile.x0;

    const int tid = threadIdx.x;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
    const int nchunks = a.c_in / BK;                      // host: c_in % 32 == 0

    if (wv >= 4) {
        const HaloEmuSource src = {reinterpret_cast<const float*>(a.x), (unsigned)a.x_pix_stride, a.H, a.W, bfr, y0, x0, 1, 1,
                                   nullptr, nullptr, false, 0, a.w, a.c_out_pad, a.k_pad, a.c_in, n0, nchunks};
        halo_emu_produce<BN, KS, 1, false, true>(src, As, Bs, tid, wv, [] {});
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
    dispatch_act(a.act, [&](auto act) { bf16in_store<decltype(act)::value, TM, TN>(a, acc, pix0, nvalid, ncol0, li, lh); });
}

// The layers the encoder hands to this kernel (bts_conv3x3_bf16in_plan): exactly those bts_conv_plan_f32 sends to
// BTS_CONV_KIND_HALO_BF16 at precision 2 -- the plan query asks conv_plan itself, with a split-K workspace lent (the encoder
// lends one; without one the dispatch only becomes more willing), so the two cannot drift apart.  The measured table stands
// next to the query (conv_mfma.hip): no class it admits loses, so it has no threshold of its own.
template <int BN>
int launch_conv3x3_bf16in(Conv3x3Bf16InArgs a, const ConvRun& r) {
    const long n_mtiles = (long)a.B * tiles_4x32(a.H, a.W);
    a.n_ntiles = (a.c_out + BN - 1) / BN;
    const long nwg = n_mtiles * a.n_ntiles;
    constexpr size_t lds = (size_t)HaloEmuGeom<BN, 3, 1>::LDS_BYTES;
    static_assert(lds <= 80 * 1024, "two workgroups per CU");
    return conv_launch<conv3x3_bf16in_kernel<BN>>(r, ConvChoice{}, BTS_ERR_UNSUPPORTED, nwg, nwg, 512, lds, a);
}
