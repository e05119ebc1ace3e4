// Encoder stem: 7x7 stride-2 convolution of the 3-channel image (torchvision features.conv0 / conv1, walked by
// reference pytorch/bts.py:327-338) -- included by conv_mfma.hip inside its anonymous namespace.
//
// On the generic kernel the stem is the worst-priced launch of the forward (0.31 of the MFMA roof): its K axis is
// 49 taps x 4 channels (3 real + 1 pad), so every lane decodes its own tap per staged f32x4, the 96 output channels
// take two N tiles that gather the same pixels twice, and a quarter of every MFMA multiplies the pad channel.
// Everything about this layer is static, so here:
//   * the WHOLE weight matrix [c_out][224] sits in LDS (88 KB for 96 channels), staged once per workgroup; workgroups
//     are persistent and walk output tiles of 8 rows x 32 pixels (one row per wave, all channels per wave);
//   * the input patch with halo (21 x 69 pixels x 4 channels, 27 KB) is staged once per tile, de-interleaved into an
//     even-x and an odd-x plane: the stride-2 taps of 32 consecutive output pixels are then 32 consecutive 16-byte
//     pixels of one plane -- the A fragment of tap (ky,kx) is ONE conflict-free ds_read_b128 at
//     plane(kx&1)[row 2r+ky][ox + kx/2], no im2col expansion;
//   * a fragment's four k are the pixel's four channels, so MFMA k-step q = channel q and the pad channel's step (q = 3)
//     is simply not issued when every weight of channel 3 is zero (checked while staging): 150 k per output instead of 224;
//   * the next tile's patch is loaded into registers before the MFMA loop and written to the other LDS buffer after it.
// K order: k = tap*4 + c ascending, as the generic kernel's packed weights (ops.pack_conv_weight, c_in_ld = 4).
template <int BN>
__global__ __launch_bounds__(512, 1) void conv_stem_kernel(const ConvArgs a, int n_ty, int n_tx, int n_tiles) {
    constexpr int TN = BN / 32, TH = 8, TW = 32;
    constexpr int PR = 2 * TH + 5, PC = 2 * TW + 5;            // patch rows / pixels per row: 21 x 69
    constexpr int PLANE = 160, ROW = 2 * PLANE;                // floats: 40 pixels per parity plane (35 / 34 used); 640 B = the other half of the banks
    constexpr int A_FLOATS = PR * ROW;
    constexpr int KP = 224, WLD = 228;                         // packed K, LDS row (57 x 16 B: rows land on distinct 16-B slots)
    constexpr int NPASS = (PR * PC + 511) / 512;               // 3
    typedef float acc_t __attribute__((ext_vector_type(16)));
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    float* const Ws = reinterpret_cast<float*>(smem_raw);      // [BN][WLD]
    float* const As = Ws + BN * WLD;                           // [2][PR][2][PLANE]

    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int li = lane & 31, lh = lane >> 5;
    int w3_nonzero = 0;                                         // does any weight of input channel 3 differ from zero?
    for (int i = tid; i < BN * (KP / 4); i += 512) {
        const int n = i / (KP / 4), k4 = i - n * (KP / 4);
        const f32x4 wv4 = *reinterpret_cast<const f32x4*>(a.w + (size_t)n * a.k_pad + 4 * k4);
        *reinterpret_cast<f32x4*>(Ws + n * WLD + 4 * k4) = wv4;
        w3_nonzero |= (wv4.w != 0.f) ? 1 : 0;
    }
    // the image has 3 real channels (4th = layout padding, zero weights): its k-step is then never issued; a caller
    // with four real channels gets all four (workgroup-uniform: every workgroup reads the same weights)
    const bool four_channels = __syncthreads_or(w3_nonzero) != 0;
    // this thread's patch elements: e = tid + 512 p -> (row, xi); LDS slot = plane (xi & 1), pixel xi >> 1
    int prow[NPASS], pxi[NPASS], plds[NPASS];
#pragma unroll
    for (int p = 0; p < NPASS; ++p) {
        const int e = min(tid + 512 * p, PR * PC - 1);
        prow[p] = e / PC; pxi[p] = e - prow[p] * PC;
        plds[p] = prow[p] * ROW + (pxi[p] & 1) * PLANE + (pxi[p] >> 1) * 4;
    }
    const int tiles_per_frame = n_ty * n_tx;
    auto load_patch = [&](int tile, f32x4 (&v)[NPASS], unsigned& ok) {
        const int b = tile / tiles_per_frame, tr = tile - b * tiles_per_frame;
        const int ty = tr / n_tx, y0 = ty * TH, x0 = (tr - ty * n_tx) * TW;
        unsigned m = 0;
#pragma unroll
        for (int p = 0; p < NPASS; ++p) {
            const int gy = 2 * y0 - 3 + prow[p], gx = 2 * x0 - 3 + pxi[p];
            const bool in = (unsigned)gy < (unsigned)a.h_in && (unsigned)gx < (unsigned)a.w_in && tid + 512 * p < PR * PC;
            const int yc = min(max(gy, 0), a.h_in - 1), xc = min(max(gx, 0), a.w_in - 1);
            v[p] = *reinterpret_cast<const f32x4*>(a.x + ((size_t)b * a.h_in * a.w_in + (size_t)yc * a.w_in + xc) * (size_t)a.x_pix_stride);
            m |= (in ? 1u : 0u) << p;
        }
        ok = m;
    };
    auto store_patch = [&](float* buf, const f32x4 (&v)[NPASS], unsigned ok) {
#pragma unroll
        for (int p = 0; p < NPASS; ++p) {
            f32x4 t = v[p];
            asm volatile("" : "+v"(t));                         // first use of the loaded value pinned here (conv_halo.inc)
            const bool in = (ok >> p) & 1u;                     // zero padding
            t.x = in ? t.x : 0.f; t.y = in ? t.y : 0.f; t.z = in ? t.z : 0.f; t.w = in ? t.w : 0.f;
            if (tid + 512 * p < PR * PC) *reinterpret_cast<f32x4*>(buf + plds[p]) = t;
        }
    };

    int tile = blockIdx.x;
    f32x4 pv[NPASS];
    unsigned pok = 0;
    if (tile < n_tiles) {
        load_patch(tile, pv, pok);
        store_patch(As, pv, pok);
    }
    __syncthreads();                                           // (the weights were already fenced by __syncthreads_or)

    // per-lane fragment bases: A = output pixel (row wv, column li) of the tile; B = channel li of each 32-wide N tile
    const float* const a_lane = As + (2 * wv) * ROW + li * 4;
    const float* const b_lane = Ws + li * WLD + 4 * lh;
    const int wvs = __builtin_amdgcn_readfirstlane(wv);
    int cur = 0;
    for (; tile < n_tiles; tile += gridDim.x) {
        const int nxt = tile + gridDim.x;
        load_patch(min(nxt, n_tiles - 1), pv, pok);            // unconditional, clamped: lands under the MFMA loop
        acc_t acc[1][TN];
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[0][j][r] = 0.f;
        const float* const ab = a_lane + cur * A_FLOATS;
        auto mfma_loop = [&](auto nq_tag) __attribute__((always_inline)) {
            constexpr int NQ = decltype(nq_tag)::value;         // k-steps per tap = input channels multiplied
#pragma unroll
            for (int g = 0; g < 25; ++g) {
                // taps 2g (lanes 0-31) and 2g+1 (lanes 32-63); tap 49 does not exist: its weights are zero, read tap 48's pixels
                const int t0 = 2 * g, t1 = 2 * g + 1 < 49 ? 2 * g + 1 : 48;
                const int o0 = (t0 / 7) * ROW + ((t0 % 7) & 1) * PLANE + ((t0 % 7) >> 1) * 4;
                const int o1 = (t1 / 7) * ROW + ((t1 % 7) & 1) * PLANE + ((t1 % 7) >> 1) * 4;
                const f32x4 fa = *reinterpret_cast<const f32x4*>(ab + (lh ? o1 : o0));
                f32x4 fb[TN];
#pragma unroll
                for (int j = 0; j < TN; ++j) fb[j] = *reinterpret_cast<const f32x4*>(b_lane + j * 32 * WLD + 8 * g);
#pragma unroll
                for (int q = 0; q < NQ; ++q)                    // q = input channel
#pragma unroll
                    for (int j = 0; j < TN; ++j)
                        acc[0][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[q], fb[j][q], acc[0][j], 0, 0, 0);
            }
        };
        if (four_channels) mfma_loop(std::integral_constant<int, 4>{});
        else               mfma_loop(std::integral_constant<int, 3>{});
        if (nxt < n_tiles) store_patch(As + (cur ^ 1) * A_FLOATS, pv, pok);
        {   // epilogue: row tile = 32 consecutive pixels of output row y0 + wv
            const int b = tile / tiles_per_frame, tr = tile - b * tiles_per_frame;
            const int ty = tr / n_tx, y = ty * TH + wvs, x0 = (tr - ty * n_tx) * TW;
            long pix0[1] = {((long)b * a.H + y) * a.W + x0};
            const int xleft = a.W - x0;
            int nvalid[1] = {y < a.H ? (xleft >= 32 ? 32 : xleft) : 0};
            fast_epilogue_nhwc<1, TN, 32, 16>(a, acc, pix0, nvalid, 1, 0, li, lh);     // dispatch guarantees the fast path
        }
        __syncthreads();
        cur ^= 1;
    }
}

// 7x7 / stride 2 / pad 3 over a 4-channel-padded NHWC image, 64 or 96 output channels, BN(+ReLU) epilogue, NHWC out
inline bool stem_eligible(const ConvArgs& a, bool nchw, int prec) {
    return prec != 1 && !nchw && a.ksize == 7 && a.stride == 2 && a.pad == 3 && a.dil == 1 && a.ups == 0 && !a.subpix && !a.bundled &&
           a.c_in_ld == 4 && a.k_pad == 224 && (a.c_out == 96 || a.c_out == 64) && a.c_out_pad == a.c_out &&
           a.pre_scale == nullptr && a.res == nullptr && a.act != 3 && a.n_tail == 0 &&
           (double)32 * (double)(a.y_pix_stride > a.y2_pix_stride ? a.y_pix_stride : a.y2_pix_stride) < 2147483648.0;
}

template <int BN>
int launch_stem(const ConvArgs& a0, const ConvRun& r) {
    ConvArgs a = a0;
    const int n_ty = (a.H + 7) / 8, n_tx = (a.W + 31) / 32;
    const long n_tiles = (long)a.B * n_ty * n_tx;
    a.n_ntiles = 1; a.tiles_per_class = (int)n_tiles; a.ksplit = 1;
    const size_t lds = (size_t)(BN * 228 + 2 * 21 * 320) * sizeof(float);
    const long nwg = n_tiles < 256 ? n_tiles : 256;            // persistent: one workgroup per CU of the MI355X (141 KB of LDS each)
    return conv_launch<conv_stem_kernel<BN>>(r, ConvChoice{BTS_CONV_KIND_STEM, 256, BN, 1}, BTS_ERR_INVALID, n_tiles, nwg, 512, lds,
                                             a, n_ty, n_tx, (int)n_tiles);
}
