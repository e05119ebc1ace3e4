// Wide-tile 1x1 convolution (included by conv_mfma.hip inside its anonymous namespace, after conv_halo.inc).
//
// A 1x1 convolution has no taps to share an input patch between, so what the halo-tile kernel saves for the 3x3
// layers -- input staging work per MFMA -- has to come from the other direction: ONE workgroup computes ALL (or 128/256
// of) the output channels of its 128 pixels, so the input tile, and the BN+ReLU prologue applied to it, is staged once
// instead of once per 64-wide N tile.  DenseNet bottlenecks (c_out 192 = 4 x growth 48: 108 launches per forward,
// a quarter of the step) ran as three 128x64 tiles per pixel tile: 3 staged f32x4 per thread per 16 MFMAs; here a
// 128x192 tile stages 5 per 48 MFMAs -- the halo kernel's ratio -- with the same pipeline rules (every load
// unconditional with clamped indices, every ds_write before any new load, first use of a staged register pinned).
// Eight waves as 4 (pixels) x 2 (channels): a wave owns 32 pixels x BN/2 channels (TN = BN/64 accumulators).
// The K order is the row-tiled kernel's (ascending channel, same fragment layout), so for a given layer both kernels
// produce the same bits.
// Measured: steady state 113 TFLOP/s (DenseNet block 1), but a fixed ~190 us per block-1 layer on top (first-load latency
// and the drain of 96 KB of output stores per workgroup, nothing else resident on the CU to hide them).  A persistent
// variant with a cross-tile software pipeline did NOT recover it: on gfx950 stores count in the same in-order vmcnt as
// loads, so the next tile's first wait for a load also waits for the previous tile's stores.
// SB (single B buffer; the 64-row tile's default): the weight tile [BN][32] is kept ONCE in LDS, the input tile stays
// double-buffered: 46 instead of 74 KB, THREE four-wave workgroups per CU instead of two, which is what a 3-11-step K loop
// needs to hide its neighbours' first-load latency and output stores (fixed cost per tile round, measured on block 1:
// ~9.6 us against 3.1 us per K-step).  The price is a second barrier per K-step: the next step's tiles are written after
// every wave holds its LAST fragments of the current step in registers (barrier), in the shadow of the step's last MFMA
// group, and become visible at the step's end (barrier).  Block 1 / 2 bottlenecks: -3 ... -11 % per layer (K = 720 ... 96).
// Measured and dropped: the same for the 128-row tile (two eight-wave workgroups per CU: no gain), and ONE buffer for both
// tiles (37 KB, four workgroups per CU: twice as slow).
template <int BN, int WM = 4, bool SB = false>
__global__ __launch_bounds__(WM * 128, (SB && WM == 2 ? 3 : 2)) void conv1x1_kernel(const ConvArgs a) {
    constexpr int NT = WM * 128, BM = WM * 32, MF = 32, WN = 2;
    constexpr int RPP = NT / 8;                       // tile rows staged per pass
    constexpr int PA = BM / RPP, PB = BN / RPP;
    constexpr int TN = BN / WN / MF;                  // accumulators per wave (TM = 1)
    constexpr int LDS_LD = LdsLd<MF>::value;
    constexpr int A_FLOATS = BM * LDS_LD, B_FLOATS = BN * LDS_LD;
    constexpr int KG = 256 / MF, NG = BK / KG;        // 8 k per fragment group, 4 groups per step
    static_assert(BN % (WN * MF) == 0 && BN % RPP == 0, "tile/wave layout");
    typedef float acc_t __attribute__((ext_vector_type(16)));
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    float* const As = reinterpret_cast<float*>(smem_raw);          // [2][BM][LDS_LD]
    constexpr int B_STRIDE = SB ? 0 : B_FLOATS;                    // distance between the two B buffers (0: one buffer)
    float* const Bs = As + 2 * A_FLOATS;                           // [2 or 1][BN][LDS_LD]

    const int nwg = gridDim.x, bid = blockIdx.x;
    const int swz = xcd_swizzle(bid, nwg);
    const int mt_idx = swz / a.n_ntiles, nt_idx = swz - mt_idx * a.n_ntiles;
    const long m0 = (long)mt_idx * BM;
    const int n0 = nt_idx * BN;

    const int tid = threadIdx.x;
    const int lrow = tid >> 3, lk = (tid & 7) * 4;
    const int nsteps = (a.c_in_ld + BK - 1) / BK;
    const int ng_last = (a.c_in_ld - (nsteps - 1) * BK + KG - 1) / KG;

    unsigned abase[PA], avalid = 0;
#pragma unroll
    for (int p = 0; p < PA; ++p) {
        const long m = m0 + p * RPP + lrow;
        const bool v = m < a.M;
        avalid |= (v ? 1u : 0u) << p;
        abase[p] = (unsigned)(v ? m : 0) * (unsigned)a.x_pix_stride;      // host: every element offset < 2^32
    }
    unsigned wrow[PB];
#pragma unroll
    for (int p = 0; p < PB; ++p) {
        int n = n0 + p * RPP + lrow;
        n = n < a.c_out_pad ? n : a.c_out_pad - 1;
        wrow[p] = (unsigned)n * (unsigned)a.k_pad;
    }
    const bool has_pre = a.pre_scale != nullptr;

    f32x4 ra[PA], rb[PB], ps = {1.f, 1.f, 1.f, 1.f}, pb = {0.f, 0.f, 0.f, 0.f};
    auto load_step = [&](int step) {                   // loads only: clamped channel offset, nothing touches the values
        const int c = step * BK + lk;
        const unsigned cs = c < a.c_in_ld ? (unsigned)c : 0u;
#pragma unroll
        for (int p = 0; p < PA; ++p) ra[p] = *reinterpret_cast<const f32x4*>(a.x + (abase[p] + cs));
        if (has_pre) {
            ps = *reinterpret_cast<const f32x4*>(a.pre_scale + cs);
            pb = *reinterpret_cast<const f32x4*>(a.pre_shift + cs);
        }
#pragma unroll
        for (int p = 0; p < PB; ++p) rb[p] = *reinterpret_cast<const f32x4*>(a.w + (wrow[p] + cs));
    };
    auto store_step = [&](int step, float* adst, float* bdst) {
        const bool cok = step * BK + lk < a.c_in_ld;
        f32x4 s4 = ps, b4 = pb;
        if (has_pre) asm volatile("" : "+v"(s4), "+v"(b4));
#pragma unroll
        for (int p = 0; p < PA; ++p) {
            f32x4 v = ra[p];
            asm volatile("" : "+v"(v));                // first use pinned here (see conv_halo.inc)
            if (has_pre) v = v * s4 + b4;
            if (a.pre_relu) { v.x = fmaxf(v.x, 0.f); v.y = fmaxf(v.y, 0.f); v.z = fmaxf(v.z, 0.f); v.w = fmaxf(v.w, 0.f); }
            const bool ok = cok && ((avalid >> p) & 1u);
            v.x = ok ? v.x : 0.f; v.y = ok ? v.y : 0.f; v.z = ok ? v.z : 0.f; v.w = ok ? v.w : 0.f;
            *reinterpret_cast<f32x4*>(adst + (p * RPP + lrow) * LDS_LD + lk) = v;
        }
#pragma unroll
        for (int p = 0; p < PB; ++p) {
            f32x4 v = rb[p];
            asm volatile("" : "+v"(v));
            v.x = cok ? v.x : 0.f; v.y = cok ? v.y : 0.f; v.z = cok ? v.z : 0.f; v.w = cok ? v.w : 0.f;
            *reinterpret_cast<f32x4*>(bdst + (p * RPP + lrow) * LDS_LD + lk) = v;
        }
    };

    const int wv = tid >> 6, lane = tid & 63;
    const int wm = wv / WN, wn = wv % WN;
    const int li = lane & (MF - 1), lh = lane / MF;

    load_step(0);
    store_step(0, As, Bs);
    load_step(nsteps > 1 ? 1 : 0);
    acc_t acc[1][TN];
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[0][j][r] = 0.f;
    __syncthreads();

    const int a_off = (wm * MF + li) * LDS_LD + 4 * lh;
    const int b_off = (wn * TN * MF + li) * LDS_LD + 4 * lh;
    f32x4 fa[2], fb[2][TN];
    auto read_frags = [&](const float* abuf, const float* bbuf, int g, int slot) {
        fa[slot] = *reinterpret_cast<const f32x4*>(abuf + a_off + KG * g);
#pragma unroll
        for (int j = 0; j < TN; ++j) fb[slot][j] = *reinterpret_cast<const f32x4*>(bbuf + b_off + j * MF * LDS_LD + KG * g);
    };
    read_frags(As, Bs, 0, 0);

    auto run_step = [&](auto partial_tag, int s) __attribute__((always_inline)) {
        constexpr bool PARTIAL = decltype(partial_tag)::value;
        const float* curA = As + (s & 1) * A_FLOATS;
        const float* curB = Bs + (s & 1) * B_STRIDE;
        float* nxtA = As + ((s + 1) & 1) * A_FLOATS;
        float* nxtB = Bs + ((s + 1) & 1) * B_STRIDE;
        const int ngc = PARTIAL ? ng_last : NG;
#pragma unroll
        for (int g = 0; g < NG; ++g) {
            if (g + 1 < NG && (!PARTIAL || g + 1 < ngc)) read_frags(curA, curB, g + 1, (g + 1) & 1);
            if (SB && g == NG - 1 && !PARTIAL) {            // every wave has read its last fragments of this step: B may be overwritten
                __syncthreads();
                if (s + 1 < nsteps) store_step(s + 1, nxtA, nxtB);
                load_step(min(s + 2, nsteps - 1));
            }
            if (!PARTIAL || g < ngc) {
#pragma unroll
                for (int q = 0; q < 4; ++q)
#pragma unroll
                    for (int j = 0; j < TN; ++j)
                        acc[0][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[g & 1][q], fb[g & 1][j][q], acc[0][j], 0, 0, 0);
            }
            if (!SB && g == 0 && !PARTIAL) {            // a partial step is the last one: nothing left to stage
                if (s + 1 < nsteps) store_step(s + 1, nxtA, nxtB);        // ds_writes first (loads of a step ago) ...
                load_step(min(s + 2, nsteps - 1));                        // ... then the unconditional, clamped loads
            }
        }
        __syncthreads();
        if (s + 1 < nsteps) read_frags(nxtA, nxtB, 0, 0);
    };
    for (int s = 0; s + 1 < nsteps; ++s) run_step(std::false_type{}, s);
    if (ng_last == NG) run_step(std::false_type{}, nsteps - 1);
    else               run_step(std::true_type{}, nsteps - 1);

    // ---------------------------------------------------------------- epilogue (NHWC)
    {
        const int wms = __builtin_amdgcn_readfirstlane(wm), wns = __builtin_amdgcn_readfirstlane(wn);
        long pix0[1] = {m0 + wms * MF};
        const long left = a.M - pix0[0];
        int nvalid[1] = {left >= MF ? MF : (left > 0 ? (int)left : 0)};
        if (fast_epilogue_nhwc<1, TN, MF, 16>(a, acc, pix0, nvalid, 1, n0 + wns * TN * MF, li, lh)) return;
    }
    const bool has_e1 = a.e1_scale != nullptr, has_e2 = a.e2_scale != nullptr;
#pragma unroll
    for (int j = 0; j < TN; ++j) {
        const int n = n0 + (wn * TN + j) * MF + li;
        float s1 = 1.f, b1 = 0.f, s2 = 1.f, b2 = 0.f;
        const bool nok = n < a.c_out;
        if (has_e1 && n < a.c_out_pad) { s1 = a.e1_scale[n]; b1 = a.e1_shift[n]; }
        if (has_e2 && n < a.c_out_pad) { s2 = a.e2_scale[n]; b2 = a.e2_shift[n]; }
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int drow = (r & 3) + 8 * (r >> 2) + 4 * lh;
            const long m = m0 + wm * MF + drow;
            float v = acc[0][j][r];
            if (has_e1) v = v * s1 + b1;
            if (a.res != nullptr && nok && m < a.M) v += a.res[m * a.res_pix_stride + n];
            v = apply_act(v, a.act);
            if (has_e2) v = v * s2 + b2;
            if (nok && m < a.M) {
                a.y[m * a.y_pix_stride + n] = v;
                if (a.y2) a.y2[m * a.y2_pix_stride + n] = v;
            }
        }
    }
}

// Plain 1x1 (stride 1, no padding, no upsample, NHWC out, fp32 MFMA) with enough pixel tiles per DECLARED launch
// (fill_frames x H x W; 150 tiles of 128 pixels) to fill the chip without split-K -- per-frame geometry and the caller's
// declaration only, like every other kernel choice.  DenseNet block 3 (22x76) qualifies from fill_frames 12 on: the
// bench's B=16 declares 16; the library default of 8 leaves it on the row-tiled kernel, which is what a single-frame
// caller that never declares anything needs.
inline bool conv1x1_eligible(const ConvArgs& a, bool nchw, int bn) {
    if (a.ksize != 1 || a.stride != 1 || a.pad != 0 || a.ups != 0 || a.bundled || a.subpix || nchw || a.n_tail > 0) return false;
    if (a.c_out % bn != 0) return false;
    const long tiles8 = ((long)a.fill_frames * a.H * a.W + 127) / 128 * ((a.c_out + bn - 1) / bn);      // nominal launch
    constexpr long kMinTiles = 150;
    return tiles8 >= kMinTiles;
}

template <int BN, int WM = 4, bool SB = false>
int launch_conv1x1(const ConvArgs& a0, const ConvRun& r) {
    ConvArgs a = a0;
    constexpr int BM = WM * 32;
    const long n_mtiles = (a.M + BM - 1) / BM;
    a.n_ntiles = (a.c_out + BN - 1) / BN;
    a.tiles_per_class = (int)(n_mtiles * a.n_ntiles);
    a.ksplit = 1;
    const long nwg = n_mtiles * a.n_ntiles;
    const size_t lds = (size_t)(2 * BM + (SB ? 1 : 2) * BN) * LdsLd<32>::value * sizeof(float);
    return conv_launch<conv1x1_kernel<BN, WM, SB>>(r, ConvChoice{BTS_CONV_KIND_WIDE_1X1, BM, BN, 1}, BTS_ERR_INVALID, nwg, nwg, WM * 128, lds, a);
}
