// Halo-tile variant of the implicit-GEMM convolution (included by conv_mfma.hip inside its anonymous namespace).
//
// conv_fwd_kernel stages, for EVERY tap of a 3x3 convolution, a fresh [BM pixels][32 channels] slab of the input:
// nine gathers of (almost) the same pixels per 32-channel chunk.  HBM does not notice (the re-reads hit L2), but the
// staging INSTRUCTIONS do: address arithmetic, global loads and ds_writes per MFMA are what keeps the matrix pipe at
// 55-65 % busy (profiles/r01_pmc_mfma.json).  For stride-1, dilation-1 3x3 convolutions -- and the four 2x2 parity
// classes of the sub-pixel upconv -- the output tile here is a SPATIAL patch, TH rows x TW pixels of one frame, and
// the kernel stages its input patch WITH HALO, (TH+KS-1) x (TW+KS-1) pixels x 32 channels, ONCE per channel chunk;
// all KS*KS taps then run out of LDS as shifted views of that patch (the tap's offset is a uniform LDS address shift,
// so the conflict-free 36/40-float row stride of the plain kernel still holds).  Global->LDS traffic and staging work
// for the input drop by KS*KS*TH*TW / ((TH+KS-1)*(TW+KS-1)) = 5.6x (3x3, 4x32 tile); only the weight tile
// ([BN][32] per tap) is re-staged every step.
//
// TW = the MFMA row-tile (32, or 16 for the 16x16x4 shape), so every MFMA row tile is one run of TW consecutive
// pixels of one patch row; TH = 128 / TW.  Used when the frame's width and height tile without much waste
// (halo_eligible); everything else (dilated ASPP branches, strided / up-sampling gathers, grouped bundles, deep
// split-K maps) stays on conv_fwd_kernel.  Same ConvArgs, same epilogue semantics, same result up to the order of
// the K summation (chunk-major here, tap-major there): both are exact-f32 fmaf chains.
template <int BN, int MF, int KS, int DIL = 1>
constexpr int halo_lds_bytes() {
    return 2 * ((128 / MF + KS - 1) * (MF + (KS - 1) * DIL) + BN) * LdsLd<MF>::value * 4;
}
// waves per SIMD the register allocator must leave room for: two workgroups per CU when two fit in the 160 KB of LDS
template <int BN, int NT, int MF, int KS, int DIL = 1>
constexpr int halo_min_waves() { return (NT / 256) * (2 * halo_lds_bytes<BN, MF, KS, DIL>() <= 160 * 1024 ? 2 : 1); }

//
// TAIL (bts_conv_desc.tail_planes): up to four extra input channels that live in dense one-channel planes [B,H,W] --
// the LPG depth maps and reduc1x1 that the reference concatenates behind the feature channels (bts.py:260, 274, 287).
// They form their own 4-channel K chunk after the main chunks: loaded at kernel start (held in registers across the
// main loop, long since landed when used), written to LDS once the main loop is done and consumed by KS*KS tap groups
// without further barriers.  The concat buffer then never holds those channels: no 4-byte scattered writes into a
// 228-float-stride row, no pack_planes pass.
//
// DIL > 1 (the dilated 3x3 of an ASPP branch, bts.py:73-77, dilation = padding = DIL): the "dilation-aware halo".  A
// contiguous 4x32 output patch would need a (4 + 2 DIL) x (32 + 2 DIL) input patch (704 pixels at DIL 6: it does not fit).
// The tile's four output ROWS are therefore taken DIL apart -- y0, y0 + DIL, y0 + 2 DIL, y0 + 3 DIL -- so the input rows
// their three kernel rows touch are y0 - DIL ... y0 + 4 DIL in steps of DIL: SIX patch rows, exactly as for dilation 1;
// only the columns keep their natural halo, 32 + 2 DIL pixels.  Patch row p is image row y0 + (p - 1) DIL, tap (ky, kx)
// is the uniform LDS shift (ky * PW + kx * DIL) pixels: the tap loop, the conflict-free row stride and the whole
// pipeline are the dilation-1 kernel's.  Input staging per MFMA drops 9 * 128 / (6 * (32 + 2 DIL)) = 5.1x (DIL 3) ...
// 3.4x (DIL 12) against the row-tiled gather.  Tile rows are dealt as (group of 4 DIL rows, phase): a 44-row map wastes
// 4 of 48 rows for DIL 3 / 6 / 12; DIL 18 / 24 would waste 39 / 54 % and stay on the row-tiled kernel, which skips their
// all-padding taps instead (tile_tapmask).
template <int BN, int WM, int WN, int MF, int KS, bool NCHW_OUT, bool TAIL = false, bool SB = false, int DIL = 1>
__global__ __launch_bounds__(WM * WN * 64, (SB ? (DIL > 1 ? 1 : 2) * (WM * WN * 64 / 256) : halo_min_waves<BN, WM * WN * 64, MF, KS, DIL>())) void conv_halo_kernel(const ConvArgs a) {
    static_assert(!(SB && TAIL), "the planar tail's weights need both B buffers");
    static_assert(DIL == 1 || (KS == 3 && !TAIL && !NCHW_OUT && MF == 32), "dilated tiles: plain 3x3, NHWC, 32x32x2 MFMA");
    constexpr int NT = WM * WN * 64;
    constexpr int BM = 128;
    constexpr int TW = MF, TH = BM / TW;
    constexpr int PH = TH + KS - 1, PW = TW + (KS - 1) * DIL, NPIX = PH * PW;
    constexpr int T = KS * KS;                       // tap-steps per channel chunk
    constexpr int RPP = NT / 8;                      // patch pixels (or weight rows) staged per pass: 8 lanes x 16 B each
    constexpr int PA = (NPIX + RPP - 1) / RPP;       // passes over the patch
    constexpr int PPS = (PA + T - 2) / (T - 1);      // patch passes per tap-step (all written before the chunk ends)
    constexpr int PB = (BN + RPP - 1) / RPP;
    constexpr int TM = BM / WM / MF, TN = BN / WN / MF;
    constexpr int LDS_LD = LdsLd<MF>::value;
    constexpr int NACC = MF == 32 ? 16 : 4;
    constexpr int A_FLOATS = NPIX * LDS_LD, B_FLOATS = BN * LDS_LD;
    // SB: ONE weight buffer.  The 128-wide tile then takes 77 instead of 96 KB of LDS and two eight-wave workgroups share a
    // CU; the next step's tiles are written after a barrier that follows the step's last fragment reads, in the shadow of
    // its last MFMA group (conv_1x1.inc has the same scheme): conv4 -2 %, daspp_conv -2 %, upconv3 -9 %.  The 32-wide tile
    // (four waves per workgroup) goes from two to three workgroups per CU: upconv1 -14 %.
    constexpr int B_STRIDE = SB ? 0 : B_FLOATS;
    typedef float acc_t __attribute__((ext_vector_type(NACC)));
    static_assert(BM % (WM * MF) == 0 && BN % (WN * MF) == 0 && TM >= 1 && TN >= 1, "tile/wave layout");
    static_assert(PPS * (T - 1) >= PA, "patch passes must fit the chunk's tap-steps");
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    // a single channel chunk (conv1: 32 channels + planar tail) never stages a second patch: one A buffer, which lets
    // twice as many workgroups share a CU and overlap each other's patch-load prologue and output-store epilogue --
    // all such a short K loop (9 tap-steps) leaves to hide them with
    const int a_bufs = a.halo_single_a ? 1 : 2;                    // wave-uniform (SGPR)
    float* const As = reinterpret_cast<float*>(smem_raw);          // [a_bufs][NPIX][LDS_LD]
    float* const Bs = As + a_bufs * A_FLOATS;                      // [2][BN][LDS_LD]

    // ---- tile decode (XCD-aware bijective remap as in conv_fwd_kernel)
    const int nwg = gridDim.x, bid = blockIdx.x;
    const int swz = xcd_swizzle(bid, nwg);
    const int cls = a.subpix ? (swz & 3) : 0;                      // sub-pixel: class-minor order (source patch shared via L2)
    const int tcl = a.subpix ? (swz >> 2) : swz;
    const int mt_idx = tcl / a.n_ntiles, nt_idx = tcl - mt_idx * a.n_ntiles;
    const int n0 = nt_idx * BN;
    const int n_tx = (a.W + TW - 1) / TW, n_ty = DIL > 1 ? ((a.H + TH * DIL - 1) / (TH * DIL)) * DIL : (a.H + TH - 1) / TH;
    const int bfr = mt_idx / (n_tx * n_ty);
    const int trem = mt_idx - bfr * (n_tx * n_ty);
    const int tyi = trem / n_tx;
    // DIL > 1: tile row index = (group of TH*DIL image rows, phase inside the group); the tile's rows are DIL apart
    const int y0 = DIL > 1 ? (tyi / DIL) * (TH * DIL) + tyi % DIL : tyi * TH, x0 = (trem - tyi * n_tx) * TW;
    const int spy = cls >> 1, spx = cls & 1;
    const int pad_y = a.subpix ? 1 - spy : a.pad, pad_x = a.subpix ? 1 - spx : a.pad;
    const float* __restrict__ wbase = a.w + (size_t)cls * a.c_out_pad * a.k_pad;

    const int tid = threadIdx.x;
    const int lrow = tid >> 3, lk = (tid & 7) * 4;
    const int c_main = TAIL ? a.c_in_ld - 4 : a.c_in_ld;           // channels read from the NHWC buffer
    const int nchunks = (c_main + BK - 1) / BK;

    // ---- per-thread patch elements: pass p covers patch pixels [p*RPP, (p+1)*RPP); this thread owns pixel
    // p*RPP + lrow, channels lk..lk+3 of the chunk.  Element offsets are clamped into the frame, validity is a bit.
    unsigned abase[PA];
    unsigned inimg = 0, inpatch = 0;
#pragma unroll
    for (int p = 0; p < PA; ++p) {
        const int pix = p * RPP + lrow;
        const int pyy = pix / PW, pxx = pix - pyy * PW;
        const int gy = y0 - pad_y + pyy * DIL, gx = x0 - pad_x + pxx;      // DIL > 1: pad = DIL, patch rows DIL apart
        const bool inp = pix < NPIX;
        const bool ok = inp && (unsigned)gy < (unsigned)a.H && (unsigned)gx < (unsigned)a.W;
        const int yc = min(max(gy, 0), a.H - 1), xc = min(max(gx, 0), a.W - 1);
        abase[p] = ((unsigned)bfr * (unsigned)(a.H * a.W) + (unsigned)(yc * a.W + xc)) * (unsigned)a.x_pix_stride;
        inimg |= (ok ? 1u : 0u) << p;
        inpatch |= (inp ? 1u : 0u) << p;
    }
    unsigned wrow[PB];
#pragma unroll
    for (int p = 0; p < PB; ++p) {
        int n = n0 + p * RPP + lrow;
        n = n < a.c_out_pad ? n : a.c_out_pad - 1;               // rows past c_out_pad feed outputs that are never stored
        wrow[p] = (unsigned)n * (unsigned)a.k_pad;
    }
    const bool has_pre = a.pre_scale != nullptr;

    auto load_a = [&](int p, int chunk, f32x4& v, f32x4& ps, f32x4& pb) {
        const int c = chunk * BK + lk;
        const unsigned cs = c < c_main ? (unsigned)c : 0u;                       // partial last chunk: stay inside the pixel's row
        v = *reinterpret_cast<const f32x4*>(a.x + (abase[p] + cs));
        if (has_pre) {
            ps = *reinterpret_cast<const f32x4*>(a.pre_scale + cs);
            pb = *reinterpret_cast<const f32x4*>(a.pre_shift + cs);
        }
    };
    // store_*: the empty volatile asm pins the first USE of a staged register to this point.  With the tap loop
    // unrolled hipcc otherwise hoists the prologue / mask arithmetic up to just behind the load of the previous step
    // (it is pure ALU, nothing orders it behind the barrier) -- and with it the s_waitcnt for that load.
    auto store_a = [&](int p, int chunk, float* dstbuf, f32x4 v, f32x4 ps, f32x4 pb) {
        if (!((inpatch >> p) & 1u)) return;
        asm volatile("" : "+v"(v));
        if (has_pre) { asm volatile("" : "+v"(ps), "+v"(pb)); v = v * ps + pb; }
        if (a.pre_relu) { v.x = fmaxf(v.x, 0.f); v.y = fmaxf(v.y, 0.f); v.z = fmaxf(v.z, 0.f); v.w = fmaxf(v.w, 0.f); }
        const bool ok = ((inimg >> p) & 1u) && (chunk * BK + lk) < c_main;         // zero padding AFTER the prologue
        v.x = ok ? v.x : 0.f; v.y = ok ? v.y : 0.f; v.z = ok ? v.z : 0.f; v.w = ok ? v.w : 0.f;
        *reinterpret_cast<f32x4*>(dstbuf + (p * RPP + lrow) * LDS_LD + lk) = v;
    };
    // loads only LOAD (clamped address): any arithmetic on the loaded value here would make the wave wait for the
    // data right after issuing the load; the partial-chunk mask is applied a step later, on the way to LDS
    auto load_b = [&](int chunk, int tap, f32x4 (&rb)[PB]) {
        const int c = chunk * BK + lk;
        const unsigned kofs = (unsigned)(tap * a.c_in_ld + (c < c_main ? c : 0));
#pragma unroll
        for (int p = 0; p < PB; ++p) rb[p] = *reinterpret_cast<const f32x4*>(wbase + (wrow[p] + kofs));
    };
    auto store_b = [&](float* dstbuf, int chunk, const f32x4 (&rb)[PB]) {
        const bool cok = chunk * BK + lk < c_main;
#pragma unroll
        for (int p = 0; p < PB; ++p)
            if ((p + 1) * RPP <= BN || p * RPP + lrow < BN) {
                f32x4 v = rb[p];
                asm volatile("" : "+v"(v));
                v.x = cok ? v.x : 0.f; v.y = cok ? v.y : 0.f; v.z = cok ? v.z : 0.f; v.w = cok ? v.w : 0.f;
                *reinterpret_cast<f32x4*>(dstbuf + (p * RPP + lrow) * LDS_LD + lk) = v;
            }
    };

    const int wv = tid >> 6, lane = tid & 63;
    const int wm = wv / WN, wn = wv % WN;
    const int li = lane & (MF - 1), lh = lane / MF;
    const bool late = NT == 512 && MF == 16 && !SB && a.stagger != 0 && __builtin_amdgcn_readfirstlane(wv) >= 4;      // wave-uniform

    // ---- tail operand: issue its loads now.  Patch: thread (lrow, *) reads its pixel from each plane (the 8 lanes of a
    // pixel read the same word: one L1 line); weights: [KS*KS taps][BN rows] x 4 channels at k = tap*c_in_ld + c_main
    constexpr int PTB = TAIL ? (T * BN + NT - 1) / NT : 1;
    f32x4 tp[TAIL ? PA : 1], tb[PTB];
    if constexpr (TAIL) {
        static_assert(MF == 32, "the planar tail is built for the 32x32x2 tiles");
#pragma unroll
        for (int p = 0; p < PA; ++p) {
            const int pix = p * RPP + lrow;
            const int pyy = pix / PW, pxx = pix - pyy * PW;
            const int yc = min(max(y0 - pad_y + pyy, 0), a.H - 1), xc = min(max(x0 - pad_x + pxx, 0), a.W - 1);
            const unsigned po = (unsigned)bfr * (unsigned)(a.H * a.W) + (unsigned)(yc * a.W + xc);
            tp[p] = f32x4{a.tail[0][po], a.tail[1][po], a.tail[2][po], a.tail[3][po]};      // unused planes alias plane 0
        }
#pragma unroll
        for (int u = 0; u < PTB; ++u) {
            const int e = min(u * NT + tid, T * BN - 1);
            const int tap = e / BN;
            int n = n0 + (e - tap * BN);
            n = n < a.c_out_pad ? n : a.c_out_pad - 1;
            tb[u] = *reinterpret_cast<const f32x4*>(wbase + ((unsigned)n * (unsigned)a.k_pad + (unsigned)(tap * a.c_in_ld + c_main)));
        }
    }

    // ---- prologue: the whole patch of chunk 0, weight tiles of steps 0 and 1
    f32x4 rb[PB];
    {
        f32x4 va[PA], ps[PA], pb[PA];
#pragma unroll
        for (int p = 0; p < PA; ++p) load_a(p, 0, va[p], ps[p], pb[p]);
        load_b(0, 0, rb);
#pragma unroll
        for (int p = 0; p < PA; ++p) store_a(p, 0, As, va[p], ps[p], pb[p]);
        store_b(Bs, 0, rb);
    }
    load_b(0, 1, rb);                          // step 1 = (chunk 0, tap 1); T >= 4
    acc_t acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int r = 0; r < NACC; ++r) acc[i][j][r] = 0.f;
    __syncthreads();

    constexpr int KG = 256 / MF;              // k covered by one ds_read_b128 per lane set: 8 (MF 32) / 16 (MF 16)
    constexpr int NG = BK / KG;               // fragment groups per step: 4 / 2
    // A fragment of row tile i: patch row (wm*TM + i), pixels li.. of that row, + the tap's uniform shift
    const int a_off = ((wm * TM) * PW + li) * LDS_LD + 4 * lh;
    const int b_off = (wn * TN * MF + li) * LDS_LD + 4 * lh;
    f32x4 fa[2][TM], fb[2][TN];
    auto read_frags = [&](const float* abuf, const float* bbuf, int tapoff, int g, int slot) {
#pragma unroll
        for (int i = 0; i < TM; ++i) fa[slot][i] = *reinterpret_cast<const f32x4*>(abuf + a_off + tapoff + i * PW * LDS_LD + KG * g);
#pragma unroll
        for (int j = 0; j < TN; ++j) fb[slot][j] = *reinterpret_cast<const f32x4*>(bbuf + b_off + j * MF * LDS_LD + KG * g);
    };
    read_frags(As, Bs, 0, 0, 0);

    f32x4 sa[PPS], sps[PPS], spb[PPS];        // patch elements of the NEXT chunk in flight (one step ahead of their ds_write)
    // the last chunk may hold fewer than 32 channels (36, 164, 228 ...): it runs only the fragment groups that hold
    // real channels (a group = KG consecutive k), so odd channel counts cost what the tap-major flattened K of
    // conv_fwd_kernel costs, not a whole padded chunk
    const int ng_last = (c_main - (nchunks - 1) * BK + KG - 1) / KG;
    // PARTIAL = false: all NG groups, no conditionals in the MFMA stream (every chunk but possibly the last);
    // PARTIAL = true: the last chunk when it holds fewer than 32 channels -- groups beyond ng_last are skipped
    auto run_chunk = [&](auto partial_tag, int chunk) __attribute__((always_inline)) {
        constexpr bool PARTIAL = decltype(partial_tag)::value;
        const float* curA = As + (chunk & (a_bufs - 1)) * A_FLOATS;
        float* nxtA = As + ((chunk + 1) & (a_bufs - 1)) * A_FLOATS;      // never written when there is one chunk
        const bool more = chunk + 1 < nchunks;
        const int ngc = PARTIAL ? ng_last : NG;                // wave-uniform
#pragma unroll
        for (int t = 0; t < T; ++t) {
            const int s = chunk * T + t;
            const float* curB = Bs + (s & 1) * B_STRIDE;
            float* nxtB = Bs + ((s + 1) & 1) * B_STRIDE;
            const int tapoff = ((t / KS) * PW + (t % KS) * DIL) * LDS_LD;
            auto stage_next = [&]() __attribute__((always_inline)) {
                    // Staging in the shadow of the remaining MFMA groups.  Two rules keep hipcc's s_waitcnt placement
                    // exact (it falls back to vmcnt(0) -- a full round trip exposed every step -- as soon as the number
                    // of loads in flight depends on a branch):
                    //   * every load is issued UNCONDITIONALLY, with its (chunk, tap, pass) clamped into range; past the
                    //     end of K it re-reads the last tile and nothing consumes it;
                    //   * every ds_write (each waits for a load issued a step ago) comes before any new load is issued:
                    //     vmcnt counts in order, a write placed after a fresh load would wait for that load.
                    // The weight tile of step s+1 goes to the other B buffer and its registers take the loads of step
                    // s+2; the next chunk's patch trickles in PPS passes per step, written one step after their loads.
                    store_b(nxtB, t + 1 < T ? chunk : chunk + 1, rb);
                    if (more) {
#pragma unroll
                        for (int u = 0; u < PPS; ++u) {
                            const int pw = (t - 1) * PPS + u;                 // pass written now (issued during step t-1)
                            if (t >= 1 && pw < PA) store_a(pw, chunk + 1, nxtA, sa[u], sps[u], spb[u]);
                        }
                    }
                    {
                        const int t2 = t + 2 < T ? t + 2 : t + 2 - T;
                        const int c2 = t + 2 < T ? chunk : chunk + 1;
                        load_b(min(c2, nchunks - 1), t2, rb);
                    }
#pragma unroll
                    for (int u = 0; u < PPS; ++u) {
                        const int pl = t * PPS + u;                           // pass issued now
                        if (t < T - 1 && pl < PA) load_a(pl, min(chunk + 1, nchunks - 1), sa[u], sps[u], spb[u]);
                    }
            };
#pragma unroll
            for (int g = 0; g < NG; ++g) {
                if (g + 1 < NG && (!PARTIAL || g + 1 < ngc)) read_frags(curA, curB, tapoff, g + 1, (g + 1) & 1);
                if (SB && g == NG - 1) {      // every wave holds its last fragments of this step: the one B buffer may be overwritten;
                    __syncthreads();          // the writes and the new loads issue in the shadow of this group's MFMAs
                    stage_next();
                }
                if (!PARTIAL || g < ngc) {
#pragma unroll
                    for (int q = 0; q < 4; ++q)
#pragma unroll
                        for (int i = 0; i < TM; ++i)
#pragma unroll
                            for (int j = 0; j < TN; ++j) {
                                const float ra_ = NCHW_OUT ? fb[g & 1][j][q] : fa[g & 1][i][q];
                                const float rb_ = NCHW_OUT ? fa[g & 1][i][q] : fb[g & 1][j][q];
                                if constexpr (MF == 32) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(ra_, rb_, acc[i][j], 0, 0, 0);
                                else                    acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(ra_, rb_, acc[i][j], 0, 0, 0);
                            }
                }
                // STAGGER (eight-wave 48-wide tile): the two waves that share a SIMD (w and w + 4) run this same program in
                // lockstep, so both sit in the staging block (VALU, ds_write, address arithmetic: no MFMA) at the same time
                // and the SIMD's matrix pipe idles through it.  Waves 4..7 stage half a step later: their staging overlaps
                // the partner's MFMA group and vice versa (MI355X_MICROARCH.md, two waves per SIMD, item 9).  Measured
                // (gpurun_out/r3c): DenseNet block 1 / 2 growth convolutions -2 %; the same stagger on the eight-wave
                // row-tiled and wide 1x1 kernels measured +1.5 ... +2.5 % / neutral and is not applied there
                if (!SB && g == (late ? NG / 2 : 0)) stage_next();
            }
            __syncthreads();
            if (more || t + 1 < T) {
                const int tn = t + 1 < T ? t + 1 : 0;
                const float* nA = t + 1 < T ? curA : nxtA;
                read_frags(nA, nxtB, ((tn / KS) * PW + (tn % KS) * DIL) * LDS_LD, 0, 0);
            }
        }
    };
    for (int chunk = 0; chunk + 1 < nchunks; ++chunk) run_chunk(std::false_type{}, chunk);
    if (ng_last == NG) run_chunk(std::false_type{}, nchunks - 1);
    else               run_chunk(std::true_type{}, nchunks - 1);

    // ---------------------------------------------------------------- planar tail chunk
    if constexpr (TAIL) {
        // the main loop ended on a barrier: both LDS regions are free.  Patch rows keep the LDS_LD stride with k 0..3 =
        // the planes and k 4..7 = 0 (the k-half of lanes lh = 1); weights go to Bs as [tap][BN][8].
        float* const Bt = Bs;
        static_assert(T * BN * 8 <= 2 * B_FLOATS, "tail weights fit the B region");
#pragma unroll
        for (int p = 0; p < PA; ++p) {
            f32x4 v = tp[p];
            asm volatile("" : "+v"(v));
            v.y = a.n_tail > 1 ? v.y : 0.f; v.z = a.n_tail > 2 ? v.z : 0.f; v.w = a.n_tail > 3 ? v.w : 0.f;   // unused slots
            if (((inpatch >> p) & 1u) && lk < 8) {
                const bool ok = ((inimg >> p) & 1u) && lk == 0;                   // zero padding; upper k-half is zero
                v.x = ok ? v.x : 0.f; v.y = ok ? v.y : 0.f; v.z = ok ? v.z : 0.f; v.w = ok ? v.w : 0.f;
                *reinterpret_cast<f32x4*>(As + (p * RPP + lrow) * LDS_LD + lk) = v;
            }
        }
#pragma unroll
        for (int u = 0; u < PTB; ++u) {
            const int e = u * NT + tid;
            f32x4 v = tb[u];
            asm volatile("" : "+v"(v));
            if (e < T * BN) {
                *reinterpret_cast<f32x4*>(Bt + e * 8) = v;
                *reinterpret_cast<f32x4*>(Bt + e * 8 + 4) = f32x4{0.f, 0.f, 0.f, 0.f};
            }
        }
        __syncthreads();
#pragma unroll
        for (int t = 0; t < T; ++t) {
            const int tapoff = ((t / KS) * PW + (t % KS) * DIL) * LDS_LD;
            f32x4 ta[TM], tbf[TN];
#pragma unroll
            for (int i = 0; i < TM; ++i) ta[i] = *reinterpret_cast<const f32x4*>(As + a_off + tapoff + i * PW * LDS_LD);
#pragma unroll
            for (int j = 0; j < TN; ++j) tbf[j] = *reinterpret_cast<const f32x4*>(Bt + ((t * BN + (wn * TN + j) * MF + li) * 8 + 4 * lh));
#pragma unroll
            for (int q = 0; q < 4; ++q)
#pragma unroll
                for (int i = 0; i < TM; ++i)
#pragma unroll
                    for (int j = 0; j < TN; ++j) {
                        const float ra_ = NCHW_OUT ? tbf[j][q] : ta[i][q];
                        const float rb_ = NCHW_OUT ? ta[i][q] : tbf[j][q];
                        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(ra_, rb_, acc[i][j], 0, 0, 0);
                    }
        }
    }

    // ---------------------------------------------------------------- epilogue
    // D register r of lane (li, lh) is D[row][col = li] with row = (r&3) + 8*(r>>2) + 4*lh (MF 32) or 4*lh + r (MF 16);
    // GEMM row (wm*TM + i)*MF + row_in_tile  <->  pixel (y0 + wm*TM + i, x0 + row_in_tile)
    const long HW = (long)a.H * a.W;
    {   // compact epilogues (conv_mfma.hip): row tile i = TW consecutive pixels of image row y0 + wm*TM + i
        const int wms = __builtin_amdgcn_readfirstlane(wm), wns = __builtin_amdgcn_readfirstlane(wn);
        const int xleft = a.W - x0;
        if constexpr (!NCHW_OUT) {
            long pix0[TM];
            int nvalid[TM];
#pragma unroll
            for (int i = 0; i < TM; ++i) {
                const int y = y0 + (wms * TM + i) * DIL;
                pix0[i] = a.subpix ? ((long)bfr * (2 * a.H) + 2 * y + spy) * (2 * a.W) + 2 * x0 + spx
                                   : ((long)bfr * a.H + y) * a.W + x0;
                nvalid[i] = y < a.H ? (xleft >= MF ? MF : xleft) : 0;
            }
            if (fast_epilogue_nhwc<TM, TN, MF, NACC>(a, acc, pix0, nvalid, a.subpix ? 2 : 1, n0 + wns * TN * MF, li, lh)) return;
        } else {
            if (a.e1_scale == nullptr && a.e2_scale == nullptr && a.act != 3 && HW * MF < 2147483648L) {
                long chan_base[TM];
                unsigned lane_pix[TM];
                bool pix_ok[TM];
#pragma unroll
                for (int i = 0; i < TM; ++i) {
                    const int y = y0 + (wms * TM + i) * DIL;
                    chan_base[i] = (long)bfr * a.c_out;
                    pix_ok[i] = y < a.H && li < xleft;
                    lane_pix[i] = (unsigned)((pix_ok[i] ? y : 0) * a.W + x0 + (pix_ok[i] ? li : 0));
                }
                const int nc0 = n0 + wns * TN * MF;
                if (a.act == 1) store_tiles_nchw<1, TM, TN, MF, NACC>(a, acc, chan_base, lane_pix, pix_ok, HW, nc0, lh);
                else if (a.act == 2) store_tiles_nchw<2, TM, TN, MF, NACC>(a, acc, chan_base, lane_pix, pix_ok, HW, nc0, lh);
                else store_tiles_nchw<0, TM, TN, MF, NACC>(a, acc, chan_base, lane_pix, pix_ok, HW, nc0, lh);
                return;
            }
        }
    }
    const bool has_e1 = a.e1_scale != nullptr, has_e2 = a.e2_scale != nullptr;
#pragma unroll
    for (int i = 0; i < TM; ++i) {
        const int y = y0 + (wm * TM + i) * DIL;
#pragma unroll
        for (int j = 0; j < TN; ++j) {
            if (!NCHW_OUT) {
                const int n = n0 + (wn * TN + j) * MF + li;
                float s1 = 1.f, b1 = 0.f, s2 = 1.f, b2 = 0.f;
                const bool nok = n < a.c_out;
                if (has_e1 && n < a.c_out_pad) { s1 = a.e1_scale[n]; b1 = a.e1_shift[n]; }
                if (has_e2 && n < a.c_out_pad) { s2 = a.e2_scale[n]; b2 = a.e2_shift[n]; }
#pragma unroll
                for (int r = 0; r < NACC; ++r) {
                    const int drow = MF == 32 ? (r & 3) + 8 * (r >> 2) + 4 * lh : 4 * lh + r;
                    const int x = x0 + drow;
                    const bool mok = y < a.H && x < a.W;
                    const long m = ((long)bfr * a.H + y) * a.W + x;
                    float v = acc[i][j][r];
                    if (has_e1) v = v * s1 + b1;
                    // sub-pixel: source pixel (b,y,x) of this parity class is output pixel (b, 2y+py, 2x+px); the residual lives there too
                    const long op = a.subpix ? ((long)bfr * (2 * a.H) + 2 * y + spy) * (2 * a.W) + 2 * x + spx : m;
                    if (a.res != nullptr && nok && mok) v += a.res[op * a.res_pix_stride + n];
                    v = apply_act(v, a.act);
                    if (has_e2) v = v * s2 + b2;
                    if (nok && mok) {
                        a.y[op * a.y_pix_stride + n] = v;
                        if (a.y2) a.y2[op * a.y2_pix_stride + n] = v;
                    }
                }
            } else {
                const int x = x0 + li;
                const bool mok = y < a.H && x < a.W;
                const long yx = (long)y * a.W + x;
#pragma unroll
                for (int r = 0; r < NACC; ++r) {
                    const int drow = MF == 32 ? (r & 3) + 8 * (r >> 2) + 4 * lh : 4 * lh + r;
                    const int n = n0 + (wn * TN + j) * MF + drow;
                    float v = acc[i][j][r];
                    if (n < a.c_out_pad) {
                        if (has_e1) v = v * a.e1_scale[n] + a.e1_shift[n];
                        v = apply_act(v, a.act);
                        if (has_e2) v = v * a.e2_scale[n] + a.e2_shift[n];
                    }
                    if (mok && n < a.c_out) a.y[((long)bfr * a.c_out + n) * HW + yx] = v;
                }
            }
        }
    }
}

// Spatial tiles waste the rows / columns that overhang the frame: use the halo kernel only when at least `min_fill`
// of the tile grid is real pixels (e.g. 22x76 maps with 4x32 tiles: 0.72 -- stay on the row-tiled kernel).
inline bool halo_eligible(const ConvArgs& a, bool precision0, int mf, double* fill_out) {
    if (!precision0 || a.bundled || a.ups != 0 || a.stride != 1) return false;
    if (a.subpix) { if (a.ksize != 2 || a.dil != 1) return false; }
    else if (a.ksize != 3 || a.pad != a.dil) return false;
    // dilated tiles (conv_halo_kernel, DIL > 1): built for the ASPP branches' dilations whose row groups tile the map
    // Measured at B=16 on the 44x152 map (gpurun_out/r3d, us per launch, row-tiled with tap skipping -> dilated tile):
    // dilation 3: 662 -> 654; 6: 590 -> 625; 12: 504 -> 594.  The row-tiled kernel skips the all-padding taps (4 / 9 / 18 %
    // of the tap-steps at dilation 3 / 6 / 12) and shares a CU between two workgroups; the dilated tile needs 84 ... 115 KB of
    // LDS (one workgroup per CU) and wastes 13 % of its grid on this map.  So only dilation 3 takes it by default
    // (BTS_CONV_HALO_DIL=2: also 6 and 12; 0: none).
    if (a.dil != 1 && !(mf == 32 && ((a.dil == 3 && knobs().halo_dil >= 1) || ((a.dil == 6 || a.dil == 12) && knobs().halo_dil >= 2)))) return false;
    const int TW = mf, TH = 128 / mf;
    const long ntx = (a.W + TW - 1) / TW, nty = a.dil > 1 ? (long)((a.H + TH * a.dil - 1) / (TH * a.dil)) * a.dil : (a.H + TH - 1) / TH;
    const double fill = (double)a.H * a.W / (double)(ntx * TW * nty * TH);
    if (fill_out) *fill_out = fill;
    return fill >= 0.80;
}

template <int BN, int WM, int WN, int MF, int KS, bool TAIL = false, bool SB = false, int DIL = 1>
int launch_halo(const ConvArgs& a0, const ConvRun& r) {
    ConvArgs a = a0;
    constexpr int TW = MF, TH = 128 / MF;
    constexpr int NPIX = (TH + KS - 1) * (TW + (KS - 1) * DIL);
    const long n_ty = DIL > 1 ? (long)((a.H + TH * DIL - 1) / (TH * DIL)) * DIL : (a.H + TH - 1) / TH;
    const long n_mtiles = (long)a.B * n_ty * ((a.W + TW - 1) / TW);
    a.n_ntiles = (a.c_out + BN - 1) / BN;
    a.tiles_per_class = (int)(n_mtiles * a.n_ntiles);
    a.ksplit = 1;
    const long nwg = n_mtiles * a.n_ntiles * a.n_classes;
    if (DIL > 1 && (r.nchw || a.dil != DIL || a.pad != DIL)) return BTS_ERR_INVALID;
    const ConvChoice c{(TAIL ? BTS_CONV_KIND_HALO_TAIL : BTS_CONV_KIND_HALO) | (BN == 48 && WM == 8 ? BTS_CONV_FLAG_W8 : 0) | (DIL > 1 ? BTS_CONV_FLAG_DIL : 0), 128, BN, 1};
    static_assert(halo_lds_bytes<BN, MF, KS, DIL>() == 2 * (NPIX + BN) * LdsLd<MF>::value * 4, "LDS size");
    const int c_main = TAIL ? a.c_in_ld - 4 : a.c_in_ld;
    a.halo_single_a = c_main <= BK ? 1 : 0;
    const size_t lds = SB ? (size_t)(2 * NPIX + BN) * LdsLd<MF>::value * 4
                          : (a.halo_single_a ? (size_t)(NPIX + 2 * BN) * LdsLd<MF>::value * 4 : (size_t)halo_lds_bytes<BN, MF, KS, DIL>());
    static_assert(!SB || (size_t)(2 * NPIX + BN) * LdsLd<MF>::value * 4 <= 160 * 1024, "single-weight-buffer tile must fit the LDS");
    if (SB) a.halo_single_a = 0;
    a.stagger = (BN == 48 && WM * WN == 8) ? 1 : 0;
    if constexpr (DIL == 1) {                          // the dilated tiles have no NCHW twin
        if (r.nchw) return conv_launch<conv_halo_kernel<BN, WM, WN, MF, KS, true, TAIL, SB>>(r, c, BTS_ERR_INVALID, nwg, nwg, WM * WN * 64, lds, a);
    }
    return conv_launch<conv_halo_kernel<BN, WM, WN, MF, KS, false, TAIL, SB, DIL>>(r, c, BTS_ERR_INVALID, nwg, nwg, WM * WN * 64, lds, a);
}
