// The bf16 halo tile: the producer and the consumer body of conv_halo_emu_kernel (below: bts_conv_desc.precision = 1 and 2)
// and of conv_tail_bf16_kernel (conv_tail_bf16.inc).  Included by conv_mfma.hip inside its anonymous namespace, after
// conv_halo.inc.
//
// The arithmetic is conv_fwd_kernel's PREC mode (split_store: every fp32 operand = three bf16 pieces h + m + l by
// truncation, six v_mfma_f32_32x32x16_bf16 per 16 k of a 32x32 block -- hh, hm, mh, hl, lh, mm -- accumulated in fp32;
// error 1.2e-6 of max|result| on K = 2304, the fp32-MFMA chain's own level).  What changes is where the split happens:
//
//   * INPUT: the tile is conv_halo_kernel's spatial patch (4 x 32 output pixels of one frame, its input patch WITH halo
//     staged once per 32-channel chunk, all KS*KS taps running out of LDS as shifted views).  The patch is split ONCE on
//     its way to LDS -- three bf16 planes of 64-byte pixel rows, XOR-swizzled (emu_a_off) -- and serves all KS*KS taps: the
//     row-tiled emulation re-split the same pixels for every tap (~30 VALU instructions per staged f32x4, nine times).
//   * WEIGHTS: split OFFLINE (ops.split_bf16x3: the same truncation split, done once per packed weight) into
//     [class][plane][c_out_pad][k_pad] bf16.  A tap-step's weight tile is then plain bytes: it goes global -> LDS by
//     LDS-DMA (global_load_lds_dwordx4: no VGPRs, no VALU, no ds_write), 16 rows x 64 B per wave instruction into
//     unpadded 64-byte rows whose four 16-byte chunks are XOR-swizzled with bits 2-3 of the row (the swizzle is applied
//     to the per-lane SOURCE address; the reader applies it again: conflict-free ds_read_b128, emu_off's layout).
//
// NP = 1 is the bf16 mode (bts_conv_desc.precision = 2): the same tile with ONE plane -- the patch rounded to nearest even
// on its way to LDS (rne_store), the weights pre-rounded offline (ops.round_bf16, [class][1][c_out_pad][k_pad]) -- and one
// v_mfma_f32_32x32x16_bf16 per 16 k of a 32x32 block instead of six.  A third of the LDS and of the weight DMA.
//
// Eight waves in two ROLES.  Waves 0..3 (one per SIMD) are CONSUMERS (halo_emu_consume): 2 (patch-row pairs) x 2 (channel
// halves), each a 64-pixel x BN/2-channel tile -- LDS fragment reads and MFMAs only, 12 ds_read_b128 per 24 MFMAs.  Waves
// 4..7 (their SIMD partners) are PRODUCERS (halo_emu_produce): they issue the weight DMA, load the next chunk's patch,
// split it and write it to LDS.  In the first version every wave did both, in lockstep with its SIMD partner: DMA issue
// (~100 cycles per wave instruction), split arithmetic and waits then stopped BOTH waves of a SIMD at once and the matrix
// pipe idled through them (see DESIGN 3b for the measured steps).
//
// THREE weight stages: the DMA for step s+2 is issued at the start of step s into the stage that step s-1 read (the
// barrier that ended step s-1 protects it); before the barrier that ends step s every wave waits, with a COUNTED vmcnt,
// for everything but its own operations of step s -- so the tile of step s+1 has landed and the tile of s+2 stays in flight
// across the barrier (raw s_barrier: __syncthreads() would drain the DMA, cdna_hip_programming.md "Pipelining across
// barriers").  Every vector-memory operation of the loop is unconditional (clamped), so the counts are compile-time
// constants.  The next chunk's patch trickles in one 32-pixel pass (two with KS 2) per tap-step: loaded in step t by loads
// the compiler does not track (load_untracked), converted and written in step t+1 behind a counted wait.
//
// LDS image of the patch: NP bf16 planes of UNPADDED 64-byte pixel rows (32 channels); the four 16-byte chunks of a row
// are XOR-swizzled with bits 2-3 of the pixel index.  A ds_read_b128 lane group covers 16 pixels that are distinct mod
// 16 whatever uniform shift the tap adds (base + {0-3, 12-15, 20-27}), so (pixel & 3, chunk ^ (pixel >> 2 & 3)) -- the
// 16-byte bank slot -- is distinct too: conflict-free for every tap.  The swizzle makes a tap's address non-additive, so
// the KS*KS x 2 fragment addresses of a lane are computed once, before the loop (they do not depend on the chunk).
__device__ __forceinline__ int emu_a_off(int pix, int chunk16) { return pix * EMU_ROW_BYTES + (((chunk16 ^ (pix >> 2)) & 3) << 4); }

// Sizes of one tile: the input patch of 4 x 32 outputs under a KS x KS kernel, and its LDS image -- As [2][NP planes][NPIX]
// [64 B], then Bs [3 stages][NP planes][BN][64 B]
template <int BN, int KS, int NP>
struct HaloEmuGeom {
    static constexpr int TW = 32, TH = 4, PH = TH + KS - 1, PW = TW + KS - 1, NPIX = PH * PW, T = KS * KS;
    static constexpr int A_PLANE = NPIX * EMU_ROW_BYTES, A_BUF = NP * A_PLANE;
    static constexpr int B_PLANE = BN * EMU_ROW_BYTES, B_STAGE = NP * B_PLANE;
    static constexpr int LDS_BYTES = 2 * A_BUF + 3 * B_STAGE;
    static_assert(NP == 3 || NP == 1, "NP: 3 bf16x3 planes (precision 1) or one bf16 plane (precision 2)");
};

// 4 x 32 output tiles of one H x W frame, and the share of that tile grid that is real pixels
inline long tiles_4x32(int H, int W, double* fill = nullptr) {
    const long n = (long)((H + 3) / 4) * ((W + 31) / 32);
    if (fill) *fill = (double)H * W / (double)(n * 128);
    return n;
}

// Tile `tcl` of a launch (or of its parity class) -> channel tile n0, frame, top-left output pixel (as conv_halo_kernel)
struct Tile4x32 { int n0, bfr, y0, x0; };
template <int BN>
__device__ __forceinline__ Tile4x32 decode_tile_4x32(int tcl, int n_ntiles, int H, int W) {
    const int mt_idx = tcl / n_ntiles, nt_idx = tcl - mt_idx * n_ntiles;
    const int n_tx = (W + 31) / 32, n_ty = (H + 3) / 4;
    const int bfr = mt_idx / (n_tx * n_ty);
    const int trem = mt_idx - bfr * (n_tx * n_ty);
    const int tyi = trem / n_tx;
    return Tile4x32{nt_idx * BN, bfr, tyi * 4, (trem - tyi * n_tx) * 32};
}

// One patch pass of a producer thread in flight: four channels of one pixel and, with AFFINE, their prologue scale and
// shift.  Without AFFINE the two do not exist: a "+v" operand would keep their registers alive.
template <bool AFFINE> struct PatchRegs { f32x4 v = {0.f, 0.f, 0.f, 0.f}, ps = {1.f, 1.f, 1.f, 1.f}, pb = {0.f, 0.f, 0.f, 0.f}; };
template <> struct PatchRegs<false> { f32x4 v = {0.f, 0.f, 0.f, 0.f}; };

// global_load_dwordx4 whose result the compiler does not track: beside LDS-DMA traffic hipcc waits vmcnt(0) at the first
// use of any ordinary load's result, which would drain the weight ring every step.  The consumer passes the registers
// through wait_vm<N>() first (a counted s_waitcnt the values depend on).
__device__ __forceinline__ void load_untracked(f32x4& dst, const float* p) {
    asm volatile("global_load_dwordx4 %0, %1, off" : "=v"(dst) : "v"(p) : "memory");
}
template <int N, bool AFFINE> __device__ __forceinline__ void wait_vm(PatchRegs<AFFINE>& r) {
    if constexpr (AFFINE) asm volatile("s_waitcnt vmcnt(%3)" : "+v"(r.v), "+v"(r.ps), "+v"(r.pb) : "n"(N) : "memory");
    else asm volatile("s_waitcnt vmcnt(%1)" : "+v"(r.v) : "n"(N) : "memory");
}
// ... with `k` patch passes (LPP loads each) and BASE other operations younger than r's loads; k is a constant once the
// step loop is unrolled.  k <= 3: the later pass of the same step and the two of the next (KS 2).
template <int BASE, int LPP, bool AFFINE> __device__ __forceinline__ void wait_vm_passes(int k, PatchRegs<AFFINE>& r) {
    switch (k) {
        case 0: wait_vm<BASE>(r); break;
        case 1: wait_vm<BASE + LPP>(r); break;
        case 2: wait_vm<BASE + 2 * LPP>(r); break;
        case 3: wait_vm<BASE + 3 * LPP>(r); break;
        default: wait_vm<0>(r); break;
    }
}
// A patch pass whose source is ALREADY bf16 (halo_emu_produce's XBF16: conv3x3_bf16in_kernel): the thread's four channels are
// 8 bytes, one untracked global_load_dwordx2, and go to LDS as they are.  One vector-memory operation per pass, like the
// four-register load above (LPP = 1): vmcnt counts operations, not bytes, so every counted wait below keeps its number.
struct PatchRegsBf16 { u32x2 v = {0u, 0u}; };
__device__ __forceinline__ void load_untracked(u32x2& dst, const unsigned short* p) {
    asm volatile("global_load_dwordx2 %0, %1, off" : "=v"(dst) : "v"(p) : "memory");
}
template <int N> __device__ __forceinline__ void wait_vm(PatchRegsBf16& r) {
    asm volatile("s_waitcnt vmcnt(%1)" : "+v"(r.v) : "n"(N) : "memory");
}
template <int BASE, int LPP> __device__ __forceinline__ void wait_vm_passes(int k, PatchRegsBf16& r) {
    switch (k) {
        case 0: wait_vm<BASE>(r); break;
        case 1: wait_vm<BASE + LPP>(r); break;
        case 2: wait_vm<BASE + 2 * LPP>(r); break;
        case 3: wait_vm<BASE + 3 * LPP>(r); break;
        default: wait_vm<0>(r); break;
    }
}
// The raw barrier between tap-steps, behind the wait that says what has to be complete by then: every LDS operation of the
// wave and all but its VM youngest vector-memory operations (NO_VM: a consumer has none)
constexpr int NO_VM = -1;
template <int VM> __device__ __forceinline__ void wait_then_barrier() {
    if constexpr (VM == NO_VM) asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    else asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)" :: "n"(VM) : "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
}

// What a producer reads
struct HaloEmuSource {
    const float* x; unsigned x_pix_stride; int H, W, bfr, y0, x0, pad_y, pad_x;      // NHWC input, the tile, the padding
                                                                                     // (XBF16: a bf16 buffer, stride in bf16 elements)
    const float* pre_scale; const float* pre_shift; bool has_pre; int pre_relu;      // AFFINE: scale / shift per input channel
                                                                                     // (any readable address without has_pre)
    const unsigned short* w; int w_rows, w_ld;     // bf16 weights [NP planes][w_rows][w_ld], k = tap * tap_stride + channel
    int tap_stride;
    int n0, nchunks;                               // first output channel of the tile; 32-channel chunks of the K axis
};

// PRODUCER waves 4..7 (one per SIMD), from the start of the kernel to the end of the K loop.  `before_first_barrier` runs
// once the patch of chunk 0 is stored.  XBF16 (NP 1, no AFFINE): the patch source holds bf16 -- load_a is one 8-byte load,
// store_a zeroes the pixels outside the image and writes the 8 bytes to the slot plane_store<1> would have rounded them into.
// Nothing else differs: the same addresses (in elements), the same clamps, one operation per pass, the same waits.
template <int BN, int KS, int NP, bool AFFINE, bool XBF16 = false, typename Extra>
__device__ __forceinline__ void halo_emu_produce(const HaloEmuSource& in, char* const As, char* const Bs, int tid, int wv,
                                                 Extra&& before_first_barrier) {
    using G = HaloEmuGeom<BN, KS, NP>;
    constexpr int PW = G::PW, NPIX = G::NPIX, T = G::T;
    constexpr int RPP = 256 / 8;                         // patch pixels staged per pass by the 256 producer threads
    constexpr int PA = (NPIX + RPP - 1) / RPP;           // passes over the patch: 7 (3x3), 6 (2x2)
    constexpr int PPS = (PA + T - 2) / (T - 1);          // passes per tap-step: 1 (3x3), 2 (2x2)
    constexpr int LPP = AFFINE ? 3 : 1;                  // loads per pass: the values, and their scale and shift
    constexpr int NI = NP * BN / 16;                     // DMA wave-instructions per weight stage (16 rows x 64 B each)
    constexpr int NIW = NI / 4;                          // ... per producer wave: 6 / 3 (BN 128 / 64, NP 3), 2 / 1 (NP 1)
    static_assert(NI % 4 == 0 && PPS * (T - 1) >= PA && PPS <= 2, "producer work divides evenly");
    static_assert(!XBF16 || (NP == 1 && !AFFINE), "a bf16 patch is the one-plane tile's, without a prologue");
    typedef std::conditional_t<XBF16, PatchRegsBf16, PatchRegs<AFFINE>> regs_t;
    const int ptid = tid - 256, lane = tid & 63;
    const int lrow = ptid >> 3, lk = (ptid & 7) * 4;
    const int nsteps = in.nchunks * T;
    // patch elements of this thread (pass p: patch pixel p*RPP + lrow, channels lk..lk+3 of the chunk)
    unsigned abase[PA];
    int awr[PA];                                      // LDS byte offset of this thread's 8 bytes inside a plane
    unsigned inimg = 0, inpatch = 0;
#pragma unroll
    for (int p = 0; p < PA; ++p) {
        const int pix = p * RPP + lrow;
        const int pyy = pix / PW, pxx = pix - pyy * PW;
        const int gy = in.y0 - in.pad_y + pyy, gx = in.x0 - in.pad_x + pxx;
        const bool inp = pix < NPIX;
        const bool ok = inp && (unsigned)gy < (unsigned)in.H && (unsigned)gx < (unsigned)in.W;
        const int yc = min(max(gy, 0), in.H - 1), xc = min(max(gx, 0), in.W - 1);
        abase[p] = ((unsigned)in.bfr * (unsigned)(in.H * in.W) + (unsigned)(yc * in.W + xc)) * in.x_pix_stride + (unsigned)lk;
        awr[p] = emu_a_off(inp ? pix : 0, lk >> 3) + (lk & 7) * 2;
        inimg |= (ok ? 1u : 0u) << p;
        inpatch |= (inp ? 1u : 0u) << p;
    }
    auto load_a = [&](int p, int chunk, regs_t& r) {
        const unsigned cs = (unsigned)(chunk * BK);
        if constexpr (XBF16) load_untracked(r.v, reinterpret_cast<const unsigned short*>(in.x) + (abase[p] + cs));
        else load_untracked(r.v, in.x + (abase[p] + cs));
        if constexpr (AFFINE) {
            load_untracked(r.ps, in.pre_scale + (cs + lk));
            load_untracked(r.pb, in.pre_shift + (cs + lk));
        }
    };
    auto store_a = [&](int p, char* dstbuf, regs_t r) {
        if (!((inpatch >> p) & 1u)) return;
        if constexpr (XBF16) {
            const bool ok = (inimg >> p) & 1u;                           // zero padding: bf16 +0 is fp32 +0 rounded
            *reinterpret_cast<u32x2*>(dstbuf + awr[p]) = u32x2{ok ? r.v.x : 0u, ok ? r.v.y : 0u};
            return;
        } else {
        f32x4 v = r.v;
        if constexpr (AFFINE) {
            if (in.has_pre) v = v * r.ps + r.pb;
            if (in.pre_relu) { v.x = fmaxf(v.x, 0.f); v.y = fmaxf(v.y, 0.f); v.z = fmaxf(v.z, 0.f); v.w = fmaxf(v.w, 0.f); }
        }
        const bool ok = (inimg >> p) & 1u;                               // zero padding AFTER the prologue
        v.x = ok ? v.x : 0.f; v.y = ok ? v.y : 0.f; v.z = ok ? v.z : 0.f; v.w = ok ? v.w : 0.f;
        plane_store<NP>(dstbuf, G::A_PLANE, awr[p], v);
        }
    };
    // weight DMA: producer wave pw sends wave-instructions q = pw + 4u: rows [16 rb, 16 rb + 16) of plane q / (BN/16)
    const int pw = wv - 4;
    unsigned wsrc[NIW];                               // per-lane source element offset (without the step's k offset)
    int wdst[NIW];                                    // wave-uniform LDS byte offset inside a stage
#pragma unroll
    for (int u = 0; u < NIW; ++u) {
        const int q = pw + 4 * u;
        const int plane = q / (BN / 16), rb = q - plane * (BN / 16);
        const int r = rb * 16 + (lane >> 2);
        const int chunk = (lane & 3) ^ ((r >> 2) & 3);     // source-side swizzle (the reader XORs again)
        int n = in.n0 + r;
        n = n < in.w_rows ? n : in.w_rows - 1;              // rows past the last feed outputs that are never stored
        wsrc[u] = ((unsigned)plane * (unsigned)in.w_rows + (unsigned)n) * (unsigned)in.w_ld + (unsigned)(chunk * 8);
        wdst[u] = plane * G::B_PLANE + rb * 1024;
    }
    auto dma_b = [&](int step, int stage_idx) {        // the weight tile of `step` (clamped: a repeat goes to a stage nobody reads)
        const int sc = step < nsteps ? step : nsteps - 1;
        const int chunk = sc / T, tap = sc - chunk * T;
        const unsigned koff = (unsigned)(tap * in.tap_stride + chunk * BK);
        char* const stage = Bs + stage_idx * G::B_STAGE;
#pragma unroll
        for (int u = 0; u < NIW; ++u)
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(in.w + (wsrc[u] + koff)),
                                             (__attribute__((address_space(3))) void*)(stage + wdst[u]), 16, 0, 0);
    };

    // prologue: weight tiles of steps 0 and 1 in flight, the whole patch of chunk 0
    dma_b(0, 0);
    dma_b(1, 1);
    {
        regs_t ra[PA];
#pragma unroll
        for (int p = 0; p < PA; ++p) load_a(p, 0, ra[p]);
#pragma unroll
        for (int p = 0; p < PA; ++p) {
            wait_vm<0>(ra[p]);
            store_a(p, As, ra[p]);
        }
    }
    before_first_barrier();
    wait_then_barrier<0>();

    // Per step: DMA of step s+2 (NIW ops), then the loads of this step's patch passes (LPP ops each, PPS passes while any
    // are left); the passes loaded in step t-1 are converted and written now, behind a counted wait.  Every operation is
    // unconditional (clamped), so all counts are compile-time constants.
    auto npass = [](int t) { return t * PPS < PA ? (t * PPS + PPS <= PA ? PPS : PA - t * PPS) : 0; };      // passes loaded in step t
    regs_t ra[2][PPS];                                 // two sets: step t's loads fly while step t-1's are written
    int stage3 = 0;                                    // s % 3 (uniform)
    for (int chunk = 0; chunk < in.nchunks; ++chunk) {
        char* nxtA = As + ((chunk + 1) & 1) * G::A_BUF;
        const bool more_chunks = chunk + 1 < in.nchunks;
        const int nchunk_c = more_chunks ? chunk + 1 : chunk;      // clamped: the loads are unconditional
#pragma unroll
        for (int t = 0; t < T; ++t) {
            const int s = chunk * T + t;
            const int nload = npass(t);
            dma_b(s + 2, stage3 == 0 ? 2 : stage3 - 1);           // into the stage step s-1 read ((s+2) % 3)
#pragma unroll
            for (int u = 0; u < PPS; ++u)
                if (t * PPS + u < PA) load_a(t * PPS + u, nchunk_c, ra[t & 1][u]);
            if (t >= 1) {
#pragma unroll
                for (int u = 0; u < PPS; ++u)
                    if ((t - 1) * PPS + u < PA) {
                        // loaded in step t-1: younger ops = this step's DMA (NIW), and LPP for each later pass of step t-1
                        // and each pass of this step
                        regs_t& r = ra[(t - 1) & 1][u];
                        wait_vm_passes<NIW, LPP>(npass(t - 1) - 1 - u + nload, r);
                        if (more_chunks) store_a((t - 1) * PPS + u, nxtA, r);
                    }
            }
            // the weight tile of step s+1 (DMA issued in step s-1) has landed once all but this step's own ops are done
            switch (nload) {                                        // compile-time after unrolling
                case 0: wait_then_barrier<NIW>(); break;
                case 1: wait_then_barrier<NIW + LPP>(); break;
                default: wait_then_barrier<NIW + 2 * LPP>(); break;
            }
            stage3 = stage3 == 2 ? 0 : stage3 + 1;
        }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");              // the clamped repeats of the last two steps
}

// CONSUMER waves 0..3 (one per SIMD), from the producers' prologue to the last MFMA: LDS fragment reads + MFMA only.
// acc[i][j]: patch row cm*TM + i (32 pixels) x channels (cn*TN + j)*32 .. +31 of the tile.
template <int NP, int TM, int TN, int KS, int A_PLANE, int B_PLANE, typename AccT>
__device__ __forceinline__ void halo_emu_consume(const char* const As, const char* const Bs, int nchunks, int cm, int cn, int li, int lh,
                                                 AccT (&acc)[TM][TN]) {
    constexpr int PW = 32 + KS - 1, T = KS * KS, A_BUF = NP * A_PLANE, B_STAGE = NP * B_PLANE;
    int a_addr[T][TM][2];                                 // fragment byte offsets inside a plane, per (tap, patch row, k16 step)
#pragma unroll
    for (int t = 0; t < T; ++t)
#pragma unroll
        for (int i = 0; i < TM; ++i) {
            const int pix = (cm * TM + i + t / KS) * PW + (t % KS) + li;
            a_addr[t][i][0] = emu_a_off(pix, 0 + lh);
            a_addr[t][i][1] = emu_a_off(pix, 2 + lh);
        }
    const int sw = (li >> 2) & 3;
    const int b_off0 = (cn * TN * 32 + li) * EMU_ROW_BYTES + (((0 + lh) ^ sw) << 4);      // ks = 0
    const int b_off1 = (cn * TN * 32 + li) * EMU_ROW_BYTES + (((2 + lh) ^ sw) << 4);      // ks = 1
    wait_then_barrier<NO_VM>();                                      // the producers' prologue

    constexpr int PA_[6] = {0, 0, 1, 0, 2, 1}, PB_[6] = {0, 1, 0, 2, 0, 1};      // hh, hm, mh, hl, lh, mm (NP 1: the first)
    constexpr int NQ = NP == 3 ? 6 : 1;                                            // products per k16 block
    u32x4 fa0[NP][TM], fb0[NP][TN], fa1[NP][TM], fb1[NP][TN];
    auto read_frags = [&](const char* A, const char* B, const int (&aoff)[TM][2], int ks, int boff, u32x4 (&fa)[NP][TM], u32x4 (&fb)[NP][TN]) {
#pragma unroll
        for (int pl = 0; pl < NP; ++pl) {
#pragma unroll
            for (int i = 0; i < TM; ++i) fa[pl][i] = *reinterpret_cast<const u32x4*>(A + pl * A_PLANE + aoff[i][ks]);
#pragma unroll
            for (int j = 0; j < TN; ++j) fb[pl][j] = *reinterpret_cast<const u32x4*>(B + pl * B_PLANE + j * 32 * EMU_ROW_BYTES + boff);
        }
    };
    auto mfmas = [&](const u32x4 (&fa)[NP][TM], const u32x4 (&fb)[NP][TN]) {
#pragma unroll
        for (int q = 0; q < NQ; ++q)
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int j = 0; j < TN; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, fa[PA_[q]][i]),
                                                                        __builtin_bit_cast(bf16x8, fb[PB_[q]][j]), acc[i][j], 0, 0, 0);
    };
    // Software pipeline by half a step: the second k16 block of step s-1 runs AFTER the barrier that ends step s-1 (its
    // fragments are in registers), covering the LDS latency of step s's first fragment reads.
    int stage3 = 0;
    for (int chunk = 0; chunk < nchunks; ++chunk) {
        const char* curA = As + (chunk & 1) * A_BUF;
#pragma unroll
        for (int t = 0; t < T; ++t) {
            const int s = chunk * T + t;
            const char* curB = Bs + stage3 * B_STAGE;
            read_frags(curA, curB, a_addr[t], 0, b_off0, fa0, fb0);
            if (s > 0) mfmas(fa1, fb1);                           // (s-1, k16 block 1)
            read_frags(curA, curB, a_addr[t], 1, b_off1, fa1, fb1);
            mfmas(fa0, fb0);                                      // (s, k16 block 0)
            wait_then_barrier<NO_VM>();       // this step's fragments are in registers: its stage / patch may be overwritten
            stage3 = stage3 == 2 ? 0 : stage3 + 1;
        }
    }
    mfmas(fa1, fb1);                                              // (last step, k16 block 1)
}

// ---- the bf16x3 (NP 3) and bf16 (NP 1) halo-tile convolution of bts_conv_fwd_f32: stride-1 3x3 and sub-pixel 2x2 -----------
template <int BN, int KS, int NP>
__global__ __launch_bounds__(512, 2) void conv_halo_emu_kernel(const ConvArgs a) {
    using G = HaloEmuGeom<BN, KS, NP>;
    constexpr int MF = 32, TM = 2, TN = BN / 2 / MF;      // consumer wave tile: 2 patch rows (64 pixels) x BN/2 channels
    static_assert(G::A_PLANE % 16 == 0 && TN >= 1, "layout");
    typedef float acc_t __attribute__((ext_vector_type(16)));
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    char* const As = smem_raw;
    char* const Bs = smem_raw + 2 * G::A_BUF;

    const int swz = xcd_swizzle(blockIdx.x, gridDim.x);
    const int cls = a.subpix ? (swz & 3) : 0;
    const Tile4x32 tile = decode_tile_4x32<BN>(a.subpix ? (swz >> 2) : swz, a.n_ntiles, a.H, a.W);
    const int n0 = tile.n0, bfr = tile.bfr, y0 = tile.y0, x0 = tile.x0;
    const int spy = cls >> 1, spx = cls & 1;

    const int tid = threadIdx.x;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
    const int nchunks = a.c_in_ld / BK;                   // host: c_in_ld % 32 == 0

    if (wv >= 4) {
        const bool has_pre = a.pre_scale != nullptr;      // without: a.w, always a valid address (the loads are unconditional)
        const HaloEmuSource src = {a.x, (unsigned)a.x_pix_stride, a.H, a.W, bfr, y0, x0, a.subpix ? 1 - spy : a.pad, a.subpix ? 1 - spx : a.pad,
                                   has_pre ? a.pre_scale : a.w, has_pre ? a.pre_shift : a.w, has_pre, a.pre_relu,
                                   reinterpret_cast<const unsigned short*>(a.w_split) + (size_t)cls * NP * a.c_out_pad * a.k_pad,
                                   a.c_out_pad, a.k_pad, a.c_in_ld, n0, nchunks};
        halo_emu_produce<BN, KS, NP, true>(src, As, Bs, tid, wv, [] {});
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
    halo_emu_consume<NP, TM, TN, KS, G::A_PLANE, G::B_PLANE>(As, Bs, nchunks, cm, cn, li, lh, acc);

    // ---------------------------------------------------------------- epilogue (NHWC; conv_mfma.hip's compact paths)
    {
        const int cms = __builtin_amdgcn_readfirstlane(cm), cns = __builtin_amdgcn_readfirstlane(cn);
        const int xleft = a.W - x0;
        long pix0[TM];
        int nvalid[TM];
#pragma unroll
        for (int i = 0; i < TM; ++i) {
            const int y = y0 + cms * TM + i;
            pix0[i] = a.subpix ? ((long)bfr * (2 * a.H) + 2 * y + spy) * (2 * a.W) + 2 * x0 + spx : ((long)bfr * a.H + y) * a.W + x0;
            nvalid[i] = y < a.H ? (xleft >= MF ? MF : xleft) : 0;
        }
        if (fast_epilogue_nhwc<TM, TN, MF, 16>(a, acc, pix0, nvalid, a.subpix ? 2 : 1, n0 + cns * TN * MF, li, lh)) return;
    }
    const bool has_e1 = a.e1_scale != nullptr, has_e2 = a.e2_scale != nullptr;
#pragma unroll
    for (int i = 0; i < TM; ++i) {
        const int y = y0 + cm * TM + i;
#pragma unroll
        for (int j = 0; j < TN; ++j) {
            const int n = n0 + (cn * TN + j) * MF + li;
            float s1 = 1.f, b1 = 0.f, s2 = 1.f, b2 = 0.f;
            const bool nok = n < a.c_out;
            if (has_e1 && n < a.c_out_pad) { s1 = a.e1_scale[n]; b1 = a.e1_shift[n]; }
            if (has_e2 && n < a.c_out_pad) { s2 = a.e2_scale[n]; b2 = a.e2_shift[n]; }
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int x = x0 + (r & 3) + 8 * (r >> 2) + 4 * lh;
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
        }
    }
}

// Eligibility on top of halo_eligible(): whole 32-channel chunks (the weight DMA moves whole 64-byte rows), pre-split
// (precision 1) or pre-rounded (precision 2) weights supplied, plain NHWC output, no planar tail, dilation 1.
inline bool halo_emu_eligible(const ConvArgs& a, bool nchw) {
    if (a.w_split == nullptr || nchw || a.n_tail > 0 || a.dil != 1 || (a.c_in_ld % BK) != 0) return false;
    if (((uintptr_t)a.w_split & 15) || (a.k_pad & 7)) return false;
    return halo_eligible(a, true, 32, nullptr);
}

template <int BN, int KS, int NP = 3>
int launch_halo_emu(const ConvArgs& a0, const ConvRun& r) {
    ConvArgs a = a0;
    const long n_mtiles = (long)a.B * tiles_4x32(a.H, a.W);
    a.n_ntiles = (a.c_out + BN - 1) / BN;
    a.tiles_per_class = (int)(n_mtiles * a.n_ntiles);
    a.ksplit = 1;
    const long nwg = n_mtiles * a.n_ntiles * a.n_classes;
    constexpr size_t lds = (size_t)HaloEmuGeom<BN, KS, NP>::LDS_BYTES;
    static_assert(lds <= 160 * 1024, "LDS");
    return conv_launch<conv_halo_emu_kernel<BN, KS, NP>>(r, ConvChoice{NP == 3 ? BTS_CONV_KIND_HALO_EMU : BTS_CONV_KIND_HALO_BF16, 128, BN, 1},
                                                         BTS_ERR_INVALID, nwg, nwg, 512, lds, a);
}
