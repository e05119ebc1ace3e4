// Planar-tail 3x3 convolution (decoder conv3 / conv2) with bf16 main operands: conv_halo_emu_kernel<BN, 3, 1>'s one-plane
// halo tile over the MAIN channels, plus the one-plane tail added in fp32 before the epilogue (included by conv_mfma.hip
// inside its anonymous namespace, after conv_halo_emu.inc whose helpers it shares).  Opt-in: its own entry point
// (bts_conv_tail_bf16_fwd_f32); bts_conv_fwd_f32 keeps these layers on conv_halo_kernel<..., tail> whatever `precision` says.
//
//   y[b][y][x][n] = e2(act( sum_{tap,c<c_main} bf16(x[b][y+dy][x+dx][c]) * w_main[n][tap*c_main + c]      (fp32 accumulation)
//                         + sum_tap t[b][y+dy][x+dx] * w_tail[n][tap][0] ))                               (fp32 FMAs, unrounded)
//
// What is the halo-emu kernel's, unchanged: the 4 x 32-pixel tile of one frame, four consumer waves (2 row pairs x 2
// channel halves, LDS fragment reads + v_mfma_f32_32x32x16_bf16 only) and four producer waves (weight LDS-DMA three stages
// deep, the next chunk's patch one 32-pixel pass per tap-step, rounded to nearest even on its way to LDS), raw s_barrier
// with counted vmcnt, swizzled 64-byte rows (emu_a_off).  What differs:
//   * WEIGHTS are two operands of their own.  The layer's packed K axis is tap * (c_main + 4) + c, which puts the main block
//     of an odd tap at a byte offset that is no multiple of 16 in a bf16 plane; w_main is re-laid as [c_out_pad][9 * c_main]
//     (k = tap * c_main + c), so every tap-step's 64-byte DMA rows are 16-byte aligned.  w_tail is fp32 [c_out_pad][9][4].
//   * NO prologue affine: the patch pass is ONE untracked load (three in conv_halo_emu_kernel: value, scale, shift), and the
//     counted waits are written for that: a tap-step issues NIW DMA instructions and at most one patch load.
//   * THE TAIL: the producers stage the tile's 6 x 34 plane values (zero outside the map) into LDS once, in the prologue.
//     After the K loop a consumer lane reads, per four adjacent outputs, the 3 x 6 plane values they share (a broadcast
//     read: the address depends on the lane's k-half only) and adds nine fp32 FMAs per output and channel tile.
constexpr int TAILBF_PW = 34, TAILBF_PH = 6;

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
constexpr int tail_bf16_lds_bytes() {
    return 2 * (TAILBF_PH * TAILBF_PW) * EMU_ROW_BYTES + 3 * BN * EMU_ROW_BYTES + TAILBF_PH * TAILBF_PW * 4;
}

template <int N> __device__ __forceinline__ void wait_vm1(f32x4& v) {
    asm volatile("s_waitcnt vmcnt(%1)" : "+v"(v) : "n"(N) : "memory");
}

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

// Four waves per SIMD (two workgroups per CU: one's prologue, tail and epilogue run under the other's MFMAs): a 128-register
// budget, which both instantiations meet without scratch (DESIGN 3c)
template <int BN>
__global__ __launch_bounds__(512, 4) void conv_tail_bf16_kernel(const TailBf16Args a) {
    constexpr int KS = 3, MF = 32, TM = 2, TN = BN / 2 / MF;
    constexpr int TW = 32, TH = 4, PH = TAILBF_PH, PW = TAILBF_PW, NPIX = PH * PW, T = KS * KS;
    constexpr int RPP = 256 / 8;                         // patch pixels staged per pass by the 256 producer threads
    constexpr int PA = (NPIX + RPP - 1) / RPP;           // passes over the patch: 7, one per tap-step
    constexpr int A_BUF = NPIX * EMU_ROW_BYTES;
    constexpr int B_STAGE = BN * EMU_ROW_BYTES;
    constexpr int NI = BN / 16;                          // DMA wave-instructions per weight stage (16 rows x 64 B each)
    constexpr int NIW = NI / 4;                          // ... per producer wave: 2 / 1 (BN 128 / 64)
    static_assert(NI % 4 == 0 && T - 1 >= PA && TN >= 1, "producer work divides evenly");
    typedef float acc_t __attribute__((ext_vector_type(16)));
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    char* const As = smem_raw;                            // [2][NPIX][64 B]
    char* const Bs = smem_raw + 2 * A_BUF;                // [3 stages][BN][64 B]
    float* const Ts = reinterpret_cast<float*>(smem_raw + 2 * A_BUF + 3 * B_STAGE);      // [6][34] plane values of the tile

    // ---- tile decode (as conv_halo_emu_kernel)
    const int nwg = gridDim.x, bid = blockIdx.x;
    const int swz = xcd_swizzle(bid, nwg);
    const int mt_idx = swz / a.n_ntiles, nt_idx = swz - mt_idx * a.n_ntiles;
    const int n0 = nt_idx * BN;
    const int n_tx = (a.W + TW - 1) / TW, n_ty = (a.H + TH - 1) / TH;
    const int bfr = mt_idx / (n_tx * n_ty);
    const int trem = mt_idx - bfr * (n_tx * n_ty);
    const int tyi = trem / n_tx;
    const int y0 = tyi * TH, x0 = (trem - tyi * n_tx) * TW;

    const int tid = threadIdx.x;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
    const int nchunks = a.c_main / BK;                    // host: c_main % 32 == 0
    const int nsteps = nchunks * T;
    const int kmain = T * a.c_main;                       // row length of w_main

    if (wv >= 4) {
        // =============================================================== PRODUCER waves 4..7 (one per SIMD)
        const int ptid = tid - 256;
        const int lrow = ptid >> 3, lk = (ptid & 7) * 4;
        unsigned abase[PA];
        int awr[PA];
        unsigned inimg = 0, inpatch = 0;
#pragma unroll
        for (int p = 0; p < PA; ++p) {
            const int pix = p * RPP + lrow;
            const int pyy = pix / PW, pxx = pix - pyy * PW;
            const int gy = y0 - 1 + pyy, gx = x0 - 1 + pxx;
            const bool inp = pix < NPIX;
            const bool ok = inp && (unsigned)gy < (unsigned)a.H && (unsigned)gx < (unsigned)a.W;
            const int yc = min(max(gy, 0), a.H - 1), xc = min(max(gx, 0), a.W - 1);
            abase[p] = ((unsigned)bfr * (unsigned)(a.H * a.W) + (unsigned)(yc * a.W + xc)) * (unsigned)a.x_pix_stride + (unsigned)lk;
            awr[p] = emu_a_off(inp ? pix : 0, lk >> 3) + (lk & 7) * 2;
            inimg |= (ok ? 1u : 0u) << p;
            inpatch |= (inp ? 1u : 0u) << p;
        }
        auto load_a = [&](int p, int chunk, f32x4& v) { load_untracked(v, a.x + (abase[p] + (unsigned)(chunk * BK))); };
        auto store_a = [&](int p, char* dstbuf, f32x4 v) {
            if (!((inpatch >> p) & 1u)) return;
            const bool ok = (inimg >> p) & 1u;                               // zero padding
            v.x = ok ? v.x : 0.f; v.y = ok ? v.y : 0.f; v.z = ok ? v.z : 0.f; v.w = ok ? v.w : 0.f;
            rne_store(dstbuf, awr[p], v);
        };
        // weight DMA: producer wave pw sends wave-instructions q = pw + 4u: rows [16 q, 16 q + 16) of the stage
        const int pw = wv - 4;
        unsigned wsrc[NIW];                               // per-lane source element offset (without the step's k offset)
        int wdst[NIW];                                    // wave-uniform LDS byte offset inside a stage
#pragma unroll
        for (int u = 0; u < NIW; ++u) {
            const int rb = pw + 4 * u;
            const int r = rb * 16 + (lane >> 2);
            const int chunk = (lane & 3) ^ ((r >> 2) & 3);     // source-side swizzle (the reader XORs again)
            int n = n0 + r;
            n = n < a.c_out_pad ? n : a.c_out_pad - 1;          // rows past c_out_pad feed outputs that are never stored
            wsrc[u] = (unsigned)n * (unsigned)kmain + (unsigned)(chunk * 8);
            wdst[u] = rb * 1024;
        }
        auto dma_b = [&](int step, int stage_idx) {        // the weight tile of `step` (clamped: a repeat goes to a stage nobody reads)
            const int sc = step < nsteps ? step : nsteps - 1;
            const int chunk = sc / T, tap = sc - chunk * T;
            const unsigned koff = (unsigned)(tap * a.c_main + chunk * BK);
            char* const stage = Bs + stage_idx * B_STAGE;
#pragma unroll
            for (int u = 0; u < NIW; ++u)
                __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(a.w_main + (wsrc[u] + koff)),
                                                 (__attribute__((address_space(3))) void*)(stage + wdst[u]), 16, 0, 0);
        };

        // prologue: weight tiles of steps 0 and 1 in flight, the whole patch of chunk 0, the tile's plane values
        dma_b(0, 0);
        dma_b(1, 1);
        {
            f32x4 va[PA];
#pragma unroll
            for (int p = 0; p < PA; ++p) load_a(p, 0, va[p]);
#pragma unroll
            for (int p = 0; p < PA; ++p) {
                wait_vm1<0>(va[p]);
                store_a(p, As, va[p]);
            }
        }
        if (ptid < NPIX) {
            const int pyy = ptid / PW, pxx = ptid - pyy * PW;
            const int gy = y0 - 1 + pyy, gx = x0 - 1 + pxx;
            const bool ok = (unsigned)gy < (unsigned)a.H && (unsigned)gx < (unsigned)a.W;
            const int yc = min(max(gy, 0), a.H - 1), xc = min(max(gx, 0), a.W - 1);
            const float tv = a.tail[((long)bfr * a.H + yc) * a.W + xc];
            Ts[ptid] = ok ? tv : 0.f;
        }
        asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");

        // Per step: DMA of step s+2 (NIW ops), then the load of this step's patch pass (1 op, steps 0..PA-1); the pass loaded in
        // step t-1 is rounded and written now, behind a counted wait.  Every operation is unconditional (clamped), so all
        // counts are compile-time constants.
        f32x4 va[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};      // step t's load flies while step t-1's is written
        int stage3 = 0;                                    // s % 3 (uniform)
        for (int chunk = 0; chunk < nchunks; ++chunk) {
            char* nxtA = As + ((chunk + 1) & 1) * A_BUF;
            const bool more_chunks = chunk + 1 < nchunks;
            const int nchunk_c = more_chunks ? chunk + 1 : chunk;      // clamped: the loads are unconditional
#pragma unroll
            for (int t = 0; t < T; ++t) {
                const int s = chunk * T + t;
                const int nload = t < PA ? 1 : 0;                      // compile-time after unrolling
                dma_b(s + 2, stage3 == 0 ? 2 : stage3 - 1);           // into the stage step s-1 read ((s+2) % 3)
                if (t < PA) load_a(t, nchunk_c, va[t & 1]);
                if (t >= 1 && t - 1 < PA) {
                    // loaded in step t-1: younger ops = this step's DMA (NIW) and load (nload)
                    if (nload) wait_vm1<NIW + 1>(va[(t - 1) & 1]);
                    else wait_vm1<NIW>(va[(t - 1) & 1]);
                    if (more_chunks) store_a(t - 1, nxtA, va[(t - 1) & 1]);
                }
                // the weight tile of step s+1 (DMA issued in step s-1) has landed once all but this step's own ops are done
                if (nload) asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)" :: "n"(NIW + 1) : "memory");
                else asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)" :: "n"(NIW) : "memory");
                __builtin_amdgcn_s_barrier();
                asm volatile("" ::: "memory");
                stage3 = stage3 == 2 ? 0 : stage3 + 1;
            }
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");              // the clamped repeats of the last two steps
        return;
    }

    // =================================================================== CONSUMER waves 0..3 (one per SIMD): LDS reads + MFMA only
    const int cm = wv >> 1, cn = wv & 1;
    const int li = lane & 31, lh = lane >> 5;
    int a_addr[T][TM][2];                                 // fragment byte offsets, per (tap, patch row, k16 step)
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
    acc_t acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();                                    // the producers' prologue
    asm volatile("" ::: "memory");

    u32x4 fa0[TM], fb0[TN], fa1[TM], fb1[TN];
    auto read_frags = [&](const char* A, const char* B, const int (&aoff)[TM][2], int ks, int boff, u32x4 (&fa)[TM], u32x4 (&fb)[TN]) {
#pragma unroll
        for (int i = 0; i < TM; ++i) fa[i] = *reinterpret_cast<const u32x4*>(A + aoff[i][ks]);
#pragma unroll
        for (int j = 0; j < TN; ++j) fb[j] = *reinterpret_cast<const u32x4*>(B + j * 32 * EMU_ROW_BYTES + boff);
    };
    auto mfmas = [&](const u32x4 (&fa)[TM], const u32x4 (&fb)[TN]) {
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int j = 0; j < TN; ++j)
                acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, fa[i]), __builtin_bit_cast(bf16x8, fb[j]),
                                                                    acc[i][j], 0, 0, 0);
    };
    // Software pipeline by half a step, as conv_halo_emu_kernel
    {
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
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");    // this step's fragments are in registers
                __builtin_amdgcn_s_barrier();
                asm volatile("" ::: "memory");
                stage3 = stage3 == 2 ? 0 : stage3 + 1;
            }
        }
        mfmas(fa1, fb1);                                              // (last step, k16 block 1)
    }

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
    const long ntx = (W + 31) / 32, nty = (H + 3) / 4;
    const int bn = tail_bf16_bn(c_out);
    *wgs_per_frame = ntx * nty * ((c_out + bn - 1) / bn);
    return (double)H * W / (double)(ntx * 32 * nty * 4) >= kTailBf16MinFill;
}

template <int BN>
int launch_tail_bf16(TailBf16Args a, hipStream_t s) {
    const long n_mtiles = (long)a.B * ((a.H + 3) / 4) * ((a.W + 31) / 32);
    a.n_ntiles = (a.c_out + BN - 1) / BN;
    const long nwg = n_mtiles * a.n_ntiles;
    if (nwg > 0x7fffffffL) return BTS_ERR_UNSUPPORTED;
    constexpr size_t lds = (size_t)tail_bf16_lds_bytes<BN>();
    static_assert(lds <= 80 * 1024, "two workgroups per CU");
    auto k = conv_tail_bf16_kernel<BN>;
    static std::atomic<unsigned long long> lds_set{0};
    if (hipError_t e = bts_ensure_dynamic_lds((const void*)k, lds, lds_set); e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(k, dim3((unsigned)nwg), dim3(512), lds, s, a);
    return (int)hipGetLastError();
}
