// Fused Winograd F(2x2, 3x3) convolution on the fp32-input MFMA (included by conv_mfma.hip inside its anonymous namespace).
//
// A stride-1 3x3 convolution costs 9 multiply-adds per output and input channel.  Winograd's F(2x2,3x3) computes a 2x2
// block of outputs from a 4x4 input window with 16: 4 per output, 2.25x fewer -- the one lever left on the ~20 ms of
// stride-1 3x3 work once the direct kernels sit at 0.8 of the matrix pipe (DESIGN 7).  Non-fused it is hopeless here (the
// transformed tensors are 4x the activations: HBM-bound below ~400 channels); this kernel keeps everything on chip:
//
//   Y = A^T [ sum_c (G g_c G^T) .* (B^T d_c B) ] A        per 2x2 output block ("tile"), d = its 4x4 input window
//
//   * U = G g G^T is computed OFFLINE per (c_out, c_in) (ops.pack_wino_weight) and stored in MFMA B-fragment order, so a
//     wave loads the fragments of its 16 MFMAs with one coalesced 1-KB global load: no LDS, no staging for the weights.
//     (The 16 transform positions xi are 16 INDEPENDENT GEMMs: no two waves share a weight fragment.)
//   * A workgroup owns 4 x 8 = 32 tiles (8 x 16 output pixels) x BN output channels.  Per 32-channel chunk its 10 x 18-pixel
//     input patch is staged into LDS once (as the halo kernel does: prologue = BN affine + ReLU, zero padding after it);
//     every thread then reads ONE tile's 4x4 window for ONE channel pair from it (16 x ds_read_b64 at immediate offsets),
//     transforms (B^T d B: 32 adds per channel) and writes the 16 values V[xi][tile][c] back to LDS.  V is double-buffered:
//     the transform of chunk c+1 runs between the MFMA groups of chunk c.  (The first version read the windows straight
//     from global memory -- every pixel four times, 16 eight-byte loads with 64-bit addresses per thread and chunk, the
//     prologue applied to all 16 -- and spent 29 % of its time there: ablation in gpurun_out/r3s.)
//   * GEMM per xi: M[xi][32 tiles][BN] += V[xi][32 tiles][32 c] * U[xi][32 c][BN] on v_mfma_f32_32x32x2_f32, the 16 xi
//     spread over the 8 waves (wave w owns xi = 2w, 2w+1 and all BN channels: 2 x BN/32 accumulator tiles).
//   * After the last chunk the accumulators go through LDS once (the V buffers are free by then) so that a thread holds
//     all 16 xi of one (tile, 4 channels); it applies A^T M A, the epilogue (affine, activation, affine) and stores the
//     2x2 pixels x 4 channels.
//
// Numerics: every product is an exact-f32 MFMA product as in the direct kernels; the transforms add and subtract f32
// values (G's 1/2 and 1/4 are exact), so the result differs from the direct kernels by a few ulp of the LARGEST partial
// sum (measured against fp64 in tests/test_round3_gpu.py next to the direct kernel's own error).
constexpr int WINO_PLD = 36;            // floats per patch pixel row (32 channels + 4 pad: a window pixel is base + immediate)
constexpr int WINO_PPIX = 10 * 18;      // input patch of the 8 x 16-pixel workgroup tile, with halo

// V rows are UNPADDED (128 B = 32 channels) so that two buffers and the patch fit the LDS; the eight 16-byte chunks of a
// row are XOR-swizzled with bits 1-3 of the row (tile) index: a ds_read_b128 lane group reads rows {0-3, 12-15, 20-27}
// + const, whose (row parity, chunk ^ (row >> 1 & 7)) pairs -- the 16-byte bank slots -- are all distinct.
__device__ __forceinline__ int wino_v_off(int row, int chunk16) { return row * 128 + (((chunk16 ^ (row >> 1)) & 7) << 4); }

template <int BN, bool TAIL = false>
constexpr int wino_lds_bytes() {
    constexpr int v = 2 * 16 * 32 * 128 + WINO_PPIX * WINO_PLD * 4;      // V double buffer + patch
    // epilogue: exchange [16 xi][32 tiles][64 + 4 channels]; planar tail: + its patch [180 px][4] + its weights [9 taps][BN][4]
    constexpr int m = 16 * 32 * 68 * 4 + (TAIL ? WINO_PPIX * 16 + 9 * BN * 16 : 0);
    return v > m ? v : m;
}

// TAIL (bts_conv_desc.tail_planes, conv3 / conv2 of the decoder): up to four extra input channels that live in dense
// one-channel planes -- the LPG depth maps.  They do NOT go through the Winograd transforms: a depth map may hold +-inf
// (a denominator that is exactly 0, bts.py:168-173) or values 1e3 times its neighbours' (the +-1e-3 clamp), and B^T d B
// would smear such a pixel over its whole 4x4 window (inf - inf = NaN; rounding relative to the LARGEST value of the
// window).  The main channels run as above; the tail's 9 x n_tail products per output are added DIRECTLY in the epilogue
// (VALU, from the tail patch staged in LDS and the packed fp32 weights): the same non-finite pattern and the same
// per-product accuracy as the direct kernels.
template <int BN, bool TAIL = false>
__global__ __launch_bounds__(512, 2) void conv_wino_kernel(const ConvArgs a) {
    // BN = 48 (DenseNet growth convolutions, c_out = 48): v_mfma_f32_16x16x4_f32 tiles -- two 16-tile row tiles x three
    // 16-channel column tiles per transform position -- instead of padding the 48 channels to two 32-wide tiles (25 % of
    // the MFMA work wasted).  Same V image, same transforms; U is packed for the 16x16x4 B operand (ops.pack_wino_weight).
    constexpr bool MF16 = BN == 48;
    constexpr int NTL = MF16 ? 3 : BN / 32;                       // output-channel tiles per workgroup (16 wide when MF16, else 32)
    constexpr int NGRP = MF16 ? 4 : 8;                            // fragment groups per chunk and wave: 2 xi x (32 k / KG), KG = 16 (MF16) or 8
    // (Measured and dropped, gpurun_out/r3y: a producer / consumer split for BN <= 64 -- waves 0..3 only MFMA, four
    // transform positions each, waves 4..7 stage and transform for everyone.  One MFMA wave per SIMD does not keep the
    // pipe fed between its own fragment reads and weight loads: block-1 growth convolutions 431-467 -> 473-494 us, conv2
    // 2.10 -> 2.56 ms, whole step 34.2 -> 35.6 ms.)
    constexpr int TY = 4, TX = 8;                                 // Winograd tiles per workgroup: 4 rows x 8 columns (8 x 16 pixels)
    constexpr int V_BUF = 16 * 32 * 128;                          // bytes per V buffer
    constexpr int PW = 18;                                        // patch width in pixels
    constexpr int RPP = 64, PA = (WINO_PPIX + RPP - 1) / RPP;     // patch pixels per staging pass, passes (3)
    typedef float acc_t __attribute__((ext_vector_type(16)));
    typedef float f32x2 __attribute__((ext_vector_type(2)));
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    char* const Vs = smem_raw;                                    // [2][16 xi][32 tiles][128 B]
    float* const Ps = reinterpret_cast<float*>(smem_raw + 2 * V_BUF);      // [180 px][36]

    // ---- PERSISTENT workgroups: this one runs tiles blockIdx.x, + gridDim.x, ... of the launch's tiles_per_class tiles (the host
    //      sizes the grid so that every workgroup gets the same number of tiles, +-1).  A 157 KB-LDS workgroup is alone on its
    //      CU, so between two one-tile workgroups the CU sat idle from the first output store to the next workgroup's first
    //      landed load (measured by ablation: the output stores alone were 13 % of a 6-chunk layer, the prologue's load latency
    //      another 5 %).  Here the next tile's first patch loads are issued BEFORE the epilogue, wait behind its LDS exchange
    //      and arithmetic, and the stores drain under the next tile's prologue.
    const int tid = threadIdx.x;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
    const int li = lane & 31, lh = lane >> 5;
    const int c_main = TAIL ? a.c_in_ld - 4 : a.c_in_ld;           // channels read from the NHWC buffer
    const int nchunks = c_main / BK;                               // host: whole 32-channel chunks
    const int n_tx = (a.W + 2 * TX - 1) / (2 * TX), n_ty = (a.H + 2 * TY - 1) / (2 * TY);
    const int ntiles = a.tiles_per_class;

    // ---- patch staging (as conv_halo_kernel): pass p covers patch pixels [64 p, 64 p + 64), thread = (pixel lrow, channels lk..lk+3)
    const int lrow = tid >> 3, lk = (tid & 7) * 4;
    unsigned abase[PA];
    [[maybe_unused]] unsigned pbase[TAIL ? PA : 1];                // pixel index inside a plane (planar tail)
    unsigned inimg = 0, inpatch = 0;
    int n0 = 0, bfr = 0, y0 = 0, x0 = 0;                           // of the tile whose patches are being staged
    auto decode = [&](int bid) {                                   // tile decode (XCD-aware bijective swizzle over the ntiles tile ids)
        const int swz = xcd_swizzle(bid, ntiles);
        const int mt_idx = swz / a.n_ntiles, nt_idx = swz - mt_idx * a.n_ntiles;
        n0 = nt_idx * BN;
        bfr = mt_idx / (n_tx * n_ty);
        const int trem = mt_idx - bfr * (n_tx * n_ty);
        const int tyi = trem / n_tx;
        y0 = tyi * 2 * TY; x0 = (trem - tyi * n_tx) * 2 * TX;      // first output pixel of the tile
        inimg = 0; inpatch = 0;
#pragma unroll
        for (int p = 0; p < PA; ++p) {
            const int pix = p * RPP + lrow;
            const int pyy = pix / PW, pxx = pix - pyy * PW;
            const int gy = y0 - 1 + pyy, gx = x0 - 1 + pxx;
            const bool inp = pix < WINO_PPIX;
            const bool ok = inp && (unsigned)gy < (unsigned)a.H && (unsigned)gx < (unsigned)a.W;
            const int yc = min(max(gy, 0), a.H - 1), xc = min(max(gx, 0), a.W - 1);
            if constexpr (TAIL) pbase[p] = (unsigned)bfr * (unsigned)(a.H * a.W) + (unsigned)(yc * a.W + xc);
            abase[p] = ((unsigned)bfr * (unsigned)(a.H * a.W) + (unsigned)(yc * a.W + xc)) * (unsigned)a.x_pix_stride + (unsigned)lk;
            inimg |= (ok ? 1u : 0u) << p;
            inpatch |= (inp ? 1u : 0u) << p;
        }
    };
    int bid = blockIdx.x;
    decode(bid);
    const bool has_pre = a.pre_scale != nullptr;
    const float* const psrc = has_pre ? a.pre_scale : a.w;         // unconditional loads: any valid address when there is no prologue
    const float* const bsrc = has_pre ? a.pre_shift : a.w;
    f32x4 pin[PA], ps4 = {1.f, 1.f, 1.f, 1.f}, pb4 = {0.f, 0.f, 0.f, 0.f};
    auto load_patch = [&](int chunk) {                             // loads only (clamped): nothing touches the values here
        const unsigned cs = (unsigned)(chunk * BK);
#pragma unroll
        for (int p = 0; p < PA; ++p) pin[p] = *reinterpret_cast<const f32x4*>(a.x + (abase[p] + cs));
        ps4 = *reinterpret_cast<const f32x4*>(psrc + (cs + lk));
        pb4 = *reinterpret_cast<const f32x4*>(bsrc + (cs + lk));
    };
    auto store_patch = [&](int chunk) {                            // prologue (BN affine + ReLU), zero padding AFTER it, to LDS
        f32x4 s4 = ps4, b4 = pb4;
        asm volatile("" : "+v"(s4), "+v"(b4));
#pragma unroll
        for (int p = 0; p < PA; ++p) {
            f32x4 v = pin[p];
            asm volatile("" : "+v"(v));                            // first use pinned here (conv_halo.inc)
            if (has_pre) v = v * s4 + b4;
            if (a.pre_relu) { v.x = fmaxf(v.x, 0.f); v.y = fmaxf(v.y, 0.f); v.z = fmaxf(v.z, 0.f); v.w = fmaxf(v.w, 0.f); }
            const bool ok = (inimg >> p) & 1u;
            v.x = ok ? v.x : 0.f; v.y = ok ? v.y : 0.f; v.z = ok ? v.z : 0.f; v.w = ok ? v.w : 0.f;
            if ((inpatch >> p) & 1u) *reinterpret_cast<f32x4*>(Ps + (p * RPP + lrow) * WINO_PLD + lk) = v;
        }
    };
    // ---- this thread's transform item: tile tau (0..31), channel pair cp (0..15) of the chunk
    const int tau = tid >> 4, cp = tid & 15;
    const int ty = tau >> 3, tx = tau & 7;
    const float* const pwin = Ps + ((2 * ty) * PW + 2 * tx) * WINO_PLD + 2 * cp;       // window pixel (r, c): + (r * PW + c) * WINO_PLD
    const int v_wr = wino_v_off(tau, cp >> 1) + (cp & 1) * 8;      // byte offset inside one xi plane
    auto transform_store = [&](char* vbuf) {
        f32x2 d[16];
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int c = 0; c < 4; ++c) d[4 * r + c] = *reinterpret_cast<const f32x2*>(pwin + (r * PW + c) * WINO_PLD);
        f32x2 t[16];
#pragma unroll
        for (int c = 0; c < 4; ++c) {                              // B^T d  (over rows)
            t[0 * 4 + c] = d[0 * 4 + c] - d[2 * 4 + c];
            t[1 * 4 + c] = d[1 * 4 + c] + d[2 * 4 + c];
            t[2 * 4 + c] = d[2 * 4 + c] - d[1 * 4 + c];
            t[3 * 4 + c] = d[1 * 4 + c] - d[3 * 4 + c];
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {                              // (B^T d) B  (over columns)
            const f32x2 v0 = t[r * 4 + 0] - t[r * 4 + 2];
            const f32x2 v1 = t[r * 4 + 1] + t[r * 4 + 2];
            const f32x2 v2 = t[r * 4 + 2] - t[r * 4 + 1];
            const f32x2 v3 = t[r * 4 + 1] - t[r * 4 + 3];
            *reinterpret_cast<f32x2*>(vbuf + (4 * r + 0) * 4096 + v_wr) = v0;
            *reinterpret_cast<f32x2*>(vbuf + (4 * r + 1) * 4096 + v_wr) = v1;
            *reinterpret_cast<f32x2*>(vbuf + (4 * r + 2) * 4096 + v_wr) = v2;
            *reinterpret_cast<f32x2*>(vbuf + (4 * r + 3) * 4096 + v_wr) = v3;
        }
    };

    // ---- weights: fragment-ordered U, [16 xi][nchunks][channel tiles][groups per chunk][64 lanes][4]
    //      (32-wide tiles, 4 groups of 8 k -- or, MF16, 16-wide tiles and 2 groups of 16 k; host: whole tiles per workgroup)
    constexpr int GPC = MF16 ? 2 : 4;                              // groups per chunk
    const int n_ct = MF16 ? a.c_out / 16 : a.c_out_pad / 32;
    const f32x4* ubase = nullptr;                                  // set per tile (depends on its channel tile n0)
    const size_t xi_stride = (size_t)nchunks * n_ct * (GPC * 64), chunk_stride = (size_t)n_ct * (GPC * 64);
    auto ufrag = [&](int e, int chunk, int j, int g) -> f32x4 { return ubase[e * xi_stride + chunk * chunk_stride + j * (GPC * 64) + g * 64]; };

    acc_t acc[2][MF16 ? 1 : NTL];                                  // 32x32 tiles: [xi slot][channel tile]
    f32x4 acc16[2][2][MF16 ? NTL : 1];                             // 16x16 tiles: [xi slot][row tile][channel tile]
    // A-fragment byte offsets inside an xi plane: 32x32x2: row li, chunk 2g + lh per group g (4);
    // 16x16x4: row 16 i + (lane & 15), chunk 4 g + (lane >> 4) per (row tile i, group g) (2 x 2)
    int a_off[4];
#pragma unroll
    for (int g = 0; g < 4; ++g) a_off[g] = MF16 ? wino_v_off(16 * (g >> 1) + (lane & 15), 4 * (g & 1) + (lane >> 4)) : wino_v_off(li, 2 * g + lh);
    const bool late = wv >= 4;                                     // waves 4..7 transform half a chunk later than their SIMD partners
    load_patch(0);                                                 // chunk 0 of the first tile
  for (;;) {                                                       // ---- one tile per iteration; pin[] holds its chunk 0 (in flight)
    ubase = reinterpret_cast<const f32x4*>(a.w_wino) + ((size_t)(2 * wv) * nchunks * n_ct + n0 / (MF16 ? 16 : 32)) * (GPC * 64) + lane;
#pragma unroll
    for (int e = 0; e < 2; ++e) {
#pragma unroll
        for (int j = 0; j < (MF16 ? 1 : NTL); ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[e][j][r] = 0.f;
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < (MF16 ? NTL : 1); ++j) acc16[e][i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    }

    // ---- prologue: patch and V of chunk 0, patch registers of chunk 1, first weight fragments
    store_patch(0);
    load_patch(nchunks > 1 ? 1 : 0);
    __syncthreads();
    transform_store(Vs);
    f32x4 ub[2][NTL];                                              // weight fragments: two-slot ring, one group ahead
#pragma unroll
    for (int j = 0; j < NTL; ++j) ub[0][j] = ufrag(0, 0, j, 0);
    __syncthreads();

    for (int chunk = 0; chunk < nchunks; ++chunk) {
        const char* cur = Vs + (chunk & 1) * V_BUF;
        char* nxt = Vs + ((chunk + 1) & 1) * V_BUF;
        const bool more = chunk + 1 < nchunks;
        // the next chunk's patch goes to LDS first (its loads are a chunk old), the loads of the one after follow
        if (more) store_patch(chunk + 1);
        load_patch(chunk + 2 < nchunks ? chunk + 2 : nchunks - 1);
#pragma unroll
        for (int grp = 0; grp < NGRP; ++grp) {
            const int e = grp / GPC, g = grp % GPC;
            {                                                      // next group's fragments (the next chunk's first group at the end)
                const int ne = grp + 1 < NGRP ? (grp + 1) / GPC : 0, ng = (grp + 1) % GPC;
                const int nc = grp + 1 < NGRP ? chunk : (more ? chunk + 1 : chunk);
#pragma unroll
                for (int j = 0; j < NTL; ++j) ub[(grp + 1) & 1][j] = ufrag(ne, nc, j, ng);
            }
            if constexpr (MF16) {
                f32x4 fa[2];
#pragma unroll
                for (int i = 0; i < 2; ++i) fa[i] = *reinterpret_cast<const f32x4*>(cur + (2 * wv + e) * 4096 + a_off[2 * i + g]);
#pragma unroll
                for (int q = 0; q < 4; ++q)
#pragma unroll
                    for (int i = 0; i < 2; ++i)
#pragma unroll
                        for (int j = 0; j < NTL; ++j)
                            acc16[e][i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(fa[i][q], ub[grp & 1][j][q], acc16[e][i][j], 0, 0, 0);
            } else {
                const f32x4 fa = *reinterpret_cast<const f32x4*>(cur + (2 * wv + e) * 4096 + a_off[g]);
#pragma unroll
                for (int q = 0; q < 4; ++q)
#pragma unroll
                    for (int j = 0; j < NTL; ++j)
                        acc[e][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[q], ub[grp & 1][j][q], acc[e][j], 0, 0, 0);
            }
            if (grp == 0) __syncthreads();                         // the patch of chunk + 1 is complete in LDS
            if (grp == (late ? NGRP / 2 : 1) && more) transform_store(nxt);      // in the shadow of the remaining groups
        }
        __syncthreads();                                           // V[nxt] complete, V[cur] and the patch free
    }
    // ---------------------------------------------------------------- output transform + epilogue
    // M[xi][tile][64 channels] through LDS (the V buffers are free), 64 channels per pass
    float* const Ms = reinterpret_cast<float*>(smem_raw);          // [16 xi][32 tiles][68] (V buffers and patch are free)
    constexpr int M_LD = 68;
    const int cq = tid & 15;                                        // this thread's 4 channels of the pass
    const bool has_e1 = a.e1_scale != nullptr, has_e2 = a.e2_scale != nullptr;
    constexpr int NPASS = MF16 ? 1 : (NTL + 1) / 2;
    [[maybe_unused]] float* const Ts = reinterpret_cast<float*>(smem_raw + 16 * 32 * M_LD * 4);      // planar tail patch [180 px][4], behind M
    [[maybe_unused]] f32x4* const Wt = reinterpret_cast<f32x4*>(smem_raw + 16 * 32 * M_LD * 4 + WINO_PPIX * 16);      // tail weights [9][BN], behind it
    if constexpr (TAIL) {
        static_assert(wino_lds_bytes<BN, true>() <= 160 * 1024, "tail patch and weights fit behind the exchange buffer");
        // the tail channels' weights [tap][channel of the tile][4 tail slots] (fp32, from the packed direct-form matrix: K index
        // tap * c_in_ld + c_main): 9 x BN 16-byte items, staged per tile (this region is the patch during the main loop)
        for (int i = tid; i < 9 * BN; i += 512) {
            const int tap = i / BN, ch = i - tap * BN;
            Wt[i] = *reinterpret_cast<const f32x4*>(a.w + ((size_t)(n0 + ch) * a.k_pad + tap * a.c_in_ld + c_main));
        }
        if (lk == 0) {                                              // one lane per patch pixel (unused planes alias plane 0)
#pragma unroll
            for (int p = 0; p < PA; ++p) {
                f32x4 v = f32x4{a.tail[0][pbase[p]], a.tail[1][pbase[p]], a.tail[2][pbase[p]], a.tail[3][pbase[p]]};
                const bool ok = (inimg >> p) & 1u;                  // zero padding; unused tail slots are zero (their weights are too)
                v.x = ok ? v.x : 0.f; v.y = ok && a.n_tail > 1 ? v.y : 0.f; v.z = ok && a.n_tail > 2 ? v.z : 0.f; v.w = ok && a.n_tail > 3 ? v.w : 0.f;
                if ((inpatch >> p) & 1u) *reinterpret_cast<f32x4*>(Ts + (p * RPP + lrow) * 4) = v;
            }
        }
    }
    // the tile being finished keeps its coordinates; the staging state moves on to the next tile, whose first patch loads
    // fly under the exchange and the output transform below
    const int cy0 = y0, cx0 = x0, cbfr = bfr, cn0 = n0;
    const int nbid = bid + (int)gridDim.x;
    const bool have_next = nbid < ntiles;
    constexpr bool EARLY = BN <= 64;                               // (the 128-wide tile has no registers to carry the loads through its epilogue: 128 accumulators)
    if (EARLY && have_next) { decode(nbid); load_patch(0); }
#pragma unroll
    for (int p = 0; p < NPASS; ++p) {
        if (p > 0) __syncthreads();
        if constexpr (MF16) {
#pragma unroll
            for (int e = 0; e < 2; ++e)
#pragma unroll
                for (int i = 0; i < 2; ++i)
#pragma unroll
                    for (int j = 0; j < NTL; ++j)
#pragma unroll
                        for (int r = 0; r < 4; ++r)                                    // D[row = 4 (lane >> 4) + r][col = lane & 15]
                            Ms[((2 * wv + e) * 32 + 16 * i + 4 * (lane >> 4) + r) * M_LD + j * 16 + (lane & 15)] = acc16[e][i][j][r];
        } else {
#pragma unroll
            for (int e = 0; e < 2; ++e)
#pragma unroll
                for (int jj = 0; jj < 2; ++jj) {
                    const int j = 2 * p + jj;
                    if (j < NTL) {
#pragma unroll
                        for (int r = 0; r < 16; ++r) {
                            const int trow = (r & 3) + 8 * (r >> 2) + 4 * lh;          // tile index (D row)
                            Ms[((2 * wv + e) * 32 + trow) * M_LD + jj * 32 + li] = acc[e][j][r];
                        }
                    }
                }
        }
        __syncthreads();
        const int nch = cn0 + p * 64 + 4 * cq;                       // first of this thread's 4 output channels
        if (4 * cq < (MF16 ? 48 : (NTL - 2 * p >= 2 ? 64 : 32))) {
            f32x4 m[16];
#pragma unroll
            for (int xi = 0; xi < 16; ++xi) m[xi] = *reinterpret_cast<const f32x4*>(Ms + (xi * 32 + tau) * M_LD + 4 * cq);
            f32x4 s[8];                                             // A^T M: rows {0,1} x columns 0..3
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                s[0 * 4 + c] = m[0 * 4 + c] + m[1 * 4 + c] + m[2 * 4 + c];
                s[1 * 4 + c] = m[1 * 4 + c] - m[2 * 4 + c] - m[3 * 4 + c];
            }
            // planar tail: its 9 x n_tail products per output, directly (see the kernel's header comment)
            [[maybe_unused]] f32x4 tacc[4];
            if constexpr (TAIL) {
#pragma unroll
                for (int o = 0; o < 4; ++o) tacc[o] = f32x4{0.f, 0.f, 0.f, 0.f};
                const f32x4* const wt = Wt + (p * 64 + 4 * cq);                          // + tap * BN + k: this thread's channels
                if (a.n_tail == 1) {                                                     // the decoder's conv3 / conv2: one depth plane
                    float tvx[16];                                                       // the tile's 4x4 window of the plane
#pragma unroll
                    for (int r = 0; r < 4; ++r)
#pragma unroll
                        for (int c = 0; c < 4; ++c) tvx[4 * r + c] = Ts[((2 * ty + r) * PW + 2 * tx + c) * 4];
#pragma unroll
                    for (int tap = 0; tap < 9; ++tap) {
                        float wk[4];
#pragma unroll
                        for (int k = 0; k < 4; ++k) wk[k] = wt[tap * BN + k].x;
#pragma unroll
                        for (int o = 0; o < 4; ++o)
#pragma unroll
                            for (int k = 0; k < 4; ++k)
                                tacc[o][k] = fmaf(wk[k], tvx[4 * ((o >> 1) + tap / 3) + (o & 1) + tap % 3], tacc[o][k]);
                    }
                } else {
#pragma unroll 3
                    for (int tap = 0; tap < 9; ++tap) {                                 // (not fully unrolled: 36 weight registers would spill)
                        f32x4 wk[4];
#pragma unroll
                        for (int k = 0; k < 4; ++k) wk[k] = wt[tap * BN + k];
#pragma unroll
                        for (int o = 0; o < 4; ++o) {
                            const f32x4 tv = *reinterpret_cast<const f32x4*>(Ts + ((2 * ty + (o >> 1) + tap / 3) * PW + 2 * tx + (o & 1) + tap % 3) * 4);
#pragma unroll
                            for (int k = 0; k < 4; ++k) {
                                float sacc = tacc[o][k];
                                sacc = fmaf(wk[k].x, tv.x, sacc);
                                sacc = fmaf(wk[k].y, tv.y, sacc);
                                if (a.n_tail > 2) sacc = fmaf(wk[k].z, tv.z, sacc);
                                if (a.n_tail > 3) sacc = fmaf(wk[k].w, tv.w, sacc);
                                tacc[o][k] = sacc;
                            }
                        }
                    }
                }
            }
            if (EARLY && p == 0 && have_next) {                              // the next tile's loads land HERE, in front of every store of this tile
#pragma unroll                                                      // (vmcnt completes in issue order: a wait behind the stores would wait for them too)
                for (int q = 0; q < PA; ++q) asm volatile("" : "+v"(pin[q]));
                asm volatile("" : "+v"(ps4), "+v"(pb4));
            }
            f32x4 e1s = {1.f, 1.f, 1.f, 1.f}, e1b = {0.f, 0.f, 0.f, 0.f}, e2s = e1s, e2b = e1b;
            const bool cin_range = nch + 3 < a.c_out_pad;
            if (has_e1 && cin_range) { e1s = *reinterpret_cast<const f32x4*>(a.e1_scale + nch); e1b = *reinterpret_cast<const f32x4*>(a.e1_shift + nch); }
            if (has_e2 && cin_range) { e2s = *reinterpret_cast<const f32x4*>(a.e2_scale + nch); e2b = *reinterpret_cast<const f32x4*>(a.e2_shift + nch); }
#pragma unroll
            for (int oy = 0; oy < 2; ++oy)
#pragma unroll
                for (int ox = 0; ox < 2; ++ox) {
                    f32x4 v = ox == 0 ? s[oy * 4 + 0] + s[oy * 4 + 1] + s[oy * 4 + 2] : s[oy * 4 + 1] - s[oy * 4 + 2] - s[oy * 4 + 3];
                    if constexpr (TAIL) v += tacc[2 * oy + ox];
                    const int y = cy0 + 2 * ty + oy, x = cx0 + 2 * tx + ox;
                    if (y < a.H && x < a.W) {
                        const long pix = ((long)cbfr * a.H + y) * a.W + x;
                        float o[4];
#pragma unroll
                        for (int k = 0; k < 4; ++k) {
                            float t = v[k] * e1s[k] + e1b[k];
                            if (a.res != nullptr && nch + k < a.c_out) t += a.res[pix * a.res_pix_stride + nch + k];
                            t = apply_act(t, a.act);
                            o[k] = t * e2s[k] + e2b[k];
                        }
                        float* yp = a.y + pix * a.y_pix_stride + nch;
                        if (nch + 3 < a.c_out && ((a.y_pix_stride & 3) == 0) && ((reinterpret_cast<uintptr_t>(yp) & 15) == 0)) {
                            *reinterpret_cast<f32x4*>(yp) = f32x4{o[0], o[1], o[2], o[3]};
                        } else {
#pragma unroll
                            for (int k = 0; k < 4; ++k) if (nch + k < a.c_out) yp[k] = o[k];
                        }
                        if (a.y2) {
                            float* y2p = a.y2 + pix * a.y2_pix_stride + nch;
#pragma unroll
                            for (int k = 0; k < 4; ++k) if (nch + k < a.c_out) y2p[k] = o[k];
                        }
                    }
                }
        }
    }
    if (!have_next) break;
    if (!EARLY) { decode(nbid); load_patch(0); }
    __syncthreads();                                               // everybody is done with M and the tail patch: the next tile's patch / V may land
    bid = nbid;
  }
}

// stride-1 3x3, padding 1, dilation 1, whole 32-channel chunks, NHWC output, pre-transformed weights supplied, and a map
// whose 8x16-pixel workgroup tiles are mostly real pixels (fill >= 0.70)
inline bool wino_eligible(const ConvArgs& a, bool nchw) {
    if (a.w_wino == nullptr || nchw || a.subpix || a.bundled || a.ups != 0) return false;
    const int c_main = a.n_tail > 0 ? a.c_in_ld - 4 : a.c_in_ld;
    if (a.ksize != 3 || a.stride != 1 || a.dil != 1 || a.pad != 1 || c_main <= 0 || (c_main % BK) != 0) return false;
    if (((uintptr_t)a.w_wino & 15)) return false;
    const long ntx = (a.W + 15) / 16, nty = (a.H + 7) / 8;
    // break-even against the direct kernels is a tile-grid fill of ~0.65 (Winograd runs 1.5-1.7x their rate on the pixels it
    // computes); 0.70 keeps a margin.  The NYU decoder's 52x68 maps (0.79) are in, 26x34 (0.58) and 11x38 (0.54) stay out.
    constexpr double min_fill = 0.70;
    return (double)a.H * a.W / (double)(ntx * 16 * nty * 8) >= min_fill;
}

template <int BN, bool TAIL = false>
int launch_wino(const ConvArgs& a0, const ConvRun& r) {
    ConvArgs a = a0;
    const long n_mtiles = (long)a.B * ((a.H + 7) / 8) * ((a.W + 15) / 16);
    a.n_ntiles = (a.c_out + BN - 1) / BN;
    a.tiles_per_class = (int)(n_mtiles * a.n_ntiles);
    a.ksplit = 1;
    const long nwg = n_mtiles * a.n_ntiles;
    constexpr size_t lds = (size_t)wino_lds_bytes<BN, TAIL>();
    static_assert(lds <= 160 * 1024, "LDS");
    // persistent grid: R = tiles per workgroup when 256 CUs share them; every workgroup gets R tiles (some R - 1), and a launch
    // that cannot fill the chip leaves whole CUs to the other streams instead of a ragged last round
    const long R = (nwg + 255) / 256;
    long G = ((nwg + R - 1) / R + 7) & ~7L;                        // multiple of 8: a workgroup's tiles stay on its XCD's slice of the swizzle
    if (G > nwg) G = nwg;
    return conv_launch<conv_wino_kernel<BN, TAIL>>(r, ConvChoice{BTS_CONV_KIND_WINO, 128, BN, 1}, BTS_ERR_INVALID, nwg, G, 512, lds, a);
}
