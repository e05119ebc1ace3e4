// Sub-pixel upconv (nearest-2x + 3x3, pytorch/bts.py:83-94) as a shared-patch F(2x2,2x2) kernel on the fp32-input MFMA:
// 9 products per source pixel, input and output channel instead of the sub-pixel halo kernel's 16 (included by
// conv_mfma.hip inside its anonymous namespace, after conv_wino.inc whose V image layout it shares).
//
// ops.pack_upconv_subpixel states the operation as four 2x2 convolutions on the SOURCE map, one per output parity class
// (py, px), with pre-summed filters g_(py,px).  F(2,2) computes two outputs of a 2-tap filter from three inputs with
// three products (m1 = (d0 - d1) g0, m2 = d1 (g0 + g1), m3 = (d2 - d1) g1; y0 = m1 + m2, y1 = m2 + m3).  In 2-D, with
// one 3x3 source window d per "window" (source rows r0..r0+2, columns c0..c0+2, r0 = 2 wy - 1, c0 = 2 wx - 1):
//
//   V = B^T d B,  B^T = [[1,-1,0],[0,1,0],[0,-1,1]]                                (12 subtractions, ONCE per window)
//   U_(py,px) = G g_(py,px) G^T,  G = [[1,0],[1,1],[0,1]]                          (offline: ops.pack_upconv_up9)
//   Y_(py,px) = A^T [ sum_c U_(py,px) .* V ] A,  A^T = [[1,1,0],[0,1,1]]
//
// All four classes share the window and therefore V: class (py, px) yields the outputs at source positions
// (2 wy - py + i, 2 wx - px + j), i, j in {0,1}, i.e. output pixels (2 sy + py, 2 sx + px); together the four classes
// write the contiguous 4x4 output block at rows 4 wy - 1 .. 4 wy + 2.  Windows wy = 0 .. H / 2 cover every output pixel
// exactly once.  So: 9 transform positions xi, one input transform per window, and a GEMM whose N is 4 * c_out.
//
//   * A workgroup (4 waves) owns 4 x 8 windows (8 x 16 source pixels, a 9 x 17-pixel patch) x 32 output channels x the
//     4 classes: wave w IS class w and runs all nine xi on its own 32 columns, so no two waves share a weight fragment
//     and -- unlike conv_wino_kernel -- a lane ends up holding all nine xi of its (window, channel) elements: the output
//     transform is done IN REGISTERS, the accumulators never pass through LDS.
//   * Per 32-channel chunk the patch is staged into LDS once (zero padding applied there; there is no prologue), every
//     thread transforms two (window, channel pair) items into V[9][32 windows][32 channels] (conv_wino.inc's swizzled
//     128-byte rows), then each wave runs 9 x 16 MFMAs with U fragments loaded straight from global memory
//     (fragment-ordered, a six-slot ring five groups ahead).
//   * V is SINGLE-buffered: 36 KB + 22 KB patch = 58 KB of LDS and <= 256 registers, so TWO workgroups share a CU and
//     one's staging, transform and epilogue run under the other's MFMAs (two waves per SIMD, one of each workgroup).
//   * Epilogue: Y = A^T M A per accumulator register (10 additions), activation, optional e2 affine, NHWC stores into a
//     channel slice (y_pix_stride >= c_out): a store instruction writes two pixels x 32 channels (2 x 128 B).
//
// Numerics: exact-f32 MFMA products; U sums up to nine weights, V up to four inputs, so the result differs from the
// sub-pixel halo kernel's by a few ulp of the largest partial sum.  Non-finite inputs: V's differences turn an inf into
// NaN over its whole window, as in conv_wino_kernel's main channels -- the upconv inputs are ELU / BN outputs.
constexpr int UP9_PLD = 36;                 // floats per patch pixel (32 channels + 4 pad)
constexpr int UP9_PW = 17, UP9_PH = 9;      // patch of the 4 x 8-window workgroup tile
constexpr int UP9_PPIX = UP9_PW * UP9_PH;   // 153
constexpr int UP9_WY = 4, UP9_WX = 8;       // windows per workgroup

typedef float up9_acc_t __attribute__((ext_vector_type(16)));

struct Up9Args {
    const float* x; long x_pix_stride; int B, H, W, c_in;       // source map (NHWC), H x W source pixels
    const float* u; int c_out;                                   // U in fragment order (ops.pack_upconv_up9)
    const float* e2_scale; const float* e2_shift; int act;
    float* y; long y_pix_stride;                                 // NHWC [B, 2H, 2W], pixel stride >= c_out
    int n_ntiles, n_ty, n_tx, ntiles;                            // c_out / 32, workgroup tiles per frame (rows, columns), all tiles
};

// Output transform and stores of one wave (class (py, px), 32 windows x 32 channels).  Accumulator register r holds window
// row r >> 2 of the tile and window column (r & 3) + 4 lh: the output row and its validity are wave-uniform, so a store's
// address is a uniform 64-bit row base plus ONE per-lane 32-bit offset computed once (as store_tiles_nhwc does), and the
// column validity of the eight (r & 3, j) slots is a per-lane bit mask computed once.
template <int ACT>
__device__ __forceinline__ void up9_epilogue(const Up9Args& a, const up9_acc_t (&accv)[9], int py, int px, int bfr, int wy0, int wx0,
                                             int n, int lh) {
    const float s2 = a.e2_scale ? a.e2_scale[n] : 1.f, b2 = a.e2_scale ? a.e2_shift[n] : 0.f;
    const int wxl = wx0 + 4 * lh;                                             // window column of this lane's r & 3 == 0 registers
    const unsigned lane_off = (unsigned)(4 * wxl) * (unsigned)a.y_pix_stride + (unsigned)n;
    unsigned xok = 0;                                                         // bit 2 (r & 3) + j: source column 2 (wxl + (r & 3)) - px + j is inside
#pragma unroll
    for (int c = 0; c < 8; ++c) xok |= ((unsigned)(2 * (wxl + (c >> 1)) - px + (c & 1)) < (unsigned)a.W ? 1u : 0u) << c;
    const long frame = (long)bfr * (2 * a.H);
#pragma unroll
    for (int rq = 0; rq < 4; ++rq) {
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int sy = 2 * (wy0 + rq) - py + i;                           // wave-uniform source row
            if ((unsigned)sy >= (unsigned)a.H) continue;
            // output pixel (2 sy + py, 4 (wxl + (r & 3)) - px + 2 j): the uniform part of its address, without the lane's 4 wxl columns
            float* const yrow = a.y + ((frame + 2 * sy + py) * (2 * a.W) - px) * a.y_pix_stride;
#pragma unroll
            for (int rl = 0; rl < 4; ++rl) {
                const int r = 4 * rq + rl;
                float s[3];
#pragma unroll
                for (int b = 0; b < 3; ++b) s[b] = accv[3 * i + b][r] + accv[3 * i + 3 + b][r];
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    float v = s[j] + s[j + 1];
                    v = act_fn<ACT>(v);
                    v = fmaf(v, s2, b2);
                    if ((xok >> (2 * rl + j)) & 1u) (yrow + (long)(4 * rl + 2 * j) * a.y_pix_stride)[lane_off] = v;
                }
            }
        }
    }
}

template <int BN>
__global__ __launch_bounds__(256, 2) void conv_up9_kernel(const Up9Args a) {
    static_assert(BN == 32, "one 32-channel tile x 4 classes per workgroup");
    constexpr int RPP = 32, PA = (UP9_PPIX + RPP - 1) / RPP;      // patch pixels per staging pass, passes (5)
    typedef float f32x2 __attribute__((ext_vector_type(2)));
    __shared__ __attribute__((aligned(16))) char Vs[9 * 4096];    // [9 xi][32 windows][128 B], wino_v_off swizzle
    __shared__ __attribute__((aligned(16))) float Ps[UP9_PPIX * UP9_PLD];

    const int tid = threadIdx.x;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
    const int li = lane & 31, lh = lane >> 5;
    const int nchunks = a.c_in / BK;
    // tile decode (XCD-aware bijective swizzle, as conv_wino_kernel: the channel tiles of one patch stay on one XCD's L2)
    const int bid = blockIdx.x, ntiles = a.ntiles;
    const int swz = xcd_swizzle(bid, ntiles);
    const int mt_idx = swz / a.n_ntiles, nt_idx = swz - mt_idx * a.n_ntiles;
    const int bfr = mt_idx / (a.n_tx * a.n_ty);
    const int trem = mt_idx - bfr * (a.n_tx * a.n_ty);
    const int tyi = trem / a.n_tx;
    const int wy0 = tyi * UP9_WY, wx0 = (trem - tyi * a.n_tx) * UP9_WX;       // first window of the tile
    const int n0 = nt_idx * BN;

    // ---- patch staging: pass p covers patch pixels [32 p, 32 p + 32), thread = (pixel lrow, channels lk..lk+3)
    const int lrow = tid >> 3, lk = (tid & 7) * 4;
    unsigned abase[PA];
    unsigned inimg = 0, inpatch = 0;
#pragma unroll
    for (int p = 0; p < PA; ++p) {
        const int pix = p * RPP + lrow;
        const int pyy = pix / UP9_PW, pxx = pix - pyy * UP9_PW;
        const int gy = 2 * wy0 - 1 + pyy, gx = 2 * wx0 - 1 + pxx;
        const bool inp = pix < UP9_PPIX;
        const bool ok = inp && (unsigned)gy < (unsigned)a.H && (unsigned)gx < (unsigned)a.W;
        const int yc = min(max(gy, 0), a.H - 1), xc = min(max(gx, 0), a.W - 1);
        abase[p] = ((unsigned)bfr * (unsigned)(a.H * a.W) + (unsigned)(yc * a.W + xc)) * (unsigned)a.x_pix_stride + (unsigned)lk;
        inimg |= (ok ? 1u : 0u) << p;
        inpatch |= (inp ? 1u : 0u) << p;
    }
    f32x4 pin[PA];
    auto load_patch = [&](int chunk) {                             // loads only (clamped addresses): nothing touches the values here
        const unsigned cs = (unsigned)(chunk * BK);
#pragma unroll
        for (int p = 0; p < PA; ++p) pin[p] = *reinterpret_cast<const f32x4*>(a.x + (abase[p] + cs));
    };
    auto store_patch = [&]() {                                     // zero padding, to LDS
#pragma unroll
        for (int p = 0; p < PA; ++p) {
            f32x4 v = pin[p];
            const bool ok = (inimg >> p) & 1u;
            v.x = ok ? v.x : 0.f; v.y = ok ? v.y : 0.f; v.z = ok ? v.z : 0.f; v.w = ok ? v.w : 0.f;
            if ((inpatch >> p) & 1u) *reinterpret_cast<f32x4*>(Ps + (p * RPP + lrow) * UP9_PLD + lk) = v;
        }
    };
    // ---- transform items: window tau (0..31) x channel pair cp (0..15), two per thread (tau = tid >> 4 and 16 + tid >> 4)
    const int cp = tid & 15;
    auto transform_store = [&]() {
#pragma unroll
        for (int it = 0; it < 2; ++it) {
            const int tau = 16 * it + (tid >> 4);
            const float* const pwin = Ps + ((2 * (tau >> 3)) * UP9_PW + 2 * (tau & 7)) * UP9_PLD + 2 * cp;
            char* const vw = Vs + wino_v_off(tau, cp >> 1) + (cp & 1) * 8;
            f32x2 d[9];
#pragma unroll
            for (int r = 0; r < 3; ++r)
#pragma unroll
                for (int c = 0; c < 3; ++c) d[3 * r + c] = *reinterpret_cast<const f32x2*>(pwin + (r * UP9_PW + c) * UP9_PLD);
            f32x2 t[9];
#pragma unroll
            for (int c = 0; c < 3; ++c) {                          // B^T d  (over rows)
                t[0 + c] = d[0 + c] - d[3 + c];
                t[3 + c] = d[3 + c];
                t[6 + c] = d[6 + c] - d[3 + c];
            }
#pragma unroll
            for (int r = 0; r < 3; ++r) {                          // (B^T d) B  (over columns)
                *reinterpret_cast<f32x2*>(vw + (3 * r + 0) * 4096) = t[3 * r + 0] - t[3 * r + 1];
                *reinterpret_cast<f32x2*>(vw + (3 * r + 1) * 4096) = t[3 * r + 1];
                *reinterpret_cast<f32x2*>(vw + (3 * r + 2) * 4096) = t[3 * r + 2] - t[3 * r + 1];
            }
        }
    };

    // ---- weights: fragment-ordered U, [9 xi][nchunks][c_out / 32][4 classes][4 groups][64 lanes][4]; this wave's column tile
    //      is (channel tile nt_idx, class wv)
    const int n_ct = a.c_out / 8;                                  // 32-column tiles: 4 classes x c_out / 32
    const f32x4* const ubase = reinterpret_cast<const f32x4*>(a.u) + (size_t)(nt_idx * 4 + wv) * 256 + lane;
    const size_t chunk_stride = (size_t)n_ct * 256, xi_stride = (size_t)nchunks * chunk_stride;
    auto ufrag = [&](int chunk, int grp) -> f32x4 { return ubase[(grp >> 2) * xi_stride + chunk * chunk_stride + (grp & 3) * 64]; };
    int a_off[4];
#pragma unroll
    for (int g = 0; g < 4; ++g) a_off[g] = wino_v_off(li, 2 * g + lh);

    up9_acc_t acc[9];
#pragma unroll
    for (int e = 0; e < 9; ++e)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[e][r] = 0.f;

    constexpr int NGRP = 36, RING = 6, AHEAD = RING - 1;              // (xi, 8-channel group) steps per chunk; fragment ring (36 % RING == 0)
    f32x4 ub[RING];
    load_patch(0);
#pragma unroll
    for (int g = 0; g < AHEAD; ++g) ub[g] = ufrag(0, g);
    store_patch();
    if (nchunks > 1) load_patch(1);
    __syncthreads();
    for (int chunk = 0; chunk < nchunks; ++chunk) {
        transform_store();
        __syncthreads();                                           // V complete, the patch is free
        const bool more = chunk + 1 < nchunks;
        if (more) store_patch();                                   // chunk + 1 (its loads are a chunk old)
        if (chunk + 2 < nchunks) load_patch(chunk + 2);
        // One (xi, 8-channel group) step = 4 MFMAs.  Its weight fragment was loaded AHEAD steps earlier and its A fragment one
        // step earlier; a scheduling fence after every step keeps the loads where they are written (left alone, the compiler
        // sinks each weight load to one step before its use, and a wave then waits out the load latency every 4 MFMAs).
        const int nc = more ? chunk + 1 : chunk;                   // the steps past the end prefetch the next chunk's first ones
        f32x4 fa[2];
        fa[0] = *reinterpret_cast<const f32x4*>(Vs + a_off[0]);
#pragma unroll
        for (int grp = 0; grp < NGRP; ++grp) {
            const int ng = grp + AHEAD;
            ub[ng % RING] = ng < NGRP ? ufrag(chunk, ng) : ufrag(nc, ng - NGRP);
            if (grp + 1 < NGRP) fa[(grp + 1) & 1] = *reinterpret_cast<const f32x4*>(Vs + ((grp + 1) >> 2) * 4096 + a_off[(grp + 1) & 3]);
            const int e = grp >> 2;
#pragma unroll
            for (int q = 0; q < 4; ++q) acc[e] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[grp & 1][q], ub[grp % RING][q], acc[e], 0, 0, 0);
            __builtin_amdgcn_sched_barrier(0);
        }
        __syncthreads();                                           // V free, the patch of chunk + 1 complete
    }
    // ---------------------------------------------------------------- output transform + epilogue, in registers
    const int py = wv >> 1, px = wv & 1, n = n0 + li;
    if (a.act == 2) up9_epilogue<2>(a, acc, py, px, bfr, wy0, wx0, n, lh);
    else if (a.act == 1) up9_epilogue<1>(a, acc, py, px, bfr, wy0, wx0, n, lh);
    else up9_epilogue<0>(a, acc, py, px, bfr, wy0, wx0, n, lh);
}

// Host: workgroup tiles of one frame and the share of their windows that are real (the tile-grid fill)
inline void up9_grid(int H, int W, int* n_ty, int* n_tx, double* fill) {
    const int nwy = H / 2 + 1, nwx = W / 2 + 1;                    // windows wy = 0 .. H / 2
    *n_ty = (nwy + UP9_WY - 1) / UP9_WY; *n_tx = (nwx + UP9_WX - 1) / UP9_WX;
    *fill = (double)nwy * nwx / ((double)*n_ty * UP9_WY * *n_tx * UP9_WX);
}

// The layers the decoder hands to this kernel (bts_upconv_up9_plan): fp32 arithmetic, whole 32-channel chunks both ways,
// a tile grid that is mostly real windows, and a DECLARED launch (fill_frames x tiles, never B) of at least kUp9MinWgs
// workgroups -- four rounds of the chip's 512 resident ones.  The single-frame declarations (fill_frames 1 / 2) stay below
// it on every decoder map, so the batch-1 path keeps the sub-pixel halo kernel and its bits.
constexpr long kUp9MinWgs = 2048;
constexpr double kUp9MinFill = 0.70;
inline bool up9_eligible(int H, int W, int c_in, int c_out, int precision, int fill_frames, long* wgs_per_frame) {
    *wgs_per_frame = 0;
    if (H <= 0 || W <= 0 || c_in <= 0 || c_out <= 0 || (c_in % BK) || (c_out % 32) || precision != 0) return false;
    int n_ty, n_tx; double fill;
    up9_grid(H, W, &n_ty, &n_tx, &fill);
    *wgs_per_frame = (long)n_ty * n_tx * (c_out / 32);
    return fill >= kUp9MinFill && (long)fill_frames * *wgs_per_frame >= kUp9MinWgs;
}
