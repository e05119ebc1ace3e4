// conv1 of the decoder (pytorch/bts.py:287-288) as a fused Winograd F(2x2,3x3) kernel on the fp32-input MFMA: 32 NHWC
// feature channels in Winograd form plus up to four dense depth planes in DIRECT form, 32 output channels, activation,
// NCHW result (included by conv_mfma.hip inside its anonymous namespace, after conv_wino.inc whose V row swizzle it shares).
//
//   y[b][n][Y][X] = act( sum_{tap, c<32} x[b][Y+dy][X+dx][c] w[n][c][tap] + sum_{tap, j<n_tail} plane_j[b][Y+dy][X+dx] w_tail[n][tap][j] )
//
// Main term, per 2x2 output block ("window", 4x4 input pixels d):  Y = A^T [ sum_c U_c .* (B^T d_c B) ] A, U = G g G^T made
// offline (ops.pack_conv_tail_wino): 16 products per window, channel pair instead of the direct form's 36.
//
//   * MFMA roles are SWAPPED relative to conv_wino_kernel: v_mfma_f32_16x16x4_f32 with A = U (rows = 16 output channels)
//     and B = V (columns = 16 windows).  D then puts window l & 15 and channels 4 (l >> 4) + r on lane l, for every
//     transform position xi: a lane holds all 16 xi of its own (window, channel) elements, the output transform A^T M A
//     runs in registers (64 accumulator registers per wave), and for a fixed channel the 16 lanes of a group hold 16
//     x-consecutive windows -- a store writes 128 contiguous bytes of one NCHW row.
//   * A workgroup (4 waves) owns 2 x 16 windows (4 x 32 output pixels, a 6 x 34 input patch) x 32 channels; wave
//     (wb, cb) runs window row wb and channels 16 cb .. 16 cb + 15: 16 xi x 8 k-steps = 128 MFMAs.
//   * conv1 is ONE 32-channel chunk, so there is no K loop to hide a staging pass under: every thread loads one 4x4
//     window x 4 channels straight from global memory (16 x 16 B, clamped addresses; consecutive lanes read the eight
//     channel quads of a pixel, so a load touches whole 128-byte lines and the 4x window overlap is L1 traffic), zeroes
//     the padding, applies B^T d B and writes V[16 xi][32 windows][32 channels] (64 KB, single-buffered).  64 KB of LDS
//     and <= 256 registers: TWO workgroups share a CU and cover each other's loads, transform and stores.
//   * U (64 KB in all, 32 KB per wave) comes straight from global memory / L2 in fragment order through a register ring
//     two steps (32 MFMAs) ahead; one step = 4 xi x 4 k-steps = 16 MFMAs on four independent accumulators, so a dependent
//     MFMA is always three issues behind its predecessor.  A scheduling fence per step keeps the loads where they are
//     written (conv_up9.inc records why).
//   * Tail on the matrix pipe, in DIRECT form: the four plane slots are exactly one k-step.  Lane l holds the 4x4 window
//     of plane l >> 4 at window l & 15 (16 dword loads, zero outside the image and for absent planes); for each of the
//     four output positions of a window and each tap one MFMA takes the window element shifted by that tap as B and the
//     tap's weights as A: 36 MFMAs into four accumulators with the same D layout, added after the output transform.  A
//     non-finite plane value therefore reaches exactly the outputs whose nine taps touch it, as in the direct kernels.
//
// Measured and not kept (B = 16, 352x1216, stand-alone launches, this kernel 1.02-1.03 ms; DESIGN 6): persistent workgroups
// (512, the next tile's windows and planes loaded under the current tile's MFMAs, 251-253 VGPRs) 1.08-1.10 ms; a U ring
// four or eight steps ahead (185 / 245 VGPRs) 1.07-1.08 ms; the plane loads issued first or masked behind the main term
// 1.03-1.04 ms.  By ablation the launch loses 0.05 ms to the U loads, 0.05 to the x loads, 0.08 to the stores and 0.18 to
// the tail, additively: no single wait is the limit.
//
// Numerics: exact-f32 products; V adds up to four inputs, the output transform up to nine products sums: a few ulp of
// the largest partial sum away from the direct kernel.  A non-finite x value spreads over its 4x4 window (as in
// conv_wino_kernel).  Summation order is fixed: a frame's bits depend neither on B nor on any launch declaration.
constexpr int WT_WY = 2, WT_WX = 16;        // windows per workgroup (rows, columns)

struct WinoTailArgs {
    const float* x; long x_pix_stride; int B, H, W;
    const float* u;                           // [16 xi][2 cb][2 halves][64 lanes][4]   (ops.pack_conv_tail_wino)
    const float* w_tail;                      // [2 cb][9 taps][64 lanes]
    const float* tail[4]; int n_tail;         // dense [B,H,W] planes; slots >= n_tail hold any readable address
    int act;
    float* y;                                 // NCHW [B,32,H,W]
    int n_ty, n_tx, ntiles;                   // workgroup tiles per frame (rows, columns), all tiles
};

template <int ACT>
__device__ __forceinline__ void wino_tail_epilogue(const WinoTailArgs& a, const f32x4 (&acc)[16], const f32x4 (&tacc)[4], int bfr,
                                                   int Y0, int X, int n) {
    const long plane = (long)a.H * a.W;
    float* const ybase = a.y + ((long)bfr * 32 + n) * plane + (long)Y0 * a.W + X;
    const bool even = (a.W & 1) == 0;                                   // X is even: both columns inside or both outside
    const bool ok0 = X < a.W, ok1 = X + 1 < a.W;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        float s[4][2];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            s[q][0] = (acc[4 * q + 0][r] + acc[4 * q + 1][r]) + acc[4 * q + 2][r];
            s[q][1] = (acc[4 * q + 1][r] - acc[4 * q + 2][r]) - acc[4 * q + 3][r];
        }
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            if (Y0 + i >= a.H) continue;                                // wave-uniform
            float v[2];
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const float m = i == 0 ? (s[0][j] + s[1][j]) + s[2][j] : (s[1][j] - s[2][j]) - s[3][j];
                v[j] = act_fn<ACT>(m + tacc[2 * i + j][r]);
            }
            float* const p = ybase + r * plane + (long)i * a.W;
            if (even) {
                typedef float f32x2 __attribute__((ext_vector_type(2)));
                if (ok0) *reinterpret_cast<f32x2*>(p) = f32x2{v[0], v[1]};
            } else {
                if (ok0) p[0] = v[0];
                if (ok1) p[1] = v[1];
            }
        }
    }
}

template <int BN>
__global__ __launch_bounds__(256, 2) void conv_wino_tail_kernel(const WinoTailArgs a) {
    static_assert(BN == 32, "32 main channels -> 32 output channels");
    __shared__ __attribute__((aligned(16))) char Vs[16 * 4096];   // [16 xi][32 windows][128 B], wino_v_off swizzle

    const int tid = threadIdx.x;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
    const int wb = wv & 1, cb = wv >> 1;                          // window row / 16-channel block of this wave
    const int lw = lane & 15, lg = lane >> 4;
    // tile decode (XCD-aware bijective swizzle, as conv_up9_kernel: vertically adjacent tiles share an XCD's L2)
    const int bid = blockIdx.x, ntiles = a.ntiles;
    const int swz = xcd_swizzle(bid, ntiles);
    const int bfr = swz / (a.n_tx * a.n_ty);
    const int trem = swz - bfr * (a.n_tx * a.n_ty);
    const int tyi = trem / a.n_tx;
    const int y0 = tyi * 2 * WT_WY, x0 = (trem - tyi * a.n_tx) * 2 * WT_WX;   // first output pixel of the tile
    const unsigned fbase = (unsigned)bfr * (unsigned)(a.H * a.W);

    // ---- weights: the first two steps of this wave's U fragments and its nine tail fragments, before anything else
    const f32x4* const ubase = reinterpret_cast<const f32x4*>(a.u) + cb * 128 + lane;
    auto ufrag = [&](int xi, int half) -> f32x4 { return ubase[xi * 256 + half * 64]; };
    constexpr int NSTEP = 8, RING = 3;                            // step s = (xi group s >> 1, channel half s & 1): 16 MFMAs
    f32x4 ub[RING][4];
#pragma unroll
    for (int s = 0; s < RING - 1; ++s)
#pragma unroll
        for (int e = 0; e < 4; ++e) ub[s][e] = ufrag(4 * (s >> 1) + e, s & 1);
    float wt[9];
#pragma unroll
    for (int t = 0; t < 9; ++t) wt[t] = a.w_tail[(cb * 9 + t) * 64 + lane];

    // ---- input transform: thread = (window tau, channel quad cq); 16 clamped loads, zero padding, B^T d B, V
    {
        const int cq = tid & 7, tau = tid >> 3;
        const int gy0 = y0 + 2 * (tau >> 4) - 1, gx0 = x0 + 2 * (tau & 15) - 1;
        unsigned roff[4], coff[4], okm = 0;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int gy = gy0 + r, gx = gx0 + r;
            roff[r] = fbase + (unsigned)(min(max(gy, 0), a.H - 1) * a.W);
            coff[r] = (unsigned)min(max(gx, 0), a.W - 1);
            okm |= ((unsigned)gy < (unsigned)a.H ? 1u : 0u) << r;
            okm |= ((unsigned)gx < (unsigned)a.W ? 1u : 0u) << (4 + r);
        }
        f32x4 d[16];
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int c = 0; c < 4; ++c)
                d[4 * r + c] = *reinterpret_cast<const f32x4*>(a.x + ((roff[r] + coff[c]) * (unsigned)a.x_pix_stride + (unsigned)(4 * cq)));
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const bool ok = ((okm >> r) & (okm >> (4 + c)) & 1u) != 0;
                f32x4 v = d[4 * r + c];
                v.x = ok ? v.x : 0.f; v.y = ok ? v.y : 0.f; v.z = ok ? v.z : 0.f; v.w = ok ? v.w : 0.f;
                d[4 * r + c] = v;
            }
        f32x4 t[16];
#pragma unroll
        for (int c = 0; c < 4; ++c) {                              // B^T d  (over rows)
            t[0 * 4 + c] = d[0 * 4 + c] - d[2 * 4 + c];
            t[1 * 4 + c] = d[1 * 4 + c] + d[2 * 4 + c];
            t[2 * 4 + c] = d[2 * 4 + c] - d[1 * 4 + c];
            t[3 * 4 + c] = d[1 * 4 + c] - d[3 * 4 + c];
        }
        char* const vw = Vs + wino_v_off(tau, cq);
#pragma unroll
        for (int r = 0; r < 4; ++r) {                              // (B^T d) B  (over columns)
            *reinterpret_cast<f32x4*>(vw + (4 * r + 0) * 4096) = t[r * 4 + 0] - t[r * 4 + 2];
            *reinterpret_cast<f32x4*>(vw + (4 * r + 1) * 4096) = t[r * 4 + 1] + t[r * 4 + 2];
            *reinterpret_cast<f32x4*>(vw + (4 * r + 2) * 4096) = t[r * 4 + 2] - t[r * 4 + 1];
            *reinterpret_cast<f32x4*>(vw + (4 * r + 3) * 4096) = t[r * 4 + 1] - t[r * 4 + 3];
        }
    }

    // ---- tail: this lane's 4x4 window of plane lg at window (wb, lw); the loads land under the main term's MFMAs
    float pw[16];
    {
        const float* const tp = lg == 0 ? a.tail[0] : lg == 1 ? a.tail[1] : lg == 2 ? a.tail[2] : a.tail[3];
        const bool present = lg < a.n_tail;
        const int gy0 = y0 + 2 * wb - 1, gx0 = x0 + 2 * lw - 1;
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const int gy = gy0 + r, gx = gx0 + c;
                const bool ok = present && (unsigned)gy < (unsigned)a.H && (unsigned)gx < (unsigned)a.W;
                const float v = tp[fbase + (unsigned)(min(max(gy, 0), a.H - 1) * a.W + min(max(gx, 0), a.W - 1))];
                pw[4 * r + c] = ok ? v : 0.f;
            }
    }
    __syncthreads();                                               // V complete

    // ---- main term: 8 steps x 16 MFMAs
    f32x4 acc[16];
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[e] = f32x4{0.f, 0.f, 0.f, 0.f};
    int b_off[2];
#pragma unroll
    for (int hf = 0; hf < 2; ++hf) b_off[hf] = wino_v_off(16 * wb + lw, 4 * hf + lg);
    f32x4 fb[2][4];
#pragma unroll
    for (int e = 0; e < 4; ++e) fb[0][e] = *reinterpret_cast<const f32x4*>(Vs + e * 4096 + b_off[0]);
#pragma unroll
    for (int s = 0; s < NSTEP; ++s) {
        const int ns = s + RING - 1;
        if (ns < NSTEP) {
#pragma unroll
            for (int e = 0; e < 4; ++e) ub[ns % RING][e] = ufrag(4 * (ns >> 1) + e, ns & 1);
        }
        if (s + 1 < NSTEP) {
#pragma unroll
            for (int e = 0; e < 4; ++e)
                fb[(s + 1) & 1][e] = *reinterpret_cast<const f32x4*>(Vs + (4 * ((s + 1) >> 1) + e) * 4096 + b_off[(s + 1) & 1]);
        }
#pragma unroll
        for (int q = 0; q < 4; ++q)
#pragma unroll
            for (int e = 0; e < 4; ++e)
                acc[4 * (s >> 1) + e] = __builtin_amdgcn_mfma_f32_16x16x4f32(ub[s % RING][e][q], fb[s & 1][e][q], acc[4 * (s >> 1) + e], 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);
    }

    // ---- tail term, direct form: output position (i, j) of the window, tap (dy, dx) -> window element (i + dy, j + dx)
    f32x4 tacc[4];
#pragma unroll
    for (int p = 0; p < 4; ++p) tacc[p] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int t = 0; t < 9; ++t)
#pragma unroll
        for (int p = 0; p < 4; ++p)
            tacc[p] = __builtin_amdgcn_mfma_f32_16x16x4f32(wt[t], pw[4 * ((p >> 1) + t / 3) + (p & 1) + t % 3], tacc[p], 0, 0, 0);

    // ---- output transform + activation + NCHW stores, in registers
    const int Y0 = y0 + 2 * wb, X = x0 + 2 * lw, n = 16 * cb + 4 * lg;
    dispatch_act(a.act, [&](auto act) { wino_tail_epilogue<decltype(act)::value>(a, acc, tacc, bfr, Y0, X, n); });
}

// Host: workgroup tiles of one frame and the share of their pixels that are real (the tile-grid fill)
inline void wino_tail_grid(int H, int W, int* n_ty, int* n_tx, double* fill) {
    *n_ty = (H + 2 * WT_WY - 1) / (2 * WT_WY); *n_tx = (W + 2 * WT_WX - 1) / (2 * WT_WX);
    *fill = (double)H * W / ((double)*n_ty * 2 * WT_WY * *n_tx * 2 * WT_WX);
}

// The layers the decoder hands to this kernel (bts_conv_tail_wino_plan): fp32 arithmetic, 32 main channels -> 32 output
// channels (bts_size 512's conv1), at most four planes, a tile grid that is mostly real pixels and a DECLARED launch
// (fill_frames x tiles, never B) of at least 2048 workgroups -- conv_up9_kernel's thresholds.
inline bool wino_tail_eligible(int H, int W, int c_main, int c_out, int n_tail, int precision, int fill_frames, long* wgs_per_frame) {
    *wgs_per_frame = 0;
    if (H <= 0 || W <= 0 || c_main != 32 || c_out != 32 || n_tail < 0 || n_tail > 4 || precision != 0) return false;
    int n_ty, n_tx; double fill;
    wino_tail_grid(H, W, &n_ty, &n_tx, &fill);
    *wgs_per_frame = (long)n_ty * n_tx;
    return fill >= kUp9MinFill && (long)fill_frames * *wgs_per_frame >= kUp9MinWgs;
}
