/*
 * bts_hip.h -- C ABI of libbts_hip.so: the MI355X (gfx950) native BTS decoder hot path.
 *
 * Drop-in boundary for the hot path of minghanz/bts (reference files cited per entry,
 * paths relative to the reference checkout).  Conventions mirror the only native
 * interface the reference has, LocalPlanarGuidanceKernel<Device>::operator()
 * (tensorflow/custom_layer/local_planar_guidance.h:22-49): borrowed `const float*`
 * inputs, caller-allocated outputs, dims as `int`, work enqueued on a caller stream.
 *
 *  - all pointers are DEVICE pointers to fp32 unless stated; the caller owns every buffer;
 *  - `stream` is a hipStream_t passed as void* (NULL = the null stream);
 *  - nothing here allocates, frees or synchronises: calls are hipGraph-capturable;
 *  - return value: 0 = ok, >0 = a hipError_t from the launch, <0 = BTS_ERR_* (bad
 *    arguments); errors are raised by the wrapper, never thrown across the ABI
 *    (cf. OP_REQUIRES / errors::InvalidArgument in local_planar_guidance.cc:36-44,123);
 *  - re-entrant per (device, stream): every entry point works on the calling thread's current device and the given
 *    stream.  The library keeps no mutable state between calls except one idempotent, lock-free cache: "the
 *    dynamic-LDS limit of kernel K has been raised on device D" (a bit per device ordinal; the attribute is per
 *    device, so a process driving several GPUs -- nn.DataParallel, bts_test.py:91 -- gets it set on each).  The
 *    BTS_CONV_* environment knobs (conv_mfma.hip, ConvKnobs) are read once into immutable values.
 */
#ifndef BTS_HIP_H_
#define BTS_HIP_H_

#ifdef __cplusplus
extern "C" {
#endif

#define BTS_HIP_ABI_VERSION 17

#define BTS_ERR_INVALID      (-1)   /* bad argument (null pointer, non-positive dim, misalignment) */
#define BTS_ERR_UNSUPPORTED  (-2)   /* valid in the reference but not built here (e.g. odd upratio)  */

typedef void* bts_stream_t;

int         bts_hip_abi_version(void);
const char* bts_hip_error_string(int code);

/* ------------------------------------------------------------------------------------------
 * Local planar guidance, forward.
 * Replaces local_planar_guidance.forward (pytorch/bts.py:149-173); native statement:
 * LocalPlanarGuidanceKernel<GPUDevice> (tensorflow/custom_layer/local_planar_guidance.cu:33-72).
 *
 *   plane_eq : [B,4,h,w] NCHW planar (n1,n2,n3,n4), as the PyTorch module receives it
 *   depth    : [B,h*k,w*k]
 *   abs_min  : optional 1-float device scalar <- min |n1*u+n2*v+n3| (bts.py:167), may be NULL
 * Bit-exact with the reference on the same inputs: separate mul/add roundings (no FMA),
 * the +-1e-3 clamp of bts.py:168-171 and an IEEE division.  upratio in {1,2,4,8}.
 */
int bts_lpg_fwd_f32(const float* plane_eq, int B, int h, int w, int upratio,
                    float* depth, float* abs_min, bts_stream_t stream);

/* Local planar guidance, backward (training callers).
 * Replaces autograd through local_planar_guidance.forward (pytorch/bts.py:149-173); native statement:
 * LocalPlanarGuidanceGradKernel<GPUDevice> (tensorflow/custom_layer/local_planar_guidance.cu:95-150, same
 * one-thread-per-input-cell mapping and argument order: depth_grad, input -> grad_input).
 *   grad_depth [B,h*k,w*k] -> grad_plane_eq [B,4,h,w].  True derivative of the PyTorch module: includes the n4
 *   factor the TF op drops (cu:143-145) and zeroes d/dn1..n3 where the +-1e-3 clamp is active (bts.py:168-171).
 */
int bts_lpg_bwd_f32(const float* plane_eq, const float* grad_depth, int B, int h, int w, int upratio,
                    float* grad_plane_eq, bts_stream_t stream);

/* Fused LPG + glue, as bts.forward uses it (pytorch/bts.py:250-256, 264-270, 278-283):
 *   plane4   : [B*h*w,4] cell-interleaved (n1,n2,n3,n4) -- what bts_reduc_fwd_f32 emits
 *   normalize: !=0 -> n[0:3] /= max(||n||_2, 1e-12)  (F.normalize, bts.py:251); 0 if already done
 *   depth_scaled : [B,1,h*k,w*k] = lpg(plane)/max_depth                      (bts.py:255)
 *   ds_out   : optional nearest-downsampled copy [::ds_factor, ::ds_factor] (bts.py:256,270),
 *              element (b,y,x) written at ds_out[((b*Hd+y)*Wd+x)*ds_pix_stride]; NULL to skip
 *   abs_min  : optional, as above
 */
int bts_lpg_fused_fwd_f32(const float* plane4, int B, int h, int w, int upratio, int normalize,
                          float max_depth, float* depth_scaled,
                          float* ds_out, int ds_factor, long ds_pix_stride,
                          float* abs_min, bts_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * reduction_1x1 forward: the whole 1x1-conv(+ELU) chain and its epilogue in one kernel.
 * Replaces reduction_1x1.forward (pytorch/bts.py:97-136).
 *
 *   x        : NHWC activations, pixel p channel c at x[p*x_pix_stride + c], c in [0,c_in)
 *   npix     : B*h*w
 *   c_in, c_first_out : the module's (num_in_filters, num_out_filters); the chain halves the
 *              width until it is < 8 exactly as bts.py:105-122 does.  Built chains:
 *              (128,128) (128,64) (64,32) (32,16).
 *   w_frag   : the chain's weights in MFMA fragment order (see bts_amd/ops.py:pack_reduc_weights)
 *   is_final : 0 -> out[p*4 + {0..3}] = (sin t cos f, sin t sin f, cos t, sigmoid(c2)*max_depth)
 *                   with t = sigmoid(c0)*pi/3, f = sigmoid(c1)*2pi (bts.py:127-134); if
 *                   `normalize` the normal is L2-normalised here (bts.py:251) so LPG need not;
 *              1 -> out[p] = sigmoid(c0) (bts.py:108-110)
 */
int bts_reduc_fwd_f32(const float* x, long x_pix_stride, long npix, int c_in, int c_first_out,
                      const float* w_frag, long w_frag_floats, float max_depth, int is_final,
                      int normalize, float* out, bts_stream_t stream);

/* reduction_1x1 (non-final) -> F.normalize -> local_planar_guidance -> /max_depth -> nearest downsample in ONE launch:
 * one scale of pytorch/bts.py:249-256 (8x8), 263-270 (4x4), 277-283 (2x2).  The plane equations go from the chain's
 * registers straight into the k x k depth block of their cell; they reach HBM only if `plane4` is given.
 *   x            : NHWC activations [B*h*w, >= c_in] (pixel stride x_pix_stride)
 *   (c_in, c_first_out, upratio) : (128,128,8), (128,64,4) or (64,32,2) -- the three scales of bts_size 512
 *   plane4       : optional [B*h*w,4] (n1,n2,n3 normalised, n4) for callers that want the plane equation; NULL to skip
 *   depth_scaled : [B,1,h*k,w*k] = lpg(plane)/max_depth                                  (bts.py:255, 269, 283)
 *   ds_out       : optional dense plane [B,2h,2w] = depth_scaled[..., ::k/2, ::k/2]        (bts.py:256, 270: scale_factor
 *                  0.25 at k=8, 0.5 at k=4); must be NULL for k=2
 *   abs_min      : optional 1-float device scalar <- min |den| over the batch, NaN if any denominator is NaN (bts.py:167)
 */
int bts_reduc_lpg_fwd_f32(const float* x, long x_pix_stride, int B, int h, int w, int c_in, int c_first_out,
                          const float* w_frag, long w_frag_floats, float max_depth, int upratio,
                          float* plane4, float* depth_scaled, float* ds_out, float* abs_min, bts_stream_t stream);

/* Backward-data of one reduction_1x1 scale for training callers: the gradient that autograd through
 * pytorch/bts.py:124-136 + F.normalize + local_planar_guidance + /max_depth (bts.py:249-256, 263-270, 277-283) hands to the
 * chain's input, plus the two row buffers from which bts_conv_wgrad_f32 computes every layer's weight gradient.
 *   x, B, h, w   : as bts_reduc_lpg_fwd_f32 (final chain: the map itself, npix = B*h*w)
 *   (c_in, c_first_out, upratio) : (128,128,8), (128,64,4), (64,32,2), or the final chain (32,16) with upratio 0;
 *                  anything else returns BTS_ERR_UNSUPPORTED
 *   w_frag       : the chain's weights in the 32x32x2 fragment order for EVERY chain (ops.pack_reduc_weights(..., wide=True);
 *                  the forward entry points take the narrow chains in the 16x16x4 order instead)
 *   wt_frag      : the transposed weights W_l^T in reverse layer order, the last layer's 3 (1) outputs zero-padded to 8
 *                  columns, in the same fragment order (ops.pack_reduc_weights_bwd)
 *   grad_out     : upratio > 0: gradient of depth_scaled, contiguous [B,1,h*k,w*k]; final: gradient of the sigmoid output [B,1,h,w]
 *   dx           : optional [npix, c_in] rows at dx_pix_stride (a multiple of 4, >= c_in); columns >= c_in are not written
 *   Y            : [npix, YC] packed rows, the hidden layers' post-ELU activations (recomputed), layer l at the columns below
 *   G            : optional [npix, YC + 4] packed rows, the gradient w.r.t. every layer's pre-activation; the last layer's
 *                  3 (1) values sit in the last 4 columns, zero-padded
 *   column tables (layer: first column, width), YC = width of Y:
 *     (128,128): 128->128: 0,128   128->64: 128,64   64->32: 192,32   32->16: 224,16   16->8: 240,8   [G: 8->3: 248,4]   YC 248
 *     (128, 64): 128->64:  0,64    64->32:  64,32    32->16: 96,16    16->8:  112,8    [G: 8->3: 120,4]                   YC 120
 *     ( 64, 32): 64->32:   0,32    32->16:  32,16    16->8:  48,8     [G: 8->3: 56,4]                                     YC 56
 *     ( 32, 16): 32->16:   0,16    16->8:   16,8     [G: 8->1: 24,4]                                                      YC 24
 *   Layer l's weight gradient is bts_conv_wgrad_f32 (ksize 1) with dy = G's columns of layer l and x = Y's columns of
 *   layer l-1 (the chain's input for the first layer).  No atomics: dx, G and Y are bit-reproducible.  All pointers 16-byte aligned.
 */
int bts_reduc_bwd_f32(const float* x, long x_pix_stride, int B, int h, int w, int c_in, int c_first_out,
                      const float* w_frag, long w_frag_floats, const float* wt_frag, long wt_frag_floats,
                      float max_depth, int upratio, const float* grad_out, float* dx, long dx_pix_stride,
                      float* G, float* Y, bts_stream_t stream);

/* The most waves bts_reduc_bwd_f32 launches for a chain (its grid cap x 8 waves; each wave walks 32-pixel tiles in a
 * grid-stride loop), or BTS_ERR_UNSUPPORTED.  Host arithmetic only. */
long bts_reduc_bwd_max_waves(int c_in, int c_first_out, int upratio);

/* ------------------------------------------------------------------------------------------
 * NHWC implicit-GEMM convolution on fp32-input MFMA (v_mfma_f32_32x32x2_f32), with fused
 * per-channel affine/activation prologue and epilogue.  Covers atrous_conv's two convolutions
 * (pytorch/bts.py:65-80: [first_bn]->ReLU->conv1x1->BN->ReLU->conv3x3 dilated) and the other
 * decoder convolutions (upconv bts.py:83-94, conv5..conv1, daspp_conv bts.py:183-221).
 *
 *   y[p, n] = E( sum_{tap,c} P(x[q(p,tap), c]) * w[tap][n][c] )
 *   P(v) = pre_relu( v*pre_scale[c] + pre_shift[c] )         (zero padding applied AFTER P)
 *   E(a) = post2( act( a*e1_scale[n] + e1_shift[n] ) ),  post2(v) = v*e2_scale[n] + e2_shift[n]
 *   q(p,tap): input pixel of output pixel p for the tap, with `stride`, `dil`ation, `pad`ding and an
 *   optional nearest `up`x upsample of the input folded into the index.
 */
typedef struct bts_conv_desc {
    const float* x;        /* input, NHWC: pixel q channel c at x[q*x_pix_stride + c]              */
    long  x_pix_stride;    /* floats between pixels (>= c_in_ld, multiple of 4)                   */
    int   c_in_ld;         /* loadable input channels (multiple of 4; pad channels must be 0)     */
    int   k_pad;           /* padded flattened K of the packed weights: multiple of 32,
                              >= ksize*ksize*c_in_ld; k = tap*c_in_ld + c                          */
    int   B, h_in, w_in;   /* input spatial size before the optional upsample                     */
    int   up;              /* 1 or 2: nearest upsample folded into the gather (bts.py:91)         */
    int   ksize;           /* odd, 1..7                                                            */
    int   dil;             /* dilation (>= 1)                                                      */
    int   stride;          /* output stride (1 or 2; must be 1 when up == 2)                       */
    int   pad;             /* zero padding on each side (reference convs: dil*(ksize/2))           */
    const float* w;        /* packed weights [c_out_pad][k_pad], c_out_pad % 32 == 0               */
    int   c_out;           /* real output channels                                                 */
    int   c_out_pad;
    const float* pre_scale;  /* [c_in_ld] or NULL (identity)                                       */
    const float* pre_shift;  /* [c_in_ld] or NULL                                                  */
    int   pre_relu;
    const float* e1_scale;   /* [c_out_pad] or NULL                                                */
    const float* e1_shift;
    int   act;               /* 0 none, 1 ReLU, 2 ELU, 3 sigmoid                                   */
    const float* e2_scale;   /* [c_out_pad] or NULL                                                */
    const float* e2_shift;
    float* y;                /* output                                                             */
    long  y_pix_stride;      /* NHWC: floats between pixels; ignored for NCHW                      */
    int   y_nchw;            /* 0: y[p*y_pix_stride + n]; 1: y[(b*c_out + n)*H*W + yx] (boundary)  */
    int   subpixel;          /* 1: "sub-pixel upconv" -- nearest-2x upsample + 3x3 conv (bts.py:90-92) computed as four
                                2x2 convolutions on the SOURCE pixels, one per output parity (py,px), 2.25x fewer
                                FLOPs, same result: requires ksize 2, up 1, stride 1, dil 1, NHWC output;
                                w = [4][c_out_pad][k_pad] (class = 2*py+px, taps pre-summed, see
                                bts_amd/ops.py:pack_upconv_subpixel); output is [B, 2*h_in, 2*w_in, c_out]   */
    float* y2;               /* optional second NHWC destination of the same result (a skip tensor
                                that must live in two concat buffers), or NULL                      */
    long  y2_pix_stride;
    float* splitk_ws;        /* optional scratch (caller-owned, exclusive to this stream while the call runs) that
                                lets under-filled launches split K over several workgroups: partial sums go here
                                and a second kernel reduces them in a fixed order (deterministic); NULL = never split */
    long  splitk_ws_floats;  /* its size in floats (8 * M * round_up(c_out,4) is always enough)                     */
    const float* res;        /* optional residual, NHWC [B,H,W,>=c_out]: y = act(e1(conv) + res) -- the bottleneck's
                                `out += identity; relu` of the ResNet/ResNeXt encoders (torchvision Bottleneck.forward,
                                caller side of pytorch/bts.py:327-338); NULL = none; NHWC output only                 */
    long  res_pix_stride;
    int   n_bundles;         /* 0/1: ordinary convolution.  > 1: grouped convolution run as n_bundles independent
                                channel bundles in ONE launch (ResNeXt's 32-group 3x3, groups packed block-diagonally
                                into bundles of >= 32 channels by the host): bundle j reads input channels
                                [j*c_in_ld, (j+1)*c_in_ld) and writes output channels [j*c_out, (j+1)*c_out);
                                w = [n_bundles][c_out_pad][k_pad]; pre_* hold n_bundles*c_in_ld and e1_/e2_*
                                n_bundles*c_out_pad entries; x_pix_stride >= n_bundles*c_in_ld,
                                y_pix_stride >= n_bundles*c_out; no sub-pixel, NCHW output or split-K               */
    int   precision;         /* 0: fp32-input MFMA (v_mfma_f32_32x32x2_f32: exact fp32 products, fp32 accumulation).
                                1: fp32 EMULATED on the bf16 matrix cores -- every operand split into three bf16
                                pieces on the way to LDS, six bf16 MFMAs per product block, fp32 accumulation; the
                                result differs from mode 0 only by fp32 rounding (measured 1.2e-6 vs 1.1e-6 of
                                max|result| against fp64), at up to 2.6x the MFMA rate.  Same inputs, outputs, tiles.
                                2: bf16 OPERANDS (an inference mode): the conv input after the prologue and zero padding,
                                and the packed weights `w`, are rounded to bf16 (round to nearest, ties to even); each
                                product of two bf16 values is exact and accumulates in fp32 (one v_mfma_f32_32x32x16_bf16 per
                                16 k).  The epilogue and the HBM tensors stay fp32; bf16 keeps fp32's exponent range.  The
                                planar-tail layers and the 7x7 encoder stem stay on their fp32 kernels; no Winograd.
                                $BTS_CONV_PRECISION (0 / 1) overrides this field in every mode.                          */
    const float* tail_planes[4];  /* planar tail operand: n_tail (1..4) extra input channels that live in dense one-channel
                                planes [B,h_in,w_in] instead of the NHWC buffer -- the LPG depth maps / reduc1x1 that the
                                reference concatenates behind the features (pytorch/bts.py:260, 274, 287: cat[upconv3, skip,
                                depth_8x8_scaled_ds] ...).  They are channels [c_in_ld-4, c_in_ld-4+n_tail) of the packed K
                                axis (c_in_ld = buffer channels + 4; weights of the unused tail slots are zero), x then
                                only needs c_in_ld-4 channels.  3x3, pad 1, stride 1, dil 1, up 1 only (the decoder's
                                conv3 / conv2 / conv1); computed on the fp32-input MFMA whatever `precision` says.         */
    int   n_tail;              /* 0 = no tail                                                                              */
    int   fill_frames;         /* 0 = default (8, or $BTS_CONV_FILL_FRAMES).  How many frames the caller expects to share one
                                launch: the launch-filling choices (whether and how far an under-filled layer splits K,
                                whether the wide 1x1 tile has enough pixel tiles) are sized for fill_frames x H x W pixels.
                                They are NEVER derived from B itself -- a frame's bits must not depend on its batch -- so a
                                caller that runs single frames (the reference's test loop, pytorch/bts_test.py:127-147) says
                                so here: fill_frames = 1 or 2 splits K on many more layers (352x1216, batch 1: 8.2 -> 5.7 ms of
                                GPU time per frame).  A batched caller declares the frames that share the chip (bench.py: its
                                per-GPU batch, at most 16): from 12-14 frames on, the DenseNet block-3 layers (22x76 maps) move
                                from the split-K kernels to the wide 1x1 tile and the halo kernel -- choices that would cost a
                                single-frame caller 45 % if they were tied to the default.  Results of different fill_frames
                                differ in summation order (fp32 rounding)                                                  */
    const void* w_split;       /* optional, precision = 1 or 2 only.  Precision 1: the packed weights `w` pre-split into three bf16 planes --
                                [classes][3][c_out_pad][k_pad] bf16 (classes = 4 for sub-pixel, else 1), plane 0 = the top 16
                                bits of w, plane 1 = the top 16 bits of (w - plane 0), plane 2 = the top 16 bits of the rest
                                (the kernels' own truncation split; bts_amd/ops.py:split_bf16x3).  With it the halo-tile
                                kernel of the emulated mode streams weight tiles global -> LDS by LDS-DMA; NULL = the
                                row-tiled kernel splits `w` on the fly.  Precision 2: ONE plane [classes][1][c_out_pad][k_pad]
                                bf16 (int16 bits), `w` rounded to nearest even (bts_amd/ops.py:round_bf16); the bf16 halo-tile
                                kernel streams it by LDS-DMA; NULL = the row-tiled kernel rounds `w` on the fly, the same
                                rounding.  The layout follows THIS descriptor's precision: when $BTS_CONV_PRECISION
                                overrides it, w_split is ignored.  16-byte aligned.                                        */
    const float* w_wino;       /* optional, precision = 0, stride-1 3x3 / padding 1 / dilation 1 only: the weights in Winograd
                                F(2x2,3x3) form U = G g G^T, in MFMA B-fragment order [16 xi][c_in_ld/32][c_out_pad/32][4][64][4]
                                (bts_amd/ops.py:pack_wino_weight).  With it (and $BTS_CONV_WINO) eligible layers run the fused
                                Winograd kernel (csrc/conv_wino.inc): 2.25x fewer MFMA products, results equal to the direct
                                kernels' up to fp32 rounding of the transforms.  NULL = direct kernels.  16-byte aligned.   */
} bts_conv_desc;

int bts_conv_fwd_f32(const bts_conv_desc* desc, bts_stream_t stream);

/* Tap-sum stage of an upconv (nearest-2x + 3x3 conv + activation + affine, pytorch/bts.py:90-94 and the bn that follows,
 * :227, 231) computed as a TAP GEMM: first ONE 1x1 convolution of the source map with the nine kernel taps side by side
 * (bts_conv_fwd_f32, c_out = 9*c, weights [t*c + n][c_in] = w[n][c_in][t], no activation) into `taps`, then this call:
 *   y[b][2Y+py][2X+px][n] = e2(act( sum_{ky,kx} taps[b][Y+dy(py,ky)][X+dx(px,kx)][(3*ky+kx)*c + n] )),
 *   dy(0,.) = (-1,0,0), dy(1,.) = (0,0,+1), same for dx; source pixels outside the map contribute 0.
 * 9 tap-products per source pixel instead of the sub-pixel form's 16 (or the reference's 36): what a small, wide map wants
 * (upconv5: 11x38, 2208 -> 512).  taps: [B*h*w] pixels of taps_pix_stride >= 9*c floats; y: NHWC [B,2h,2w] with
 * y_pix_stride >= c; c % 4 == 0; act 0 none / 1 ReLU / 2 ELU; e2_* [c] or both NULL.  Sum order fixed (tap 0..8). */
int bts_upconv_combine_f32(const float* taps, long taps_pix_stride, int B, int h, int w, int c,
                           const float* e2_scale, const float* e2_shift, int act, float* y, long y_pix_stride,
                           bts_stream_t stream);

/* The same upconv (nearest-2x + 3x3 conv + activation + affine) as ONE fused launch in shared-patch F(2x2,2x2) form
 * (csrc/conv_up9.inc): the four parity classes of the sub-pixel statement share one transformed 3x3 source window, so
 * the matrix pipe issues 9 products per source pixel, input and output channel instead of the sub-pixel halo kernel's
 * 16.  Opt-in: bts_conv_fwd_f32 never takes this path on its own.
 *   x: NHWC source map [B,h,w], x_pix_stride >= c_in floats per pixel (a multiple of 4), 16-byte aligned
 *   u: U = G g_(py,px) G^T for the four classes in MFMA B-fragment order, 36 * c_in * c_out floats, 16-byte aligned:
 *      float index ((((((xi * (c_in/32) + chunk) * (c_out/32) + ct) * 4 + cls) * 4 + g) * 64 + lh * 32 + li) * 4 + q
 *      = U_cls[xi][n = 32 ct + li][k = 32 chunk + 8 g + 4 lh + q], cls = 2 py + px, xi = 3 a + b (bts_amd/ops.py:pack_upconv_up9)
 *   y: NHWC [B,2h,2w], y_pix_stride >= c_out; act 0 none / 1 ReLU / 2 ELU; e2_* [c_out] or both NULL
 * c_in % 32 == 0 and c_out % 32 == 0, else BTS_ERR_UNSUPPORTED.  Non-finite inputs spread over their 3x3 window (inf -> NaN). */
int bts_upconv_up9_fwd_f32(const float* x, long x_pix_stride, int B, int h, int w, int c_in, const float* u, int c_out,
                           const float* e2_scale, const float* e2_shift, int act, float* y, long y_pix_stride,
                           bts_stream_t stream);

/* Should a layer take bts_upconv_up9_fwd_f32 (host-side query, no GPU work, no pointers)?  Eligible: precision 0, whole
 * 32-channel chunks both ways, a grid of 4x8-window workgroup tiles that is at least 0.70 real windows, and a declared
 * launch (fill_frames as in bts_conv_desc, 0 = the library default; never B) of at least 2048 workgroups.
 *   *bm = windows per workgroup (32), *bn = output channels per workgroup (32), *workgroups = workgroups PER FRAME;
 *   all three 0 when the layer should stay on bts_conv_fwd_f32's sub-pixel path. */
int bts_upconv_up9_plan(int h, int w, int c_in, int c_out, int precision, int fill_frames, int* bm, int* bn, long* workgroups);

/* A planar-tail 3x3 convolution (stride 1, padding 1: the decoder's conv3 / conv2, whose last input channel is a dense depth
 * plane) with bf16 MAIN operands and an fp32 tail, in one launch (csrc/conv_tail_bf16.inc):
 *   y[b][Y][X][n] = e2(act( sum_{tap, c < c_main} bf16(x[b][Y+dy][X+dx][c]) * w_main[n][tap * c_main + c]
 *                         + sum_{tap} tail_plane[b][Y+dy][X+dx] * w_tail[n][tap][0] )),   tap = 3 (dy+1) + (dx+1)
 * The main products are exact products of bf16 pairs accumulated in fp32 (v_mfma_f32_32x32x16_bf16); x is rounded to the
 * nearest bf16 (ties to even) on its way to LDS, w_main is supplied rounded.  The tail is NOT rounded: nine fp32 FMAs per
 * output, added after the main sum.  Pixels outside the map contribute 0 to both.  Opt-in: bts_conv_fwd_f32 never takes
 * this path on its own (precision 2 keeps these layers on BTS_CONV_KIND_HALO_TAIL, in fp32).
 *   x         : NHWC [B,h,w], x_pix_stride >= c_main floats per pixel (a multiple of 4), 16-byte aligned; c_main % 32 == 0
 *   w_main    : bf16 [c_out_pad][9 * c_main], k = tap * c_main + c, 16-byte aligned (bts_amd/ops.py:pack_conv_tail_bf16)
 *   w_tail    : fp32 [c_out_pad][9][4], slot j = tail plane j (unused slots zero), 16-byte aligned
 *   tail_plane: fp32 [B,h,w], 4-byte aligned; n_tail = 1 (2..4: BTS_ERR_UNSUPPORTED)
 *   y         : NHWC [B,h,w], y_pix_stride >= c_out (a channel slice is fine: nothing is written outside it)
 *   c_out_pad % 32 == 0, >= c_out (rows past c_out are read, never stored); act 0 none / 1 ReLU / 2 ELU; e2_* [c_out] or both NULL
 * c_main % 32 != 0: BTS_ERR_UNSUPPORTED.  Sum order fixed: bits do not depend on B. */
int bts_conv_tail_bf16_fwd_f32(const float* x, long x_pix_stride, int B, int h, int w, int c_main, const void* w_main,
                               const float* w_tail, const float* tail_plane, int n_tail, int c_out, int c_out_pad,
                               const float* e2_scale, const float* e2_shift, int act, float* y, long y_pix_stride,
                               bts_stream_t stream);

/* Should a planar-tail layer take bts_conv_tail_bf16_fwd_f32 (host-side query, no GPU work, no pointers)?  Eligible:
 * n_tail == 1, c_main % 32 == 0, c_out >= 64 and a grid of 4x32-pixel tiles that is at least 0.80 real pixels (the bf16 halo
 * tile's own threshold).  Per-frame geometry and the declared fill_frames (as in bts_conv_desc, 0 = the library default)
 * only, never B.
 *   *bn = output channels per workgroup (128 or 64), *workgroups = workgroups of the DECLARED launch (fill_frames frames);
 *   both 0 when the layer should stay on bts_conv_fwd_f32's fp32 tail kernel. */
int bts_conv_tail_bf16_plan(int h, int w, int c_main, int c_out, int n_tail, int fill_frames, int* bn, long* workgroups);

/* A 1x1 convolution with c_out % 192 == 0 (DenseNet161's bottleneck layers) in the precision-2 arithmetic, in one launch of
 * the wide bf16 tile (csrc/conv_1x1_bf16.inc: one workgroup = 128 pixels x ALL 192 channels of an N tile, so every input
 * value is fetched, affined and converted once):
 *   y[p][n] = act( e1( sum_{c < c_in} bf16( P(x[p][c]) ) * w_bf16[n][c] ) )
 *   P(v)  = fma(v, pre_scale[c], pre_shift[c]), then max(., 0) when pre_relu     (identity when pre_* are NULL)
 *   e1(a) = fma(a, e1_scale[n], e1_shift[n])                                    (identity when e1_* are NULL)
 * ROUNDED: P's result, once, to the nearest bf16 (ties to even); P itself is ONE fused multiply-add in fp32.  w_bf16 is
 * supplied rounded.  NOT rounded: the products (exact in fp32), the sum (fp32, v_mfma_f32_32x32x16_bf16), the epilogue, and
 * every tensor in memory (x, y and the vectors are fp32).  Opt-in: bts_conv_fwd_f32 never takes this path on its own
 * (precision 2 keeps these layers on BTS_CONV_KIND_ROW_BF16).
 *   x       : [npix] NHWC pixels, x_pix_stride >= c_in floats per pixel (a multiple of 4), 16-byte aligned; c_in % 16 == 0.
 *             A channel-prefix view is fine: channels >= c_in are never loaded.
 *   w_bf16  : bf16 [c_out_pad][k_pad], k = c, 16-byte aligned: the one-plane precision-2 form of the packed weight
 *             (bts_amd/ops.py:round_bf16 of pack_conv_weight's matrix); k_pad % 32 == 0, k_pad >= c_in.  Columns >= c_in of
 *             a row are read when c_in % 32 == 16 and never multiplied; rows >= c_out are never read.
 *   pre_*   : c_in floats each, 4-byte aligned, or both NULL;  e1_*: c_out floats each, 4-byte aligned, or both NULL
 *   y       : [npix] NHWC pixels, y_pix_stride >= c_out (a multiple of 4), 4-byte aligned; a channel slice of a wider
 *             buffer is fine: nothing is written outside [p][0 .. c_out)
 *   act 0 none / 1 ReLU / 2 ELU
 * BTS_ERR_UNSUPPORTED: c_out % 192 != 0, c_in % 16 != 0, k_pad % 32 != 0, k_pad < c_in, a pixel stride >= 2^26 floats,
 * c_out_pad * k_pad >= 2^32 (32-bit offsets inside a row block and inside the plane), c_in so large that the prologue vectors
 * do not fit LDS.  Any supported shape runs, whatever the plan query says.
 * Sum order fixed (ascending c, in 16-channel MFMA blocks): a pixel's bits depend neither on npix nor on fill_frames.
 * Non-finite values: an input value reaches exactly the outputs of its own pixel; max(NaN, 0) = 0 under pre_relu, as in
 * every other prologue of this library. */
int bts_conv1x1_bf16_fwd_f32(const float* x, long x_pix_stride, long npix, int c_in, const void* w_bf16, int k_pad,
                             int c_out, int c_out_pad, const float* pre_scale, const float* pre_shift, int pre_relu,
                             const float* e1_scale, const float* e1_shift, int act, float* y, long y_pix_stride,
                             bts_stream_t stream);

/* Should a 1x1 layer take bts_conv1x1_bf16_fwd_f32 (host-side query, no GPU work, no pointers)?  Eligible: c_out % 192 == 0,
 * c_in % 16 == 0, and a declared launch (fill_frames as in bts_conv_desc, 0 = the library default; never B) whose pixel
 * tiles fall in the range where the measured bench has the kernel win (csrc/conv_1x1_bf16.inc: the constants and their source).
 *   *bm = pixels per workgroup (128), *bn = output channels per workgroup (192), *workgroups = workgroups PER FRAME
 *   (ceil(h w / 128) * c_out / 192; a launch tiles its B h w pixels as one run, so it has at most that many per frame);
 *   all three 0 when the layer should stay on bts_conv_fwd_f32. */
int bts_conv1x1_bf16_plan(int h, int w, int c_in, int c_out, int fill_frames, int* bm, int* bn, long* workgroups);

/* bts_conv1x1_bf16_fwd_f32 with a BF16 destination: the first bf16-RESIDENT activation of the library (the bottleneck
 * intermediate of a dense layer under BtsModel.bf16_mid_storage, read back by bts_conv3x3_bf16in_fwd_f32).  Everything the fp32
 * entry point says about x, w_bf16, pre_*, e1_*, act, rounding of the operands, sum order and non-finite values holds; the
 * value it would have stored, act(e1(sum)), is rounded ONCE more, to the nearest bf16 (ties to even; v_cvt_pk_bf16_f32, the
 * conversion every precision-2 kernel applies to its input on the way to LDS: NaN stays NaN, infinity infinity), and stored
 * in two bytes.  A consumer that rounds its input to bf16 anyway therefore sees the bits it would have seen.
 *   y       : bf16 [npix] NHWC pixels, y_pix_stride >= c_out counted in BF16 ELEMENTS (a multiple of 4), base 8-byte aligned; a
 *             channel slice of a wider buffer is fine: nothing is written outside [p][0 .. c_out)
 * Every host check of bts_conv1x1_bf16_fwd_f32 applies, with the same two error codes (a pixel stride >= 2^26 elements
 * included).  Any supported shape runs, whatever a plan query says. */
int bts_conv1x1_bf16_fwd_bf16(const float* x, long x_pix_stride, long npix, int c_in, const void* w_bf16, int k_pad,
                              int c_out, int c_out_pad, const float* pre_scale, const float* pre_shift, int pre_relu,
                              const float* e1_scale, const float* e1_shift, int act, void* y, long y_pix_stride,
                              bts_stream_t stream);

/* A 3x3 convolution (stride 1, padding 1, dilation 1) whose input is a BF16 NHWC tensor, in one launch of the one-plane bf16
 * halo tile (csrc/conv_3x3_bf16in.inc):
 *   y[b][Y][X][n] = act( e1( sum_{tap, c < c_in} x[b][Y+dy][X+dx][c] * w_bf16[n][tap * c_in + c] ) ),   tap = 3 (dy+1) + (dx+1)
 * Products of bf16 pairs are exact in fp32 and accumulate in fp32 (v_mfma_f32_32x32x16_bf16); pixels outside the map
 * contribute 0; e1(a) = fma(a, e1_scale[n], e1_shift[n]).  NOTHING is rounded here: x and w_bf16 are supplied in bf16.  Where
 * x holds the nearest-even rounding of an fp32 tensor, the result is bit for bit bts_conv_fwd_f32's at precision 2 on that
 * tensor wherever that runs BTS_CONV_KIND_HALO_BF16 (same tile, sum order and epilogue).  Opt-in: bts_conv_fwd_f32 never takes
 * this path on its own.
 *   x       : bf16 NHWC [B,h,w], x_pix_stride >= c_in counted in bf16 elements (a multiple of 4), base 8-byte aligned;
 *             c_in % 32 == 0.  A channel-prefix view is fine: channels >= c_in are never loaded.
 *   w_bf16  : bf16 [c_out_pad][k_pad], k = tap * c_in + c, 16-byte aligned: the one-plane precision-2 form of the packed 3x3
 *             weight (bts_amd/ops.py:round_bf16 of pack_conv_weight's matrix); k_pad % 8 == 0, k_pad >= 9 c_in
 *   y       : fp32 NHWC [B,h,w], y_pix_stride >= c_out floats, 4-byte aligned (a channel slice is fine: nothing is written
 *             outside it)
 *   c_out_pad % 32 == 0, >= c_out (rows past c_out are read, never stored); act 0 none / 1 ReLU / 2 ELU; e1_* [c_out_pad] or
 *   both NULL.  Output channels per workgroup: 128 where bts_conv_fwd_f32 would pick 128 for c_out, else 64.
 * BTS_ERR_INVALID: null or misaligned operands, strides that are no multiple of 4 or too short, act == 3.
 * BTS_ERR_UNSUPPORTED: c_in % 32 != 0, k_pad % 8 != 0 or < 9 c_in, B h w x_pix_stride >= 2^32, B h w >= 2^31,
 * c_out_pad k_pad >= 2^32, 64 y_pix_stride >= 2^32 (the 32-bit offsets of bts_conv_tail_bf16_fwd_f32).  Any supported shape
 * runs, whatever the plan query says.  Sum order fixed: bits do not depend on B. */
int bts_conv3x3_bf16in_fwd_f32(const void* x, long x_pix_stride, int B, int h, int w, int c_in, const void* w_bf16, int k_pad,
                               int c_out, int c_out_pad, const float* e1_scale, const float* e1_shift, int act, float* y,
                               long y_pix_stride, bts_stream_t stream);

/* Should a 3x3 layer whose input a caller could keep in bf16 take bts_conv3x3_bf16in_fwd_f32 (host-side query, no GPU work, no
 * pointers)?  Accepted: exactly the layers for which bts_conv_plan_f32 answers BTS_CONV_KIND_HALO_BF16 at precision 2 with no
 * prologue, no residual, no y2, stride 1, dilation 1 and NHWC output -- asked with a split-K workspace lent, as the encoder
 * lends one (without one that answer covers a superset) -- less the classes the per-layer bench has lose
 * (csrc/conv_mfma.hip: the constant and its source).  Per-frame geometry and the declared fill_frames (as in bts_conv_desc,
 * 0 = the library default) only, never B.
 *   *bn = output channels per workgroup (128 or 64), *workgroups = workgroups of the DECLARED launch (fill_frames frames);
 *   both 0 when the layer should stay on bts_conv_fwd_f32 (and its input in fp32). */
int bts_conv3x3_bf16in_plan(int h, int w, int c_in, int c_out, int fill_frames, int* bn, long* workgroups);

/* The same wide bf16 tile at 128, 192 or 256 output channels per workgroup, with the bottleneck epilogue: ResNe(X)t's conv1 /
 * conv3 / stride-1 downsample 1x1 layers and DenseNet121's bottlenecks (c_out 128) in the precision-2 arithmetic.  Everything
 * bts_conv1x1_bf16_fwd_f32 says about x, w_bf16, pre_*, e1_*, y, act, rounding, sum order and non-finite values holds; added:
 *   y[p][n] = act( e1( sum ... ) + res[p][n] )      ONE fp32 add after e1 and before the activation (bts_conv_desc.res);
 *                                                   with e1 absent y = act(sum + res)
 *   res     : NULL, or [npix] NHWC pixels, res_pix_stride >= c_out (a multiple of 4), 4-byte aligned; only [p][0 .. c_out) of
 *             pixels p < npix is read.  A NaN in res[p][n] reaches y[p][n] (and y2[p][n]) and nothing else.
 *   y2      : NULL, or a second destination of the same values (bts_conv_desc.y2: the skip tap of layers 1-3), [npix] NHWC
 *             pixels, y2_pix_stride >= c_out (a multiple of 4), 4-byte aligned; nothing is written outside [p][0 .. c_out)
 *             A stride given for a NULL res / y2 is ignored.
 *   bn      : 128, 192 or 256 forces that tile (BTS_ERR_UNSUPPORTED unless it divides c_out; BTS_ERR_INVALID for any other
 *             value); 0 = the library's choice, a pure function of c_out: 192 where c_out % 192 == 0, else 128 -- the
 *             per-layer bench has 256 lose to 128 on some class of every width (csrc/conv_1x1_bf16.inc).  A pixel's bits
 *             do not depend on bn.
 * BTS_ERR_UNSUPPORTED: c_out a multiple of neither 128 nor 192 (ResNet-50/101's 64-wide layer-1 conv1 stays on
 * bts_conv_fwd_f32), and everything bts_conv1x1_bf16_fwd_f32 answers it for (res / y2 strides >= 2^26 included).
 * Any supported shape runs, whatever the plan query says.  bn = 192 without res and y2 is the launch of
 * bts_conv1x1_bf16_fwd_f32 itself. */
int bts_conv1x1_bf16_wide_fwd_f32(const float* x, long x_pix_stride, long npix, int c_in, const void* w_bf16, int k_pad,
                                  int c_out, int c_out_pad, const float* pre_scale, const float* pre_shift, int pre_relu,
                                  const float* e1_scale, const float* e1_shift, const float* res, long res_pix_stride,
                                  int act, float* y, long y_pix_stride, float* y2, long y2_pix_stride, int bn,
                                  bts_stream_t stream);

/* Should a 1x1 layer take bts_conv1x1_bf16_wide_fwd_f32 (host-side query, no GPU work, no pointers, no batch: fill_frames as
 * in bts_conv_desc, 0 = the library default)?  has_res: the layer adds an identity (ResNet's conv3).  Eligible: a supported
 * width whose layer class the per-layer bench measured to win (csrc/conv_1x1_bf16.inc: the constants and their source); a
 * class that was not measured to win is refused.
 *   *bm = 128, *bn = the tile bn = 0 launches, *workgroups = workgroups PER FRAME (ceil(h w / 128) * c_out / bn);
 *   all three 0 when the layer should stay on bts_conv_fwd_f32. */
int bts_conv1x1_bf16_wide_plan(int h, int w, int c_in, int c_out, int has_res, int fill_frames, int* bm, int* bn,
                               long* workgroups);

/* The decoder's full-resolution planar-tail 3x3 convolution (conv1: stride 1, padding 1, 32 NHWC feature channels plus up to
 * four dense depth planes in, 32 channels out, activation, NCHW result) in one launch of a fused Winograd F(2x2,3x3) kernel
 * (csrc/conv_wino_tail.inc):
 *   y[b][n][Y][X] = act( sum_{tap, c < 32} x[b][Y+dy][X+dx][c] * w[n][c][tap]
 *                      + sum_{tap, j < n_tail} plane_j[b][Y+dy][X+dx] * w_tail[n][tap][j] ),   tap = 3 (dy+1) + (dx+1)
 * zero padding, stride 1, no affine stage.  MAIN term: Winograd F(2x2,3x3) with exact fp32 MFMA products, 16 per 2x2
 * output window and channel pair instead of 36; U = G g G^T is made offline in fp64 and rounded once.  TAIL term: DIRECT
 * form (36 MFMAs of one k-step), added after the output transform: a non-finite plane value reaches exactly the outputs
 * whose nine taps touch it; a non-finite x value may spread over its 4x4 window.  Opt-in: bts_conv_fwd_f32 never takes
 * this path on its own.
 *   x      : NHWC [B,h,w], x_pix_stride >= 32 floats per pixel (a multiple of 4), 16-byte aligned
 *   u      : 16 * 32 * 32 floats, 16-byte aligned, in MFMA A-fragment order (bts_amd/ops.py:pack_conv_tail_wino):
 *            float index ((((xi * 2 + cb) * 2 + half) * 64 + lane) * 4 + q
 *            = U[xi = 4 a + b][n = 16 cb + (lane & 15)][c = 16 half + 4 (lane >> 4) + q],  U[.][n][c] = G w[n][c] G^T,
 *            G = [[1,0,0],[1/2,1/2,1/2],[1/2,-1/2,1/2],[0,0,1]]
 *   w_tail : 2 * 9 * 64 floats: index (cb * 9 + tap) * 64 + lane = w_tail[n = 16 cb + (lane & 15)][tap][j = lane >> 4],
 *            the tail weights bit for bit, slots j >= n_tail zero
 *   tail0..3 : dense fp32 planes [B,h,w], 4-byte aligned; the first n_tail (0..4) are read, the others ignored (may be NULL):
 *            an absent plane contributes exact zeros
 *   y      : contiguous NCHW [B,32,h,w], 8-byte aligned;  act 0 none / 1 ReLU / 2 ELU
 * c_main != 32 or c_out != 32: BTS_ERR_UNSUPPORTED.  Sum order fixed: a frame's bits depend neither on B nor on fill_frames. */
int bts_conv_tail_wino_fwd_f32(const float* x, long x_pix_stride, int B, int h, int w, int c_main, const float* u,
                               const float* w_tail, const float* tail0, const float* tail1, const float* tail2,
                               const float* tail3, int n_tail, int c_out, int act, float* y, bts_stream_t stream);

/* Should a layer take bts_conv_tail_wino_fwd_f32 (host-side query, no GPU work, no pointers)?  Eligible: precision 0,
 * c_main == 32, c_out == 32, n_tail 0..4, a grid of 4x32-pixel workgroup tiles that is at least 0.70 real pixels, and a
 * declared launch (fill_frames as in bts_conv_desc, 0 = the library default; never B) of at least 2048 workgroups.
 *   *bm = windows per workgroup (32), *bn = output channels per workgroup (32), *workgroups = workgroups PER FRAME;
 *   all three 0 when the layer should stay on bts_conv_fwd_f32. */
int bts_conv_tail_wino_plan(int h, int w, int c_main, int c_out, int n_tail, int precision, int fill_frames, int* bm, int* bn,
                            long* workgroups);

/* ResNeXt's grouped 3x3 convolution (stride 1, padding 1, dilation 1, c channels in and out in `groups` groups of
 * cg = c / groups channels; forward, fp32) in one launch of the multi-block fp32 MFMA kernel (csrc/conv_grouped.inc,
 * v_mfma_f32_16x16x1_4b_f32: one 16-channel block per MFMA block):
 *   y[p][n] = act( e1( sum_{tap, k < cg} x[q(p, tap)][cg * (n / cg) + k] * w[n][k][tap] ) ),   tap = 3 (dy+1) + (dx+1)
 * zero padding; e1 = per-channel scale / shift (both or neither); act 0 none / 1 ReLU / 2 ELU.  Opt-in: bts_conv_fwd_f32
 * never takes this path on its own (it runs grouped layers as bts_conv_desc.n_bundles channel bundles).
 *   x, y     : NHWC [B,h,w], pixel strides >= c floats (multiples of 4), 16-byte aligned; y may be a channel slice
 *   w_packed : 144 * c floats, 16-byte aligned (bts_amd/ops.py:pack_grouped_native): float index
 *              ((s * 9 + tap) * 16 + k) * 64 + lane = the weight from input channel 64 s + 16 (lane >> 4) + k to output
 *              channel n = 64 s + lane: w[n][(16 (lane >> 4) + k) mod cg][tap] when that input channel lies in n's group,
 *              else 0 (cg < 16: the 16-channel block is block-diagonal)
 *   e1_scale, e1_shift : c floats each, 16-byte aligned, or both NULL
 * c % 64 != 0 or cg not in {4, 8, 16}: BTS_ERR_UNSUPPORTED.  Any supported shape runs, whatever the plan query says.
 * Sum order fixed (tap-major, input channel ascending): a frame's bits depend neither on B nor on fill_frames.
 * Non-finite values: an input value reaches only outputs of its own 16-channel block whose nine taps touch it -- its own
 * group for cg 16; for cg < 16 also the other groups of that block (0 * inf; the bundle path does the same over 32 channels). */
int bts_conv_grouped_fwd_f32(const float* x, long x_pix_stride, int B, int h, int w, int c, int groups, const float* w_packed,
                             const float* e1_scale, const float* e1_shift, int act, float* y, long y_pix_stride,
                             bts_stream_t stream);

/* Should a grouped layer take bts_conv_grouped_fwd_f32 (host-side query, no GPU work, no pointers)?  Eligible: precision 0,
 * c % 64 == 0, cg in {4, 8, 16}, a grid of 8x16-pixel tiles that is at least 0.55 real pixels, and a declared launch
 * (fill_frames as in bts_conv_desc, 0 = the library default; never B) of at least 1024 (tile, 64-channel slab) pairs.
 *   *bm = pixels per workgroup tile (128), *bn = output channels per workgroup (64), *workgroups = (tile, slab) pairs PER
 *   FRAME; all three 0 when the layer should stay on bundles. */
int bts_conv_grouped_plan(int h, int w, int c, int groups, int precision, int fill_frames, int* bm, int* bn, long* workgroups);

/* The same grouped 3x3 convolution with bf16 operands (the arithmetic of bts_conv_desc.precision = 2) in one launch of the
 * bf16 grouped kernel (csrc/conv_grouped_bf16.inc, v_mfma_f32_16x16x16_bf16: one 16-channel block x one tap per MFMA):
 *   y[p][n] = act( e1( sum_{tap, k < cg} bf16(x[q(p, tap)][cg * (n / cg) + k]) * bf16(w[n][k][tap]) ) ),   tap = 3 (dy+1) + (dx+1)
 * x is rounded to bf16 (nearest, ties to even) on its way to LDS, padding is an exact zero; products are exact in fp32 and
 * accumulate in fp32; e1 and act as above, in fp32.  Opt-in: bts_conv_fwd_f32 never takes this path on its own.
 *   x, y          : as bts_conv_grouped_fwd_f32 (fp32 NHWC, pixel strides >= c floats and multiples of 4, 16-byte aligned)
 *   w_packed_bf16 : 144 * c bf16 (no padding tap), 16-byte aligned (bts_amd/ops.py:pack_grouped_native_bf16): bf16 index
 *                   (((s * 9 + tap) * 4 + b) * 64 + lane) * 4 + j = the weight from input channel
 *                   ci = 64 s + 16 b + 4 (lane >> 4) + j to output channel n = 64 s + 16 b + (lane & 15):
 *                   bf16_rne(w[n][ci mod cg][tap]) when ci lies in n's group, else 0 (cg < 16: block-diagonal)
 *   e1_scale, e1_shift : as bts_conv_grouped_fwd_f32
 * Any supported shape runs, whatever bts_conv_grouped_bf16_plan says.  c % 64 != 0 or cg outside {4, 8, 16}: BTS_ERR_UNSUPPORTED.
 * Sum order fixed (tap-major, the 16 channels of a block inside one MFMA): a frame's bits depend neither on B nor on
 * fill_frames.  Non-finite values: as bts_conv_grouped_fwd_f32 (own 16-channel block, 3x3 neighbourhood). */
int bts_conv_grouped_bf16_fwd_f32(const float* x, long x_pix_stride, int B, int h, int w, int c, int groups,
                                  const void* w_packed_bf16, const float* e1_scale, const float* e1_shift, int act, float* y,
                                  long y_pix_stride, bts_stream_t stream);

/* Should a grouped layer take bts_conv_grouped_bf16_fwd_f32 (host-side query, no GPU work, no pointers)?  Eligible only for
 * precision 2, c % 64 == 0, cg in {4, 8, 16}, and the tile-grid fill and declared-launch thresholds written next to the
 * constants in csrc/conv_grouped_bf16.inc (fill_frames as in bts_conv_desc, 0 = the library default; never B).
 *   *bm = 128, *bn = 64, *workgroups = (tile, slab) pairs PER FRAME; all three 0 when the layer should stay on bundles. */
int bts_conv_grouped_bf16_plan(int h, int w, int c, int groups, int precision, int fill_frames, int* bm, int* bn, long* workgroups);

/* Weight gradient of the same grouped 3x3 convolution (csrc/conv_grouped_wgrad.inc, v_mfma_f32_16x16x1_4b_f32: one
 * instruction accumulates four 16 x 16 (output channel x input channel) blocks from one dy and one x float per lane):
 *   dw[n][k][tap] = sum_{b, p} dy[b, p][n] * x[b, q(p, tap)][cg * (n / cg) + k],   tap = 3 (dy+1) + (dx+1)
 * stride 1, padding 1, zero padding.  The input gradient needs no entry point of its own: bts_conv_grouped_fwd_f32 on dy
 * with the weights of bts_pack_weights_f32's gmode 4.
 *   x, dy : NHWC [B,h,w], pixel strides >= c floats (multiples of 4), 16-byte aligned; either may be a channel slice of a
 *           wider buffer
 *   dw    : c * cg * 9 floats, 16-byte aligned, the parameter's own OIHW layout [c][cg][3][3]; every float is written
 *   ws    : ws_floats floats of scratch for the split partials, 16-byte aligned, or NULL
 * The tile axis (8 x 16-pixel tiles of all B frames) is split over workgroups; partials [split][c / 64][9][16][64] go to ws
 * and a second launch sums the in-group entries in ascending split order and writes OIHW (no atomics; the products of a
 * 16-channel block that cross groups, cg < 16, are computed and never reach dw).  The split count is a function of
 * (B, h, w, c, groups, ws_floats) only: min(ceil(512 / (c / 64)), tiles), lowered to what ws holds (ws_floats / (144 c)),
 * 1 with ws == NULL or room for fewer than two partials -- never an error; then settled so that no split is empty.
 * c % 64 != 0 or cg not in {4, 8, 16}: BTS_ERR_UNSUPPORTED, as is B * h * w >= 2^31 (32-bit pixel and tile indices).
 * Sum order fixed by the shape and the split count: bit-reproducible.  Non-finite values: an x or dy value reaches only dw
 * entries of its own 16-channel block; the cross-group products are dropped, so for the written entries its own group.
 * Pixels of ragged tiles outside the map are skipped, never multiplied by zero. */
int bts_conv_grouped_wgrad_f32(const float* x, long x_pix_stride, const float* dy, long dy_pix_stride, int B, int h, int w, int c,
                               int groups, float* dw, float* ws, long ws_floats, bts_stream_t stream);

/* The split bts_conv_grouped_wgrad_f32 runs with a workspace of ws_floats floats (host-side query, no GPU work, no pointers;
 * ws_floats 0 = no workspace) and the floats of it the launch writes (0 when unsplit; <= ws_floats).  Unsupported shapes are
 * refused as by the launch. */
int bts_conv_grouped_wgrad_plan(int B, int h, int w, int c, int groups, long ws_floats, int* splits, long* ws_floats_used);

/* Which kernel bts_conv_fwd_f32 will launch for this descriptor (host-side query, no GPU work: it walks the real
 * dispatch path): lets a profiler attribute a launch to its kernel instantiation.
 *   *kind = one kernel family (kind & BTS_CONV_KIND_MASK) plus any of the BTS_CONV_FLAG_* bits. */
enum {
    BTS_CONV_KIND_ROW       = 0,   /* conv_fwd_kernel: row-tiled, BM x BN (precision 0 and 1)                          */
    BTS_CONV_KIND_HALO      = 1,   /* conv_halo_kernel: spatial 128-pixel tile x BN                                    */
    BTS_CONV_KIND_HALO_TAIL = 2,   /* conv_halo_kernel with the planar tail operand                                    */
    BTS_CONV_KIND_WIDE_1X1  = 3,   /* conv1x1_kernel: bm = 128 or 64 pixels x BN                                       */
    BTS_CONV_KIND_STEM      = 4,   /* conv_stem_kernel: 7x7 / stride-2 encoder stem, 8x32-pixel tiles x BN             */
    BTS_CONV_KIND_HALO_EMU  = 5,   /* conv_halo_emu_kernel, precision 1: bf16x3 halo tile                              */
    BTS_CONV_KIND_WINO      = 6,   /* conv_wino_kernel: Winograd F(2x2,3x3)                                            */
    BTS_CONV_KIND_ROW_BF16  = 7,   /* conv_fwd_kernel with bf16 operands (precision 2, row-tiled)                      */
    BTS_CONV_KIND_HALO_BF16 = 8,   /* conv_halo_emu_kernel with one bf16 plane (precision 2, halo tile)                */
    BTS_CONV_KIND_MASK      = 15,
    BTS_CONV_FLAG_SPLITK    = 16,  /* split-K (+ splitk_reduce_kernel); row-tiled families only                        */
    BTS_CONV_FLAG_W8        = 32,  /* the eight-wave variant of the 48-wide halo tile (under-filled launches)          */
    BTS_CONV_FLAG_DIL       = 64   /* the dilated halo tile (dilation 3 / 6 / 12 ASPP branches, c_out 128)             */
};
int bts_conv_plan_f32(const bts_conv_desc* desc, int* bm, int* bn, int* kind);

/* Tap-steps the launch really issues vs. the dense count (host-side query, no GPU work).  The row-tiled kernel skips,
 * per 128/64-pixel row tile, the taps that fall into the zero padding for ALL of the tile's pixels (a dilated ASPP
 * branch, reference pytorch/bts.py:65-80: dilation 24 on a 44-row map leaves 6 of 9 taps for most tiles); the
 * skipped products are exact zeros, results are unchanged.  issued / dense = the share of the algorithmic FLOPs
 * the matrix pipe executes; both are 0 for launches that never skip (halo-tile and wide 1x1 kernels). */
int bts_conv_plan_ksteps_f32(const bts_conv_desc* desc, long* issued, long* dense);

/* ------------------------------------------------------------------------------------------
 * Training step (reference: autograd of the nn.Conv2d modules of pytorch/bts.py:70-77, 87-93, 108-119,
 * 180-221, driven by bts_main.py:476-500).  The input gradient of a stride-1 convolution IS a convolution
 * (flipped, transposed weights; pad' = dil*(ksize-1) - pad) and goes through bts_conv_fwd_f32; the weight
 * gradient is this entry point:
 *
 *   dw[co][tap][ci] = sum_p dy[p][co] * x[q(p,tap)][ci]        (q as in bts_conv_desc, incl. `up`)
 *
 * dw is written in OHWI order ([c_out][ksize*ksize][c_in], the layout the forward kernel packs from); the caller
 * permutes to the state dict's OIHW.  c_in % 4 == 0 and c_out % 4 == 0 (pad odd channel counts with zeros).
 * ws: optional scratch for the deterministic split over pixels; without it one workgroup column walks all pixels.
 */
typedef struct bts_conv_wgrad_desc {
    const float* x;         /* forward input, NHWC: pixel q channel c at x[q*x_pix_stride + c]           */
    long  x_pix_stride;
    int   c_in;
    const float* dy;        /* gradient of the forward output, NHWC [B,H,W,c_out]                        */
    long  dy_pix_stride;
    int   c_out;
    int   B, h_in, w_in;    /* forward input size before the optional upsample                           */
    int   up, ksize, dil, stride, pad;
    float* dw;              /* [c_out][ksize*ksize][c_in]                                                */
    float* ws;              /* NULL or scratch, exclusive to this stream while the call runs             */
    long  ws_floats;
    int   n_bundles;        /* 0/1: ordinary.  > 1: grouped convolution as channel bundles (see bts_conv_desc):
                               c_in / c_out are PER BUNDLE, bundle j uses x channels [j*c_in, ..) and dy channels
                               [j*c_out, ..); dw = [n_bundles][c_out][ksize*ksize][c_in] dense blocks, of which the
                               caller keeps each group's diagonal block                                            */
    const float* pre_scale; /* optional [n_bundles*c_in] (16-byte aligned): the forward convolution consumed           */
    const float* pre_shift; /* relu?(x*pre_scale + pre_shift) (a norm layer folded into its prologue, see               */
    int   pre_relu;         /* bts_conv_desc.pre_*); the gather applies the same transform, padding stays zero        */
} bts_conv_wgrad_desc;

int bts_conv_wgrad_f32(const bts_conv_wgrad_desc* desc, bts_stream_t stream);

/* Which tile and pixel split bts_conv_wgrad_f32 will use for this descriptor (host-side query, no GPU work, no device
 * needed: it runs the launch's own validation and planning, so it also rejects what the launch rejects).
 *   bm x bn       : the dw tile of one workgroup -- 128x128, 64x128, 32x128 or 64x64
 *   split         : workgroups along the pixel axis; > 1 means partials in `ws` plus the fixed-order reduction
 *   pix_per_split : pixels per split (a multiple of 32); (split-1)*pix_per_split < B*H*W <= split*pix_per_split
 * The launch writes split * n_bundles * c_out * ksize^2 * c_in floats of `ws` when split > 1.  Pointer fields are only
 * checked (non-null, alignment), never dereferenced; any of the four outputs may be NULL. */
int bts_conv_wgrad_plan_f32(const bts_conv_wgrad_desc* desc, int* bm, int* bn, long* split, long* pix_per_split);

/* Many weight gradients in one launch (a DenseNet block's 2*L problems average tens of microseconds each when launched
 * one at a time, and each is split over pixels far enough to fill the chip on its own; taken together they fill it with
 * little or no split).  Three calls:
 *
 *   bts_conv_wgrad_batch_table_bytes(n)   bytes of the table for n problems (host and device copy have the same size)
 *   bts_conv_wgrad_batch_plan_f32(...)    host only, no GPU work, no device needed: validates every descriptor with the
 *                                         rules of bts_conv_wgrad_f32 (and rejects nothing else), plans tiles and splits
 *                                         for the batch as a whole and fills `table_host`
 *   bts_conv_wgrad_batch_f32(...)         at most one launch per tile shape present in the batch plus one launch that
 *                                         sums the partials of every split problem in wgrad_reduce's fixed order
 *
 * The table is relocatable: every pointer of every descriptor (x, dy, dw, pre_scale, pre_shift) -- together with the
 * whole extent the kernel reads or writes through it -- must lie inside one of n_bases <= 8 caller-declared ranges
 * [bases[j], bases[j] + base_bytes[j]) (16-byte aligned), else BTS_ERR_INVALID; the table stores (base index, byte
 * offset) and the launch receives the current base pointers by value.  The caller copies table_host to the device once
 * per geometry (table_dev) and may then launch every step with that step's buffers, uploading nothing more.  The launch
 * receives base pointers only, no sizes: that every range given at launch is at least as large as the one given to the
 * plan is the caller's contract (as for every buffer of this header), not something the launch can check.  descs[i].ws / ws_floats must be NULL / 0: the
 * partials of the whole batch live in the one workspace `ws` of `ws_floats` floats at disjoint offsets (plan[i].ws_offset,
 * in floats; -1 for an unsplit problem).  The plan never fails for lack of workspace: it lowers the splits, down to 1.
 * The launch writes plan[i].split * n_bundles * c_out * ksize^2 * c_in floats at plan[i].ws_offset for every problem with
 * split > 1 and nothing else of `ws`.  The plan is a function of the problems' shapes and ws_floats only -- not of the
 * pointers or of the device; tile, split and pix_per_split do not depend on the order of the batch either (items follow their
 * problems), ws_offset goes by position among problems of equal shape.  dw regions of different
 * problems that overlap are a caller error (not detected): each is written by its own workgroups in no defined order.
 * Like everything here the launch allocates nothing, synchronises nothing and is hipGraph-capturable.  n = 0 is valid
 * and launches nothing. */
typedef struct bts_conv_wgrad_batch_item {
    int  bm, bn;             /* the dw tile of one workgroup, as in bts_conv_wgrad_plan_f32       */
    long split;              /* workgroups along the pixel axis                                   */
    long pix_per_split;      /* multiple of 32; (split-1)*pix_per_split < B*H*W                   */
    long ws_offset;          /* floats into `ws` where this problem's partials live; -1: split 1  */
} bts_conv_wgrad_batch_item;

long bts_conv_wgrad_batch_table_bytes(int n);
int  bts_conv_wgrad_batch_plan_f32(const bts_conv_wgrad_desc* descs, int n, const void* const* bases, const long* base_bytes,
                                   int n_bases, long ws_floats, void* table_host, bts_conv_wgrad_batch_item* plan /* [n] or NULL */);
int  bts_conv_wgrad_batch_f32(const void* table_host, const void* table_dev, int n, const void* const* bases, int n_bases,
                              float* ws, bts_stream_t stream);

/* The weight gradient with bf16 operands and fp32 accumulation (the training step's opt-in train_precision "bf16"):
 *
 *   dw[co][tap][ci] = sum_p bf16(dy[p][co]) * bf16(x'[q(p,tap)][ci])
 *
 * x' is the gathered input after pre_scale / pre_shift / pre_relu with the zero padding applied after that prologue; both
 * operands are rounded to the nearest bf16 (ties to even) on their way to the matrix cores (v_mfma_f32_32x32x16_bf16),
 * products of bf16 pairs are exact in fp32 and the sums are fp32.  Everything in memory stays fp32.  Descriptor, checks,
 * tile, split, pix_per_split, workspace use and the fixed-order split sum are EXACTLY those of bts_conv_wgrad_f32 -- a
 * value that is representable in bf16 gives the fp32 entry point's result up to the order of the fp32 additions inside a
 * split.  bts_conv_wgrad_bf16_plan_f32 answers what bts_conv_wgrad_plan_f32 answers, or BTS_ERR_UNSUPPORTED for a shape
 * class the bf16 body is not offered for (none today): the caller then launches bts_conv_wgrad_f32.
 * bts_conv_wgrad_batch_bf16_f32 consumes the table of bts_conv_wgrad_batch_plan_f32 unchanged. */
int  bts_conv_wgrad_bf16_f32(const bts_conv_wgrad_desc* desc, bts_stream_t stream);
int  bts_conv_wgrad_bf16_plan_f32(const bts_conv_wgrad_desc* desc, int* bm, int* bn, long* split, long* pix_per_split);
int  bts_conv_wgrad_batch_bf16_f32(const void* table_host, const void* table_dev, int n, const void* const* bases, int n_bases,
                                   float* ws, bts_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Sub-pixel upconv in the training step (reference upconv, pytorch/bts.py:83-94: nearest-2x + 3x3 convolution).  With
 * S_0 = [[1,0,0],[0,1,1]], S_1 = [[1,1,0],[0,0,1]] and the class filters g_(py,px) = S_py w S_px^T (2x2, the filters of
 * bts_conv_desc.subpixel), x zero outside the [h,w] source map:
 *   forward          y[2Y+py, 2X+px] = sum_{ty,tx} g_(py,px)[ty,tx] x[Y-1+py+ty, X-1+px+tx]        (bts_conv_fwd_f32, subpixel)
 *   input gradient   dx[Y,X] = sum_{r,s in 0..3} K[r,s] dy[2Y-1+r, 2X-1+s],  K[3-py-2ty, 3-px-2tx] = g_(py,px)[ty,tx]^T
 *   weight gradient  dg_(py,px)[ty,tx] = sum_{b,Y,X} dy[2Y+py, 2X+px] (x) x[Y-1+py+ty, X-1+px+tx],
 *                    dw[ky,kx] = sum_{py,px} dg_(py,px)[tau_py(ky), tau_px(kx)],  tau_0 = (0,1,1), tau_1 = (0,0,1)
 * 16 products per source pixel, input and output channel in every pass (the 3x3 on the upsampled grid issues 36).
 * c_in % 4 == 0 and c_out % 4 == 0 throughout, every pointer 16-byte aligned, pixel strides multiples of 4 floats and at
 * least the channel count; anything else is BTS_ERR_INVALID before any GPU work.
 *
 * bts_upconv_dgrad_f32: dx = the 4x4 / stride-2 / padding-1 convolution above, on the row-tiled convolution kernel.
 *   dy: NHWC [B,2h,2w], dy_pix_stride >= c_out;  dx: NHWC [B,h,w], dx_pix_stride >= c_in (every real channel written)
 *   w_dgrad: [round_up(c_in,32)][round_up(16*c_out,32)], element [c][(4r+s)*c_out + n] = K[r,s][c][n], zero padded
 *            (bts_upconv_train_pack_f32 writes it)
 *   precision, fill_frames, splitk_ws / splitk_ws_floats: as in bts_conv_desc (precision 0 or 1 in training; the
 *            workspace is NULL with 0 floats, or lets under-filled launches split K with the fixed-order reduction).
 * bts_upconv_dgrad_plan: the kernel that launch will take (host only, no pointers): *bm x *bn tile and *kind as
 * bts_conv_plan_f32 reports them (BTS_CONV_KIND_ROW, plus BTS_CONV_FLAG_SPLITK when it splits). */
int bts_upconv_dgrad_f32(const float* dy, long dy_pix_stride, int B, int h, int w, int c_out, const float* w_dgrad, int c_in,
                         float* dx, long dx_pix_stride, int precision, int fill_frames, float* splitk_ws, long splitk_ws_floats,
                         bts_stream_t stream);
int bts_upconv_dgrad_plan(int B, int h, int w, int c_out, int c_in, int precision, int fill_frames, long splitk_ws_floats,
                          int* bm, int* bn, int* kind);

/* bts_upconv_wgrad_f32: dw in OHWI [c_out][9][c_in] (the layout bts_conv_wgrad_f32 writes).
 *   x: forward input NHWC [B,h,w], x_pix_stride >= c_in;  dy: NHWC [B,2h,2w], dy_pix_stride >= c_out
 *   ws: MANDATORY scratch of ws_floats floats, exclusive to this stream while the call runs (the class gradients need a
 *       home even unsplit).  The launch writes EXACTLY split * 16 * c_out * c_in floats -- [split][class][c_out][4*c_in],
 *       class = 2 py + px, column (2 ty + tx) * c_in + ci -- and nothing beyond; ws_floats below 16 * c_out * c_in is
 *       BTS_ERR_INVALID.
 * Tile and pixel split are bts_conv_wgrad_f32's planner on M = B*h*w source pixels, N = 4*c_in and four bundles (the
 * classes).  A second launch sums in a fixed order (no atomics, bit-reproducible): per class the split partials exactly as
 * bts_conv_wgrad_f32's reduction does (lane j of 16 adds splits j, j+16, ... four at a time as (a0+a1)+(a2+a3), then the
 * 16 lane sums in lane order) giving r_0..r_3, then dw = ((r_0 + r_1) + r_2) + r_3.
 * bts_upconv_wgrad_plan_f32: tile, split and pixels per split that launch will use for a workspace of ws_floats floats
 * (host only, no pointers, no device; rejects what the launch rejects); any of the four outputs may be NULL. */
int bts_upconv_wgrad_f32(const float* x, long x_pix_stride, int B, int h, int w, int c_in, const float* dy, long dy_pix_stride,
                         int c_out, float* dw, float* ws, long ws_floats, bts_stream_t stream);
int bts_upconv_wgrad_plan_f32(int B, int h, int w, int c_in, int c_out, long ws_floats, int* bm, int* bn, long* split,
                              long* pix_per_split);

/* bts_upconv_train_pack_f32: both packs of every registered upconv weight in ONE launch, once per training step.
 * table: n_entries device records of 12 int64 each --
 *   { src (OIHW float* [c_out][c_in][3][3]), fwd (float*), dgrad (float*), c_out, c_in, c_in_ld, c_out_ld, c_out_pad,
 *     k_pad_f, c_in_pad, k_pad_d, first_block (prefix sum of bts_upconv_train_pack_blocks over the table) }
 *   fwd   [4][c_out_pad][k_pad_f]: [2py+px][n][(2ty+tx)*c_in_ld + c] = g_(py,px)[ty,tx][n][c]   (bts_conv_desc.subpixel)
 *   dgrad [c_in_pad][k_pad_d]    : [c][(4r+s)*c_out_ld + n] = K[r,s][c][n]                       (bts_upconv_dgrad_f32)
 * zero elsewhere.  Every element is the fp32 sum of the 1, 2 or 4 taps of w it covers, added in the order ky outer, kx
 * inner with one rounding per addition (no fused contraction): the forward pack is bit-identical to
 * bts_amd/ops.py:pack_upconv_subpixel, and a dgrad element has the bits of its forward twin. */
long bts_upconv_train_pack_blocks(long c_out_pad, long k_pad_f, long c_in_pad, long k_pad_d);
int bts_upconv_train_pack_f32(const void* table, int n_entries, long total_blocks, bts_stream_t stream);

/* Batched weight re-packing for the training step (the optimiser rewrites the OIHW parameters every iteration,
 * bts_main.py:606): one launch lays every registered weight out as bts_conv_fwd_f32 wants it.
 * table: n_entries device records of 14 int64 each --
 *   { src (OIHW float*), dst (float* [rows_pad][k_pad]), rows, inner, ksize, c_in_ld, rows_pad, k_pad,
 *     s_row, s_c (element strides of packed row / inner channel in src), flip (1 = spatially flipped taps),
 *     first_block (prefix sum of bts_pack_weights_blocks over the table),
 *     cg, gmode (grouped weights packed block-diagonally per bundle: channels per group and 1 = forward /
 *     2 = input-gradient layout; 0, 0 for dense weights) }
 *   forward layout : rows = c_out, inner = c_in, s_row = c_in*k*k, s_c = k*k, flip 0
 *   input gradient : rows = c_in, inner = c_out, s_row = k*k, s_c = c_in*k*k, flip 1   (transposed, flipped kernel)
 * dst[row][tap*c_in_ld + c] = src[row*s_row + c*s_c + (flip ? k*k-1-tap : tap)], zero elsewhere.
 * gmode 3 / 4: src is a whole grouped [c][cg][3][3] weight and dst the 144 * c floats bts_conv_grouped_fwd_f32 reads
 * (rows_pad * k_pad = 144 * c; of the other fields only cg is read).  With n = 64 s + lane the output channel and
 * ci = 64 s + 16 (lane >> 4) + k the input channel of float ((s * 9 + tap) * 16 + k) * 64 + lane:
 *   gmode 3 (forward)        : w[n][ci mod cg][tap]           where ci lies in n's group, else 0  (ops.pack_grouped_native's bits)
 *   gmode 4 (input gradient) : w[ci][n mod cg][8 - tap]       where ci lies in n's group, else 0  -- the forward layout of
 *                              w_t[cg g + i][o][8 - tap] = w[cg g + o][i][tap]: run on dy it yields dx.
 */
long bts_pack_weights_blocks(long rows_pad, long k_pad);
int bts_pack_weights_f32(const void* table, int n_entries, long total_blocks, bts_stream_t stream);

/* Winograd F(2x2,3x3) form of a packed 3x3 weight (bts_conv_desc.w_wino; the reference has no counterpart: its 3x3
 * convolutions, pytorch/bts.py:83-94 / 183-221 and the DenseNet growth convolutions, go to cuDNN).  `w_packed` is the
 * [c_out_pad][k_pad] matrix bts_conv_fwd_f32 reads (K tap-major, k = tap * c_in_ld + c).  U = G g G^T per (output, input)
 * channel, computed in fp64 and rounded once, written in the B-fragment order of the fused Winograd kernel:
 *   32-wide channel tiles (c_out16 == 0): float ((((xi*nchunks + chunk)*n_ct + ct)*4 + g)*64 + lh*32 + li)*4 + q
 *       = U[xi][n = 32 ct + li][k = 32 chunk + 8 g + 4 lh + q],  n_ct = c_out_pad / 32;
 *   16-wide tiles (c_out16 = real output channels, a multiple of 16: the 48-wide DenseNet tile):
 *       ((((xi*nchunks + chunk)*n_ct + ct)*2 + g)*64 + l)*4 + q = U[xi][n = 16 ct + (l & 15)][k = 32 chunk + 16 g + 4 (l >> 4) + q].
 * n_tail > 0: the last 4 of the c_in_ld channels are the planar tail operand and are left out (the kernel adds their
 * products directly).  bts_pack_wino_floats = floats `out` must hold (16-byte aligned), or -1 for an unsupported shape
 * (buffer channels and c_out_pad must be whole multiples of 32). */
long bts_pack_wino_floats(int c_out_pad, int c_in_ld, int n_tail, int c_out16);
int bts_pack_wino_f32(const float* w_packed, int c_out_pad, long k_pad, int c_in_ld, int n_tail, int c_out16,
                      float* out, bts_stream_t stream);

/* Batch-statistic BatchNorm over NHWC rows [npix][C] (nn.BatchNorm2d in train() mode: pytorch/bts.py:69-76,
 * 182-202 and the DenseNet norm layers), C % 4 == 0, row strides % 4 == 0 and >= C (channel slices work in place).
 *
 * bts_bn_train_stats_f32 : per-channel batch mean and biased variance (deterministic tree of Chan-merged partials of x minus its first row)
 *     -> mean, invstd = 1/sqrt(var+eps), scale = gamma*invstd, shift = beta - mean*scale; running_mean/var (may be
 *     NULL) updated as PyTorch does: r = (1-momentum)*r + momentum*{mean | unbiased var}.  gamma/beta NULL = 1/0.
 *     ws: scratch of bts_bn_train_ws_floats(npix, C) floats.
 * bts_bn_apply_nhwc_f32  : y = [relu](x*scale + shift)   (relu != 0 fuses the ReLU that follows the norm layer)
 * bts_bn_train_bwd_f32   : with dy' = dy masked by the fused ReLU (recomputed from x): dbeta = sum dy',
 *     dgamma = sum dy'*xhat, dx = scale*(dy' - dbeta/n - xhat*dgamma/n)  (dx may be NULL: statistics only).
 *
 * Frozen statistics (an eval()-mode nn.BatchNorm2d inside a train()-mode model: bts_main.py --bn_no_track_stats, set_misc ->
 * bn_init_as_tf); the forward is bts_bn_frozen_vectors_f32 followed by bts_bn_apply_nhwc_f32:
 * bts_bn_frozen_vectors_f32 : the same four vectors from the running buffers, which are read and never written:
 *     mean = running_mean, invstd = 1/sqrt(running_var+eps), scale = gamma*invstd, shift = beta - mean*scale.  gamma/beta
 *     NULL = 1/0.  One small launch; the outputs are 16-byte aligned (they may be rows of a wider slab).
 * bts_bn_frozen_bwd_f32     : dbeta = sum dy', dgamma = sum dy'*xhat, dx = scale*dy' (accumulate != 0: dx += scale*dy').  dx
 *     depends on no sum, so this is ONE streaming pass over x and dy (plus the finalize of the sums): 12 bytes per element,
 *     16 accumulating, 8 for the sums alone, against 20 for bts_bn_train_bwd_f32.  dgamma and dbeta are given together
 *     or both NULL (no reduction, ws unused, a single launch); dx NULL = sums only; all three NULL is invalid.  The sums
 *     take the chunk plan (ws of bts_bn_train_ws_floats(npix, C) floats) and the summation order of bts_bn_train_bwd_f32:
 *     deterministic, no atomics.  dx may lie in the same wide buffer as dy in other columns.
 */
long bts_bn_train_ws_floats(long npix, int C);
int bts_bn_train_stats_f32(const float* x, long x_pix_stride, long npix, int C, const float* gamma,
                           const float* beta, float eps, float momentum, float* running_mean, float* running_var,
                           float* ws, long ws_floats, float* mean, float* invstd, float* scale, float* shift,
                           bts_stream_t stream);
int bts_bn_apply_nhwc_f32(const float* x, long x_pix_stride, long npix, int C, const float* scale,
                          const float* shift, int relu, float* y, long y_pix_stride, bts_stream_t stream);
int bts_bn_train_bwd_f32(const float* x, long x_pix_stride, const float* dy, long dy_pix_stride, long npix, int C,
                         const float* mean, const float* invstd, const float* scale, const float* shift, int relu,
                         float* ws, long ws_floats, float* dgamma, float* dbeta, float* dx, long dx_pix_stride,
                         bts_stream_t stream);
int bts_bn_frozen_vectors_f32(const float* gamma, const float* beta, const float* running_mean,
                              const float* running_var, float eps, int C,
                              float* mean, float* invstd, float* scale, float* shift, bts_stream_t stream);
int bts_bn_frozen_bwd_f32(const float* x, long x_pix_stride, const float* dy, long dy_pix_stride, long npix, int C,
                          const float* mean, const float* invstd, const float* scale, const float* shift, int relu,
                          float* ws, long ws_floats, float* dgamma, float* dbeta,
                          float* dx, long dx_pix_stride, int accumulate, bts_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Layout movers between the NCHW boundary (pytorch/bts.py:347-349 tensors) and the NHWC
 * interior.  dst/src NHWC element (p,c) lives at base[p*pix_stride + c].
 *   relu != 0 applies max(v,0) on the way (bts.py:225: dense_features = ReLU(features[5])).
 *   No alignment demand on dst: C == 4 stores 16 bytes per pixel when dst is 16-byte aligned and
 *   dst_pix_stride % 4 == 0, and four scalars otherwise.
 */
int bts_nchw_to_nhwc_f32(const float* src, int B, int C, long HW, float* dst, long dst_pix_stride,
                         int relu, bts_stream_t stream);
int bts_nhwc_to_nchw_f32(const float* src, long src_pix_stride, int B, int C, long HW, float* dst,
                         bts_stream_t stream);

/* Interleave up to four 1-channel planes ([npix] each, e.g. reduc1x1 and the three LPG depth maps)
 * into consecutive channels of an NHWC buffer: dst[p*dst_pix_stride + i] = plane_i[p].
 * Builds the tail of concat1 = cat[upconv1, reduc1x1, depth_2x2, depth_4x4, depth_8x8]
 * (pytorch/bts.py:287) without a torch.cat pass.  Unused planes = NULL (n_planes 1..4).
 */
int bts_pack_planes_f32(const float* p0, const float* p1, const float* p2, const float* p3, int n_planes,
                        long npix, float* dst, long dst_pix_stride, bts_stream_t stream);

/* Encoder-side NHWC pooling (torchvision DenseNet pool0 = MaxPool2d(3,2,1), transition pool =
 * AvgPool2d(2,2); the encoder is the caller side of the hot path, pytorch/bts.py:295-338).
 * maxpool: [B,h,w,C] -> [B,ceil(h/2),ceil(w/2),C], optionally to two destinations.
 * bn_relu_avgpool2: dst = mean_{2x2} relu(src*scale + shift)  (transition norm+relu+pool; its 1x1 conv
 * commutes with the mean and runs afterwards on the pooled map).  C % 4 == 0, strides % 4 == 0 and
 * >= C, pointers 16-byte aligned; anything else is BTS_ERR_INVALID before any GPU work.
 */
int bts_maxpool3x3s2_nhwc_f32(const float* src, long src_pix_stride, int B, int h, int w, int C, float* dst,
                              long dst_pix_stride, float* dst2, long dst2_pix_stride, bts_stream_t stream);
int bts_bn_relu_avgpool2_nhwc_f32(const float* src, long src_pix_stride, int B, int h, int w, int C,
                                  const float* scale, const float* shift, float* dst, long dst_pix_stride,
                                  bts_stream_t stream);

/* get_depth + final scaling (pytorch/bts.py:220-221, 289-291):
 *   final_depth[b,0,y,x] = max_depth * sigmoid( conv3x3(iconv1, w)[b,0,y,x] ) [* focal[b] / 715.0873]
 *   iconv1 : [B,C,H,W] NCHW (the tensor bts.forward returns), w : [1,C,3,3] as stored in the
 *   state dict (get_depth.0.weight), focal : [B] or NULL (non-KITTI datasets skip the focal term).
 */
int bts_get_depth_f32(const float* iconv1, const float* w, int B, int C, int H, int W, float max_depth,
                      const float* focal, float* final_depth, bts_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Evaluation metrics as GPU reductions.  Replaces the per-sample body of online_eval +
 * compute_errors (pytorch/bts_main.py:87-108, 221-254; same code in bts_eval.py:81-102, 237-307), which copies both
 * maps to the host and runs ~25 NumPy passes per sample.
 *
 *   pred  : [B,Hp,Wp] network output (metres).  With do_kb_crop the prediction is pasted into a zero canvas of the
 *           ground truth's size at (top,left) = (Hg-352, (Wg-1216)/2) (bts_main.py:221-227); otherwise Hp==Hg,
 *           Wp==Wg, top=left=0.
 *   gt    : [B,Hg,Wg] ground-truth depth.
 *   clamp : pred<min -> min, pred>max -> max, +inf -> max, NaN -> min (bts_main.py:229-232)
 *   valid : min < gt < max (bts_main.py:234) AND y in [y0,y1), x in [x0,x1) -- the Garg / Eigen crop rectangle of
 *           bts_main.py:236-249 in ground-truth coordinates (0,Hg,0,Wg = no crop)
 *   per_frame : [B][10] doubles <- silog, abs_rel, log10, rms, sq_rel, log_rms, d1, d2, d3 (bts_main.py:84 order),
 *           then the number of valid pixels.
 *   accum : optional [10] doubles, the running `eval_measures` of online_eval: += the nine measures and [9] += 1 for
 *           every frame that has valid pixels (bts_main.py:253-254); all-reduced by the caller (bts_main.py:258-260).
 *   ws    : scratch of bts_eval_ws_doubles(B,Hg,Wg) doubles.
 * Sums are fp64 in a fixed order (no atomics): bit-reproducible; the reference reduces in float32.
 */
long bts_eval_ws_doubles(int B, int Hg, int Wg);
int bts_eval_depth_metrics_f32(const float* pred, int B, int Hp, int Wp, const float* gt, int Hg, int Wg,
                               int top, int left, float min_depth_eval, float max_depth_eval,
                               int y0, int y1, int x0, int x1, double* ws, long ws_doubles,
                               double* per_frame, double* accum, bts_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Training losses: silog_loss.forward (pytorch/bts.py:41-48) and depth_l1_loss.forward
 * (pytorch/bts.py:50-63) on the valid pixels of the whole batch, as the training step uses them
 * (pytorch/bts_main.py:551-565), and their gradient w.r.t. the estimate.  No boolean gather: nothing waits for the host
 * and no shape depends on the data.
 *
 *   est, gt  : [npix] fp32, npix = B*H*W, any 4-byte aligned address (16 bytes per lane are loaded where est, gt and mask
 *              share their offset to a 16-byte / 4-byte boundary, one element per lane otherwise)
 *   mask     : [npix] bytes, valid where != 0 (torch.bool or uint8), or NULL: valid where gt > gt_min (bts_main.py:551-553:
 *              1.0 for KITTI, 0.1 for NYU).  est / gt at invalid pixels are never used (0, negative, inf, NaN are fine).
 *   kind     : 0 = silog, d = log est - log gt, loss = 10 sqrt(E[d^2] - param E[d]^2), param = variance_focus;
 *              1 = L1, e = est - gt, loss = E[e > 0 ? param e : -e] (E|e| when param == 1), param = inbalance_to_closer.
 *   ws       : scratch of the size query's answer, in doubles (8-byte aligned)
 *   stats    : [4] doubles <- valid count n, E[d], E[d^2] (0, 0 for L1), loss; the backward call reads them
 *   loss     : one fp32 <- the loss
 *   grad_loss: one fp32 ON THE DEVICE, the upstream gradient;  grad_est : [npix] fp32 <- d loss / d est, 0 at invalid pixels
 * Sums are fp64 in a fixed order (no atomics, block count a function of npix): bit-reproducible; rounded to fp32 once.
 * Deliberate deviations (torch gives NaN / inf): n == 0 -> loss 0, gradient 0;  silog with E[d^2] - param E[d]^2 <= 0 ->
 * loss 0, gradient 0.  A NaN or non-positive est at a VALID pixel propagates as IEEE log does, as in torch.
 * All argument checks (BTS_ERR_INVALID: null required pointer, npix <= 0, kind outside {0,1}, ws_doubles below the
 * query, ws / stats not 8-byte aligned, est / gt / grad_est / loss / grad_loss not 4-byte aligned) come before any HIP call.
 */
long bts_depth_loss_ws_doubles(long npix);
int bts_depth_loss_fwd_f32(const float* est, const float* gt, const unsigned char* mask /*NULL: gt > gt_min*/,
                           float gt_min, long npix, int kind, float param /*variance_focus | inbalance_to_closer*/,
                           double* ws, long ws_doubles, double* stats /*[4]: n, mean d, mean d^2 (0,0 for L1), loss*/,
                           float* loss, bts_stream_t stream);
int bts_depth_loss_bwd_f32(const float* est, const float* gt, const unsigned char* mask, float gt_min, long npix,
                           int kind, float param, const double* stats, const float* grad_loss, float* grad_est,
                           bts_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * AdamW for the training step in ONE launch over every parameter (torch.optim.AdamW with amsgrad=False, maximize=False;
 * the reference's optimiser, pytorch/bts_main.py:354-356, 606), which also writes the updated convolution weights out in
 * the layouts of bts_pack_weights_f32 while they are on the chip.
 *
 *   p <- p * (1 - lr*wd);  m <- m + (g - m) * (1 - beta1);  v <- beta2 * v + (1 - beta2) * g * g;
 *   p <- p - step_size * m / (sqrt(v) * inv_sqrt_bc2 + eps),   step_size = lr / (1 - beta1^step),
 *   inv_sqrt_bc2 = 1 / sqrt(1 - beta2^step)
 * in fp32 with IEEE sqrt and division (m and v each end in one fused multiply-add, nothing else is contracted); step_size, inv_sqrt_bc2 and the factors
 * (1 - lr*wd), (1 - beta1), (1 - beta2) are computed in double on the host by the launch call and rounded once.  The
 * update is elementwise: its bits do not depend on the launch shape.
 *
 * An item is one parameter: p, g (gradient), m (exp_avg), v (exp_avg_sq), `numel` contiguous floats each, 4-byte aligned,
 * and the index of its hyper-parameter record (< 8).  n_packs == 0: a FLAT record (c_out, c_in, ksize may all be 0; when
 * given they must multiply to numel); 16 bytes per lane where p, g, m, v share their offset to a 16-byte line.
 * n_packs 1 or 2: a TILE record -- a dense OIHW weight [c_out][c_in][k][k], k in {1, 3} -- whose new values are also
 * written to each pack destination as dst[row*k_pad + tap*c_in_ld + c]:
 *   mode 0 (forward)        : row = c_out index, c = c_in index,  tap as stored,        c_in_ld >= c_in
 *   mode 1 (input gradient) : row = c_in index,  c = c_out index, tap = k*k-1 - stored, c_in_ld >= c_out
 * k_pad >= k*k*c_in_ld, dst 16-byte aligned.  Only the real elements are written: the padding of a destination (rows
 * beyond the real ones, c >= inner, columns >= k*k*c_in_ld) is never touched.
 *
 *   bts_adamw_table_bytes(n)  bytes of the table for n items (host and device copy have the same size; 8-byte aligned
 *                             records, the device copy 16-byte aligned)
 *   bts_adamw_flat_span()     floats of a flat record that one workgroup covers
 *   bts_adamw_plan_f32(...)   host only, no device needed: validates the items and fills `table_host`; *total_blocks is
 *                             the grid; plan (may be NULL) receives kind (0 flat, 1 tile), first_block (the prefix sum of
 *                             n_blocks) and n_blocks per item.  kind and the block counts are a function of the shapes and
 *                             n_packs only, never of the pointers.  BTS_ERR_INVALID: a null pointer, numel <= 0,
 *                             c_out*c_in*k*k != numel, ksize outside {1, 3} together with packs, more than 2 packs, a pack
 *                             with c_in_ld < inner or k_pad < k*k*c_in_ld or a mode outside {0, 1}, a destination not
 *                             16-byte aligned, p / g / m / v not 4-byte aligned, a hyper index outside [0, 8), more than
 *                             2^31 - 1 blocks.  n = 0 is valid (total_blocks = 0).
 *   bts_adamw_step_f32(...)   the launch.  `hyper`: n_hyper <= 8 HOST records, passed to the kernel by value.  `skip`:
 *                             optional DEVICE scalar; non-zero or NaN leaves every byte of every buffer untouched (a
 *                             non-finite loss skips the step without a host read).  Allocates nothing, synchronises
 *                             nothing, hipGraph-capturable.  n = 0 launches nothing.  Overlapping items are a caller error.
 */
typedef struct bts_adamw_pack {
    float* dst;
    long   k_pad;
    int    c_in_ld;
    int    mode;             /* 0 = forward layout, 1 = input-gradient layout */
} bts_adamw_pack;

typedef struct bts_adamw_item {
    float* p; const float* g; float* m; float* v;
    long   numel;
    int    hyper;
    int    c_out, c_in, ksize;
    int    n_packs, reserved;
    bts_adamw_pack packs[2];
} bts_adamw_item;

typedef struct bts_adamw_hyper { double lr, beta1, beta2, eps, weight_decay, step; } bts_adamw_hyper;

typedef struct bts_adamw_plan_item { int kind, reserved; long first_block, n_blocks; } bts_adamw_plan_item;

long bts_adamw_table_bytes(int n);
long bts_adamw_flat_span(void);
int  bts_adamw_plan_f32(const bts_adamw_item* items, int n, void* table_host, long* total_blocks,
                        bts_adamw_plan_item* plan /* [n] or NULL */);
int  bts_adamw_step_f32(const void* table_dev, int n, long total_blocks, const bts_adamw_hyper* hyper, int n_hyper,
                        const float* skip, bts_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * One-call execution of a recorded forward ("plan").  A BtsModel forward is a fixed sequence of ~120 (B=1) to ~460
 * (B=16, four sub-batches) launches of the entry points above with arguments that depend only on the input shape:
 * workspaces, packed weights and dims are fixed per shape, only the caller's input / output tensors move.  The host
 * records that sequence once per shape as an array of `bts_op` records -- bts_amd/plan.py -- and replays it with ONE call per stream:
 * the reference's inference loop is batch 1, eager (pytorch/bts_test.py:127-147), where the per-launch host path is
 * what bounds the frame rate.
 *
 *   ops      : the recorded calls, in order; each holds the argument list of its entry point (stream excluded)
 *   patches  : pointer fields that refer to per-call tensors: field := slots[slot] + delta (bytes), applied IN PLACE
 *              to `ops` before the launches (idempotent; a plan must not be replayed by two threads at once)
 *   slots    : base device pointers of this call's tensors (image, focal, the six outputs, abs_min scalars ...)
 * Returns the first non-zero code of an entry point (the remaining ops are not enqueued), 0 otherwise.
 */
enum { BTS_OP_CONV = 1, BTS_OP_REDUC = 2, BTS_OP_REDUC_LPG = 3, BTS_OP_LPG_FUSED = 4, BTS_OP_NCHW_TO_NHWC = 5,
       BTS_OP_NHWC_TO_NCHW = 6, BTS_OP_MAXPOOL = 7, BTS_OP_BN_RELU_AVGPOOL = 8, BTS_OP_GET_DEPTH = 9, BTS_OP_LPG = 10,
       BTS_OP_UPCONV_COMBINE = 11, BTS_OP_UPCONV_UP9 = 12, BTS_OP_CONV_TAIL_BF16 = 13,
       BTS_OP_CONV_TAIL_WINO = 14 };

typedef struct bts_op {
    int kind;          /* BTS_OP_*                                                              */
    int failed_code;   /* out: the entry point's return code when it was the one that failed   */
    union {
        bts_conv_desc conv;
        struct { const float* x; long x_pix_stride; long npix; int c_in, c_first_out; const float* w_frag; long w_frag_floats;
                 float max_depth; int is_final, normalize; float* out; } reduc;
        struct { const float* x; long x_pix_stride; int B, h, w, c_in, c_first_out; const float* w_frag; long w_frag_floats;
                 float max_depth; int upratio; float* plane4; float* depth_scaled; float* ds_out; float* abs_min; } reduc_lpg;
        struct { const float* plane4; int B, h, w, upratio, normalize; float max_depth; float* depth_scaled; float* ds_out;
                 int ds_factor; long ds_pix_stride; float* abs_min; } lpg_fused;
        struct { const float* plane_eq; int B, h, w, upratio; float* depth; float* abs_min; } lpg;
        struct { const float* src; int B, C; long HW; float* dst; long dst_pix_stride; int relu; } nchw_to_nhwc;
        struct { const float* src; long src_pix_stride; int B, C; long HW; float* dst; } nhwc_to_nchw;
        struct { const float* src; long src_pix_stride; int B, h, w, C; float* dst; long dst_pix_stride; float* dst2;
                 long dst2_pix_stride; } maxpool;
        struct { const float* src; long src_pix_stride; int B, h, w, C; const float* scale; const float* shift; float* dst;
                 long dst_pix_stride; } avgpool;
        struct { const float* iconv1; const float* w; int B, C, H, W; float max_depth; const float* focal;
                 float* final_depth; } get_depth;
        struct { const float* taps; long taps_pix_stride; int B, h, w, c; const float* e2_scale; const float* e2_shift; int act;
                 float* y; long y_pix_stride; } upconv_combine;
        struct { const float* x; long x_pix_stride; int B, h, w, c_in; const float* u; int c_out; const float* e2_scale;
                 const float* e2_shift; int act; float* y; long y_pix_stride; } upconv_up9;
        struct { const float* x; long x_pix_stride; int B, h, w, c_main; const void* w_main; const float* w_tail;
                 const float* tail_plane; int n_tail, c_out, c_out_pad; const float* e2_scale; const float* e2_shift; int act;
                 float* y; long y_pix_stride; } conv_tail_bf16;
        struct { const float* x; long x_pix_stride; int B, h, w, c_main; const float* u; const float* w_tail; const float* tail0;
                 const float* tail1; const float* tail2; const float* tail3; int n_tail, c_out, act; float* y; } conv_tail_wino;
    } u;
} bts_op;

typedef struct bts_plan_patch { int op; int field_offset; int slot; int reserved; long delta; } bts_plan_patch;

int bts_plan_run(bts_op* ops, int n_ops, const bts_plan_patch* patches, int n_patches, void* const* slots, int n_slots,
                 bts_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* BTS_HIP_H_ */
