// torch operator boundary over the C ABI of libbts_hip.so (include/bts_hip.h) -- `TORCH_LIBRARY(bts_hip, ...)`.
//
// The reference's own native side registers its hot op with the framework it runs under:
// tensorflow/custom_layer/local_planar_guidance.cc:31-72 (REGISTER_OP "LocalPlanarGuidance" + shape function),
// :116-156 (the OpKernel: validates `upratio`, allocates the output, hands raw pointers + dims to the functor) and
// :234-239 (the gradient op).  This file is the same layer for PyTorch-ROCm: every operator
//   * checks device / dtype / shape / contiguity / alignment with TORCH_CHECK (the C ABI itself only returns codes),
//   * sets a c10::hip device guard for the tensors' device and launches on the CURRENT HIP stream,
//   * hands raw device pointers and dims to the extern "C" entry point -- no torch type crosses that line.
// Built with g++ only (no device code): `make -C bts_amd/csrc torch` -> bts_amd/libbts_torch.so, loaded by
// bts_amd/_lib.py with torch.ops.load_library.  Autograd for `bts_hip::lpg` is registered in bts_amd/ops.py
// (torch.library.register_autograd) on top of `bts_hip::lpg_backward`, for `bts_hip::depth_loss` on top of
// `bts_hip::depth_loss_backward`, and for `bts_hip::reduc_lpg_train` / `reduction_1x1_train` on top of `bts_hip::reduc_bwd`.
#include <ATen/ATen.h>
#include <ATen/hip/impl/HIPGuardImplMasqueradingAsCUDA.h>      // PyTorch-ROCm tensors carry the device type "cuda": its guard / stream
#include <ATen/hip/impl/HIPStreamMasqueradingAsCUDA.h>         // accessors are the *MasqueradingAsCUDA forms
#include <torch/library.h>

#include <cstdint>
#include <tuple>
#include <vector>

#include "../../include/bts_hip.h"

namespace {

using at::Tensor;
using OptTensor = c10::optional<Tensor>;

const char* err_text(int rc) { return bts_hip_error_string(rc); }

void need_f32_cuda(const Tensor& t, const char* op, const char* what) {
    TORCH_CHECK(t.is_cuda(), op, ": ", what, " must be a CUDA(ROCm) tensor (no CPU fallback)");
    TORCH_CHECK(t.scalar_type() == at::kFloat, op, ": ", what, " must be float32, got ", t.scalar_type());
}

void same_device(const Tensor& a, const Tensor& b, const char* op, const char* what) {
    TORCH_CHECK(a.device() == b.device(), op, ": ", what, " lives on ", b.device(), ", expected ", a.device());
}

// [rows, C] view of an NHWC buffer: unit channel stride, any row stride that is a multiple of 4 floats, 16-byte aligned
long rows2d_stride(const Tensor& t, const char* op, const char* what) {
    need_f32_cuda(t, op, what);
    TORCH_CHECK(t.dim() == 2 && t.stride(1) == 1, op, ": ", what, " must be a 2-D view with unit channel stride");
    const long s = t.size(0) > 1 ? t.stride(0) : t.size(1);
    TORCH_CHECK(s % 4 == 0 && (reinterpret_cast<uintptr_t>(t.data_ptr()) & 15) == 0, op, ": ", what,
                " must have a pixel stride that is a multiple of 4 floats and a 16-byte aligned base");
    return s;
}

float* opt_ptr(const OptTensor& t) { return t.has_value() && t->defined() ? t->data_ptr<float>() : nullptr; }

bts_stream_t current_stream() { return (bts_stream_t)c10::hip::getCurrentHIPStreamMasqueradingAsCUDA().stream(); }

void check_rc(int rc, const char* op) { TORCH_CHECK(rc == 0, op, " failed: ", err_text(rc), " (code ", rc, ")"); }

// ---------------------------------------------------------------------------------------------- local_planar_guidance
// pytorch/bts.py:138-173; returns (depth [B, h*k, w*k], abs_min 0-d).  Bit-exact module-level op (csrc/lpg.hip).
std::tuple<Tensor, Tensor> lpg(const Tensor& plane_eq, int64_t upratio) {
    need_f32_cuda(plane_eq, "bts_hip::lpg", "plane_eq");
    TORCH_CHECK(plane_eq.dim() == 4 && plane_eq.size(1) == 4, "bts_hip::lpg: plane_eq must be [B,4,h,w], got ", plane_eq.sizes());
    TORCH_CHECK(upratio == 1 || upratio == 2 || upratio == 4 || upratio == 8,
                "bts_hip::lpg: upratio must be 1, 2, 4 or 8 (local_planar_guidance.cc:36-44 rejects the rest), got ", upratio);
    c10::hip::HIPGuardMasqueradingAsCUDA guard(plane_eq.device());
    const Tensor pe = plane_eq.contiguous();
    const int B = (int)pe.size(0), h = (int)pe.size(2), w = (int)pe.size(3), k = (int)upratio;
    Tensor depth = at::empty({B, h * k, w * k}, pe.options());
    Tensor abs_min = at::empty({}, pe.options());
    check_rc(bts_lpg_fwd_f32(pe.data_ptr<float>(), B, h, w, k, depth.data_ptr<float>(), abs_min.data_ptr<float>(), current_stream()),
             "bts_hip::lpg");
    return {depth, abs_min};
}

// gradient w.r.t. plane_eq (autograd of bts.py:149-173 incl. the clamp mask; native statement: local_planar_guidance.cu:95-150)
Tensor lpg_backward(const Tensor& plane_eq, const Tensor& grad_depth, int64_t upratio) {
    need_f32_cuda(plane_eq, "bts_hip::lpg_backward", "plane_eq");
    need_f32_cuda(grad_depth, "bts_hip::lpg_backward", "grad_depth");
    same_device(plane_eq, grad_depth, "bts_hip::lpg_backward", "grad_depth");
    TORCH_CHECK(plane_eq.dim() == 4 && plane_eq.size(1) == 4, "bts_hip::lpg_backward: plane_eq must be [B,4,h,w]");
    const int B = (int)plane_eq.size(0), h = (int)plane_eq.size(2), w = (int)plane_eq.size(3), k = (int)upratio;
    TORCH_CHECK(grad_depth.numel() == (int64_t)B * h * k * w * k, "bts_hip::lpg_backward: grad_depth must have B*h*k*w*k elements");
    c10::hip::HIPGuardMasqueradingAsCUDA guard(plane_eq.device());
    const Tensor pe = plane_eq.contiguous(), gd = grad_depth.contiguous();
    Tensor g = at::empty_like(pe);
    check_rc(bts_lpg_bwd_f32(pe.data_ptr<float>(), gd.data_ptr<float>(), B, h, w, k, g.data_ptr<float>(), current_stream()),
             "bts_hip::lpg_backward");
    return g;
}

// ------------------------------------------------------------------------------------------------------ reduction_1x1
// pytorch/bts.py:97-136, the whole chain in one launch; x2d: NHWC [npix, >= c_in] view; out: [npix*4] (or [npix] when final)
void reduction_1x1(const Tensor& x2d, int64_t c_in, int64_t c_first_out, const Tensor& w_frag, double max_depth, bool is_final,
                   bool normalize, Tensor out) {
    const long xs = rows2d_stride(x2d, "bts_hip::reduction_1x1", "x2d");
    need_f32_cuda(w_frag, "bts_hip::reduction_1x1", "w_frag");
    need_f32_cuda(out, "bts_hip::reduction_1x1", "out");
    same_device(x2d, w_frag, "bts_hip::reduction_1x1", "w_frag");
    same_device(x2d, out, "bts_hip::reduction_1x1", "out");
    TORCH_CHECK(x2d.size(1) >= c_in, "bts_hip::reduction_1x1: x2d has ", x2d.size(1), " channels, the chain reads ", c_in);
    TORCH_CHECK(w_frag.is_contiguous() && out.is_contiguous(), "bts_hip::reduction_1x1: w_frag and out must be contiguous");
    const int64_t npix = x2d.size(0);
    TORCH_CHECK(out.numel() == npix * (is_final ? 1 : 4), "bts_hip::reduction_1x1: out must hold ", npix * (is_final ? 1 : 4), " floats");
    TORCH_CHECK(max_depth > 0, "bts_hip::reduction_1x1: max_depth must be positive");
    c10::hip::HIPGuardMasqueradingAsCUDA guard(x2d.device());
    check_rc(bts_reduc_fwd_f32(x2d.data_ptr<float>(), xs, npix, (int)c_in, (int)c_first_out, w_frag.data_ptr<float>(), w_frag.numel(),
                               (float)max_depth, is_final ? 1 : 0, normalize ? 1 : 0, out.data_ptr<float>(), current_stream()),
             "bts_hip::reduction_1x1");
}

// reduction_1x1 -> F.normalize -> LPG -> /max_depth (+ nearest-downsampled plane, abs_min): bts.py:249-256 / 263-270 / 277-283
void reduc_lpg(const Tensor& x2d, int64_t B, int64_t h, int64_t w, int64_t c_in, int64_t c_first_out, const Tensor& w_frag,
               double max_depth, int64_t upratio, Tensor depth_scaled, OptTensor ds_out, OptTensor abs_min, OptTensor plane4) {
    const long xs = rows2d_stride(x2d, "bts_hip::reduc_lpg", "x2d");
    need_f32_cuda(w_frag, "bts_hip::reduc_lpg", "w_frag");
    need_f32_cuda(depth_scaled, "bts_hip::reduc_lpg", "depth_scaled");
    same_device(x2d, w_frag, "bts_hip::reduc_lpg", "w_frag");
    same_device(x2d, depth_scaled, "bts_hip::reduc_lpg", "depth_scaled");
    const int64_t npix = B * h * w, k = upratio;
    TORCH_CHECK(B > 0 && h > 0 && w > 0 && x2d.size(0) == npix && x2d.size(1) >= c_in, "bts_hip::reduc_lpg: x2d ", x2d.sizes(),
                " does not match B=", B, " ", h, "x", w, " with ", c_in, " channels");
    TORCH_CHECK(depth_scaled.is_contiguous() && depth_scaled.numel() == npix * k * k, "bts_hip::reduc_lpg: depth_scaled must be contiguous [B,1,h*k,w*k]");
    for (const OptTensor* t : {&ds_out, &abs_min, &plane4})
        if (t->has_value() && (*t)->defined()) {
            need_f32_cuda(**t, "bts_hip::reduc_lpg", "optional output");
            same_device(x2d, **t, "bts_hip::reduc_lpg", "optional output");
            TORCH_CHECK((*t)->is_contiguous(), "bts_hip::reduc_lpg: optional outputs must be contiguous");
        }
    if (ds_out.has_value() && ds_out->defined()) TORCH_CHECK(k != 2 && ds_out->numel() == npix * 4, "bts_hip::reduc_lpg: ds_out must be a [B,2h,2w] plane (k = 8 or 4)");
    if (plane4.has_value() && plane4->defined()) TORCH_CHECK(plane4->numel() == npix * 4, "bts_hip::reduc_lpg: plane4 must be [B*h*w,4]");
    if (abs_min.has_value() && abs_min->defined()) TORCH_CHECK(abs_min->numel() == 1, "bts_hip::reduc_lpg: abs_min must hold one float");
    c10::hip::HIPGuardMasqueradingAsCUDA guard(x2d.device());
    check_rc(bts_reduc_lpg_fwd_f32(x2d.data_ptr<float>(), xs, (int)B, (int)h, (int)w, (int)c_in, (int)c_first_out, w_frag.data_ptr<float>(),
                                   w_frag.numel(), (float)max_depth, (int)k, opt_ptr(plane4), depth_scaled.data_ptr<float>(), opt_ptr(ds_out),
                                   opt_ptr(abs_min), current_stream()),
             "bts_hip::reduc_lpg");
}

// ---------------------------------------------------------------------------------------------- reduction, training
// Backward-data of one reduction scale (csrc/reduc_bwd.hip): fills Y, and G / dx when given.  upratio 0 = the final chain.
void reduc_bwd(const Tensor& x2d, int64_t B, int64_t h, int64_t w, int64_t c_in, int64_t c_first_out, const Tensor& w_frag,
               const Tensor& wt_frag, double max_depth, int64_t upratio, const Tensor& grad_out, OptTensor dx, OptTensor G, Tensor Y) {
    const char* op = "bts_hip::reduc_bwd";
    const long xs = rows2d_stride(x2d, op, "x2d");
    const int64_t npix = B * h * w, kk = upratio > 0 ? upratio * upratio : 1;
    TORCH_CHECK(B > 0 && h > 0 && w > 0 && x2d.size(0) == npix && x2d.size(1) >= c_in, op, ": x2d ", x2d.sizes(), " does not match B=", B, " ", h,
                "x", w, " with ", c_in, " channels");
    for (const Tensor* t : {&w_frag, &wt_frag, &grad_out, (const Tensor*)&Y}) {
        need_f32_cuda(*t, op, "tensor argument");
        same_device(x2d, *t, op, "tensor argument");
        TORCH_CHECK(t->is_contiguous(), op, ": w_frag, wt_frag, grad_out and Y must be contiguous");
    }
    TORCH_CHECK(grad_out.numel() == npix * kk, op, ": grad_out must hold ", npix * kk, " floats");
    TORCH_CHECK(Y.dim() == 2 && Y.size(0) == npix, op, ": Y must be [npix, YC]");
    const int64_t yc = Y.size(1);
    float* gp = nullptr;
    if (G.has_value() && G->defined()) {
        need_f32_cuda(*G, op, "G");
        same_device(x2d, *G, op, "G");
        TORCH_CHECK(G->is_contiguous() && G->dim() == 2 && G->size(0) == npix && G->size(1) == yc + 4, op, ": G must be contiguous [npix, YC + 4]");
        gp = G->data_ptr<float>();
    }
    float* dxp = nullptr;
    long dxs = 0;
    if (dx.has_value() && dx->defined()) {
        dxs = rows2d_stride(*dx, op, "dx");
        same_device(x2d, *dx, op, "dx");
        TORCH_CHECK(dx->size(0) == npix && dx->size(1) >= c_in, op, ": dx must be a [npix, >= c_in] view");
        dxp = dx->data_ptr<float>();
    }
    // the kernel addresses Y by the chain's own column count: refuse a buffer of another width before it runs
    int64_t want = 0;
    for (int64_t m = c_first_out; m >= 8; m /= 2) want += m;
    TORCH_CHECK(yc == want, op, ": Y has ", yc, " columns, the chain (", c_in, ",", c_first_out, ") writes ", want);
    c10::hip::HIPGuardMasqueradingAsCUDA guard(x2d.device());
    check_rc(bts_reduc_bwd_f32(x2d.data_ptr<float>(), xs, (int)B, (int)h, (int)w, (int)c_in, (int)c_first_out, w_frag.data_ptr<float>(),
                               w_frag.numel(), wt_frag.data_ptr<float>(), wt_frag.numel(), (float)max_depth, (int)upratio,
                               grad_out.data_ptr<float>(), dxp, dxs, gp, Y.data_ptr<float>(), current_stream()), op);
}

void train_args(const char* op, const Tensor& x2d, const std::vector<Tensor>& weights, const std::vector<Tensor>& packs) {
    TORCH_CHECK(!weights.empty() && weights[0].dim() == 4, op, ": weights must be the chain's [cout,cin,1,1] tensors");
    TORCH_CHECK(packs.size() == 3, op, ": packs must be ops.reduc_train_packs(weights): (w_frag, w_frag_wide, wt_frag)");
    for (const Tensor& t : packs) { need_f32_cuda(t, op, "pack"); same_device(x2d, t, op, "pack"); }
}

// Out-of-place forms of reduc_lpg / reduction_1x1 for training callers: fresh outputs, and autograd registered in
// bts_amd/ops.py on top of bts_hip::reduc_bwd.  `weights` are there to be differentiated; the kernels read `packs`.
std::tuple<Tensor, Tensor> reduc_lpg_train(const Tensor& x2d, int64_t B, int64_t h, int64_t w, std::vector<Tensor> weights,
                                           std::vector<Tensor> packs, double max_depth, int64_t upratio) {
    train_args("bts_hip::reduc_lpg_train", x2d, weights, packs);
    need_f32_cuda(x2d, "bts_hip::reduc_lpg_train", "x2d");
    TORCH_CHECK(upratio == 8 || upratio == 4 || upratio == 2, "bts_hip::reduc_lpg_train: upratio must be 8, 4 or 2, got ", upratio);
    c10::hip::HIPGuardMasqueradingAsCUDA guard(x2d.device());
    Tensor depth = at::empty({B, 1, h * upratio, w * upratio}, x2d.options());
    Tensor abs_min = at::empty({}, x2d.options());
    reduc_lpg(x2d, B, h, w, weights[0].size(1), weights[0].size(0), packs[0], max_depth, upratio, depth, OptTensor(), abs_min, OptTensor());
    return {depth, abs_min};
}

Tensor reduction_1x1_train(const Tensor& x2d, int64_t B, int64_t h, int64_t w, std::vector<Tensor> weights, std::vector<Tensor> packs,
                           double max_depth) {
    train_args("bts_hip::reduction_1x1_train", x2d, weights, packs);
    need_f32_cuda(x2d, "bts_hip::reduction_1x1_train", "x2d");
    TORCH_CHECK(B > 0 && h > 0 && w > 0 && x2d.dim() == 2 && x2d.size(0) == B * h * w, "bts_hip::reduction_1x1_train: x2d must have B*h*w rows");
    c10::hip::HIPGuardMasqueradingAsCUDA guard(x2d.device());
    Tensor out = at::empty({B, 1, h, w}, x2d.options());
    reduction_1x1(x2d, weights[0].size(1), weights[0].size(0), packs[0], max_depth, /*is_final=*/true, /*normalize=*/false, out);
    return out;
}

// ------------------------------------------------------------------------------------------------------------- conv
// One fused convolution = one bts_conv_desc (include/bts_hip.h): atrous_conv's 1x1 and dilated 3x3 (bts.py:65-80), upconv
// (bts.py:83-94), conv5..conv1, daspp_conv.  geom = {x_pix_stride, c_in_ld, k_pad, B, h_in, w_in, up, ksize, dil, stride, pad,
// c_out, c_out_pad, pre_relu, act, y_pix_stride, y_nchw, subpixel, y2_pix_stride, res_pix_stride, n_bundles, precision,
// fill_frames}.
constexpr int kGeomLen = 23;

void conv_fwd(const Tensor& x, const Tensor& w, OptTensor pre_scale, OptTensor pre_shift, OptTensor e1_scale, OptTensor e1_shift,
              OptTensor e2_scale, OptTensor e2_shift, Tensor y, OptTensor y2, OptTensor res, OptTensor splitk_ws,
              std::vector<Tensor> tail_planes, OptTensor w_split, OptTensor w_wino, std::vector<int64_t> geom) {
    const char* op = "bts_hip::conv_fwd";
    TORCH_CHECK((int)geom.size() == kGeomLen, op, ": geom must hold ", kGeomLen, " integers, got ", geom.size());
    need_f32_cuda(x, op, "x");
    need_f32_cuda(w, op, "w");
    need_f32_cuda(y, op, "y");
    same_device(x, w, op, "w");
    same_device(x, y, op, "y");
    TORCH_CHECK(w.is_contiguous(), op, ": packed weights must be contiguous");
    bts_conv_desc d{};
    int i = 0;
    d.x_pix_stride = geom[i++]; d.c_in_ld = (int)geom[i++]; d.k_pad = (int)geom[i++];
    d.B = (int)geom[i++]; d.h_in = (int)geom[i++]; d.w_in = (int)geom[i++]; d.up = (int)geom[i++];
    d.ksize = (int)geom[i++]; d.dil = (int)geom[i++]; d.stride = (int)geom[i++]; d.pad = (int)geom[i++];
    d.c_out = (int)geom[i++]; d.c_out_pad = (int)geom[i++]; d.pre_relu = (int)geom[i++]; d.act = (int)geom[i++];
    d.y_pix_stride = geom[i++]; d.y_nchw = (int)geom[i++]; d.subpixel = (int)geom[i++]; d.y2_pix_stride = geom[i++];
    d.res_pix_stride = geom[i++]; d.n_bundles = (int)geom[i++]; d.precision = (int)geom[i++]; d.fill_frames = (int)geom[i++];
    TORCH_CHECK(d.B > 0 && d.h_in > 0 && d.w_in > 0 && d.c_in_ld > 0 && d.c_out > 0 && d.x_pix_stride > 0, op, ": non-positive dimension");
    const int nb = d.n_bundles > 1 ? d.n_bundles : 1;
    // the input view must cover the last pixel's channels; the weights the packed [classes][c_out_pad][k_pad] block
    const int64_t in_pix = (int64_t)d.B * d.h_in * d.w_in;
    const int64_t x_need = (in_pix - 1) * d.x_pix_stride + (int64_t)(d.c_in_ld - ((int)tail_planes.size() > 0 ? 4 : 0)) * nb;
    TORCH_CHECK(x.dim() >= 1 && x.stride(-1) == 1, op, ": x must have unit channel stride");
    TORCH_CHECK((int64_t)x.numel() > 0 && x_need <= (int64_t)(x.storage().nbytes() / 4 - x.storage_offset()), op, ": x (", x.sizes(),
                ") is smaller than B*h_in*w_in pixels of ", d.c_in_ld, " channels at pixel stride ", d.x_pix_stride);
    const int64_t classes = d.subpixel ? 4 : nb;
    TORCH_CHECK(w.numel() == classes * (int64_t)d.c_out_pad * d.k_pad, op, ": packed weights hold ", w.numel(), " floats, expected ",
                classes * (int64_t)d.c_out_pad * d.k_pad, " ([classes][c_out_pad][k_pad])");
    d.x = x.data_ptr<float>();
    d.w = w.data_ptr<float>();
    auto vec = [&](const OptTensor& t, int64_t n, const char* what) -> const float* {
        if (!(t.has_value() && t->defined())) return nullptr;
        need_f32_cuda(*t, op, what);
        same_device(x, *t, op, what);
        TORCH_CHECK(t->is_contiguous() && t->numel() == n, op, ": ", what, " must be a contiguous vector of ", n, " floats, got ", t->sizes());
        return t->data_ptr<float>();
    };
    d.pre_scale = vec(pre_scale, (int64_t)d.c_in_ld * nb, "pre_scale");
    d.pre_shift = vec(pre_shift, (int64_t)d.c_in_ld * nb, "pre_shift");
    d.e1_scale = vec(e1_scale, (int64_t)d.c_out_pad * nb, "e1_scale");
    d.e1_shift = vec(e1_shift, (int64_t)d.c_out_pad * nb, "e1_shift");
    d.e2_scale = vec(e2_scale, (int64_t)d.c_out_pad * nb, "e2_scale");
    d.e2_shift = vec(e2_shift, (int64_t)d.c_out_pad * nb, "e2_shift");
    // output extent: the library computes H, W from the geometry; mirror it for the bounds check
    const int Hs = d.h_in * d.up, Ws = d.w_in * d.up;
    int H = (Hs + 2 * d.pad - d.dil * (d.ksize - 1) - 1) / (d.stride > 0 ? d.stride : 1) + 1;
    int W = (Ws + 2 * d.pad - d.dil * (d.ksize - 1) - 1) / (d.stride > 0 ? d.stride : 1) + 1;
    if (d.subpixel) { H = 2 * d.h_in; W = 2 * d.w_in; }
    TORCH_CHECK(H > 0 && W > 0, op, ": empty output");
    const int64_t out_pix = (int64_t)d.B * H * W;
    auto out_check = [&](const Tensor& t, int64_t pix_stride, bool nchw, const char* what) {
        const int64_t have = (int64_t)(t.storage().nbytes() / 4) - t.storage_offset();
        const int64_t need = nchw ? out_pix * d.c_out : (out_pix - 1) * pix_stride + (int64_t)d.c_out * nb;
        TORCH_CHECK(need <= have, op, ": ", what, " (", t.sizes(), ") is smaller than the ", d.B, "x", H, "x", W, "x", d.c_out * nb, " result");
    };
    out_check(y, d.y_pix_stride, d.y_nchw != 0, "y");
    d.y = y.data_ptr<float>();
    if (y2.has_value() && y2->defined()) { need_f32_cuda(*y2, op, "y2"); same_device(x, *y2, op, "y2"); out_check(*y2, d.y2_pix_stride, false, "y2"); d.y2 = y2->data_ptr<float>(); }
    if (res.has_value() && res->defined()) { need_f32_cuda(*res, op, "res"); same_device(x, *res, op, "res"); out_check(*res, d.res_pix_stride, false, "res"); d.res = res->data_ptr<float>(); }
    if (splitk_ws.has_value() && splitk_ws->defined()) {
        need_f32_cuda(*splitk_ws, op, "splitk_ws");
        same_device(x, *splitk_ws, op, "splitk_ws");
        TORCH_CHECK(splitk_ws->is_contiguous(), op, ": splitk_ws must be contiguous");
        d.splitk_ws = splitk_ws->data_ptr<float>();
        d.splitk_ws_floats = splitk_ws->numel();
    }
    TORCH_CHECK(tail_planes.size() <= 4, op, ": at most 4 tail planes");
    d.n_tail = (int)tail_planes.size();
    for (int j = 0; j < d.n_tail; ++j) {
        need_f32_cuda(tail_planes[j], op, "tail plane");
        same_device(x, tail_planes[j], op, "tail plane");
        TORCH_CHECK(tail_planes[j].is_contiguous() && tail_planes[j].numel() == in_pix, op, ": every tail plane must be a contiguous [B,1,h_in,w_in] map");
        d.tail_planes[j] = tail_planes[j].data_ptr<float>();
    }
    if (w_split.has_value() && w_split->defined()) {
        // precision 1: three truncation planes (ops.split_bf16x3); precision 2: one round-to-nearest-even plane (ops.round_bf16)
        const int64_t planes = d.precision == 2 ? 1 : 3;
        TORCH_CHECK(w_split->is_cuda() && w_split->scalar_type() == at::kShort && w_split->is_contiguous() && w_split->numel() == planes * w.numel(), op,
                    planes == 1 ? ": w_split must be the contiguous int16 [classes][1][c_out_pad][k_pad] bf16 rounding of w (ops.round_bf16)"
                                : ": w_split must be the contiguous int16 [classes][3][c_out_pad][k_pad] split of w (ops.split_bf16x3)");
        same_device(x, *w_split, op, "w_split");
        d.w_split = w_split->data_ptr();
    }
    if (w_wino.has_value() && w_wino->defined()) {
        need_f32_cuda(*w_wino, op, "w_wino");
        same_device(x, *w_wino, op, "w_wino");
        const int64_t cm = d.n_tail > 0 ? d.c_in_ld - 4 : d.c_in_ld;
        TORCH_CHECK(w_wino->is_contiguous() && (w_wino->numel() == (int64_t)16 * d.c_out_pad * cm || w_wino->numel() == (int64_t)16 * d.c_out * cm), op,
                    ": w_wino must be the contiguous Winograd form of w, 16 * c_out_pad * (buffer channels) floats (ops.pack_wino_weight)");
        d.w_wino = w_wino->data_ptr<float>();
    }
    c10::hip::HIPGuardMasqueradingAsCUDA guard(x.device());
    check_rc(bts_conv_fwd_f32(&d, current_stream()), op);
}

// ---------------------------------------------------------------------------------------- upconv, F(2x2,2x2) form
// nearest-2x + conv3x3 + activation + affine (bts.py:90-94) as one launch of the shared-patch F(2x2,2x2) kernel
// (bts_upconv_up9_fwd_f32).  x: [B*h*w, >= c_in] NHWC view; u: ops.pack_upconv_up9 (36 * c_in * c_out floats);
// y: [B*2h*2w, c_out] NHWC view.  geom = {B, h, w, c_in, c_out, act}.
void upconv_up9(const Tensor& x, const Tensor& u, OptTensor e2_scale, OptTensor e2_shift, Tensor y, std::vector<int64_t> geom) {
    const char* op = "bts_hip::upconv_up9";
    TORCH_CHECK(geom.size() == 6, op, ": geom must hold 6 integers, got ", geom.size());
    const int64_t B = geom[0], h = geom[1], w = geom[2], c_in = geom[3], c_out = geom[4], act = geom[5];
    TORCH_CHECK(B > 0 && h > 0 && w > 0 && c_in > 0 && c_out > 0, op, ": non-positive dimension");
    TORCH_CHECK(c_in % 32 == 0 && c_out % 32 == 0, op, ": c_in (", c_in, ") and c_out (", c_out, ") must be multiples of 32");
    const long xs = rows2d_stride(x, op, "x"), ys = rows2d_stride(y, op, "y");
    need_f32_cuda(u, op, "u");
    same_device(x, u, op, "u");
    same_device(x, y, op, "y");
    TORCH_CHECK(x.size(0) == B * h * w && x.size(1) >= c_in, op, ": x (", x.sizes(), ") is not a [B*h*w, >= c_in] view");
    TORCH_CHECK(y.size(0) == 4 * B * h * w && y.size(1) == c_out, op, ": y (", y.sizes(), ") is not a [B*2h*2w, c_out] view");
    TORCH_CHECK(u.is_contiguous() && u.numel() == 36 * c_in * c_out, op, ": u must be the contiguous F(2x2,2x2) form of the weight, ",
                36 * c_in * c_out, " floats (ops.pack_upconv_up9), got ", u.numel());
    auto vec = [&](const OptTensor& t, const char* what) -> const float* {
        if (!(t.has_value() && t->defined())) return nullptr;
        need_f32_cuda(*t, op, what);
        same_device(x, *t, op, what);
        TORCH_CHECK(t->is_contiguous() && t->numel() >= c_out, op, ": ", what, " must be a contiguous vector of at least ", c_out, " floats");
        return t->data_ptr<float>();
    };
    const float* es = vec(e2_scale, "e2_scale");
    const float* eb = vec(e2_shift, "e2_shift");
    TORCH_CHECK((es == nullptr) == (eb == nullptr), op, ": give both e2 vectors or neither");
    c10::hip::HIPGuardMasqueradingAsCUDA guard(x.device());
    check_rc(bts_upconv_up9_fwd_f32(x.data_ptr<float>(), xs, (int)B, (int)h, (int)w, (int)c_in, u.data_ptr<float>(), (int)c_out, es, eb, (int)act,
                                    y.data_ptr<float>(), ys, current_stream()), op);
}

// ------------------------------------------------------------------------------- planar-tail 3x3, bf16 main operands
// conv3x3 over [main channels | one depth plane] + activation + affine as one launch of the bf16 halo tile with an fp32 tail
// (bts_conv_tail_bf16_fwd_f32).  x: [B*h*w, >= c_main] NHWC view; w_main: bf16 [c_out_pad, 9 * c_main]; w_tail: fp32
// [c_out_pad, 9, 4] (ops.pack_conv_tail_bf16); tail: the plane, B*h*w floats; y: [B*h*w, c_out] NHWC view.
// geom = {B, h, w, c_main, c_out, act}.
void conv_tail_bf16(const Tensor& x, const Tensor& w_main, const Tensor& w_tail, const Tensor& tail, OptTensor e2_scale, OptTensor e2_shift,
                    Tensor y, std::vector<int64_t> geom) {
    const char* op = "bts_hip::conv_tail_bf16";
    TORCH_CHECK(geom.size() == 6, op, ": geom must hold 6 integers, got ", geom.size());
    const int64_t B = geom[0], h = geom[1], w = geom[2], c_main = geom[3], c_out = geom[4], act = geom[5];
    TORCH_CHECK(B > 0 && h > 0 && w > 0 && c_main > 0 && c_out > 0, op, ": non-positive dimension");
    TORCH_CHECK(c_main % 32 == 0, op, ": c_main (", c_main, ") must be a multiple of 32");
    const long xs = rows2d_stride(x, op, "x"), ys = rows2d_stride(y, op, "y");
    TORCH_CHECK(w_main.is_cuda(), op, ": w_main must be a CUDA(ROCm) tensor (no CPU fallback)");
    TORCH_CHECK(w_main.scalar_type() == at::kBFloat16, op, ": w_main must be bfloat16, got ", w_main.scalar_type());
    need_f32_cuda(w_tail, op, "w_tail");
    need_f32_cuda(tail, op, "tail");
    same_device(x, w_main, op, "w_main");
    same_device(x, w_tail, op, "w_tail");
    same_device(x, tail, op, "tail");
    same_device(x, y, op, "y");
    TORCH_CHECK(x.size(0) == B * h * w && x.size(1) >= c_main, op, ": x (", x.sizes(), ") is not a [B*h*w, >= c_main] view");
    TORCH_CHECK(y.size(0) == B * h * w && y.size(1) == c_out, op, ": y (", y.sizes(), ") is not a [B*h*w, c_out] view");
    TORCH_CHECK(w_main.is_contiguous() && w_main.dim() == 2 && w_main.size(1) == 9 * c_main && w_main.size(0) >= c_out && w_main.size(0) % 32 == 0,
                op, ": w_main must be contiguous [c_out_pad, 9 * c_main] with c_out_pad a multiple of 32 (ops.pack_conv_tail_bf16), got ", w_main.sizes());
    const int64_t c_out_pad = w_main.size(0);
    TORCH_CHECK(w_tail.is_contiguous() && w_tail.numel() == c_out_pad * 36, op, ": w_tail must be contiguous [c_out_pad, 9, 4], got ", w_tail.sizes());
    TORCH_CHECK(tail.is_contiguous() && tail.numel() == B * h * w, op, ": tail must be one contiguous plane of B*h*w floats (n_tail 1), got ",
                tail.sizes());
    TORCH_CHECK(act >= 0 && act <= 2, op, ": act must be 0 (none), 1 (ReLU) or 2 (ELU), got ", act);
    auto vec = [&](const OptTensor& t, const char* what) -> const float* {
        if (!(t.has_value() && t->defined())) return nullptr;
        need_f32_cuda(*t, op, what);
        same_device(x, *t, op, what);
        TORCH_CHECK(t->is_contiguous() && t->numel() >= c_out, op, ": ", what, " must be a contiguous vector of at least ", c_out, " floats");
        return t->data_ptr<float>();
    };
    const float* es = vec(e2_scale, "e2_scale");
    const float* eb = vec(e2_shift, "e2_shift");
    TORCH_CHECK((es == nullptr) == (eb == nullptr), op, ": give both e2 vectors or neither");
    c10::hip::HIPGuardMasqueradingAsCUDA guard(x.device());
    check_rc(bts_conv_tail_bf16_fwd_f32(x.data_ptr<float>(), xs, (int)B, (int)h, (int)w, (int)c_main, w_main.data_ptr(), w_tail.data_ptr<float>(),
                                        tail.data_ptr<float>(), 1, (int)c_out, (int)c_out_pad, es, eb, (int)act, y.data_ptr<float>(), ys,
                                        current_stream()), op);
}

// ------------------------------------------------------------------------------- wide 1x1, bf16 operands (c_out % 192 == 0)
// act(e1(conv1x1(bf16(pre(x))))) as one launch of the wide bf16 tile (bts_conv1x1_bf16_fwd_f32).  x: [npix, >= c_in] NHWC
// view; w_plane: the one-plane bf16 form of the packed weight, [c_out_pad, k_pad] or [1, c_out_pad, k_pad], int16 bits
// (ops.round_bf16) or bfloat16; y: [npix, c_out] NHWC view.  geom = {npix, c_in, c_out, pre_relu, act}.
void conv1x1_bf16(const Tensor& x, const Tensor& w_plane, OptTensor pre_scale, OptTensor pre_shift, OptTensor e1_scale, OptTensor e1_shift,
                  Tensor y, std::vector<int64_t> geom) {
    const char* op = "bts_hip::conv1x1_bf16";
    TORCH_CHECK(geom.size() == 5, op, ": geom must hold 5 integers, got ", geom.size());
    const int64_t npix = geom[0], c_in = geom[1], c_out = geom[2], pre_relu = geom[3], act = geom[4];
    TORCH_CHECK(npix > 0 && c_in > 0 && c_out > 0, op, ": non-positive dimension");
    TORCH_CHECK(c_in % 16 == 0 && c_out % 192 == 0, op, ": needs c_in % 16 == 0 and c_out % 192 == 0, got ", c_in, " -> ", c_out);
    const long xs = rows2d_stride(x, op, "x"), ys = rows2d_stride(y, op, "y");
    TORCH_CHECK(w_plane.is_cuda(), op, ": w_plane must be a CUDA(ROCm) tensor (no CPU fallback)");
    TORCH_CHECK(w_plane.scalar_type() == at::kShort || w_plane.scalar_type() == at::kBFloat16, op,
                ": w_plane must hold bf16 bits (int16 from ops.round_bf16, or bfloat16), got ", w_plane.scalar_type());
    same_device(x, w_plane, op, "w_plane");
    same_device(x, y, op, "y");
    TORCH_CHECK(x.size(0) == npix && x.size(1) >= c_in, op, ": x (", x.sizes(), ") is not a [npix, >= c_in] view");
    TORCH_CHECK(y.size(0) == npix && y.size(1) == c_out, op, ": y (", y.sizes(), ") is not a [npix, c_out] view");
    const int64_t wd = w_plane.dim();
    TORCH_CHECK(w_plane.is_contiguous() && (wd == 2 || (wd == 3 && w_plane.size(0) == 1)), op,
                ": w_plane must be contiguous [c_out_pad, k_pad] or [1, c_out_pad, k_pad] (ops.round_bf16), got ", w_plane.sizes());
    const int64_t c_out_pad = w_plane.size(wd - 2), k_pad = w_plane.size(wd - 1);
    TORCH_CHECK(c_out_pad >= c_out && k_pad >= c_in && k_pad % 32 == 0, op, ": w_plane ", w_plane.sizes(), " does not hold ", c_out, " rows of ",
                c_in, " channels padded to a multiple of 32");
    TORCH_CHECK(act >= 0 && act <= 2, op, ": act must be 0 (none), 1 (ReLU) or 2 (ELU), got ", act);
    auto vec = [&](const OptTensor& t, const char* what, int64_t n) -> const float* {
        if (!(t.has_value() && t->defined())) return nullptr;
        need_f32_cuda(*t, op, what);
        same_device(x, *t, op, what);
        TORCH_CHECK(t->is_contiguous() && t->numel() >= n, op, ": ", what, " must be a contiguous vector of at least ", n, " floats");
        return t->data_ptr<float>();
    };
    const float* ps = vec(pre_scale, "pre_scale", c_in);
    const float* pb = vec(pre_shift, "pre_shift", c_in);
    const float* es = vec(e1_scale, "e1_scale", c_out);
    const float* eb = vec(e1_shift, "e1_shift", c_out);
    TORCH_CHECK((ps == nullptr) == (pb == nullptr) && (es == nullptr) == (eb == nullptr), op, ": give both vectors of an affine or neither");
    c10::hip::HIPGuardMasqueradingAsCUDA guard(x.device());
    check_rc(bts_conv1x1_bf16_fwd_f32(x.data_ptr<float>(), xs, (long)npix, (int)c_in, w_plane.data_ptr(), (int)k_pad, (int)c_out, (int)c_out_pad,
                                      ps, pb, (int)(pre_relu != 0), es, eb, (int)act, y.data_ptr<float>(), ys, current_stream()), op);
}

// ------------------------------------------------------------------------------- the bf16-resident bottleneck intermediate
// [rows, C] view of a BFLOAT16 NHWC buffer: unit channel stride, a row stride that is a multiple of 4 elements, 8-byte aligned
long rows2d_stride_bf16(const Tensor& t, const char* op, const char* what) {
    TORCH_CHECK(t.is_cuda(), op, ": ", what, " must be a CUDA(ROCm) tensor (no CPU fallback)");
    TORCH_CHECK(t.scalar_type() == at::kBFloat16, op, ": ", what, " must be bfloat16, got ", t.scalar_type());
    TORCH_CHECK(t.dim() == 2 && t.stride(1) == 1, op, ": ", what, " must be a 2-D view with unit channel stride");
    const long s = t.size(0) > 1 ? t.stride(0) : t.size(1);
    TORCH_CHECK(s % 4 == 0 && (reinterpret_cast<uintptr_t>(t.data_ptr()) & 7) == 0, op, ": ", what,
                " must have a pixel stride that is a multiple of 4 elements and an 8-byte aligned base");
    return s;
}

// conv1x1_bf16 above with a bfloat16 destination (bts_conv1x1_bf16_fwd_bf16): y is a [npix, c_out] view of a bf16 NHWC buffer.
// The other operands and geom = {npix, c_in, c_out, pre_relu, act} as conv1x1_bf16.
void conv1x1_bf16_ybf16(const Tensor& x, const Tensor& w_plane, OptTensor pre_scale, OptTensor pre_shift, OptTensor e1_scale,
                        OptTensor e1_shift, Tensor y, std::vector<int64_t> geom) {
    const char* op = "bts_hip::conv1x1_bf16_ybf16";
    TORCH_CHECK(geom.size() == 5, op, ": geom must hold 5 integers, got ", geom.size());
    const int64_t npix = geom[0], c_in = geom[1], c_out = geom[2], pre_relu = geom[3], act = geom[4];
    TORCH_CHECK(npix > 0 && c_in > 0 && c_out > 0, op, ": non-positive dimension");
    TORCH_CHECK(c_in % 16 == 0 && c_out % 192 == 0, op, ": needs c_in % 16 == 0 and c_out % 192 == 0, got ", c_in, " -> ", c_out);
    const long xs = rows2d_stride(x, op, "x"), ys = rows2d_stride_bf16(y, op, "y");
    TORCH_CHECK(w_plane.is_cuda(), op, ": w_plane must be a CUDA(ROCm) tensor (no CPU fallback)");
    TORCH_CHECK(w_plane.scalar_type() == at::kShort || w_plane.scalar_type() == at::kBFloat16, op,
                ": w_plane must hold bf16 bits (int16 from ops.round_bf16, or bfloat16), got ", w_plane.scalar_type());
    same_device(x, w_plane, op, "w_plane");
    same_device(x, y, op, "y");
    TORCH_CHECK(x.size(0) == npix && x.size(1) >= c_in, op, ": x (", x.sizes(), ") is not a [npix, >= c_in] view");
    TORCH_CHECK(y.size(0) == npix && y.size(1) == c_out, op, ": y (", y.sizes(), ") is not a [npix, c_out] view");
    const int64_t wd = w_plane.dim();
    TORCH_CHECK(w_plane.is_contiguous() && (wd == 2 || (wd == 3 && w_plane.size(0) == 1)), op,
                ": w_plane must be contiguous [c_out_pad, k_pad] or [1, c_out_pad, k_pad] (ops.round_bf16), got ", w_plane.sizes());
    const int64_t c_out_pad = w_plane.size(wd - 2), k_pad = w_plane.size(wd - 1);
    TORCH_CHECK(c_out_pad >= c_out && k_pad >= c_in && k_pad % 32 == 0, op, ": w_plane ", w_plane.sizes(), " does not hold ", c_out, " rows of ",
                c_in, " channels padded to a multiple of 32");
    TORCH_CHECK(act >= 0 && act <= 2, op, ": act must be 0 (none), 1 (ReLU) or 2 (ELU), got ", act);
    auto vec = [&](const OptTensor& t, const char* what, int64_t n) -> const float* {
        if (!(t.has_value() && t->defined())) return nullptr;
        need_f32_cuda(*t, op, what);
        same_device(x, *t, op, what);
        TORCH_CHECK(t->is_contiguous() && t->numel() >= n, op, ": ", what, " must be a contiguous vector of at least ", n, " floats");
        return t->data_ptr<float>();
    };
    const float* ps = vec(pre_scale, "pre_scale", c_in);
    const float* pb = vec(pre_shift, "pre_shift", c_in);
    const float* es = vec(e1_scale, "e1_scale", c_out);
    const float* eb = vec(e1_shift, "e1_shift", c_out);
    TORCH_CHECK((ps == nullptr) == (pb == nullptr) && (es == nullptr) == (eb == nullptr), op, ": give both vectors of an affine or neither");
    c10::hip::HIPGuardMasqueradingAsCUDA guard(x.device());
    check_rc(bts_conv1x1_bf16_fwd_bf16(x.data_ptr<float>(), xs, (long)npix, (int)c_in, w_plane.data_ptr(), (int)k_pad, (int)c_out, (int)c_out_pad,
                                       ps, pb, (int)(pre_relu != 0), es, eb, (int)act, y.data_ptr(), ys, current_stream()), op);
}

// act(e1(conv3x3(x))) from a bfloat16 NHWC input as one launch of the bf16 halo tile (bts_conv3x3_bf16in_fwd_f32).  x: [B*h*w,
// >= c_in] view of a bf16 buffer; w_plane: the one-plane bf16 form of the packed 3x3 weight, [c_out_pad, k_pad] or
// [1, c_out_pad, k_pad], int16 bits (ops.round_bf16) or bfloat16; y: [B*h*w, c_out] fp32 NHWC view.
// geom = {B, h, w, c_in, c_out, act}.
void conv3x3_bf16in(const Tensor& x, const Tensor& w_plane, OptTensor e1_scale, OptTensor e1_shift, Tensor y, std::vector<int64_t> geom) {
    const char* op = "bts_hip::conv3x3_bf16in";
    TORCH_CHECK(geom.size() == 6, op, ": geom must hold 6 integers, got ", geom.size());
    const int64_t B = geom[0], h = geom[1], w = geom[2], c_in = geom[3], c_out = geom[4], act = geom[5];
    TORCH_CHECK(B > 0 && h > 0 && w > 0 && c_in > 0 && c_out > 0, op, ": non-positive dimension");
    TORCH_CHECK(c_in % 32 == 0, op, ": c_in (", c_in, ") must be a multiple of 32");
    const long xs = rows2d_stride_bf16(x, op, "x");
    need_f32_cuda(y, op, "y");
    TORCH_CHECK(y.dim() == 2 && y.stride(1) == 1, op, ": y must be a 2-D view with unit channel stride");
    const long ys = y.size(0) > 1 ? y.stride(0) : y.size(1);
    TORCH_CHECK(w_plane.is_cuda(), op, ": w_plane must be a CUDA(ROCm) tensor (no CPU fallback)");
    TORCH_CHECK(w_plane.scalar_type() == at::kShort || w_plane.scalar_type() == at::kBFloat16, op,
                ": w_plane must hold bf16 bits (int16 from ops.round_bf16, or bfloat16), got ", w_plane.scalar_type());
    same_device(x, w_plane, op, "w_plane");
    same_device(x, y, op, "y");
    TORCH_CHECK(x.size(0) == B * h * w && x.size(1) >= c_in, op, ": x (", x.sizes(), ") is not a [B*h*w, >= c_in] view");
    TORCH_CHECK(y.size(0) == B * h * w && y.size(1) == c_out, op, ": y (", y.sizes(), ") is not a [B*h*w, c_out] view");
    const int64_t wd = w_plane.dim();
    TORCH_CHECK(w_plane.is_contiguous() && (wd == 2 || (wd == 3 && w_plane.size(0) == 1)), op,
                ": w_plane must be contiguous [c_out_pad, k_pad] or [1, c_out_pad, k_pad] (ops.round_bf16), got ", w_plane.sizes());
    const int64_t c_out_pad = w_plane.size(wd - 2), k_pad = w_plane.size(wd - 1);
    TORCH_CHECK(c_out_pad >= c_out && c_out_pad % 32 == 0 && k_pad >= 9 * c_in && k_pad % 8 == 0, op, ": w_plane ", w_plane.sizes(),
                " does not hold ", c_out, " rows (padded to a multiple of 32) of 9 x ", c_in, " channels");
    TORCH_CHECK(act >= 0 && act <= 2, op, ": act must be 0 (none), 1 (ReLU) or 2 (ELU), got ", act);
    auto vec = [&](const OptTensor& t, const char* what) -> const float* {
        if (!(t.has_value() && t->defined())) return nullptr;
        need_f32_cuda(*t, op, what);
        same_device(x, *t, op, what);
        TORCH_CHECK(t->is_contiguous() && t->numel() >= c_out_pad, op, ": ", what, " must be a contiguous vector of at least ", c_out_pad, " floats");
        return t->data_ptr<float>();
    };
    const float* es = vec(e1_scale, "e1_scale");
    const float* eb = vec(e1_shift, "e1_shift");
    TORCH_CHECK((es == nullptr) == (eb == nullptr), op, ": give both e1 vectors or neither");
    c10::hip::HIPGuardMasqueradingAsCUDA guard(x.device());
    check_rc(bts_conv3x3_bf16in_fwd_f32(x.data_ptr(), xs, (int)B, (int)h, (int)w, (int)c_in, w_plane.data_ptr(), (int)k_pad, (int)c_out,
                                        (int)c_out_pad, es, eb, (int)act, y.data_ptr<float>(), ys, current_stream()), op);
}

// ---------------------------------------------------------- wide 1x1, bf16 operands, 128 / 192 / 256 wide, bottleneck epilogue
// act(e1(conv1x1(bf16(pre(x)))) + res), also written to y2, as one launch of bts_conv1x1_bf16_wide_fwd_f32.  The operands of
// conv1x1_bf16 above, plus res / y2: optional [npix, c_out] NHWC views.  geom = {npix, c_in, c_out, pre_relu, act, bn}.
void conv1x1_bf16_wide(const Tensor& x, const Tensor& w_plane, OptTensor pre_scale, OptTensor pre_shift, OptTensor e1_scale,
                       OptTensor e1_shift, OptTensor res, Tensor y, OptTensor y2, std::vector<int64_t> geom) {
    const char* op = "bts_hip::conv1x1_bf16_wide";
    TORCH_CHECK(geom.size() == 6, op, ": geom must hold 6 integers, got ", geom.size());
    const int64_t npix = geom[0], c_in = geom[1], c_out = geom[2], pre_relu = geom[3], act = geom[4], bn = geom[5];
    TORCH_CHECK(npix > 0 && c_in > 0 && c_out > 0, op, ": non-positive dimension");
    TORCH_CHECK(c_in % 16 == 0 && (c_out % 128 == 0 || c_out % 192 == 0), op,
                ": needs c_in % 16 == 0 and c_out a multiple of 128 or 192, got ", c_in, " -> ", c_out);
    TORCH_CHECK(bn == 0 || ((bn == 128 || bn == 192 || bn == 256) && c_out % bn == 0), op,
                ": bn must be 0 or one of 128 / 192 / 256 that divides c_out, got ", bn);
    const long xs = rows2d_stride(x, op, "x"), ys = rows2d_stride(y, op, "y");
    TORCH_CHECK(w_plane.is_cuda(), op, ": w_plane must be a CUDA(ROCm) tensor (no CPU fallback)");
    TORCH_CHECK(w_plane.scalar_type() == at::kShort || w_plane.scalar_type() == at::kBFloat16, op,
                ": w_plane must hold bf16 bits (int16 from ops.round_bf16, or bfloat16), got ", w_plane.scalar_type());
    same_device(x, w_plane, op, "w_plane");
    same_device(x, y, op, "y");
    TORCH_CHECK(x.size(0) == npix && x.size(1) >= c_in, op, ": x (", x.sizes(), ") is not a [npix, >= c_in] view");
    TORCH_CHECK(y.size(0) == npix && y.size(1) == c_out, op, ": y (", y.sizes(), ") is not a [npix, c_out] view");
    auto view = [&](const OptTensor& t, const char* what, long* stride) -> float* {
        *stride = 0;
        if (!(t.has_value() && t->defined())) return nullptr;
        *stride = rows2d_stride(*t, op, what);
        same_device(x, *t, op, what);
        TORCH_CHECK(t->size(0) == npix && t->size(1) == c_out, op, ": ", what, " (", t->sizes(), ") is not a [npix, c_out] view");
        return t->data_ptr<float>();
    };
    long rs = 0, y2s = 0;
    const float* rp = view(res, "res", &rs);
    float* y2p = view(y2, "y2", &y2s);
    const int64_t wd = w_plane.dim();
    TORCH_CHECK(w_plane.is_contiguous() && (wd == 2 || (wd == 3 && w_plane.size(0) == 1)), op,
                ": w_plane must be contiguous [c_out_pad, k_pad] or [1, c_out_pad, k_pad] (ops.round_bf16), got ", w_plane.sizes());
    const int64_t c_out_pad = w_plane.size(wd - 2), k_pad = w_plane.size(wd - 1);
    TORCH_CHECK(c_out_pad >= c_out && k_pad >= c_in && k_pad % 32 == 0, op, ": w_plane ", w_plane.sizes(), " does not hold ", c_out, " rows of ",
                c_in, " channels padded to a multiple of 32");
    TORCH_CHECK(act >= 0 && act <= 2, op, ": act must be 0 (none), 1 (ReLU) or 2 (ELU), got ", act);
    auto vec = [&](const OptTensor& t, const char* what, int64_t n) -> const float* {
        if (!(t.has_value() && t->defined())) return nullptr;
        need_f32_cuda(*t, op, what);
        same_device(x, *t, op, what);
        TORCH_CHECK(t->is_contiguous() && t->numel() >= n, op, ": ", what, " must be a contiguous vector of at least ", n, " floats");
        return t->data_ptr<float>();
    };
    const float* ps = vec(pre_scale, "pre_scale", c_in);
    const float* pb = vec(pre_shift, "pre_shift", c_in);
    const float* es = vec(e1_scale, "e1_scale", c_out);
    const float* eb = vec(e1_shift, "e1_shift", c_out);
    TORCH_CHECK((ps == nullptr) == (pb == nullptr) && (es == nullptr) == (eb == nullptr), op, ": give both vectors of an affine or neither");
    c10::hip::HIPGuardMasqueradingAsCUDA guard(x.device());
    check_rc(bts_conv1x1_bf16_wide_fwd_f32(x.data_ptr<float>(), xs, (long)npix, (int)c_in, w_plane.data_ptr(), (int)k_pad, (int)c_out,
                                           (int)c_out_pad, ps, pb, (int)(pre_relu != 0), es, eb, rp, rs, (int)act, y.data_ptr<float>(), ys,
                                           y2p, y2s, (int)bn, current_stream()), op);
}

// ------------------------------------------------------------------------------------------------------ training losses
// silog_loss / depth_l1_loss (pytorch/bts.py:41-63) over the valid pixels of the whole batch, csrc/loss.hip: no boolean gather, no host
// sync.  kind 0 = silog (param = variance_focus), 1 = asymmetric L1 (param = inbalance_to_closer); mask bool / uint8 or None (gt > gt_min).
const unsigned char* depth_loss_checks(const char* op, const Tensor& est, const Tensor& gt, const OptTensor& mask, int64_t kind) {
    need_f32_cuda(est, op, "est");
    need_f32_cuda(gt, op, "gt");
    same_device(est, gt, op, "gt");
    TORCH_CHECK(est.sizes() == gt.sizes(), op, ": est ", est.sizes(), " and gt ", gt.sizes(), " must have the same shape");
    TORCH_CHECK(est.numel() > 0, op, ": empty depth map");
    TORCH_CHECK(est.is_contiguous() && gt.is_contiguous(), op, ": est and gt must be contiguous");
    TORCH_CHECK(kind == 0 || kind == 1, op, ": kind must be 0 (silog) or 1 (L1), got ", kind);
    if (!(mask.has_value() && mask->defined())) return nullptr;
    TORCH_CHECK(mask->is_cuda(), op, ": mask must be a CUDA(ROCm) tensor (no CPU fallback)");
    TORCH_CHECK(mask->scalar_type() == at::kBool || mask->scalar_type() == at::kByte, op, ": mask must be bool or uint8, got ", mask->scalar_type());
    same_device(est, *mask, op, "mask");
    TORCH_CHECK(mask->sizes() == est.sizes(), op, ": mask ", mask->sizes(), " and est ", est.sizes(), " must have the same shape");
    TORCH_CHECK(mask->is_contiguous(), op, ": mask must be contiguous");
    return static_cast<const unsigned char*>(mask->data_ptr());
}

// returns (loss 0-d fp32, stats [4] fp64: valid count, mean d, mean d^2 (0, 0 for L1), loss)
std::tuple<Tensor, Tensor> depth_loss(const Tensor& est, const Tensor& gt, const OptTensor& mask, double gt_min, int64_t kind, double param) {
    const char* op = "bts_hip::depth_loss";
    const unsigned char* m = depth_loss_checks(op, est, gt, mask, kind);
    c10::hip::HIPGuardMasqueradingAsCUDA guard(est.device());
    const long npix = (long)est.numel(), nws = bts_depth_loss_ws_doubles(npix);
    Tensor ws = at::empty({nws}, est.options().dtype(at::kDouble));
    Tensor stats = at::empty({4}, est.options().dtype(at::kDouble));
    Tensor loss = at::empty({}, est.options());
    check_rc(bts_depth_loss_fwd_f32(est.data_ptr<float>(), gt.data_ptr<float>(), m, (float)gt_min, npix, (int)kind, (float)param,
                                    ws.data_ptr<double>(), nws, stats.data_ptr<double>(), loss.data_ptr<float>(), current_stream()), op);
    return {loss, stats};
}

// d loss / d est scaled by the DEVICE scalar grad_loss; 0 at invalid pixels
Tensor depth_loss_backward(const Tensor& est, const Tensor& gt, const OptTensor& mask, double gt_min, int64_t kind, double param,
                           const Tensor& stats, const Tensor& grad_loss) {
    const char* op = "bts_hip::depth_loss_backward";
    const unsigned char* m = depth_loss_checks(op, est, gt, mask, kind);
    need_f32_cuda(grad_loss, op, "grad_loss");
    same_device(est, grad_loss, op, "grad_loss");
    same_device(est, stats, op, "stats");
    TORCH_CHECK(grad_loss.numel() == 1, op, ": grad_loss must hold one float, got ", grad_loss.sizes());
    TORCH_CHECK(stats.is_cuda() && stats.scalar_type() == at::kDouble && stats.is_contiguous() && stats.numel() == 4, op,
                ": stats must be the contiguous float64 [4] tensor the forward returned");
    c10::hip::HIPGuardMasqueradingAsCUDA guard(est.device());
    // the gradient starts at est's offset from a 16-byte line, so that the kernel can store 16 bytes per lane next to its loads
    const int64_t off = (reinterpret_cast<uintptr_t>(est.data_ptr()) & 15) >> 2;
    Tensor g = at::empty({est.numel() + off}, est.options()).narrow(0, off, est.numel()).view(est.sizes());
    check_rc(bts_depth_loss_bwd_f32(est.data_ptr<float>(), gt.data_ptr<float>(), m, (float)gt_min, (long)est.numel(), (int)kind, (float)param,
                                    stats.data_ptr<double>(), grad_loss.data_ptr<float>(), g.data_ptr<float>(), current_stream()), op);
    return g;
}

}  // namespace

TORCH_LIBRARY(bts_hip, m) {
    m.def("lpg(Tensor plane_eq, int upratio) -> (Tensor, Tensor)");
    m.def("lpg_backward(Tensor plane_eq, Tensor grad_depth, int upratio) -> Tensor");
    m.def("reduction_1x1(Tensor x2d, int c_in, int c_first_out, Tensor w_frag, float max_depth, bool is_final, bool normalize, Tensor(a!) out) -> ()");
    m.def("reduc_lpg(Tensor x2d, int B, int h, int w, int c_in, int c_first_out, Tensor w_frag, float max_depth, int upratio, "
          "Tensor(a!) depth_scaled, Tensor(b!)? ds_out, Tensor(c!)? abs_min, Tensor(d!)? plane4) -> ()");
    m.def("reduc_bwd(Tensor x2d, int B, int h, int w, int c_in, int c_first_out, Tensor w_frag, Tensor wt_frag, float max_depth, int upratio, "
          "Tensor grad_out, Tensor(a!)? dx, Tensor(b!)? G, Tensor(c!) Y) -> ()");
    m.def("reduc_lpg_train(Tensor x2d, int B, int h, int w, Tensor[] weights, Tensor[] packs, float max_depth, int upratio) -> (Tensor, Tensor)");
    m.def("reduction_1x1_train(Tensor x2d, int B, int h, int w, Tensor[] weights, Tensor[] packs, float max_depth) -> Tensor");
    m.def("conv_fwd(Tensor x, Tensor w, Tensor? pre_scale, Tensor? pre_shift, Tensor? e1_scale, Tensor? e1_shift, Tensor? e2_scale, "
          "Tensor? e2_shift, Tensor(a!) y, Tensor(b!)? y2, Tensor? res, Tensor(c!)? splitk_ws, Tensor[] tail_planes, Tensor? w_split, "
          "Tensor? w_wino, int[] geom) -> ()");
    m.def("upconv_up9(Tensor x, Tensor u, Tensor? e2_scale, Tensor? e2_shift, Tensor(a!) y, int[] geom) -> ()");
    m.def("conv_tail_bf16(Tensor x, Tensor w_main, Tensor w_tail, Tensor tail, Tensor? e2_scale, Tensor? e2_shift, Tensor(a!) y, int[] geom) -> ()");
    m.def("conv1x1_bf16(Tensor x, Tensor w_plane, Tensor? pre_scale, Tensor? pre_shift, Tensor? e1_scale, Tensor? e1_shift, Tensor(a!) y, "
          "int[] geom) -> ()");
    m.def("conv1x1_bf16_ybf16(Tensor x, Tensor w_plane, Tensor? pre_scale, Tensor? pre_shift, Tensor? e1_scale, Tensor? e1_shift, "
          "Tensor(a!) y, int[] geom) -> ()");
    m.def("conv3x3_bf16in(Tensor x, Tensor w_plane, Tensor? e1_scale, Tensor? e1_shift, Tensor(a!) y, int[] geom) -> ()");
    m.def("conv1x1_bf16_wide(Tensor x, Tensor w_plane, Tensor? pre_scale, Tensor? pre_shift, Tensor? e1_scale, Tensor? e1_shift, Tensor? res, "
          "Tensor(a!) y, Tensor(b!)? y2, int[] geom) -> ()");
    m.def("depth_loss(Tensor est, Tensor gt, Tensor? mask, float gt_min, int kind, float param) -> (Tensor loss, Tensor stats)");
    m.def("depth_loss_backward(Tensor est, Tensor gt, Tensor? mask, float gt_min, int kind, float param, Tensor stats, Tensor grad_loss) -> Tensor");
}

TORCH_LIBRARY_IMPL(bts_hip, CUDA, m) {
    m.impl("lpg", &lpg);
    m.impl("lpg_backward", &lpg_backward);
    m.impl("reduction_1x1", &reduction_1x1);
    m.impl("reduc_lpg", &reduc_lpg);
    m.impl("reduc_bwd", &reduc_bwd);
    m.impl("reduc_lpg_train", &reduc_lpg_train);
    m.impl("reduction_1x1_train", &reduction_1x1_train);
    m.impl("conv_fwd", &conv_fwd);
    m.impl("upconv_up9", &upconv_up9);
    m.impl("conv_tail_bf16", &conv_tail_bf16);
    m.impl("conv1x1_bf16", &conv1x1_bf16);
    m.impl("conv1x1_bf16_ybf16", &conv1x1_bf16_ybf16);
    m.impl("conv3x3_bf16in", &conv3x3_bf16in);
    m.impl("conv1x1_bf16_wide", &conv1x1_bf16_wide);
    m.impl("depth_loss", &depth_loss);
    m.impl("depth_loss_backward", &depth_loss_backward);
}
