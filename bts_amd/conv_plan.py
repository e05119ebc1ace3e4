"""What bts_conv_fwd_f32 will launch for a descriptor: the one Python home of the library's host-side plan queries
(bts_conv_plan_f32 / bts_conv_plan_ksteps_f32, include/bts_hip.h), the names of the kernel kinds they report, the
kernel name a profiler shows for a plan, and a descriptor builder from plain integers.  No GPU work and no torch: the
queries walk the real dispatch on the host and never dereference the descriptor's pointers."""
from __future__ import annotations

import ctypes as C
from collections import namedtuple
from enum import IntEnum, IntFlag

from . import _lib
from ._lib import ConvDesc

# The header's BTS_CONV_KIND_* (kernel family = kind & FAMILY_MASK) and BTS_CONV_FLAG_* (bits on top), documented there
class Family(IntEnum):
    ROW, HALO, HALO_TAIL, WIDE_1X1, STEM, HALO_EMU, WINO, ROW_BF16, HALO_BF16 = range(9)


FAMILY_MASK = 15


class Flag(IntFlag):
    SPLITK, W8, DIL = 16, 32, 64


Plan = namedtuple("Plan", "rc family bm bn splitk w8 dil kind issued dense")


def query(desc: ConvDesc, ksteps: bool = False) -> Plan:
    """The library's own answer for ``desc``: return code, kernel family, tile, flags and the raw ``kind``; with
    ``ksteps`` also the tap-steps issued / dense (None otherwise).  Always asks the real library: these are pure host
    queries, a plan recording (bts_amd/plan.py) must never see them."""
    lib = _lib.load_real()
    bm, bn, kind = C.c_int(0), C.c_int(0), C.c_int(0)
    rc = lib.bts_conv_plan_f32(C.byref(desc), C.byref(bm), C.byref(bn), C.byref(kind))
    issued = dense = None
    if ksteps:
        i, d = C.c_long(0), C.c_long(0)
        rc2 = lib.bts_conv_plan_ksteps_f32(C.byref(desc), C.byref(i), C.byref(d))
        assert rc2 == rc, (rc, rc2)                  # both walk the same dispatch
        issued, dense = i.value, d.value
    k = kind.value
    return Plan(rc, Family(k & FAMILY_MASK), bm.value, bn.value, bool(k & Flag.SPLITK), bool(k & Flag.W8),
                bool(k & Flag.DIL), k, issued, dense)


def kernel_name(plan: Plan, nchw: bool, subpixel: bool) -> str:
    """The kernel instantiation as rocprofv3 names it (and bench.py's roofline leg parses it)."""
    f, lay, k = plan.family, "nchw" if nchw else "nhwc", 2 if subpixel else 3
    if f in (Family.ROW, Family.ROW_BF16):
        return "conv_fwd_kernel<%d,%d,%s%s%s>" % (plan.bm, plan.bn, lay, ",splitk" if plan.splitk else "",
                                                 ",bf16" if f == Family.ROW_BF16 else "")
    if f in (Family.HALO, Family.HALO_TAIL):
        return "conv_halo_kernel<%d,k%d,%s%s%s%s>" % (plan.bn, k, lay, ",tail" if f == Family.HALO_TAIL else "",
                                                     ",w8" if plan.w8 else "", ",dil" if plan.dil else "")
    if f in (Family.HALO_EMU, Family.HALO_BF16):
        return "conv_halo_emu_kernel<%d,k%d%s>" % (plan.bn, k, ",bf16" if f == Family.HALO_BF16 else "")
    if f == Family.WIDE_1X1:
        return "conv1x1_kernel<%d,%d>" % (plan.bn, plan.bm // 32)      # <BN, WM>: rows = 32 * WM
    return {Family.STEM: "conv_stem_kernel<%d>", Family.WINO: "conv_wino_kernel<%d>"}[f] % plan.bn


def tail_wino_kernel_name() -> str:
    """The kernel bts_conv_tail_wino_fwd_f32 launches (its own entry point: no bts_conv_plan_f32 kind), as KernelTrace records it."""
    return "conv_wino_tail_kernel<32>"


def tail_bf16_kernel_name(bn: int) -> str:
    """The kernel bts_conv_tail_bf16_fwd_f32 launches (its own entry point: no bts_conv_plan_f32 kind), as KernelTrace records it."""
    return "conv_tail_bf16_kernel<%d>" % bn


def wide_1x1_bf16_kernel_name(bn: int = 192, y_bf16: bool = False) -> str:
    """The kernel bts_conv1x1_bf16_fwd_f32 (``y_bf16``: bts_conv1x1_bf16_fwd_bf16) launches (its own entry point: no
    bts_conv_plan_f32 kind), as KernelTrace records it."""
    return ("conv1x1_bf16_ybf16_kernel<%d>" if y_bf16 else "conv1x1_bf16_kernel<%d>") % bn


def bf16in_3x3_tile(c_out: int) -> int:
    """The column tile bts_conv3x3_bf16in_fwd_f32 launches: 128 where bts_conv_fwd_f32's tile choice (csrc/conv_mfma.hip:
    choose_tile, least padded width weighted by tile efficiency) picks 128 for ``c_out``, else 64."""
    cost = {bn: round_up(c_out, bn) * eff for bn, eff in ((128, 1.0), (64, 1.05), (32, 1.2), (48, 1.12)) if bn != 48 or c_out % 48 == 0}
    return 128 if min(cost, key=lambda bn: (cost[bn], (128, 64, 32, 48).index(bn))) == 128 else 64


def bf16in_3x3_kernel_name(bn: int) -> str:
    """The kernel bts_conv3x3_bf16in_fwd_f32 launches (its own entry point: no bts_conv_plan_f32 kind), as KernelTrace records it."""
    return "conv3x3_bf16in_kernel<%d>" % bn


def wide_1x1_bf16_tile(c_out: int) -> int:
    """The tile bts_conv1x1_bf16_wide_fwd_f32 launches for ``bn`` = 0 (csrc/conv_1x1_bf16.inc: c1w_bn; the plan query's *bn
    for a layer it accepts), for KernelTrace's kernel name."""
    return 192 if c_out % 192 == 0 else 128


def grouped_kernel_name(cg: int) -> str:
    """The kernel bts_conv_grouped_fwd_f32 launches for ``cg`` channels per group (its own entry point: no bts_conv_plan_f32
    kind), as KernelTrace records it."""
    return "conv_grouped_kernel<%d>" % cg


def grouped_bf16_kernel_name(cg: int) -> str:
    """The kernel bts_conv_grouped_bf16_fwd_f32 launches for ``cg`` channels per group, as KernelTrace records it (does not
    begin with grouped_kernel_name's prefix: launch counts tell the two kernels apart by it)."""
    return "conv_grouped_bf16_kernel<%d>" % cg


def grouped_wgrad_kernel_name(cg: int) -> str:
    """The kernel bts_conv_grouped_wgrad_f32 launches for ``cg`` channels per group, as KernelTrace records it (its reduce
    launch rides in the same record)."""
    return "conv_grouped_wgrad_kernel<%d>" % cg


def round_up(v: int, m: int) -> int:
    return (v + m - 1) // m * m


def conv_out_hw(h: int, w: int, ksize: int, dil: int, stride: int, pad: int, up: int):
    """Output extent of a convolution over the (optionally ``up``-times upsampled) h x w map."""
    return ((h * up + 2 * pad - dil * (ksize - 1) - 1) // stride + 1,
            (w * up + 2 * pad - dil * (ksize - 1) - 1) // stride + 1)


def geometry_desc(B: int, h: int, w: int, c_in_ld: int, c_out: int, ksize: int, dil: int = 1, stride: int = 1,
                  pad=None, up: int = 1, subpixel: bool = False, n_bundles: int = 0, n_tail: int = 0, nchw: bool = False,
                  fill_frames: int = 0, precision: int = 0, x_pix_stride=None, y_pix_stride=None, c_out_pad=None,
                  fake_pointers: bool = False) -> ConvDesc:
    """The integer part of a bts_conv_desc.  ``subpixel``: pass the reference's ksize 3 / up 2; the descriptor gets the
    four 2x2 classes the library computes.  Defaults: pad dil*(ksize//2), c_out_pad = c_out rounded up to 32, pixel
    strides = the channels the descriptor itself needs.  ``fake_pointers``: non-null x / w / y / tail planes, for
    host-only queries."""
    d = ConvDesc()
    nb = max(n_bundles, 1)
    d.c_in_ld, d.k_pad = c_in_ld, round_up((4 if subpixel else ksize * ksize) * c_in_ld, 32)
    d.x_pix_stride = (c_in_ld - (4 if n_tail else 0)) * nb if x_pix_stride is None else x_pix_stride
    d.B, d.h_in, d.w_in, d.up, d.ksize, d.dil, d.stride = B, h, w, up, ksize, dil, stride
    d.pad = dil * (ksize // 2) if pad is None else pad
    if subpixel:
        d.up, d.ksize, d.pad, d.subpixel = 1, 2, 0, 1
    d.c_out, d.c_out_pad = c_out, round_up(c_out, 32) if c_out_pad is None else c_out_pad
    d.y_nchw = int(bool(nchw))
    d.y_pix_stride = (0 if nchw else c_out * nb) if y_pix_stride is None else y_pix_stride
    d.n_bundles = n_bundles if n_bundles > 1 else 0
    d.n_tail, d.fill_frames, d.precision = n_tail, fill_frames, precision
    if fake_pointers:
        d.x = d.w = d.y = 0x1000
        for j in range(n_tail):
            d.tail_planes[j] = 0x5000
    return d
