"""CPU: bts_amd/conv_plan.py -- the Python names of the plan kinds against include/bts_hip.h, and the kernel name of a plan."""
import os
import subprocess

from bts_amd.conv_plan import FAMILY_MASK, Family, Flag, Plan, kernel_name

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_kind_enum_matches_header(tmp_path):
    """Family / Flag / FAMILY_MASK equal the BTS_CONV_KIND_* / BTS_CONV_FLAG_* enumerators, value for value, as a C compiler
    reads the header; neither side has a name the other lacks."""
    import re
    hdr = open(os.path.join(ROOT, "include", "bts_hip.h")).read()
    names = sorted(set(re.findall(r"\bBTS_CONV_(?:KIND|FLAG)_[A-Z0-9_]+", hdr)))
    src = tmp_path / "kinds.c"
    src.write_text('#include <stdio.h>\n#include "bts_hip.h"\nint main(void){%s return 0;}\n'
                   % "".join('printf("%s %%d\\n", (int)%s);' % (n, n) for n in names))
    exe = tmp_path / "kinds"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    c_vals = {k: int(v) for k, v in (line.split() for line in subprocess.check_output([str(exe)]).decode().splitlines())}
    py_vals = {"BTS_CONV_KIND_" + m.name: int(m) for m in Family}
    py_vals.update({"BTS_CONV_FLAG_" + m.name: int(m) for m in Flag})
    py_vals["BTS_CONV_KIND_MASK"] = FAMILY_MASK
    assert c_vals == py_vals
    assert len(Family) == 9 and len(set(c_vals.values())) == len(c_vals)


def _plan(family, bm, bn, splitk=False, w8=False, dil=False):
    kind = family | (Flag.SPLITK if splitk else 0) | (Flag.W8 if w8 else 0) | (Flag.DIL if dil else 0)
    return Plan(0, family, bm, bn, splitk, w8, dil, int(kind), None, None)


KERNEL_NAMES = [   # (plan, nchw, subpixel) -> the name KernelTrace records and bench.py's roofline leg matches
    (_plan(Family.ROW, 64, 128), False, False, "conv_fwd_kernel<64,128,nhwc>"),
    (_plan(Family.ROW, 128, 48, splitk=True), False, False, "conv_fwd_kernel<128,48,nhwc,splitk>"),
    (_plan(Family.ROW, 128, 32), True, False, "conv_fwd_kernel<128,32,nchw>"),
    (_plan(Family.ROW, 64, 64, splitk=True), True, False, "conv_fwd_kernel<64,64,nchw,splitk>"),
    (_plan(Family.ROW, 128, 64), False, True, "conv_fwd_kernel<128,64,nhwc>"),
    (_plan(Family.HALO_TAIL, 128, 32), True, False, "conv_halo_kernel<32,k3,nchw,tail>"),
    (_plan(Family.HALO_TAIL, 128, 64), False, False, "conv_halo_kernel<64,k3,nhwc,tail>"),
    (_plan(Family.HALO, 128, 128), False, True, "conv_halo_kernel<128,k2,nhwc>"),
    (_plan(Family.HALO, 128, 64), True, False, "conv_halo_kernel<64,k3,nchw>"),
    (_plan(Family.WIDE_1X1, 128, 192), False, False, "conv1x1_kernel<192,4>"),
    (_plan(Family.WIDE_1X1, 64, 192), False, False, "conv1x1_kernel<192,2>"),
    (_plan(Family.HALO, 128, 48), False, False, "conv_halo_kernel<48,k3,nhwc>"),
    (_plan(Family.HALO, 128, 48, w8=True), False, False, "conv_halo_kernel<48,k3,nhwc,w8>"),
    (_plan(Family.HALO, 128, 128), False, False, "conv_halo_kernel<128,k3,nhwc>"),
    (_plan(Family.HALO, 128, 128, dil=True), False, False, "conv_halo_kernel<128,k3,nhwc,dil>"),
    (_plan(Family.STEM, 256, 96), False, False, "conv_stem_kernel<96>"),
    (_plan(Family.STEM, 256, 64), False, False, "conv_stem_kernel<64>"),
    (_plan(Family.HALO_EMU, 128, 128), False, False, "conv_halo_emu_kernel<128,k3>"),
    (_plan(Family.HALO_EMU, 128, 64), False, True, "conv_halo_emu_kernel<64,k2>"),
    (_plan(Family.WINO, 128, 48), False, False, "conv_wino_kernel<48>"),
    (_plan(Family.WINO, 128, 128), False, False, "conv_wino_kernel<128>"),
    (_plan(Family.ROW_BF16, 128, 128), False, False, "conv_fwd_kernel<128,128,nhwc,bf16>"),
    (_plan(Family.ROW_BF16, 64, 128, splitk=True), False, False, "conv_fwd_kernel<64,128,nhwc,splitk,bf16>"),
    (_plan(Family.ROW_BF16, 128, 32), True, False, "conv_fwd_kernel<128,32,nchw,bf16>"),
    (_plan(Family.HALO_BF16, 128, 64), False, False, "conv_halo_emu_kernel<64,k3,bf16>"),
    (_plan(Family.HALO_BF16, 128, 128), False, True, "conv_halo_emu_kernel<128,k2,bf16>"),
]


def test_kernel_name_of_a_plan():
    """Every family, both layouts where they apply, and each flag -- against names written out by hand."""
    for plan, nchw, subpixel, want in KERNEL_NAMES:
        assert kernel_name(plan, nchw, subpixel) == want, plan
    assert {c[0].family for c in KERNEL_NAMES} == set(Family)
    for flag in ("splitk", "w8", "dil"):
        assert any(getattr(c[0], flag) for c in KERNEL_NAMES), flag
