"""Case table and fp64 references for the forward half of the decoder's LPG stage: csrc/reduc.hip (bts_reduc_fwd_f32,
bts_reduc_lpg_fwd_f32), csrc/lpg.hip (bts_lpg_fused_fwd_f32, bts_lpg_bwd_f32) and csrc/lpg_math.h.
tests/test_reduc_lpg_cases_host.py asserts on the CPU what the designs below rely on (dispatch coverage, denominator
zones, threshold margins, ragged tiles, wrap sizes against the caps in the source, the committed floors);
tests/test_reduc_lpg_fp64_gpu.py runs the kernels against these references.

Every reference is the oracle's arithmetic (oracle/bts_oracle.py) in fp64, composed as reduc_train_ref.scale_forward
composes it.  `python tests/reduc_lpg_cases.py` prints FLOORS: the distance of the SAME oracle in fp32 on the CPU from
the fp64 one, in the metrics the GPU test uses.  FLOORS is a measurement of the reference, never of the code under test.

Metrics.  Planes and the final chain's map: max-abs error over max-abs value per component.  Depth and its
downsampled copy: max_i |got_i - ref_i| / |ref_i| * min(1, |den_i|) over every finite reference pixel -- the weight
removes the 1/|den| conditioning of n4/den, and the clamp zone counts in full (there the denominator is a constant)."""
import os
import sys
from collections import namedtuple

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:            # `python tests/reduc_lpg_cases.py` from anywhere
    sys.path.insert(0, ROOT)

import reduc_train_ref as R  # noqa: E402
from oracle import bts_oracle as O  # noqa: E402

CSRC = os.path.join(ROOT, "bts_amd", "csrc")
MD = R.MAX_DEPTH
U = 2.0 ** -24                      # one fp32 rounding, relative
EPS = 1e-3                          # the LPG clamp, bts.py:168-171
ZONE_LO, ZONE_HI = 0.8e-3, 1.2e-3   # no reference denominator lies in between (20 % around the clamp threshold)
ORDINARY = 1e-2                     # |den| of a pixel that is not in the clamp zone
DEN_MIN = 1e-6                      # ... nor below this, the constructed zero cell excepted
SENTINEL = -12345.625               # fills the slabs around every output

# ------------------------------------------------------------------------------------------------ chain cases
# One row per dispatch row of the two entry points of csrc/reduc.hip.  body: the kernel template the row launches
# ("wide" = reduc_fwd_kernel on the 32x32x2 MFMA, "narrow" = reduc16_fwd_kernel on the 16x16x4 MFMA; nt = 16-pixel tiles
# per wave of the narrow kernel).  B = 3, h = 5, w = 7: 105 cells = three full 32-cell wave tiles and a partial one; the
# frame boundaries (cells 35, 70) and every row end fall inside tiles.  seed: chosen on the CPU so that the fp64
# reference keeps |den| >= 1e-2 on every pixel (test_reduc_lpg_cases_host.py asserts it).
ChainRow = namedtuple("ChainRow", "name entry chain c_in c_first k final body nt seed")
SHAPE = (3, 5, 7)
FWD_ROWS = [
    ChainRow("fwd_128x128", "bts_reduc_fwd_f32", "8x8", 128, 128, 8, False, "wide", 0, 0),
    ChainRow("fwd_128x64", "bts_reduc_fwd_f32", "4x4", 128, 64, 4, False, "wide", 0, 0),
    ChainRow("fwd_64x32", "bts_reduc_fwd_f32", "2x2", 64, 32, 2, False, "narrow", 2, 0),
    ChainRow("fwd_64x64", "bts_reduc_fwd_f32", "8x8/256", 64, 64, 8, False, "narrow", 2, 0),
    ChainRow("fwd_32x16", "bts_reduc_fwd_f32", "2x2/256", 32, 16, 2, False, "narrow", 2, 0),
    ChainRow("fwd_32x16_final", "bts_reduc_fwd_f32", "final", 32, 16, 0, True, "narrow", 2, 0),
    ChainRow("fwd_16x8_final", "bts_reduc_fwd_f32", "final/256", 16, 8, 0, True, "narrow", 2, 0),
]
LPG_ROWS = [
    ChainRow("lpg_128x128_k8", "bts_reduc_lpg_fwd_f32", "8x8", 128, 128, 8, False, "wide", 0, 0),
    ChainRow("lpg_128x64_k4", "bts_reduc_lpg_fwd_f32", "4x4", 128, 64, 4, False, "wide", 0, 0),
    ChainRow("lpg_64x32_k2", "bts_reduc_lpg_fwd_f32", "2x2", 64, 32, 2, False, "narrow", 2, 0),
    ChainRow("lpg_64x64_k8", "bts_reduc_lpg_fwd_f32", "8x8/256", 64, 64, 8, False, "narrow", 2, 0),
    ChainRow("lpg_64x32_k4", "bts_reduc_lpg_fwd_f32", "4x4/256", 64, 32, 4, False, "narrow", 2, 0),
    ChainRow("lpg_32x16_k2", "bts_reduc_lpg_fwd_f32", "2x2/256", 32, 16, 2, False, "narrow", 2, 0),
]
ROWS = {r.name: r for r in FWD_ROWS + LPG_ROWS}
# the if-ladders of the two entry points, as (c_in, c_first_out, is_final) and (c_in, c_first_out, upratio)
DISPATCH_FWD = [(128, 128, False), (128, 64, False), (64, 32, False), (64, 64, False), (32, 16, False), (32, 16, True),
                (16, 8, True)]
DISPATCH_LPG = [(128, 128, 8), (128, 64, 4), (64, 32, 2), (64, 64, 8), (64, 32, 4), (32, 16, 2)]
X_PAD, X_OFF = 8, 4                 # x is columns X_OFF .. X_OFF + c_in of a buffer X_PAD columns wider, NaN elsewhere

# Clamp through the chain: reduc_train_ref.CLAMP_CASE (8x8, 2 x 24 x 32 cells, seed 743, theta row x 50), forward.
# There is no 4x4 or 2x2 twin: theta <= pi/3 gives n3 >= 0.5 and |n1|, |n2| <= 0.866, and |u|, |v| <= (K-1)/(2K), so
# den >= 0.5 - 0.866 * (3/8) * sqrt(2) > 0.04 at K = 4 and more at K = 2.  Only K = 8 reaches the clamp through a chain.
CLAMP_ROW = ROWS["lpg_128x128_k8"]
CLAMP_MIN_PIXELS = 10

# NaN: one x row of NaN in frame 1 (cell (1, 2, 3) of SHAPE), through the one-launch entry on both kernel bodies
NAN_ROWS = ("lpg_128x128_k8", "lpg_64x32_k2")
NAN_CELL = (1, 2, 3)

# Wrap: just over two passes of the launch's block cap, with a ragged last tile.  cap_expr: the text of the cap in
# csrc/reduc.hip (launch_reduc: `blocks > 256L * per_cu` with per_cu = 1 because the 8x8 chain's fragments exceed 80 KiB of
# LDS; launch_reduc16: `blocks > 256L * 4`); a block has 8 waves; tile = cells per wave iteration.
# tile_expr: where the tile size is written (the narrow kernel walks 16 * NT pixels per wave, NT = RT2 / RT1 = 2 for
# the non-final / final rows at this commit, so the final chain's pass is 1024 * 8 * 32 cells as well).
WrapCase = namedtuple("WrapCase", "name row cap_blocks cap_expr tile tile_expr theta_scale seed")
WRAP_CASES = [
    WrapCase("wrap_wide_k8", "lpg_128x128_k8", 256, "if (blocks > 256L * per_cu) blocks = 256L * per_cu;", 32,
             "const long ntiles = (npix + 31) / 32;", 0.25, 0),
    WrapCase("wrap_narrow_k2", "lpg_64x32_k2", 1024, "if (blocks > 256L * 4) blocks = 256L * 4;", 32, "#define RT2 2 ", None, 0),
    WrapCase("wrap_final", "fwd_32x16_final", 1024, "if (blocks > 256L * 4) blocks = 256L * 4;", 32, "#define RT1 2 ", None, 0),
]
WRAP_SOURCE_EXPRS = ("const int per_cu = lds > 80 * 1024 ? 1 : 2;", "long blocks = (ntiles + 7) / 8;", "long blocks = (ngroups + 7) / 8;",
                     "constexpr int PXW = 16 * NT;")
WAVES_PER_BLOCK = 8


def wrap_shape(case):
    """(h, w) with h * w = 2 * cap * 8 waves * tile + r, 0 < r < tile: every wave iterates twice and the first one a
    third time on a ragged tile (the sizing of reduc_train_ref.persistent_shape)."""
    per_pass = case.cap_blocks * WAVES_PER_BLOCK * case.tile
    for r in range(1, case.tile):
        n = 2 * per_pass + r
        for h in range(2, 512):
            if n % h == 0:
                return h, n // h
    raise AssertionError("no shape")


def chain_lds_bytes(c_in, c_first):
    """Bytes of the wide kernel's weight fragments (chain_frag_float4s of csrc/reduc_chain.h: rows padded to 32)."""
    n, k, m = 0, c_in, c_first
    while m >= 8:
        n += ((m + 31) // 32) * 32 * k
        k, m = m, m // 2
    return 4 * (n + 32 * k)


# ------------------------------------------------------------------------------------------------ chain references
def chain_reference(row, B, h, w, seed, theta_scale=None, dtype=torch.float64):
    """The oracle in ``dtype``: dict with x [B,c,h,w] fp32, ws, and per output the reference.  Non-final: plane0 /
    plane1 [B,4,h,w] (normalize 0 / 1), depth [B,1,hK,wK] (depth / max_depth), den [B,hK,wK] (un-clamped), abs_min.
    Final: out [B,1,h,w]."""
    x, ws, _ = R.make_case(row.chain, B, h, w, seed, theta_scale)
    xd, wd = x.to(dtype), [wt.to(dtype) for wt in ws]
    r = O.reduction_forward(xd, wd, MD, row.final)
    ref = {"x": x, "ws": ws}
    if row.final:
        ref["out"] = r
        return ref
    ref["plane0"] = r
    plane = torch.cat([F.normalize(r[:, :3], 2, 1), r[:, 3:4]], 1)
    ref["plane1"] = plane
    depth, am = O.lpg_forward(plane, row.k)
    ref["depth"] = depth.unsqueeze(1) / MD
    ref["den"] = O.lpg_denominator(plane, row.k)
    ref["abs_min"] = am
    return ref


_CACHE = {}


def cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def row_reference(name, dtype=torch.float64):
    row = ROWS[name]
    return cached(("row", name, dtype), lambda: chain_reference(row, *SHAPE, row.seed, None, dtype))


def clamp_reference(dtype=torch.float64):
    _, B, h, w, seed, ts = R.CLAMP_CASE
    return cached(("clamp", dtype), lambda: chain_reference(CLAMP_ROW, B, h, w, seed, ts, dtype))


def wrap_reference(case, dtype=torch.float64):
    h, w = wrap_shape(case)
    return cached(("wrap", case.name, dtype), lambda: chain_reference(ROWS[case.row], 1, h, w, case.seed, case.theta_scale, dtype))


# ------------------------------------------------------------------------------------------------ metrics
def plane_errors(got, ref):
    """max-abs error over max-abs value per component of [B,C,h,w]; the max-abs error itself where the reference component
    is identically zero (d/dn1, d/dn2 at K = 1, where u = v = 0)."""
    got, ref = torch.as_tensor(got).double(), ref.double()
    out = []
    for c in range(ref.shape[1]):
        m = float(ref[:, c].abs().max())
        out.append(float((got[:, c] - ref[:, c]).abs().max()) / (m if m > 0 else 1.0))
    return out


def den_weighted_error(got, ref, den):
    """max |got - ref| / |ref| * min(1, |den|) over the finite reference pixels ([B,1,H,W] against den [B,H,W])."""
    got, ref, den = torch.as_tensor(got).double().reshape(den.shape), ref.double().reshape(den.shape), den.double()
    fin = torch.isfinite(ref)
    e = (got - ref).abs() / ref.abs() * den.abs().clamp(max=1.0)
    return float(e[fin].max())


def clamp_decisions(den):
    """-1 / 0 / +1 per pixel: clamped to -eps, untouched, clamped to +eps."""
    return ((den > 0) & (den < EPS)).to(torch.int8) - ((den < 0) & (den > -EPS)).to(torch.int8)


def zone_counts(den):
    """(pixels with DEN_MIN < |den| < ZONE_LO of positive / negative sign, pixels in the 20 % margin, pixels with
    0 < |den| <= DEN_MIN, exact zeros)."""
    a = den.double().abs()
    inz = (a > DEN_MIN) & (a < ZONE_LO)
    return (int((inz & (den > 0)).sum()), int((inz & (den < 0)).sum()), int(((a >= ZONE_LO) & (a <= ZONE_HI)).sum()),
            int(((a > 0) & (a <= DEN_MIN)).sum()), int((a == 0).sum()))


# ------------------------------------------------------------------------------------- activation error, propagated
# csrc/common.h: elu1(x) = __expf(x) - 1 for x <= 0, stated at <= 1e-7 absolute.  sigmoid1(x) = __frcp_rn(1 + __expf(-x)),
# term by term as tests/test_conv_exact_gpu.py derives E_ACT["sigmoid"], kept per value instead of maximised over |x| <= 8:
# e = e^-x carries (|x| + 2) U relative (the rounding of x log2(e), the 1-ulp hardware 2^t), 1 + e one rounding, the
# reciprocal 2 U, so with s = 1 / (1 + e) and s^2 e = s (1 - s):  |d s| <= U ((|x| + 2) s (1 - s) + 3 s)  (< 3.73 U).
# The fp32 oracle's F.elu and torch.sigmoid are correctly rounded to well under these, so FLOORS does not contain them
# and the bars add them: first order, worst case, through the actual chain.
E_ELU = 1e-7


def sigmoid_error(o, s):
    return U * ((o.abs() + 2) * s * (1 - s) + 3 * s)


E_TRIG = 4.0 * U                    # sinf / cosf at 2 ulp of a value <= 1


def logit_error_bound(x, ws):
    """[npix, n_out] fp64: a bound on what E_ELU on every hidden activation does to the last layer's outputs.
    With z_l the pre-activations and D_l = diag(elu'(z_l)) (1 for z > 0, e^z else), the error of output j is
    sum_l (W_L D_{L-1} W_{L-1} ... D_{l+1} W_{l+1})[j, :] . delta_l with |delta_l| <= E_ELU elementwise, so at most
    E_ELU * sum_l || row j of that product ||_1 -- the product with its signs, per pixel, not a product of norms."""
    B, c, h, w = x.shape
    net = x.double().permute(0, 2, 3, 1).reshape(-1, c)
    Wm = [wt.double().reshape(wt.shape[0], wt.shape[1]) for wt in ws]
    zs = []
    for W in Wm[:-1]:
        z = net @ W.t()
        zs.append(z)
        net = torch.where(z > 0, z, torch.expm1(z))
    out = torch.zeros((net.shape[0], Wm[-1].shape[0]), dtype=torch.float64)
    for j in range(Wm[-1].shape[0]):
        G = Wm[-1][j].unsqueeze(0).expand(net.shape[0], -1)
        acc = G.abs().sum(1)
        for i in range(len(Wm) - 2, 0, -1):
            G = (G * torch.where(zs[i] > 0, torch.ones_like(zs[i]), torch.exp(zs[i]))) @ Wm[i]
            acc = acc + G.abs().sum(1)
        out[:, j] = E_ELU * acc
    return out, net @ Wm[-1].t()


def activation_terms(ref, row):
    """The part of each bar that the hardware activations account for, from the fp64 reference alone (first order, x 1.01
    for the second):
      final: |d out| <= e_o s (1 - s) + sigmoid_error, over max |out|.
      non-final, per cell: s_i = sigmoid(o_i), e_i = e_o,i s_i (1 - s_i) + sigmoid_error;
        theta = s_0 pi/3, phi = s_1 2 pi (two roundings and the rounded constant: 4 U relative):
          d theta = pi/3 e_0 + 4 U theta, d phi = 2 pi e_1 + 4 U phi;
        n1 = sin theta cos phi, n2 = sin theta sin phi, n3 = cos theta, each sinf / cosf within E_TRIG and one product:
          d n1, d n2 <= d theta + sin theta d phi + 9 U, d n3 <= sin theta d theta + 4 U;
        n4 = s_2 max_depth: d n4 / n4 = e_2 / s_2 + 2 U;
        normalize (|n| = 1 up to rounding; the derivative of n / |n| is a projection, so each component moves by at most
          |dn|_2 <= |dn|_1, plus sqrt and division): d n_c <= d n1 + d n2 + d n3 + 4 U.
      depth = n4 / (den_c max_depth), den = n1 u + n2 v + n3 with |u|, |v| < 1/2:
        d den <= d n1 / 2 + d n2 / 2 + d n3 + 3 U s (the two FMAs, s as in given_bound);
        relative error <= d n4 / n4 + 5 U + d den / |den| on un-clamped pixels and d n4 / n4 + 5 U on clamped ones (the
        margins keep the decision the same); the metric multiplies by min(1, |den|).
    Returns {"planes0": [4], "planes1": [4], "depth": float, "den_abs": float} or {"out": float}."""
    e_o, o = logit_error_bound(ref["x"], ref["ws"])
    s = torch.sigmoid(o)
    e = e_o * s * (1 - s) + sigmoid_error(o, s)
    if row.final:
        return {"out": 1.01 * float(e.max() / ref["out"].abs().max())}
    theta, phi = s[:, 0] * np.pi / 3, s[:, 1] * 2 * np.pi
    dth = np.pi / 3 * e[:, 0] + 4 * U * theta
    dph = 2 * np.pi * e[:, 1] + 4 * U * phi
    d12 = dth + torch.sin(theta) * dph + 9 * U
    d3 = torch.sin(theta) * dth + 4 * U
    d4rel = e[:, 2] / s[:, 2] + 2 * U
    dn = d12 + d12 + d3 + 4 * U
    B, _, h, w = ref["plane0"].shape
    p0, p1 = ref["plane0"], ref["plane1"]
    out = {"planes0": [1.01 * float(d.max() / p0[:, c].abs().max()) for c, d in enumerate((d12, d12, d3))]
                      + [1.01 * float((d4rel * p0[:, 3].reshape(-1)).max() / p0[:, 3].abs().max())],
           "planes1": [1.01 * float(dn.max() / p1[:, c].abs().max()) for c in range(3)]
                      + [1.01 * float((d4rel * p1[:, 3].reshape(-1)).max() / p1[:, 3].abs().max())]}
    k = row.k
    up = lambda t: torch.repeat_interleave(torch.repeat_interleave(t.reshape(B, h, w), k, 1), k, 2)
    den = ref["den"]
    smag = torch.maximum(torch.maximum(up(p1[:, 0].abs() / 2), up(p1[:, 1].abs() / 2)), torch.maximum(up(p1[:, 2].abs()), den.abs()))
    dden = up(2 * dn) + 3 * U * smag
    unclamped = clamp_decisions(den) == 0
    rel = up(d4rel) + 5 * U + torch.where(unclamped, dden / den.abs() * den.abs().clamp(max=1.0), torch.zeros_like(den))
    out["depth"] = 1.01 * float(rel.max())
    out["den_abs"] = 1.01 * float(dden.max())
    return out


# ------------------------------------------------------------------------------------------------ given-plane cases
# bts_lpg_fused_fwd_f32: planes are inputs, so every sign and zone is constructed.  ds = nearest-downsample factor (0:
# no ds_out), ds_stride = its pixel stride in floats.  kernel: what launch_lpg's predicate (lpg_kernel below) picks.
GivenCase = namedtuple("GivenCase", "name k B h w normalize ds ds_stride kernel")
GIVEN_CASES = [
    GivenCase("lean_k2_ds1", 2, 2, 5, 6, 0, 1, 1, "lean"),
    GivenCase("lean_k2_ds2_s5", 2, 2, 5, 6, 0, 2, 5, "lean"),
    GivenCase("lean_k4_ds2_s5", 4, 2, 5, 6, 0, 2, 5, "lean"),
    GivenCase("lean_k4_ds4", 4, 2, 5, 6, 0, 4, 1, "lean"),
    GivenCase("lean_k4_ds1_s5", 4, 2, 5, 6, 0, 1, 5, "lean"),
    GivenCase("lean_k8_ds4_s5", 8, 2, 5, 6, 0, 4, 5, "lean"),
    GivenCase("lean_k8_ds2", 8, 2, 5, 6, 0, 2, 1, "lean"),
    GivenCase("lean_k8_none", 8, 2, 5, 6, 0, 0, 1, "lean"),
    GivenCase("general_k8_ds8", 8, 2, 5, 6, 0, 8, 1, "general_v4"),          # a factor outside {1, 2, 4}
    GivenCase("general_k4_normalize_ds2_s5", 4, 2, 5, 6, 1, 2, 5, "general_v4"),
    GivenCase("general_k2_odd_w_ds2_s5", 2, 2, 5, 7, 0, 2, 5, "general_v1"),     # width 14: not a multiple of 4
]
GIVEN = {c.name: c for c in GIVEN_CASES}
GIVEN_CLAMP_CELLS = 36              # one clamp-zone pixel each, signs alternating: 18 + 18 >= 32 per case
# bound constants of given_bound: the denominator's absolute error in units of U * s
DEN_ROUNDINGS = {"lean": 3.0, "general_v4": 5.0, "general_v1": 5.0}
NORMALIZE_ROUNDINGS = 8.0


def lpg_kernel(k, B, h, w, normalize, ds_given, ds_factor, ds_pix_stride):
    """launch_lpg<PLANAR = false, FUSED = true> of csrc/lpg.hip restated: which kernel a fused launch gets."""
    vec4 = (w * k) % 4 == 0
    lean = (not normalize and vec4 and k >= 2 and (not ds_given or ds_factor in (1, 2, 4))
            and ds_pix_stride <= 0x7fffffff and B * h * k * w * k <= 0x7fffffff)
    return "lean" if lean else ("general_v4" if vec4 else "general_v1")


def _given_try(case, seed):
    k, B, h, w = case.k, case.B, case.h, case.w
    g = torch.Generator().manual_seed(seed)
    n = B * h * w
    sgn = lambda: torch.randint(0, 2, (n,), generator=g).double() * 2 - 1
    n1 = (0.15 + 0.25 * torch.rand(n, generator=g, dtype=torch.float64)) * sgn()
    n2 = (0.15 + 0.25 * torch.rand(n, generator=g, dtype=torch.float64)) * sgn()
    n3 = (0.5 + 0.5 * torch.rand(n, generator=g, dtype=torch.float64)) * sgn()
    n4 = (0.5 + 60.0 * torch.rand(n, generator=g, dtype=torch.float64)) * sgn()
    cells = torch.randperm(n - 1, generator=g)[:GIVEN_CLAMP_CELLS] + 1
    px = torch.randint(0, k, (GIVEN_CLAMP_CELLS, 2), generator=g).double()
    uv = (px - (k - 1) * 0.5) / k
    t = (5e-5 + 6.5e-4 * torch.rand(GIVEN_CLAMP_CELLS, generator=g, dtype=torch.float64))
    t = t * (1 - 2 * (torch.arange(GIVEN_CLAMP_CELLS) % 2).double())
    # a clamp cell's slopes are (a, +-a / K) in either order, |a| in [0.7, 0.95]: den - t = (i + j / K) a / K over the
    # cell's pixels vanishes on the chosen pixel alone, and is at least a / K^2 >= 1.09e-2 elsewhere
    a = (0.7 + 0.25 * torch.rand(GIVEN_CLAMP_CELLS, generator=g, dtype=torch.float64)) * (torch.randint(0, 2, (GIVEN_CLAMP_CELLS,), generator=g).double() * 2 - 1)
    b = a / k * (torch.randint(0, 2, (GIVEN_CLAMP_CELLS,), generator=g).double() * 2 - 1)
    swap = torch.randint(0, 2, (GIVEN_CLAMP_CELLS,), generator=g).bool()
    n1[cells], n2[cells] = torch.where(swap, b, a), torch.where(swap, a, b)
    base = -n1[cells] * uv[:, 0] - n2[cells] * uv[:, 1]
    norm = torch.sqrt(n1[cells] ** 2 + n2[cells] ** 2 + base ** 2) if case.normalize else 1.0
    n3[cells] = t * norm + base
    n1[0] = n2[0] = n3[0] = 0.0
    n4[0] = -3.0
    if case.normalize:
        f = 0.5 + 2.5 * torch.rand(n, generator=g, dtype=torch.float64)
        n1, n2, n3 = n1 * f, n2 * f, n3 * f
    return torch.stack([n1, n2, n3, n4], 1).float().view(B, h, w, 4).permute(0, 3, 1, 2).contiguous()


def _given_den(case, planes, dtype=torch.float64):
    p = planes.to(dtype)
    if case.normalize:
        p = torch.cat([F.normalize(p[:, :3], 2, 1), p[:, 3:4]], 1)
    return p, O.lpg_denominator(p, case.k)


def given_zones_ok(case, den):
    pos, neg, margin, tiny, zeros = zone_counts(den)
    a = den.double().abs()
    between = int(((a > ZONE_HI) & (a < ORDINARY)).sum())           # an ordinary pixel has |den| >= 1e-2
    return pos >= 16 and neg >= 16 and margin == 0 and tiny == 0 and between == 0 and zeros == case.k * case.k


def given_planes(case):
    """[B,4,h,w] fp32 (the kernel's input, un-normalised when case.normalize).  Ordinary cells: |n1|, |n2| in
    [0.15, 0.4], |n3| in [0.5, 1], every sign: |den| >= 0.1.  GIVEN_CLAMP_CELLS cells: n3 is solved so that one chosen
    pixel of the cell has den = t, 5e-5 <= |t| <= 7e-4 with alternating sign (times |n| when the kernel is to normalise).
    The slopes of such a cell keep its other pixels ordinary (see _given_try).  Cell 0: n1 = n2 = n3 = 0, n4 = -3: den == 0 exactly, no clamp applies to a zero, and
    O.lpg_forward gives n4 / 0 = -inf.  With normalize the first three rows are then scaled by a per-cell factor in
    [0.5, 3].  The construction is repeated with the next seed until the fp64 denominators of the fp32 planes meet
    given_zones_ok: the reference alone decides."""
    for attempt in range(50):
        planes = _given_try(case, 1000 + 17 * GIVEN_CASES.index(case) + 1000 * attempt)
        if given_zones_ok(case, _given_den(case, planes)[1]):
            return planes
    raise AssertionError("no seed meets the zones for " + case.name)


def given_reference(case, dtype=torch.float64):
    """{"planes" fp32 input, "plane" (normalised if asked) in dtype, "depth" [B,1,H,W], "den" [B,H,W], "abs_min"}."""
    def make():
        planes = given_planes(case)
        p, _ = _given_den(case, planes, dtype)
        depth, am = O.lpg_forward(p, case.k)
        return {"planes": planes, "plane": p, "depth": depth.unsqueeze(1) / MD, "den": O.lpg_denominator(p, case.k), "abs_min": am}
    return cached(("given", case.name, dtype), make)


def given_bound(case, ref):
    """Per pixel |got - ref| <= bound, and the bound of abs_min.  The reference reads the same fp32 planes, so this is
    rounding alone.  With s = max(|n1| / 2, |n2| / 2, |n3|, |den|):
      lean kernel (lpg_cell_outputs): base = fma(n2, v, n3) rounds at |base| <= 2 s, d = fma(n1, u, base) at |d| <= s
        (u, v and u0 + i / K are exact): |d - den| <= 3 U s.  Then d max_depth (U), the hardware reciprocal at 1 ulp
        (2 U), the product with n4 (U), and 1e-3f against 1e-3 on a clamped pixel (0.8 U): 5 U relative.
      general kernel: n1 u, n2 v, their sum and the sum with n3 round separately: (1/2 + 1/2 + 1 + 1) s + slack = 5 U s;
        two IEEE divisions and the clamp constant: 3 U, kept at 5 U.
      normalize (general kernel only): (n1^2 + n2^2) + n3^2 carries 2 U relative, its root 2 U, the division one more:
        each component 4 U relative, |n1 u| + |n2 v| + |n3| <= 2 s: 8 U s more.
    An un-clamped pixel divides by d: relative error 5 U + c U s / |den|; a clamped one divides by a constant: 5 U, the
    20 % margin keeping the decision.  x 1.01 for second order.  abs_min: min_i |d_i| against min_i |den_i| differ by at
    most max_i |d_i - den_i| = c U max s."""
    p, den = ref["plane"].double(), ref["den"].double()
    k = case.k
    up = lambda t: torch.repeat_interleave(torch.repeat_interleave(t, k, 1), k, 2)
    s = torch.maximum(torch.maximum(up(p[:, 0].abs() / 2), up(p[:, 1].abs() / 2)), torch.maximum(up(p[:, 2].abs()), den.abs()))
    c = DEN_ROUNDINGS[case.kernel] + (NORMALIZE_ROUNDINGS if case.normalize else 0.0)
    unclamped = (clamp_decisions(den) == 0) & (den != 0)
    rel = 5 * U + torch.where(unclamped, c * U * s / den.abs().clamp(min=1e-300), torch.zeros_like(den))
    return 1.01 * rel.unsqueeze(1) * ref["depth"].double().abs(), 1.01 * c * U * float(s.max())


# ------------------------------------------------------------------------------------------------ LPG backward
# bts_lpg_bwd_f32 at 2 x 9 x 31 = 558 cells: two full 256-thread blocks and 46 threads of a third.  |n1|, |n2| <= 0.5 and
# |n3| in [0.6, 1] of either sign keep |den| >= 0.16; cells 100 and 400 are n1 = n2 = 0, n3 = +-5e-4: clamped on every
# pixel, one of each sign; the output gradient over those two cells is scaled by 1e-3, so that their 1 / 1e-3 does not set
# the scale of d/dn4 and hide every other cell behind it.  Reference: fp64 autograd through O.lpg_forward.
BWD_KS = (1, 2, 4, 8)
BWD_SHAPE = (2, 9, 31)
BWD_CLAMPED = ((100, 5e-4), (400, -5e-4))
BWD_TODAY = 2e-5                    # the bar of tests/test_hip_ops.py::test_lpg_backward_vs_autograd


def bwd_case(k):
    B, h, w = BWD_SHAPE
    g = torch.Generator().manual_seed(500 + k)
    sgn = lambda: torch.randint(0, 2, (B, h, w), generator=g).float() * 2 - 1
    p = torch.empty(B, 4, h, w)
    p[:, 0] = torch.rand(B, h, w, generator=g) - 0.5
    p[:, 1] = torch.rand(B, h, w, generator=g) - 0.5
    p[:, 2] = (0.6 + 0.4 * torch.rand(B, h, w, generator=g)) * sgn()
    p[:, 3] = (1.0 + 40.0 * torch.rand(B, h, w, generator=g)) * sgn()
    for cell, n3 in BWD_CLAMPED:
        b, r = divmod(cell, h * w)
        p[b, :3, r // w, r % w] = torch.tensor([0.0, 0.0, n3])
    gout = torch.randn(B, h * k, w * k, generator=g)
    for cell, _ in BWD_CLAMPED:
        b, r = divmod(cell, h * w)
        gout[b, (r // w) * k:(r // w + 1) * k, (r % w) * k:(r % w + 1) * k] *= 1e-3
    return p, gout


def bwd_reference(k, dtype=torch.float64):
    def make():
        p, gout = bwd_case(k)
        pd = p.to(dtype).requires_grad_(True)
        y, _ = O.lpg_forward(pd, k)
        y.backward(gout.to(dtype))
        return {"plane": p, "gout": gout, "grad": pd.grad.detach(), "den": O.lpg_denominator(p.double(), k)}
    return cached(("bwd", k, dtype), make)


# ------------------------------------------------------------------------------------------------ floors
def _sig(v):
    return float("%.2e" % v)


def chain_floor(r64, r32, row):
    if row.final:
        return {"out": _sig(plane_errors(r32["out"], r64["out"])[0])}
    return {"planes0": [_sig(v) for v in plane_errors(r32["plane0"], r64["plane0"])],
            "planes1": [_sig(v) for v in plane_errors(r32["plane1"], r64["plane1"])],
            "depth": _sig(den_weighted_error(r32["depth"], r64["depth"], r64["den"]))}


def measure_floors(wrap=True):
    """The fp32 oracle against the fp64 oracle on the CPU, per case, in the metrics of the GPU test."""
    fl = {}
    for name, row in ROWS.items():
        fl[name] = chain_floor(row_reference(name), row_reference(name, torch.float32), row)
    fl["clamp"] = chain_floor(clamp_reference(), clamp_reference(torch.float32), CLAMP_ROW)
    if wrap:
        for case in WRAP_CASES:
            fl[case.name] = chain_floor(wrap_reference(case), wrap_reference(case, torch.float32), ROWS[case.row])
    for k in BWD_KS:
        fl["bwd_k%d" % k] = [_sig(v) for v in plane_errors(bwd_reference(k, torch.float32)["grad"], bwd_reference(k)["grad"])]
    return fl


# Measured by `python tests/reduc_lpg_cases.py` on the CPU.  fp32 sums depend on the host's BLAS blocking and thread
# count, so tests/test_reduc_lpg_cases_host.py accepts a re-measurement within a factor of two of these.
FLOORS = {
    'fwd_128x128': {'planes0': [8.93e-07, 9.48e-07, 7.45e-08, 2.03e-07], 'planes1': [8.93e-07, 9.48e-07, 7.78e-08, 2.03e-07], 'depth': 5.74e-07},
    'fwd_128x64': {'planes0': [6.98e-07, 6.37e-07, 1.43e-07, 2.55e-07], 'planes1': [6.98e-07, 6.37e-07, 1.43e-07, 2.55e-07], 'depth': 5.79e-07},
    'fwd_64x32': {'planes0': [5.78e-07, 6.63e-07, 8.14e-08, 1.6e-07], 'planes1': [5.78e-07, 6.63e-07, 9.31e-08, 1.6e-07], 'depth': 8.4e-07},
    'fwd_64x64': {'planes0': [4.01e-07, 4.64e-07, 1.16e-07, 2.59e-07], 'planes1': [4.38e-07, 4.64e-07, 1.31e-07, 2.59e-07], 'depth': 5.6e-07},
    'fwd_32x16': {'planes0': [6.62e-07, 4.27e-07, 9.82e-08, 1.44e-07], 'planes1': [6.62e-07, 4.27e-07, 7.84e-08, 1.44e-07], 'depth': 6.31e-07},
    'fwd_32x16_final': {'out': 1.53e-07},
    'fwd_16x8_final': {'out': 9.15e-08},
    'lpg_128x128_k8': {'planes0': [8.93e-07, 9.48e-07, 7.45e-08, 2.03e-07], 'planes1': [8.93e-07, 9.48e-07, 7.78e-08, 2.03e-07], 'depth': 5.74e-07},
    'lpg_128x64_k4': {'planes0': [6.98e-07, 6.37e-07, 1.43e-07, 2.55e-07], 'planes1': [6.98e-07, 6.37e-07, 1.43e-07, 2.55e-07], 'depth': 5.79e-07},
    'lpg_64x32_k2': {'planes0': [5.78e-07, 6.63e-07, 8.14e-08, 1.6e-07], 'planes1': [5.78e-07, 6.63e-07, 9.31e-08, 1.6e-07], 'depth': 8.4e-07},
    'lpg_64x64_k8': {'planes0': [4.01e-07, 4.64e-07, 1.16e-07, 2.59e-07], 'planes1': [4.38e-07, 4.64e-07, 1.31e-07, 2.59e-07], 'depth': 5.6e-07},
    'lpg_64x32_k4': {'planes0': [5.78e-07, 6.63e-07, 8.14e-08, 1.6e-07], 'planes1': [5.78e-07, 6.63e-07, 9.31e-08, 1.6e-07], 'depth': 8.81e-07},
    'lpg_32x16_k2': {'planes0': [6.62e-07, 4.27e-07, 9.82e-08, 1.44e-07], 'planes1': [6.62e-07, 4.27e-07, 7.84e-08, 1.44e-07], 'depth': 6.31e-07},
    'clamp': {'planes0': [9.26e-06, 4.06e-06, 4.79e-06, 2.4e-07], 'planes1': [9.26e-06, 4.06e-06, 4.79e-06, 2.4e-07], 'depth': 8.67e-06},
    'wrap_wide_k8': {'planes0': [1.36e-06, 1.73e-06, 1.05e-07, 4.54e-07], 'planes1': [1.36e-06, 1.73e-06, 1.12e-07, 4.54e-07], 'depth': 1.42e-06},
    'wrap_narrow_k2': {'planes0': [1.03e-06, 1.45e-06, 2.37e-07, 2.91e-07], 'planes1': [1.03e-06, 1.43e-06, 2.37e-07, 2.91e-07], 'depth': 1.14e-06},
    'wrap_final': {'out': 1.64e-07},
    'bwd_k1': [0.0, 0.0, 3.85e-08, 5.55e-08],
    'bwd_k2': [7.01e-08, 7.45e-08, 8.29e-08, 8.38e-08],
    'bwd_k4': [8.6e-08, 1.14e-07, 7.88e-08, 6.64e-08],
    'bwd_k8': [1.57e-07, 9.38e-08, 1.35e-07, 8.5e-08],
}


if __name__ == "__main__":
    print("FLOORS = {")
    for name, v in measure_floors().items():
        print("    %r: %r," % (name, v))
    print("}")
