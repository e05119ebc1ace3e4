"""Case table and plain fp64 CPU statements for the streaming kernels around the MFMA ones: csrc/bn_train.hip, pool.hip,
layout.hip, tail.hip and the tap-sum stage of upconv.hip.  tests/test_stream_cases_host.py asserts on the CPU what the
designs below rely on (chunk counts, exactness of the integer designs, coverage, grid-stride sizes);
tests/test_stream_kernels_gpu.py runs the kernels against these statements.

Integer designs: operands are small integers and powers of two, so that every product and every partial sum is exactly
representable in fp32 -- the order of a reduction, an FMA contraction or a different vector width cannot change a bit,
and the comparison is torch.equal."""
import os
import re

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "bts_amd", "csrc")
THREADS = 256                       # block size of every grid-stride kernel here
FOCAL_UNIT = 715.0873               # bts.py:291


def _gen(*key):
    g = torch.Generator()
    seed = 12345
    for k in key:
        seed = (seed * 1000003 + int(k)) % (2 ** 31 - 1)
    g.manual_seed(seed)
    return g


def _ints(g, lo, hi, shape):
    """Uniform integers in [lo, hi] as fp32."""
    return torch.randint(lo, hi + 1, shape, generator=g).float()


def _choice(g, values, n):
    return torch.tensor(values, dtype=torch.float32)[torch.randint(0, len(values), (n,), generator=g)]


def ulp32(v):
    """Spacing of fp32 at |v| (elementwise), as fp64."""
    a = v.abs().float()
    return (torch.nextafter(a, torch.full_like(a, float("inf"))) - a).double()


# --------------------------------------------------------------------------------------------------- block caps
def block_caps():
    """{source file: the block cap of its grid-stride launches}, read out of the sources."""
    def text(name):
        with open(os.path.join(CSRC, name)) as f:
            return f.read()
    m = re.search(r"b > (\d+) \? (\d+) :", text("bn_train.hip"))
    assert m and m.group(1) == m.group(2), "bn_train.hip: elem_blocks cap not found"
    caps = {"bn_train.hip": int(m.group(1))}
    for name in ("pool.hip", "layout.hip", "tail.hip", "upconv.hip"):
        found = {int(a) * int(b) for a, b in re.findall(r"blocks > (\d+)L \* (\d+)\) blocks = ", text(name))}
        assert len(found) == 1, "%s: expected one block cap, found %s" % (name, sorted(found))
        caps[name] = found.pop()
    return caps


# ------------------------------------------------------------------------------------------------------ BN-train
# (npix, C) -> chunks of plan_chunks (csrc/bn_train.hip): 1 chunk; 2 with a ragged last one; the 8 / 16 / 32-lane kernels
# with a partial last channel group; up to 24 chunks = the finalize kernel's remainder walk alone; 25 = the first count at
# which `k + 24 < nchunks` holds (lane 0 only, no remainder step after it); 33 = every lane takes one unrolled trip and
# lane 0 a remainder step after it; 1024 = the cap (32 unrolled trips per lane).  finalize_walk() restates the walk.
BN_SHAPES = [((2, 4), 1), ((33, 8), 1), ((64, 32), 1), ((65, 32), 2), ((70, 48), 2), ((129, 44), 3), ((515, 108), 9),
             ((577, 112), 10), ((1537, 132), 25), ((1601, 64), 26), ((2049, 8), 33), ((3650, 16), 58), ((12, 2208), 1),
             ((98304, 8), 1024)]
BN_GRID_STRIDE = (16500, 512)       # npix * C / 4 threads' worth of work > cap * 256: a second grid-stride trip
BN_EPS = 1e-5
BN_EXTRA = 8                        # channels a test buffer is wider than C; the slice sits at channel BN_EXTRA // 2
def finalize_walk(nchunks):
    """bn_stats_finalize_kernel's walk over the chunk partials, per lane 0..7: (chunks read by the 4-way unrolled loop,
    chunks read by the remainder loop), in order."""
    out = []
    for lane in range(8):
        k, unrolled, rest = lane, [], []
        while k + 24 < nchunks:
            unrolled += [k, k + 8, k + 16, k + 24]
            k += 32
        while k < nchunks:
            rest.append(k)
            k += 8
        out.append((unrolled, rest))
    return out


def lanes_for(C):
    """float4 lanes per pixel row of the two reduce kernels (csrc/bn_train.hip: lanes_for)."""
    return 32 if C >= 112 else (16 if C >= 48 else 8)


STATS_KINDS = ("gauss", "cancel")
STATS_KEYS = ("mean", "invstd", "scale", "shift", "running_mean", "running_var")


def bn_stats_input(npix, C, kind):
    """(x [npix, C] fp32, gamma, beta, running_mean, running_var).  "gauss": mean 0.4, std 1.7.  "cancel": a per-channel
    offset near 1000 and std 0.01 -- E[x^2] - E[x]^2 in fp32 has no correct digit there."""
    g = _gen(npix, C, STATS_KINDS.index(kind))
    if kind == "gauss":
        x = 0.4 + 1.7 * torch.randn((npix, C), generator=g, dtype=torch.float64)
    else:
        off = 1000.0 + torch.randint(-50, 51, (C,), generator=g).double()
        x = off + 0.01 * torch.randn((npix, C), generator=g, dtype=torch.float64)
    gamma = (0.5 + torch.rand(C, generator=g)).float()
    beta = torch.randn(C, generator=g).float()
    rm = torch.randn(C, generator=g).float()
    rv = (0.5 + torch.rand(C, generator=g)).float()
    return x.float(), gamma, beta, rm, rv


def bn_stats_statement(x, gamma, beta, rm, rv, momentum, dtype, eps=BN_EPS):
    """nn.BatchNorm2d.train() on rows [npix, C], plain two-pass, every operation in `dtype` on the same fp32 values:
    {mean, invstd, scale, shift, running_mean, running_var, m2}.  gamma / beta None = 1 / 0; rm / rv None = absent."""
    x = x.to(dtype)
    n = x.shape[0]
    mean = x.sum(0) / n
    d = x - mean
    m2 = (d * d).sum(0)
    var = m2 / n
    invstd = 1.0 / torch.sqrt(var + eps)
    scale = invstd if gamma is None else gamma.to(dtype) * invstd
    shift = -mean * scale if beta is None else beta.to(dtype) - mean * scale
    out = dict(mean=mean, invstd=invstd, scale=scale, shift=shift, m2=m2)
    if rm is not None:
        out["running_mean"] = (1.0 - momentum) * rm.to(dtype) + momentum * mean
    if rv is not None:
        out["running_var"] = (1.0 - momentum) * rv.to(dtype) + momentum * (m2 / (n - 1) if n > 1 else var)
    return out


def bn_stats_floor(x, gamma, beta, rm, rv, momentum):
    """(ref64, E32, tol): the fp64 statement; per quantity the largest error over the channels of the fp32 two-pass
    statement against it; and the per-channel tolerance of the kernel, max(4 * E32, 2 ulp of the value's magnitude) --
    the 4x is for the kernel's different summation tree."""
    r64 = bn_stats_statement(x, gamma, beta, rm, rv, momentum, torch.float64)
    r32 = bn_stats_statement(x, gamma, beta, rm, rv, momentum, torch.float32)
    e32 = {k: float((r32[k].double() - r64[k]).abs().max()) for k in STATS_KEYS if k in r64}
    tol = {k: torch.clamp(2.0 * ulp32(r64[k]), min=4.0 * e32[k]) for k in e32}
    return r64, e32, tol


APPLY_SCALES = (-2.0, -1.0, -0.5, 0.5, 1.0, 2.0)


def bn_apply_case(npix, C, salt=0):
    """x integers in [-64, 64], scale in {+-0.5, +-1, +-2}, integer shift: x*scale + shift is exact with or without FMA."""
    g = _gen(npix, C, 10 + salt)
    return _ints(g, -64, 64, (npix, C)), _choice(g, APPLY_SCALES, C), _ints(g, -8, 8, (C,))


def bn_apply_ref(x, scale, shift, relu):
    y = x.double() * scale.double() + shift.double()
    return y.clamp_min(0.0) if relu else y


def bn_bwd_case(npix, C):
    """(x, dy, mean, invstd, scale, shift): integer x, dy in [-8, 8], integer mean, invstd in {1/4, 1/2, 1}, scale a signed
    power of two, integer shift = -scale * k with k even: the pre-activation x*scale + shift is exactly 0 wherever x == k."""
    g = _gen(npix, C, 20)
    x, dy = _ints(g, -8, 8, (npix, C)), _ints(g, -8, 8, (npix, C))
    mean = _ints(g, -2, 2, (C,))
    invstd = _choice(g, (0.25, 0.5, 1.0), C)
    scale = _choice(g, APPLY_SCALES, C)
    shift = -scale * 2.0 * _ints(g, -3, 3, (C,))
    return x, dy, mean, invstd, scale, shift


def bn_bwd_ref(x, dy, mean, invstd, scale, shift, relu):
    """fp64: g = dy masked by z > 0 (z = x*scale + shift; relu only), xhat, dbeta = sum g, dgamma = sum g*xhat,
    dx = scale*(g - dbeta/n - xhat*dgamma/n) and the elementwise bound of dx's fp32 evaluation.  The expression has 8
    roundings (1/n, the two means, xhat * mean, the two differences, the product with scale; x - mean and * invstd are
    exact in this design), each at most 2^-24 relative to a partial result no larger than the sum of magnitudes below;
    doubled for second-order terms: 16 * 2^-24 * |scale| * (|g| + |dbeta|/n + |xhat| |dgamma|/n)."""
    xd, g = x.double(), dy.double()
    n = x.shape[0]
    z = xd * scale.double() + shift.double()
    if relu:
        g = torch.where(z > 0, g, torch.zeros_like(g))
    xhat = (xd - mean.double()) * invstd.double()
    dbeta, dgamma = g.sum(0), (g * xhat).sum(0)
    dx = scale.double() * (g - dbeta / n - xhat * (dgamma / n))
    bound = 16.0 * 2.0 ** -24 * scale.double().abs() * (g.abs() + dbeta.abs() / n + xhat.abs() * dgamma.abs() / n)
    return dict(z=z, g=g, xhat=xhat, dbeta=dbeta, dgamma=dgamma, dx=dx, bound=bound,
                abs_sums=(g.abs().sum(0), (g * xhat).abs().sum(0)))


# ------------------------------------------------------------------------------------------------------- pooling
MAXPOOL_SHAPES = [(1, 1, 1, 4), (2, 1, 7, 8), (2, 6, 1, 8), (1, 2, 2, 4), (2, 9, 14, 24), (1, 8, 8, 132)]
AVGPOOL_SHAPES = [(1, 2, 2, 4), (2, 8, 14, 24), (3, 4, 6, 132)]
POOL_GRID_STRIDE = (1, 130, 130, 1024)              # (B, h, w, C): outputs / 4 > cap * 256 for both pooling kernels


def maxpool_case(B, h, w, C):
    """Distinct integers (|v| < 2^24): a maximum taken over a wrong window cannot hit the right value by accident."""
    n = B * h * w * C
    return (torch.randperm(n, generator=_gen(B, h, w, C, 30)) - n // 2).float().view(B, h, w, C)


def maxpool_ref(x):
    return F.max_pool2d(x.double().permute(0, 3, 1, 2), 3, 2, 1).permute(0, 2, 3, 1).contiguous()


def avgpool_case(B, h, w, C):
    g = _gen(B, h, w, C, 31)
    return _ints(g, -64, 64, (B, h, w, C)), _choice(g, APPLY_SCALES, C), _ints(g, -8, 8, (C,))


def avgpool_ref(x, scale, shift):
    z = (x.double() * scale.double() + shift.double()).clamp_min(0.0)
    return 0.25 * (z[:, 0::2, 0::2] + z[:, 0::2, 1::2] + z[:, 1::2, 0::2] + z[:, 1::2, 1::2])


# -------------------------------------------------------------------------------------------------------- layout
LAYOUT_C = (1, 2, 3, 4, 5, 31, 32, 33, 37, 64)
LAYOUT_HW = (1, 31, 32, 33, 45)
LAYOUT_B = (1, 3)
LAYOUT_GRID_STRIDE = (1, 1050000)                   # (B, HW) of the C <= 4 kernel: B * HW > cap * 256


def layout_case(B, C, HW):
    """[B, C, 1, HW] fp32 of both signs, with -0.0 and +0.0 sprinkled in."""
    g = _gen(B, C, HW, 40)
    x = torch.randn((B, C, 1, HW), generator=g)
    r = torch.rand((B, C, 1, HW), generator=g)
    x[r < 0.1] = -0.0
    x[r > 0.95] = 0.0
    if x.numel() > 1:
        x.view(-1)[0], x.view(-1)[-1] = -0.0, -1.5
    return x


def bits(t):
    return t.contiguous().view(torch.int32)


# ---------------------------------------------------------------------------------------------------- depth tail
DEPTH_C = (32, 16)
DEPTH_W = (8, 16, 136)
DEPTH_H = (1, 2, 3, 34, 35)
DEPTH_B = 2
DEPTH_MAX = {32: 80.0, 16: 10.0}
DEPTH_FOCAL = (518.8579, 721.5377)                  # one per frame
DEPTH_EXACT_ACC = 8                                 # |pre-activation| up to which the logit recovers the integer exactly
DEPTH_CASES = [(C, H, W) for C in DEPTH_C for H in DEPTH_H for W in DEPTH_W]


def depth_case(C, H, W):
    """(iconv1 [B,C,H,W] of +-1 at 2 % density, weight [1,C,3,3] of integers in [-2, 2], acc [B,1,H,W] fp64 = the
    zero-padded 3x3 stencil, an exact small integer)."""
    g = _gen(C, H, W, 50)
    shape = (DEPTH_B, C, H, W)
    x = (torch.rand(shape, generator=g) < 0.02).float() * (2.0 * torch.randint(0, 2, shape, generator=g).float() - 1.0)
    w = _ints(g, -2, 2, (1, C, 3, 3))
    return x, w, F.conv2d(x.double(), w.double(), padding=1)


def depth_ref(acc, max_depth, focal):
    v = max_depth * torch.sigmoid(acc)
    return v if focal is None else v * focal.double().view(-1, 1, 1, 1) / FOCAL_UNIT


def depth_recover(out, max_depth, focal):
    """The integer pre-activation back out of a depth: round(logit(out * 715.0873 / (max_depth * focal))) in fp64."""
    t = out.double() / max_depth
    if focal is not None:
        t = t * FOCAL_UNIT / focal.double().view(-1, 1, 1, 1)
    return torch.round(torch.log(t) - torch.log1p(-t))


PACK_N = (1, 2, 3, 4)
PACK_NPIX = (1, 255, 257)
PACK_GRID_STRIDE = 1050000                          # npix > cap * 256


def pack_case(n, npix):
    return [_ints(_gen(n, npix, 60 + i), -1000, 1000, (npix,)) for i in range(n)]


# ------------------------------------------------------------------------------------------------ upconv_combine
COMBINE_SHAPES = [(1, 1, 1, 4), (2, 1, 5, 8), (2, 4, 1, 8), (2, 3, 5, 36)]
COMBINE_GRID_STRIDE = (1, 64, 66, 512)              # 4*B*h*w*c/4 > cap * 256 ((1,64,64,512) is exactly the cap: no second trip)
COMBINE_PAD = 8                                     # taps_pix_stride = 9c + COMBINE_PAD, NaN in the padding columns
ELU_ABS_TOL = 1e-6                                  # common.h states <= 1e-7 absolute for elu1; 10x margin


def combine_case(B, h, w, c):
    """(taps [B*h*w, 9c] integers in [-8, 8], e2 scale in {+-0.5, +-1}, integer e2 shift in [-3, 3])."""
    g = _gen(B, h, w, c, 70)
    return _ints(g, -8, 8, (B * h * w, 9 * c)), _choice(g, (-1.0, -0.5, 0.5, 1.0), c), _ints(g, -3, 3, (c,))


def combine_ref(taps, B, h, w, c, act, e2):
    """The fp64 sum of upconv.hip's header comment: (y [B,2h,2w,c], v = the sum before activation and e2).
    y[2Y+py][2X+px][n] = sum_{ky,kx} P[Y + d(py,ky)][X + d(px,kx)][(3ky+kx)c + n], d(0,.) = (-1,0,0), d(1,.) = (0,0,+1),
    zero outside the source map; act 0 none, 1 ReLU, 2 ELU; then v*scale + shift."""
    P = F.pad(taps.double().view(B, h, w, 9, c), (0, 0, 0, 0, 1, 1, 1, 1))
    d = ((-1, 0, 0), (0, 0, 1))
    v = torch.zeros((B, 2 * h, 2 * w, c), dtype=torch.float64)
    for py in range(2):
        for px in range(2):
            for ky in range(3):
                for kx in range(3):
                    y0, x0 = 1 + d[py][ky], 1 + d[px][kx]
                    v[:, py::2, px::2] += P[:, y0:y0 + h, x0:x0 + w, 3 * ky + kx]
    y = v
    if act == 1:
        y = v.clamp_min(0.0)
    elif act == 2:
        y = torch.where(v > 0, v, torch.expm1(v))
    if e2 is not None:
        y = y * e2[0].double() + e2[1].double()
    return y, v
