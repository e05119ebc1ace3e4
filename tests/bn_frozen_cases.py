"""Cases, fp64 statements and bounds of the frozen-statistics norm kernels (csrc/bn_train.hip: bn_frozen_vectors_kernel,
bn_frozen_bwd_kernel) and the seeds of the training-node cases run with frozen norm layers.
tests/test_bn_frozen_host.py asserts on the CPU what the designs rely on; tests/test_bn_frozen_gpu.py and
tests/test_train_frozen_norm_gpu.py run the kernels and the nodes against these statements.  No bound here was read off
the kernel: each counts the roundings of the expression it bounds.

Borrowed private helpers (existing test modules stay as they are, so they are used under their own names): stream_cases._gen
and stream_cases._ints -- the seeded generator and integer draw that bn_bwd_case itself uses, so dx_old comes from the same
family of streams -- and train_node_cases._kink_of_records, the (m, d) reduction behind train_node_cases.kink.

Backward: stream_cases.bn_bwd_case (integer x, dy in [-8, 8], scale a signed power of two in {0.5, 1, 2}) plus an integer
dx_old in [-8, 8].  scale * dy' is a multiple of 0.5 of magnitude <= 16 and dx_old + scale * dy' one of magnitude <= 24:
both exact in fp32, fused or not, so dx is compared bit for bit.  The sums are the exact integer-design sums of
stream_cases.bn_bwd_ref (torch.equal)."""
import torch

import stream_cases as sc

U = 2.0 ** -24                       # one fp32 rounding, relative

BWD_SHAPES = [s for s, _ in sc.BN_SHAPES] + [sc.BN_GRID_STRIDE]
BWD_FORMS = ("dx", "dx_sums", "sums", "accumulate", "accumulate_sums", "shared")


def frozen_bwd_case(npix, C):
    """stream_cases.bn_bwd_case plus dx_old: (x, dy, mean, invstd, scale, shift, dx_old)."""
    return sc.bn_bwd_case(npix, C) + (sc._ints(sc._gen(npix, C, 21), -8, 8, (npix, C)),)


def frozen_bwd_ref(x, dy, mean, invstd, scale, shift, dx_old, relu):
    """fp64: dbeta, dgamma as stream_cases.bn_bwd_ref; dx = scale * dy', dx_acc = dx_old + scale * dy'."""
    r = sc.bn_bwd_ref(x, dy, mean, invstd, scale, shift, relu)
    dx = scale.double() * r["g"]
    return dict(dbeta=r["dbeta"], dgamma=r["dgamma"], dx=dx, dx_acc=dx_old.double() + dx, g=r["g"], z=r["z"], xhat=r["xhat"])


# ------------------------------------------------------------------------------------------------------- vectors
VEC_C = (4, 8, 44, 132, 2208)
VEC_EPS = (1e-5, 1.1e-5)


def frozen_vectors_case(C, salt=0):
    """(gamma, beta, running_mean, running_var): gamma and running_var in [0.5, 1.5], beta and running_mean N(0, 1);
    channel 1 has var = 0 and channel 2 var = 1e-12 (invstd = 1/sqrt(eps) territory)."""
    g = sc._gen(C, 80 + salt)
    gamma = (0.5 + torch.rand(C, generator=g)).float()
    beta = torch.randn(C, generator=g).float()
    rm = torch.randn(C, generator=g).float()
    rv = (0.5 + torch.rand(C, generator=g)).float()
    rv[1], rv[2] = 0.0, 1e-12
    return gamma, beta, rm, rv


def frozen_vectors_ref(gamma, beta, rm, rv, eps):
    """fp64 on the same fp32 values (eps as the fp32 number the entry point receives): {mean, invstd, scale, shift} and a
    per-element bound for each.  Roundings of the fp32 evaluation, each at most U relative (sqrtf and the division are
    correctly rounded without fast-math; a fused multiply-add only removes roundings):
      invstd = 1 / sqrt(var + eps)   : the sum (U, halved by the square root), the square root, the reciprocal   <= 3 U
      scale  = g * invstd            : + one product (none when g is absent)                                     <= 4 U
      shift  = b - (mean * g) * invstd: the product carries invstd's 3 U and two products (one without g), the difference
                                       one rounding of the result                       <= 5 U |mean g invstd| + U |shift|
    every bound doubled for second-order terms.  mean is a copy: exact."""
    e = float(torch.tensor(eps, dtype=torch.float32))
    mean, var = rm.double(), rv.double()
    invstd = 1.0 / torch.sqrt(var + e)
    g = torch.ones_like(invstd) if gamma is None else gamma.double()
    b = torch.zeros_like(invstd) if beta is None else beta.double()
    scale = g * invstd
    prod = mean * g * invstd
    shift = b - prod
    bounds = dict(mean=torch.zeros_like(mean), invstd=2 * 3 * U * invstd.abs(), scale=2 * 4 * U * scale.abs(),
                  shift=2 * U * (5 * prod.abs() + shift.abs()))
    return dict(mean=mean, invstd=invstd, scale=scale, shift=shift), bounds


# ------------------------------------------------------------------------------------- training nodes, frozen norms
# train_node_cases.CASES run with every norm layer in eval mode: seed and the kink ratio m / d (train_node_cases.kink with
# bn_eval=True, 8 CPU threads).  The rule asks for >= 32; seeds searched here asked for >= 48.  d161, d121_tiny keep the
# stored seeds; rx_id and rn_ds were searched afresh at the 48 margin (the stored seeds give 36.4 and 33.9).
FROZEN_SEEDS = {"d121": 6, "d161": 9, "d121_tiny": 0, "rx_ds": 223, "rx_id": 28, "rn_ds": 20, "stem": 73, "daspp2": 10}
FROZEN_RATIOS = {"d121": 58.8, "d161": 38.9, "d121_tiny": 154.8, "rx_ds": 59.1, "rx_id": 48.9, "rn_ds": 53.6, "stem": 61.8,
                 "daspp2": 184.0}
FROZEN_STEP2_SEED = {"d121": 22}     # second-step parameters of d121 (seed 6) with frozen norms: ratio 61.1
MIXED_SEED = {"d121": 29}            # denselayer1's norms frozen, the rest in train() mode: ratio 79.6
MIXED_FROZEN_LAYERS = ("denselayer1",)


def kink_mixed(c):
    """train_node_cases.kink for the mixed block: (m, d, number of hooked tensors)."""
    import train_node_cases as T
    recs = []
    for dtype in (torch.float64, torch.float32):
        rec = dict(relu=[], pool=[])
        T.reference_step(c, set_mixed(T.twin(c, dtype)), rec=rec)
        recs.append(rec)
    return T._kink_of_records(*recs)


def set_mixed(module):
    """The norm layers of MIXED_FROZEN_LAYERS in eval mode, every other layer as it is."""
    for name in MIXED_FROZEN_LAYERS:
        for m in module[name].modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                m.eval()
    return module
