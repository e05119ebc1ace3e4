"""GPU: the native AdamW step (csrc/optim.hip, bts_amd/optim.py).

Yardstick of the update: the four formulas of the kernel's header evaluated in fp64 on the CPU from the same fp32 inputs.
Floor: torch.optim.AdamW(foreach=False, fused=False) in fp32 on the CPU against that fp64 run, per tensor, max-abs, for p,
exp_avg and exp_avg_sq.  Bar: 4 x the floor per tensor (the project's usual margin over a same-precision CPU run).  The
kernel rounds m and v exactly as ATen's CPU lerp_ / addcmul_ do (one fused multiply-add each), so on those it sits ON the
floor; p differs from the CPU's in the order of the last two roundings of the update only.

Packs: after every step each destination equals a fresh bts_pack_weights_f32 of the updated parameter bit for bit, padding
included, and every float outside the planned extents of p / m / v / the destinations keeps its poison bits.  A fresh pack
is the pack kernel's word, so each destination is also held against the plain statement of tests/pack_cases.py, and the ABI
test runs a second time with the destinations' padding poisoned: the step writes the real elements and nothing else."""
import copy
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import adamw_cases as AC
import pack_cases as PC
from bts_amd import _lib, synth
from parity_util import Params, t as as_tensor

pytestmark = pytest.mark.gpu

LR, EPS, BETAS, WDS = 1e-4, 1e-3, (0.9, 0.999), (1e-2, 0.0)
MAGS = (1e-6, 1e-3, 1.0)                     # gradient magnitude of the three consecutive steps
POISON = 0x7FA5A5A5                          # a NaN with a recognisable payload
GUARD = 64                                   # floats between two regions of an arena (a multiple of 4: keeps 16-byte lines)


@pytest.fixture(autouse=True)
def _packer_trust_is_reset():
    """The training step's packer is process-wide: leave it as a torch optimiser would (versions not trusted), so later
    tests that step a raw torch optimiser see the parent's behaviour."""
    yield
    from bts_amd import train
    train._PACKER.versions_trusted = False


def _fp64_step(p, g, m, v, wd, step):
    b1, b2 = BETAS
    step_size = LR / (1.0 - b1 ** step)
    inv_sqrt_bc2 = 1.0 / (1.0 - b2 ** step) ** 0.5
    p = p * (1.0 - LR * wd)
    m = m + (g - m) * (1.0 - b1)
    v = b2 * v + (1.0 - b2) * g * g
    p = p - step_size * m / (v.sqrt() * inv_sqrt_bc2 + EPS)
    return p, m, v


@pytest.fixture(scope="module")
def ref():
    """Inputs, the fp64 yardstick and the fp32 CPU floor of three steps over every case, computed once."""
    span = int(_lib.load_real().bts_adamw_flat_span())
    cases = AC.cases(span)
    gen = torch.Generator().manual_seed(20240607)
    p0 = [torch.randn(shape, generator=gen) * 0.5 for _, shape, _ in cases]
    grads = [[torch.randn(shape, generator=gen) * mag for _, shape, _ in cases] for mag in MAGS]
    group = [i % 2 for i in range(len(cases))]
    params = [torch.nn.Parameter(p.clone()) for p in p0]
    opt = torch.optim.AdamW([{"params": [q for q, gi in zip(params, group) if gi == k], "weight_decay": WDS[k]} for k in (0, 1)],
                            lr=LR, eps=EPS, betas=BETAS, foreach=False, fused=False)
    p64 = [p.double() for p in p0]
    m64 = [torch.zeros_like(p) for p in p64]
    v64 = [torch.zeros_like(p) for p in p64]
    want, floor = [], []
    for s in range(3):
        for q, g in zip(params, grads[s]):
            q.grad = g.clone()
        opt.step()
        fl = []
        for i in range(len(cases)):
            p64[i], m64[i], v64[i] = _fp64_step(p64[i], grads[s][i].double(), m64[i], v64[i], WDS[group[i]], s + 1)
            st = opt.state[params[i]]
            fl.append(dict(p=(params[i].detach().double() - p64[i]).abs().max().item(),
                           m=(st["exp_avg"].double() - m64[i]).abs().max().item(),
                           v=(st["exp_avg_sq"].double() - v64[i]).abs().max().item()))
        want.append(dict(p=[x.clone() for x in p64], m=[x.clone() for x in m64], v=[x.clone() for x in v64]))
        floor.append(fl)
    return SimpleNamespace(span=span, cases=cases, p0=p0, grads=grads, group=group, want=want, floor=floor)


def _check_against_fp64(ref, s, i, got, what=""):
    """got = dict(p, m, v) of case i after step s (0-based); prints every figure, then asserts 4 x the floor."""
    name = ref.cases[i][0]
    for k in ("p", "m", "v"):
        err = (got[k].detach().double().cpu().reshape(-1) - ref.want[s][k][i].reshape(-1)).abs().max().item()
        fl = ref.floor[s][i][k]
        print("adamw %s step %d %-18s %s: gpu err %.3e  cpu fp32 floor %.3e  |x|max %.3e" % (
            what, s + 1, name, k, err, fl, ref.want[s][k][i].abs().max().item()))
        assert err <= 4.0 * fl, (what, s + 1, name, k, err, fl)


# ------------------------------------------------------------------------------------------------ the C ABI on raw buffers
class _Arena:
    """A poisoned device buffer with regions carved out of it; `inside` marks the floats some region owns."""

    def __init__(self):
        self.cursor = GUARD
        self.regions = []

    def carve(self, n, off=0):
        start = self.cursor + off
        self.regions.append((start, n))
        self.cursor = AC.round_up(start + n, 4) + GUARD
        return start

    def alloc(self):
        self.bits = torch.full((self.cursor,), POISON, dtype=torch.int32, device="cuda")
        self.f = self.bits.view(torch.float32)
        inside = torch.zeros(self.cursor, dtype=torch.bool)
        for s, n in self.regions:
            inside[s:s + n] = True
        self.outside = (~inside).cuda()
        assert self.f.data_ptr() % 256 == 0

    def ptr(self, start):
        return self.f.data_ptr() + 4 * start

    def untouched_outside(self):
        return bool((self.bits[self.outside] == POISON).all())


def _fresh_pack(w4d, mode):
    """[rows_pad][k_pad] of a dense OIHW tensor by the ordinary pack launch (a packer of its own: nothing is cached)."""
    from bts_amd import train
    ld = AC.pack_geometry(tuple(w4d.shape), mode)[2]
    return train.WeightPacker().get(w4d, ld, mode)


def _statement(w4d, mode):
    """int32 bits [rows_pad][k_pad] and the real-element mask of a dense weight's pack, from tests/pack_cases.py."""
    shape = tuple(w4d.shape)
    row = PC.dense_row(shape, mode, AC.pack_geometry(shape, mode)[2])
    return torch.from_numpy(PC.dense_statement(w4d, row).view(np.int32)), torch.from_numpy(PC.real_mask(row))


def _assert_entry_is_the_statement(key, e, what):
    """A live packer entry (dense, bundled or native) against the statement of its parameter's current values."""
    w = e["wref"]().detach().cpu()
    rows = PC.table_rows(PC.Case("", tuple(key[1]), key[4], key[3], key[2], None))
    assert rows == [tuple(r) for r in e["rows"]], (what, key[1:])
    want = PC.statement(w, rows, tuple(e["dst"].shape), key[4])
    assert np.array_equal(e["dst"].cpu().view(torch.int32).numpy(), want), (what, key[1:])


def _offsets(ref, name):
    """Float offsets of (p, g, m, v) from a 16-byte line: one record with all four 4 bytes off (16 B per lane after a
    3-float head), one with only p off (one element per lane), and the 5-float record as one head element + one group."""
    return {"flat%d" % (ref.span + 1): (1, 1, 1, 1), "flat%d" % (ref.span - 1): (1, 0, 0, 0), "flat5": (3, 3, 3, 3)}.get(name, (0, 0, 0, 0))


def _build_state(ref, poison_pad=False):
    P, G, M, V, D = _Arena(), _Arena(), _Arena(), _Arena(), _Arena()
    regs = []
    for name, shape, modes in ref.cases:
        n = int(np.prod(shape))
        off = _offsets(ref, name)
        dst = []
        for mode in modes:
            _, _, _, rows_pad, k_pad = AC.pack_geometry(shape, mode)
            dst.append((D.carve(rows_pad * k_pad), rows_pad, k_pad))
        regs.append(SimpleNamespace(n=n, p=P.carve(n, off[0]), g=G.carve(n, off[1]), m=M.carve(n, off[2]), v=V.carve(n, off[3]), dst=dst))
    extra = P.carve(37)                                   # a parameter without a gradient: not part of the launch
    for a in (P, G, M, V, D):
        a.alloc()
    for r, p0, (_, shape, modes) in zip(regs, ref.p0, ref.cases):
        P.f[r.p:r.p + r.n] = p0.reshape(-1).cuda()
        M.f[r.m:r.m + r.n] = 0
        V.f[r.v:r.v + r.n] = 0
        G.f[r.g:r.g + r.n] = 0
        for (start, rows_pad, k_pad), mode in zip(r.dst, modes):
            D.f[start:start + rows_pad * k_pad] = _fresh_pack(p0.cuda(), mode).reshape(-1)
            if poison_pad:                                  # the step must write the real elements and nothing else
                pad = ~_statement(p0.view(shape), mode)[1].reshape(-1)
                D.bits[start:start + rows_pad * k_pad][pad.cuda()] = POISON
    P.f[extra:extra + 37] = 1.25
    ptrs = [(P.ptr(r.p), G.ptr(r.g), M.ptr(r.m), V.ptr(r.v), [D.ptr(s) for s, _, _ in r.dst]) for r in regs]
    items = AC.make_items(ref.cases, ptrs, ref.group)
    rc, total, plan, table = AC.plan(items)
    assert rc == 0
    nbytes = int(_lib.load_real().bts_adamw_table_bytes(len(items)))
    table_dev = torch.from_numpy(table[:nbytes].copy()).cuda()
    return SimpleNamespace(P=P, G=G, M=M, V=V, D=D, regs=regs, extra=extra, table_dev=table_dev, total=total, n=len(items))


def _launch(st, ref, s, skip=None):
    for r, g in zip(st.regs, ref.grads[s]):
        st.G.f[r.g:r.g + r.n] = g.reshape(-1).cuda()
    hy = (_lib.AdamwHyper * 2)()
    for k in (0, 1):
        hy[k].lr, hy[k].beta1, hy[k].beta2, hy[k].eps, hy[k].weight_decay, hy[k].step = LR, BETAS[0], BETAS[1], EPS, WDS[k], s + 1.0
    rc = _lib.load_real().bts_adamw_step_f32(st.table_dev.data_ptr(), st.n, st.total, C.addressof(hy), 2,
                                             skip.data_ptr() if skip is not None else None,
                                             torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    torch.cuda.synchronize()


def _snapshot(st):
    return [a.bits.clone() for a in (st.P, st.M, st.V, st.D)]


def _three_steps(ref, poison_pad):
    st = _build_state(ref, poison_pad)
    for s in range(3):
        _launch(st, ref, s)
        for i, (r, (name, shape, modes)) in enumerate(zip(st.regs, ref.cases)):
            got = dict(p=st.P.f[r.p:r.p + r.n], m=st.M.f[r.m:r.m + r.n], v=st.V.f[r.v:r.v + r.n])
            _check_against_fp64(ref, s, i, got, "abi")
            for (start, rows_pad, k_pad), mode in zip(r.dst, modes):
                fresh = _fresh_pack(got["p"].clone().view(shape), mode)
                assert fresh.shape == (rows_pad, k_pad)
                mine = st.D.f[start:start + rows_pad * k_pad].view(rows_pad, k_pad)
                want, real = _statement(got["p"].cpu().view(shape), mode)
                assert want.shape == (rows_pad, k_pad)
                assert torch.equal(fresh.cpu().view(torch.int32), want), (s + 1, name, mode, "the pack kernel against the statement")
                if poison_pad:
                    mine = mine.cpu().view(torch.int32)
                    assert torch.equal(mine[real], want[real]), (s + 1, name, mode)
                    assert bool((mine[~real] == POISON).all()), (s + 1, name, mode, "the step wrote padding")
                    continue
                assert torch.equal(mine.view(torch.int32), fresh.view(torch.int32)), (s + 1, name, mode)
                assert torch.equal(mine.cpu().view(torch.int32), want), (s + 1, name, mode)
        for a, what in ((st.P, "p"), (st.M, "m"), (st.V, "v"), (st.D, "packs"), (st.G, "g")):
            assert a.untouched_outside(), "step %d wrote outside the planned extents of %s" % (s + 1, what)
        assert bool((st.P.f[st.extra:st.extra + 37] == 1.25).all())


def test_three_steps_match_fp64_packs_are_exact_and_nothing_else_is_written(ref):
    _three_steps(ref, poison_pad=False)                   # destinations start as fresh packs: padding +0.0 before and after
    _three_steps(ref, poison_pad=True)                    # padding poisoned before the first step: still poison after each


def test_skip_leaves_every_byte_and_zero_equals_null(ref):
    st = _build_state(ref)
    _launch(st, ref, 2)                                   # some non-trivial state first
    before = _snapshot(st)
    for value in (1.0, -3.0, float("nan"), float("inf")):
        _launch(st, ref, 1, skip=torch.tensor([value], device="cuda"))
        for a, b in zip(before, _snapshot(st)):
            assert torch.equal(a, b), "skip = %r changed something" % value
    other = _build_state(ref)
    _launch(other, ref, 2)
    assert all(torch.equal(a, b) for a, b in zip(before, _snapshot(other)))       # bit-reproducible
    _launch(st, ref, 1, skip=torch.tensor([0.0], device="cuda"))
    _launch(other, ref, 1, skip=None)
    after = _snapshot(st)
    assert all(torch.equal(a, b) for a, b in zip(after, _snapshot(other)))
    assert not torch.equal(before[0], after[0])


# ------------------------------------------------------------------------------------------------ NativeAdamW + the packer
def _native_setup(ref):
    from bts_amd import train
    from bts_amd.optim import NativeAdamW
    params, keep = [], []
    for (name, shape, modes), p0 in zip(ref.cases, ref.p0):
        n = p0.numel()
        if name == "flat%d" % (ref.span + 1):               # 4 bytes off a 16-byte line
            buf = torch.zeros(n + 8, device="cuda")
            keep.append(buf)
            buf[1:1 + n] = p0.cuda()
            q = torch.nn.Parameter(buf[1:1 + n])
            assert q.data_ptr() % 16 == 4
        else:
            q = torch.nn.Parameter(p0.cuda())
        params.append(q)
        for mode in modes:
            train._PACKER.get(q, AC.pack_geometry(shape, mode)[2], mode)          # registered and packed once
    idle = torch.nn.Parameter(torch.full((37,), 1.25, device="cuda"))             # never gets a gradient
    groups = [{"params": [q for q, gi in zip(params, ref.group) if gi == k] + ([idle] if k == 1 else []), "weight_decay": WDS[k]}
              for k in (0, 1)]
    opt = NativeAdamW(groups, lr=LR, eps=EPS, betas=BETAS)
    return params, idle, opt, keep


def _check_native(ref, s, params, opt):
    from bts_amd import train
    for i, q in enumerate(params):
        stt = opt.state[q]
        assert stt["step"].device.type == "cpu" and float(stt["step"]) == s + 1
        _check_against_fp64(ref, s, i, dict(p=q, m=stt["exp_avg"], v=stt["exp_avg_sq"]), "native")
    mine = {id(e) for e in opt.attached}
    n_attached = 0
    for key, e in train._PACKER.entries.items():
        w = e["wref"]()
        if w is None or not any(w is q for q in params):
            continue
        assert id(e) in mine and e["version"] == w._version
        fresh = _fresh_pack(w.detach().clone(), key[3])
        assert torch.equal(e["dst"].view(torch.int32), fresh.view(torch.int32)), (s + 1, key[1], key[3])
        _assert_entry_is_the_statement(key, e, "native step %d" % (s + 1))
        n_attached += 1
    assert n_attached == sum(len(m) for _, _, m in ref.cases) == len(opt.attached)
    assert opt.unattached == []


def test_native_optimizer_follows_moved_gradients_and_reloaded_state_without_steady_uploads(ref):
    from bts_amd import train
    params, idle, opt, keep = _native_setup(ref)
    versions = [q._version for q in params]
    held = []
    for s in range(3):
        for q, g in zip(params, ref.grads[s]):
            q.grad = g.cuda()                               # new tensors every step; the old ones stay alive in `held`,
            held.append(q.grad)                             # so the addresses really differ
        if s > 0:
            assert all(a.data_ptr() != b.data_ptr() for a, b in zip(held[-len(params):], held[-2 * len(params):-len(params)]))
            opt.load_state_dict(copy.deepcopy(opt.state_dict()))                 # cloned state tensors at new addresses
        up = opt.uploads
        opt.step()
        assert opt.launches == 1 and opt.uploads == up + 1
        assert train._PACKER.versions_trusted is True
        _check_native(ref, s, params, opt)
        assert all(q._version > v0 for q, v0 in zip(params, versions))
        versions = [q._version for q in params]
        assert idle not in opt.state and idle._version == 0 and bool((idle == 1.25).all())
    up = opt.uploads
    for s in range(3):                                      # steady state: gradients rewritten in place, nothing moves
        for q, g in zip(params, ref.grads[s]):
            q.grad.copy_(g)
        opt.step()
    assert opt.uploads == up, "a steady step re-sent the table"
    assert all(float(opt.state[q]["step"]) == 6 for q in params)
    # a non-contiguous gradient is made contiguous, a ninth distinct (group, step) pair means a second launch
    w = params[-1]
    w.grad = torch.randn(tuple(reversed(w.shape)), device="cuda").permute(3, 2, 1, 0) if w.dim() == 4 else w.grad
    assert w.dim() != 4 or not w.grad.is_contiguous()
    for j, q in enumerate(params[:9]):
        opt.state[q]["step"].fill_(10 + j)
    opt.step()
    assert opt.launches == 2
    assert bool(torch.isfinite(w).all())


# ------------------------------------------------------------------------------------------------------------ in the model
def _model(enc, seed=4):
    from bts_amd import bts as M
    torch.manual_seed(seed)
    m = M.BtsModel(Params(enc, 512, 80.0, "kitti"))
    sd = {k: (torch.tensor(v) if np.ndim(v) == 0 else as_tensor(v))
          for k, v in synth.decoder_state(synth.ENCODER_CHANNELS[enc], 512, 0).items()}
    m.decoder.load_state_dict(sd, strict=True)
    return m.eval()


def _data():
    img = as_tensor(synth.image_batch(2, 64, 96, 11)).cuda()
    foc = as_tensor(synth.focal_values(2, "kitti", 11)).cuda()
    gt = (torch.rand(2, 1, 64, 96, generator=torch.Generator().manual_seed(5)) * 60 + 2).cuda()
    return img, foc, gt


def _live_entries(model):
    from bts_amd import train
    mine = {id(p) for p in model.parameters()}
    return [(key, e) for key, e in train._PACKER.entries.items() if e["wref"]() is not None and id(e["wref"]()) in mine]


def _assert_entries_current(entries, what):
    from bts_amd import train
    for key, e in entries:
        w = e["wref"]()
        fresh = train.WeightPacker().get(w.detach().clone(), key[2], key[3], key[4])
        assert torch.equal(e["dst"].view(torch.int32), fresh.view(torch.int32)), (what, key[1:])
        _assert_entry_is_the_statement(key, e, what)


def _train_run(enc, steps, native, freeze=False, base=None):
    """`steps` train_steps on a copy of `base`; returns losses, the eval depth before / after, and per-step records of
    the pack launch (which entries it covered) and of the library launches (kernel names)."""
    from bts_amd import bts as M, ops, train, trainer
    img, foc, gt = _data()
    m = copy.deepcopy(base).cuda()
    with torch.no_grad():
        before = m.eval()(img, foc)[4].clone()
    m.train()
    frozen = trainer.set_misc(m, enc) if freeze else []
    opt = trainer.make_optimizer(m, 1e-3, 1e-2, 1e-3, native=True) if native else trainer.make_optimizer(m, 1e-3, 1e-2, 1e-3, fused=False)
    crit = M.silog_loss(0.85)
    frozen_ps = [(n, p, p.detach().clone(), p._version) for n, p in m.encoder.named_parameters() if not p.requires_grad]
    assert bool(frozen_ps) == freeze
    losses, packed, kernels = [], [], []
    real_launch = train._PACKER._launch
    for s in range(steps):
        covered = []

        def spy(items, table, blocks, n_rows):
            covered.extend(items)
            return real_launch(items, table, blocks, n_rows)

        train._PACKER._launch = spy
        tr = ops.KernelTrace()
        ops.set_trace(tr)
        try:
            loss, _ = trainer.train_step(m, opt, crit, img, foc, gt)
        finally:
            ops.set_trace(None)
            train._PACKER._launch = real_launch
        losses.append(float(loss.detach()))
        packed.append(covered)
        kernels.append([r[0] for r in tr.records] + [r[1] for r in tr.records])
        if native:
            # right after the step every entry is current except those the optimiser reports as unattached (they wait for
            # the next forward's pack launch): with the stem frozen that is every registered entry of the model
            entries = _live_entries(m)
            waiting = {id(e) for e in opt.unattached}
            assert {id(e) for e in opt.attached} <= {id(e) for _, e in entries}
            _assert_entries_current([(k, e) for k, e in entries if id(e) not in waiting], "right after step %d" % (s + 1))
    if native:
        train.begin_step()                                  # what the next forward does first
        _assert_entries_current(_live_entries(m), "every entry, at the next forward")
    for n, p, was, ver in frozen_ps:
        assert torch.equal(p.detach().view(torch.int32), was.view(torch.int32)) and p._version == ver, n
    with torch.no_grad():
        after = m.eval()(img, foc)[4].clone()
    return SimpleNamespace(model=m, opt=opt, losses=losses, before=before, after=after, packed=packed, kernels=kernels, frozen=frozen)


def _assert_same_training(a, b):
    assert abs(a.losses[0] - b.losses[0]) <= 1e-6 * abs(a.losses[0]), (a.losses, b.losses)
    for x, y in zip(a.losses, b.losses):
        assert abs(x - y) <= 2e-3 * abs(x), (a.losses, b.losses)
    assert all(b.losses[i + 1] != b.losses[i] for i in range(len(b.losses) - 1)), "the loss never moved"
    err = (a.after - b.after).abs().max().item() / a.after.abs().max().item()
    print("native vs torch AdamW: losses %s / %s, eval depth err %.3e" % (a.losses, b.losses, err))
    assert err < 2e-2, err
    assert not torch.equal(b.before, b.after), "eval forward still uses the weights packed before training"


@pytest.fixture(scope="module")
def densenet():
    return _model("densenet121_bts")


def test_model_three_native_steps_match_torch_adamw_and_only_unattached_entries_are_repacked(densenet):
    torch_run = _train_run("densenet121_bts", 3, native=False, base=densenet)
    nat = _train_run("densenet121_bts", 3, native=True, base=densenet)
    _assert_same_training(torch_run, nat)
    assert "optim.adamw" in nat.kernels[0] and "adamw_step_kernel" in nat.kernels[2]
    assert "adamw_step_kernel" not in torch_run.kernels[1]
    assert len(nat.opt.attached) > 100
    # unfrozen: the 7x7 stem is updated but not a tile record -- its entries, and only they, go through the pack launch
    want = {id(e) for e in nat.opt.unattached}
    assert want, "the stem convolution should be an unattached entry"
    for s in (1, 2):
        assert {id(e) for e in nat.packed[s]} == want, s + 1
    assert nat.opt.uploads <= 3 and nat.opt.launches == 1


def test_model_with_frozen_stem_launches_no_pack_and_guards_a_nonfinite_loss(densenet):
    from bts_amd import bts as M, trainer
    nat = _train_run("densenet121_bts", 3, native=True, freeze=True, base=densenet)
    assert nat.frozen and any("conv0" in n for n in nat.frozen)
    for s in (1, 2):
        assert "pack_weights_kernel" not in nat.kernels[s] and nat.packed[s] == [], "step %d re-packed something" % (s + 1)
        assert "adamw_step_kernel" in nat.kernels[s]
    assert nat.opt.unattached == []
    assert all(nat.losses[i + 1] != nat.losses[i] for i in range(2))
    # a non-finite loss: parameters and optimiser state keep their bits, without the host reading the loss
    m, opt = nat.model.train(), nat.opt
    img, foc, gt = _data()
    crit = M.silog_loss(0.85)
    with pytest.raises(ValueError):
        trainer.train_step(m, trainer.make_optimizer(m, fused=False), crit, img, foc, gt, guard_nonfinite=True)
    bad = gt.clone()
    bad[0, 0, 3, 5] = float("inf")
    ps = [p for p in m.parameters() if p.requires_grad]
    snap = [(p.detach().clone(), opt.state[p]["exp_avg"].clone(), opt.state[p]["exp_avg_sq"].clone()) for p in ps if p in opt.state]
    loss, _ = trainer.train_step(m, opt, crit, img, foc, bad, guard_nonfinite=True)
    assert not bool(torch.isfinite(loss))
    live = [p for p in ps if p in opt.state]
    for p, (p0, m0, v0) in zip(live, snap):
        stt = opt.state[p]
        assert torch.equal(p.detach().view(torch.int32), p0.view(torch.int32))
        assert torch.equal(stt["exp_avg"].view(torch.int32), m0.view(torch.int32))
        assert torch.equal(stt["exp_avg_sq"].view(torch.int32), v0.view(torch.int32))
    loss, _ = trainer.train_step(m, opt, crit, img, foc, gt, guard_nonfinite=True)   # a finite step still updates
    assert bool(torch.isfinite(loss))
    changed = sum(0 if torch.equal(p.detach(), p0) else 1 for p, (p0, _, _) in zip(live, snap))
    print("finite step after the guarded one: %d of %d parameters changed" % (changed, len(live)))
    assert changed > len(live) // 2, (changed, len(live))
    assert all(bool(torch.isfinite(p).all()) for p in live)


def test_resnext_grouped_entries_stay_on_the_pack_launch():
    base = _model("resnext50_bts")
    torch_run = _train_run("resnext50_bts", 2, native=False, base=base)
    nat = _train_run("resnext50_bts", 2, native=True, base=base)
    _assert_same_training(torch_run, nat)
    from bts_amd import train
    grouped = {id(e) for key, e in _live_entries(nat.model) if key[4] > 1}
    assert grouped and grouped <= {id(e) for e in nat.opt.unattached}
    assert not grouped & {id(e) for e in nat.opt.attached}
    assert grouped <= {id(e) for e in nat.packed[1]}, "step 2's pack launch must cover the grouped weights"
    assert {id(e) for e in nat.packed[1]} == {id(e) for e in nat.opt.unattached}
    assert train._PACKER.versions_trusted is True
