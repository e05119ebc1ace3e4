"""CPU estimate of the bf16 inference mode's accuracy with ``bf16_tail_convs`` on: the oracle decoder with every convolution
the mode takes run on operands rounded to bf16 (``Tensor.to(torch.bfloat16)``, then fp32 ``F.conv2d``) -- conv3 / conv2 with
their MAIN channels rounded and the depth plane (input and weights) left in fp32 -- against the plain fp32 oracle on the
same input.  Prints, per channel plan, median / max relative change of the five depth maps (near-singular LPG pixels
masked, as tests/parity_util.singular_masks) with the switch off and on.  tests/test_conv_tail_bf16_gpu.py holds the GPU to
twice the "on" figures.  No GPU.
    python scripts/bf16_tail_cpu_estimate.py [B H W seed]"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

from oracle import bts_oracle as O                                                              # noqa: E402
from parity_util import CONFIGS, OUT_NAMES, make_inputs, oracle_run, singular_masks             # noqa: E402
from bts_amd import synth                                                                       # noqa: E402

FP32_LAYERS = ("reduc", "conv1.", "get_depth.")          # what the mode keeps in fp32 whatever the switch says
TAIL_LAYERS = ("conv3.", "conv2.")


def _rne(v):
    return v.to(torch.bfloat16).float()


def emulated_run(cname, B, H, W, seed, tail_bf16):
    enc, md, ds, _, _ = CONFIGS[cname]
    state = O.state_from_numpy(synth.decoder_state(synth.ENCODER_CHANNELS[enc], 512, 0))
    names = {id(v): k for k, v in state.items()}
    real = O.F.conv2d

    def conv2d(x, w, *a, **kw):
        name = names.get(id(w), "reduc")                 # the reduction chains pass re-shaped copies of their weights
        if name.startswith(FP32_LAYERS):
            return real(x, w, *a, **kw)
        if name.startswith(TAIL_LAYERS):
            if not tail_bf16:
                return real(x, w, *a, **kw)
            c = w.shape[1] - 1
            return real(_rne(x[:, :c]), _rne(w[:, :c]), *a, **kw) + real(x[:, c:], w[:, c:], *a, **kw)
        return real(_rne(x), _rne(w), *a, **kw)

    feats, focal = make_inputs(cname, B, H, W, seed)
    O.F.conv2d = conv2d
    try:
        with torch.no_grad():
            return O.decoder_forward(state, feats, focal, md, ds)
    finally:
        O.F.conv2d = real


def depth_stats(got, ref_outs, inter):
    B, _, H, W = ref_outs[0].shape
    masks = singular_masks(inter, B, H, W)
    rep = {}
    for i, k in ((0, 8), (1, 4), (2, 2), (3, None), (4, None)):
        g, r = got[i].double().numpy(), ref_outs[i].double().numpy()
        m = masks[k] if k else np.ones_like(r, dtype=bool)
        rel = np.abs(g[m] - r[m]) / np.maximum(np.abs(r[m]), 1e-30)
        rep[OUT_NAMES[i]] = (float(np.median(rel)), float(rel.max()))
    return rep


def main():
    B, H, W, seed = [int(v) for v in sys.argv[1:5]] if len(sys.argv) >= 5 else (2, 64, 128, 4321)
    for cname in ("K", "N"):
        ref_outs, inter = oracle_run(cname, B, H, W, seed)
        for on in (False, True):
            rep = depth_stats(emulated_run(cname, B, H, W, seed, on), ref_outs, inter)
            print("%s %dx%dx%d bf16_tail_convs=%s" % (cname, B, H, W, on))
            for n, (med, mx) in rep.items():
                print("    %-18s median %.3e  max %.3e" % (n, med, mx))


if __name__ == "__main__":
    main()
