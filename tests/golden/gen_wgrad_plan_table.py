"""Writes wgrad_plan_table.npz: what the three weight-gradient planners of libbts_hip.so (bts_conv_wgrad_plan_f32,
bts_upconv_wgrad_plan_f32, bts_conv_wgrad_batch_plan_f32) give a fixed grid of problems, as
tests/test_wgrad_plan_table.py re-checks it.  Tile, split, pix_per_split and ws_offset decide the summation order of
training's weight gradients and the launch shapes measured in DESIGN.md 3a; the exact kernel tests cannot see them.

single  every case of tests/wgrad_cases.py (CASES, PATH_CASES) and the 20 training shapes of scripts/wgrad_bench.py at
        B = 1, 4, 16; each with no workspace, 8 Mi floats and train.WGRAD_WS_FLOATS
upconv  every tests/upconv_train_cases.py WGRAD_CASES and the decoder's five ratio-2 upconvs (bts_size 512 on
        DenseNet161) at 4x352x704 and 1x352x1216; each with the minimal workspace and train.WGRAD_WS_FLOATS
batch   every batch of tests/wgrad_batch_cases.py and the four DenseNet161 blocks as scripts/wgrad_bench.py: blocks()
        lays them out (B = 4, 352x704); each with 0, 1 Mi and train.WGRAD_WS_FLOATS floats; `mixed` once more reversed
Host-side queries only: the pointers are fake and never dereferenced.

    python tests/golden/gen_wgrad_plan_table.py            # rewrite tests/golden/wgrad_plan_table.npz
    python tests/golden/gen_wgrad_plan_table.py --out F    # write F instead
"""
import argparse
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (os.path.join(ROOT, "scripts"), os.path.join(ROOT, "tests"), ROOT):
    sys.path.insert(0, p)
import upconv_train_cases as uc  # noqa: E402
import wgrad_batch_cases as bc  # noqa: E402
import wgrad_bench  # noqa: E402
import wgrad_cases as wc  # noqa: E402
from bts_amd import ops  # noqa: E402
from bts_amd.train import WGRAD_WS_FLOATS  # noqa: E402

TABLE = os.path.join(ROOT, "tests", "golden", "wgrad_plan_table.npz")
MI = 1 << 20
SINGLE_WS = (None, 8 * MI, WGRAD_WS_FLOATS)
BATCH_WS = (0, 1 * MI, WGRAD_WS_FLOATS)
DECODER_UPCONVS = ((32, 2208, 512), (16, 512, 256), (8, 256, 128), (4, 128, 64), (2, 64, 32))     # (stride of the source map, c_in, c_out)
DECODER_INPUTS = ((4, 352, 704), (1, 352, 1216))


def single_queries():
    """conv_wgrad_plan keyword arguments."""
    for c in wc.CASES + [c for _, c in wc.PATH_CASES]:
        nb = max(c.n_bundles, 1)
        for ws in SINGLE_WS:
            yield dict(B=c.B, h_in=c.h, w_in=c.w, c_in=c.c_in, c_out=c.c_out, ksize=c.ksize, dil=c.dil, stride=c.stride, pad=c.pad,
                       up=c.up, ws_floats=ws, n_bundles=c.n_bundles, pre=c.pre, pre_relu=c.pre_relu,
                       x_pix_stride=nb * c.c_in + c.x_extra, dy_pix_stride=nb * c.c_out + c.dy_extra)
    for _, _, h, w, cin, cout, k, dil, up in wgrad_bench.SHAPES:
        for B in (1, 4, 16):
            for ws in SINGLE_WS:
                yield dict(B=B, h_in=h, w_in=w, c_in=cin, c_out=cout, ksize=k, dil=dil, stride=1, pad=dil * (k // 2), up=up,
                           ws_floats=ws, n_bundles=1, pre=False, pre_relu=False, x_pix_stride=cin, dy_pix_stride=cout)


def upconv_queries():
    """(B, h, w, c_in, c_out, ws_floats)."""
    shapes = [(c.B, c.h, c.w, c.c_in, c.c_out, c.ws_floats) for c in uc.WGRAD_CASES]
    shapes += [(B, H // s, W // s, cin, cout, None) for B, H, W in DECODER_INPUTS for s, cin, cout in DECODER_UPCONVS]
    for B, h, w, cin, cout, ws in shapes:
        for ws_floats in sorted({16 * cout * cin, WGRAD_WS_FLOATS} | ({ws} if ws else set())):
            yield (B, h, w, cin, cout, ws_floats)


def block_problems(H, W, C0, L, B=4, g=48, mid=192):
    """One DenseNet161 block's 2*L problems on the buffers of scripts/wgrad_bench.py: blocks(): the 1x1 reads a prefix of the
    block buffer (Ct columns) against a dense slab, the 3x3 a dense slab against a column slice of the Ct-wide gradient."""
    Ct = C0 + L * g
    out = []
    for i in range(L):
        Ci = C0 + i * g
        geo = dict(B=B, h_in=H, w_in=W, pre=True, pre_relu=True)
        out.append(dict(geo, c_in=Ci, c_out=mid, ksize=1, x_pix_stride=Ct, dy_pix_stride=mid))
        out.append(dict(geo, c_in=mid, c_out=g, ksize=3, x_pix_stride=mid, dy_pix_stride=Ct))
    return out


def batch_queries():
    """(problems, ws_floats)."""
    batches = [[bc.problem_of(c) for c in cases] for _, cases in bc.BATCHES.values()]
    batches += [block_problems(H, W, C0, L) for _, H, W, C0, L in wgrad_bench.BLOCKS]
    batches.append([bc.problem_of(c) for c in reversed(bc.BATCHES["mixed"][1])])
    for problems in batches:
        for ws_floats in BATCH_WS:
            yield problems, ws_floats


def _key(h, d):
    h.update(np.asarray([-1 if d[k] is None else int(d[k]) for k in sorted(d)], np.int64).tobytes())


def run():
    keys = hashlib.sha256()
    single, upconv, batch, batch_id = [], [], [], []
    for q in single_queries():
        _key(keys, q)
        single.append(ops.conv_wgrad_plan(**q))
    for q in upconv_queries():
        keys.update(np.asarray(q, np.int64).tobytes())
        upconv.append(ops.upconv_wgrad_plan(*q))
    for i, (problems, ws_floats) in enumerate(batch_queries()):
        keys.update(np.asarray([len(problems), ws_floats], np.int64).tobytes())
        for pr in problems:
            _key(keys, pr)
        plan = ops.conv_wgrad_batch_plan(problems, ws_floats)
        batch += plan
        batch_id += [i] * len(plan)
    return dict(single=np.asarray(single, np.int64), upconv=np.asarray(upconv, np.int64), batch=np.asarray(batch, np.int64),
                batch_id=np.asarray(batch_id, np.int32), grid_sha256=np.frombuffer(keys.digest(), np.uint8))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=TABLE)
    args = ap.parse_args()
    t = run()
    np.savez_compressed(args.out, **t)
    print("%d single, %d upconv, %d batch problems in %d batches -> %s"
          % (len(t["single"]), len(t["upconv"]), len(t["batch"]), int(t["batch_id"][-1]) + 1, args.out))


if __name__ == "__main__":
    main()
