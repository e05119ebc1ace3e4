"""CPU: the convolution dispatch (kernel family, tile, split-K, tap-steps) of every query in the recorded grid equals the
table tests/golden/gen_conv_plan_table.py wrote, and every malformed descriptor of its second table is rejected with the
recorded code -- host-side plan queries, no GPU work.

The plan query reports kernel family, tile (bm, bn), split-K and tap-steps only.  Variants that share all of these -- 8- vs
4-wave row tiles, one vs two weight buffers, the bf16x3 buffering -- look the same here; which kernels the library holds
at all is visible in its gfx950 code object's symbol list."""
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GEN = os.path.join(ROOT, "tests", "golden", "gen_conv_plan_table.py")


def regenerate(out, *flags):
    # a fresh process without any BTS_* variable: the library reads its knobs once per process
    env = {k: v for k, v in os.environ.items() if not k.startswith("BTS_")}
    subprocess.run([sys.executable, GEN, "--out", out, *flags], check=True, env=env, cwd=ROOT, timeout=600)
    return np.load(out)


def test_conv_dispatch_matches_recorded_plan_table(golden_dir, tmp_path):
    got = regenerate(str(tmp_path / "plan.npz"))
    want = np.load(os.path.join(golden_dir, "conv_plan_table.npz"))
    assert sorted(got.files) == sorted(want.files)
    assert np.array_equal(got["grid_sha256"], want["grid_sha256"]), "the query grid changed: regenerate the table"
    for name in want.files:
        bad = np.flatnonzero(got[name] != want[name])
        assert bad.size == 0, "%s differs at %d of %d queries, first at %s" % (name, bad.size, want[name].size, bad[:5])


def test_malformed_descriptors_are_rejected_as_recorded(golden_dir, tmp_path):
    """Error code (and the outputs a rejecting query leaves behind) of every check of the forward host path, and which of two
    violated checks answers: bts_conv_plan_f32 / _ksteps_f32, bts_upconv_dgrad_plan, bts_upconv_dgrad_f32's argument checks."""
    got = regenerate(str(tmp_path / "rejects.npz"), "--rejects")
    want = np.load(os.path.join(golden_dir, "conv_reject_table.npz"))
    assert sorted(got.files) == sorted(want.files)
    assert np.array_equal(got["name"], want["name"]) and np.array_equal(got["grid_sha256"], want["grid_sha256"]), \
        "the descriptors changed: regenerate the table"
    for name in want.files:
        bad = np.flatnonzero(got[name] != want[name])
        assert bad.size == 0, "%s differs for %s" % (name, [(str(want["name"][i]), int(want[name][i]), int(got[name][i])) for i in bad[:5]])
