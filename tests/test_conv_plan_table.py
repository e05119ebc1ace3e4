"""CPU: the convolution dispatch (kernel family, tile, split-K, tap-steps) of every query in the recorded grid equals the
table tests/golden/gen_conv_plan_table.py wrote -- host-side plan queries, no GPU work.

The plan query reports kernel family, tile (bm, bn), split-K and tap-steps only.  Variants that share all of these -- 8- vs
4-wave row tiles, one vs two weight buffers, the bf16x3 buffering -- look the same here; which kernels the library holds
at all is visible in its gfx950 code object's symbol list."""
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GEN = os.path.join(ROOT, "tests", "golden", "gen_conv_plan_table.py")


def test_conv_dispatch_matches_recorded_plan_table(golden_dir, tmp_path):
    out = str(tmp_path / "plan.npz")
    # a fresh process without any BTS_* variable: the library reads its knobs once per process
    env = {k: v for k, v in os.environ.items() if not k.startswith("BTS_")}
    subprocess.run([sys.executable, GEN, "--out", out], check=True, env=env, cwd=ROOT, timeout=600)
    want, got = np.load(os.path.join(golden_dir, "conv_plan_table.npz")), np.load(out)
    assert sorted(got.files) == sorted(want.files)
    assert np.array_equal(got["grid_sha256"], want["grid_sha256"]), "the query grid changed: regenerate the table"
    for name in want.files:
        bad = np.flatnonzero(got[name] != want[name])
        assert bad.size == 0, "%s differs at %d of %d queries, first at %s" % (name, bad.size, want[name].size, bad[:5])
