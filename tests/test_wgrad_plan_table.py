"""CPU: tile, split, pix_per_split and ws_offset of every query in the recorded grid -- single, sub-pixel upconv and batch
weight-gradient planners, on the test case tables and the training shapes -- equal the table
tests/golden/gen_wgrad_plan_table.py wrote.  Host-side plan queries, no GPU work.

The exact kernel tests cannot see a planner change (any tile and split gives the same bits on small integers) and the
plan tests check invariants only; this table is what says that a change to wgrad.hip moved no launch shape."""
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GEN = os.path.join(ROOT, "tests", "golden", "gen_wgrad_plan_table.py")


def test_wgrad_planners_match_recorded_plan_table(golden_dir, tmp_path):
    out = str(tmp_path / "plan.npz")
    env = {k: v for k, v in os.environ.items() if not k.startswith("BTS_")}
    subprocess.run([sys.executable, GEN, "--out", out], check=True, env=env, cwd=ROOT, timeout=600)
    want, got = np.load(os.path.join(golden_dir, "wgrad_plan_table.npz")), np.load(out)
    assert sorted(got.files) == sorted(want.files)
    assert np.array_equal(got["grid_sha256"], want["grid_sha256"]), "the query grid changed: regenerate the table"
    for name in want.files:
        assert got[name].shape == want[name].shape, name
        bad = np.flatnonzero((got[name] != want[name]).reshape(len(want[name]), -1).any(axis=1))
        assert bad.size == 0, "%s differs at %d of %d rows, first at %s: got %s, recorded %s" % (
            name, bad.size, len(want[name]), bad[:5], got[name][bad[:3]].tolist(), want[name][bad[:3]].tolist())
