"""bench.py on one GPU: a plain run carries the headline (and the roofline of the kernels timed inside its steps) and
nothing else; --full adds the check of scan seed 0's voxel counts, the forward-only rate and the CPU baseline (left out
here with --no-cpu-baseline: it is the slowest leg and never touches the GPU)."""
import json
import os
import subprocess
import sys

import pytest

from helpers import REPO

pytestmark = pytest.mark.gpu


def _line(*extra):
    out = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1",
                          *extra], capture_output=True, text=True, timeout=600, cwd=REPO)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, out.stdout[-2000:]
    return json.loads(lines[0])


def test_plain_run_leaves_the_extras_to_full():
    from lidog_amd import synth
    plain = _line()
    full = _line("--full", "--no-cpu-baseline")
    for line in (plain, full):
        assert line["unit"] == "scans/s" and line["higher_is_better"] is True and line["dtype"] == "f32"
        assert line["value"] > 0 and line["ms_per_step"] > 0 and line["steps"] == 2 and "roofline" in line
        assert "cpu_baseline" not in line
    assert plain["config"]["seed0_stride_counts"] is None and "forward_only_scans_per_s" not in plain
    assert tuple(full["config"]["seed0_stride_counts"]) == synth.BASELINE_COUNTS["kitti120k"]
    assert full["forward_only_scans_per_s"] > 0
    # --full adds nothing to the warm-up and timed steps: they compute the same
    assert abs(full["loss"] - plain["loss"]) <= 2e-5 * abs(plain["loss"]), (full["loss"], plain["loss"])
