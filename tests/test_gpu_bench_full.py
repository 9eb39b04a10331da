"""``bench.py --full``: a plain run prints the headline and the roofline of its own timed steps; ``--full`` adds the legs that
take runs of their own (cold figure, stage profile, stand-alone gather).  A 64x64 map, the long legs (quality, extra
configurations, CPU baseline) switched off."""
import json
import os
import subprocess
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(REPO, "bench.py")


def _bench_line(*extra):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_PORT", "DAGL_SPAWNED",
                                                             "DAGL_BENCH_FORCE_SPAWN", "DAGL_BENCH_FORCE_DIST")}
    r = subprocess.run([sys.executable, BENCH, "--gpus", "1", "--steps", "3", "--warmup", "1", "--size", "64", *extra], env=env,
                       capture_output=True, text=True, timeout=600, cwd=REPO)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_run_leaves_the_other_legs_to_full():
    plain = _bench_line()
    full = _bench_line("--full", "--no-quality", "--no-cpu-baseline", "--no-extra")
    for line in (plain, full):
        assert line["value"] > 0 and line["ms_per_step"] > 0 and line["steps"] == 3 and line["warmup"] == 1
        assert (line["unit"], line["dtype"], line["higher_is_better"]) == ("patches/s", "f32", True)
        assert line["roofline"]["ms_per_launch"] > 0          # from the events of the timed steps, in both
    assert plain["full"] is False and full["full"] is True
    for key in ("ms_per_step_cold", "stage_ms", "hip_block_ms"):
        assert key not in plain and key in full, key
    assert plain["roofline_gather"] is None and full["roofline_gather"]["ms_per_launch"] > 0
