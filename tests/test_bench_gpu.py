"""GPU: a plain bench.py run is the headline alone - one JSON line, none of what --full adds (checks, other legs, cpu_baseline, the
full document) - at a size a test can afford."""
import json
import os
import subprocess
import sys

import pytest

from conftest import ROOT


@pytest.mark.gpu
def test_plain_run_is_the_headline_alone(tmp_path):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "3", "--warmup", "2", "--net", "mini", "--games", "256",
                        "--sims", "64", "--dump-outputs", str(tmp_path / "out")],
                       cwd=tmp_path, capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-1500:]
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 1, r.stdout[-1500:]
    line = json.loads(lines[0])
    assert line["steps"] == 3 and line["warmup"] == 2 and line["value"] > 0 and line["ms_per_step"] > 0
    assert line["parity_spotcheck"] == "skipped" and line["parity_spotcheck_timed_batch"] == "skipped"
    assert line["full_document"] is None and "cpu_baseline" not in line and "whole_games_measured" not in line
    assert not any(k.startswith(("config1", "config5", "ch5_yml", "headline_on", "worker_end", "bitboard")) for k in line), sorted(line)
    assert os.path.exists(tmp_path / "out" / "leaf_policy.npy")
