"""CPU: bench.py's command-line contract where no GPU is needed to check it - it must refuse loudly (never fall back to a
CPU path), `--gpus N` started without a launcher must try to become N ranks, and the spot-check bookkeeping must count
the root-expansion simulation."""
import os
import subprocess
import sys

import pytest

from conftest import ROOT


def _run(*args, env=None):
    e = dict(os.environ)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        e.pop(k, None)
    e.update(env or {})
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *args], capture_output=True, text=True, env=e, timeout=300)


def _no_gpu():
    import torch
    return not torch.cuda.is_available()


@pytest.mark.skipif(not _no_gpu(), reason="checks the behaviour on a box without a GPU")
def test_bench_refuses_without_a_gpu():
    r = _run()
    assert r.returncode != 0 and "needs a GPU" in (r.stdout + r.stderr) and "no CPU fallback" in (r.stdout + r.stderr)


@pytest.mark.skipif(not _no_gpu(), reason="checks the behaviour on a box without a GPU")
def test_bench_gpus_n_spawns_or_refuses():
    r = _run("--gpus", "2")
    assert r.returncode != 0 and "only 0 GPU(s) visible" in (r.stdout + r.stderr)
    # a launcher's environment that disagrees with --gpus is an error, not a silent 1-GPU run
    r = _run("--gpus", "4", env={"RANK": "0", "WORLD_SIZE": "2", "LOCAL_RANK": "0"})
    assert r.returncode != 0 and "--gpus 4 but WORLD_SIZE=2" in (r.stdout + r.stderr)


def test_bench_line_schema_is_documented():
    """The keys the driver's contract names are assembled in headline_leg (a static check: no GPU here)."""
    src = open(os.path.join(ROOT, "bench.py")).read()
    for key in ('"metric"', '"value"', '"unit"', '"n_gpus"', '"steps"', '"warmup"', '"ms_per_step"', '"higher_is_better"', '"scaling"',
                '"vs_baseline"', '"dtype"', '"data"', '"config"', '"roofline"', '"cpu_baseline"', '"parity_spotcheck"'):
        assert key in src, key
    assert "BASELINE configs[2]" in src and "oracle" in src.split("def headline_leg")[0]   # the oracle only in the checker functions


def test_bench_refuses_zero_steps():
    r = _run("--steps", "0")
    assert r.returncode != 0 and "--steps must be at least 1" in (r.stdout + r.stderr)


def test_dump_outputs_of_a_full_batch(tmp_path):
    """--dump-outputs on the headline's shapes (8192 games, 72 plies of records, f64 root W recorded): float32 / float64 .npy files
    within the 64 MB cap, rows the last step did not evaluate zeroed, the same seeded sample of slots every time."""
    import types
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    import bench
    from reversi_alpha_zero_amd.engine import PLY_HEADER
    n, mp = 8192, 72
    rng = np.random.default_rng(5)
    active = torch.from_numpy((rng.random(n) < 0.9).astype(np.uint8))
    hdr = np.zeros((n, mp), dtype=PLY_HEADER)
    hdr["action"] = rng.integers(-1, 64, (n, mp))
    hdr["q"] = rng.random((n, mp))
    raw = dict(headers=hdr, root_n=rng.integers(0, 900, (n, mp, 64)).astype(np.uint32), root_w=rng.random((n, mp, 64)),
               n_plies=rng.integers(0, mp, n).astype(np.uint32), status=rng.integers(0, 4, n).astype(np.uint8))
    eng = types.SimpleNamespace(n_games=n, read_raw=lambda: raw, leaf_exchange=lambda: {
        "active": active, "policy": torch.ones(n, 64), "value": torch.full((n,), 0.5)})
    out = bench.timed_outputs(eng)
    bench.dump_outputs(str(tmp_path), out)
    got = {f[:-4]: np.load(tmp_path / f) for f in os.listdir(tmp_path)}
    assert set(got) == set(out) and sum(a.nbytes for a in got.values()) <= 64 << 20
    assert all(a.dtype in (np.float32, np.float64) for a in got.values())
    a = active.numpy() != 0
    assert (got["leaf_policy"][~a] == 0).all() and (got["leaf_policy"][a] == 1).all() and (got["leaf_value"][~a] == 0).all()
    pick = got["record_slots"].astype(np.int64)
    assert len(pick) == bench.DUMP_SAMPLE_SLOTS and np.array_equal(pick, bench.timed_outputs(eng)["record_slots"])
    assert np.array_equal(got["record_root_n"], raw["root_n"][pick]) and np.array_equal(got["record_root_w"], raw["root_w"][pick])
    assert np.array_equal(got["record_action"], hdr["action"][pick])
