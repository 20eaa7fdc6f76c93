"""CPU: the options of bench.py that need no device (--full, --dump-outputs, --steps)."""
import importlib.util
import os
import subprocess
import sys
import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    spec = importlib.util.spec_from_file_location("bench_under_test", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    return bench


def test_bench_plain_run_leaves_the_extra_legs_to_full(monkeypatch):
    bench = _bench()
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "7", "--warmup", "2"])
    a = bench.parse()
    assert a.steps == 7 and a.warmup == 2 and not a.full and a.dump_outputs is None
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--dump-outputs", "out"])
    a = bench.parse()
    assert a.full and a.dump_outputs == "out"


def test_bench_dump_outputs_writes_float32_tables_within_the_limit(tmp_path):
    """One file per FOV of the last step, float32, values unchanged; a step whose tables exceed 64 MB is cut after the
    FOVs that fit, in step order."""
    bench = _bench()
    rng = np.random.RandomState(0)
    tabs = [rng.rand(n, 11).astype(np.float32) for n in (5, 0, 3)]
    bench.dump_outputs(str(tmp_path / "d"), tabs)
    for j, t in enumerate(tabs):
        got = np.load(str(tmp_path / "d" / ("spots_fov%d.npy" % j)))
        assert got.dtype == np.float32 and got.shape == t.shape and np.array_equal(got, t)
    big = [np.zeros((400000, 11), np.float32)] * 6   # 17.6 MB each: three fit in 64 MiB
    bench.dump_outputs(str(tmp_path / "big"), big)
    names = sorted(os.listdir(str(tmp_path / "big")))
    assert names == ["spots_fov%d.npy" % j for j in range(3)]
    assert sum(os.path.getsize(str(tmp_path / "big" / n)) for n in names) <= bench.DUMP_LIMIT_BYTES


@pytest.mark.parametrize("args", [["--steps", "0"], ["--warmup", "-1"]])
def test_bench_rejects_a_run_without_timed_steps(args):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1"] + args, capture_output=True,
                       text=True, timeout=120)
    assert r.returncode != 0 and "--steps" in r.stderr, r.stderr[-400:]
