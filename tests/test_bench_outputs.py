"""bench.py's plain run and --dump-outputs: a plain run prints the headline line only (what else the
benchmark measures is behind --full), --steps sets the number of timed steps, and --dump-outputs writes
the last timed step's probabilities -- the same from run to run, and the oracle's on the same rows."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STEPS, WARMUP, B = 3, 2, 65536
FULL_ONLY = ("stages", "stage_sum_ms", "roofline", "cpu_baseline", "predict_auc", "models", "parity_check_ranks")


def test_dump_sample_keeps_small_arrays_and_samples_large_ones():
    import bench
    a = np.arange(1000, dtype=np.float64)
    s = bench.dump_sample(a)
    assert s.dtype == np.float32 and np.array_equal(s, a.astype(np.float32))
    n = bench.DUMP_ARRAY_BYTES // 4 + 12345
    big = np.arange(n, dtype=np.float32)
    s1, s2 = bench.dump_sample(big), bench.dump_sample(big.copy())
    assert s1.nbytes == bench.DUMP_ARRAY_BYTES and np.array_equal(s1, s2)
    assert np.all(np.diff(s1) >= 0) and s1[0] >= 0 and s1[-1] < n  # elements of the array, in order


def test_write_dump_names_and_cap(tmp_path):
    import bench
    d = str(tmp_path / "o")
    bench.write_dump(d, {"out": np.ones(4, np.float32)})
    bench.write_dump(d, {"out": np.zeros(4, np.float32)}, rank=1)
    assert sorted(os.listdir(d)) == ["out.npy", "out_rank1.npy"]
    assert np.load(os.path.join(d, "out.npy")).dtype == np.float32
    too_big = {str(i): np.zeros(bench.DUMP_ARRAY_BYTES // 4, np.float32) for i in range(5)}
    with pytest.raises(RuntimeError):
        bench.write_dump(d, too_big)


def _plain_run(out_dir):
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(STEPS),
                        "--warmup", str(WARMUP), "--dump-outputs", str(out_dir)],
                       capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, p.stdout
    return json.loads(lines[0]), np.load(os.path.join(str(out_dir), "out.npy"))


@pytest.fixture(scope="module")
def plain(tmp_path_factory):
    return _plain_run(tmp_path_factory.mktemp("dump_a"))


@pytest.mark.gpu
def test_plain_run_prints_the_headline_only(plain):
    line, _ = plain
    assert line["unit"] == "examples/s" and line["higher_is_better"] is True and line["dtype"] == "f32"
    assert line["steps"] == STEPS and line["warmup"] == WARMUP and line["n_gpus"] == 1
    assert line["value"] > 0 and line["ms_per_step"] > 0
    # value and ms_per_step describe the same timed steps
    assert line["value"] == pytest.approx(B / (line["ms_per_step"] / 1e3), rel=1e-3)
    assert not [k for k in FULL_ONLY if k in line]


@pytest.mark.gpu
def test_dumped_output_is_the_last_timed_batch(plain):
    import bench
    _, out = plain
    assert out.dtype == np.float32 and out.shape == (B,)
    # step i runs batch i of the set, warm-up first: the last timed step is batch WARMUP + STEPS - 1
    pc = bench.parity_check("deepfm", out, (WARMUP + STEPS - 1) * B, n=64)
    print("max |p_gpu - p_oracle| = %.3g (tol %.0e)" % (pc["max_abs_diff"], pc["tol"]))
    assert pc["tol"] == 1e-5 and pc["ok"], pc


@pytest.mark.gpu
def test_dump_is_identical_from_run_to_run(plain, tmp_path):
    _, out_b = _plain_run(tmp_path / "dump_b")
    assert np.array_equal(plain[1], out_b)
