"""bench.py's command line: a plain run reports the headline only (the other legs wait for --full), --steps sets
the number of timed steps, --dump-outputs writes what the last timed step computed.

The GPU test runs the real bench once at a small batch (global batch 4 = micro-batch 2 x 2 accumulation, the
full-size model) and the tests below share its output.
"""

import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")
STEPS, WARMUP = 2, 1


def _env():
    return {k: v for k, v in os.environ.items()
            if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "PZ_DEVICE", "PZ_RANKS_PER_GPU", "PZ_VISIBLE_GPUS")}


def test_zero_steps_refused():
    r = subprocess.run([sys.executable, BENCH, "--gpus", "1", "--steps", "0"], env=_env(), capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 2
    assert "--steps" in r.stderr
    assert r.stdout.strip() == ""


def test_full_and_dump_options_listed():
    r = subprocess.run([sys.executable, BENCH, "--help"], env=_env(), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0
    assert "--full" in r.stdout and "--dump-outputs" in r.stdout


@pytest.fixture(scope="module")
def plain_run(tmp_path_factory):
    out = tmp_path_factory.mktemp("bench_dump")
    r = subprocess.run([sys.executable, "-u", BENCH, "--gpus", "1", "--steps", str(STEPS), "--warmup", str(WARMUP),
                        "--micro-batch", "2", "--global-batch", "4", "--dump-outputs", str(out)],
                       env=_env(), capture_output=True, text=True, timeout=280)
    assert r.returncode == 0, r.stderr[-4000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0]), out


@pytest.mark.gpu
def test_plain_run_reports_headline_only(plain_run):
    line, _ = plain_run
    assert line["metric"].startswith("train samples/sec") and line["unit"] == "samples/s"
    assert line["higher_is_better"] is True and line["dtype"] == "bf16"
    assert line["steps"] == STEPS and line["warmup"] == WARMUP
    assert len(line["loss_per_step"]) == STEPS + WARMUP  # --steps is the number of timed steps
    assert line["ms_per_step"] > 0
    # value and ms_per_step are the same measurement: global batch / seconds per timed step
    assert line["value"] == pytest.approx(line["config"]["global_batch"] / (line["ms_per_step"] * 1e-3), rel=1e-9)
    for leg in ("roofline", "inference", "c5_inference", "cpu_baseline"):  # --full only
        assert line[leg] is None, leg


@pytest.mark.gpu
def test_dump_outputs_written(plain_run):
    line, out = plain_run
    files = sorted(os.listdir(out))
    assert files == ["grad_norm_per_step.npy", "grad_sample.npy", "loss_per_step.npy", "param_sample.npy"]
    arrs = {f[:-4]: np.load(os.path.join(out, f)) for f in files}
    assert all(a.dtype in (np.float32, np.float64) for a in arrs.values())
    assert sum(a.nbytes for a in arrs.values()) <= 64 << 20
    assert all(np.isfinite(a).all() for a in arrs.values())
    # the dumped losses / norms are the ones the result line reports
    assert arrs["loss_per_step"].tolist() == line["loss_per_step"]
    assert arrs["grad_norm_per_step"].tolist() == line["grad_norm_per_step"]
    g, p = arrs["grad_sample"], arrs["param_sample"]
    assert g.shape == p.shape and g.ndim == 1 and g.size >= 1 << 20
    # a real gradient and real weights: most sampled positions are trained parameters (2.6 B of the 3.2 B arena)
    assert np.count_nonzero(g) > 0.5 * g.size and np.count_nonzero(p) > 0.5 * p.size
