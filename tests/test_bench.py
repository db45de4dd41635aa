"""bench.py as the measurement is run: a plain run (set-up, warm-up, the timed steps, one JSON line) and --dump-outputs."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT


def _plain_run(steps, warmup, dump_dir):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT", "HPRLP_TEST_HOOKS")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--workload", "c5_tiny", "--steps", str(steps),
                        "--warmup", str(warmup), "--dump-outputs", str(dump_dir)],
                       env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    lines = [ln for ln in r.stdout.decode().splitlines() if ln.strip()]
    assert len(lines) == 1, lines
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_bench_line_and_dumped_outputs(gpu, tmp_path):
    """A plain run times exactly --steps steps and reports ms_per_step = 1 / value; the --full fields are not in its line;
    --dump-outputs writes x and y of the last timed step as float64 .npy files, and a second run with the same arguments
    writes the same vectors."""
    dumps = []
    for k in range(2):
        d = _plain_run(7, 3, tmp_path / f"run{k}")
        assert d["steps"] == 7 and d["warmup"] == 3 and d["n_gpus"] == 1
        assert d["metric"] == "HPR iterations/sec (FP64)" and d["unit"] == "iterations/s" and d["dtype"] == "f64" and d["higher_is_better"]
        assert d["value"] > 0 and abs(d["value"] * d["ms_per_step"] - 1e3) <= 1e-6 * 1e3
        assert not {"spmv_only", "kkt_after_run", "time_to_tol", "other_configs", "ladder", "predicted_scaling", "cpu_baseline"} & set(d)
        x, y = np.load(tmp_path / f"run{k}" / "x.npy"), np.load(tmp_path / f"run{k}" / "y.npy")
        assert x.dtype == np.float64 and y.dtype == np.float64 and x.shape == (d["config"]["n"],) and y.shape == (d["config"]["m"],)
        assert np.isfinite(x).all() and np.isfinite(y).all() and np.abs(x).max() > 0
        dumps.append((x, y))
    for a, b in zip(*dumps):
        np.testing.assert_allclose(a, b, rtol=1e-9, atol=1e-12)
