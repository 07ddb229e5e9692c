"""bench.py's plain run and --dump-outputs: the plain line carries the headline fields and none of the --full legs; the
records of the last timed step are written as float64 arrays, the same from run to run and with --full, and they are the
records the sequential run of --full counts."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

ENV = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}


def _bench(args):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, env=ENV, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    return json.loads(lines[0])


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d)) if f.endswith(".npy")}


def test_plain_run_and_dumped_outputs(tmp_path):
    steps, K, B = 3, 4, 8
    common = ["--gpus", "1", "--steps", str(steps), "--warmup", "1", "--batch", str(B), "--batches-per-step", str(K)]
    plain = _bench(common + ["--dump-outputs", str(tmp_path / "plain")])
    for key in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert key in plain, key
    assert plain["steps"] == steps and plain["verified"] is True and plain["value"] > 0
    assert plain["ms_per_step"] == pytest.approx(1e3 * plain["config"]["timed_region_s"] / steps)
    assert plain["config"]["buffers_timed"] == steps * K * B
    # none of the --full legs ran
    assert "cpu_baseline" not in plain and plain["config"]["dense_band"] is None and plain["roofline"]["power_probe"] is None
    assert plain["verify"]["sequential_run_identical"] is None and plain["roofline"]["kernel_ms_isolated"] is None

    full = _bench(common + ["--full", "--no-cpu-baseline", "--no-dense", "--no-power-probe", "--dump-outputs", str(tmp_path / "full")])
    assert full["verified"] is True and full["verify"]["sequential_run_identical"] is True
    assert full["dtype"] == plain["dtype"] and full["metric"] == plain["metric"] and full["unit"] == plain["unit"]

    a, b = _load(tmp_path / "plain"), _load(tmp_path / "full")
    assert sorted(a) == sorted(b) and {"batch_index", "cell_counts", "cell_n_id_1", "cell_n_id_2", "cell_pss_pow", "cell_sfn"} <= set(a)
    assert sum(x.nbytes for x in a.values()) <= 64 << 20
    for name in a:
        assert a[name].dtype == np.float64, name
        np.testing.assert_array_equal(a[name], b[name], err_msg=name)      # NaNs compare equal here
    counts = a["cell_counts"]
    assert counts.shape == (K, B) and np.array_equal(a["batch_index"], np.arange(K))
    assert all(x.shape == (int(counts.sum()),) for n, x in a.items() if n.startswith("cell_") and n != "cell_counts")
    # batch m of the last step is distinct batch m (K = the number of distinct batches): its records are the sequential run's
    assert [int(c) for c in counts.sum(axis=1)] == full["config"]["cells_per_distinct_batch"]
    assert counts.sum() > 0 and np.all(np.isfinite(a["cell_pss_pow"]))
