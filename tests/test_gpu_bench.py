"""bench.py's plain run: exactly --steps timed steps, the result line's fields, and --dump-outputs writing what the
last step returned -- checked against the CPU oracle on the same seeded inputs."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_run_dumps_the_last_step(gpu_pkg, tmp_path):
    import bench

    rows, steps, warmup = 20000, 3, 2
    out = tmp_path / "dump"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup",
                        str(warmup), "--rows", str(rows), "--dump-outputs", str(out)],
                       cwd=tmp_path, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    line = json.loads(lines[0])
    for key in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert key in line, key
    assert line["steps"] == steps and line["repeats"] == 1
    assert line["ms_per_step"] > 0 and line["value"] > 0
    assert line["value"] == pytest.approx(bench.BATCH / (line["ms_per_step"] * 1e-3), rel=1e-2)
    # a plain run measures the headline only
    assert line["ivf"] is None and line["cpu_baseline"] is None and line["bf_int8"] is None

    ids, dists, flags = (np.load(out / f"bf_{n}.npy") for n in ("ids", "dists", "flags"))
    k1 = bench.K + 1
    assert ids.dtype == np.float64 and dists.dtype == np.float32 and flags.dtype == np.float64
    assert ids.shape == (bench.BATCH, k1) and dists.shape == (bench.BATCH, k1) and flags.shape == (bench.BATCH,)
    # steps 0..2 form one multi-batch call over query batches 0..2: the last step is batch 2
    base = gpu_pkg.synth_sift(rows, seed=bench.SEED_BASE)
    q = gpu_pkg.synth_sift(4096, seed=bench.SEED_QUERY)[(steps - 1) * bench.BATCH:steps * bench.BATCH]
    oid, od = oracle.search_bf(base, q, k1)
    assert np.array_equal(dists, od)
    untied = flags == 0  # flagged queries hold equal distances: their order among equals is the caller's to resolve
    assert untied.any()
    assert np.array_equal(ids[untied], oid[untied].astype(np.float64))
