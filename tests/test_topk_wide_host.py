"""Host side of the wide-k brute force: the CLI's argument checks (they run before anything touches HIP, so they hold on a
machine without a GPU) and select_topk's slot semantics for k >= 17 against the oracle."""
import os
import subprocess

import numpy as np
import pytest

import oracle


@pytest.fixture(scope="module")
def vsearch_bf(pkg):
    exe = os.path.join(os.path.dirname(pkg.LIB_PATH), "vsearch_bf")
    if not os.path.exists(exe):
        pkg.build(targets=("all",))
    assert os.path.exists(exe)
    return exe


@pytest.fixture(scope="module")
def fvecs(pkg, tmp_path_factory):
    d = tmp_path_factory.mktemp("topk_wide_cli")
    base, q = str(d / "base.fvecs"), str(d / "q.fvecs")
    pkg.write_fvecs(base, np.zeros((40, 128), dtype=np.float32))
    pkg.write_fvecs(q, np.zeros((3, 128), dtype=np.float32))
    return base, q, str(d)


@pytest.mark.parametrize("args", [
    ["--groundtruth"],
    ["--groundtruth", "BASE", "Q"],
    ["--groundtruth", "BASE", "Q", "OUT", "0"],
    ["--groundtruth", "BASE", "Q", "OUT", "129"],
    ["--groundtruth", "BASE", "Q", "OUT", "ten"],
    ["--groundtruth", "BASE", "Q", "OUT", "100", "extra"],
    ["--groundtruth", "BASE", "missing.fvecs", "OUT"],
    ["--groundtruth", "missing.fvecs", "Q", "OUT"],
    ["--groundtruth", "BASE", "Q", "OUT", "20", "--gpus", "2"],
    ["BASE", "Q", "129", "OUT"],
    ["BASE", "Q", "0", "OUT"],
    ["BASE", "Q", "16", "OUT", "--gpus", "2"],
])
def test_cli_rejects_bad_arguments_before_hip(vsearch_bf, fvecs, args):
    base, q, d = fvecs
    argv = [{"BASE": base, "Q": q, "OUT": os.path.join(d, "out.ivecs")}.get(a, a) for a in args]
    r = subprocess.run([vsearch_bf] + argv, capture_output=True, text=True, timeout=60, cwd=d)
    assert r.returncode != 0
    assert "usage:" in r.stderr
    # the banner (device count) comes after the checks: nothing asked HIP anything
    assert "HIP device" not in r.stdout
    assert not os.path.exists(os.path.join(d, "out.ivecs"))


@pytest.mark.parametrize("k", [17, 100, 128])
def test_select_topk_slots_wide_k(pkg, k):
    rng = np.random.default_rng(k)
    for trial in range(4):
        m = int(rng.integers(k // 2, 4 * k + 50))
        rows = np.sort(rng.choice(100000, size=m, replace=False)).astype(np.int32)
        dist = rng.integers(0, 6 if trial < 2 else 60, size=m).astype(np.float32)  # tie-heavy
        got = pkg.select_topk_slots(rows, dist, k)
        want = oracle.select_topk_sparse(rows, dist, k)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
