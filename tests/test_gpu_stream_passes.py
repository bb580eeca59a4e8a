"""The pass walk and the pass entry of the streaming scans, and the single-call scan's prologue, against the oracle.

A wave of scan_f32s_kernel / scan_i8w_kernel takes whole passes over the rows as far as the launch's passes deal evenly
to the 8 waves, and a contiguous range of the remaining passes' tiles (next_tile, vs_scan.hip); on entering a pass it
loads the pass's query operands with loads the compiler does not see and waits for them by hand (vs_ring.h).  The launches below are the
shapes in which that walk and that entry differ: a range inside one pass, ranges over two passes, whole passes only,
whole passes plus ranges, and (two batches per pass) an odd batch count, which leaves the second half of the last pass
dead.  65 537 rows is the smallest base that takes the seeded streaming scans, with a ragged last tile.  Every launch is
compared with the oracle the way test_gpu_parity.py compares search_dev_multi (dev_multi_check.py), never with another
GPU path."""
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle

pytestmark = pytest.mark.gpu

N_ROWS, N_SMALL, N_QUERIES, K = 65537, 100, 1024, 5


@pytest.fixture(scope="module")
def data_file(tmp_path_factory):
    """Integer-valued rows in [0, 255], integer-valued queries near rows, and the oracle's lists: computed once."""
    rng = np.random.default_rng(20261)
    base = rng.integers(0, 256, size=(N_ROWS, 128)).astype(np.float32)
    near = rng.integers(0, N_ROWS, size=N_QUERIES)
    q = np.clip(base[near] + rng.integers(-3, 4, size=(N_QUERIES, 128)), 0, 255).astype(np.float32)
    q[: N_QUERIES // 2] = np.clip(base[near[: N_QUERIES // 2] % N_SMALL] + rng.integers(-3, 4, size=(N_QUERIES // 2, 128)), 0, 255)
    small = base[:N_SMALL].copy()
    oi, od = oracle.search_bf(base, q, K)
    soi, sod = oracle.search_bf(small, q[:16], K)
    path = tmp_path_factory.mktemp("stream_passes") / "data.npz"
    np.savez(path, base=base, q=q, oi=oi, od=od, small_base=small, small_oi=soi, small_od=sod)
    return str(path)


def _cases(batches, Bs):
    return ",".join(f"{nb}:{B}" for B in Bs for nb in batches)


STREAM = {"VSEARCH_SEED_MIN": "1"}
F32 = dict(STREAM, VSEARCH_F32_FILTER="0")
RUNS = {
    # fp32 rows, one batch per pass: 1 .. 32 passes
    "f32_one_batch_per_pass": (dict(F32, VSEARCH_F32_PAIR="0"), 1, _cases((1, 5, 8, 9, 13, 16, 17, 32), (32,)) + ",13:20"),
    # fp32 rows, two batches per pass: 1, 2, 8, 8, 9, 9, 16, 16 passes, the odd counts with a dead second half
    "f32_two_batches_per_pass": (dict(F32, VSEARCH_F32_PAIR="2"), 1, _cases((2, 3, 15, 16, 17, 18, 31, 32), (32,)) + ",17:20"),
    # byte rows, 4 / 8 / 12 column blocks per pass
    "i8_wide_4": (dict(STREAM, VSEARCH_I8_WIDE="4"), 2, _cases((1, 3, 8, 9, 17, 32), (32, 20))),
    "i8_wide_8": (dict(STREAM, VSEARCH_I8_WIDE="8"), 2, _cases((1, 3, 8, 9, 17, 32), (32, 20))),
    "i8_wide_12": (dict(STREAM, VSEARCH_I8_WIDE="12"), 2, _cases((1, 3, 8, 9, 17, 32), (32, 20))),
    # the single-call scan (short calls on fp32 rows): on the small base most waves have no first or second tile
    "single_call": ({}, 1, "1:1,1:5,1:16,s1:1,s1:5,s1:16"),
}


@pytest.mark.parametrize("name", list(RUNS))
def test_stream_passes_match_oracle(gpu_pkg, data_file, name):
    env, precision, cases = RUNS[name]
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    e = dict(os.environ)
    e.update(env)
    r = subprocess.run([sys.executable, os.path.join(root, "tests", "stream_passes_child.py"), root, data_file, str(precision), cases],
                       env=e, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "STREAM_PASSES_OK" in r.stdout, (name, r.stdout[-400:], r.stderr[-1500:])
