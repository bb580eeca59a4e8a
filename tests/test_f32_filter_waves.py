"""The two organisations of the bf16 prefilter sweep (scan_f32f_kernel) -- one 8-wave workgroup per CU
(VSEARCH_F32F_WAVES=8) and two 4-wave workgroups per CU (VSEARCH_F32F_WAVES=4) -- against each other and against
scan_f32s_kernel (VSEARCH_F32_FILTER=0), bit for bit, and the single merge launch behind the sweep and its fallback scan.

The shard is the smallest that takes the prefilter: 65 537 rows = 1025 units, 4 or 5 per sweeper, one to two turns of
the ring, a ragged last unit.  The batch counts are the ones at which the 4-wave organisation changes: a second half
without any column block (1 and 2 batches: it returns at once), partly live (3), full at one column block per wave (4),
two column blocks per wave with dead ones (5), eight with blocks 34..63 dead (17), and the full launch (32).  Each side
runs in a process of its own: the knobs are read when the library loads."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:  # (also run as a script: the worker below)
    sys.path.insert(0, ROOT)

ROWS = 65_537
# (name, metric, queries per batch, id offset, batch counts, every n-th query gets a 2^-70 component)
CASES = [
    ("l2", 0, 32, 0, (1, 2, 3, 4, 5, 17, 32), 0),
    ("ip", 1, 32, 0, (4, 32), 0),
    ("b20", 0, 20, 3_000_000, (5, 32), 0),
    # E = +inf for a query with a component below 2^-60: every row is its candidate.  One such query per batch, as
    # first asked for, does not overflow at this size: a wave holds one of them and writes the 256 - 320 rows of its
    # workgroup's units, against 1024 entries per wave buffer (measured: overflowed 0 on both organisations, 265 104
    # entries written by the sweep, 2768 kept by the recheck, as without that query).  Every third query (5 or 6 per
    # 16-query column block: 1280 entries and more per wave) does (measured: overflowed 1, 2 820 132 written).  Both are
    # run; the first is held to the no-overflow assertions, the second to the overflow ones.
    ("tiny1", 0, 32, 0, (4,), 32),
    ("tiny3", 0, 32, 0, (4,), 3),
]
SIDES = {"w4": {"VSEARCH_F32F_WAVES": "4"}, "w8": {"VSEARCH_F32F_WAVES": "8"}, "f32": {"VSEARCH_F32_FILTER": "0"}}


def _data(rows, seed):  # as in test_f32_filter_ring.py
    rng = np.random.default_rng(seed)
    g = rng.standard_normal((rows, 128)).astype(np.float32)
    # queries near rows, and 12 near-duplicates per query around its 5th / 6th best
    q = (g[rng.integers(0, rows, 32 * 32)] + 0.3 * rng.standard_normal((32 * 32, 128))).astype(np.float32)
    u = rng.standard_normal((256, 128))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    for m in range(12):
        g[256 * m: 256 * (m + 1)] = (q[:256] + (1.0 + m * 2.0 ** -20) * u).astype(np.float32)
    return g, q


def _keys():
    return [f"{name}_nb{nb}" for name, _, _, _, nbs, _ in CASES for nb in nbs]


def _worker(argv):
    """python test_f32_filter_waves.py <out.npz>: the searches of one side, in a process of its own."""
    import torch
    import __graft_entry__ as ge

    pkg = ge.load_package()
    dev = torch.device("cuda", 0)
    res = {}
    filtered = os.environ.get("VSEARCH_F32_FILTER") != "0"
    base, q0 = _data(ROWS, 808)
    for name, metric, B, id_offset, nbs, tiny in CASES:
        q = q0.copy()
        if tiny:
            q[::tiny, 3] = 2.0 ** -70
        with pkg.BruteForceIndex(base, metric=metric, id_offset=id_offset) as idx:
            idx.set_precision(1)
            for nb in nbs:
                qd = torch.from_numpy(np.ascontiguousarray(q[: nb * B])).to(dev)
                o_d = torch.zeros((nb * B, 6), dtype=torch.float32, device=dev)
                o_i = torch.full((nb * B, 6), -7, dtype=torch.int32, device=dev)
                fl = torch.full((nb * B,), -7, dtype=torch.int32, device=dev)
                if filtered:
                    idx.filter_stats(reset=True)
                idx.search_dev_multi(qd.data_ptr(), nb, B, 5, o_i.data_ptr(), o_d.data_ptr(), fl.data_ptr(),
                                     torch.cuda.current_stream().cuda_stream)
                torch.cuda.synchronize()
                key = f"{name}_nb{nb}"
                res[key + "_i"] = o_i.cpu().numpy()
                res[key + "_d"] = o_d.cpu().numpy()
                res[key + "_f"] = fl.cpu().numpy()
                if filtered:
                    res[key + "_stats"] = np.array(idx.filter_stats(reset=True), dtype=np.int64)
    np.savez(argv[0], **res)


_RUNS = {}


def _side(tmp_path_factory, side):
    if side not in _RUNS:  # every side once per session, shared by the tests below and left unchanged
        out = str(tmp_path_factory.mktemp("waves") / f"{side}.npz")
        env = dict(os.environ, VSEARCH_SEED_MIN="1")  # every batch count takes the seeded streaming scan
        for k in ("VSEARCH_F32F_WAVES", "VSEARCH_F32_FILTER"):
            env.pop(k, None)
        env.update(SIDES[side])
        subprocess.run([sys.executable, os.path.abspath(__file__), out], env=env, check=True, timeout=600)
        _RUNS[side] = dict(np.load(out))
    return _RUNS[side]


@pytest.mark.gpu
def test_both_organisations_equal_the_fp32_kernel_bit_for_bit(gpu_pkg, tmp_path_factory):
    a, b, c = (_side(tmp_path_factory, s) for s in ("w4", "w8", "f32"))
    keys = _keys()
    assert len(keys) == 7 + 2 + 2 + 1 + 1
    for k in keys:
        for s in ("_i", "_d", "_f"):
            assert np.array_equal(a[k + s], c[k + s]), ("4 waves against fp32", k + s)
            assert np.array_equal(b[k + s], c[k + s]), ("8 waves against fp32", k + s)
    for name, metric, B, id_offset, nbs, tiny in CASES:  # the lists are not empty: ids of the shard, offset applied
        ids = c[f"{name}_nb{nbs[-1]}_i"][:, :5]
        assert ((ids >= id_offset) & (ids < id_offset + ROWS)).all(), name


@pytest.mark.gpu
def test_both_organisations_score_the_same_candidates(gpu_pkg, tmp_path_factory):
    """Where nothing overflows: one prefilter launch per call on either organisation, and equal counts of candidates
    written by the sweep and kept by the recheck -- every (row, query) value comes from the same MFMA chain."""
    a, b = (_side(tmp_path_factory, s) for s in ("w4", "w8"))
    for k in _keys():
        if k.startswith("tiny3"):
            continue
        sa, sb = [int(x) for x in a[k + "_stats"]], [int(x) for x in b[k + "_stats"]]
        print(f"{k}: (launches, overflowed, written, kept) 4 waves {sa}  8 waves {sb}")
        assert sa[0] == 1 and sb[0] == 1, k
        assert sa[1] == 0 and sb[1] == 0, k
        assert sa[2] == sb[2] and sa[3] == sb[3], k
        assert sa[2] >= sa[3] > 0, k


@pytest.mark.gpu
def test_one_merge_launch_returns_the_fallback_after_an_overflow(gpu_pkg, tmp_path_factory):
    """The wave buffers overflow, the fallback scan behind the sweep runs, and the single merge launch ranks its lane
    lists instead of the candidate lists: the outputs are scan_f32s_kernel's."""
    a, b, c = (_side(tmp_path_factory, s) for s in ("w4", "w8", "f32"))
    k = "tiny3_nb4"
    for name, side in (("4 waves", a), ("8 waves", b)):
        launches, overflowed, written, kept = (int(x) for x in side[k + "_stats"])
        print(f"{k}, {name}: launches {launches} overflowed {overflowed} written {written} kept {kept}")
        assert launches == 1 and overflowed == 1, (name, launches, overflowed)
        for s in ("_i", "_d", "_f"):
            assert np.array_equal(side[k + s], c[k + s]), (name, k + s)
    assert (c[k + "_i"][:, :5] >= 0).all()


if __name__ == "__main__":
    _worker(sys.argv[1:])
