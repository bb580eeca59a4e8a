"""The bf16 prefilter's shared-ring organisation (scan_f32f_kernel) against scan_f32s_kernel
(VSEARCH_F32_FILTER=0), bit for bit: every split of the launch's column blocks over the 8 waves (1 to 32 batches,
waves with no column block included), ragged last tiles, the smallest shard that takes the prefilter (a workgroup has
one to two ring depths of tiles), the shard size of an 8-rank split, a non-zero id offset, partial batches and both
metrics.  Each side runs in a process of its own."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:  # (also run as a script: the A/B worker below)
    sys.path.insert(0, ROOT)

# (name, rows, metric, queries per batch, id offset, batch counts)
CASES = [
    ("min_l2", 65_537, 0, 32, 0, (1, 3, 4, 5, 7, 8, 20, 31, 32)),
    ("min_ip", 65_537, 1, 32, 0, (1, 4, 7, 32)),
    ("shard8_l2", 125_000, 0, 32, 3_000_000, (1, 3, 5, 8, 20, 32)),
    ("shard8_ip", 125_000, 1, 32, 3_000_000, (2, 5, 31)),
    ("odd_b20", 200_003, 0, 20, 0, (3, 8, 20)),
    ("odd_b16_ip", 200_003, 1, 16, 7, (1, 5, 32)),
]


def _data(rows, seed):
    rng = np.random.default_rng(seed)
    g = rng.standard_normal((rows, 128)).astype(np.float32)
    # queries near rows, and 12 near-duplicates per query around its 5th / 6th best
    q = (g[rng.integers(0, rows, 32 * 32)] + 0.3 * rng.standard_normal((32 * 32, 128))).astype(np.float32)
    u = rng.standard_normal((256, 128))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    for m in range(12):
        g[256 * m: 256 * (m + 1)] = (q[:256] + (1.0 + m * 2.0 ** -20) * u).astype(np.float32)
    return g, q


def _worker(argv):
    """python test_f32_filter_ring.py <out.npz>: the searches of one A/B side, in a process of its own."""
    import torch
    import __graft_entry__ as ge

    pkg = ge.load_package()
    dev = torch.device("cuda", 0)
    res = {}
    for ci, (name, rows, metric, B, id_offset, nbs) in enumerate(CASES):
        base, q = _data(rows, 100 + ci)
        with pkg.BruteForceIndex(base, metric=metric, id_offset=id_offset) as idx:
            idx.set_precision(1)
            for nb in nbs:
                qd = torch.from_numpy(np.ascontiguousarray(q[: nb * B])).to(dev)
                o_d = torch.zeros((nb * B, 6), dtype=torch.float32, device=dev)
                o_i = torch.full((nb * B, 6), -7, dtype=torch.int32, device=dev)
                fl = torch.full((nb * B,), -7, dtype=torch.int32, device=dev)
                idx.search_dev_multi(qd.data_ptr(), nb, B, 5, o_i.data_ptr(), o_d.data_ptr(), fl.data_ptr(),
                                     torch.cuda.current_stream().cuda_stream)
                torch.cuda.synchronize()
                key = f"{name}_nb{nb}"
                res[key + "_i"] = o_i.cpu().numpy()
                res[key + "_d"] = o_d.cpu().numpy()
                res[key + "_f"] = fl.cpu().numpy()
    np.savez(sys.argv[1], **res)


def _run_side(tmp_path, flt):
    out = str(tmp_path / f"ring_{flt}.npz")
    # every batch count takes the seeded streaming scan (the default seeds from 4 batches on)
    env = dict(os.environ, VSEARCH_F32_FILTER=str(flt), VSEARCH_SEED_MIN="1")
    subprocess.run([sys.executable, os.path.abspath(__file__), out], env=env, check=True, timeout=900)
    return dict(np.load(out))


@pytest.mark.gpu
def test_shared_ring_equals_fp32_kernel_bit_for_bit(gpu_pkg, tmp_path):
    a = _run_side(tmp_path, 1)
    b = _run_side(tmp_path, 0)
    assert a.keys() == b.keys() and len(a) == 3 * sum(len(c[5]) for c in CASES)
    for k in a:
        assert np.array_equal(a[k], b[k]), k
    for name, rows, metric, B, id_offset, nbs in CASES:  # the lists are not empty: ids of the shard, offset applied
        ids = a[f"{name}_nb{nbs[-1]}_i"][:, :5]
        assert ((ids >= id_offset) & (ids < id_offset + rows)).all(), name


if __name__ == "__main__":
    _worker(sys.argv[1:])
