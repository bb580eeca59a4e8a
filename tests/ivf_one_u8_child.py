"""Child process of test_gpu_ivf_one_u8.py:  ivf_one_u8_child.py <repository root> <out .npz> <toggle_u8 | toggle_one | forced>

  toggle_u8  : run under VSEARCH_IVF_ONE_U8=0 (read when an IVF index is created): the short calls of CALLS on the byte
               index over the 100-d integer set of test_gpu_ivf_nd.py keep the group route.
  toggle_one : the same under VSEARCH_IVF_ONE=0, which turns both short routes off.
  forced     : run under VSEARCH_IVF_ND_FORCE=1: vs_ivf_create_nd_u8 at dim 128 builds the GENERAL byte index and its short
               calls take the byte route.

Each writes the calls' outputs as i<n>, d<n>, and per call what IVFIndex.one_u8_stats() and nd_u8_stats() counted (-1 where
the index is not a general one and has no such counters); the parent makes the same calls in its own process and compares."""
import os
import sys

import numpy as np

# (batches, queries per batch, k, nprobe, metric): short calls
CALLS = [(1, 1, 10, 8, 0), (1, 16, 5, 4, 0), (3, 16, 16, 24, 0), (2, 7, 1, 1, 0), (2, 16, 5, 4, 1)]


def mixed_queries(q):
    """every third query carries a value that is no byte"""
    q = np.array(q[:48])
    for j, i in enumerate(range(1, 48, 3)):
        q[i, (7 * j) % q.shape[1]] = (0.5, 256.0, -1.0)[j % 3]
    return q


def _calls(pkg, ivf, q, counted):
    import torch

    dev = torch.device("cuda:0")
    res, one, nd = {}, [], []
    for n, (nb, B, k, nprobe, metric) in enumerate(CALLS):
        if counted:
            ivf.one_u8_stats(reset=True)
            ivf.nd_u8_stats(reset=True)
        qd = torch.from_numpy(np.array(q[:nb * B])).to(dev)
        oi = torch.full((nb * B, k), -7, dtype=torch.int32, device=dev)
        od = torch.full((nb * B, k), 7.0, dtype=torch.float32, device=dev)
        ivf.search_metric_dev_multi(qd.data_ptr(), nb, B, k, nprobe, metric, oi.data_ptr(), od.data_ptr(), torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        res[f"i{n}"], res[f"d{n}"] = oi.cpu().numpy(), od.cpu().numpy()
        one.append(ivf.one_u8_stats() if counted else (-1, -1, -1))
        nd.append(ivf.nd_u8_stats() if counted else (-1, -1))
        if counted:
            assert ivf.one_stats() == (0, 0)
    res["one_u8"], res["nd_u8"] = np.array(one), np.array(nd)
    return res


def run_toggle(pkg):
    from test_gpu_ivf_nd import _int_index

    vr, cents, off, r2o, q = _int_index(100)
    with pkg.IVFIndex.from_u8(vr.astype(np.uint8), cents, off, r2o) as ivf:
        return _calls(pkg, ivf, mixed_queries(q), True)


def run_forced(pkg, want_general):
    from test_gpu_ivf_nd import _int_index

    vr, cents, off, r2o, q = _int_index(128)
    with pkg.IVFIndex.from_u8(vr.astype(np.uint8), cents, off, r2o) as ivf:
        out = (__import__("ctypes").c_int64 * 2)()
        general = pkg.lib().vs_ivf_nd_u8_stats(ivf._h, out, 0) == 0
        assert bool(general) == want_general
        res = _calls(pkg, ivf, np.array(q[:48]), general)  # (byte-valued queries: the specialised index has no per-query rule to compare)
    res["general"] = np.array(bool(general))
    return res


def main():
    root, out, mode = sys.argv[1], sys.argv[2], sys.argv[3]
    for p in (root, os.path.join(root, "tests")):
        if p not in sys.path:
            sys.path.insert(0, p)
    import __graft_entry__ as ge

    pkg = ge.load_package()
    if mode == "toggle_u8":
        assert os.environ.get("VSEARCH_IVF_ONE_U8") == "0" and "VSEARCH_IVF_ONE" not in os.environ
        res = run_toggle(pkg)
    elif mode == "toggle_one":
        assert os.environ.get("VSEARCH_IVF_ONE") == "0" and "VSEARCH_IVF_ONE_U8" not in os.environ
        res = run_toggle(pkg)
    else:
        assert os.environ.get("VSEARCH_IVF_ND_FORCE") == "1"
        res = run_forced(pkg, want_general=True)
    np.savez(out, **res)
    print("IVF_ONE_U8_CHILD_OK")


if __name__ == "__main__":
    main()
