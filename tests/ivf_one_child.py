"""Child process of test_gpu_ivf_one.py:  ivf_one_child.py <repository root> <out .npz> <toggle | forced>

  toggle : run under VSEARCH_IVF_ONE=0 (read when an IVF index is created): the short calls of CALLS on the 100-d integer
           index of test_gpu_ivf_nd.py keep the group route.
  forced : run under VSEARCH_IVF_ND_FORCE=1: vs_ivf_create builds the GENERAL index over 128-d synth_sift rows and its
           short calls take the two-launch route.

Both write the calls' outputs as i<n>, d<n> and the batches IVFIndex.one_stats() counted per call (-1 where the index is not
a general one and has no such counter); the parent makes the same calls in its own process and compares."""
import os
import sys

import numpy as np

# (batches, queries per batch, k, nprobe): short calls
CALLS = [(1, 1, 10, 8), (1, 16, 5, 4), (3, 16, 16, 24), (2, 7, 1, 1)]


def _calls(pkg, ivf, q, counted):
    import torch

    dev = torch.device("cuda:0")
    res, batches = {}, []
    for n, (nb, B, k, nprobe) in enumerate(CALLS):
        if counted:
            ivf.one_stats(reset=True)
        qd = torch.from_numpy(np.array(q[:nb * B])).to(dev)
        oi = torch.full((nb * B, k), -7, dtype=torch.int32, device=dev)
        od = torch.full((nb * B, k), 7.0, dtype=torch.float32, device=dev)
        ivf.search_dev_multi(qd.data_ptr(), nb, B, k, nprobe, oi.data_ptr(), od.data_ptr(), torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        res[f"i{n}"], res[f"d{n}"] = oi.cpu().numpy(), od.cpu().numpy()
        batches.append(ivf.one_stats()[0] if counted else -1)
    res["batches"] = np.array(batches)
    return res


def run_toggle(pkg):
    from test_gpu_ivf_nd import _int_index

    vr, cents, off, r2o, q = _int_index(100)
    with pkg.IVFIndex(vectors_reordered=vr, centroids=cents, cluster_offsets=off, reorder_to_original=r2o) as ivf:
        return _calls(pkg, ivf, q, True)


def run_forced(pkg, want_general):
    base = pkg.synth_sift(20000, seed=41)
    q = pkg.synth_sift(48, seed=42)
    cents = base[:: len(base) // 64][:64].copy()
    b, c = base.astype(np.int64), cents.astype(np.int64)
    assign = ((b * b).sum(1)[:, None] - 2 * (b @ c.T) + (c * c).sum(1)[None, :]).argmin(1)
    vr, off, r2o = pkg.ivf_layout_from_assignment(base, assign, 64)
    with pkg.IVFIndex(vectors_reordered=vr, centroids=cents, cluster_offsets=off, reorder_to_original=r2o) as ivf:
        general = pkg.lib().vs_set_precision(ivf._h, 2) == -5 and b"dim = 128" in pkg.lib().vs_last_error()
        assert bool(general) == want_general
        ivf.set_precision(1)
        res = _calls(pkg, ivf, q, general)
    res["general"] = np.array(bool(general))
    return res


def main():
    root, out, mode = sys.argv[1], sys.argv[2], sys.argv[3]
    for p in (root, os.path.join(root, "tests")):
        if p not in sys.path:
            sys.path.insert(0, p)
    import __graft_entry__ as ge

    pkg = ge.load_package()
    if mode == "toggle":
        assert os.environ.get("VSEARCH_IVF_ONE") == "0"
        res = run_toggle(pkg)
    else:
        assert os.environ.get("VSEARCH_IVF_ND_FORCE") == "1"
        res = run_forced(pkg, want_general=True)
    np.savez(out, **res)
    print("IVF_ONE_CHILD_OK")


if __name__ == "__main__":
    main()
