"""Child process of test_gpu_nd_one.py:  nd_one_child.py <repository root> <out .npz>

Run under VSEARCH_ND_FORCE=1 (read when the library loads), so that vs_bf_create builds the GENERAL index at dim 128 and
short calls take scan_one_nd_kernel there: the calls of CALLS on cancel_data.case(*KEY), written to the .npz as i<k>,
d<k>, f<k>.  The parent makes the same calls on the specialised index (scan_one_kernel) and compares."""
import os
import sys

import numpy as np

KEY = (3000, 48, 128, 4)
NB, B = 3, 16
KS = (1, 5, 15)


def run(pkg, want_route):
    """the calls on an index over KEY's rows at precision 1, after asserting the route the plan gives them"""
    import torch

    import cancel_data

    base, q, _ = cancel_data.case(*KEY)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    dev = torch.device("cuda:0")
    res = {}
    with pkg.BruteForceIndex(base) as idx:
        idx.set_precision(1)
        for k in KS:
            assert pkg.BruteForceIndex.one_plan(len(base), 128, cus, NB, B, k)[0] == want_route
            qd = torch.from_numpy(np.array(q[:NB * B])).to(dev)
            oi = torch.full((NB * B, k + 1), -7, dtype=torch.int32, device=dev)
            od = torch.full((NB * B, k + 1), 7.0, dtype=torch.float32, device=dev)
            fl = torch.full((NB * B,), -7, dtype=torch.int32, device=dev)
            idx.search_dev_multi(qd.data_ptr(), NB, B, k, oi.data_ptr(), od.data_ptr(), fl.data_ptr(),
                                 torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
            res[f"i{k}"], res[f"d{k}"], res[f"f{k}"] = oi.cpu().numpy(), od.cpu().numpy(), fl.cpu().numpy()
    return res


def main():
    root, out = sys.argv[1], sys.argv[2]
    for p in (root, os.path.join(root, "tests")):
        if p not in sys.path:
            sys.path.insert(0, p)
    assert os.environ.get("VSEARCH_ND_FORCE") == "1"
    import __graft_entry__ as ge

    np.savez(out, **run(ge.load_package(), 2))
    print("ND_ONE_CHILD_OK")


if __name__ == "__main__":
    main()
