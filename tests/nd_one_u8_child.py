"""Child process of test_gpu_nd_one_u8.py:  nd_one_u8_child.py <repository root> <out .npz>

Run under VSEARCH_ND_ONE_U8=0 (read when an index is created), so that short calls on the byte rows keep the per-batch
route (reset, nd_prep_i8_kernel, scan_nd_i8_kernel, merge): the calls of run() on the indexes of cases(), written to the
.npz as <case>_<k>_<call>_<batches>_<B>_{i,d,f}, with the single-call counters of each index after its calls as
<case>_stats.  The parent makes the same calls on the default route (scan_one_nd_i8_kernel) and compares."""
import os
import sys

import numpy as np

SHAPES = (("one", 1, 1), ("one", 1, 7), ("one", 1, 12), ("one", 1, 16), ("multi", 3, 12), ("multi", 3, 16))  # (call, batches, queries per batch)
KS = (1, 5, 15)
N, NQ = 20000, 48
BAD_QUERY, BAD_COLUMN = 20, 3  # (in the second batch of the 3 x 12 and 3 x 16 calls, in the only batch of no other shape)


def cases():
    """name -> (base uint8, queries float32, metric): squared L2 at dim 320 (five 64-byte segments: a half step), inner
    product at dim 128 (the general byte form; 16-query batches keep the per-batch route there on both sides)
    and squared L2 at dim 200 with a value that is no byte in query 20"""
    import nd_u8_data
    import nd_u8_ip_data

    out = {}
    base, q = nd_u8_data.u8_data(np.random.default_rng(31000), N, NQ, 320)
    out["l2_320"] = (base, q.astype(np.float32), 0)
    base, q = nd_u8_ip_data.ip_data(np.random.default_rng(31001), N, NQ, 128)
    out["ip_128"] = (base, q.astype(np.float32), 1)
    base, q = nd_u8_data.u8_data(np.random.default_rng(31002), N, NQ, 200)
    q = q.astype(np.float32)
    q[BAD_QUERY, BAD_COLUMN] = 7.5
    out["l2_200_refused"] = (base, q, 0)
    return out


def run(pkg):
    import test_gpu_cancel as tc

    res = {}
    for name, (base, q, metric) in cases().items():
        with pkg.BruteForceIndex.from_u8(base, metric=metric) as idx:
            for k in KS:
                for call, nb, B in SHAPES:
                    gi, gd, fl = tc._bf_dev(idx, q, nb, B, k, call)
                    key = f"{name}_{k}_{call}_{nb}_{B}"
                    res[key + "_i"], res[key + "_d"], res[key + "_f"] = gi, gd, fl
            res[name + "_stats"] = np.array(idx.one_stats(), dtype=np.int64)
    return res


def main():
    root, out = sys.argv[1], sys.argv[2]
    for p in (root, os.path.join(root, "tests")):
        if p not in sys.path:
            sys.path.insert(0, p)
    assert os.environ.get("VSEARCH_ND_ONE_U8") == "0"
    import __graft_entry__ as ge

    np.savez(out, **run(ge.load_package()))
    print("ND_ONE_U8_CHILD_OK")


if __name__ == "__main__":
    main()
