"""Child process of test_gpu_nd_wide_u8.py:  nd_wide_u8_child.py <repository root> <out .npz>

Run under VSEARCH_ND_WIDE_U8=0 (read when an index is created), so that wide calls (k >= 16) on an index with byte rows
keep the fp32 launches: the calls of run() on the indexes of cases(), written to the .npz as <case>_<k>_{i,d,f} (device
call) and <case>_<k>_{hi,hd} (host call), with vs_bf_wide_stats of each index after its calls as <case>_stats.  The parent
makes the same calls on the default route (the byte rows) and compares."""
import os
import sys

import numpy as np

KS = (16, 100)
NQ, B = 40, 20
BAD_QUERY, BAD_COLUMN = 25, 3  # (in the second batch)


def dev_topk(idx, q, nb, B, k):
    """search_topk_dev_multi on the first nb * B queries: ids, dists, flags"""
    import torch
    dev = torch.device("cuda:0")
    n = nb * B
    qd = torch.from_numpy(np.array(q[:n], dtype=np.float32)).to(dev)
    oi = torch.full((n, k + 1), -7, dtype=torch.int32, device=dev)
    od = torch.full((n, k + 1), 7.0, dtype=torch.float32, device=dev)
    fl = torch.full((n,), -7, dtype=torch.int32, device=dev)
    idx.search_topk_dev_multi(qd.data_ptr(), nb, B, k, oi.data_ptr(), od.data_ptr(), fl.data_ptr(),
                              torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return oi.cpu().numpy(), od.cpu().numpy(), fl.cpu().numpy()


def cases(pkg):
    """name -> (base uint8, queries float32, metric): squared L2 at dim 200 and inner product at dim 96, each with rows
    behind the prefix of either k (three full blocks and a ragged one behind the longer one), and squared L2 at dim 65
    with a value that is no byte in query 25"""
    import nd_u8_data
    import nd_u8_ip_data

    n = pkg.BruteForceIndex.wide_plan(10 ** 5, 96, max(KS))[1] + 209
    out = {}
    base, q = nd_u8_data.u8_data(np.random.default_rng(41000), n, NQ, 200)
    out["l2_200"] = (base, q.astype(np.float32), 0)
    base, q = nd_u8_ip_data.ip_data(np.random.default_rng(41001), n, NQ, 96)
    out["ip_96"] = (base, q.astype(np.float32), 1)
    base, q = nd_u8_data.u8_data(np.random.default_rng(41002), n, NQ, 65)
    q = q.astype(np.float32)
    q[BAD_QUERY, BAD_COLUMN] = 7.5
    out["l2_65_refused"] = (base, q, 0)
    return out


def run(pkg):
    res = {}
    for name, (base, q, metric) in cases(pkg).items():
        with pkg.BruteForceIndex.from_u8(base, metric=metric) as idx:
            idx.set_batch(B)
            for k in KS:
                key = f"{name}_{k}"
                res[key + "_i"], res[key + "_d"], res[key + "_f"] = dev_topk(idx, q, NQ // B, B, k)
                res[key + "_hi"], res[key + "_hd"] = idx.search_topk(q, k)
            res[name + "_stats"] = np.array(idx.wide_stats(), dtype=np.int64)
    return res


def main():
    root, out = sys.argv[1], sys.argv[2]
    for p in (root, os.path.join(root, "tests")):
        if p not in sys.path:
            sys.path.insert(0, p)
    assert os.environ.get("VSEARCH_ND_WIDE_U8") == "0"
    import __graft_entry__ as ge

    np.savez(out, **run(ge.load_package()))
    print("ND_WIDE_U8_CHILD_OK")


if __name__ == "__main__":
    main()
