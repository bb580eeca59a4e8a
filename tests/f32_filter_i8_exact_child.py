"""Child process of test_gpu_f32_filter_i8_exact.py (the VSEARCH_* toggles are read when the library loads, so every side
is a process of its own):  f32_filter_i8_exact_child.py <repository root> <out .npz>

Runs every launch of LAUNCHES under precision 1 and writes ids, distance bits, flags and the int8 sweep's counters per
launch.  The launch table and the data live here, so that the test module (which imports this file) and the child share
one copy."""
import os
import sys

import numpy as np

K = 5
ROWS = 65_536 + 37   # the smallest shard a seeded launch takes, last unit partial
ROW_LO, ROW_HI = 4321, 65_536 + 20   # planted rows of all 0 and all 255 (the second in the partial last unit)
Q_LO, Q_HI = 3, 6    # queries of all 0 and all 255 in every batch (both below 7)
ID_OFFSET = 3_000_000

# (key, queries per batch, batches, id offset): 4, 9 and 32 batches are 1, 4 and 8 column blocks per wave (8-wave workgroups
# at 4 batches, two 4-wave halves at 9 and 32); 7 queries per batch leave padding queries
LAUNCHES = [(f"b{B}_nb{nb}", B, nb, 0) for B in (32, 7) for nb in (4, 9, 32)] + [("b32_nb9_off", 32, 9, ID_OFFSET)]


def base_rows():
    """Random SIFT-range bytes (no repeated rows: nothing overflows), one row of all 0 and one of all 255."""
    rng = np.random.default_rng(1103)
    g = np.minimum(rng.gamma(1.2, 24.0, (ROWS, 128)), 255).astype(np.int64)
    g[::89] = rng.integers(0, 256, (len(g[::89]), 128))
    g[ROW_LO], g[ROW_HI] = 0, 255
    return g.astype(np.float32)


def queries(B, nb):
    rng = np.random.default_rng(1104)
    q = np.minimum(rng.gamma(1.2, 24.0, (32 * 32, 128)), 255).astype(np.int64)[: nb * B].reshape(nb, B, 128)
    q[:, Q_LO], q[:, Q_HI] = 0, 255
    return np.ascontiguousarray(q.reshape(nb * B, 128), dtype=np.float32)


def main():
    root, out = sys.argv[1], sys.argv[2]
    sys.path.insert(0, root)
    import torch

    import __graft_entry__ as ge

    pkg = ge.load_package()
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream().cuda_stream
    has_filter = os.environ.get("VSEARCH_F32_FILTER") != "0"
    base = base_rows()
    res = {}
    for key, B, nb, id_offset in LAUNCHES:
        with pkg.BruteForceIndex(base, id_offset=id_offset) as idx:
            idx.set_precision(1)
            qd = torch.from_numpy(queries(B, nb)).to(dev)
            o_d = torch.full((nb * B, K + 1), float("nan"), dtype=torch.float32, device=dev)
            o_i = torch.full((nb * B, K + 1), -7, dtype=torch.int32, device=dev)
            fl = torch.full((nb * B,), -7, dtype=torch.int32, device=dev)
            idx.filter_i8_stats(reset=True)
            idx.search_dev_multi(qd.data_ptr(), nb, B, K, o_i.data_ptr(), o_d.data_ptr(), fl.data_ptr(), stream)
            torch.cuda.synchronize()
            res[key + "_i"], res[key + "_d"], res[key + "_f"] = o_i.cpu().numpy(), o_d.cpu().numpy(), fl.cpu().numpy()
            res[key + "_i8"] = np.array(idx.filter_i8_stats(), dtype=np.int64)
            res[key + "_bf16"] = np.array(idx.filter_stats() if has_filter else (0, 0, 0, 0), dtype=np.int64)
            print(f"{key}: int8 stats {res[key + '_i8'].tolist()} prefilter stats {res[key + '_bf16'].tolist()}", flush=True)
    np.savez(out, **res)


if __name__ == "__main__":
    main()
