"""Child process of test_gpu_seed_block.py (VSEARCH_SEED_I8 and its neighbours are read when the library loads, so every
side is a process of its own):  seed_block_child.py <repository root> <out .npz>

Runs every launch of LAUNCHES on one handle per shard and writes ids, distance bits, flags and the counters of the int8
and the bf16 sweep per launch.  The launch table and the data live here, so that the test module (which imports this
file) and the child share one copy."""
import sys

import numpy as np

K = 5
ROWS = {"even": 65_536, "ragged": 65_536 + 37}   # the smallest shard a seeded launch takes; the second with a partial last tile
MIXED_ONE = (1, 3)    # (batch, query) set to x + 0.5: the second batch of a block at every block size
MIXED_LAST = 8        # of 9 batches: every query set to x + 0.5 (a block of one at every block size)

# (key, shard, queries per batch, batches, precision, query set)
#   "head": the first batches of the query set          "mixed_one" / "mixed_last": head with the changes above
#   "tail": the query set backwards (other queries in every batch than the launch before it on the handle)
LAUNCHES = [(f"{w}_b{B}_nb{nb}", w, B, nb, 1, "head") for w in ("even", "ragged") for B in (32, 17, 1) for nb in (4, 5, 7, 8, 9, 32)]
LAUNCHES += [("ragged_mixed_one", "ragged", 32, 9, 1, "mixed_one"), ("ragged_mixed_last", "ragged", 32, 9, 1, "mixed_last"),
             # one handle, two group sizes in a row: 32 batches, then 5 with other queries
             ("ragged_long", "ragged", 32, 32, 1, "head"), ("ragged_short_after_long", "ragged", 32, 5, 1, "tail"),
             ("ragged_prec2", "ragged", 32, 8, 2, "head")]


def base_rows(pkg, which):
    return pkg.synth_sift(ROWS["ragged"], seed=1)[: ROWS[which]]   # (the even shard is the ragged one without its last 37 rows)


def query_set(pkg, kind, B, nb):
    q = pkg.synth_sift(1024, seed=2)
    if kind == "tail":
        q = q[::-1]
    q = np.ascontiguousarray(q[: nb * B]).reshape(nb, B, 128)
    if kind == "mixed_one":
        q[MIXED_ONE[0], MIXED_ONE[1]] += 0.5
    elif kind == "mixed_last":
        q[MIXED_LAST] += 0.5
    return q.reshape(nb * B, 128)


def main():
    root, out = sys.argv[1], sys.argv[2]
    sys.path.insert(0, root)
    import torch

    import __graft_entry__ as ge

    pkg = ge.load_package()
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream().cuda_stream
    res = {}
    for which in ROWS:
        with pkg.BruteForceIndex(base_rows(pkg, which)) as idx:
            for key, w, B, nb, prec, kind in LAUNCHES:
                if w != which:
                    continue
                idx.set_precision(prec)
                qd = torch.from_numpy(query_set(pkg, kind, B, nb)).to(dev)
                o_d = torch.full((nb * B, K + 1), float("nan"), dtype=torch.float32, device=dev)
                o_i = torch.full((nb * B, K + 1), -7, dtype=torch.int32, device=dev)
                fl = torch.full((nb * B,), -7, dtype=torch.int32, device=dev)
                idx.filter_i8_stats(reset=True)
                idx.filter_stats(reset=True)
                idx.search_dev_multi(qd.data_ptr(), nb, B, K, o_i.data_ptr(), o_d.data_ptr(), fl.data_ptr(), stream)
                torch.cuda.synchronize()
                res[key + "_i"], res[key + "_d"], res[key + "_f"] = o_i.cpu().numpy(), o_d.cpu().numpy(), fl.cpu().numpy()
                res[key + "_i8"] = np.array(idx.filter_i8_stats(), dtype=np.int64)
                res[key + "_bf16"] = np.array(idx.filter_stats(), dtype=np.int64)
                print(f"{key}: int8 stats {res[key + '_i8'].tolist()} bf16 stats {res[key + '_bf16'].tolist()}", flush=True)
    np.savez(out, **res)


if __name__ == "__main__":
    main()
