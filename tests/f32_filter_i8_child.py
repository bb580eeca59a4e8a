"""Child process of test_gpu_f32_filter_i8.py (the VSEARCH_* toggles are read when the library loads, so every leg is a
process of its own):  f32_filter_i8_child.py <repository root> <out .npz>

Runs every launch of LAUNCHES under precision 1 and writes ids, distance bits, flags and both counters
(filter_stats, filter_i8_stats; zeros where the leg has no prefilter) per launch.  The launch table and the data live
here, so that the test module (which imports this file) and the child share one copy."""
import os
import sys

import numpy as np

K = 5
ROWS_A = 65_536 + 37   # the smallest shard a seeded launch takes, last unit partial
ROWS_B = 131_072
NQ = 32 * 32

# (key, base, metric, queries per batch, batches, id offset, query set)
LAUNCHES = (
    [(f"a_b32_nb{nb}", "A", 0, 32, nb, 0, "bytes") for nb in (4, 5, 9, 17, 32)]      # CBW 1 / 2 / 4 / 8, both NW
    + [(f"a_b7_nb{nb}", "A", 0, 7, nb, 0, "bytes") for nb in (4, 5, 9, 17, 32)]      # padding queries
    + [("a_off_nb9", "A", 0, 32, 9, 3_000_000, "bytes")]
    + [(f"b_b32_nb{nb}", "B", 0, 32, nb, 0, "bytes") for nb in (4, 32)]
    + [("a_mixed_nb9", "A", 0, 32, 9, 0, "mixed"), ("a_ties_nb4", "A", 0, 8, 4, 0, "ties")]
    + [("o_over_nb4", "O", 0, 32, 4, 0, "over")]
    + [("a_ip_nb4", "A", 1, 32, 4, 0, "bytes")]
)
ALL_BYTES = [l[0] for l in LAUNCHES if l[6] == "bytes" and l[2] == 0]


def base_rows(which):
    """Byte-valued rows: SIFT-like small values with full-range rows among them, rows of all 0 and all 255, and twelve
    rows around each of the first 256 queries at nearly and exactly equal distances."""
    if which == "O":  # 64 distinct rows, repeated: thousands of rows under every bound
        rng = np.random.default_rng(77)
        return np.tile(rng.integers(0, 256, (64, 128)).astype(np.float32), (ROWS_B // 64, 1))
    rows = ROWS_A if which == "A" else ROWS_B
    rng = np.random.default_rng(4100 + ord(which))
    g = np.minimum(rng.gamma(1.2, 24.0, (rows, 128)), 255).astype(np.int64)
    g[::97] = rng.integers(0, 256, (len(g[::97]), 128))
    g[5], g[6] = 0, 255
    q = queries(which, raw=True)
    # row m of query i has `count` components moved by one, so it lies at distance `count`: m + 1 for an even i (neighbouring
    # integers: as near as byte-valued distances get without a tie), 4 + (m >> 2) for an odd i (ties of four)
    even = (np.arange(256) % 2 == 0)[:, None]
    for m in range(12):
        blk = q[:256].copy()
        count = np.where(even, m + 1, 4 + (m >> 2))
        for c in range(12):
            col = (7 * m + c) % 128
            step = np.where(blk[:, col] < 255, 1, -1)[:, None]
            blk[:, col:col + 1] += np.where(c < count, step, 0)
        g[1000 + 256 * m: 1000 + 256 * (m + 1)] = blk
    return g.astype(np.float32)


def queries(which, raw=False):
    """Byte-valued queries near nothing in particular, with 0 and 255 among their values and two constant queries."""
    rng = np.random.default_rng(9100 + ord(which))
    q = np.minimum(rng.gamma(1.2, 24.0, (NQ, 128)), 255).astype(np.int64)
    q[:, 3] = np.where(np.arange(NQ) % 3 == 0, 255, q[:, 3])
    q[:, 9] = np.where(np.arange(NQ) % 5 == 0, 0, q[:, 9])
    q[40], q[41] = 0, 255
    return q if raw else q.astype(np.float32)


def query_set(kind, base, which):
    if kind == "over":  # the rows themselves: 2048 copies at distance 0
        return base[:NQ].copy()
    q = queries(which)
    if kind == "mixed":  # batch 2 carries a value of 0.5, batch 7 a value of 256
        q[2 * 32 + 3, 17] = 0.5
        q[7 * 32 + 31, 127] = 256.0
    if kind == "ties":  # on the bisecting hyperplane of their 5th and 6th nearest rows, a few ulps off it (not byte valued)
        import near_ties
        q, _ = near_ties.boundary_queries(base, q[:4 * 8], K, np.random.default_rng(5), rounds=3)
    return np.ascontiguousarray(q, dtype=np.float32)


def main():
    root, out = sys.argv[1], sys.argv[2]
    sys.path.insert(0, root)
    sys.path.insert(0, os.path.join(root, "tests"))
    import torch

    import __graft_entry__ as ge

    pkg = ge.load_package()
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream().cuda_stream
    has_filter = os.environ.get("VSEARCH_F32_FILTER") != "0"
    res, bases = {}, {}
    for key, which, metric, B, nb, id_offset, kind in LAUNCHES:
        if which not in bases:
            bases[which] = base_rows(which)
        base = bases[which]
        q = query_set(kind, base, which)
        with pkg.BruteForceIndex(base, metric=metric, id_offset=id_offset) as idx:
            idx.set_precision(1)
            qd = torch.from_numpy(np.ascontiguousarray(q[: nb * B])).to(dev)
            o_d = torch.full((nb * B, K + 1), float("nan"), dtype=torch.float32, device=dev)
            o_i = torch.full((nb * B, K + 1), -7, dtype=torch.int32, device=dev)
            fl = torch.full((nb * B,), -7, dtype=torch.int32, device=dev)
            idx.filter_i8_stats(reset=True)
            if has_filter:
                idx.filter_stats(reset=True)
            idx.search_dev_multi(qd.data_ptr(), nb, B, K, o_i.data_ptr(), o_d.data_ptr(), fl.data_ptr(), stream)
            torch.cuda.synchronize()
            res[key + "_i"], res[key + "_d"], res[key + "_f"] = o_i.cpu().numpy(), o_d.cpu().numpy(), fl.cpu().numpy()
            res[key + "_bf16"] = np.array(idx.filter_stats() if has_filter else (0, 0, 0, 0), dtype=np.int64)
            res[key + "_i8"] = np.array(idx.filter_i8_stats(), dtype=np.int64)
            res[key + "_plan"] = np.array(int(idx.filter_i8_plan(nb, K)))
            print(f"{key}: bf16 stats {res[key + '_bf16'].tolist()} int8 stats {res[key + '_i8'].tolist()}", flush=True)
    np.savez(out, **res)


if __name__ == "__main__":
    main()
