"""Child process of test_gpu_mixed_batches.py (the VSEARCH_* knobs are read when the library loads, so every knob setting
is a process of its own):  mixed_batches_child.py <repository root> <data .npz> <task>,<task>,...

A task is matrix:X (the launch matrix of base X), rerun:X (what a caller does with flags == 2) or edges:L (values at the
edges of the byte range).  Every launch is one search_dev_multi call, compared with the exact integer lists in the data
file (and, for a live query that the task changes itself, with lists computed here by the same function).  One line per
launch that misses, "CASE <launch> FAIL <what>", and one per task, "TASK <task> OK" or "TASK <task> FAIL <launches>"; a
failed assertion ends its launch only, any other error ends the process.

The launch tables and the reference live here as well, so that the test module (which imports this file) and the child
share one copy."""
import sys

import numpy as np

KK = 16  # reference entries per query: k + 1 for the largest k
BK = ((32, 5), (32, 15), (16, 5), (16, 15), (20, 5))  # scan_kernel<2|1, 8|16, kModeTopK, 1>, and padding columns
ROWS = {"S": 3000, "M": 40000, "L": 65537, "D": 100000}
NQ = {"S": 3 * 32, "M": 3 * 32, "L": 9 * 32, "D": 5 * 32}
_THREE = [(3, s) for s in ((0,), (1,), (2,), (0, 1), (0, 2), (0, 1, 2))]
MATRIX = {
    "S": _THREE,
    "M": _THREE,
    "L": _THREE + [(8, s) for s in ((0,), (3,), (4,), (1, 2), (7,), (0, 1, 2, 3), (1, 3, 5, 7), tuple(range(8)))]
    + [(9, (8,)), (9, (4,))],
    "D": [(5, (0,)), (5, (2,))],
}
RERUN = [(3, (1,), 256.0), (3, (0, 2), -1.0)]
EDGE_OK = (255.0, -0.0)
EDGE_BAD = (256.0, -1.0, 0.5, float(np.nextafter(np.float32(255), np.float32(0))), 3e9, -3e9, float("inf"), float("nan"))


def plant_pos(li, b, B):
    """Row (within the batch) and column of the planted element of batch b in launch li: row B - 1, row 0 and rows in
    between, column 127, column 0 and columns in between."""
    rs, cs = (li + b) % 3, (li + 2 * b) % 3
    row = B - 1 if rs == 0 else (0 if rs == 1 else (7 * li + 3 * b + 1) % B)
    col = 127 if cs == 0 else (0 if cs == 1 else (37 * li + 11 * b + 5) % 128)
    return row, col


def d_queries(q, ov, B):
    """Base D's queries for batches of B: the two overflowing queries are the first two of batch 1."""
    q = q.copy()
    q[B], q[B + 1] = ov[0], ov[1]
    return q


def d_lists(ri, rd, ov_ri, ov_rd, B):
    ri, rd = ri.copy(), rd.copy()
    ri[B:B + 2], rd[B:B + 2] = ov_ri, ov_rd
    return ri, rd


def exact_lists(q, base_u8, kk=KK):
    """The kk nearest rows of every query by (squared distance, id), from exact integer distances: the products are taken
    in float64, where every partial sum is an integer below 2^53.  Returns ids int32 [nq, kk] and distances float32
    [nq, kk] (exact: every distance is below 2^24, which is asserted)."""
    q64 = np.asarray(q, dtype=np.float64)
    assert np.array_equal(q64, np.rint(q64))
    b64 = base_u8.astype(np.float64)
    d = (q64 * q64).sum(1)[:, None] + (b64 * b64).sum(1)[None, :] - 2.0 * (q64 @ b64.T)
    d = d.astype(np.int64)
    assert d.min() >= 0 and d.max() < 1 << 24 and base_u8.shape[0] <= 1 << 17
    key = (d << 17) | np.arange(base_u8.shape[0], dtype=np.int64)[None, :]
    key = np.sort(np.partition(key, kk - 1, axis=1)[:, :kk], axis=1)
    return (key & ((1 << 17) - 1)).astype(np.int32), (key >> 17).astype(np.float32)


def tied(rd, k):
    """Queries whose k + 1 nearest hold two equal distances."""
    return (np.diff(rd[:, :k + 1], axis=1) == 0).any(axis=1)


def live_mask(nb, B, skipped):
    m = np.ones(nb * B, dtype=bool)
    for b in skipped:
        m[b * B:(b + 1) * B] = False
    return m


def check_cap(rd, nb, B, k, skipped, by_construction=()):
    """At least 99 % of a launch's live queries are checked id for id (queries tied by construction aside)."""
    m = live_mask(nb, B, skipped)
    m[list(by_construction)] = False
    if m.any():
        share = tied(rd[:nb * B], k)[m].mean()
        assert share <= 0.01, (nb, B, k, skipped, share)


def main():
    root, data_path, tasks = sys.argv[1], sys.argv[2], sys.argv[3].split(",")
    sys.path.insert(0, root)
    import torch

    import __graft_entry__ as ge

    pkg = ge.load_package()
    data = np.load(data_path)
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream().cuda_stream

    def launch(idx, qd, nb, B, k):
        """One search_dev_multi call into outputs prefilled with -7 / NaN."""
        nq = nb * B
        o_d = torch.full((nq, k + 1), float("nan"), dtype=torch.float32, device=dev)
        o_i = torch.full((nq, k + 1), -7, dtype=torch.int32, device=dev)
        fl = torch.full((nq,), -7, dtype=torch.int32, device=dev)
        idx.search_dev_multi(qd.data_ptr(), nb, B, k, o_i.data_ptr(), o_d.data_ptr(), fl.data_ptr(), stream)
        torch.cuda.synchronize()
        return o_i.cpu().numpy(), o_d.cpu().numpy(), fl.cpu().numpy()

    def check(out, q, base_u8, ri, rd, nb, B, k, skipped, flags_only=()):
        """out against the reference lists ri, rd of the queries q as launched; of the skipped batches in flags_only
        (non-finite plants) only the flags are looked at."""
        gi, gd, f = out
        nq, kk = nb * B, k + 1
        live = live_mask(nb, B, skipped)
        assert (f[~live] == 2).all(), ("skipped batches not flagged 2", f)
        empty = ~live & live_mask(nb, B, flags_only)
        assert (gi[empty] == -1).all() and np.isposinf(gd[empty]).all(), "lists of a skipped batch are not -1 / +inf"
        assert np.isin(f[live], (0, 1)).all(), ("flags of the live batches", np.unique(f[live]))
        ref_i, ref_d = ri[:nq, :kk], rd[:nq, :kk]
        bad = np.flatnonzero(live & (gd.view(np.uint32) != ref_d.view(np.uint32)).any(axis=1))
        assert bad.size == 0, ("distances differ from the reference, queries", bad[:8], gd[bad[:1]], ref_d[bad[:1]])
        assert np.array_equal(f[live] == 1, tied(ref_d, k)[live]), "flag 1 is not 'an equal pair among the k + 1'"
        plain = live & (f == 0)
        bad = np.flatnonzero(plain & (gi != ref_i).any(axis=1))
        assert bad.size == 0, ("ids differ from the reference, queries", bad[:8], gi[bad[:1]], ref_i[bad[:1]])
        for i in np.flatnonzero(live & (f == 1)):  # a valid tie order: distinct rows at exactly the returned distances
            ids = gi[i].astype(np.int64)
            assert ids.min() >= 0 and ids.max() < base_u8.shape[0] and np.unique(ids).size == kk, (i, ids)
            diff = q[i].astype(np.int64)[None, :] - base_u8[ids].astype(np.int64)
            assert np.array_equal((diff * diff).sum(1).astype(np.float32), gd[i]), (i, ids)

    def same_bytes(a, b):
        return all(x.tobytes() == y.tobytes() for x, y in zip(a, b))

    def load_base(X, B):
        base_u8, q, ri, rd = data["base_" + X], data["q_" + X], data["ri_" + X], data["rd_" + X]
        if X == "D":
            q = d_queries(q, data["ov_q"], B)
            ri, rd = d_lists(ri, rd, data["ov_ri"], data["ov_rd"], B)
        return base_u8, q, ri, rd

    def planted(q, ri, rd, base_u8, nb, B, plants, relist):
        """q with plants {batch: (row, col, value)} applied; relist: the lists of the changed queries are recomputed."""
        q, ri, rd = q[:nb * B].copy(), ri[:nb * B].copy(), rd[:nb * B].copy()
        rows = []
        for b, (row, col, v) in plants.items():
            q[b * B + row, col] = v
            rows.append(b * B + row)
        if relist:
            rows = [i for i in rows if i in relist]
            if rows:
                ri[rows], rd[rows] = exact_lists(q[rows], base_u8)
        return q, ri, rd

    failed = []

    def case(tag, body):
        """One launch (with what is issued behind it): a failed assertion is reported and the task goes on."""
        try:
            body()
        except AssertionError as e:
            failed.append(tag)
            print(f"CASE {tag} FAIL {str(e.args)[:400]}", flush=True)

    def task_matrix(idx, X):
        for B, k in BK:
            base_u8, q, ri, rd = load_base(X, B)
            clean = torch.from_numpy(q).to(dev)
            for li, (nb, skipped) in enumerate(MATRIX[X]):
                check_cap(rd, nb, B, k, skipped, (B, B + 1) if X == "D" else ())
                qp, _, _ = planted(q, ri, rd, base_u8, nb, B, {b: plant_pos(li, b, B) + (7.5,) for b in skipped}, None)
                qd = torch.from_numpy(qp).to(dev)

                def body():
                    idx.set_precision(2)
                    first = launch(idx, qd, nb, B, k)
                    again = launch(idx, qd, nb, B, k)
                    after = launch(idx, clean, nb, B, k)  # byte-valued batches only, right behind: no stale verdict
                    check(first, qp, base_u8, ri, rd, nb, B, k, skipped)
                    assert same_bytes(first, again), "the same launch a second time gives other bytes"
                    check(after, q, base_u8, ri, rd, nb, B, k, ())
                    if li == 1 and (B, k) == BK[0]:  # precision 0 takes the same path
                        idx.set_precision(0)
                        auto = launch(idx, qd, nb, B, k)
                        check(auto, qp, base_u8, ri, rd, nb, B, k, skipped)
                        assert same_bytes(first, auto), "precision 0 gives other bytes than precision 2"

                case(("matrix", X, nb, B, k, skipped), body)

    def task_rerun(idx, X):
        for B, k in BK:
            base_u8, q, ri, rd = load_base(X, B)
            for li, (nb, skipped, v) in enumerate(RERUN):
                plants = {b: plant_pos(li, b, B) + (v,) for b in skipped}
                # (exact_lists asserts that the planted queries' distances stay below 2^24 as well)
                qp, pi, pd = planted(q, ri, rd, base_u8, nb, B, plants, set(range(nb * B)))
                qd = torch.from_numpy(qp).to(dev)

                def body():
                    idx.set_precision(2)
                    check(launch(idx, qd, nb, B, k), qp, base_u8, ri, rd, nb, B, k, skipped)
                    idx.set_precision(1)  # what the caller is told to do: every batch, the planted ones included
                    check(launch(idx, qd, nb, B, k), qp, base_u8, pi, pd, nb, B, k, ())

                case(("rerun", X, nb, B, k, skipped, v), body)

    def task_edges(idx, X):
        B, k = 32, 5
        base_u8, q, ri, rd = load_base(X, B)
        # a bad value in the even batches, 255.0 / -0.0 in the odd ones: a live batch behind every skipped one
        rows = [[EDGE_BAD[i], 255.0, EDGE_BAD[i + 1], -0.0, EDGE_BAD[i + 2], 255.0, EDGE_BAD[i + 3], -0.0] for i in (0, 4)]
        rows += [[v, 255.0, -0.0] for v in EDGE_BAD] + [[255.0, -0.0, v] for v in EDGE_BAD[:2]]
        idx.set_precision(2)
        for li, vals in enumerate(rows):
            nb = len(vals)
            plants = {b: plant_pos(li, b, B) + (v,) for b, v in enumerate(vals)}
            skipped = tuple(b for b, v in enumerate(vals) if v not in EDGE_OK)
            ok_rows = {b * B + plants[b][0] for b in range(nb) if b not in skipped}
            qp, pi, pd = planted(q, ri, rd, base_u8, nb, B, plants, ok_rows)
            flags_only = tuple(b for b, v in enumerate(vals) if not np.isfinite(v))

            def body():
                out = launch(idx, torch.from_numpy(qp).to(dev), nb, B, k)
                check(out, qp, base_u8, pi, pd, nb, B, k, skipped, flags_only)

            case(("edges", X, nb, tuple(vals)), body)

    run = {"matrix": task_matrix, "rerun": task_rerun, "edges": task_edges}
    for X in "SMLD":
        mine = [t for t in tasks if t.endswith(":" + X)]
        if not mine:
            continue
        with pkg.BruteForceIndex(data["base_" + X].astype(np.float32)) as idx:
            for t in mine:
                del failed[:]
                run[t.split(":")[0]](idx, X)
                print(f"TASK {t} " + (f"FAIL {len(failed)} cases: {failed}"[:3000] if failed else "OK"), flush=True)
    print("MIXED_BATCHES_DONE")


if __name__ == "__main__":
    main()
