"""Inner-product brute force (VS_METRIC_IP) against an exact numpy reference, on every scan path of the library.

Integer-valued data, so that the float64 product q @ base.T is the exact score and -- while dim * max|q| * max|b| < 2^24 --
so is every fp32 partial sum a kernel can form, in any order: scores must match bit for bit (compared by value, so that
-0.0 == +0.0), ids exactly.  The order among equal scores is ascending id on every call (no tie replay for this metric);
the device calls return -q.v ascending, the host calls q.v descending.

Three seeded data sets (`_data`): `signed` (values in [-100, 100], scores of both signs, practically no ties), `ties`
(values in [-2, 2]: most queries have equal scores among their k + 1 best) and `zeros` (all-zero queries, queries
orthogonal to planted rows -- scores that are exactly 0 between positive and negative ones -- and every fifth row an exact
copy of an earlier row).

The knobs of the scans are read when the library is loaded: the cases that need one run this file as a child process
(`python tests/test_gpu_ip.py MODE ...`), which checks against the same reference."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SETS = ("signed", "ties", "zeros")
OFFSET = 3_000_000
K1_REF = 16  # the reference lists hold the 16 best: the k + 1 best of every k <= 15 are their prefixes
N_SEEDED = 65537  # >= 2 * 2048 sample tiles of 16 rows: launches of >= 4 batches are seeded
STREAM_CASES = ((4, 32), (7, 32), (5, 20), (9, 1), (32, 32))  # (batches, queries per batch)
ZERO_QUERIES = (0, 5, 37)                 # of the `zeros` set: all-zero queries
ORTH_QUERIES = (1, 2, 3, 4, 6, 7, 8, 9)   # ... queries orthogonal to planted rows
LIGHT_Q0 = 64                             # ... from here on: the orthogonal queries again, no all-zero query


# ------------------------------------------------------------------ the reference
def _assert_exact(q, base):
    """Integer values small enough that every partial sum of a dot product is an integer below 2^24."""
    assert np.array_equal(q, np.rint(q)) and np.array_equal(base, np.rint(base))
    assert base.shape[1] * float(np.abs(q).max()) * float(np.abs(base).max()) < 2 ** 24


def _topk_by_score(q, base, k1, id_offset=0):
    """The k1 best rows per query by (-q.v ascending, id ascending) from the float64 product: ids + id_offset (int32) and
    -q.v (float32), (-1, +inf) in the slots past n_rows."""
    n, nq = len(base), len(q)
    m = min(k1, n)
    ids = np.full((nq, k1), -1, dtype=np.int32)
    d = np.full((nq, k1), np.inf, dtype=np.float32)
    b64 = base.astype(np.float64)
    for c0 in range(0, nq, 128):
        neg = 0.0 - q[c0:c0 + 128].astype(np.float64) @ b64.T
        kth = np.partition(neg, m - 1, axis=1)[:, m - 1]
        for r in range(len(neg)):
            cand = np.nonzero(neg[r] <= kth[r])[0]  # every row at the m-th score: (score, id) then picks the right ones
            o = cand[np.lexsort((cand, neg[r, cand]))[:m]]
            ids[c0 + r, :m] = o + id_offset
            d[c0 + r, :m] = neg[r, o]
    return ids, d


def _ip_reference(q, base, k1, id_offset=0):
    _assert_exact(q, base)
    return _topk_by_score(q, base, k1, id_offset)


def _tie_flags(d):
    """1 exactly where two finite neighbours of a list are equal."""
    return (np.isfinite(d[:, 1:]) & (d[:, 1:] == d[:, :-1])).any(1).astype(np.int32)


def test_reference_helper_matches_lexsort():
    rng = np.random.default_rng(1)
    base = rng.integers(-1, 2, size=(40, 128)).astype(np.float32)
    base[30:35] = base[3]
    q = rng.integers(-1, 2, size=(9, 128)).astype(np.float32)
    q[0] = 0.0
    q[1] = base[3]
    s = q.astype(np.float64) @ base.astype(np.float64).T
    for k1, off in ((6, 0), (16, 0), (6, OFFSET), (40, 7), (44, 0)):
        ids, d = _ip_reference(q, base, k1, off)
        m = min(k1, 40)
        for r in range(len(q)):
            o = np.lexsort((np.arange(40), -s[r]))[:m]
            assert np.array_equal(ids[r, :m], o + off)
            assert np.array_equal(d[r, :m], (-s[r, o]).astype(np.float32))
        assert (ids[:, m:] == -1).all() and np.isposinf(d[:, m:]).all()
        fl = _tie_flags(d)
        for r in range(len(q)):
            assert fl[r] == int(any(d[r, t] == d[r, t + 1] and np.isfinite(d[r, t + 1]) for t in range(k1 - 1)))
    assert _tie_flags(_ip_reference(q, base, 6)[1])[:2].tolist() == [1, 1]  # all scores 0; five copies of the best row
    assert _tie_flags(np.array([[1, 2, np.inf, np.inf]], dtype=np.float32)).tolist() == [0]  # padding is no tie
    with pytest.raises(AssertionError):
        _assert_exact(q + 0.5, base)
    with pytest.raises(AssertionError):
        _assert_exact(q * 400, base * 400)


# ------------------------------------------------------------------ data
@functools.lru_cache(maxsize=None)
def _data(name, n, nq, dim=128):
    """(base [n, dim], queries [nq, dim]) of a named set, read-only."""
    rng = np.random.default_rng({"signed": 101, "ties": 202, "zeros": 303}[name] + 7 * n + dim)
    if name == "signed":
        base = rng.integers(-100, 101, size=(n, dim)).astype(np.float32)
        q = rng.integers(-100, 101, size=(nq, dim)).astype(np.float32)
    elif name == "ties":
        base = rng.integers(-2, 3, size=(n, dim)).astype(np.float32)
        q = rng.integers(-2, 3, size=(nq, dim)).astype(np.float32)
    else:
        # Coordinates 0..15 are negative in every ordinary row.  "Orthogonal" query t (of 8) is positive on its own pair of
        # them, (2 t, 2 t + 1), and 0 everywhere else: ordinary rows score < 0, the two rows that are + 1 on all 16 score
        # > 0, and three planted rows score exactly 0 by cancellation (q_a * c q_b - q_b * c q_a).  Its 6 best are
        # therefore two positive scores (equal), three zeros and a negative one.
        assert n >= 1000 and nq >= 10 and dim >= 16
        base = rng.integers(-3, 4, size=(n, dim)).astype(np.float32)
        base[:, :16] = rng.integers(-40, 0, size=(n, 16))
        q = rng.integers(-3, 4, size=(nq, dim)).astype(np.float32)
        # every fifth row a copy of an earlier row (one that is no copy itself), about half its index away
        dst = np.arange(5, n, 5)
        src = dst - 1 - 5 * (dst // 10)
        base[dst] = base[src]
        q[10::4] = base[dst[rng.integers(0, len(dst), size=len(q[10::4]))]]  # best score shared by a row and its copy
        spots = [int(x) for x in np.linspace(1, n - 2, 26).astype(np.int64)]
        for t, i in enumerate(ORTH_QUERIES):
            a, b = 2 * t, 2 * t + 1
            q[i] = 0.0
            q[i, a], q[i, b] = rng.integers(1, 10, size=2)
            for rep in range(3):
                row = spots[3 * t + rep]
                base[row, :16] = -1.0
                base[row, a], base[row, b] = q[i, b] * (rep + 1), -q[i, a] * (rep + 1)
        for row in spots[24:]:
            base[row, :16] = 1.0
        for i in ZERO_QUERIES:  # all-zero queries: every score is 0
            if i < nq:
                q[i] = 0.0
        # the same orthogonal queries once more behind the all-zero ones: a launch of queries 64.. has exact zeros among its
        # best scores without the candidate overflow that an all-zero query forces
        if nq >= LIGHT_Q0 + 8:
            q[LIGHT_Q0:LIGHT_Q0 + 8] = q[list(ORTH_QUERIES)]
    base.setflags(write=False)
    q.setflags(write=False)
    return base, q


@functools.lru_cache(maxsize=None)
def _ref(name, n, nq, dim=128, k1=K1_REF):
    base, q = _data(name, n, nq, dim)
    ids, d = _ip_reference(q, base, k1)
    ids.setflags(write=False)
    d.setflags(write=False)
    return ids, d


def _expect(ref, n_q, k, id_offset=0):
    """(ids, -scores, flags) of the first n_q queries for k: the k + 1 best."""
    ids, d = ref[0][:n_q, :k + 1], ref[1][:n_q, :k + 1]
    return np.where(ids >= 0, ids + id_offset, ids), d, _tie_flags(d)


# ------------------------------------------------------------------ calls
def _dev_call(idx, q, nb, B, k, call):
    """call: "dev" (vs_bf_search_dev, nb == 1), "multi" (vs_bf_search_dev_multi), "topk" (vs_bf_search_topk_dev_multi)."""
    import torch
    dev = torch.device("cuda:0")
    qd = torch.from_numpy(np.array(q[:nb * B], dtype=np.float32)).to(dev)  # (a copy: the cached sets are read-only)
    oi = torch.full((nb * B, k + 1), -7, dtype=torch.int32, device=dev)
    od = torch.zeros((nb * B, k + 1), dtype=torch.float32, device=dev)
    fl = torch.full((nb * B,), -7, dtype=torch.int32, device=dev)
    s = torch.cuda.current_stream().cuda_stream
    if call == "dev":
        assert nb == 1
        idx.search_dev(qd.data_ptr(), B, k, oi.data_ptr(), od.data_ptr(), fl.data_ptr(), s)
    elif call == "multi":
        idx.search_dev_multi(qd.data_ptr(), nb, B, k, oi.data_ptr(), od.data_ptr(), fl.data_ptr(), s)
    else:
        idx.search_topk_dev_multi(qd.data_ptr(), nb, B, k, oi.data_ptr(), od.data_ptr(), fl.data_ptr(), s)
    torch.cuda.synchronize()
    return oi.cpu().numpy(), od.cpu().numpy(), fl.cpu().numpy()


def _assert_lists(got, want, what):
    """ids exactly, scores by value (-0.0 == +0.0), flags exactly."""
    gi, gd, gf = got
    wi, wd, wf = want
    bad = np.nonzero((gi != wi).any(1) | (gd != wd).any(1))[0]
    assert bad.size == 0, f"{what}: {bad.size} queries differ, first {bad[0]}: ids {gi[bad[0]]} / {wi[bad[0]]}, d {gd[bad[0]]} / {wd[bad[0]]}"
    if gf is not None:
        assert np.array_equal(gf, wf), f"{what}: flags differ at queries {np.nonzero(gf != wf)[0][:8]}"


def _check_dev(idx, q, ref, nb, B, k, call, id_offset, what):
    _assert_lists(_dev_call(idx, q, nb, B, k, call), _expect(ref, nb * B, k, id_offset), f"{what} {call} nb={nb} B={B} k={k}")


def _check_host(pkg, idx, q, ref, k, id_offset, what, search="search"):
    """The host calls: q.v descending, equal scores by ascending id, no tie replay."""
    tm = pkg.Timing()
    ids, s = getattr(idx, search)(q, k, tm)
    wi, wd, _ = _expect(ref, len(q), k, id_offset)
    _assert_lists((ids, s, None), (wi[:, :k], np.where(np.isfinite(wd[:, :k]), -wd[:, :k], np.inf), None), f"{what} {search} k={k}")
    assert tm.tie_queries == 0


def _offset_of(name):
    return OFFSET if name == "ties" else 0


def _index(pkg, base, id_offset=0):
    return pkg.BruteForceIndex(base, metric=pkg.METRIC_IP, id_offset=id_offset)


# ------------------------------------------------------------------ properties of the data the tests lean on
def test_data_sets_have_the_edges_they_claim():
    fl = {name: _tie_flags(_ref(name, N_SEEDED, 160)[1][:, :6]) for name in SETS}
    assert fl["signed"].sum() == 0
    assert fl["ties"].mean() > 0.5
    ids, d = _ref("zeros", N_SEEDED, 160)
    assert (d[list(ZERO_QUERIES)] == 0).all() and np.array_equal(ids[0], np.arange(16))
    for i in ORTH_QUERIES + tuple(range(LIGHT_Q0, LIGHT_Q0 + 8)):  # two positive scores, three exact zeros, a negative one
        assert d[i, 0] == d[i, 1] < 0 and (d[i, 2:5] == 0).all() and d[i, 5] > 0, (i, d[i, :6])
    assert fl["zeros"][10::4].sum() >= 10  # a row and its copy score alike (a longer row can still beat both)
    s = _data("signed", 3000, 16)[1].astype(np.float64) @ _data("signed", 3000, 16)[0].astype(np.float64).T
    assert (s > 0).any() and (s < 0).any()


# ------------------------------------------------------------------ the paths of bf_launch
@pytest.mark.gpu
@pytest.mark.parametrize("name", SETS)
def test_single_call_scan(gpu_pkg, name):
    """3 000 fp32 rows, fewer than 4 batches of at most 16 queries: one scan_one_kernel launch per batch.  The kernel walks
    its tiles forwards and backwards on alternate calls: every call is made twice."""
    n, off = 3000, _offset_of(name)
    base, q = _data(name, n, 48)
    ref = _ref(name, n, 48)
    with _index(gpu_pkg, base, off) as idx:
        for B in (1, 5, 16):
            for nb in (1, 2, 3):
                for k in ((5, 15) if B == 5 else (5,)):
                    for _ in range(2):
                        _check_dev(idx, q, ref, nb, B, k, "multi", off, name)
                        if nb == 1:
                            _check_dev(idx, q, ref, 1, B, k, "dev", off, name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", SETS)
def test_per_batch_scan_without_exchange(gpu_pkg, name):
    """20 000 rows, batches of more than 16 queries: scan_kernel, too few tiles per workgroup for the threshold exchange."""
    n, off = 20000, _offset_of(name)
    base, q = _data(name, n, 96)
    ref = _ref(name, n, 96)
    with _index(gpu_pkg, base, off) as idx:
        for nb, B in ((1, 17), (1, 32), (3, 17), (3, 32)):
            for k in (1, 5, 10):
                _check_dev(idx, q, ref, nb, B, k, "multi", off, name)
                if nb == 1:
                    _check_dev(idx, q, ref, 1, B, k, "dev", off, name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", SETS)
def test_per_batch_scan_with_threshold_exchange(gpu_pkg, name):
    """One batch of 32 queries on 98 304 + 5 rows: 6 145 tiles / 48 >= half of 256 CUs, so scan_geometry gives every
    workgroup 49 tiles and the workgroups trade their bounds while they scan."""
    n, off = 98304 + 5, _offset_of(name)
    base, q = _data(name, n, 32)
    ref = _ref(name, n, 32)
    with _index(gpu_pkg, base, off) as idx:
        for k in (5, 15):
            _check_dev(idx, q, ref, 1, 32, k, "dev", off, name)
        _check_dev(idx, q, ref, 1, 20, 5, "dev", off, name)


def _check_stream_cases(pkg, name):
    """Launches of >= 4 batches on 65 537 rows: bounds from the seed launch, then the streaming scan the loaded knobs
    select (the bf16 prefilter with the exact recheck, or the fp32 scan), then the flat merge."""
    off = _offset_of(name)
    base, q = _data(name, N_SEEDED, 1061)
    ref = _ref(name, N_SEEDED, 1061)
    with _index(pkg, base, off) as idx:
        for nb, B in STREAM_CASES:
            for k in ((5, 10) if nb == 7 else (5,)):
                _check_dev(idx, q, ref, nb, B, k, "multi", off, name)
        # (`zeros`: query 0 scores 0 on every row, so each launch above overflows its candidate lists and is answered by
        # the fallback scan; the launches below start behind the all-zero queries and stay on the streaming scan)
        o = LIGHT_Q0
        for nb, B in ((4, 32), (9, 1), (5, 20)):
            _check_dev(idx, q[o:], (ref[0][o:], ref[1][o:]), nb, B, 5, "multi", off, f"{name} from query {o}")


@pytest.mark.gpu
@pytest.mark.parametrize("name", SETS)
def test_seeded_prefilter_scan(gpu_pkg, name):
    _check_stream_cases(gpu_pkg, name)


def _run_child(mode, args, env):
    e = dict(os.environ)
    e.update(env)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), mode, *args], env=e, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0 and "IP_CHILD_OK" in r.stdout, (mode, args, env, r.stdout[-600:], r.stderr[-1500:])


@pytest.mark.gpu
@pytest.mark.parametrize("pair", ["2", "0"])
@pytest.mark.parametrize("name", SETS)
def test_seeded_fp32_streaming_scan(gpu_pkg, name, pair):
    """The same launches with the prefilter off: scan_f32s_kernel, two batches per pass over the rows and one."""
    _run_child("stream", [name], {"VSEARCH_F32_FILTER": "0", "VSEARCH_F32_PAIR": pair})


def _overflow_data(name):
    base, q = (a.copy() for a in _data(name, N_SEEDED, 160))
    r = int(np.argmax((base.astype(np.float64) ** 2).sum(1)))  # the longest row: no row scores higher with it than itself
    base[20000:50000] = base[r]  # 30 000 copies of it
    q[0] = base[r]               # 30 001 equal candidates at the best score
    q[33] = 0.0                  # every row scores 0: 65 537 equal candidates
    return base, q


@pytest.mark.gpu
@pytest.mark.parametrize("name", SETS)
def test_candidate_overflow_falls_back_to_the_per_batch_scan(gpu_pkg, name):
    """More rows over a query's bound than its candidate lists hold: the streaming scan raises the overflow word and the
    per-batch scan enqueued behind it writes the result."""
    off = _offset_of(name)
    base, q = _overflow_data(name)
    ref = _ip_reference(q, base, K1_REF)
    # both queries have far more rows at or above their 6th best score than the 16 x 128 candidate slots of a query
    s2 = q[[0, 33]].astype(np.float64) @ base.astype(np.float64).T
    assert ((-s2 <= ref[1][[0, 33], 5:6]).sum(1) >= 30000).all() and ref[0][33, :6].tolist() == list(range(6))
    with _index(gpu_pkg, base, off) as idx:
        _check_dev(idx, q, ref, 5, 32, 5, "multi", off, name)
        _check_host(gpu_pkg, idx, q, ref, 5, off, name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", SETS)
def test_score_matrix(gpu_pkg, name):
    """vs_bf_scores_dev (store mode of scan_kernel): the [B, ld] matrix holds -q.v exactly, padding columns untouched."""
    import torch
    n, ld = 12345, 12352
    base, q = _data(name, n, 32)
    _assert_exact(q, base)
    want = (0.0 - q.astype(np.float64) @ base.astype(np.float64).T).astype(np.float32)
    dev = torch.device("cuda:0")
    with _index(gpu_pkg, base, _offset_of(name)) as idx:
        for B in (20, 32):
            sc = torch.full((B, ld), -7.5, dtype=torch.float32, device=dev)
            qd = torch.from_numpy(np.array(q[:B], dtype=np.float32)).to(dev)
            idx.scores_dev(qd.data_ptr(), B, sc.data_ptr(), ld, torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
            got = sc.cpu().numpy()
            assert np.array_equal(got[:, :n], want[:B]), (name, B)
            assert np.all(got[:, n:] == -7.5)


@pytest.mark.gpu
@pytest.mark.parametrize("k", [16, 100, 128])
@pytest.mark.parametrize("name", ["signed", "ties"])
def test_wide_k(gpu_pkg, name, k):
    """k + 1 > 16 on 70 000 rows: prefix selection, filtered pass, selection over the candidates."""
    n, off = 70000, _offset_of(name)
    base, q = _data(name, n, 64)
    ref = _ref(name, n, 64, 128, 129)
    with _index(gpu_pkg, base, off) as idx:
        _check_dev(idx, q, ref, 2, 32, k, "topk", off, name)
        _check_host(gpu_pkg, idx, q, ref, k, off, name, search="search_topk")


@pytest.mark.gpu
@pytest.mark.parametrize("dim", [100, 960])
@pytest.mark.parametrize("name", SETS)
def test_general_dimension(gpu_pkg, name, dim):
    """scan_nd_kernel: 20 000 rows of 100 and 960 values, 3 batches of 32 (960 * 100 * 100 < 2^24: still exact)."""
    n, off = 20000, _offset_of(name)
    base, q = _data(name, n, 96, dim)
    ref = _ref(name, n, 96, dim)
    with _index(gpu_pkg, base, off) as idx:
        assert idx.getDim() == dim
        _check_dev(idx, q, ref, 3, 32, 5, "multi", off, name)
        _check_dev(idx, q, ref, 1, 17, 15, "dev", off, name)
        _check_host(gpu_pkg, idx, q, ref, 5, off, name)


# ------------------------------------------------------------------ host calls
@pytest.mark.gpu
@pytest.mark.parametrize("name", SETS)
def test_host_call(gpu_pkg, name):
    """vs_bf_search on 65 537 rows with 1 024 + 37 queries: two chunks, a ragged tail batch.  Scores q.v descending, equal
    scores by ascending id, nothing replayed; precisions 0 and 1 are the same fp32 rows, and an IP index has no byte copy."""
    off = _offset_of(name)
    base, q = _data(name, N_SEEDED, 1061)
    ref = _ref(name, N_SEEDED, 1061)
    with _index(gpu_pkg, base, off) as idx:
        for precision in (0, 1):
            idx.set_precision(precision)
            for k in (1, 5, 15):
                _check_host(gpu_pkg, idx, q, ref, k, off, f"{name} precision={precision}")
        with pytest.raises(gpu_pkg.VSearchError) as e:
            idx.set_precision(2)
        assert e.value.status == -5  # VS_ERR_UNSUPPORTED


@pytest.mark.gpu
def test_base_smaller_than_k(gpu_pkg):
    base, q = _data("ties", 3, 7)
    ref = _ip_reference(q, base, 6)
    assert (ref[0][:, 3:] == -1).all() and np.isposinf(ref[1][:, 3:]).all()
    with _index(gpu_pkg, base, OFFSET) as idx:
        _check_host(gpu_pkg, idx, q, ref, 5, OFFSET, "3 rows")
        _check_dev(idx, q, ref, 1, 7, 5, "dev", OFFSET, "3 rows")


@pytest.mark.gpu
@pytest.mark.parametrize("world", [2, 8])
def test_virtual_shards(gpu_pkg, world):
    """vs_bf_search_vshards over 65 537 rows of the `ties` set: the unsharded answer, equal scores across shard
    boundaries in ascending global id."""
    base, q = _data("ties", N_SEEDED, 1061)
    ref = _ref("ties", N_SEEDED, 1061)
    q = q[:165]
    bounds = gpu_pkg.row_shard_bounds(len(base), world)
    shards = [gpu_pkg.BruteForceIndex(base[bounds[g]:bounds[g + 1]], metric=gpu_pkg.METRIC_IP, id_offset=int(bounds[g])) for g in range(world)]
    try:
        for k in (5, 10):
            tm = gpu_pkg.Timing()
            ids, s = gpu_pkg.BruteForceIndex.search_vshards(shards, q, k, tm)
            wi, wd, wf = _expect(ref, len(q), k)
            _assert_lists((ids, s, None), (wi[:, :k], -wd[:, :k], None), f"world={world} k={k}")
            assert tm.tie_queries == 0
            # the test is about ties across shard boundaries: some query's k best hold equal scores from two shards
            sh = np.searchsorted(bounds, wi[:, :k], side="right")
            assert any(wd[r, t] == wd[r, t + 1] and sh[r, t] != sh[r, t + 1] for r in range(len(q)) for t in range(k - 1))
    finally:
        for s_ in shards:
            s_.close()


# ------------------------------------------------------------------ knobs (one process per setting)
def _knob_data():
    """`signed` with ties: 400 rows copied far away, every eighth query equal to a copied row."""
    base, q = (a.copy() for a in _data("signed", N_SEEDED, 160))
    dst = 40000 + 50 * np.arange(400)
    base[dst] = base[np.arange(400) * 3]
    q[::8] = base[dst[:20]]
    return base, q


def _check_knobs(pkg, nb):
    base, q = _knob_data()
    ref = _ip_reference(q, base, K1_REF)
    assert _tie_flags(ref[1][:, :6])[::8].all()
    with _index(pkg, base) as idx:
        for k in (5, 10):
            _check_dev(idx, q, ref, nb, 32, k, "multi", 0, "knobs")
            _check_host(pkg, idx, q, ref, k, 0, "knobs")


@pytest.mark.gpu
@pytest.mark.parametrize("env,nb", [({}, 5), ({"VSEARCH_F32_FILTER": "0"}, 5), ({"VSEARCH_F32_FILTER": "0", "VSEARCH_F32_PAIR": "2"}, 5),
                                    ({"VSEARCH_F32_FILTER": "0", "VSEARCH_F32_PAIR": "0"}, 5), ({"VSEARCH_STREAM": "0"}, 5),
                                    ({"VSEARCH_SEED_MIN": "1"}, 2), ({"VSEARCH_XCHG_IT": "-1"}, 5), ({"VSEARCH_GRID_CUS": "64"}, 5),
                                    ({"VSEARCH_LANES": "2"}, 5)])
def test_tuning_knobs_keep_ip_results(gpu_pkg, env, nb):
    """Every VSEARCH_* knob that selects a brute-force scan, on an IP index: vs_bf_search_dev_multi and vs_bf_search
    against the reference inside the child process."""
    _run_child("knobs", [str(nb)], env)


# ------------------------------------------------------------------ non-integer data
def _check_gaussian(pkg):
    """N(0, 1) rows and queries, 65 537 rows, 5 x 32 queries, against the float64 product.

    Tolerance: a length-n fp32 dot product summed in any order has error at most gamma_n * sum|q_i b_i| with gamma_n =
    n u / (1 - n u) (Higham, Accuracy and Stability of Numerical Algorithms, section 3.1); sum|q_i b_i| <= ||q|| ||b||
    (Cauchy-Schwarz).  With n = 128, u = 2^-24 and n u << 1: tol = 128 * 2^-24 * max||q|| * max||b||.  Ids are compared
    at every (query, rank) whose reference score is more than 2 tol away from both neighbours in the ranking: two rows
    each off by at most tol cannot swap there."""
    rng = np.random.default_rng(31)
    base = rng.normal(0, 1, size=(N_SEEDED, 128)).astype(np.float32)
    q = rng.normal(0, 1, size=(160, 128)).astype(np.float32)
    nq_, nb_ = np.sqrt((q.astype(np.float64) ** 2).sum(1)).max(), np.sqrt((base.astype(np.float64) ** 2).sum(1)).max()
    tol = 128 * 2.0 ** -24 * nq_ * nb_
    k = 5
    ri, rd = _topk_by_score(q, base, k + 2)  # float32-rounded scores would blur the gaps: recompute them in float64
    rd64 = -np.take_along_axis(q.astype(np.float64) @ base.astype(np.float64).T, ri.astype(np.int64), 1)
    gap = np.diff(rd64, axis=1)  # [160, k + 1], ascending lists: >= 0
    lo = np.concatenate([np.full((160, 1), np.inf), gap[:, :-1]], axis=1)
    ok = (np.minimum(lo, gap) > 2 * tol)  # ranks 0 .. k
    with _index(pkg, base) as idx:
        gi, gd, _ = _dev_call(idx, q, 5, 32, k, "multi")
        hi_, hs = idx.search(q, k)
    print(f"gaussian: tol {tol:.3e}, comparable {ok.mean():.4f} (device ranks), {ok[:, :k].mean():.4f} (host ranks), "
          f"max |err| device {np.abs(gd - rd64[:, :k + 1]).max():.3e}, host {np.abs(hs + rd64[:, :k]).max():.3e}")
    assert ok.mean() >= 0.9 and ok[:, :k].mean() >= 0.9
    assert np.abs(gd - rd64[:, :k + 1]).max() <= tol
    assert np.abs(hs + rd64[:, :k]).max() <= tol
    assert np.array_equal(gi[ok], ri[:, :k + 1][ok])
    assert np.array_equal(hi_[ok[:, :k]], ri[:, :k][ok[:, :k]])
    assert (np.diff(gd, axis=1) >= 0).all() and (np.diff(hs, axis=1) <= 0).all()


@pytest.mark.gpu
def test_non_integer_data_prefilter(gpu_pkg):
    _check_gaussian(gpu_pkg)


@pytest.mark.gpu
def test_non_integer_data_fp32_streaming_scan(gpu_pkg):
    _run_child("gaussian", [], {"VSEARCH_F32_FILTER": "0"})


# ------------------------------------------------------------------ the child process
def _child_main(argv):
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    import __graft_entry__ as ge
    pkg = ge.load_package()
    assert pkg.device_count() >= 1
    mode = argv[0]
    if mode == "stream":
        _check_stream_cases(pkg, argv[1])
    elif mode == "knobs":
        _check_knobs(pkg, int(argv[1]))
    elif mode == "gaussian":
        _check_gaussian(pkg)
    else:
        raise SystemExit(f"unknown mode {mode}")
    print("IP_CHILD_OK")


if __name__ == "__main__":
    _child_main(sys.argv[1:])
