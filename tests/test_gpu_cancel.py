"""Squared-L2 search where distances cancel: queries that ARE rows of a real-valued base with duplicate rows
(tests/cancel_data.py).  The smallest distances are then rounding noise of either sign -- negative distances, exact +0
between them, bounds tau <= 0, ties on distances that are no integers -- which nothing else in the suite produces.

Expected values are the chain oracle's bits (dot_order="chain" restates the fp32 MFMA kernels): np.array_equal on the
int32 view of the distances and exact ids for EVERY query, no tolerance, no gap filter.  Every test asserts first that
its expected arrays hold a negative distance, a +0 and a tie (cancel_data.require); test_oracle.py asserts the fuller
counts for every data set on the CPU."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.dirname(os.path.abspath(__file__))):  # (also run as a script: the prefilter's A/B worker below)
    if _p not in sys.path:
        sys.path.insert(0, _p)
import cancel_data  # noqa: E402
import oracle  # noqa: E402
from cancel_data import bits  # noqa: E402

pytestmark = pytest.mark.gpu

_REF = {}


def _sorted_ref(key):
    """the 130 best of every query of data set `key` by (distance, row id), from the chain score matrix: made once"""
    if key not in _REF:
        base, q, _ = cancel_data.case(*key)
        _REF[key] = cancel_data.sorted_scores(q, base, 130)
    return _REF[key]


def _assert_same(got, want, tag):
    """ids and distance bits of every query (and total_candidates where both sides carry it)"""
    gi, gd, wi, wd = got[0], got[1], want[0], want[1]
    assert gi.shape == wi.shape and gd.shape == wd.shape, (tag, gi.shape, wi.shape)
    bad = [i for i in range(len(wi)) if not (np.array_equal(bits(gd[i]), bits(wd[i])) and np.array_equal(gi[i], wi[i]))]
    if bad:
        i = bad[0]
        c = np.nonzero((bits(gd[i]) != bits(wd[i])) | (gi[i] != wi[i]))[0][:4]
        print(f"{tag}: {len(bad)} of {len(wi)} queries differ, first {bad[:10]}; query {i} columns {c.tolist()}: device ids "
              f"{gi[i][c].tolist()} dists {[float(x) for x in gd[i][c]]} ({[hex(x & 0xffffffff) for x in bits(gd[i])[c]]}), expected ids "
              f"{wi[i][c].tolist()} dists {[float(x) for x in wd[i][c]]} ({[hex(x & 0xffffffff) for x in bits(wd[i])[c]]})")
    assert not bad, (tag, "queries differ from the chain oracle", bad[:10])
    if len(got) > 2 and len(want) > 2:
        assert got[2] == want[2], (tag, "total_candidates", got[2], want[2])


def _flags(d):
    """1 exactly where two of the k + 1 (ascending) distances compare equal"""
    return (np.isfinite(d[:, :-1]) & (d[:, :-1] == d[:, 1:])).any(1).astype(np.int32)


def _bf_dev(idx, q, nb, B, k, call="multi"):
    """search_dev (one batch), search_dev_multi or search_topk_dev_multi on the first nb * B queries: ids, dists, flags"""
    import torch
    dev = torch.device("cuda:0")
    n = nb * B
    qd = torch.from_numpy(np.array(q[:n])).to(dev)  # (a copy: the data sets are read-only)
    oi = torch.full((n, k + 1), -7, dtype=torch.int32, device=dev)
    od = torch.full((n, k + 1), 7.0, dtype=torch.float32, device=dev)
    fl = torch.full((n,), -7, dtype=torch.int32, device=dev)
    s = torch.cuda.current_stream().cuda_stream
    if call == "one":
        assert nb == 1
        idx.search_dev(qd.data_ptr(), B, k, oi.data_ptr(), od.data_ptr(), fl.data_ptr(), s)
    elif call == "multi":
        idx.search_dev_multi(qd.data_ptr(), nb, B, k, oi.data_ptr(), od.data_ptr(), fl.data_ptr(), s)
    else:
        idx.search_topk_dev_multi(qd.data_ptr(), nb, B, k, oi.data_ptr(), od.data_ptr(), fl.data_ptr(), s)
    torch.cuda.synchronize()
    return oi.cpu().numpy(), od.cpu().numpy(), fl.cpu().numpy()


def _check_dev(idx, key, nb, B, k, call, tag):
    """a device call against the k + 1 best by (distance, id) and the flags that follow from them"""
    q = cancel_data.case(*key)[1]
    ri, rd = _sorted_ref(key)
    n = nb * B
    wi, wd = ri[:n, :k + 1], rd[:n, :k + 1]
    cancel_data.require(wd, k, f"{tag} {call} nb {nb} B {B} k {k}")
    gi, gd, fl = _bf_dev(idx, q, nb, B, k, call)
    _assert_same((gi, gd), (wi, wd), (tag, call, nb, B, k))
    assert np.array_equal(fl, _flags(wd)), (tag, call, nb, B, k, "flags", np.nonzero(fl != _flags(wd))[0][:10])
    return gi, gd, fl


def _check_host(idx, key, k, tag, nq=None, topk=False):
    """search / search_topk against oracle.search_bf in the chain order: select_topk's slot order among equal distances"""
    base, q, _ = cancel_data.case(*key)
    q = q[:nq]
    wi, wd = oracle.search_bf(base, q, k, dot_order="chain")
    cancel_data.require(_sorted_ref(key)[1][:len(q)], k, f"{tag} host k {k}")
    import __graft_entry__ as ge
    tm = ge.load_package().Timing()
    got = idx.search_topk(q, k, tm) if topk else idx.search(q, k, tm)
    _assert_same(got, (wi, wd), (tag, "host", k))
    return tm


# ------------------------------------------------------------------------------------------ brute force, 128-d index
@pytest.fixture(scope="module", params=[0, 4], ids=["offset0", "offset4"])
def bf128(gpu_pkg, request):
    key = (20000, 640, 128, request.param)
    with gpu_pkg.BruteForceIndex(cancel_data.case(*key)[0]) as idx:
        idx.set_precision(1)
        yield idx, key


@pytest.mark.parametrize("k", [1, 5, 15])
def test_bf128_host_search_replays_ties_on_real_valued_distances(bf128, k):
    idx, key = bf128
    tm = _check_host(idx, key, k, "bf128")
    assert tm.tie_queries > 0  # bit-equal rows give bit-equal distances: the replay ran, on distances that are no integers


@pytest.mark.parametrize("k", [1, 5, 15])
def test_bf128_device_calls(bf128, k):
    idx, key = bf128
    _check_dev(idx, key, 1, 32, k, "one", "bf128")
    for nb in (4, 20):
        _check_dev(idx, key, nb, 32, k, "multi", "bf128")


@pytest.mark.parametrize("offset", [0, 4])
def test_bf128_scan_one_kernel(gpu_pkg, offset):
    """3 000 rows, 3 batches of 16 queries: fewer than 4 batches of at most 16 take one scan_one_kernel launch each"""
    key = (3000, 48, 128, offset)
    with gpu_pkg.BruteForceIndex(cancel_data.case(*key)[0]) as idx:
        idx.set_precision(1)
        for k in (1, 5, 15):
            _check_dev(idx, key, 3, 16, k, "multi", "scan_one")
            _check_dev(idx, key, 1, 16, k, "one", "scan_one")


PREFILTER_KEY = (66000, 128, 128, 4)


def _worker(out):
    """python test_gpu_cancel.py <out.npz>: the prefilter case's searches in a process of its own (the A/B switch is read
    when the library is loaded)"""
    import __graft_entry__ as ge
    pkg = ge.load_package()
    res = {}
    with pkg.BruteForceIndex(cancel_data.case(*PREFILTER_KEY)[0]) as idx:
        idx.set_precision(1)
        for k in (1, 5, 15):
            res[f"i{k}"], res[f"d{k}"], res[f"f{k}"] = _bf_dev(idx, cancel_data.case(*PREFILTER_KEY)[1], 4, 32, k)
    np.savez(out, **res)


def test_bf128_prefilter_and_fp32_scan_agree_with_the_oracle(gpu_pkg, tmp_path):
    """66 000 rows (the smallest shard that builds the bf16 image), 4 batches of 32, rows with a common offset of 4: bf16
    rounding makes the prefilter's error bound E large against distances near 0 and many rows survive it.  With the
    prefilter and, in a child process, with VSEARCH_F32_FILTER=0: both equal the oracle, so each other."""
    assert os.environ.get("VSEARCH_F32_FILTER", "1") != "0"
    with gpu_pkg.BruteForceIndex(cancel_data.case(*PREFILTER_KEY)[0]) as idx:
        idx.set_precision(1)
        assert idx.filter_image(0, 64).shape == (64, 128)  # the image exists: the seeded streaming launches prefilter on it
        here = {k: _check_dev(idx, PREFILTER_KEY, 4, 32, k, "multi", "prefilter") for k in (1, 5, 15)}
    out = str(tmp_path / "fp32.npz")
    subprocess.run([sys.executable, os.path.abspath(__file__), out], env=dict(os.environ, VSEARCH_F32_FILTER="0"), check=True, timeout=300)
    other = dict(np.load(out))
    ri, rd = _sorted_ref(PREFILTER_KEY)
    for k in (1, 5, 15):
        _assert_same((other[f"i{k}"], other[f"d{k}"]), (ri[:, :k + 1], rd[:, :k + 1]), ("fp32 scan", k))
        assert np.array_equal(other[f"f{k}"], _flags(rd[:, :k + 1]))
        assert all(np.array_equal(bits(a) if a.dtype == np.float32 else a, bits(b) if b.dtype == np.float32 else b)
                   for a, b in zip(here[k], (other[f"i{k}"], other[f"d{k}"], other[f"f{k}"])))


@pytest.mark.parametrize("offset", [0, 4])
def test_bf128_wide_k(gpu_pkg, offset):
    key = (30000, 128, 128, offset)
    with gpu_pkg.BruteForceIndex(cancel_data.case(*key)[0]) as idx:
        idx.set_precision(1)
        for k in (16, 50, 128):
            _check_host(idx, key, k, "wide", topk=True)
            _check_dev(idx, key, 4, 32, k, "topk", "wide")


@pytest.mark.parametrize("offset", [0, 4])
def test_bf128_three_row_shards_equal_the_unsharded_oracle(gpu_pkg, offset):
    """rows 0 .. 1999 (shard 0) have copies at 10 037 .. 10 086 (shard 1) and 18 000 .. 19 999 (shard 2)"""
    key = (20000, 640, 128, offset)
    base, q, _ = cancel_data.case(*key)
    b = gpu_pkg.row_shard_bounds(len(base), 3)
    m, mid = cancel_data.layout(len(base))
    assert m < b[1] < mid and mid + cancel_data.TRIPLE < b[2] < len(base) - m
    q, k = q[:128], 5
    wi, wd = oracle.search_bf(base, q, k, dot_order="chain")
    cancel_data.require(_sorted_ref(key)[1][:128], k, "vshards")
    shards = [gpu_pkg.BruteForceIndex(base[b[g]:b[g + 1]], id_offset=int(b[g])) for g in range(3)]
    try:
        for s in shards:
            s.set_precision(1)
        tm = gpu_pkg.Timing()
        got = gpu_pkg.BruteForceIndex.search_vshards(shards, q, k, tm)
    finally:
        for s in shards:
            s.close()
    _assert_same(got, (wi, wd), "vshards")
    assert tm.tie_queries > 0


# ------------------------------------------------------------------------------------------ brute force, general index
@pytest.mark.parametrize("offset", [0, 4])
@pytest.mark.parametrize("dim", [20, 100, 384])  # dim_p / 16 = 2, 7 and 24 segments: even, odd, even
def test_bf_general_index(gpu_pkg, dim, offset):
    key = (20000, 96, dim, offset)
    with gpu_pkg.BruteForceIndex(cancel_data.case(*key)[0]) as idx:
        for k in (1, 5, 15):
            tm = _check_host(idx, key, k, f"nd {dim}")
            assert tm.tie_queries > 0
            _check_dev(idx, key, 3, 32, k, "multi", f"nd {dim}")
        for k in (16, 128):
            _check_host(idx, key, k, f"nd {dim}", topk=True)
            _check_dev(idx, key, 3, 32, k, "topk", f"nd {dim}")


# ------------------------------------------------------------------------------------------ IVF
def _open(pkg, data):
    vr, off, r2o, cents, _ = data
    return pkg.IVFIndex(vectors_reordered=vr, centroids=cents, cluster_offsets=off, reorder_to_original=r2o)


def _ivf_dev(ivf, q, nb, B, k, nprobe, topk=False):
    import torch
    dev = torch.device("cuda:0")
    qd = torch.from_numpy(np.array(q[:nb * B])).to(dev)
    oi = torch.full((nb * B, k), -7, dtype=torch.int32, device=dev)
    od = torch.full((nb * B, k), 7.0, dtype=torch.float32, device=dev)
    call = ivf.search_topk_dev_multi if topk else ivf.search_dev_multi
    call(qd.data_ptr(), nb, B, k, nprobe, oi.data_ptr(), od.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return oi.cpu().numpy(), od.cpu().numpy()


def _check_ivf(ivf, data, k, nprobe, tag, wide=False, scan_order=None, nq=None):
    """host call (ids, bits, total_candidates) and device call (ids, bits) against oracle.ivf_search in the chain order;
    the expected arrays hold a negative distance, a +0 and a tie, the probes' coarse scores a negative one and a +0"""
    vr, off, r2o, cents, q = data
    q = q[:nq]
    want1 = oracle.ivf_search(vr, off, r2o, cents, q, k + 1, nprobe, dot_order="chain", scan_order=scan_order, return_coarse=True)
    cancel_data.require(want1[1], k, f"{tag} k {k} nprobe {nprobe}")
    assert (want1[4] < 0).any() and ((want1[4] == 0) & ~np.signbit(want1[4])).any()
    want = (want1[0][:, :k], want1[1][:, :k], want1[2])
    got = ivf.search_topk(q, k, nprobe) if wide else ivf.searchBatch(q, len(q), k, nprobe)
    _assert_same(got, want, (tag, "host", k, nprobe))
    nb = len(q) // 32
    _assert_same(_ivf_dev(ivf, q, nb, 32, k, nprobe, topk=wide), (want[0][:nb * 32], want[1][:nb * 32]), (tag, "device", k, nprobe))
    return want


@pytest.fixture(scope="module", params=[0, 4], ids=["offset0", "offset4"])
def ivf128(gpu_pkg, request):
    data = cancel_data.ivf_case(20000, 96, 128, request.param, 64)
    with _open(gpu_pkg, data) as ivf:
        ivf.set_precision(1)
        yield ivf, data


@pytest.mark.parametrize("nprobe", [1, 8])
@pytest.mark.parametrize("k", [1, 2, 3, 10, 16])
def test_ivf128_fp32_rows(ivf128, k, nprobe):
    """k = 1: the k-th best is the noise value itself; k = 2 and 3: the copies of a triple (the first 24 queries)"""
    ivf, data = ivf128
    want = _check_ivf(ivf, data, k, nprobe, "ivf128")
    if k in (2, 3):  # a triple's copies are equal rows in one list: its query's k best are k equal distances
        assert (want[1][:24, :k] == want[1][:24, :1]).all(1).sum() >= 8


@pytest.mark.parametrize("nprobe", [1, 8])
@pytest.mark.parametrize("k", [17, 100])
def test_ivf128_fp32_rows_wide_k(ivf128, k, nprobe):
    ivf, data = ivf128
    _check_ivf(ivf, data, k, nprobe, "ivf128 wide", wide=True)


def test_ivf128_query_major_above_4096_lists(gpu_pkg):
    """5 000 lists: coarse scores on the MFMA scan kernel, one workgroup per (query, probe) whose list scan sums in its
    own order ("fold8"); 96 self-queries and 160 queries that are centroids"""
    data = cancel_data.ivf_case(20000, 96, 128, 0, 5000)
    with _open(gpu_pkg, data) as ivf:
        ivf.set_precision(1)
        for k in (1, 5):
            _check_ivf(ivf, data, k, 24, "ivf128 nlist 5000", scan_order="fold8", nq=256)


@pytest.mark.parametrize("offset", [0, 4])
@pytest.mark.parametrize("dim", [20, 100])
def test_ivf_general_index(gpu_pkg, dim, offset):
    data = cancel_data.ivf_case(6000, 64, dim, offset, 24)
    with _open(gpu_pkg, data) as ivf:
        for k, nprobe in ((1, 1), (10, 4), (16, 8)):
            _check_ivf(ivf, data, k, nprobe, f"ivf nd {dim}")
        assert ivf.nd_widek_stats(reset=True) == (0, 0, 0)
        for k, nprobe in ((40, 8), (128, 24)):
            _check_ivf(ivf, data, k, nprobe, f"ivf nd {dim} wide", wide=True)
            stats = ivf.nd_widek_stats(reset=True)
            assert stats[0] > 0, stats  # candidates were ranked from the candidate lists


@pytest.mark.parametrize("dim", [20, 100])
def test_ivf_general_index_exact_fallback_ranks_negative_keys(gpu_pkg, dim):
    """8 500 copies of a row whose distance to itself is negative, in a 9 000-row list and a query equal to it: the
    bound is that negative number, 8 500 rows meet it, the 8 192-key candidate list overflows and the exact fallback
    ranks the query -- on negative keys.  The other queries are rows outside the run."""
    rng = np.random.default_rng(cancel_data.SEED + 7000 + dim)
    k, nlist = 100, 8
    sizes = [9000] + [200] * 7
    n = sum(sizes)
    vr = (rng.standard_normal((n, dim)) + 4).astype(np.float32)
    j = next(j for j in range(300) if oracle.l2_row(vr[j], vr[j:j + 1], dot_order="chain")[0] < 0)
    rep = vr[j].copy()
    vr[300:8800] = rep  # with row j itself: 8 501 equal rows
    off = np.zeros(nlist + 1, dtype=np.int32)
    off[1:] = np.cumsum(sizes)
    r2o = rng.permutation(n).astype(np.int32)
    cents = np.stack([vr[off[c]:off[c + 1]].astype(np.float64).mean(0) for c in range(nlist)]).astype(np.float32)
    q = np.ascontiguousarray(vr[rng.choice(np.r_[0:300, 8800:n], 32, replace=False)])
    q[2] = rep
    want = oracle.ivf_search(vr, off, r2o, cents, q, k, nlist, dot_order="chain")
    assert np.array_equal(want[0][2], r2o[np.r_[j, 300:399]]) and (want[1][2] < 0).all() and (want[1][2] == want[1][2, 0]).all()
    assert ((want[1][:, 0] == 0) & ~np.signbit(want[1][:, 0])).any() and (want[1][np.arange(32) != 2, 0] < 0).any()
    with _open(gpu_pkg, (vr, off, r2o, cents, q)) as ivf:
        got = ivf.search_topk(q, k, nlist)
        stats = ivf.nd_widek_stats()
    _assert_same(got, want, ("fallback", dim))
    assert stats[2] >= 1, stats


if __name__ == "__main__":
    _worker(sys.argv[1])
