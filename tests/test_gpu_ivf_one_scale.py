"""The two-launch route of short IVF calls (ivf_one_coarse_kernel + ivf_one_scan_kernel) at the sizes it was
written for: nlist up to 1024 (a coarse launch of several workgroups, 16 scores per lane of the selection, two lists per
thread of the unit table), nprobe up to 256, and more units than the scan launch has workgroups.

The data is tests/ivf_one_scale_data.py; tests/test_ivf_one_scale_host.py asserts its preconditions on the CPU.  The
reference is oracle.ivf_search.  On the integer index everything is exact in fp32, so every comparison is equality of ids,
distance bits, empty slots and total_candidates; the one Gaussian case compares with the oracle in the kernels' summation
order.  Every case asserts through IVFIndex.one_stats() that its calls took the route before it compares anything."""
import numpy as np
import pytest

import ivf_one_scale_data as S
import near_ties
import oracle
from test_gpu_ivf_nd import _open
from test_gpu_ivf_one import _bits, _dev, _host_form, _same

pytestmark = pytest.mark.gpu

L2, IP = 0, 1
BS = (1, 9, 16)  # at B = 9 wave 0 of the selection takes two queries and reuses its winners' table


def _cus():
    import torch
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def _host(ivf, q, k, nprobe, metric=L2):
    """one host call of len(q) <= 16 queries: (ids, dists, total_candidates), one batch down the route"""
    ivf.one_stats(reset=True)
    got = ivf.searchBatch(q, len(q), k, nprobe) if metric == L2 else ivf.search_metric(q, k, nprobe, IP)
    assert ivf.one_stats()[0] == 1, "the call did not take the two-launch route"
    return got


def _check_host(ivf, data, q, k, nprobe, tag, metric=L2, dot_order="lanes8"):
    """B = 1, 9, 16 of the same queries against one oracle run; the candidate count pins the probe set"""
    vr, cents, off, r2o = data[:4]
    want = oracle.ivf_search(vr, off, r2o, cents, q, k, nprobe, return_probes=True, metric=metric, dot_order=dot_order)
    rows = np.diff(off)[want[3]].sum(1)
    form = _host_form(want) if metric == IP else want
    for B in BS:
        ids, d, total = _host(ivf, q[:B], k, nprobe, metric)
        _same((ids, d), (form[0][:B], form[1][:B]), tag + (B,))
        assert total == rows[:B].sum(), tag + (B, "total_candidates")
    return want


# ---------------------------------------------------------------------------------------------- 1. the coarse launch across workgroups
@pytest.mark.parametrize("nlist", [65, 512, 513, 1000, 1023, 1024])
@pytest.mark.parametrize("dim", S.DIMS)
def test_coarse_launch_across_workgroups(gpu_pkg, dim, nlist):
    full = S.int_index(dim)
    data = full[:4] if nlist == S.NLIST else S.first_lists(full, nlist)
    k = 5
    plan = gpu_pkg.ivf_one_plan(len(data[0]), dim, nlist, _cus(), 1, 16, k, 8)
    assert plan[0] == 1 and plan[1] == min(_cus(), 256, (nlist + 63) // 64) and plan[1] > 1
    with _open(gpu_pkg, *data) as ivf:
        ivf.set_batch(16)
        sets = dict(S.query_sets(dim), last=S.last_lists_queries(data[1], nlist))
        for name in ("groups", "hot", "last"):
            for nprobe in (1, 8):
                _check_host(ivf, data, sets[name], k, nprobe, (dim, nlist, name, nprobe))


# ---------------------------------------------------------------------------------------------- 2. equal coarse scores
@pytest.mark.parametrize("dim", S.DIMS)
def test_equal_coarse_scores(gpu_pkg, dim):
    data = S.int_index(dim)
    vr, cents, off, r2o, _ = data
    sizes = np.diff(off)
    q = S.query_sets(dim)["dups"]
    k = 5
    with _open(gpu_pkg, *data[:4]) as ivf:
        ivf.set_batch(16)
        _check_host(ivf, data, q, k, 1, (dim, "dups", 1))
        _check_host(ivf, data, q, k, 2, (dim, "dups", 2))
        for B in BS:
            ids, d, total = _host(ivf, q[:B], k, 1)
            assert total == sum(int(sizes[S.PAIRS[i % 4][0]]) for i in range(B))  # the lower list's rows and nothing else
            for i in range(B):
                planted = r2o[off[S.PAIRS[i % 4][1]] + S.PLANT_ROW]
                assert planted not in ids[i] and d[i, 0] > 0
            ids, d, total = _host(ivf, q[:B], k, 2)
            assert total == B * sum(S.PAIR_SIZES)
            for i in range(B):
                assert ids[i, 0] == r2o[off[S.PAIRS[i % 4][1]] + S.PLANT_ROW] and d[i, 0] == 0 and d[i, 1] > 0


# ---------------------------------------------------------------------------------------------- 3. nprobe 64 .. 256
@pytest.mark.parametrize("nprobe", [64, 65, 255, 256])
@pytest.mark.parametrize("dim", S.DIMS)
def test_many_probes(gpu_pkg, dim, nprobe):
    data = S.int_index(dim)
    with _open(gpu_pkg, *data[:4]) as ivf:
        ivf.set_batch(16)
        for k in (1, 8, 16):  # (both KCAP instantiations of the scan)
            for name in ("groups", "hot", "dups"):
                _check_host(ivf, data, S.query_sets(dim)[name], k, nprobe, (dim, name, k, nprobe))


@pytest.mark.parametrize("nprobe", [65, 256])
@pytest.mark.parametrize("dim", S.DIMS)
def test_many_probes_inner_product(gpu_pkg, dim, nprobe):
    data = S.signed_variant(dim)
    q = data[4]
    assert q.min() < 0 < q.max() and data[0].min() < 0 < data[0].max()
    with _open(gpu_pkg, *data[:4]) as ivf:
        ivf.set_batch(16)
        for k in (8, 16):
            for a in (0, 16, 32):  # the groups, hot and dups sets
                _check_host(ivf, data, q[a:a + 16], k, nprobe, (dim, "ip", a, k, nprobe), metric=IP)


# ---------------------------------------------------------------------------------------------- 4. more units than workgroups
@pytest.mark.parametrize("name,nprobe", [("groups", 64), ("hot", 256)])
@pytest.mark.parametrize("dim", S.DIMS)
def test_more_units_than_workgroups(gpu_pkg, dim, name, nprobe):
    data = S.int_index(dim)
    vr, cents, off, r2o, _ = data
    q = S.query_sets(dim)[name]
    with _open(gpu_pkg, *data[:4]) as ivf:
        for k in (8, 16):
            plan = gpu_pkg.ivf_one_plan(len(vr), dim, S.NLIST, _cus(), 1, 16, k, nprobe)
            assert plan[0] == 1 and plan[2] == S.UNIT
            grid = plan[3]
            want = oracle.ivf_search(vr, off, r2o, cents, q, k, nprobe, return_probes=True)
            ivf.one_stats(reset=True)
            got = _dev(ivf, q, 1, 16, k, nprobe)
            batches, units = ivf.one_stats()
            assert batches == 1
            assert units >= 2 * grid + 1, (units, grid)  # some workgroup takes a third unit
            assert units == S.units_of(off, want[3])
            _same(got, want, (dim, name, k, nprobe))


# ---------------------------------------------------------------------------------------------- 5. the mask carried across units
def test_mask_carried_across_units(gpu_pkg):
    """Copies of query j sit in at least 20 lists that other queries of the batch probe and j does not: a workgroup that
    keeps the previous unit's column mask, or takes the wrong bit of it, returns one of them for j at distance 0."""
    dim, k, nprobe = 100, 8, 256
    _, cents, off, r2o, _ = S.int_index(dim)
    vr, planted = S.planted_index(dim)
    q = S.query_sets(dim)["hot"]
    want = oracle.ivf_search(vr, off, r2o, cents, q, k, nprobe, return_probes=True)
    for j, (lists, rows) in planted.items():
        assert len(lists) >= 20 and not set(lists.tolist()) & set(want[3][j].tolist())
        assert not set(r2o[rows].tolist()) & set(want[0][j].tolist()) and want[1][j, 0] > 0
    with _open(gpu_pkg, vr, cents, off, r2o) as ivf:
        for B in (16, 12):  # (B = 12 holds the three queries too)
            ivf.one_stats(reset=True)
            got = _dev(ivf, q, 1, B, k, nprobe)
            assert ivf.one_stats()[0] == 1
            for j, (lists, rows) in planted.items():
                assert not set(r2o[rows].tolist()) & set(got[0][j].tolist()), (B, j, "a planted row came back")
            _same(got, (want[0][:B], want[1][:B]), ("planted", B))


# ---------------------------------------------------------------------------------------------- 6. ties across workgroups in the final merge
def test_ties_across_workgroups(gpu_pkg):
    dim, k, nprobe = 100, 16, 64
    _, cents, off, r2o, _ = S.int_index(dim)
    vr = S.one_vector_index(dim)
    q = S.query_sets(dim)["groups"]
    want = oracle.ivf_search(vr, off, r2o, cents, q, k, nprobe, return_probes=True)
    grid = gpu_pkg.ivf_one_plan(len(vr), dim, S.NLIST, _cus(), 1, 16, k, nprobe)[3]
    with _open(gpu_pkg, vr, cents, off, r2o) as ivf:
        got = _dev(ivf, q, 1, 16, k, nprobe)
        batches, units = ivf.one_stats()
        assert batches == 1 and units >= grid  # every workgroup of the scan contributes a partial list
        for i in range(16):
            pos = np.sort(np.concatenate([np.arange(off[c], off[c + 1]) for c in want[3][i]]))[:k]
            assert got[0][i].tolist() == r2o[pos].tolist(), (i, "not the 16 lowest positions in position order")
            assert len(set(_bits(got[1][i]).tolist())) == 1
        _same(got, want, "one vector")


# ---------------------------------------------------------------------------------------------- 7. three batches back to back
@pytest.mark.parametrize("dim", S.DIMS)
def test_three_batches_back_to_back(gpu_pkg, dim):
    import torch
    data = S.int_index(dim)
    vr, cents, off, r2o, _ = data
    sets = S.query_sets(dim)
    q = np.concatenate([sets["groups"], sets["hot"], sets["dups"]])
    assert gpu_pkg.ivf_one_plan(len(vr), dim, S.NLIST, _cus(), 3, 16, 8, 64)[:2] == (1, min(_cus(), 256, 16))
    st = torch.cuda.Stream()
    with _open(gpu_pkg, *data[:4]) as ivf:
        for k, nprobe in ((8, 64), (16, 256), (5, 2)):
            want = oracle.ivf_search(vr, off, r2o, cents, q, k, nprobe)
            ivf.one_stats(reset=True)
            first = _dev(ivf, q, 3, 16, k, nprobe, stream=st)
            again = _dev(ivf, q, 3, 16, k, nprobe, stream=st)
            assert ivf.one_stats()[0] == 6
            _same(first, want, (dim, k, nprobe, "first"))
            assert np.array_equal(first[0], again[0]) and np.array_equal(_bits(first[1]), _bits(again[1]))


# ---------------------------------------------------------------------------------------------- 8. the edge of the rule
def test_nlist_1025_stays_off_the_route(gpu_pkg):
    dim, k = 100, 5
    data = S.one_more_list(dim)
    vr, cents, off, r2o = data
    assert gpu_pkg.ivf_one_plan(len(vr), dim, S.NLIST + 1, _cus(), 1, 16, k, 8)[0] == 0
    assert gpu_pkg.ivf_one_plan(len(vr), dim, S.NLIST, _cus(), 1, 16, k, 8)[0] == 1
    q = S.query_sets(dim)["groups"]
    with _open(gpu_pkg, *data) as ivf:
        ivf.set_batch(16)
        for nprobe in (8, 64):
            want = oracle.ivf_search(vr, off, r2o, cents, q, k, nprobe)
            got = ivf.searchBatch(q, 16, k, nprobe)
            assert ivf.one_stats() == (0, 0)
            _same(got, want, ("nlist 1025", nprobe))
            assert got[2] == want[2]
            one = _dev(ivf, q, 1, 1, k, nprobe)
            assert ivf.one_stats() == (0, 0)
            _same(one, (want[0][:1], want[1][:1]), ("nlist 1025, B = 1", nprobe))


# ---------------------------------------------------------------------------------------------- 9. non-integer data, once
def test_non_integer_data(gpu_pkg):
    vr, cents, off, r2o, q, fq, mask = S.gauss_index()
    k, nprobe = 5, S.GAUSS_NPROBE
    near_ties.require_teeth(mask, f"two-launch route, nlist 1024, nprobe {nprobe}")
    qq = np.concatenate([q, fq])
    want = oracle.ivf_search(vr, off, r2o, cents, qq, k, nprobe, return_probes=True, dot_order="chain")
    rows = np.diff(off)[want[3]].sum(1)
    with _open(gpu_pkg, vr, cents, off, r2o) as ivf:
        ivf.set_batch(16)
        for a in range(0, len(qq), 48):  # three batches of 16 per host call: every launch group is short
            part = qq[a:a + 48]
            ivf.one_stats(reset=True)
            ids, d, total = ivf.searchBatch(part, len(part), k, nprobe)
            assert ivf.one_stats()[0] == (len(part) + 15) // 16
            for i in range(len(part)):
                same = np.array_equal(ids[i], want[0][a + i]) and np.array_equal(_bits(d[i]), _bits(want[1][a + i]))
                assert same, near_ties.describe(cents, qq, a + i, nprobe)
            assert total == rows[a:a + 48].sum()
