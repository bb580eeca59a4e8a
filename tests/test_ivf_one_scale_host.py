"""The preconditions of tests/test_gpu_ivf_one_scale.py, asserted against the CPU oracle alone: the data of
tests/ivf_one_scale_data.py does what the GPU cases rely on.  Nothing here needs a device."""
import numpy as np
import pytest

import ivf_one_scale_data as S
import near_ties
import oracle

K = 5


def _probes(data, q, nprobe, **kw):
    vr, cents, off, r2o = data[:4]
    return oracle.ivf_search(vr, off, r2o, cents, q, K, nprobe, return_probes=True, **kw)


def test_twin_dimension_has_an_odd_number_of_segments():
    dim_p = lambda d: (d + 15) & ~15  # nd_dim_p
    assert (dim_p(20) // 16) % 2 == 0  # why the twin is not dim 20
    for dim in S.DIMS:
        assert (dim_p(dim) // 16) % 2 == 1
    assert dim_p(40) * 64 < dim_p(100) * 64 < 8 * 256 * 4  # the won table is the larger overlay at both (dim_p < 128)


@pytest.mark.parametrize("dim", S.DIMS)
def test_integer_exactness_and_list_shapes(dim):
    vr, cents, off, r2o, anchors = S.int_index(dim)
    hi = 256
    assert 2 * dim * (hi - 1) ** 2 < 2 ** 24
    sets = S.query_sets(dim)
    for a in (vr, cents, *sets.values()):
        assert a.dtype == np.float32 and np.array_equal(a, np.rint(a)) and a.min() >= 0 and a.max() <= hi - 1
        assert not a.flags.writeable
    n = len(vr)
    sizes = np.diff(off)
    assert len(cents) == S.NLIST and off[0] == 0 and off[-1] == n and 12000 <= n <= 14000 and vr.nbytes < 6 << 20
    assert sorted(r2o.tolist()) == list(range(n))
    for c, rows in S.SHAPED.items():
        assert sizes[c] == rows
    assert {0, 1, 63, 64, 65, 511, 512, 513} <= set(sizes.tolist())
    assert sizes[S.HOT] >= 3000 and (sizes[S.HOT] + S.UNIT - 1) // S.UNIT >= 6
    rest = np.delete(sizes, list(S.SHAPED))
    assert rest.min() >= 4 and rest.max() <= 12
    assert sizes[-1] > 0  # the last list ends at row N
    # the distances of the oracle are the exact integers (and so is any fp32 evaluation of them)
    q = np.concatenate(list(sets.values()))
    oi, od, _ = oracle.ivf_search(vr, off, r2o, cents, q, K, 8)
    exact = oracle.exact_int_dists(q, vr)
    o2r = np.argsort(r2o)
    for i in range(len(q)):
        got = od[i][oi[i] >= 0]
        assert np.array_equal(got, exact[i, o2r[oi[i][oi[i] >= 0]]].astype(np.float32))


def test_groups_are_spread_over_lanes_and_slots():
    g = S.group_of()
    for grp in range(S.GROUPS):
        ids = np.nonzero(g == grp)[0]
        assert len(ids) == S.PER_GROUP
        lanes, slots = ids & 63, ids >> 6
        assert len(set(lanes.tolist())) >= 32                      # many lanes
        assert np.bincount(lanes, minlength=64).max() >= 2         # several register slots of one lane
        assert len(set(slots.tolist())) >= 12
        assert ids.max() - ids.min() > 4 * S.PER_GROUP              # no contiguous id range
        assert (ids >= 512).any() and (ids < 512).any()
    for lo, hi in S.PAIRS:
        assert g[lo] == g[hi]
    (a, a64), (b, b960), (c, c1), (d, d513) = S.PAIRS
    assert a64 == a + 64 and (a & 63) == (a64 & 63) and (a64 >> 6) == (a >> 6) + 1
    assert b960 == b + 960 and (b & 63) == (b960 & 63) and (b >> 6, b960 >> 6) == (0, 15)
    assert c1 == c + 1 and (c >> 6) == (c1 >> 6)
    assert d513 == d + 513 and d // 2 != d513 // 2  # two lists per thread of the unit table: different owners


@pytest.mark.parametrize("dim", S.DIMS)
def test_group_queries_probe_their_group(dim):
    data = S.int_index(dim)
    off, g = data[2], S.group_of()
    q = S.query_sets(dim)["groups"]
    probes = _probes(data, q, 64)[3]
    for i in range(16):
        assert sorted(probes[i].tolist()) == np.nonzero(g == i)[0].tolist()
    assert len(np.unique(probes)) == S.NLIST  # the union is every list: every unit's mask has exactly one bit
    units = S.units_of(off, probes)
    assert units == int(((np.diff(off) + S.UNIT - 1) // S.UNIT).sum()) and units >= 2 * 256 + 1
    # nprobe 1 and 8 stay inside the group as well
    for nprobe in (1, 8):
        p = _probes(data, q, nprobe)[3]
        assert all(set(p[i].tolist()) <= set(np.nonzero(g == i)[0].tolist()) for i in range(16))


@pytest.mark.parametrize("dim", S.DIMS)
def test_hot_queries_probe_the_hot_list_and_differ(dim):
    data = S.int_index(dim)
    off = data[2]
    q = S.query_sets(dim)["hot"]
    assert (_probes(data, q, 64)[3] == S.HOT).any(1).all()
    probes = _probes(data, q, 256)[3]
    assert (probes == S.HOT).any(1).all()
    masks = np.zeros(S.NLIST, dtype=np.int64)
    for i in range(16):
        masks[probes[i]] |= 1 << i
    assert masks[S.HOT] == 0xffff
    live = masks[masks != 0]
    assert len(set(live.tolist())) >= 8                                 # many different masks
    bits = np.array([bin(m).count("1") for m in live])
    assert (bits >= 2).sum() >= 256 and (bits >= 8).sum() >= 64          # ... that carry many bits
    assert (live[1:] != live[:-1]).mean() > 0.5                          # ... and differ from unit to unit
    assert S.units_of(off, probes) >= 2 * 256 + 1                        # more units than twice the largest grid


@pytest.mark.parametrize("dim", S.DIMS)
def test_duplicate_centroids(dim):
    data = S.int_index(dim)
    vr, cents, off, r2o, _ = data
    sizes = np.diff(off)
    q = S.query_sets(dim)["dups"]
    _, inv, cnt = np.unique(cents, axis=0, return_inverse=True, return_counts=True)
    twins = {tuple(np.nonzero(inv.ravel() == u)[0].tolist()) for u in np.nonzero(cnt > 1)[0]}
    assert twins == set(S.PAIRS)  # these four pairs and no other
    p1, p2 = _probes(data, q, 1), _probes(data, q, 2)
    for i in range(16):
        lo, hi = S.PAIRS[i % 4]
        assert np.array_equal(cents[lo].view(np.int32), cents[hi].view(np.int32)) and np.array_equal(q[i], cents[lo])
        assert sizes[lo] != sizes[hi] and sizes[lo] > 0 and sizes[hi] > 0
        planted = off[hi] + S.PLANT_ROW
        assert np.array_equal(vr[planted], cents[hi])
        assert not (vr[off[lo]:off[lo + 1]] == cents[lo]).all(1).any()
        # nprobe 1: the lower list id wins; the planted row is absent; the candidates are the lower list's rows
        assert p1[3][i].tolist() == [lo]
        assert r2o[planted] not in p1[0][i] and p1[1][i, 0] > 0
        # nprobe 2: both, the lower first, and the planted row (distance 0) leads
        assert p2[3][i].tolist() == [lo, hi]
        assert p2[0][i, 0] == r2o[planted] and p2[1][i, 0] == 0 and p2[1][i, 1] > 0
    assert p1[2] == sum(int(sizes[S.PAIRS[i % 4][0]]) for i in range(16))
    assert p2[2] == 16 * sum(S.PAIR_SIZES)


def test_planted_copies_leave_the_probes_alone():
    dim = 100
    data = S.int_index(dim)
    vr, cents, off, r2o, _ = data
    q = S.query_sets(dim)["hot"]
    pv, planted = S.planted_index(dim)
    before = _probes(data, q, 256)
    after = _probes((pv, cents, off, r2o), q, 256)
    assert np.array_equal(before[3], after[3])  # the probes depend on the centroids alone
    sizes = np.diff(off)
    assert sorted(planted) == sorted(S.MASK_QUERIES)
    all_rows = np.concatenate([rows for _, rows in planted.values()])
    assert len(set(all_rows.tolist())) == len(all_rows)  # no copy overwrites another
    for j, (lists, rows) in planted.items():
        assert len(lists) >= 20
        others = set(np.delete(after[3], j, axis=0).ravel().tolist())
        assert set(lists.tolist()) <= others and not set(lists.tolist()) & set(after[3][j].tolist())
        for c, row in zip(lists, rows):
            assert off[c] <= row < off[c + 1] and np.array_equal(pv[row], q[j])
            assert row - off[c] >= 64 or sizes[c] <= 66
        assert any(row - off[c] >= 64 for c, row in zip(lists, rows))
        assert after[1][j, 0] > 0 and not set(r2o[rows].tolist()) & set(after[0][j].tolist())
        # ... and a scan that let column j take those units would return them: they are rows at distance 0
        assert np.all(oracle.exact_int_dists(q[j:j + 1], pv[rows]) == 0)


def test_one_vector_index_ranks_by_position():
    dim = 100
    vr, cents, off, r2o, _ = S.int_index(dim)
    ov = S.one_vector_index(dim)
    assert (ov == ov[0]).all()
    q = S.query_sets(dim)["groups"]
    oi, od, _, probes = oracle.ivf_search(ov, off, r2o, cents, q, 16, 64, return_probes=True)
    for i in range(16):
        pos = np.sort(np.concatenate([np.arange(off[c], off[c + 1]) for c in probes[i]]))[:16]
        assert oi[i].tolist() == r2o[pos].tolist() and len(set(od[i].tolist())) == 1


def test_one_more_list_is_past_the_rule():
    dim = 100
    vr, cents, off, r2o = S.one_more_list(dim)
    assert len(cents) == S.NLIST + 1 == len(off) - 1 and off[-1] == len(vr) == len(r2o)
    assert sorted(r2o.tolist()) == list(range(len(vr)))


@pytest.mark.parametrize("dim", S.DIMS)
def test_first_lists(dim):
    data = S.int_index(dim)
    highs = {hi: lo for lo, hi in S.PAIRS}
    for nlist in (65, 512, 513, 1000, 1023):
        sub = S.first_lists(data, nlist)
        vr, cents, off, r2o = sub
        assert len(cents) == nlist and off[-1] == len(vr) == len(r2o) and sorted(r2o.tolist()) == list(range(len(vr)))
        assert np.array_equal(np.argsort(r2o), np.argsort(data[3][:len(vr)], kind="stable"))  # the ids keep their order
        assert S.HOT < nlist and off[-1] > off[-2]
        # a query on a list's centroid probes that list first (the higher list of a pair: the lower one)
        p = _probes(sub, S.last_lists_queries(cents, nlist), 1)[3][:, 0]
        assert p.tolist() == [highs.get(c, c) for c in range(nlist - 1, nlist - 17, -1)] and p[0] == nlist - 1


def test_gauss_index_has_teeth():
    vr, cents, off, r2o, q, fq, mask = S.gauss_index()
    assert len(cents) == S.NLIST and vr.shape[1] == 100 and not np.array_equal(vr, np.rint(vr))
    near_ties.require_teeth(mask, f"two-launch route, nlist 1024, nprobe {S.GAUSS_NPROBE}")
