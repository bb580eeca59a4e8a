"""The two-launch route of short calls on a general IVF index (ivf_one_coarse_kernel + ivf_one_scan_kernel):
a launch group of fewer than 4 batches of at most 16 queries, k <= 16.  The result of a call does not depend on the route,
so every case asserts through IVFIndex.one_stats() which route its calls took and then equality -- ids, distance bits,
empty slots, total_candidates -- with the CPU oracle or with the group route of the same library.

Data comes from the existing IVF tests (imported, not copied): the integer sets of test_gpu_ivf_nd.py and ivf_ip_data.py
(N = 6000 rows in 24 lists: one empty, one of 1 row, lists of 63 / 64 / 65 rows, one of 1200 rows, the last list ending at
row N), the forced coarse near-ties of near_ties.py and the cancelling self-queries of cancel_data.py.  Every precondition
is asserted on the CPU before the device is called."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import cancel_data
import ivf_ip_data as D
import ivf_one_child
import near_ties
import oracle
from test_gpu_ivf_nd import DIMS, EMPTY, N, NLIST, _gauss_index, _int_index, _int_lists, _open

pytestmark = pytest.mark.gpu

L2, IP = 0, 1
B16 = 16  # queries per batch of a short call at most


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def _same(got, want, tag):
    """ids and distance bits per query"""
    bad = [i for i in range(len(want[0])) if not (np.array_equal(_bits(got[1][i]), _bits(want[1][i])) and np.array_equal(got[0][i], want[0][i]))]
    assert not bad, (tag, "queries differ", bad[:10], got[0][bad[0]][:8], want[0][bad[0]][:8], got[1][bad[0]][:8], want[1][bad[0]][:8])


def _batches(nq, batch=B16):
    """batches a host call of nq queries under set_batch(batch) sends down the two-launch route: its launch group of full
    batches when there are fewer than 4 of them, and its ragged tail"""
    full, rem = divmod(nq, batch)
    return (full if full < 4 else 0) + (1 if rem else 0)


def _short_host(ivf, q, k, nprobe, metric=L2, chunk=3 * B16):
    """a host call per `chunk` queries (three batches of 16 at most: every launch group is short); returns (ids, dists,
    total_candidates, batches the calls should have sent down the route)"""
    ids, ds, total, nb = [], [], 0, 0
    for a in range(0, len(q), chunk):
        part = q[a:a + chunk]
        if metric == L2:
            i, d, t = ivf.searchBatch(part, len(part), k, nprobe)
        else:
            i, d, t = ivf.search_metric(part, k, nprobe, metric)
        ids.append(i)
        ds.append(d)
        total += t
        nb += _batches(len(part))
    return np.concatenate(ids), np.concatenate(ds), total, nb


def _dev(ivf, q, nb, B, k, nprobe, metric=L2, stream=None):
    """search_metric_dev_multi on [nb][B] queries; (ids, distances as the device returns them)"""
    import torch
    dev = torch.device("cuda:0")
    st = stream or torch.cuda.current_stream()
    with torch.cuda.stream(st):
        qd = torch.from_numpy(np.array(q[:nb * B], dtype=np.float32)).to(dev)
        gi = torch.full((nb * B, k), -7, dtype=torch.int32, device=dev)
        gd = torch.full((nb * B, k), 7.0, dtype=torch.float32, device=dev)
        ivf.search_metric_dev_multi(qd.data_ptr(), nb, B, k, nprobe, metric, gi.data_ptr(), gd.data_ptr(), st.cuda_stream)
    st.synchronize()
    return gi.cpu().numpy(), gd.cpu().numpy()


def _host_form(want):
    """an inner-product oracle result (s = -(q.v) ascending) as the host call returns it: q.v, +inf in empty slots"""
    return want[0], np.where(want[0] >= 0, -want[1], np.float32(np.inf)).astype(np.float32)


# ---------------------------------------------------------------------------------------------- 1. every dimension
@pytest.mark.parametrize("dim", DIMS)
def test_every_dimension(gpu_pkg, dim):
    data = _int_index(dim)
    vr, cents, off, r2o, q = data
    q = q[:40]
    with _open(gpu_pkg, vr, cents, off, r2o) as ivf:
        ivf.set_batch(B16)
        assert ivf.one_stats() == (0, 0)  # zero before the first short call
        for k, nprobe in ((1, 1), (5, 4), (16, NLIST)):
            oi, od, _, probes = oracle.ivf_search(vr, off, r2o, cents, q, k, nprobe, return_probes=True)
            rows = np.diff(off)[probes].sum(1)  # candidates per query
            if nprobe == 1:  # query 4 sits on the empty list's centroid
                assert probes[4, 0] == EMPTY and oi[4, 0] == -1 and od[4, 0] == np.inf
            for nq in (1, 16, 40):  # 40 = two full batches and a ragged one of 8
                ivf.one_stats(reset=True)
                ids, d, total = ivf.searchBatch(q[:nq], nq, k, nprobe)
                assert ivf.one_stats()[0] == _batches(nq) == {1: 1, 16: 1, 40: 3}[nq]
                _same((ids, d), (oi[:nq], od[:nq]), (dim, k, nprobe, nq))
                assert total == rows[:nq].sum(), (dim, k, nprobe, nq)
        # lists shorter than k: queries that probe only the 1-row list / only the empty one
        qq = np.stack([vr[off[5]], cents[EMPTY]])
        oi, od, ot = oracle.ivf_search(vr, off, r2o, cents, qq, 5, 1)
        assert oi[0, 0] == r2o[off[5]] and np.all(oi[0, 1:] == -1) and np.all(oi[1] == -1)
        ivf.one_stats(reset=True)
        ids, d, total = ivf.searchBatch(qq, 2, 5, 1)
        assert ivf.one_stats()[0] == 1
        assert np.array_equal(ids, oi) and np.array_equal(_bits(d), _bits(od)) and total == ot == 1
        assert np.all(ids[1] == -1) and np.all(d[1] == np.inf) and np.all(d[0, 1:] == np.inf)


# ---------------------------------------------------------------------------------------------- 2. the column mask
@pytest.mark.parametrize("nprobe", [1, 4])
def test_column_mask(gpu_pkg, nprobe):
    """A copy of query j's vector sits in a list another query of the batch probes and j does not: a scan that lets every
    column take every unit's rows returns it for j at distance 0."""
    dim, k = 100, 5
    vr, cents, off, r2o, q = _int_index(dim)
    q = np.array(q[:B16])
    vr = np.array(vr)
    oi, od, _, probes = oracle.ivf_search(vr, off, r2o, cents, q, k, nprobe, return_probes=True)
    sizes = np.diff(off)
    pick = None
    for j in range(5, B16):  # (queries 0..3 are rows, query 4 probes the empty list)
        for other in range(B16):
            for lst in probes[other]:
                if other != j and lst not in probes[j] and sizes[lst] > 70 and od[j, 0] > 0:
                    pick = (j, other, int(lst))
                    break
            if pick:
                break
        if pick:
            break
    assert pick, "no query of the batch has a list of its own"
    j, other, lst = pick
    row = off[lst] + 66  # (in the list's second 64-row block)
    vr[row] = q[j]
    want = oracle.ivf_search(vr, off, r2o, cents, q, k, nprobe, return_probes=True)
    assert np.array_equal(want[3], probes)  # the probes depend on the centroids alone
    assert lst not in want[3][j] and lst in want[3][other]
    assert r2o[row] not in want[0][j] and want[1][j, 0] > 0  # the planted row (distance 0) would be j's best
    with _open(gpu_pkg, vr, cents, off, r2o) as ivf:
        got = _dev(ivf, q, 1, B16, k, nprobe)
        assert ivf.one_stats()[0] == 1
        _same(got, want, ("mask", nprobe, pick))
        assert r2o[row] not in got[0][j]


# ---------------------------------------------------------------------------------------------- 3. lists cut across units
def test_lists_cut_across_units(gpu_pkg):
    dim, k = 100, 8
    unit = gpu_pkg.ivf_one_plan(3000, dim, 4, 256, 1, B16, k, 4)[2]
    assert unit == 512, "the sizes below are written for the unit the plan states"
    long_list = 4 * unit + 1
    n = long_list + 951
    vr, cents, off, r2o, hi, rng = _int_lists(dim, n, [long_list, 300, 300, 351], 7100)
    vr = np.array(vr)
    row = rng.integers(0, hi, size=dim).astype(np.float32)
    where = [0, unit + 5, 3 * unit - 1, 4 * unit]  # both ends of the list, four different units
    assert len({w // unit for w in where}) == 4 and where[-1] == long_list - 1
    vr[where] = row
    assert int((vr == row).all(1).sum()) == 4
    q = rng.integers(0, hi, size=(B16, dim)).astype(np.float32)
    q[0] = q[7] = row
    want = oracle.ivf_search(vr, off, r2o, cents, q, k, 4)
    assert want[0][0, :4].tolist() == r2o[where].tolist() and np.all(want[1][0, :4] == 0) and want[1][0, 4] > 0
    with _open(gpu_pkg, vr, cents, off, r2o) as ivf:
        got = ivf.searchBatch(q, B16, k, 4)
        batches, most_units = ivf.one_stats()
        assert batches == 1 and most_units >= 5
        assert most_units == sum((s + unit - 1) // unit for s in np.diff(off))
        _same(got, want, "units")
        assert got[2] == want[2]
        for i in (0, 7):  # ties come back in position order
            assert got[0][i, :4].tolist() == r2o[where].tolist()
        one = ivf.search(row, k, 4)  # (IVFIndex.search: one query, one batch)
        assert one[0][:4].tolist() == r2o[where].tolist() and ivf.one_stats()[1] == most_units


# ---------------------------------------------------------------------------------------------- 4. the arithmetic, bit for bit
@pytest.mark.parametrize("dim", [100, 384])
def test_forced_near_ties_l2(gpu_pkg, dim):
    vr, cents, off, r2o, q, fq, mask = _gauss_index(dim)
    near_ties.require_teeth(mask, f"two-launch route, L2, dim {dim}, nprobe 1")
    qq = np.concatenate([q, fq])
    with _open(gpu_pkg, vr, cents, off, r2o) as ivf:
        ivf.set_batch(B16)
        for k, nprobe in ((1, 1), (5, 4)):
            want = oracle.ivf_search(vr, off, r2o, cents, qq, k, nprobe, dot_order="chain")
            ivf.one_stats(reset=True)
            ids, d, total, nb = _short_host(ivf, qq, k, nprobe)
            assert ivf.one_stats()[0] == nb == (len(qq) + B16 - 1) // B16
            for i in range(len(qq)):
                same = np.array_equal(ids[i], want[0][i]) and np.array_equal(_bits(d[i]), _bits(want[1][i]))
                assert same, near_ties.describe(cents, qq, i, nprobe)
            assert total == want[2]


@pytest.mark.parametrize("dim", [100, 384])
def test_forced_near_ties_inner_product(gpu_pkg, dim):
    base, vr, cents, off, r2o, q, seeds = D.gauss_index(dim)
    fq, mask = near_ties.boundary_queries(cents, seeds, 1, np.random.default_rng(78), metric=1)
    near_ties.require_teeth(mask, f"two-launch route, inner product, dim {dim}, nprobe 1")
    qq = np.concatenate([q, fq])
    with _open(gpu_pkg, vr, cents, off, r2o) as ivf:
        ivf.set_batch(B16)
        for k, nprobe in ((1, 1), (5, 4)):
            want = oracle.ivf_search(vr, off, r2o, cents, qq, k, nprobe, metric=1, dot_order="chain")
            ivf.one_stats(reset=True)
            ids, d, total, nb = _short_host(ivf, qq, k, nprobe, metric=IP)
            assert ivf.one_stats()[0] == nb
            hw = _host_form(want)
            for i in range(len(qq)):
                same = np.array_equal(ids[i], hw[0][i]) and np.array_equal(_bits(d[i]), _bits(hw[1][i]))
                assert same, near_ties.describe(cents, qq, i, nprobe, 1)
            assert total == want[2]


@pytest.mark.parametrize("offset", [0, 4])
def test_cancelling_self_queries(gpu_pkg, offset):
    vr, off, r2o, cents, q = cancel_data.ivf_case(6000, 64, 100, offset, 24)
    k, nprobe = 5, 4
    want = oracle.ivf_search(vr, off, r2o, cents, q, k + 1, nprobe, dot_order="chain")
    cancel_data.require(want[1], k, f"two-launch route, offset {offset}")
    want = oracle.ivf_search(vr, off, r2o, cents, q, k, nprobe, dot_order="chain")
    with _open(gpu_pkg, vr, cents, off, r2o) as ivf:
        ivf.set_batch(B16)
        ids, d, total, nb = _short_host(ivf, q, k, nprobe)
        assert ivf.one_stats()[0] == nb
        _same((ids, d), want, ("cancel", offset))
        assert total == want[2]


# ---------------------------------------------------------------------------------------------- 5. inner product
@pytest.mark.parametrize("dim", [100, 768])
def test_inner_product_signed(gpu_pkg, dim):
    vr, cents, off, r2o, q = D.signed_index(dim)
    q = q[:40]
    with _open(gpu_pkg, vr, cents, off, r2o) as ivf:
        ivf.set_batch(B16)
        for k, nprobe in ((1, 1), (5, 4), (16, NLIST)):
            want = oracle.ivf_search(vr, off, r2o, cents, q, k, nprobe, metric=1)
            if nprobe == 1:
                assert np.all(want[0][4] == -1) and np.all(want[1][4] == np.inf)
            ivf.one_stats(reset=True)
            got = ivf.search_metric(q, k, nprobe, IP)
            assert ivf.one_stats()[0] == 3
            _same(got, _host_form(want), (dim, k, nprobe))
            assert got[2] == want[2]


@pytest.mark.parametrize("dim", [100, 768])
def test_inner_product_every_product_negative(gpu_pkg, dim):
    """A row past a list's end (the next list's, or a zero spare row: -0.0) would beat every real row here."""
    vr, cents, off, r2o, q = D.negative_index(dim)
    with _open(gpu_pkg, vr, cents, off, r2o) as ivf:
        for k, nprobe in ((16, 1), (5, 4)):
            want = oracle.ivf_search(vr, off, r2o, cents, q[:48], k, nprobe, return_probes=True, metric=1)
            assert np.all(want[1] > 0)
            if nprobe == 1:
                assert want[3][:4, 0].tolist() == [D.ONE_ROW, D.ROWS63, D.ROWS65, D.LAST]
            ivf.one_stats(reset=True)
            got = _dev(ivf, q, 3, B16, k, nprobe, IP)
            assert ivf.one_stats()[0] == 3
            _same(got, want, (dim, k, nprobe))
            if nprobe == 1:
                assert got[0][0, 0] == r2o[off[D.ONE_ROW]] and np.all(got[0][0, 1:] == -1) and np.all(got[1][0, 1:] == np.inf)
                lists = np.searchsorted(off, np.argsort(r2o)[np.maximum(got[0], 0)], side="right") - 1
                assert np.all((lists == want[3][:, :1]) | (got[0] < 0))  # no id from a neighbouring list or from behind row N


def test_inner_product_zero_products_are_negative_zero(gpu_pkg):
    vr, cents, off, r2o, q, planted = D.zeros_index()
    k = 5
    with _open(gpu_pkg, vr, cents, off, r2o) as ivf:
        for nprobe in (4, NLIST):
            want = oracle.ivf_search(vr, off, r2o, cents, q[:48], k, nprobe, metric=1)
            for i in D.ZERO_QUERIES:
                assert np.all(_bits(want[1][i]).view(np.uint32) == 0x80000000)
            ivf.one_stats(reset=True)
            got = _dev(ivf, q, 3, B16, k, nprobe, IP)
            assert ivf.one_stats()[0] == 3
            _same(got, want, ("zeros", nprobe))
            for i in D.ZERO_QUERIES:
                assert np.all(_bits(got[1][i]).view(np.uint32) == 0x80000000)


# ---------------------------------------------------------------------------------------------- 6. route independence
@pytest.mark.parametrize("dim", [100, 768])
def test_route_independence(gpu_pkg, dim):
    """Gaussian rows: the same 64 queries as one launch group of four batches (the group route) and as short calls."""
    base, vr, cents, off, r2o, q, seeds = D.gauss_index(dim)
    q = np.array(q[:64])
    odd = np.array(q)
    odd[3, dim // 2] = np.nan      # a query with a NaN: every score is NaN, no probe, empty slots
    odd[9, 0] = np.inf             # an infinite one
    odd[20, 1] = -np.inf
    with _open(gpu_pkg, vr, cents, off, r2o) as ivf:
        for qq, tag in ((q, "plain"), (odd, "nan/inf")):
            for metric in (L2, IP):
                for k, nprobe in ((5, 4), (16, 24)):
                    ivf.one_stats(reset=True)
                    group = _dev(ivf, qq, 4, B16, k, nprobe, metric)
                    assert ivf.one_stats() == (0, 0)  # four batches: the group route
                    parts = [_dev(ivf, qq[a:a + 32], 2, B16, k, nprobe, metric) for a in (0, 32)]
                    assert ivf.one_stats()[0] == 4
                    short = (np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts]))
                    _same(short, group, (dim, tag, metric, k, nprobe))
                    singles = [_dev(ivf, qq[a:a + 1], 1, 1, k, nprobe, metric) for a in (0, 3, 9, 20)]
                    for a, s in zip((0, 3, 9, 20), singles):
                        _same(s, (group[0][a:a + 1], group[1][a:a + 1]), (dim, tag, metric, k, nprobe, "B = 1", a))
            if tag == "nan/inf":
                assert np.all(group[0][3] == -1) and np.all(group[1][3] == np.inf)


# ---------------------------------------------------------------------------------------------- 7. state
def test_state(gpu_pkg):
    import torch
    dim, k, nprobe = 100, 5, 4
    data = _int_index(dim)
    vr, cents, off, r2o, q = data
    want = oracle.ivf_search(vr, off, r2o, cents, q, k, nprobe)
    vr2, cents2, off2, r2o2, q2 = D.signed_index(dim)
    want2 = oracle.ivf_search(vr2, off2, r2o2, cents2, q2[:16], k, nprobe)
    with _open(gpu_pkg, vr, cents, off, r2o) as ivf, _open(gpu_pkg, vr2, cents2, off2, r2o2) as other:
        first = _dev(ivf, q, 1, B16, k, nprobe)
        _same(first, (want[0][:16], want[1][:16]), "first")
        for rep in range(19):  # the tickets are left at zero: twenty identical calls
            again = _dev(ivf, q, 1, B16, k, nprobe)
            assert np.array_equal(again[0], first[0]) and np.array_equal(_bits(again[1]), _bits(first[1])), rep
        assert ivf.one_stats()[0] == 20
        # B = 1, 16, 7 between a long call on the same index and calls on a second index
        for rep in range(2):
            _same(_dev(ivf, q[40:41], 1, 1, k, nprobe), (want[0][40:41], want[1][40:41]), "B = 1")
            _same(_dev(other, q2, 1, B16, k, nprobe), want2, "second index")
            _same(_dev(ivf, q, 6, B16, k, nprobe), want, "long call")
            _same(_dev(ivf, q[16:32], 1, B16, k, nprobe), (want[0][16:32], want[1][16:32]), "B = 16")
            _same(_dev(ivf, q[50:57], 1, 7, k, nprobe), (want[0][50:57], want[1][50:57]), "B = 7")
        assert ivf.one_stats()[0] == 20 + 6 and other.one_stats()[0] == 2
        # vs_ivf_search_dev on a stream of its own
        st = torch.cuda.Stream()
        dev = torch.device("cuda:0")
        with torch.cuda.stream(st):
            qd = torch.from_numpy(np.array(q[60:65])).to(dev)
            gi = torch.full((5, k), -7, dtype=torch.int32, device=dev)
            gd = torch.zeros((5, k), dtype=torch.float32, device=dev)
            ivf.search_dev(qd.data_ptr(), 5, k, nprobe, gi.data_ptr(), gd.data_ptr(), st.cuda_stream)
        st.synchronize()
        _same((gi.cpu().numpy(), gd.cpu().numpy()), (want[0][60:65], want[1][60:65]), "stream")
        assert ivf.one_stats(reset=True)[0] == 27 and ivf.one_stats() == (0, 0)


def test_first_short_call_on_a_stream_of_its_own(gpu_pkg):
    """The route's scratch (tickets, counters) is made by the index's first short call: here that call comes on a
    non-default stream, with nprobe = 24 of 24 lists and k = 16."""
    import torch
    dim, k, nprobe = 100, 16, NLIST
    vr, cents, off, r2o, q = _int_index(dim)
    want = oracle.ivf_search(vr, off, r2o, cents, q[:B16], k, nprobe)
    with _open(gpu_pkg, vr, cents, off, r2o) as ivf:
        got = _dev(ivf, q, 1, B16, k, nprobe, stream=torch.cuda.Stream())
        assert ivf.one_stats()[0] == 1
        _same(got, want, "first call, own stream")


# ---------------------------------------------------------------------------------------------- 8. what stays off the route
def test_what_stays_off_the_route(gpu_pkg):
    dim, k, nprobe = 100, 5, 4
    vr, cents, off, r2o, q = _int_index(dim)
    q = q[:16]
    want = oracle.ivf_search(vr, off, r2o, cents, q, k, nprobe, return_probes=True)
    pairs = int((np.diff(off)[want[3]] > 0).sum())
    u8 = vr.astype(np.uint8)
    assert np.array_equal(u8.astype(np.float32), vr)
    with gpu_pkg.IVFIndex.from_u8(u8, cents, off, r2o) as ivf:
        ivf.nd_u8_stats(reset=True)
        got = ivf.searchBatch(q, 16, k, nprobe)  # precision 0: the byte rows, the group route
        assert ivf.one_stats() == (0, 0) and ivf.nd_u8_stats() == (pairs, 0)
        _same(got, want, "u8 precision 0")
        ivf.set_precision(1)
        ivf.nd_u8_stats(reset=True)
        got = ivf.searchBatch(q, 16, k, nprobe)
        assert ivf.one_stats()[0] == 1 and ivf.nd_u8_stats() == (0, pairs)
        _same(got, want, "u8 precision 1")
        assert got[2] == want[2]
    with _open(gpu_pkg, vr, cents, off, r2o) as ivf:
        w17 = oracle.ivf_search(vr, off, r2o, cents, q, 17, nprobe)
        got = ivf.search_topk(q, 17, nprobe)
        _same(got, w17, "k = 17")
        q64 = _int_index(dim)[4][:64]
        w64 = oracle.ivf_search(vr, off, r2o, cents, q64, k, nprobe)
        _same(_dev(ivf, q64, 4, B16, k, nprobe), w64, "four batches")
        assert ivf.one_stats() == (0, 0)
        out = (C.c_int64 * 2)()
    with gpu_pkg.BruteForceIndex(np.array(vr[:500])) as bf:
        assert gpu_pkg.lib().vs_ivf_one_stats(bf._h, out, 0) == -1
    base = gpu_pkg.synth_sift(2000, seed=5)
    vr128, off128, r2o128 = gpu_pkg.ivf_layout_from_assignment(base, np.arange(2000) % 8, 8)
    with _open(gpu_pkg, vr128, base[:8].copy(), off128, r2o128) as spec:  # the specialised 128-d index
        assert gpu_pkg.lib().vs_ivf_one_stats(spec._h, out, 0) == -1


# ---------------------------------------------------------------------------------------------- 9. children
def _child(tmp_path, tag, env_set):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    e = dict(os.environ)
    for name in ("VSEARCH_IVF_ONE", "VSEARCH_IVF_ND_FORCE"):
        e.pop(name, None)
    e.update(env_set)
    path = str(tmp_path / f"{tag}.npz")
    r = subprocess.run([sys.executable, os.path.join(root, "tests", "ivf_one_child.py"), root, path, tag], env=e, capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0 and "IVF_ONE_CHILD_OK" in r.stdout, (tag, r.stdout[-400:], r.stderr[-1500:])
    return np.load(path)


def test_toggle_keeps_the_group_route(gpu_pkg, tmp_path):
    """VSEARCH_IVF_ONE=0, read when the index is created: the counter stays 0 and the results are the route's."""
    child = _child(tmp_path, "toggle", {"VSEARCH_IVF_ONE": "0"})
    assert child["batches"].tolist() == [0] * len(ivf_one_child.CALLS)
    here = ivf_one_child.run_toggle(gpu_pkg)
    assert here["batches"].tolist() == [nb for nb, _, _, _ in ivf_one_child.CALLS]
    for key in here:
        if key[0] == "d":
            assert np.array_equal(_bits(child[key]), _bits(here[key])), key
        elif key != "batches":
            assert np.array_equal(child[key], here[key]), key


def test_forced_general_index_at_128d(gpu_pkg, tmp_path):
    """VSEARCH_IVF_ND_FORCE=1 on 128-d synth_sift rows (everything exact): the general index takes the route and returns
    what the specialised index returns here."""
    child = _child(tmp_path, "forced", {"VSEARCH_IVF_ND_FORCE": "1"})
    assert child["general"] and child["batches"].tolist() == [nb for nb, _, _, _ in ivf_one_child.CALLS]
    here = ivf_one_child.run_forced(gpu_pkg, want_general=False)
    for key in here:
        if key not in ("batches", "general"):
            assert np.array_equal(child[key], here[key]), key
