"""The two-launch byte route of short calls on a general IVF index made from uint8 rows (vs_ivf_create_nd_u8 at precision 0
or 2: ivf_one_coarse_kernel in its byte-index mode + ivf_one_scan_u8_kernel): a launch group of fewer than 4
batches of at most 16 queries, k <= 16.  The result of a call does not depend on the route, so every case first asserts
which route its calls took -- IVFIndex.one_u8_stats() (batches, mixed batches, most units), one_stats() == (0, 0) (the fp32
route's counters stay put) and nd_u8_stats() (pairs on bytes, pairs on fp32, per query) -- and then equality of ids,
distance bits and total_candidates with the CPU oracle, which is exact on this integer data, and with the fp32 index.

Data comes from the existing IVF tests (imported, not copied): the integer sets of test_gpu_ivf_nd.py (N = 6000 rows in 24
lists: one empty, one of 1 row, lists of 63 / 64 / 65 rows, one of 1200 rows, the last list ending at row N) and of
ivf_ip_data.py.  Every precondition is asserted on the CPU before the device is called."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import ivf_ip_data as D
import ivf_one_u8_child
import oracle
from test_gpu_ivf_nd import EMPTY, N, NLIST, _int_index, _open
from test_gpu_ivf_nd_u8 import DIMS, _with_a_row_of_255

pytestmark = pytest.mark.gpu

L2, IP = 0, 1
B16 = 16  # queries per batch of a short call at most
NOT_BYTES = (0.5, 256.0, -1.0)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def _same(got, want, tag):
    """ids and distance bits per query"""
    bad = [i for i in range(len(want[0])) if not (np.array_equal(_bits(got[1][i]), _bits(want[1][i])) and np.array_equal(got[0][i], want[0][i]))]
    assert not bad, (tag, "queries differ", bad[:10], got[0][bad[0]][:8], want[0][bad[0]][:8], got[1][bad[0]][:8], want[1][bad[0]][:8])


def _open_u8(pkg, vr, cents, off, r2o):
    u8 = vr.astype(np.uint8)
    assert np.array_equal(u8.astype(np.float32), vr)
    ivf = pkg.IVFIndex.from_u8(u8, cents, off, r2o)
    ivf.set_batch(B16)
    return ivf


def _open_f32(pkg, vr, cents, off, r2o):
    ivf = _open(pkg, vr, cents, off, r2o)
    ivf.set_batch(B16)
    return ivf


def _batches(nq):
    full, rem = divmod(nq, B16)
    assert full < 4
    return full + (1 if rem else 0)


def _is_byte_query(q, bmax):
    ok = np.all((q >= 0) & (q <= 255) & (q == np.floor(q)), axis=1)
    n2 = (np.where(ok[:, None], q, 0).astype(np.int64) ** 2).sum(1)
    return ok & (n2 <= 2 ** 24 - bmax)


def _expect(off, probes, valid, unit):
    """what the route's counters should say after ONE host call of len(probes) queries in batches of 16: (batches, mixed
    batches, most units of a batch), (pairs on bytes, pairs on fp32)"""
    sizes = np.diff(off)
    pairs = (sizes[probes] > 0).sum(1)
    mixed = most = 0
    for a in range(0, len(probes), B16):
        v, pr = valid[a:a + B16], probes[a:a + B16]
        l8 = {int(c) for c in pr[v].ravel() if c >= 0 and sizes[c] > 0}
        l32 = {int(c) for c in pr[~v].ravel() if c >= 0 and sizes[c] > 0}
        mixed += 1 if (l8 and l32) else 0
        most = max(most, sum(-(-int(sizes[c]) // unit) for c in l8) + sum(-(-int(sizes[c]) // 512) for c in l32))
    return (_batches(len(probes)), mixed, most), (int(pairs[valid].sum()), int(pairs[~valid].sum()))


def _unit(pkg, dim):
    unit = pkg.ivf_one_plan_u8(N, dim, NLIST, 256, 1, B16, 16, NLIST)[2]
    assert unit % 64 == 0 and unit >= 64
    return unit


def _spoil(q, rows, seed):
    """queries `rows` get one value that is no byte each"""
    q = np.array(q)
    rng = np.random.default_rng(seed)
    for j, i in enumerate(rows):
        q[i, rng.integers(0, q.shape[1])] = NOT_BYTES[j % 3]
    return q


def _dev(ivf, q, nb, B, k, nprobe, metric=L2, stream=None, repeat=1):
    """search_metric_dev_multi on [nb][B] queries, `repeat` times back to back into buffers of their own without
    synchronising in between; the list of (ids, distances as the device returns them)"""
    import torch
    dev = torch.device("cuda:0")
    st = stream or torch.cuda.current_stream()
    outs = []
    with torch.cuda.stream(st):
        qd = torch.from_numpy(np.array(q[:nb * B], dtype=np.float32)).to(dev)
        for _ in range(repeat):
            gi = torch.full((nb * B, k), -7, dtype=torch.int32, device=dev)
            gd = torch.full((nb * B, k), 7.0, dtype=torch.float32, device=dev)
            ivf.search_metric_dev_multi(qd.data_ptr(), nb, B, k, nprobe, metric, gi.data_ptr(), gd.data_ptr(), st.cuda_stream)
            outs.append((gi, gd))
    st.synchronize()
    return [(gi.cpu().numpy(), gd.cpu().numpy()) for gi, gd in outs]


def _host_form(want):
    """an inner-product oracle result (s = -(q.v) ascending) as the host call returns it: q.v, +inf in empty slots"""
    return want[0], np.where(want[0] >= 0, -want[1], np.float32(np.inf)).astype(np.float32)


# ---------------------------------------------------------------------------------------------- 1. every step shape
@pytest.mark.parametrize("dim", DIMS)
def test_every_step_shape(gpu_pkg, dim):
    data = _int_index(dim)
    vr, cents, off, r2o, q = data
    q = q[:40]
    sizes = np.diff(off)
    unit = _unit(gpu_pkg, dim)
    assert sizes[0] == 1200 and 1200 % 64 != 0  # the long list: its last unit ends off a block boundary
    assert unit != 512 or -(-1200 // unit) == 3  # ... and at the default unit it is a list of several units
    bmax = int((vr.astype(np.int64) ** 2).sum(1).max())
    assert np.all(_is_byte_query(q, bmax))
    valid = np.ones(40, dtype=bool)
    with _open_u8(gpu_pkg, vr, cents, off, r2o) as u8, _open_f32(gpu_pkg, vr, cents, off, r2o) as f32:
        assert u8.one_u8_stats() == (0, 0, 0)  # zero before the first such call
        for k, nprobe in ((1, 1), (5, 4), (16, NLIST)):
            oi, od, _, probes = oracle.ivf_search(vr, off, r2o, cents, q, k, nprobe, return_probes=True)
            rows = sizes[probes].sum(1)
            if nprobe == 1:  # query 4 sits on the empty list's centroid
                assert probes[4, 0] == EMPTY and oi[4, 0] == -1 and od[4, 0] == np.inf
            for nq in (1, 16, 40):  # 40 = two full batches and a ragged one of 8
                want_one, want_nd = _expect(off, probes[:nq], valid[:nq], unit)
                assert want_one[0] == {1: 1, 16: 1, 40: 3}[nq] and want_one[1] == 0 and want_nd[1] == 0
                u8.one_u8_stats(reset=True)
                u8.nd_u8_stats(reset=True)
                ids, d, total = u8.searchBatch(q[:nq], nq, k, nprobe)
                assert u8.one_u8_stats() == want_one, (dim, k, nprobe, nq)
                assert u8.one_stats() == (0, 0) and u8.nd_u8_stats() == want_nd, (dim, k, nprobe, nq)
                _same((ids, d), (oi[:nq], od[:nq]), (dim, k, nprobe, nq))
                assert total == rows[:nq].sum(), (dim, k, nprobe, nq)
                f = f32.searchBatch(q[:nq], nq, k, nprobe)
                _same((ids, d), f, (dim, k, nprobe, nq, "fp32 index"))
                assert total == f[2]
        # lists shorter than k: queries that probe only the 1-row list / only the empty one
        qq = np.stack([vr[off[5]], cents[EMPTY]])
        assert np.all(_is_byte_query(qq, bmax))
        oi, od, ot, probes = oracle.ivf_search(vr, off, r2o, cents, qq, 5, 1, return_probes=True)
        assert oi[0, 0] == r2o[off[5]] and np.all(oi[0, 1:] == -1) and np.all(oi[1] == -1)
        u8.one_u8_stats(reset=True)
        u8.nd_u8_stats(reset=True)
        ids, d, total = u8.searchBatch(qq, 2, 5, 1)
        assert u8.one_u8_stats() == (1, 0, 1) and u8.one_stats() == (0, 0) and u8.nd_u8_stats() == (1, 0)
        assert np.array_equal(ids, oi) and np.array_equal(_bits(d), _bits(od)) and total == ot == 1
        assert np.all(ids[1] == -1) and np.all(d[1] == np.inf) and np.all(d[0, 1:] == np.inf)


# ---------------------------------------------------------------------------------------------- 2. mixed batches
@pytest.mark.parametrize("dim", [100, 384])
def test_mixed_batches(gpu_pkg, dim):
    """In batches of 16 a third of the queries carry a value that is no byte: their lists are scanned on the fp32 rows by
    the same launch.  Then a batch whose queries are all of that kind (fp32 units only), and a batch in which such a query
    is the only one that probes some list."""
    vr, cents, off, r2o, q = _int_index(dim)
    sizes = np.diff(off)
    unit = _unit(gpu_pkg, dim)
    bmax = int((vr.astype(np.int64) ** 2).sum(1).max())
    q48 = _spoil(q[:48], range(1, 48, 3), 8300 + dim)
    valid48 = _is_byte_query(q48, bmax)
    assert valid48.sum() == 32 and not valid48[1::3].any()
    all_bad = _spoil(q[48:64], range(16), 8400 + dim)
    assert not _is_byte_query(all_bad, bmax).any()
    with _open_u8(gpu_pkg, vr, cents, off, r2o) as u8, _open_f32(gpu_pkg, vr, cents, off, r2o) as f32:
        for k, nprobe in ((5, 4), (16, NLIST), (16, 4), (5, NLIST)):
            probes = oracle.ivf_search(vr, off, r2o, cents, q48, k, nprobe, return_probes=True)[3]
            want_one, want_nd = _expect(off, probes, valid48, unit)
            assert want_one[:2] == (3, 3) and want_nd[0] > 0 and want_nd[1] > 0
            u8.one_u8_stats(reset=True)
            u8.nd_u8_stats(reset=True)
            got = u8.searchBatch(q48, 48, k, nprobe)
            assert u8.one_u8_stats() == want_one, (dim, k, nprobe)
            assert u8.one_stats() == (0, 0) and u8.nd_u8_stats() == want_nd, (dim, k, nprobe)
            want = f32.searchBatch(q48, 48, k, nprobe)
            _same(got, want, (dim, k, nprobe, "mixed"))
            assert got[2] == want[2]
            # every query of the batch on the fp32 rows: phase 2 only, the mixed count stays put
            probes = oracle.ivf_search(vr, off, r2o, cents, all_bad, k, nprobe, return_probes=True)[3]
            want_one, want_nd = _expect(off, probes, np.zeros(16, dtype=bool), unit)
            assert want_one[:2] == (1, 0) and want_nd[0] == 0 and want_nd[1] > 0
            u8.one_u8_stats(reset=True)
            u8.nd_u8_stats(reset=True)
            got = u8.searchBatch(all_bad, 16, k, nprobe)
            assert u8.one_u8_stats() == want_one and u8.one_stats() == (0, 0) and u8.nd_u8_stats() == want_nd, (dim, k, nprobe)
            want = f32.searchBatch(all_bad, 16, k, nprobe)
            _same(got, want, (dim, k, nprobe, "all on fp32"))
            assert got[2] == want[2]
        # a list that only a query of the fp32 kind probes: its units are fp32 units alone
        k, nprobe = 5, 4
        qb = q48[:16]
        probes = oracle.ivf_search(vr, off, r2o, cents, qb, k, nprobe, return_probes=True)[3]
        v = valid48[:16]
        alone = [(i, int(c)) for i in np.flatnonzero(~v) for c in probes[i]
                 if sizes[c] > 0 and not any(c in probes[o] for o in range(16) if o != i)]
        assert alone, "no query of the fp32 kind has a list of its own in this batch"
        got = u8.searchBatch(qb, 16, k, nprobe)
        _same(got, f32.searchBatch(qb, 16, k, nprobe), (dim, "sole prober", alone[0]))


# ---------------------------------------------------------------------------------------------- 3. the column mask across kinds
@pytest.mark.parametrize("nprobe", [1, 4])
def test_column_mask_across_kinds(gpu_pkg, nprobe):
    """A copy of byte query j's vector sits in a list that only fp32-kind queries of the batch probe, and a row one value
    away from fp32-kind query i sits in a list that only byte queries probe: a scan that lets a column take the rows of the
    other kind's units returns them, as j's and i's best by far."""
    dim, k = 100, 5
    vr, cents, off, r2o, q = _int_index(dim)
    vr = np.array(vr)
    sizes = np.diff(off)
    bmax = int((vr.astype(np.int64) ** 2).sum(1).max())
    spoiled = list(range(6, B16, 2))
    q = _spoil(q[:B16], spoiled, 8500)  # (queries 0..3 are rows, query 4 probes the empty list)
    valid = _is_byte_query(q, bmax)
    assert not valid[spoiled].any() and valid.sum() == B16 - len(spoiled)
    oi, od, _, probes = oracle.ivf_search(vr, off, r2o, cents, q, k, nprobe, return_probes=True)
    by8 = {int(c) for c in probes[valid].ravel()}
    by32 = {int(c) for c in probes[~valid].ravel()}
    pick8 = next(((j, c) for j in np.flatnonzero(valid)[5:] for c in sorted(by32 - by8) if sizes[c] > 64 and od[j, 0] > 4), None)
    pick32 = next(((i, c) for i in np.flatnonzero(~valid) for c in sorted(by8 - by32) if sizes[c] > 64 and od[i, 0] > 4), None)
    assert pick8 and pick32, "the batch has no list that only one kind of query probes"
    (j, l8), (i, l32) = pick8, pick32
    row8, row32 = off[l8] + min(66, sizes[l8] - 1), off[l32] + min(66, sizes[l32] - 1)  # (in the lists' second 64-row blocks)
    vr[row8] = q[j]
    near = np.clip(np.rint(q[i]), 0, 255)
    assert 0 < ((near - q[i]) ** 2).sum() <= 1  # one value away: the row of bytes nearest to query i
    vr[row32] = near
    assert np.array_equal(_is_byte_query(q, int((vr.astype(np.int64) ** 2).sum(1).max())), valid)
    want = oracle.ivf_search(vr, off, r2o, cents, q, k, nprobe, return_probes=True)
    assert np.array_equal(want[3], probes)  # the probes depend on the centroids alone
    assert r2o[row8] not in want[0][j] and want[1][j, 0] > 0 and r2o[row32] not in want[0][i] and want[1][i, 0] > 1
    with _open_u8(gpu_pkg, vr, cents, off, r2o) as u8, _open_f32(gpu_pkg, vr, cents, off, r2o) as f32:
        got = _dev(u8, q, 1, B16, k, nprobe)[0]
        assert u8.one_u8_stats()[:2] == (1, 1) and u8.one_stats() == (0, 0)
        _same(got, _dev(f32, q, 1, B16, k, nprobe)[0], ("mask", nprobe, pick8, pick32))
        _same((got[0][valid], got[1][valid]), (want[0][valid], want[1][valid]), ("mask, oracle", nprobe))
        assert r2o[row8] not in got[0][j] and r2o[row32] not in got[0][i]


# ---------------------------------------------------------------------------------------------- 4. the norm boundary
def test_the_norm_boundary(gpu_pkg):
    """dim 258, one row all 255: max ||b||^2 = 2^24 - 766.  A query of squared norm 766 runs on bytes, one of 767 on fp32."""
    dim = 258
    vr, cents, off, r2o, _ = _with_a_row_of_255(dim)
    assert int((vr.astype(np.int64) ** 2).sum(1).max()) == 2 ** 24 - 766
    q = np.zeros((2, dim), dtype=np.float32)
    q[0, :3] = (27, 6, 1)
    q[1, :4] = (27, 6, 1, 1)
    assert (q[0] ** 2).sum() == 766 and (q[1] ** 2).sum() == 767
    assert _is_byte_query(q, 2 ** 24 - 766).tolist() == [True, False]
    with _open_u8(gpu_pkg, vr, cents, off, r2o) as u8, _open_f32(gpu_pkg, vr, cents, off, r2o) as f32:
        for precision in (2, 0):
            u8.set_precision(precision)
            for i, want_stats in ((0, (NLIST - 1, 0)), (1, (0, NLIST - 1))):
                u8.nd_u8_stats(reset=True)
                u8.one_u8_stats(reset=True)
                got = u8.searchBatch(q[i:i + 1], 1, 5, NLIST)
                assert u8.one_u8_stats()[:2] == (1, 0) and u8.one_stats() == (0, 0) and u8.nd_u8_stats() == want_stats, (precision, i)
                want = f32.searchBatch(q[i:i + 1], 1, 5, NLIST)
                _same(got, want, ("boundary", precision, i))
                assert got[2] == want[2]
            u8.nd_u8_stats(reset=True)
            u8.one_u8_stats(reset=True)
            got = u8.searchBatch(q, 2, 16, NLIST)
            assert u8.one_u8_stats()[:2] == (1, 1) and u8.nd_u8_stats() == (NLIST - 1, NLIST - 1)
            _same(got, f32.searchBatch(q, 2, 16, NLIST), ("boundary, both", precision))
        # the exact integers, from the CPU: query 0 against every row
        d0 = ((vr.astype(np.int64) - q[0].astype(np.int64)) ** 2).sum(1)
        got = u8.searchBatch(q[:1], 1, 5, NLIST)
        assert np.array_equal(got[1][0].astype(np.int64), np.sort(d0)[:5])


# ---------------------------------------------------------------------------------------------- 5. inner product
@pytest.mark.parametrize("dim", [100, 384])
def test_inner_product(gpu_pkg, dim):
    vr, cents, off, r2o, q = _int_index(dim)
    q = np.array(q[:48])
    q[7] = 0  # every product exactly zero: -0.0 on the device form
    unit = _unit(gpu_pkg, dim)
    bmax = int((vr.astype(np.int64) ** 2).sum(1).max())
    assert np.all(_is_byte_query(q, bmax))
    qm = _spoil(q, range(1, 48, 3), 8600 + dim)
    vm = _is_byte_query(qm, bmax)
    with _open_u8(gpu_pkg, vr, cents, off, r2o) as u8, _open_f32(gpu_pkg, vr, cents, off, r2o) as f32:
        # the index's FIRST inner-product call is a short one: it builds the rows' byte sums
        want = oracle.ivf_search(vr, off, r2o, cents, q, 5, 4, metric=1, return_probes=True)
        want_one, want_nd = _expect(off, want[3], np.ones(48, dtype=bool), unit)
        got = u8.search_metric(q, 5, 4, IP)
        assert u8.one_u8_stats() == want_one and u8.one_stats() == (0, 0) and u8.nd_u8_stats() == want_nd
        _same(got, _host_form(want), (dim, "first IP call"))
        assert got[2] == want[2]
        l2_want = oracle.ivf_search(vr, off, r2o, cents, q, 5, 4)
        _same(u8.searchBatch(q, 48, 5, 4), l2_want, (dim, "L2 after IP"))
        for k, nprobe in ((16, NLIST), (1, 1), (5, 4)):
            want = oracle.ivf_search(vr, off, r2o, cents, q, k, nprobe, metric=1, return_probes=True)
            assert np.all(_bits(want[1][7][want[0][7] >= 0]).view(np.uint32) == 0x80000000)
            want_one, want_nd = _expect(off, want[3], np.ones(48, dtype=bool), unit)
            u8.one_u8_stats(reset=True)
            u8.nd_u8_stats(reset=True)
            got = _dev(u8, q, 3, B16, k, nprobe, IP)[0]
            assert u8.one_u8_stats() == want_one and u8.one_stats() == (0, 0) and u8.nd_u8_stats() == want_nd, (dim, k, nprobe)
            _same(got, want, (dim, k, nprobe, "device form"))
            assert np.all(_bits(got[1][7][got[0][7] >= 0]).view(np.uint32) == 0x80000000)
            _same(u8.search_metric(q, k, nprobe, IP), f32.search_metric(q, k, nprobe, IP), (dim, k, nprobe, "fp32 index"))
            # mixed batches
            probes = oracle.ivf_search(vr, off, r2o, cents, qm, k, nprobe, metric=1, return_probes=True)[3]
            want_one, want_nd = _expect(off, probes, vm, unit)
            assert want_one[0] == 3 and want_one[1] >= 1 and want_nd[0] > 0 and want_nd[1] > 0
            u8.one_u8_stats(reset=True)
            u8.nd_u8_stats(reset=True)
            got = u8.search_metric(qm, k, nprobe, IP)
            assert u8.one_u8_stats() == want_one and u8.nd_u8_stats() == want_nd, (dim, k, nprobe, "mixed")
            wantm = f32.search_metric(qm, k, nprobe, IP)
            _same(got, wantm, (dim, k, nprobe, "mixed"))
            assert got[2] == wantm[2]


def test_inner_product_rows_that_are_bytes_queries_that_are_not(gpu_pkg):
    """ivf_ip_data's all-negative set: the rows are bytes, every query is negative, every product negative -- fp32 units only,
    where a row past a list's end (a zero spare row: -0.0) would beat every real row."""
    dim = 100
    vr, cents, off, r2o, q = D.negative_index(dim)
    assert vr.min() >= 1 and vr.max() <= 255 and q.max() <= -1
    with _open_u8(gpu_pkg, vr, cents, off, r2o) as u8:
        for k, nprobe in ((16, 1), (5, 4)):
            want = oracle.ivf_search(vr, off, r2o, cents, q[:48], k, nprobe, return_probes=True, metric=1)
            assert np.all(want[1] > 0)
            u8.one_u8_stats(reset=True)
            u8.nd_u8_stats(reset=True)
            got = _dev(u8, q, 3, B16, k, nprobe, IP)[0]
            st, nd = u8.one_u8_stats(), u8.nd_u8_stats()
            assert st[:2] == (3, 0) and u8.one_stats() == (0, 0) and nd[0] == 0 and nd[1] == int((np.diff(off)[want[3]] > 0).sum())
            _same(got, want, (dim, k, nprobe))


# ---------------------------------------------------------------------------------------------- 6. device calls
def test_device_calls(gpu_pkg):
    """search_dev (B = 5) and search_metric_dev_multi (3 x 16) on a non-default torch stream into buffers filled with
    sentinels; the same call three times back to back without synchronising (tickets and counters are left clean); a long
    call (4 x 16: the group route) between two short ones on the same index."""
    import torch
    dev = torch.device("cuda:0")
    dim, k, nprobe = 100, 5, 4
    vr, cents, off, r2o, q = _int_index(dim)
    unit = _unit(gpu_pkg, dim)
    bmax = int((vr.astype(np.int64) ** 2).sum(1).max())
    qm = _spoil(q[:64], range(2, 64, 5), 8700)
    vm = _is_byte_query(qm, bmax)
    want = oracle.ivf_search(vr, off, r2o, cents, q[:64], k, nprobe, return_probes=True)
    with _open_u8(gpu_pkg, vr, cents, off, r2o) as u8, _open_f32(gpu_pkg, vr, cents, off, r2o) as f32:
        wantm = _dev(f32, qm, 4, B16, k, nprobe)[0]  # (four batches: the fp32 index's group route)
        st = torch.cuda.Stream()
        # the index's first short call comes on a stream of its own
        outs = _dev(u8, qm, 3, B16, k, nprobe, stream=st, repeat=3)
        want_one, want_nd = _expect(off, oracle.ivf_search(vr, off, r2o, cents, qm[:48], k, nprobe, return_probes=True)[3], vm[:48], unit)
        assert u8.one_u8_stats() == (3 * want_one[0], 3 * want_one[1], want_one[2]) and u8.one_stats() == (0, 0)
        assert u8.nd_u8_stats() == (3 * want_nd[0], 3 * want_nd[1])
        for rep, got in enumerate(outs):
            _same(got, (wantm[0][:48], wantm[1][:48]), ("3 x 16, mixed", rep))
        with torch.cuda.stream(st):
            qd = torch.from_numpy(np.array(q[40:45])).to(dev)
            si = torch.full((5, k), -7, dtype=torch.int32, device=dev)
            sd = torch.full((5, k), 7.0, dtype=torch.float32, device=dev)
            u8.one_u8_stats(reset=True)
            u8.search_dev(qd.data_ptr(), 5, k, nprobe, si.data_ptr(), sd.data_ptr(), st.cuda_stream)
        st.synchronize()
        assert u8.one_u8_stats()[:2] == (1, 0)
        _same((si.cpu().numpy(), sd.cpu().numpy()), (want[0][40:45], want[1][40:45]), "search_dev, B = 5")
        # short, long, short
        u8.one_u8_stats(reset=True)
        _same(_dev(u8, q, 1, B16, k, nprobe, stream=st)[0], (want[0][:16], want[1][:16]), "short before")
        assert u8.one_u8_stats()[0] == 1
        _same(_dev(u8, qm, 4, B16, k, nprobe, stream=st)[0], wantm, "long call")
        assert u8.one_u8_stats()[0] == 1  # the group route
        _same(_dev(u8, qm[16:], 2, B16, k, nprobe, stream=st)[0], (wantm[0][16:48], wantm[1][16:48]), "short after")
        assert u8.one_u8_stats()[0] == 3 and u8.one_stats() == (0, 0)


# ---------------------------------------------------------------------------------------------- 7. neighbouring routes left alone
def test_neighbouring_routes_are_left_alone(gpu_pkg):
    dim, k, nprobe = 100, 5, 4
    vr, cents, off, r2o, q = _int_index(dim)
    q = q[:16]
    want = oracle.ivf_search(vr, off, r2o, cents, q, k, nprobe, return_probes=True)
    pairs = int((np.diff(off)[want[3]] > 0).sum())
    out = (C.c_int64 * 3)(7, 7, 7)
    L = gpu_pkg.lib()
    with _open_u8(gpu_pkg, vr, cents, off, r2o) as u8:
        u8.set_precision(1)  # the fp32 two-launch route, unchanged
        got = u8.searchBatch(q, 16, k, nprobe)
        assert u8.one_stats()[0] == 1 and u8.one_u8_stats() == (0, 0, 0) and u8.nd_u8_stats() == (0, pairs)
        _same(got, want, "precision 1")
        u8.set_precision(0)
        w17 = oracle.ivf_search(vr, off, r2o, cents, q, 17, nprobe)
        _same(u8.search_topk(q, 17, nprobe), w17, "k = 17")  # the wide-k pipeline on the fp32 rows
        assert u8.one_u8_stats() == (0, 0, 0) and u8.one_stats()[0] == 1
        got = u8.searchBatch(q, 16, k, nprobe)
        assert u8.one_u8_stats()[0] == 1 and u8.one_stats()[0] == 1 and got[2] == want[2]
        _same(got, want, "precision 0 after 1")
    with _open(gpu_pkg, vr, cents, off, r2o) as f32:
        assert L.vs_ivf_one_u8_stats(f32._h, out, 0) == -1
    with gpu_pkg.BruteForceIndex.from_u8(np.array(vr[:500]).astype(np.uint8)) as bf:
        assert L.vs_ivf_one_u8_stats(bf._h, out, 0) == -1
    # a from_u8 index whose byte copy was dropped: no byte route, today's fp32 route for its short calls
    vr260, cents260, off260, r2o260, q260 = _with_a_row_of_255(260)
    assert int((vr260.astype(np.int64) ** 2).sum(1).max()) >= 2 ** 24
    w260 = oracle.ivf_search(vr260, off260, r2o260, cents260, q260[:16], k, nprobe)
    with _open_u8(gpu_pkg, vr260, cents260, off260, r2o260) as dropped:
        assert L.vs_ivf_one_u8_stats(dropped._h, out, 0) == -1
        got = dropped.searchBatch(q260[:16], 16, k, nprobe)
        assert dropped.one_stats()[0] == 1
        _same(got, w260, "byte copy dropped")
    assert tuple(out) == (7, 7, 7)


# ---------------------------------------------------------------------------------------------- 8, 9. children
def _child(tmp_path, tag, env_set):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    e = dict(os.environ)
    for name in ("VSEARCH_IVF_ONE", "VSEARCH_IVF_ONE_U8", "VSEARCH_IVF_ND_FORCE"):
        e.pop(name, None)
    e.update(env_set)
    path = str(tmp_path / f"{tag}.npz")
    r = subprocess.run([sys.executable, os.path.join(root, "tests", "ivf_one_u8_child.py"), root, path, tag], env=e, capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0 and "IVF_ONE_U8_CHILD_OK" in r.stdout, (tag, r.stdout[-400:], r.stderr[-1500:])
    return np.load(path)


def _compare(child, here):
    for key in here:
        if key[0] == "d":
            assert np.array_equal(_bits(child[key]), _bits(here[key])), key
        elif key[0] == "i":
            assert np.array_equal(child[key], here[key]), key


@pytest.mark.parametrize("tag,env", [("toggle_u8", {"VSEARCH_IVF_ONE_U8": "0"}), ("toggle_one", {"VSEARCH_IVF_ONE": "0"})])
def test_toggles_keep_the_group_route(gpu_pkg, tmp_path, tag, env):
    """Read when the index is created: the route's counters stay 0, the results and the pair counts are the route's."""
    for name in ("VSEARCH_IVF_ONE", "VSEARCH_IVF_ONE_U8", "VSEARCH_IVF_ND_FORCE"):
        assert name not in os.environ
    child = _child(tmp_path, tag, env)
    assert child["one_u8"].tolist() == [[0, 0, 0]] * len(ivf_one_u8_child.CALLS)
    here = ivf_one_u8_child.run_toggle(gpu_pkg)
    assert here["one_u8"][:, 0].tolist() == [nb for nb, _, _, _, _ in ivf_one_u8_child.CALLS]
    assert here["one_u8"][1:, 1].min() >= 1  # (the calls of 16-query batches hold both kinds of query)
    assert np.array_equal(child["nd_u8"], here["nd_u8"])
    _compare(child, here)


def test_forced_general_index_at_128d(gpu_pkg, tmp_path):
    """VSEARCH_IVF_ND_FORCE=1 at dim 128: from_u8 gives the general byte index, which takes the route and returns what the
    specialised index returns on this integer data."""
    child = _child(tmp_path, "forced", {"VSEARCH_IVF_ND_FORCE": "1"})
    assert child["general"]
    assert child["one_u8"][:, 0].tolist() == [nb for nb, _, _, _, _ in ivf_one_u8_child.CALLS] and child["one_u8"][:, 1].max() == 0
    assert child["nd_u8"][:, 0].min() > 0 and child["nd_u8"][:, 1].max() == 0
    here = ivf_one_u8_child.run_forced(gpu_pkg, want_general=False)
    _compare(child, here)
