"""IVF search on uint8 rows at any vector length (vs_ivf_create_nd_u8: a general IVF index that keeps its rows once more
as int8 and scans them with ivf_scan_nd_i8_kernel) against the CPU oracle and against vs_ivf_create on the same rows as
float.

Data: the small index of tests/test_gpu_ivf_nd.py (N = 6000, 24 lists cut to 0, 1, 63, 64, 65 and 1200 rows, the last one
ending at row N): integers in [0, hi) with 2 dim (hi - 1)^2 < 2^24 and hi <= 256.  Every row is a byte row, every query
qualifies for the byte rows and every fp32 quantity is exact, so oracle.ivf_search is an equality reference and the
fp32 index returns the same bits.  Results are equal by contract whichever kernel ran: vs_ivf_nd_u8_stats (pairs planned
on bytes, pairs planned on fp32; a pair is a query and a probed list that holds rows) tells which one did."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle
from test_gpu_ivf_nd import EMPTY, N, NLIST, _int_index, _open

pytestmark = pytest.mark.gpu

DIMS = [1, 63, 64, 65, 100, 130, 384, 960, 2048]  # dim_b / 64 = 1, 1, 1, 2, 2, 3 (pair + tail), 6, 15, 32


def _open_u8(pkg, vr, cents, off, r2o):
    u8 = vr.astype(np.uint8)
    assert np.array_equal(u8.astype(np.float32), vr)
    return pkg.IVFIndex.from_u8(u8, cents, off, r2o)


def _same(a, b):
    """ids, distance bits and total_candidates of two searchBatch results"""
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.int32), b[1].view(np.int32)) and a[2] == b[2]


def _pairs(probes, off):
    """(query, probe) pairs that get a slot: the probed list holds rows"""
    sizes = np.diff(off)
    return int((sizes[probes] > 0).sum())


@pytest.mark.parametrize("dim", DIMS)
def test_every_step_shape(gpu_pkg, dim):
    data = _int_index(dim)
    vr, cents, off, r2o, q = data
    q = q[:70]
    with _open_u8(gpu_pkg, vr, cents, off, r2o) as u8, _open(gpu_pkg, vr, cents, off, r2o) as f32:
        assert u8.getDim() == dim and u8.getNumVectors() == N and u8.getNumClusters() == NLIST
        for k, nprobe in ((1, 1), (5, 4), (16, NLIST)):
            oi, od, ototal, probes = oracle.ivf_search(vr, off, r2o, cents, q, k, nprobe, return_probes=True)
            u8.nd_u8_stats(reset=True)
            got = u8.searchBatch(q, len(q), k, nprobe)  # batches of 32, 32 and 6
            tag = (dim, k, nprobe)
            assert np.array_equal(got[1], od), ("dists differ", tag)
            assert np.array_equal(got[0], oi), ("ids differ", tag)
            assert got[2] == ototal, ("total_candidates differs", tag)
            assert _same(got, f32.searchBatch(q, len(q), k, nprobe)), tag
            assert u8.nd_u8_stats() == (_pairs(probes, off), 0), tag
            if nprobe == 1:  # query 4 sits on the empty list's centroid: nothing but padding
                assert got[0][4, 0] == -1 and got[1][4, 0] == np.inf
            if nprobe == NLIST:
                assert got[0].min() >= 0
        # ragged and full items: every list's run holds nq slots
        oi, od, _ = oracle.ivf_search(vr, off, r2o, cents, q[:33], 5, NLIST)
        for nq in (1, 15, 16, 17, 33):
            u8.nd_u8_stats(reset=True)
            got = u8.searchBatch(q[:nq], nq, 5, NLIST)
            assert np.array_equal(got[0], oi[:nq]) and np.array_equal(got[1], od[:nq]) and got[2] == nq * N, (dim, nq)
            assert _same(got, f32.searchBatch(q[:nq], nq, 5, NLIST)), (dim, nq)
            assert u8.nd_u8_stats() == (nq * (NLIST - 1), 0), (dim, nq)
        # lists shorter than k: queries that probe only the 1-row list / only the empty one
        qq = np.stack([vr[off[5]], cents[EMPTY]])
        oi, od, ot = oracle.ivf_search(vr, off, r2o, cents, qq, 5, 1)
        got = u8.searchBatch(qq, 2, 5, 1)
        assert np.array_equal(got[0], oi) and np.array_equal(got[1], od) and got[2] == ot
        assert np.all(got[0][1] == -1) and np.all(got[1][1] == np.inf)
        # batch sizes
        want4 = oracle.ivf_search(vr, off, r2o, cents, q, 5, 4)
        wantn = oracle.ivf_search(vr, off, r2o, cents, q, 5, NLIST)
        for batch in (1, 7, 32):
            u8.set_batch(batch)
            for nprobe, want in ((4, want4), (NLIST, wantn)):
                got = u8.searchBatch(q, len(q), 5, nprobe)
                assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and got[2] == want[2], (dim, batch, nprobe)


@pytest.mark.parametrize("dim", [100, 384])
def test_mixed_groups(gpu_pkg, dim):
    """A third of the queries of one call carry a value that is no byte (0.5, 256, -1): their pairs are planned on the fp32
    rows, the others on bytes, in the same launch group; after set_precision(1) every pair is."""
    vr, cents, off, r2o, q = _int_index(dim)
    q = np.array(q[:70])
    rng = np.random.default_rng(8100 + dim)
    bad = np.arange(1, 70, 3)
    for j, i in enumerate(bad):
        q[i, rng.integers(0, dim)] = (0.5, 256.0, -1.0)[j % 3]
    n_bad, n_ok = len(bad), 70 - len(bad)
    with _open_u8(gpu_pkg, vr, cents, off, r2o) as u8, _open(gpu_pkg, vr, cents, off, r2o) as f32:
        for k, nprobe in ((5, NLIST), (16, NLIST)):
            want = f32.searchBatch(q, 70, k, nprobe)
            u8.nd_u8_stats(reset=True)
            assert _same(u8.searchBatch(q, 70, k, nprobe), want), (dim, k)
            assert u8.nd_u8_stats() == (n_ok * (NLIST - 1), n_bad * (NLIST - 1))
        assert _same(u8.searchBatch(q, 70, 5, 4), f32.searchBatch(q, 70, 5, 4))
        u8.set_precision(1)
        u8.nd_u8_stats(reset=True)
        assert _same(u8.searchBatch(q, 70, 5, NLIST), f32.searchBatch(q, 70, 5, NLIST))
        assert u8.nd_u8_stats() == (0, 70 * (NLIST - 1))
        u8.set_precision(2)
        u8.nd_u8_stats(reset=True)
        assert _same(u8.searchBatch(q, 70, 5, NLIST), f32.searchBatch(q, 70, 5, NLIST))
        assert u8.nd_u8_stats() == (n_ok * (NLIST - 1), n_bad * (NLIST - 1))


def _with_a_row_of_255(dim):
    vr, cents, off, r2o, q = _int_index(dim)
    vr = np.array(vr)
    vr[off[0] + 700] = 255.0  # (inside the 1200-row list)
    assert vr[np.arange(N) != off[0] + 700].max() < 255
    return vr, cents, off, r2o, q


def test_the_norm_boundary(gpu_pkg):
    """dim 258, one row all 255: max ||b||^2 = 2^24 - 766.  A query of squared norm 766 runs on bytes, one of 767 on fp32."""
    dim = 258
    vr, cents, off, r2o, _ = _with_a_row_of_255(dim)
    assert int((vr.astype(np.int64) ** 2).sum(1).max()) == 2 ** 24 - 766
    q = np.zeros((2, dim), dtype=np.float32)
    q[0, :3] = (27, 6, 1)
    q[1, :4] = (27, 6, 1, 1)
    assert (q[0] ** 2).sum() == 766 and (q[1] ** 2).sum() == 767
    with _open_u8(gpu_pkg, vr, cents, off, r2o) as u8, _open(gpu_pkg, vr, cents, off, r2o) as f32:
        u8.set_precision(2)
        for i, want_stats in ((0, (NLIST - 1, 0)), (1, (0, NLIST - 1))):
            u8.nd_u8_stats(reset=True)
            got = u8.searchBatch(q[i:i + 1], 1, 5, NLIST)
            assert _same(got, f32.searchBatch(q[i:i + 1], 1, 5, NLIST)), i
            assert u8.nd_u8_stats() == want_stats, i
        u8.nd_u8_stats(reset=True)
        assert _same(u8.searchBatch(q, 2, 16, NLIST), f32.searchBatch(q, 2, 16, NLIST))
        assert u8.nd_u8_stats() == (NLIST - 1, NLIST - 1)
        # the exact integers, from the CPU: query 0 against every row
        d0 = ((vr.astype(np.int64) - q[0].astype(np.int64)) ** 2).sum(1)
        got = u8.searchBatch(q[:1], 1, 5, NLIST)
        assert np.array_equal(got[1][0].astype(np.int64), np.sort(d0)[:5])


def test_no_byte_copy_when_a_row_norm_reaches_2_24(gpu_pkg):
    dim = 260
    vr, cents, off, r2o, q = _with_a_row_of_255(dim)
    assert int((vr.astype(np.int64) ** 2).sum(1).max()) >= 2 ** 24
    q = q[:70]
    with _open_u8(gpu_pkg, vr, cents, off, r2o) as u8, _open(gpu_pkg, vr, cents, off, r2o) as f32:
        assert gpu_pkg.lib().vs_set_precision(u8._h, 2) == -5
        u8.set_precision(0)
        u8.nd_u8_stats(reset=True)
        assert _same(u8.searchBatch(q, 70, 5, NLIST), f32.searchBatch(q, 70, 5, NLIST))
        assert _same(u8.searchBatch(q, 70, 16, 4), f32.searchBatch(q, 70, 16, 4))
        by, fp = u8.nd_u8_stats()
        assert by == 0 and fp >= 70 * (NLIST - 1)


def test_device_calls(gpu_pkg):
    """search_dev (B = 5) and search_dev_multi (3 x 32) on a non-default torch stream give the host call's arrays."""
    import torch
    dev = torch.device("cuda:0")
    vr, cents, off, r2o, q = _int_index(100)
    dim, k, nprobe, nq = 100, 5, 4, 96
    with _open_u8(gpu_pkg, vr, cents, off, r2o) as u8:
        want_i, want_d, _ = u8.searchBatch(q, nq, k, nprobe)
        oi, od, _, probes = oracle.ivf_search(vr, off, r2o, cents, q, k, nprobe, return_probes=True)
        assert np.array_equal(want_i, oi) and np.array_equal(want_d, od)
        u8.nd_u8_stats(reset=True)
        st = torch.cuda.Stream()
        with torch.cuda.stream(st):
            qd = torch.from_numpy(np.array(q)).to(dev)
            gi = torch.full((nq, k), -7, dtype=torch.int32, device=dev)
            gd = torch.zeros((nq, k), dtype=torch.float32, device=dev)
            u8.search_dev_multi(qd.data_ptr(), 3, 32, k, nprobe, gi.data_ptr(), gd.data_ptr(), st.cuda_stream)
            si = torch.full((5, k), -7, dtype=torch.int32, device=dev)
            sd = torch.zeros((5, k), dtype=torch.float32, device=dev)
            u8.search_dev(qd.data_ptr() + 40 * dim * 4, 5, k, nprobe, si.data_ptr(), sd.data_ptr(), st.cuda_stream)
        st.synchronize()
        assert np.array_equal(gi.cpu().numpy(), want_i) and np.array_equal(gd.cpu().numpy(), want_d)
        assert np.array_equal(si.cpu().numpy(), want_i[40:45]) and np.array_equal(sd.cpu().numpy(), want_d[40:45])
        assert u8.nd_u8_stats() == (_pairs(probes, off) + _pairs(probes[40:45], off), 0)


_FORCED_SCRIPT = r"""
import sys, numpy as np
sys.path.insert(0, sys.argv[1])
import __graft_entry__ as ge
pkg = ge.load_package()
z = np.load(sys.argv[2])
with pkg.IVFIndex.from_u8(z["vr"], z["cents"], z["off"], z["r2o"]) as ivf:
    i5, d5, t5 = ivf.searchBatch(z["q"], len(z["q"]), 5, 4)
    i16, d16, t16 = ivf.searchBatch(z["q"], len(z["q"]), 16, 24)
    stats = ivf.nd_u8_stats()
np.savez(sys.argv[3], i5=i5, d5=d5, t5=t5, i16=i16, d16=d16, t16=t16, stats=np.array(stats))
print("FORCED_OK")
"""


def test_dim_128(gpu_pkg, tmp_path):
    """dim 128 gives vs_ivf_create's specialised index; with VSEARCH_IVF_ND_FORCE=1 (a child process: the variable is read
    at creation) the general byte index, with the same ids and distances."""
    vr, cents, off, r2o, q = _int_index(128)
    q = q[:70]
    u8rows = vr.astype(np.uint8)
    assert "VSEARCH_IVF_ND_FORCE" not in os.environ
    with gpu_pkg.IVFIndex.from_u8(u8rows, cents, off, r2o) as u8, _open(gpu_pkg, vr, cents, off, r2o) as f32:
        out = (C.c_int64 * 2)()
        assert gpu_pkg.lib().vs_ivf_nd_u8_stats(u8._h, out, 0) == -1  # the specialised index: no general byte plan
        a5, a16 = u8.searchBatch(q, 70, 5, 4), u8.searchBatch(q, 70, 16, NLIST)
        assert _same(a5, f32.searchBatch(q, 70, 5, 4)) and _same(a16, f32.searchBatch(q, 70, 16, NLIST))
    o5 = oracle.ivf_search(vr, off, r2o, cents, q, 5, 4)
    assert np.array_equal(a5[0], o5[0]) and np.array_equal(a5[1], o5[1]) and a5[2] == o5[2]
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src, dst = str(tmp_path / "in.npz"), str(tmp_path / "out.npz")
    np.savez(src, vr=u8rows, cents=cents, off=off, r2o=r2o, q=q)
    e = dict(os.environ)
    e["VSEARCH_IVF_ND_FORCE"] = "1"
    r = subprocess.run([sys.executable, "-c", _FORCED_SCRIPT, root, src, dst], env=e, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "FORCED_OK" in r.stdout, (r.stdout[-400:], r.stderr[-1200:])
    z = np.load(dst)
    assert np.array_equal(z["i5"], a5[0]) and np.array_equal(z["d5"], a5[1]) and int(z["t5"]) == a5[2]
    assert np.array_equal(z["i16"], a16[0]) and np.array_equal(z["d16"], a16[1]) and int(z["t16"]) == a16[2]
    assert z["stats"][0] > 0 and z["stats"][1] == 0  # the general byte index, every pair on bytes


def test_refusals(gpu_pkg):
    import torch
    L = gpu_pkg.lib()
    data = _int_index(100)
    vr, cents, off, r2o, q = data
    q = np.array(q[:8])

    def refused(call, *a):
        with pytest.raises(gpu_pkg.VSearchError) as e:
            call(*a)
        assert e.value.status == -5 and "100" in str(e.value), str(e.value)

    with _open_u8(gpu_pkg, vr, cents, off, r2o) as u8:
        refused(u8.searchBatch, q, len(q), 17, 4)
        refused(u8.set_metric, gpu_pkg.METRIC_IP)
        refused(u8.widek_stats)
        dev = torch.device("cuda:0")
        qd = torch.from_numpy(q).to(dev)
        gi = torch.zeros((8, 17), dtype=torch.int32, device=dev)
        gd = torch.zeros((8, 17), dtype=torch.float32, device=dev)
        s = torch.cuda.current_stream().cuda_stream
        refused(u8.search_dev, qd.data_ptr(), 8, 17, 4, gi.data_ptr(), gd.data_ptr(), s)
        refused(u8.search_dev_multi, qd.data_ptr(), 1, 8, 17, 4, gi.data_ptr(), gd.data_ptr(), s)
        refused(gpu_pkg.IVFIndex.search_dev_vshards, [u8, u8], qd.data_ptr(), 1, 8, 5, 4, gi.data_ptr(), gd.data_ptr(), s)
        u8.set_metric(gpu_pkg.METRIC_L2)
        for precision in (0, 1, 2):
            u8.set_precision(precision)
        # still usable after the refusals
        oi, od, ot = oracle.ivf_search(vr, off, r2o, cents, q, 5, 4)
        got = u8.searchBatch(q, len(q), 5, 4)
        assert np.array_equal(got[0], oi) and np.array_equal(got[1], od) and got[2] == ot
    out = (C.c_int64 * 2)(7, 7)
    with _open(gpu_pkg, vr, cents, off, r2o) as f32:
        assert L.vs_ivf_nd_u8_stats(f32._h, out, 0) == -1
    with gpu_pkg.BruteForceIndex.from_u8(vr[:500].astype(np.uint8)) as bf:
        assert L.vs_ivf_nd_u8_stats(bf._h, out, 0) == -1
    assert tuple(out) == (7, 7)


def test_save_gives_an_fp32_general_index(gpu_pkg, tmp_path):
    vr, cents, off, r2o, q = _int_index(100)
    q = q[:40]
    d = tmp_path / "idx"
    with _open_u8(gpu_pkg, vr, cents, off, r2o) as u8:
        u8.save(str(d))
        a = u8.searchBatch(q, len(q), 5, 3)
    assert np.array_equal(np.load(d / "vectors_reordered.npy"), vr) and np.array_equal(np.load(d / "centroids.npy"), cents)
    with gpu_pkg.IVFIndex(str(d)) as f32:
        assert _same(a, f32.searchBatch(q, len(q), 5, 3))
        out = (C.c_int64 * 2)()
        assert gpu_pkg.lib().vs_ivf_nd_u8_stats(f32._h, out, 0) == -1


def test_build_u8(gpu_pkg):
    """build_u8 at dim 100: k-means on the rows as float, the index on the reordered rows as bytes; at nprobe = nlist a
    search is exact brute force on the same rows (equal distances in a result may come in either id order: the index
    ranks them by reordered position)."""
    vr, _, _, _, q = _int_index(100)
    base = vr.astype(np.uint8)
    q = q[:70]
    k = 5
    ivf, iters = gpu_pkg.IVFIndex.build_u8(base, NLIST, max_iter=5, seed=7)
    with ivf, gpu_pkg.BruteForceIndex.from_u8(base) as bf:
        nlist = ivf.getNumClusters()
        assert ivf.getDim() == 100 and ivf.getNumVectors() == N and nlist == gpu_pkg.clamp_nlist(N, NLIST) and iters >= 1
        ivf.nd_u8_stats(reset=True)
        ids, d, total = ivf.searchBatch(q, len(q), k, nlist)
        by, fp = ivf.nd_u8_stats()
        bi, bd = bf.search(q, k)
    assert total == len(q) * N and fp == 0 and by > 0
    assert np.array_equal(d, bd)
    b64, q64 = base.astype(np.int64), q.astype(np.int64)
    exact = (q64 * q64).sum(1)[:, None] - 2 * (q64 @ b64.T) + (b64 * b64).sum(1)[None, :]
    for i in range(len(q)):
        assert np.array_equal(exact[i, ids[i]], d[i].astype(np.int64)), i  # every id has the distance it is listed with
        assert len(set(ids[i].tolist())) == k
        if len(set(d[i].tolist())) == k and exact[i][exact[i] == int(d[i, -1])].size == 1:  # no ties in or at the end of the result
            assert np.array_equal(ids[i], bi[i]), i
