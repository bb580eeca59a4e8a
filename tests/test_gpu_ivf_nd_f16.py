"""IVF search on float16 rows (vs_ivf_create_nd_f16, ivf_scan_nd_f16_kernel): every accepted call returns what the fp32
general index returns on the rows widened to float -- ids, distance bits, empty slots, total_candidates.

References: the CPU oracle (exact on integer data, in the kernels' chain order on real-valued data) and, in the same
process, vs_ivf_create on the widened rows.  The dimensions put 1, 1, 1, 2, 4, 5, 24 and 64 K steps of 32 elements on both
sides of the ring of four row sets (prologue only, tail only, one and many unrolled rounds); the lists are test_gpu_ivf_nd's
(empty, 1, 63, 64, 65 and 1200 rows, the last one ending at row N, where the last block reads the spare rows)."""
import ctypes as C

import numpy as np
import pytest

import ivf_ip_data as D
import near_ties
import oracle
from cancel_data import bits
from test_gpu_ivf_nd import N, NLIST, _gauss_index, _int_index, _open
from test_gpu_ivf_nd_ip import _assert_same, _dev, _host_form

pytestmark = pytest.mark.gpu

IP = 1


def _half(rows):
    """rows rounded to float16 and the same values widened back to float (what the index must behave as)"""
    h = np.ascontiguousarray(rows, dtype=np.float16)
    return h, h.astype(np.float32)


def _open_f16(pkg, rows, cents, off, r2o, exact=True):
    h, wide = _half(rows)
    assert not exact or np.array_equal(wide, rows)  # integers below 2048: the round trip is exact
    return pkg.IVFIndex.from_f16(h, cents, off, r2o)


def _check(ivf, data, q, k, nprobe):
    vr, cents, off, r2o = data[:4]
    want = oracle.ivf_search(vr, off, r2o, cents, q, k, nprobe)
    _assert_same(ivf.searchBatch(q, len(q), k, nprobe), want, (vr.shape[1], len(q), k, nprobe))


@pytest.mark.parametrize("dim", [1, 31, 32, 33, 100, 130, 768, 2048])
def test_integer_rows_equal_the_oracle(gpu_pkg, dim):
    data = _int_index(dim)
    with _open_f16(gpu_pkg, *data[:4]) as ivf:
        assert ivf.getDim() == dim and ivf.getNumVectors() == N and ivf.getNumClusters() == NLIST
        for k, nprobe in ((1, 1), (5, 4), (16, NLIST)):
            _check(ivf, data, data[4][:70], k, nprobe)


@pytest.mark.parametrize("nq,batch", [(1, 32), (15, 32), (16, 32), (17, 32), (33, 32), (70, 1), (70, 7), (70, 32)])
def test_ragged_and_full_items_and_batch_sizes(gpu_pkg, nq, batch):
    """nprobe = nlist: every list's run holds nq slots -- one ragged item, one full item, a full and a ragged one, ..."""
    data = _int_index(100)
    with _open_f16(gpu_pkg, *data[:4]) as ivf:
        ivf.set_batch(batch)
        _check(ivf, data, data[4][:nq], 5, NLIST)


@pytest.mark.parametrize("dim", [33, 384])
def test_real_valued_half_rows(gpu_pkg, dim):
    """N(0, 1) rows rounded to float16 with what a widening could get wrong planted: subnormals of both signs, a row made
    only of subnormals, +-6.0e4 (squares near 2^32) and duplicated rows.  Centroids and queries stay fp32, the forced
    coarse near-ties included.  Chain-order oracle for every query; bit for bit the fp32 index on the widened rows."""
    import torch
    vr, cents, off, r2o, q, fq, mask = _gauss_index(dim)
    near_ties.require_teeth(mask, f"general index dim {dim} nlist {NLIST} nprobe 1")
    rows = np.array(vr)
    tiny = np.float32(2.0 ** -24)  # the smallest float16 subnormal
    rows[7, :3] = (tiny, -tiny, 1023 * tiny)
    rows[off[9], -1] = -3 * tiny
    rows[N - 1] = tiny * (1 + np.arange(dim) % 1000) * np.where(np.arange(dim) % 2, -1, 1)  # the last row: subnormals only
    rows[11, 0], rows[off[7] + 1, dim // 2] = 6.0e4, -6.0e4
    rows[off[8]:off[8] + 3] = rows[off[9] + 5]  # duplicates: across two lists, and inside one
    h, wide = _half(rows)
    sub = (np.abs(wide) < 2.0 ** -14) & (wide != 0)
    assert (sub & (wide > 0)).any() and (sub & (wide < 0)).any() and sub[N - 1].all()
    assert (wide == 6.0e4).any() and (wide == -6.0e4).any() and np.isfinite(wide).all()
    qq = np.concatenate([q, fq])
    nb = len(qq) // 32
    st = torch.cuda.Stream()
    with gpu_pkg.IVFIndex.from_f16(h, cents, off, r2o) as ivf, _open(gpu_pkg, wide, cents, off, r2o) as f32:
        for k, nprobe in ((1, 1), (5, 4), (16, NLIST)):
            want = oracle.ivf_search(wide, off, r2o, cents, qq, k, nprobe, dot_order="chain")
            got = ivf.searchBatch(qq, len(qq), k, nprobe)
            _assert_same(got, want, (dim, k, nprobe, "oracle"))
            _assert_same(got, f32.searchBatch(qq, len(qq), k, nprobe), (dim, k, nprobe, "fp32 index"))
            with torch.cuda.stream(st):  # search_dev_multi on a non-default stream
                qd = torch.from_numpy(qq).to("cuda:0")
                gi = torch.full((2, nb * 32, k), -7, dtype=torch.int32, device="cuda:0")
                gd = torch.zeros((2, nb * 32, k), dtype=torch.float32, device="cuda:0")
                for j, index in enumerate((ivf, f32)):
                    index.search_dev_multi(qd.data_ptr(), nb, 32, k, nprobe, gi[j].data_ptr(), gd[j].data_ptr(), st.cuda_stream)
            st.synchronize()
            gi, gd = gi.cpu().numpy(), gd.cpu().numpy()
            _assert_same((gi[0], gd[0]), (gi[1], gd[1]), (dim, k, nprobe, "stream, fp32 index"))
            _assert_same((gi[0], gd[0]), (want[0][:nb * 32], want[1][:nb * 32]), (dim, k, nprobe, "stream, oracle"))


@pytest.mark.parametrize("dim", [20, 2048])
def test_inner_product(gpu_pkg, dim):
    """Signed integer rows, exact products; queries orthogonal to rows (and a zero query) score -0.0 on the device."""
    if dim == 20:
        vr, cents, off, r2o, q, _ = D.zeros_index()
        zero_q = D.ZERO_QUERIES
    else:
        vr, cents, off, r2o, q = D.signed_index(dim)
        q = np.array(q)
        q[3] = 0
        zero_q = (3,)
    with _open_f16(gpu_pkg, vr, cents, off, r2o) as ivf:
        for k, nprobe in ((5, 4), (16, NLIST)):
            want = oracle.ivf_search(vr, off, r2o, cents, q, k, nprobe, metric=1)
            _assert_same(ivf.search_metric(q, k, nprobe, IP), _host_form(want), (dim, k, nprobe, "host"))
            got = _dev(ivf, q, 2, 32, k, nprobe, IP)
            _assert_same(got, (want[0][:64], want[1][:64]), (dim, k, nprobe, "device"))
            for i in zero_q:
                assert np.all(bits(got[1][i]).view(np.uint32) == 0x80000000), (dim, k, nprobe, i)


def test_refusals_and_save_load(gpu_pkg, tmp_path):
    import torch
    L = gpu_pkg.lib()
    vr, cents, off, r2o, q = _int_index(100)
    q = np.array(q[:40])
    with _open_f16(gpu_pkg, vr, cents, off, r2o) as ivf:
        for call, args in ((ivf.search_topk, (q, 17, 4)), (ivf.search_metric, (q, 128, 4, IP)), (ivf.set_precision, (2,)),
                           (ivf.set_metric, (gpu_pkg.METRIC_IP,))):
            with pytest.raises(gpu_pkg.VSearchError) as e:
                call(*args)
            assert e.value.status == -5, str(e.value)
            assert call not in (ivf.search_topk, ivf.search_metric) or "half rows" in str(e.value)
        ivf.set_precision(0)
        ivf.set_precision(1)
        # the handle carries half rows, and is still no brute-force index
        qd = torch.from_numpy(q).to("cuda:0")
        gi = torch.zeros((32, 6), dtype=torch.int32, device="cuda:0")
        gd = torch.zeros((32, 6), dtype=torch.float32, device="cuda:0")
        s = torch.cuda.current_stream().cuda_stream
        assert L.vs_bf_search_dev(ivf._h, qd.data_ptr(), 32, 5, gi.data_ptr(), gd.data_ptr(), None, s) == -1
        out = (C.c_int64 * 4)(7, 7, 7, 7)
        assert L.vs_bf_one_f16_stats(ivf._h, out, 0) == -1 and L.vs_bf_filter_stats(ivf._h, out, 0) == -1
        assert L.vs_bf_f16_rows_read(ivf._h, 0, 1, np.zeros(100, dtype=np.uint16).ctypes.data_as(C.c_void_p)) == -1
        assert tuple(out) == (7, 7, 7, 7)
        ivf.save(str(tmp_path / "idx"))
        a = ivf.searchBatch(q, len(q), 5, 3)
    _assert_same(a, oracle.ivf_search(vr, off, r2o, cents, q, 5, 3), "after the refusals")
    assert np.array_equal(np.load(tmp_path / "idx" / "vectors_reordered.npy"), vr)
    with gpu_pkg.IVFIndex(str(tmp_path / "idx")) as f32:
        _assert_same(f32.searchBatch(q, len(q), 5, 3), a, "loaded fp32 index")
