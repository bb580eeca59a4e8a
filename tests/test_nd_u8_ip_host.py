"""Host-side checks of the uint8 creator under a metric (vs_bf_create_nd_u8_metric) and of the data the GPU tests of
test_gpu_nd_u8_ip.py run on: no GPU needed."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import nd_u8_ip_data as D
from nd_u8_data import sqnorm_max

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
L2, IP = 0, 1


def test_new_symbol_is_declared_exported_and_bound(pkg):
    hdr = open(os.path.join(ROOT, "include", "vsearch.h")).read()
    declared = set(re.findall(r"VS_API\s+[\w\s\*]+?\b(vs_\w+)\s*\(", hdr))
    name = "vs_bf_create_nd_u8_metric"
    assert name in declared
    assert name in pkg.exported_symbols()
    fn = getattr(pkg.lib(), name)
    assert len(fn.argtypes) == 7 and fn.restype is C.c_int32
    assert (pkg.METRIC_L2, pkg.METRIC_IP) == (L2, IP)


def test_argument_validation_in_the_stated_order(pkg):
    L = pkg.lib()
    create = L.vs_bf_create_nd_u8_metric
    base = np.zeros((8, 300), dtype=np.uint8)
    bp = base.ctypes.data_as(C.c_void_p)
    h = C.c_void_p(None)
    out = C.byref(h)
    for metric in (L2, IP, 2, -1):
        # 1: null pointers, no rows -- before anything else
        assert create(None, 8, 0, metric, 0, 0, out) == -1
        assert create(bp, 8, 2049, metric, 0, 0, None) == -1
        assert create(bp, 0, 2049, metric, 0, 0, out) == -1
        assert create(bp, -4, 300, metric, 0, 0, out) == -1
        # 2, 3: the dimension, before the metric
        assert create(bp, 8, 0, metric, 0, 0, out) == -1
        assert create(bp, 8, -3, metric, 0, 0, out) == -1
        assert create(bp, 8, 2049, metric, 0, 0, out) == -5
        assert b"2048" in L.vs_last_error()
    # 4: the metric, only after the dimension checks and before the id check
    for metric in (2, -1):
        assert create(bp, 8, 300, metric, 0, 0, out) == -1
        assert b"metric" in L.vs_last_error()
        assert create(bp, 8, 128, metric, 0, 2 ** 31, out) == -1
    # 5: ids that do not fit int32, before the device is looked at
    for metric in (L2, IP):
        for dim in (300, 128):
            assert create(bp, 8, dim, metric, 0, 2 ** 31 - 8, out) == -5
            assert b"int32" in L.vs_last_error()
    assert h.value is None
    # 6: the device
    if pkg.device_count() == 0:
        for metric in (L2, IP):
            for dim in (300, 128):
                assert create(bp, 8, dim, metric, 0, 0, out) == -3  # no device: no index, no CPU fallback
        assert h.value is None


def test_from_u8_takes_uint8_only_and_keeps_its_positions(pkg):
    import inspect
    with pytest.raises(ValueError):
        pkg.BruteForceIndex.from_u8(np.zeros((8, 300), dtype=np.float32))
    with pytest.raises(ValueError):
        pkg.BruteForceIndex.from_u8(np.zeros((8, 300), dtype=np.float32), metric=pkg.METRIC_IP)
    sig = inspect.signature(pkg.BruteForceIndex.from_u8)
    assert list(sig.parameters) == ["base_u8", "device", "id_offset", "metric"]
    assert sig.parameters["metric"].default == pkg.METRIC_L2


@pytest.mark.parametrize("dim", [1, 3, 63, 64, 65, 100, 128, 129, 192, 320, 960, 2048])
def test_planted_edges_exist(dim):
    """What test_gpu_nd_u8_ip.py relies on: byte values with both int8 extremes, every squared norm under 2^23, the zero
    query, the zero rows, the zero products of the disjoint supports, and equal scores among the best where claimed."""
    n = 20000 if dim <= 320 else 3000
    rng = np.random.default_rng(7000 + dim)
    base, q = D.ip_data(rng, n, 70, dim)
    assert base.dtype == np.uint8 and q.dtype == np.uint8
    assert base.min() == 0 and base.max() == 255 and q.max() == 255
    assert sqnorm_max(base) < 2 ** 23 and sqnorm_max(q) < 2 ** 23
    assert not q[D.ZERO_Q].any()
    for r in D.zero_rows(n):
        assert not base[r].any()
    ip = D.ip_int64(q, base)
    assert ip.dtype == np.int64 and ip.min() == 0 and ip.max() < 2 ** 23
    for j in D.ORTH_Q:
        assert q[j].any()
        for r in D.orth_rows(n):
            assert ip[j, r] == 0
            assert dim == 1 or base[r].any()
    ids, d = D.topk_ref(ip, 16)
    flags = D.tie_flags(d[:, :2])
    for j in D.TIE_Q:
        assert flags[j] == 1, "the two best of a tie query are equal"
    assert np.array_equal(ids[D.ZERO_Q], np.arange(16)) and not d[D.ZERO_Q].any()
    assert np.signbit(d[D.ZERO_Q]).all(), "-(float32)(0) is -0.0"
    assert D.tie_flags(d)[D.ZERO_Q] == 1
    hi, hs = D.host_view(ids, d, 5)
    assert (hs[:, 1:] <= hs[:, :-1]).all() and not np.signbit(hs[D.ZERO_Q]).any()


def test_reference_ranks_by_score_then_id():
    ip = np.array([[3, 9, 9, 0, 9, 1], [0, 0, 0, 0, 0, 0]], dtype=np.int64)
    ids, d = D.topk_ref(ip, 4)
    assert ids.tolist() == [[1, 2, 4, 0], [0, 1, 2, 3]]
    assert d[0].tolist() == [-9.0, -9.0, -9.0, -3.0] and np.signbit(d[1]).all()
    ids, d = D.topk_ref(ip, 8, id_offset=10)
    assert ids[0].tolist() == [11, 12, 14, 10, 15, 13, -1, -1] and np.isinf(d[0, 6:]).all()
    assert D.tie_flags(d).tolist() == [1, 1]


@pytest.mark.parametrize("dim", [2, 100, 128])
def test_small_base_shows_zero_products(dim):
    base, q = D.small_orth_base(np.random.default_rng(7100 + dim), dim)
    ip = D.ip_int64(q, base)
    assert len(base) <= 16
    for j in D.ORTH_Q:
        assert sorted(np.flatnonzero(ip[j] == 0).tolist()) == [1, 2, 4, len(base) - 1]
    assert not ip[D.ZERO_Q].any()
    assert (ip[0] > 0).sum() == len(base) - 1  # (row 2 is zero)
