"""Host-side checks of the uint8 IVF creator (vs_ivf_create_nd_u8, vs_ivf_nd_u8_stats): no GPU needed.  The refusals that
need no device come in vs_ivf_create's order -- null pointers / counts, dim < 1, dim > 2048, offsets -- and leave `out`
untouched."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_new_symbols_are_declared_and_exported(pkg):
    hdr = open(os.path.join(ROOT, "include", "vsearch.h")).read()
    declared = set(re.findall(r"VS_API\s+[\w\s\*]+?\b(vs_\w+)\s*\(", hdr))
    for name in ("vs_ivf_create_nd_u8", "vs_ivf_nd_u8_stats"):
        assert name in declared
        assert name in pkg.exported_symbols()
        assert hasattr(pkg.lib(), name)


def test_create_argument_validation_in_order(pkg):
    L = pkg.lib()
    n, dim, nlist = 8, 300, 2
    rows = np.zeros((n, dim), dtype=np.uint8)
    cents = np.zeros((nlist, dim), dtype=np.float32)
    off = np.array([0, 3, n], dtype=np.int32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    h = C.c_void_p(None)

    def create(rows_p, n_rows, d, cents_p, nl, off_p, out=C.byref(h)):
        return L.vs_ivf_create_nd_u8(rows_p, n_rows, d, cents_p, nl, off_p, None, 0, out)

    assert create(p(rows), n, 0, p(cents), nlist, p(off)) == -1  # dim < 1
    assert create(p(rows), n, -3, p(cents), nlist, p(off)) == -1
    assert create(p(rows), n, 2049, p(cents), nlist, p(off)) == -5  # dim > 2048
    assert b"2048" in L.vs_last_error()
    # null pointers and counts
    assert create(None, n, dim, p(cents), nlist, p(off)) == -1
    assert create(p(rows), n, dim, None, nlist, p(off)) == -1
    assert create(p(rows), n, dim, p(cents), nlist, None) == -1
    assert create(p(rows), n, dim, p(cents), nlist, p(off), None) == -1
    assert create(p(rows), 0, dim, p(cents), nlist, p(off)) == -1
    assert create(p(rows), n, dim, p(cents), 0, p(off)) == -1
    # ... come before the dimension, the dimension before the offsets
    assert create(None, n, 2049, p(cents), nlist, p(off)) == -1
    bad_cover = np.array([0, 3, n - 1], dtype=np.int32)
    bad_start = np.array([1, 3, n], dtype=np.int32)
    not_monotone = np.array([0, n + 1, n], dtype=np.int32)
    assert create(p(rows), n, 2049, p(cents), nlist, p(bad_cover)) == -5
    assert create(p(rows), n, 0, p(cents), nlist, p(bad_cover)) == -1 and b"dim" in L.vs_last_error()
    for bad in (bad_cover, bad_start, not_monotone):
        assert create(p(rows), n, dim, p(cents), nlist, p(bad)) == -1
        assert b"cluster_offsets" in L.vs_last_error()
    assert h.value is None
    if pkg.device_count() == 0:
        assert create(p(rows), n, dim, p(cents), nlist, p(off)) == -3  # no device: no index, no CPU fallback
        assert create(np.zeros((n, 128), dtype=np.uint8).ctypes.data_as(C.c_void_p), n, 128, p(cents), nlist, p(off)) == -3
        assert h.value is None


def test_stats_refuses_a_null_handle(pkg):
    out = (C.c_int64 * 2)(7, 7)
    assert pkg.lib().vs_ivf_nd_u8_stats(None, out, 0) == -1
    assert tuple(out) == (7, 7)


def test_python_wrappers_check_the_dtype(pkg):
    cents = np.zeros((2, 300), dtype=np.float32)
    off = np.array([0, 3, 8], dtype=np.int32)
    with pytest.raises(ValueError):
        pkg.IVFIndex.from_u8(np.zeros((8, 300), dtype=np.float32), cents, off, None)
    with pytest.raises(ValueError):
        pkg.IVFIndex.from_u8(np.zeros(300, dtype=np.uint8), cents, off, None)
    with pytest.raises(ValueError):
        pkg.IVFIndex.build_u8(np.zeros((8, 300), dtype=np.float32), 2)
