"""Host-side checks of the float16 IVF creator (vs_ivf_create_nd_f16): no GPU needed.  The refusals that need no device
come in vs_ivf_create_nd_u8's order -- null pointers / counts, dim < 1, dim > 2048, offsets -- and leave `out` untouched."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_symbol_is_declared_and_bound(pkg):
    hdr = open(os.path.join(ROOT, "include", "vsearch.h")).read()
    assert "vs_ivf_create_nd_f16" in re.findall(r"VS_API\s+[\w\s\*]+?\b(vs_\w+)\s*\(", hdr)
    assert "vs_ivf_create_nd_f16" in pkg.exported_symbols()
    assert hasattr(pkg.lib(), "vs_ivf_create_nd_f16")


def test_device_free_refusals_in_order(pkg):
    L = pkg.lib()
    n, dim, nlist = 8, 300, 2
    rows = np.zeros((n, dim), dtype=np.float16)
    cents = np.zeros((nlist, dim), dtype=np.float32)
    off = np.array([0, 3, n], dtype=np.int32)
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    h = C.c_void_p(None)

    def create(rows_, n_rows, d, cents_, nl, off_, out=C.byref(h)):
        return L.vs_ivf_create_nd_f16(p(rows_), n_rows, d, p(cents_), nl, p(off_), None, 0, out)

    bad_offsets = [np.array(o, dtype=np.int32) for o in ([0, 3, n - 1], [1, 3, n], [0, n + 1, n])]  # cover, start, monotone
    # 1. null pointers and counts, whatever the dimension and the offsets
    for d, o in ((dim, off), (2049, bad_offsets[0]), (0, off)):
        assert create(None, n, d, cents, nlist, o) == -1
        assert create(rows, n, d, None, nlist, o) == -1
        assert create(rows, n, d, cents, nlist, None) == -1
        assert create(rows, n, d, cents, nlist, o, None) == -1
        assert create(rows, 0, d, cents, nlist, o) == -1
        assert create(rows, n, d, cents, 0, o) == -1
    # 2. dim < 1 and 3. dim > 2048, before the offsets are looked at
    for o in [off] + bad_offsets:
        assert create(rows, n, 0, cents, nlist, o) == -1 and b"dim" in L.vs_last_error()
        assert create(rows, n, -3, cents, nlist, o) == -1 and b"dim" in L.vs_last_error()
        assert create(rows, n, 2049, cents, nlist, o) == -5 and b"2048" in L.vs_last_error()
    # 4. the offsets, at both ends of the dimension range
    for d in (1, dim, 2048):
        for o in bad_offsets:
            assert create(rows, n, d, cents, nlist, o) == -1 and b"cluster_offsets" in L.vs_last_error()
    assert h.value is None
    if pkg.device_count() == 0:  # 5. then the device: no index, no CPU fallback
        assert create(rows, n, dim, cents, nlist, off) == -3
        assert h.value is None


def test_python_wrappers_check_dtype_and_shape(pkg):
    cents = np.zeros((2, 300), dtype=np.float32)
    off = np.array([0, 3, 8], dtype=np.int32)
    for bad in (np.zeros((8, 300), dtype=np.float32), np.zeros((8, 300), dtype=np.uint16), np.zeros(300, dtype=np.float16)):
        with pytest.raises(ValueError):
            pkg.IVFIndex.from_f16(bad, cents, off, None)
    for bad in (np.zeros((8, 300), dtype=np.float32), np.zeros(300, dtype=np.float16)):
        with pytest.raises(ValueError):
            pkg.IVFIndex.build_f16(bad, 2)
