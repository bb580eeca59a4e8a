"""Host-side checks of the general-dimension UFIXED_POINT_8 creator (vs_q8_create_nd): no GPU needed."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_create_nd_is_declared_exported_and_bound(pkg):
    hdr = open(os.path.join(ROOT, "include", "vsearch.h")).read()
    declared = set(re.findall(r"VS_API\s+[\w\s\*]+?\b(vs_\w+)\s*\(", hdr))
    assert "vs_q8_create_nd" in declared
    assert "vs_q8_create_nd" in pkg.exported_symbols()
    assert hasattr(pkg.lib(), "vs_q8_create_nd")


def test_create_nd_check_order(pkg):
    """Null pointers, dim, ids and encodings are refused before the device is looked for, in that order."""
    L = pkg.lib()
    h = C.c_void_p(None)
    base = np.zeros((8, 64), dtype=np.float32)
    bp = base.ctypes.data_as(C.c_void_p)
    bad = pkg.Q8Encodings(1.0, 1.0, 3, 1.0)  # weight_offset > 0
    assert L.vs_q8_create_nd(None, 8, 64, None, 0, 0, C.byref(h)) == -1          # null base
    assert L.vs_q8_create_nd(bp, 8, 64, None, 0, 0, None) == -1                  # null out pointer
    assert L.vs_q8_create_nd(bp, 0, 64, None, 0, 0, C.byref(h)) == -1            # no rows
    assert L.vs_q8_create_nd(None, 8, 2049, None, 0, 0, C.byref(h)) == -1        # null before dim
    assert L.vs_q8_create_nd(bp, 8, 0, None, 0, 0, C.byref(h)) == -1             # dim < 1
    assert L.vs_q8_create_nd(bp, 8, -3, C.byref(bad), 0, 0, C.byref(h)) == -1
    assert L.vs_q8_create_nd(bp, 8, 2049, None, 0, 0, C.byref(h)) == -5          # dim > 2048
    assert L.vs_q8_create_nd(bp, 8, 2049, C.byref(bad), 0, 0, C.byref(h)) == -5  # dim before encodings
    assert L.vs_q8_create_nd(bp, 8, 64, C.byref(bad), 0, 2 ** 31 - 8, C.byref(h)) == -5  # ids before encodings
    assert L.vs_q8_create_nd(bp, 8, 64, None, 0, -1, C.byref(h)) == -5
    assert L.vs_q8_create_nd(bp, 8, 64, C.byref(bad), 0, 0, C.byref(h)) == -1    # no device needed for this one
    for e in (pkg.Q8Encodings(0.0, 1.0, 0, 1.0), pkg.Q8Encodings(1.0, float("nan"), 0, 1.0), pkg.Q8Encodings(1.0, 1.0, 0, -2.0),
              pkg.Q8Encodings(1.0, 1.0, -256, 1.0)):
        assert L.vs_q8_create_nd(bp, 8, 64, C.byref(e), 0, 0, C.byref(h)) == -1
    assert h.value is None


def test_create_nd_needs_a_device(pkg):
    L = pkg.lib()
    h = C.c_void_p(None)
    base = np.zeros((8, 64), dtype=np.float32)
    bp = base.ctypes.data_as(C.c_void_p)
    if pkg.device_count() == 0:
        good = pkg.Q8Encodings(1.0, 1.0, -3, 1.0)
        assert L.vs_q8_create_nd(bp, 8, 64, None, 0, 0, C.byref(h)) == -3  # every host check passed: only the device is missing
        assert L.vs_q8_create_nd(bp, 8, 64, C.byref(good), 0, 0, C.byref(h)) == -3
        with pytest.raises(pkg.VSearchError) as e:
            pkg.Q8Runner(np.zeros((8, 64)))
        assert e.value.status == -3
    else:
        with pkg.Q8Runner(np.zeros((8, 64))) as r:
            assert (r.getNumDocs(), r.getDim(), r.getBatchSize()) == (8, 64, 32)


def test_create_keeps_refusing_other_dimensions(pkg):
    L = pkg.lib()
    h = C.c_void_p(None)
    base = np.zeros((8, 64), dtype=np.float32)
    assert L.vs_q8_create(base.ctypes.data_as(C.c_void_p), 8, 64, None, 0, 0, C.byref(h)) == -5
    assert h.value is None
