"""Host-side checks of IVF index creation at any dimension (vs_ivf_create): the argument checks run in a fixed order and
all of these return before the library looks for a device, so the statuses are the same with and without a GPU."""
import ctypes as C

import numpy as np


def _create(pkg, n, dim, nlist, offsets, world=1, alloc_dim=None):
    L = pkg.lib()
    h = C.c_void_p(None)
    d = alloc_dim or max(dim, 1)
    v = np.zeros((n, d), dtype=np.float32)
    c = np.zeros((nlist, d), dtype=np.float32)
    off = np.ascontiguousarray(offsets, dtype=np.int32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    rc = L.vs_ivf_create(p(v), n, dim, p(c), nlist, p(off), None, 0, 0, world, C.byref(h))
    assert h.value is None
    return rc, L.vs_last_error().decode()


def test_ivf_create_dimension_checks(pkg):
    off = [0, 4, 8]
    assert _create(pkg, 8, 0, 2, off)[0] == -1    # dim < 1
    assert _create(pkg, 8, -3, 2, off)[0] == -1
    rc, msg = _create(pkg, 8, 2049, 2, off)       # dim > 2048
    assert rc == -5 and "2048" in msg


def test_general_ivf_index_cannot_be_sharded(pkg):
    rc, msg = _create(pkg, 8, 300, 2, [0, 4, 8], world=2)
    assert rc == -5 and "300" in msg


def test_offsets_are_checked_at_any_dimension(pkg):
    rc, msg = _create(pkg, 8, 300, 2, [0, 4, 7])  # do not cover the rows
    assert rc == -1 and "cover" in msg
    rc, msg = _create(pkg, 8, 300, 3, [0, 6, 4, 8])
    assert rc == -1 and "monotone" in msg
    assert _create(pkg, 8, 128, 2, [0, 4, 7])[0] == -1

