"""vs_bf_create_nd_f16 / vs_bf_f16_rows_read without a GPU: the refusals in their stated order, every one before a device
is touched (on a machine without one, only a call that passes them all reports the missing device), and from_f16's dtype."""
import ctypes as C

import numpy as np
import pytest

INVALID, DEVICE, UNSUPPORTED = -1, -3, -5


def test_creator_refusals_in_order(pkg):
    L = pkg.lib()
    h = C.c_void_p(None)
    p = np.zeros((8, 40), dtype=np.float16).ctypes.data_as(C.c_void_p)

    def create(base=p, n=8, dim=40, metric=0, device=0, id_offset=0, out=C.byref(h)):
        return L.vs_bf_create_nd_f16(base, n, dim, metric, device, id_offset, out)

    # each call breaks one rule and every rule after it: the first broken rule answers
    assert create(base=None, dim=0, metric=7, id_offset=2 ** 31) == INVALID and b"bad arguments" in L.vs_last_error()
    assert create(n=0, dim=4096) == INVALID and b"bad arguments" in L.vs_last_error()
    assert create(out=None) == INVALID
    assert create(dim=0, metric=7, id_offset=2 ** 31) == INVALID and b"at least 1" in L.vs_last_error()
    assert create(dim=2049, metric=7, id_offset=2 ** 31) == UNSUPPORTED and b"2048" in L.vs_last_error()
    assert create(metric=7, id_offset=2 ** 31) == INVALID and b"metric" in L.vs_last_error()
    assert create(id_offset=2 ** 31 - 8) == UNSUPPORTED and b"int32" in L.vs_last_error()
    if pkg.device_count() == 0:  # (last of all, and the only check that asks for a device)
        assert create() == DEVICE
    assert h.value is None  # *out is written on success only


def test_from_f16_wants_float16_and_rows_read_a_handle(pkg):
    with pytest.raises(ValueError):
        pkg.BruteForceIndex.from_f16(np.zeros((8, 40), dtype=np.float32))
    with pytest.raises(ValueError):
        pkg.BruteForceIndex.from_f16(np.zeros(8, dtype=np.float16))
    dst = np.zeros((1, 40), dtype=np.uint16)
    assert pkg.lib().vs_bf_f16_rows_read(None, 0, 1, dst.ctypes.data_as(C.c_void_p)) == INVALID
