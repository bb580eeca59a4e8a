"""Host-side checks of the uint8 interface (vs_bf_create_nd_u8, the .bvecs functions): no GPU needed."""
import ctypes as C
import os
import re
import struct

import numpy as np
import pytest

import nd_u8_data

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_new_symbols_are_declared_and_exported(pkg):
    hdr = open(os.path.join(ROOT, "include", "vsearch.h")).read()
    declared = set(re.findall(r"VS_API\s+[\w\s\*]+?\b(vs_\w+)\s*\(", hdr))
    for name in ("vs_bf_create_nd_u8", "vs_bvecs_shape", "vs_bvecs_read", "vs_bvecs_write"):
        assert name in declared
        assert name in pkg.exported_symbols()
        assert hasattr(pkg.lib(), name)


@pytest.mark.parametrize("dim", [1, 100, 2048])
def test_bvecs_round_trip(pkg, tmp_path, dim):
    rng = np.random.default_rng(dim)
    a = rng.integers(0, 256, size=(7, dim)).astype(np.uint8)
    a[0, 0], a[6, dim - 1] = 0, 255
    path = str(tmp_path / "a.bvecs")
    pkg.write_bvecs(path, a)
    assert os.path.getsize(path) == 7 * (4 + dim)
    raw = open(path, "rb").read()
    assert struct.unpack_from("<i", raw, 0)[0] == dim and struct.unpack_from("<i", raw, 4 + dim)[0] == dim
    assert raw[4:4 + dim] == a[0].tobytes()
    rows, d = C.c_int64(0), C.c_int(0)
    assert pkg.lib().vs_bvecs_shape(path.encode(), C.byref(rows), C.byref(d)) == 0
    assert (rows.value, d.value) == (7, dim)
    b = pkg.read_bvecs(path)
    assert b.dtype == np.uint8 and np.array_equal(a, b)


def test_bvecs_errors(pkg, tmp_path):
    L = pkg.lib()
    a = np.arange(5 * 100, dtype=np.int64).reshape(5, 100).astype(np.uint8)
    path = str(tmp_path / "a.bvecs")
    pkg.write_bvecs(path, a)
    rows, d = C.c_int64(0), C.c_int(0)
    dst = np.zeros(5 * 100, dtype=np.uint8)
    # cap_elems too small
    assert L.vs_bvecs_read(path.encode(), dst.ctypes.data_as(C.c_void_p), 5 * 100 - 1, C.byref(rows), C.byref(d)) == -1
    assert L.vs_bvecs_read(path.encode(), dst.ctypes.data_as(C.c_void_p), 5 * 100, C.byref(rows), C.byref(d)) == 0
    assert np.array_equal(dst.reshape(5, 100), a)
    # a record whose d differs from the first
    raw = bytearray(open(path, "rb").read())
    struct.pack_into("<i", raw, 2 * 104, 99)
    bad = str(tmp_path / "bad.bvecs")
    open(bad, "wb").write(raw)
    with pytest.raises(pkg.VSearchError) as e:
        pkg.read_bvecs(bad)
    assert e.value.status == -2 and "Inconsistent" in str(e.value)
    # truncated
    with open(path, "ab") as f:
        f.write(b"\x64\x00\x00\x00\x01\x02")
    with pytest.raises(pkg.VSearchError) as e:
        pkg.read_bvecs(path)
    assert e.value.status == -2 and "truncated" in str(e.value)
    assert L.vs_bvecs_shape(path.encode(), C.byref(rows), C.byref(d)) == -2
    with pytest.raises(pkg.VSearchError) as e:
        pkg.read_bvecs(str(tmp_path / "missing.bvecs"))
    assert e.value.status == -2 and "Cannot open" in str(e.value)
    # empty file: zero rows, as the .fvecs reader
    pe = str(tmp_path / "empty.bvecs")
    open(pe, "wb").close()
    assert pkg.read_bvecs(pe).shape[0] == 0


def test_create_nd_u8_argument_validation(pkg):
    L = pkg.lib()
    base = np.zeros((8, 300), dtype=np.uint8)
    bp = base.ctypes.data_as(C.c_void_p)
    h = C.c_void_p(None)
    assert L.vs_bf_create_nd_u8(bp, 8, 0, 0, 0, C.byref(h)) == -1      # dim < 1
    assert L.vs_bf_create_nd_u8(bp, 8, -3, 0, 0, C.byref(h)) == -1
    assert L.vs_bf_create_nd_u8(bp, 8, 2049, 0, 0, C.byref(h)) == -5   # dim > 2048
    assert L.vs_bf_create_nd_u8(None, 8, 300, 0, 0, C.byref(h)) == -1  # null base
    assert L.vs_bf_create_nd_u8(bp, 8, 300, 0, 0, None) == -1          # null out pointer
    assert L.vs_bf_create_nd_u8(bp, 0, 300, 0, 0, C.byref(h)) == -1    # no rows
    assert h.value is None
    with pytest.raises(ValueError):
        pkg.BruteForceIndex.from_u8(np.zeros((8, 300), dtype=np.float32))
    if pkg.device_count() == 0:
        assert L.vs_bf_create_nd_u8(bp, 8, 300, 0, 0, C.byref(h)) == -3  # no device: no index, no CPU fallback
        assert L.vs_bf_create_nd_u8(bp, 8, 128, 0, 0, C.byref(h)) == -3


@pytest.mark.parametrize("dim", [1, 3, 63, 64, 65, 100, 129, 192, 320, 768, 960, 1024, 2048])
def test_test_data_keeps_the_reference_exact(dim):
    """The GPU tests' inputs: byte valued, both int8 extremes present, every squared norm under 2^23 (so that
    ||q||^2 + ||b||^2 < 2^24 and oracle.search_bf is exact), ties planted."""
    rng = np.random.default_rng(1000 + dim)
    base, q = nd_u8_data.u8_data(rng, 20000, 70, dim)
    assert base.dtype == np.uint8 and q.dtype == np.uint8
    assert base.min() == 0 and base.max() == 255 and q.max() == 255
    assert nd_u8_data.sqnorm_max(base) < 2 ** 23 and nd_u8_data.sqnorm_max(q) < 2 ** 23
    assert np.array_equal(q[0], base[np.flatnonzero((base == q[0]).all(1))[0]])
    assert len(np.flatnonzero((base == q[0]).all(1))) >= 2
