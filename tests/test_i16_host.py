"""Host-side checks of the int16 cosine path (vs_i16_*): symbols, argument order, the quantiser and the .bin writer.
No GPU needed.  The reference is numpy, written out here from the contract in include/vsearch.h."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NAMES = ("vs_i16_quantize", "vs_i16_write_bin", "vs_i16_create", "vs_i16_destroy", "vs_i16_num_docs", "vs_i16_dim",
         "vs_i16_batch", "vs_i16_scale", "vs_i16_rows_read", "vs_i16_execute_dev", "vs_i16_execute", "vs_i16_search_dev",
         "vs_i16_search")
DIMS = [1, 7, 8, 9, 127, 128, 129, 136, 257, 960, 2047, 2048]
SCALES = [1000.0, 2047.0]
f32 = np.float32


def test_symbols_are_declared_exported_and_bound(pkg):
    hdr = open(os.path.join(ROOT, "include", "vsearch.h")).read()
    declared = set(re.findall(r"VS_API\s+[\w\s\*]+?\b(vs_\w+)\s*\(", hdr))
    for name in NAMES:
        assert name in declared
        assert name in pkg.exported_symbols()
        assert hasattr(pkg.lib(), name)
    assert hasattr(pkg, "I16Runner") and hasattr(pkg, "i16_quantize") and hasattr(pkg, "i16_write_bin")
    hpp = open(os.path.join(ROOT, "include", "vsearch.hpp")).read()
    assert "class I16Runner" in hpp


def test_create_check_order(pkg):
    """Null pointers, dim, ids and scale are refused before the device is looked for, in that order."""
    L = pkg.lib()
    h = C.c_void_p(None)
    base = np.zeros((8, 64), dtype=np.float32)
    bp = base.ctypes.data_as(C.c_void_p)
    nan, inf = float("nan"), float("inf")
    assert L.vs_i16_create(None, 8, 64, 1000.0, 0, 0, C.byref(h)) == -1           # null base
    assert L.vs_i16_create(bp, 8, 64, 1000.0, 0, 0, None) == -1                   # null out pointer
    assert L.vs_i16_create(bp, 0, 64, 1000.0, 0, 0, C.byref(h)) == -1             # no rows
    assert L.vs_i16_create(None, 8, 2049, 1000.0, 0, 0, C.byref(h)) == -1         # null before dim
    assert L.vs_i16_create(bp, 8, 0, 1000.0, 0, 0, C.byref(h)) == -1              # dim < 1
    assert L.vs_i16_create(bp, 8, 2049, 1000.0, 0, 0, C.byref(h)) == -5           # dim > 2048
    assert L.vs_i16_create(bp, 8, 2049, nan, 0, -1, C.byref(h)) == -5             # dim before ids and scale
    assert L.vs_i16_create(bp, 8, 64, 1000.0, 0, 2 ** 31 - 8, C.byref(h)) == -5   # ids do not fit
    assert L.vs_i16_create(bp, 8, 64, 1000.0, 0, -1, C.byref(h)) == -5
    assert L.vs_i16_create(bp, 8, 0, 0.0, 0, -1, C.byref(h)) == -1                # dim < 1 before ids
    assert L.vs_i16_create(bp, 8, 64, 0.5, 0, -1, C.byref(h)) == -5               # ids before scale
    for s in (nan, inf, -inf, 0.0, 0.999, 2047.5, -1000.0):
        assert L.vs_i16_create(bp, 8, 64, s, 0, 0, C.byref(h)) == -1              # no device needed for this one
    assert h.value is None


def test_create_needs_a_device(pkg):
    L = pkg.lib()
    h = C.c_void_p(None)
    base = np.ones((8, 64), dtype=np.float32)
    bp = base.ctypes.data_as(C.c_void_p)
    if pkg.device_count() == 0:
        for s in (1.0, 1000.0, 2047.0):
            assert L.vs_i16_create(bp, 8, 64, s, 0, 0, C.byref(h)) == -3  # every host check passed: only the device is missing
        assert h.value is None
        with pytest.raises(pkg.VSearchError) as e:
            pkg.I16Runner(base)
        assert e.value.status == -3
    else:
        with pkg.I16Runner(base) as r:
            assert (r.getNumDocs(), r.getDim(), r.getBatchSize(), r.getScale()) == (8, 64, 32, 1000.0)


def test_null_handles_and_bad_arguments(pkg):
    L = pkg.lib()
    x = np.ones((2, 4), dtype=np.float32)
    p = x.ctypes.data_as(C.c_void_p)
    assert L.vs_i16_num_docs(None) == 0 and L.vs_i16_dim(None) == 0 and L.vs_i16_batch(None) == 0 and L.vs_i16_scale(None) == 0.0
    L.vs_i16_destroy(None)
    assert L.vs_i16_execute(None, p, 1, p) == -1 and L.vs_i16_execute_dev(None, p, 1, p, 8, None) == -1
    assert L.vs_i16_search(None, p, 1, 5, p, p) == -1 and L.vs_i16_search_dev(None, p, 1, 1, 5, p, p, None) == -1
    assert L.vs_i16_rows_read(None, 0, 1, p) == -1
    out = np.zeros((2, 4), dtype=np.int16)
    op = out.ctypes.data_as(C.c_void_p)
    assert L.vs_i16_quantize(None, 2, 4, 1000.0, op) == -1 and L.vs_i16_quantize(p, 2, 4, 1000.0, None) == -1
    assert L.vs_i16_quantize(p, -1, 4, 1000.0, op) == -1
    assert L.vs_i16_quantize(p, 2, 0, 1000.0, op) == -1 and L.vs_i16_quantize(p, 2, 2049, 1000.0, op) == -1
    for s in (float("nan"), float("inf"), 0.5, 2048.0):
        assert L.vs_i16_quantize(p, 2, 4, s, op) == -1
    assert L.vs_i16_quantize(p, 0, 4, 1000.0, op) == 0
    assert L.vs_i16_write_bin(None, p, 2, 4, 1000.0, 32) == -1 and L.vs_i16_write_bin(b"/nonexistent-dir/x.bin", p, 2, 4, 1000.0, 32) == -2
    assert L.vs_i16_write_bin(b"x.bin", p, 2, 4, 1000.0, 0) == -1


# ---- the contract's P(s, n) and quantiser, vectorised over rows
def pairwise(s):
    """numpy's pairwise order on the last axis of a float32 array, every sum rounded to float32."""
    n = s.shape[1]
    if n < 8:
        res = np.zeros(s.shape[0], f32)
        for i in range(n):
            res = res + s[:, i]
        return res
    if n <= 128:
        r = s[:, :8].copy()
        i = 8
        while i + 8 <= n:
            r = r + s[:, i:i + 8]
            i += 8
        res = ((r[:, 0] + r[:, 1]) + (r[:, 2] + r[:, 3])) + ((r[:, 4] + r[:, 5]) + (r[:, 6] + r[:, 7]))
        for j in range(i, n):
            res = res + s[:, j]
        return res
    n2 = (n // 2) & ~7
    return pairwise(s[:, :n2]) + pairwise(s[:, n2:])


def quant_contract(x, scale):
    with np.errstate(all="ignore"):
        S = pairwise(x * x)
        assert S.dtype == f32
        den = np.sqrt(S) + f32(1e-8)
        v = (x / den[:, None]) * f32(scale)
        assert v.dtype == f32
        return np.where(np.isnan(v), f32(0), np.trunc(v)).astype(np.int16)


def quant_one_line(x, scale):
    return ((x / (np.linalg.norm(x, axis=1, keepdims=True) + 1e-8)) * f32(scale)).astype(np.int16)


def finite_rows(dim, seed):
    """Gaussian rows of many magnitudes, integer-valued SIFT-like rows, a zero row, a row of denormals."""
    rng = np.random.default_rng(seed)
    g = (rng.standard_normal((120, dim)) * 10.0 ** rng.uniform(-6, 6, size=(120, 1))).astype(f32)
    sift = np.floor(np.abs(rng.standard_normal((60, dim))) * 40.0).clip(0, 218).astype(f32)
    zero = np.zeros((1, dim), f32)
    den = np.full((1, dim), 1e-42, f32)
    den[0, ::3] = -3e-41
    return np.concatenate([g, sift, zero, den])


@pytest.mark.parametrize("scale", SCALES)
@pytest.mark.parametrize("dim", DIMS)
def test_quantize_against_numpy(pkg, dim, scale):
    x = finite_rows(dim, 7 * dim + int(scale))
    got = pkg.i16_quantize(x, scale)
    assert got.dtype == np.int16 and got.shape == x.shape
    assert np.array_equal(got, quant_contract(x, scale))
    assert np.array_equal(got, quant_one_line(x, scale))
    g = got.astype(np.int64)
    assert np.abs(g).max() <= scale
    assert ((g * g).sum(1) <= scale * scale + 1).all()
    assert not got[-2].any()                      # the zero row stays zero
    assert g[:120].any(axis=1).all()              # ... and no gaussian row collapses
    if dim >= 8:
        assert np.abs(g[:120]).max() > scale / (2 * np.sqrt(dim))


@pytest.mark.parametrize("scale", SCALES)
@pytest.mark.parametrize("dim", DIMS)
def test_quantize_non_finite_rows(pkg, dim, scale):
    rng = np.random.default_rng(dim)
    x = rng.standard_normal((6, dim)).astype(f32)
    x[0, dim // 2] = np.nan
    x[1, dim // 3] = 1e30        # its square overflows: the norm is infinite
    x[2, 0] = np.inf
    x[3, dim - 1] = -np.inf
    x[4] *= f32(1e-30)           # squares underflow to denormals or 0; den stays near 1e-8
    got = pkg.i16_quantize(x, scale)
    assert np.array_equal(got, quant_contract(x, scale))
    assert not got[:4].any()     # NaN, overflow and infinities: all zeros
    assert np.array_equal(got[5], quant_one_line(x[5:6], scale)[0])


@pytest.mark.parametrize("mult", [32, 256])
def test_write_bin(pkg, tmp_path, mult):
    """A.bin / B.bin of preprocess.py:33-42: the padded array's tofile()."""
    for dim, rows in ((128, 100), (9, 160), (257, 1)):
        x = finite_rows(dim, dim)[:rows]
        assert len(x) == rows
        path = str(tmp_path / f"m{mult}_{dim}.bin")
        pkg.i16_write_bin(path, x, 1000.0, mult)
        want = quant_one_line(x, 1000.0)
        pad = (-rows) % mult
        want = np.pad(want, ((0, pad), (0, 0)))
        assert want.shape[0] % mult == 0
        assert open(path, "rb").read() == want.astype("<i2").tobytes()
