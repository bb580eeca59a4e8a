"""Host-side checks of the general-dimension brute-force interface (vs_bf_create_nd): no GPU needed."""
import ctypes as C

import numpy as np


def test_create_nd_is_exported(pkg):
    assert "vs_bf_create_nd" in pkg.exported_symbols()
    assert hasattr(pkg.lib(), "vs_bf_create_nd")


def test_create_nd_argument_validation(pkg):
    L = pkg.lib()
    h = C.c_void_p(None)
    base = np.zeros((8, 2049), dtype=np.float32)
    bp = base.ctypes.data_as(C.c_void_p)
    assert L.vs_bf_create_nd(bp, 8, 0, 0, 0, 0, C.byref(h)) == -1      # dim < 1
    assert L.vs_bf_create_nd(bp, 8, -3, 0, 0, 0, C.byref(h)) == -1
    assert L.vs_bf_create_nd(bp, 8, 2049, 0, 0, 0, C.byref(h)) == -5   # dim > 2048
    assert L.vs_bf_create_nd(None, 8, 300, 0, 0, 0, C.byref(h)) == -1  # null base
    assert L.vs_bf_create_nd(bp, 8, 300, 0, 0, 0, None) == -1          # null out pointer
    assert L.vs_bf_create_nd(bp, 8, 300, 7, 0, 0, C.byref(h)) == -1    # unknown metric
    assert L.vs_bf_create(bp, 8, 64, 0, 0, 0, C.byref(h)) == -5        # vs_bf_create keeps refusing dim != 128
    if pkg.device_count() == 0:
        assert L.vs_bf_create_nd(bp, 8, 300, 0, 0, 0, C.byref(h)) == -3  # no device: no index, no CPU fallback
        assert L.vs_bf_create_nd(bp, 8, 128, 0, 0, 0, C.byref(h)) == -3


def test_fvecs_round_trip_at_dim_300(pkg, tmp_path):
    rng = np.random.default_rng(3)
    a = rng.normal(0, 1, size=(17, 300)).astype(np.float32)
    path = str(tmp_path / "a.fvecs")
    pkg.write_fvecs(path, a)
    b = pkg.read_fvecs(path)
    assert b.shape == (17, 300) and np.array_equal(a, b)


def test_synth_sift_any_dimension(pkg):
    a = pkg.synth_sift(50, seed=3, dim=960)
    assert a.shape == (50, 960) and a.dtype == np.float32
    assert np.array_equal(a, pkg.synth_sift(50, seed=3, dim=960))
    assert np.array_equal(a[10:20], pkg.synth_sift(10, seed=3, dim=960, row_begin=10))
    assert np.array_equal(a, np.floor(a)) and a.min() >= 0 and a.max() <= 255


def test_synth_sift_128_unchanged(pkg):
    """Values of the build before vs_bf_create_nd existed (seed 3, 7 rows): the benchmark's data must not move."""
    a = pkg.synth_sift(7, seed=3)
    assert a.shape == (7, 128)
    assert a[0, :6].tolist() == [0.0, 27.0, 26.0, 13.0, 61.0, 48.0]
    assert a[1, :6].tolist() == [25.0, 13.0, 83.0, 9.0, 12.0, 12.0]
    assert a[6, 120:].tolist() == [63.0, 24.0, 0.0, 60.0, 0.0, 24.0, 15.0, 123.0]
    assert float(a.sum()) == 31146.0
