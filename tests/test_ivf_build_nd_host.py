"""Host-side checks of the index builder at any dimension (vs_ivf_build_nd, vs_ivf_build_index_nd): the argument checks
run in the order include/vsearch.h states and all return before the library looks for a device, so the statuses are the
same with and without a GPU, and the outputs stay untouched."""
import ctypes as C

import numpy as np
import pytest

_P = lambda a: a.ctypes.data_as(C.c_void_p)


def _build(pkg, base, nlist, max_iter=3, tol=0.0, dim=None):
    """vs_ivf_build_nd with sentinel-filled outputs: (status, error text); asserts that nothing was written."""
    L = pkg.lib()
    base = np.ascontiguousarray(base, dtype=np.float32)
    cents = np.full((max(nlist, 1), base.shape[1]), -7.25, dtype=np.float32)
    assign = np.full(len(base), -77, dtype=np.int32)
    it = C.c_int(-55)
    rc = L.vs_ivf_build_nd(_P(base), len(base), base.shape[1] if dim is None else dim, nlist, max_iter, tol, 1, 0, _P(cents),
                           _P(assign), C.byref(it))
    assert np.all(cents == -7.25) and np.all(assign == -77) and it.value == -55
    return rc, L.vs_last_error().decode()


def _build_index(pkg, base, nlist, max_iter=3, tol=0.0, dim=None):
    L = pkg.lib()
    base = np.ascontiguousarray(base, dtype=np.float32)
    h = C.c_void_p(None)
    it = C.c_int(-55)
    rc = L.vs_ivf_build_index_nd(_P(base), len(base), base.shape[1] if dim is None else dim, nlist, max_iter, tol, 1, 0, C.byref(h),
                                 C.byref(it))
    assert h.value is None and it.value == -55
    return rc, L.vs_last_error().decode()


def _int_rows(n, dim, seed):
    return np.random.default_rng(seed).integers(0, 50, size=(n, dim)).astype(np.float32)


@pytest.mark.parametrize("call", [_build, _build_index])
@pytest.mark.parametrize("dim", [1, 100, 128, 2048])
def test_refusals_before_the_device(pkg, call, dim):
    # 200 rows: vs_ivf_clamp_nlist leaves nlist 8 alone (8 <= 200 / 10), so both entry points see the same nlist
    good = _int_rows(200, dim, dim)
    assert call(pkg, good, 8, max_iter=-1)[0] == -1
    assert call(pkg, good, 0)[0] == -1
    assert call(pkg, good, 8, dim=0)[0] == -1                      # dim < 1
    assert call(pkg, good, 8, dim=-3)[0] == -1
    rc, msg = call(pkg, good, 8, dim=2049)                         # dim > 2048 (checked before the data is read)
    assert rc == -5 and "2048" in msg
    for bad_value in (np.nan, np.inf, -np.inf):
        for tol in (0.0, 1e-4):
            base = good.copy()
            base[199, dim - 1] = bad_value
            rc, msg = call(pkg, base, 8, tol=tol)
            assert rc == -1 and msg, (bad_value, tol)
    big = good.copy()
    big[5, dim // 2] = -2.0 ** 36                                   # 200 * 2^36 > 2^43
    rc, msg = call(pkg, big, 8)
    assert rc == -1 and "2^43" in msg
    if pkg.device_count() == 0:
        big[5, dim // 2] = -2.0 ** 35                               # 200 * 2^35 < 2^43: inside the limit
        assert call(pkg, big, 8)[0] == -3 and call(pkg, good, 8)[0] == -3   # every host check passed: only the device is missing


def test_more_lists_than_rows(pkg):
    good = _int_rows(64, 100, 3)
    assert _build(pkg, good, 65)[0] == -1
    # through the index builder the clamp comes first (65 > 64 / 10 -> max(16, 0) = 16 lists): 12 rows cannot fill them
    assert _build_index(pkg, good[:12], 13)[0] == -1


def test_null_pointers(pkg):
    L = pkg.lib()
    good = _int_rows(64, 100, 4)
    cents = np.zeros((8, 100), dtype=np.float32)
    assign = np.zeros(64, dtype=np.int32)
    it = C.c_int(-55)
    h = C.c_void_p(None)
    assert L.vs_ivf_build_nd(None, 64, 100, 8, 3, 0.0, 1, 0, _P(cents), _P(assign), C.byref(it)) == -1
    assert L.vs_ivf_build_nd(_P(good), 64, 100, 8, 3, 0.0, 1, 0, None, _P(assign), C.byref(it)) == -1
    assert L.vs_ivf_build_nd(_P(good), 64, 100, 8, 3, 0.0, 1, 0, _P(cents), None, C.byref(it)) == -1
    assert L.vs_ivf_build_nd(_P(good), 0, 100, 8, 3, 0.0, 1, 0, _P(cents), _P(assign), C.byref(it)) == -1
    assert L.vs_ivf_build_index_nd(None, 64, 100, 8, 3, 0.0, 1, 0, C.byref(h), C.byref(it)) == -1
    assert L.vs_ivf_build_index_nd(_P(good), 64, 100, 8, 3, 0.0, 1, 0, None, C.byref(it)) == -1
    assert it.value == -55 and h.value is None


def test_python_wrappers_take_the_general_builder(pkg):
    """ivf_kmeans / ivf_build / IVFIndex.build at a dimension other than 128 reach vs_ivf_build_nd, not the 128-d refusal:
    without a device the status is 'no device' (-3), never 'unsupported' (-5); with one they build."""
    base = _int_rows(200, 100, 5)
    def build_index():
        ivf, _ = pkg.IVFIndex.build(base, 8, 1, 0.0, 1)
        with ivf:
            return np.empty((ivf.getNumClusters(), ivf.getDim()))

    for fn in (lambda: pkg.ivf_kmeans(base, 8, 1, 0.0, 1)[0], lambda: pkg.ivf_build(base, 8, 1, 0.0, 1)[3], build_index):
        if pkg.device_count() == 0:
            with pytest.raises(pkg.VSearchError) as e:
                fn()
            assert e.value.status == -3
        else:
            assert fn().shape == (8, 100)
