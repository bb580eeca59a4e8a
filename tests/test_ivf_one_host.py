"""vs_ivf_one_plan (host only): the rule that sends a short call on a general IVF index to the two-launch route
(ivf_one_coarse_kernel + ivf_one_scan_kernel), its refusals in the header's order and its geometry."""
import ctypes as C

import pytest

NLIST_CAP = 1024  # vsearch.h at vs_ivf_one_plan: the lists the coarse launch's selection is built for
OK = dict(n_rows=6000, dim=100, nlist=24, num_cus=256, n_batches=1, B=16, k=16, nprobe=24)


def _raw(pkg, out=True, **kw):
    a = dict(OK, **kw)
    buf = (C.c_int64 * 4)(-7, -7, -7, -7)
    rc = pkg.lib().vs_ivf_one_plan(a["n_rows"], a["dim"], a["nlist"], a["num_cus"], a["n_batches"], a["B"], a["k"], a["nprobe"],
                                   buf if out else None)
    return rc, tuple(buf)


def test_refusals_in_the_stated_order(pkg):
    assert _raw(pkg, out=False)[0] == -1
    for bad in (dict(n_rows=0), dict(nlist=0), dict(num_cus=0), dict(n_batches=0), dict(B=0), dict(B=33), dict(k=0), dict(nprobe=0)):
        assert _raw(pkg, **bad)[0] == -1, bad
        assert _raw(pkg, dim=4096, **bad)[0] == -1, bad  # ... before the dimension is looked at
    assert _raw(pkg, dim=0)[0] == -1
    assert _raw(pkg, dim=0, k=200)[0] == -1     # dim < 1 before k > 128
    assert _raw(pkg, dim=2049)[0] == -5
    assert _raw(pkg, dim=2049, k=200)[0] == -5  # (either way unsupported; the message names the dimension first)
    assert b"dim" in pkg.lib().vs_last_error()
    assert _raw(pkg, k=129)[0] == -5
    assert b"k > 128" in pkg.lib().vs_last_error()
    assert _raw(pkg, k=128)[0] == 0 and _raw(pkg, dim=2048)[0] == 0 and _raw(pkg, dim=1)[0] == 0


@pytest.mark.parametrize("dim", [1, 100, 128, 768, 2048])
@pytest.mark.parametrize("n_batches,B,k,nprobe", [(1, 1, 1, 1), (1, 16, 16, 24), (3, 16, 10, 8), (2, 7, 8, 256), (1, 1, 10, 32)])
def test_short_shapes_take_the_route(pkg, dim, n_batches, B, k, nprobe):
    plan = pkg.ivf_one_plan(1_000_000, dim, NLIST_CAP, 256, n_batches, B, k, nprobe)
    assert plan[0] == 1
    assert 1 <= plan[1] <= 256 and 1 <= plan[3] <= 256
    assert plan[2] >= 64 and plan[2] % 64 == 0


def test_everything_else_keeps_the_group_route(pkg):
    n = 1_000_000
    assert pkg.ivf_one_plan(n, 100, 1024, 256, 3, 16, 16, 256)[0] == 1
    for kw in (dict(n_batches=4), dict(B=17), dict(B=32), dict(k=17), dict(k=128), dict(nlist=NLIST_CAP + 1, nprobe=8)):
        a = dict(n_rows=n, dim=100, nlist=1024, num_cus=256, n_batches=3, B=16, k=16, nprobe=256)
        a.update(kw)
        assert pkg.ivf_one_plan(**a) == (0, 0, 0, 0), kw
    # nprobe is clamped to nlist before it is compared with 256
    assert pkg.ivf_one_plan(n, 100, 1024, 256, 1, 1, 10, 257) == (0, 0, 0, 0)
    assert pkg.ivf_one_plan(n, 100, 256, 256, 1, 1, 10, 5000)[0] == 1
    assert pkg.ivf_one_plan(n, 100, 257, 256, 1, 1, 10, 5000) == (0, 0, 0, 0)
    # the kernels count rows in 32 bits
    assert pkg.ivf_one_plan(2 ** 31 - 129, 100, 1024, 256, 1, 1, 10, 8)[0] == 1
    assert pkg.ivf_one_plan(2 ** 31 - 128, 100, 1024, 256, 1, 1, 10, 8) == (0, 0, 0, 0)


@pytest.mark.parametrize("num_cus", [1, 256])
@pytest.mark.parametrize("nlist", [1, 24, 64, 65, 1000, 1024])
def test_geometry_within_bounds(pkg, num_cus, nlist):
    route, coarse, unit, scan = pkg.ivf_one_plan(6000, 100, nlist, num_cus, 1, 16, 10, 8)
    assert route == 1
    assert 1 <= coarse <= min(num_cus, 256) and coarse <= (nlist + 63) // 64  # no workgroup of the coarse launch without a block
    assert 1 <= scan <= min(num_cus, 256)  # the tail ranks at most 256 partial lists per query
    assert unit % 64 == 0 and 64 <= unit <= 4096


def test_python_wrappers(pkg):
    assert pkg.ivf_one_plan(6000, 100, 24, 256, 1, 16, 16, 24) == _raw(pkg)[1]
    with pytest.raises(pkg.VSearchError) as e:
        pkg.ivf_one_plan(6000, 4096, 24, 256, 1, 16, 16, 24)
    assert e.value.status == -5
    with pytest.raises(pkg.VSearchError) as e:
        pkg.ivf_one_plan(6000, 100, 24, 256, 1, 16, 0, 24)
    assert e.value.status == -1
    assert callable(pkg.IVFIndex.one_stats)
    out = (C.c_int64 * 2)()
    assert pkg.lib().vs_ivf_one_stats(None, out, 0) == -1  # no index: refused before any device is touched
