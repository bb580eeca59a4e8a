"""vs_ivf_one_plan_u8 (host only): the rule that sends a short call on a general IVF index with a byte copy of its rows
(vs_ivf_create_nd_u8 at precision 0 or 2) to the two-launch byte route (ivf_one_coarse_kernel in its byte-index mode +
ivf_one_scan_u8_kernel): its refusals in vs_ivf_one_plan's order, the routes at the rule's edges, its geometry
against vs_ivf_one_plan's, and what vs_ivf_one_u8_stats refuses without a device."""
import ctypes as C
import itertools

import pytest

OK = dict(n_rows=6000, dim=100, nlist=24, num_cus=256, n_batches=1, B=16, k=16, nprobe=24)
BIG = dict(n_rows=1_000_000, dim=384, nlist=1024, num_cus=256, n_batches=3, B=16, k=16, nprobe=256)  # every condition at its edge


def _measured_slower(dim, B, nprobe, nlist):
    """vsearch.h at vs_ivf_one_plan_u8: the two shapes taken out of the rule, with their numbers there"""
    return B == 16 and (dim, min(nprobe, nlist)) in ((96, 128), (128, 256))


def _raw(pkg, out=True, fn="vs_ivf_one_plan_u8", **kw):
    a = dict(OK, **kw)
    buf = (C.c_int64 * 4)(-7, -7, -7, -7)
    rc = getattr(pkg.lib(), fn)(a["n_rows"], a["dim"], a["nlist"], a["num_cus"], a["n_batches"], a["B"], a["k"], a["nprobe"],
                                buf if out else None)
    return rc, tuple(buf)


def test_both_symbols_are_exported(pkg):
    for name in ("vs_ivf_one_plan_u8", "vs_ivf_one_u8_stats"):
        assert hasattr(pkg.lib(), name), name
    assert callable(pkg.ivf_one_plan_u8) and callable(pkg.IVFIndex.one_u8_stats)


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
    # code for code what vs_ivf_one_plan answers
    cases = [dict(), dict(n_rows=0), dict(B=33), dict(dim=0), dict(dim=2049), dict(k=129), dict(k=0, dim=4096), dict(dim=0, k=200)]
    for kw in cases:
        assert _raw(pkg, **kw)[0] == _raw(pkg, fn="vs_ivf_one_plan", **kw)[0], kw


def test_the_rules_edges(pkg):
    assert pkg.ivf_one_plan_u8(**BIG)[0] == 2
    for kw, route in ((dict(n_batches=3), 2), (dict(n_batches=4), 0), (dict(B=16), 2), (dict(B=17), 0), (dict(k=16), 2), (dict(k=17), 0),
                      (dict(nlist=1024), 2), (dict(nlist=1025, nprobe=8), 0), (dict(nprobe=256), 2), (dict(nprobe=257), 0)):
        plan = pkg.ivf_one_plan_u8(**dict(BIG, **kw))
        assert plan[0] == route, (kw, plan)
        if route == 0:
            assert plan == (0, 0, 0, 0), kw
    # nprobe is clamped to nlist before it is compared with 256
    assert pkg.ivf_one_plan_u8(**dict(BIG, nlist=256, nprobe=5000))[0] == 2
    assert pkg.ivf_one_plan_u8(**dict(BIG, nlist=257, nprobe=5000)) == (0, 0, 0, 0)
    # the kernels count rows in 32 bits
    assert pkg.ivf_one_plan_u8(**dict(BIG, n_rows=2 ** 31 - 129))[0] == 2
    assert pkg.ivf_one_plan_u8(**dict(BIG, n_rows=2 ** 31 - 128)) == (0, 0, 0, 0)


def test_the_shape_that_measured_slower(pkg):
    a = dict(n_rows=1_000_000, nlist=1024, num_cus=256, n_batches=1, k=10)
    for dim, B, nprobe, route in ((96, 16, 128, 0), (128, 16, 256, 0), (128, 16, 255, 2), (96, 16, 256, 2), (128, 16, 128, 2), (96, 15, 128, 2),
                                  (96, 16, 127, 2), (96, 16, 129, 2), (97, 16, 128, 2), (127, 16, 256, 2), (96, 1, 8, 2), (96, 8, 128, 2)):
        assert pkg.ivf_one_plan_u8(dim=dim, B=B, nprobe=nprobe, **a)[0] == route, (dim, B, nprobe)
        assert pkg.ivf_one_plan(dim=dim, B=B, nprobe=nprobe, **a)[0] == 1  # vs_ivf_one_plan itself does not change
    # nprobe is clamped to nlist first
    assert pkg.ivf_one_plan_u8(1_000_000, 96, 128, 256, 1, 16, 10, 256)[0] == 0
    assert pkg.ivf_one_plan_u8(1_000_000, 128, 256, 256, 1, 16, 10, 5000)[0] == 0


@pytest.mark.parametrize("dim", [1, 96, 100, 128, 384, 768, 2048])
def test_the_default_rule_is_vs_ivf_one_plans(pkg, dim):
    """Wherever vs_ivf_one_plan says "short", so does the byte rule -- but for the two shapes that measured slower -- with the
    same coarse and scan grids and a byte unit that is whole 64-row blocks."""
    for n_batches, B, k, nprobe, nlist, num_cus in itertools.product((1, 3, 4), (1, 12, 13, 16, 17), (1, 8, 10, 16, 17), (1, 8, 32, 128, 256, 300),
                                                                    (24, 1024, 1025), (1, 256)):
        a = dict(n_rows=1_000_000, dim=dim, nlist=nlist, num_cus=num_cus, n_batches=n_batches, B=B, k=k, nprobe=nprobe)
        f32, u8 = pkg.ivf_one_plan(**a), pkg.ivf_one_plan_u8(**a)
        assert (u8[0] == 2) == (f32[0] == 1 and not _measured_slower(dim, B, nprobe, nlist)), a
        if u8[0]:
            assert u8[1] == f32[1] and u8[3] == f32[3], a
            assert u8[2] >= 64 and u8[2] % 64 == 0 and u8[2] <= 8192, a
        else:
            assert u8 == (0, 0, 0, 0), a


def test_python_wrapper_and_the_stats_refusals(pkg):
    assert pkg.ivf_one_plan_u8(6000, 100, 24, 256, 1, 16, 16, 24) == _raw(pkg)[1]
    with pytest.raises(pkg.VSearchError) as e:
        pkg.ivf_one_plan_u8(6000, 4096, 24, 256, 1, 16, 16, 24)
    assert e.value.status == -5
    with pytest.raises(pkg.VSearchError) as e:
        pkg.ivf_one_plan_u8(6000, 100, 24, 256, 1, 16, 0, 24)
    assert e.value.status == -1
    out = (C.c_int64 * 3)(7, 7, 7)
    assert pkg.lib().vs_ivf_one_u8_stats(None, out, 0) == -1  # no index: refused before any device is touched
    assert pkg.lib().vs_ivf_one_u8_stats(None, None, 1) == -1
    assert tuple(out) == (7, 7, 7)
