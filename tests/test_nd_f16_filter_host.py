"""vs_bf_filter_f16_plan: refusals, the shapes that never take the f16 prefilter, and the rule.  No GPU."""
import ctypes as C

import pytest


def test_plan_refusals(pkg):
    L = pkg.lib()
    out = (C.c_int64 * 6)()
    cases = [((0, 0, 0, 0, 0), "at least 1"), ((1000, 0, 256, 4, 10), "dim must be at least 1"), ((1000, 4096, 256, 4, 10), "dim > 2048")]
    for args, msg in cases:
        assert L.vs_bf_filter_f16_plan(*args, out) != 0
        with pytest.raises(Exception, match=msg):
            pkg.filter_f16_plan(*args)
    assert L.vs_bf_filter_f16_plan(1000000, 64, 256, 4, 10, None) != 0
    assert "vs_bf_filter_f16_plan" in pkg.exported_symbols()


@pytest.mark.parametrize("args", [(1000000, 384, 256, 3, 10), (1000000, 384, 256, 33, 10), (1000000, 384, 256, 8, 16), (4099, 384, 256, 4, 10)])
def test_no_route(pkg, args):
    """fewer than 4 batches, more than a launch group, wide k, and a shard far below anything the rule could hold"""
    assert pkg.filter_f16_plan(*args) == (0, 0, 0, 0, 0, 0)


@pytest.mark.parametrize("n_rows", [1000000, 3000000])
@pytest.mark.parametrize("nb", [4, 9, 16, 17, 32])
def test_rule(pkg, n_rows, nb):
    """measured shapes only: 384 <= dim <= 2048, 1 000 000 <= n_rows <= 3 000 000; the geometry is the fp32
    route's (ndf_plan, through vs_bf_filter_nd_plan at a dimension both rules hold)"""
    plan = pkg.filter_f16_plan(n_rows, 768, 256, nb, 10)
    assert plan[0] == 1 and plan == pkg.bf_filter_nd_plan(n_rows, 768, 256, nb, 10)
    assert pkg.filter_f16_plan(n_rows, 2048, 256, nb, 15)[1:] == plan[1:]
    for args in ((n_rows, 383, 256, nb, 10), (999999, 768, 256, nb, 10), (3000001, 768, 256, nb, 10), (262144, 384, 256, nb, 10), (n_rows, 96, 256, nb, 10)):
        assert pkg.filter_f16_plan(*args)[0] == 0
