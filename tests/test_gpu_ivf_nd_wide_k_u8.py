"""IVF search for 17 <= k <= 128 on a from_u8 general index: both scans of a wide group on the byte rows for the queries
that qualify (ivf_scan_nd_i8_kernel<16>, ivf_scan_nd_cand_i8_kernel), on the fp32 rows for the others.

Every assertion is an equality for every query -- ids, distance bits, total_candidates -- against oracle.ivf_search (integer
data: exact in any order) and against the fp32 index on the same rows.  nd_widek_u8_stats = (pairs on the byte plan, on
the fp32 plan of the first scan; saturated pairs on the byte plan, on the fp32 plan of the rescan) tells which kernels ran."""
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle
from test_gpu_ivf_nd import EMPTY, NLIST, _hi, _int_index, _open
from test_gpu_ivf_nd_ip import _assert_same, _bits, _dev, _host_form
from test_gpu_ivf_nd_u8 import _open_u8, _pairs, _with_a_row_of_255

pytestmark = pytest.mark.gpu

# bound: infinite, infinite, finite, infinite (64 entries < 100), finite.  (33, 2) is there for the inner product: at (17, 1)
# the best list of most queries of dims 64 and 65 is a short or the empty one, and no pair of theirs is saturated
SHAPES = ((17, 1), (33, 2), (32, 4), (100, 4), (128, NLIST))


def _call(ix, q, k, nprobe, metric):
    return ix.search_metric(q, k, nprobe, metric) if metric else ix.search_topk(q, k, nprobe)


def _want(data, q, k, nprobe, metric):
    """(the oracle's result in the host call's form, its probes)"""
    vr, cents, off, r2o = data[:4]
    w = oracle.ivf_search(vr, off, r2o, cents, q, k, nprobe, return_probes=True, metric=metric)
    return (_host_form(w) if metric else w[:3]), w[3]


def _counters(vr, off, q, probes, k, metric, on_bytes):
    """what nd_widek_u8_stats must read after one call, on the CPU (float64: exact on this data).  A pair is saturated
    when its list's 16th best score is at or under the k-th best of its query's 16-bests."""
    q64, v64 = q.astype(np.float64), vr.astype(np.float64)
    s = -(q64 @ v64.T) if metric else (q64 ** 2).sum(1)[:, None] + (v64 ** 2).sum(1)[None, :] - 2 * (q64 @ v64.T)
    out = [0, 0, 0, 0]
    for i, pr in enumerate(probes):
        best = [np.sort(s[i, off[c]:off[c + 1]])[:16] for c in pr if c >= 0 and off[c + 1] > off[c]]
        top = np.sort(np.concatenate(best)) if best else np.zeros(0)
        out[0 if on_bytes[i] else 1] += len(best)
        out[2 if on_bytes[i] else 3] += sum(len(b) == 16 and (len(top) < k or b[15] <= top[k - 1]) for b in best)
    return tuple(out)


@pytest.mark.parametrize("metric", [0, 1])
@pytest.mark.parametrize("dim", [3, 64, 65, 130, 2048])
def test_every_step_shape(gpu_pkg, dim, metric):
    """dim_b / 64 = 1 (the tail step alone), 1, 2 (one full step), 3 (step + tail), 32.  The saturated pairs are counted on
    the CPU: under a finite bound some pairs of every dim stay unsaturated, so the rescan plan is a strict subset."""
    data = vr, cents, off, r2o, q = _int_index(dim)
    q = q[:70]
    with _open_u8(gpu_pkg, vr, cents, off, r2o) as u8, _open(gpu_pkg, vr, cents, off, r2o) as f32:
        for k, nprobe in SHAPES:
            want, probes = _want(data, q, k, nprobe, metric)
            u8.nd_widek_u8_stats(reset=True)
            got = _call(u8, q, k, nprobe, metric)
            _assert_same(got, want, (dim, k, nprobe, "oracle"))
            _assert_same(got, _call(f32, q, k, nprobe, metric), (dim, k, nprobe, "fp32 index"))
            cnt = _counters(vr, off, q, probes, k, metric, np.ones(70, dtype=bool))
            assert cnt[0] == _pairs(probes, off) and (cnt[2] > 0 or (metric, k) == (1, 17)) and (cnt[2] < cnt[0] or nprobe * 16 < k), (dim, k, nprobe, cnt)
            assert u8.nd_widek_u8_stats() == cnt, (dim, k, nprobe)
        if dim == 65:  # the query on the empty list's centroid and the 1-row list: (-1, +inf) tails
            qq = np.stack([cents[EMPTY], vr[off[5]]])
            got = _call(u8, qq, 17, 1, metric)
            _assert_same(got, _want(data, qq, 17, 1, metric)[0], "short lists")
            assert np.all(got[0][0] == -1) and np.all(got[1][0] == np.inf) and got[0][1, 0] == r2o[off[5]] and np.all(got[0][1, 1:] == -1)


@pytest.mark.parametrize("k", [40, 128])
def test_zero_products_under_inner_product(gpu_pkg, k):
    """an all-zero query qualifies for bytes; every score is -0.0 and the ranking is by position in vectors_reordered"""
    vr, cents, off, r2o, _ = _int_index(100)
    q = np.zeros((1, 100), dtype=np.float32)
    want = oracle.ivf_search(vr, off, r2o, cents, q, k, NLIST, metric=1)
    assert np.all(_bits(want[1]).view(np.uint32) == 0x80000000)
    with _open_u8(gpu_pkg, vr, cents, off, r2o) as u8:
        got, st = _dev(u8, q, 1, 1, k, NLIST, 1), u8.nd_widek_u8_stats()
    _assert_same(got, want[:2], k)
    assert np.array_equal(got[0][0], r2o[:k])
    assert st[0] == NLIST - 1 and st[1] == 0 and st[2] > 0 and st[3] == 0, st


@pytest.mark.parametrize("dim", [100, 384])
def test_mixed_groups(gpu_pkg, dim):
    """a third of the queries carry a value that is no byte: their pairs take the fp32 plans of the same group"""
    vr, cents, off, r2o, q = _int_index(dim)
    q = np.array(q[:70])
    rng = np.random.default_rng(8100 + dim)
    ok = np.arange(70) % 3 != 1
    bad = np.flatnonzero(~ok)
    for j, i in enumerate(bad):
        q[i, rng.integers(0, dim)] = (0.5, 256.0, -1.0)[j % 3]
    with _open_u8(gpu_pkg, vr, cents, off, r2o) as u8, _open(gpu_pkg, vr, cents, off, r2o) as f32:
        for nprobe in (4, NLIST):  # (at NLIST the 40 best spread over 23 lists: few saturated pairs, at dim 384 none on fp32)
            u8.nd_widek_u8_stats(reset=True)
            _assert_same(u8.search_topk(q, 40, nprobe), f32.search_topk(q, 40, nprobe), (dim, nprobe))
            split = _counters(vr, off, q, oracle.ivf_search(vr, off, r2o, cents, q, 40, nprobe, return_probes=True)[3], 40, 0, ok)
            assert min(split) > 0 if nprobe == 4 else split[:2] == (int(ok.sum()) * (NLIST - 1), len(bad) * (NLIST - 1)), split
            assert u8.nd_widek_u8_stats(reset=True) == split, (dim, nprobe)
        u8.set_precision(1)
        _assert_same(u8.search_topk(q, 40, NLIST), f32.search_topk(q, 40, NLIST), (dim, "precision 1"))
        assert u8.nd_widek_u8_stats(reset=True)[0::2] == (0, 0)
        u8.set_precision(2)
        _assert_same(u8.search_topk(q, 40, NLIST), f32.search_topk(q, 40, NLIST), (dim, "precision 2"))
        assert u8.nd_widek_u8_stats() == split


def test_the_rules_edges(gpu_pkg):
    vr, cents, off, r2o, q = _with_a_row_of_255(260)  # max ||b||^2 >= 2^24: no byte copy
    with _open_u8(gpu_pkg, vr, cents, off, r2o) as u8, _open(gpu_pkg, vr, cents, off, r2o) as f32:
        _assert_same(u8.search_topk(q[:70], 40, 4), f32.search_topk(q[:70], 40, 4), "no byte copy")
        assert u8.nd_u8_stats()[0] == 0
        with pytest.raises(gpu_pkg.VSearchError) as e:
            u8.nd_widek_u8_stats()
        assert e.value.status == -1
    vr, cents, off, r2o, q = _with_a_row_of_255(258)  # max ||b||^2 = 2^24 - 766
    q = np.zeros((3, 258), dtype=np.float32)
    q[0, :3], q[1, :4], q[2, :3] = (27, 6, 1), (27, 6, 1, 1), (1, 6, 27)  # ||q||^2 = 766, 767 (one too many), 766
    with _open_u8(gpu_pkg, vr, cents, off, r2o) as u8, _open(gpu_pkg, vr, cents, off, r2o) as f32:
        _assert_same(u8.search_topk(q, 128, NLIST), f32.search_topk(q, 128, NLIST), "the norm boundary")
        cnt = _counters(vr, off, q, np.tile(np.arange(NLIST), (3, 1)), 128, 0, np.array([True, False, True]))
        assert cnt[:2] == (2 * (NLIST - 1), NLIST - 1) and cnt[2] > 0 and cnt[3] > 0, cnt
        assert u8.nd_widek_u8_stats() == cnt


def test_fallbacks_on_bytes(gpu_pkg):
    """more than 8192 candidates: a 9000-row list under an infinite bound, 8500 equal rows under a bound of 0"""
    rng, dim, hi = np.random.default_rng(7400), 20, _hi(20)
    for sizes, k, nprobe in (([9000, 500, 500], 17, 1), ([9000] + [200] * 7, 100, 8)):
        n, nlist = sum(sizes), len(sizes)
        vr = rng.integers(0, hi, size=(n, dim)).astype(np.float32)
        if k == 100:
            vr[300:8800] = vr[300]
        off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
        r2o = rng.permutation(n).astype(np.int32)
        cents = np.stack([np.rint(vr[off[c]:off[c + 1]].astype(np.float64).mean(0)) for c in range(nlist)]).astype(np.float32)
        q = rng.integers(0, hi, size=(5, dim)).astype(np.float32)
        q[2] = cents[0] if k == 17 else vr[300]
        want = oracle.ivf_search(vr, off, r2o, cents, q, k, nprobe, return_probes=True)
        assert want[3][2, 0] == 0 and (k == 17 or (np.all(want[1][2] == 0) and np.array_equal(want[0][2], r2o[300:400])))
        with _open_u8(gpu_pkg, vr, cents, off, r2o) as u8:
            got = u8.search_topk(q, k, nprobe)
            st, wide = u8.nd_widek_u8_stats(), u8.nd_widek_stats()
        _assert_same(got, want[:3], sizes)
        assert wide[2] >= 1 and st[0] == 5 * nprobe and st[1] == 0 and st[2] > 0 and st[3] == 0, (wide, st)


def test_state_and_calls(gpu_pkg):
    """1100 queries in one host call are two launch groups; a k = 5 call between two wide calls; a device call on a stream"""
    import torch
    data = vr, cents, off, r2o, q = _int_index(100)
    qq = np.random.default_rng(7300).integers(0, _hi(100), size=(1100, 100)).astype(np.float32)
    qq[:96] = q
    want = _want(data, qq, 40, 4, 0)[0]
    with _open_u8(gpu_pkg, vr, cents, off, r2o) as u8:
        a = u8.search_topk(qq, 40, 4)
        s1, b1 = u8.nd_widek_u8_stats(), u8.nd_u8_stats()
        _assert_same(u8.searchBatch(q, len(q), 5, 4), _want(data, q, 5, 4, 0)[0], "k 5 between two wide calls")
        b2 = u8.nd_u8_stats()
        b = u8.search_topk(qq, 40, 4)
        s2 = u8.nd_widek_u8_stats()
        assert b1[0] == 0 and b2[0] > 0 and u8.nd_u8_stats()[0] == b2[0]
        _assert_same(a, want, "first call"), _assert_same(b, a, "second call")
        assert s1[0] > s1[2] > 0 and s1[1] == 0 and s2 == tuple(2 * v for v in s1), (s1, s2)
        got = _dev(u8, q, 3, 24, 40, 4, 0, torch.cuda.Stream())
        _assert_same(got, (want[0][:72], want[1][:72]), "device call")


_TOGGLE_SCRIPT = r"""
import sys, numpy as np
sys.path.insert(0, sys.argv[1])
import __graft_entry__ as ge
pkg = ge.load_package()
z = np.load(sys.argv[2])
with pkg.IVFIndex.from_u8(z["vr"], z["cents"], z["off"], z["r2o"]) as ivf:
    (i, d, t), (pi, pd, _) = ivf.search_topk(z["q"], 40, 4), ivf.search_metric(z["q"], 40, 4, 1)
    np.savez(sys.argv[3], i=i, d=d, t=t, pi=pi, pd=pd, stats=np.array(ivf.nd_widek_u8_stats()))
print("TOGGLE_OK")
"""


def test_toggle(gpu_pkg, tmp_path):
    """VSEARCH_IVF_ND_WIDE_U8=0 (a child process: the variable is read at creation): the same outputs, nothing on bytes"""
    vr, cents, off, r2o, q = _int_index(100)
    q, u8rows = q[:70], vr.astype(np.uint8)
    with gpu_pkg.IVFIndex.from_u8(u8rows, cents, off, r2o) as u8:
        a, p = u8.search_topk(q, 40, 4), u8.search_metric(q, 40, 4, 1)
        assert u8.nd_widek_u8_stats()[0] > 0
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src, dst = str(tmp_path / "in.npz"), str(tmp_path / "out.npz")
    np.savez(src, vr=u8rows, cents=cents, off=off, r2o=r2o, q=q)
    r = subprocess.run([sys.executable, "-c", _TOGGLE_SCRIPT, root, src, dst], env=dict(os.environ, VSEARCH_IVF_ND_WIDE_U8="0"),
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "TOGGLE_OK" in r.stdout, (r.stdout[-400:], r.stderr[-1200:])
    z = np.load(dst)
    _assert_same((z["i"], z["d"], int(z["t"])), a, "toggle, L2"), _assert_same((z["pi"], z["pd"]), p[:2], "toggle, inner product")
    assert z["stats"].tolist() == [0, 0, 0, 0]
