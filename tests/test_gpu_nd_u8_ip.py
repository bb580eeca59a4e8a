"""Inner-product brute force on uint8 rows at any vector length (vs_bf_create_nd_u8_metric, the IP instantiations of
scan_nd_i8_kernel) against the int64 reference of nd_u8_ip_data: q.astype(int64) @ base.astype(int64).T ranked by
(-q.b, id).  The expected value is never another GPU result, except where a test says it compares two indexes.

Device calls return -(q.b) ascending by (score, id), k + 1 entries, (-1, +inf) past the rows; host calls return q.b
descending, equal scores by ascending id, k entries.  Data: nd_u8_ip_data.ip_data (its planted edges are asserted on the
CPU in test_nd_u8_ip_host.py)."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import nd_u8_ip_data as D
from nd_u8_data import sqnorm_max, u8_data

pytestmark = pytest.mark.gpu

DIMS = [1, 3, 63, 64, 65, 100, 128, 129, 192, 320, 960, 2048]
K1_REF = 16  # the reference lists hold the 16 best: the k + 1 best of every k <= 15 are their prefixes
NEG_ZERO = 0x80000000


def _f32(a):
    return a.astype(np.float32)


def _dev_multi(idx, q, nb, B, k, call="search_dev_multi"):
    import torch
    dev = torch.device("cuda:0")
    s = torch.cuda.current_stream().cuda_stream
    qd = torch.from_numpy(np.ascontiguousarray(q[:nb * B], dtype=np.float32)).to(dev)
    ids = torch.full((nb * B, k + 1), -7, dtype=torch.int32, device=dev)
    d = torch.zeros((nb * B, k + 1), dtype=torch.float32, device=dev)
    fl = torch.full((nb * B,), -7, dtype=torch.int32, device=dev)
    getattr(idx, call)(qd.data_ptr(), nb, B, k, ids.data_ptr(), d.data_ptr(), fl.data_ptr(), s)
    torch.cuda.synchronize()
    return ids.cpu().numpy(), d.cpu().numpy(), fl.cpu().numpy()


def _check_dev(idx, q, ref, nb, B, k, tag, byte_scan=True):
    ri, rd = ref[0][:nb * B, :k + 1], ref[1][:nb * B, :k + 1]
    ids, d, flags = _dev_multi(idx, q, nb, B, k)
    assert np.array_equal(d, rd), "device scores differ " + tag
    assert np.array_equal(ids, ri), "device ids differ " + tag
    assert np.array_equal(flags, D.tie_flags(rd)), "device flags differ " + tag
    return ids, d, flags


def _check_host(idx, q, ref, k, tag, search="search"):
    hi, hs = D.host_view(ref[0], ref[1], k)
    ids, s = getattr(idx, search)(_f32(q), k)
    assert np.array_equal(s, hs), "host scores differ " + tag
    assert np.array_equal(ids, hi), "host ids differ " + tag


def _check_exact(pkg, base, q, ks, precisions=(2, 1), batch=None, dev_B=32, ref=None):
    ref = ref or D.topk_ref(D.ip_int64(q, base), K1_REF)
    with pkg.BruteForceIndex.from_u8(base, metric=pkg.METRIC_IP) as idx:
        assert idx.getDim() == base.shape[1] and idx.getNumDocs() == base.shape[0]
        if batch:
            idx.set_batch(batch)
        for prec in precisions:
            idx.set_precision(prec)
            for k in ks:
                tag = f"(N={base.shape[0]}, dim={base.shape[1]}, nq={len(q)}, k={k}, batch={batch}, precision={prec})"
                _check_host(idx, q, ref, k, tag)
                _check_dev(idx, q, ref, len(q) // dev_B, dev_B, k, tag)
    return ref


@pytest.mark.parametrize("dim", DIMS)
def test_exact_at_every_dimension(gpu_pkg, dim):
    """One 64-byte step with no pair, even and odd step counts, the tail step, the forced-general 128 and the maximum; k
    covers the 8- and the 16-entry lane lists; precision 2 (bytes) and 1 (fp32 rows) of one index; 70 queries through the
    host call (two batches of 32 and a ragged one of 6) and two batches of 32 through the device call."""
    n = 20000 if dim <= 320 else 3000
    rng = np.random.default_rng(7000 + dim)
    base, q = D.ip_data(rng, n, 70, dim)
    ref = _check_exact(gpu_pkg, base, q, (1, 7, 8, 15))
    assert D.tie_flags(ref[1])[:64].any()


@pytest.mark.parametrize("dim", [100, 960])
@pytest.mark.parametrize("n", [1, 5, 17, 63, 65, 4099])
def test_ragged_bases(gpu_pkg, dim, n):
    """k clamped to n; the device lists' slots past the rows are (-1, +inf)."""
    rng = np.random.default_rng(8000 + dim + n)
    base, q = D.ip_data(rng, n, 33, dim)
    if n >= 2:
        base[n - 1] = base[0]
    ref = D.topk_ref(D.ip_int64(q, base), K1_REF)
    k = min(5, n)
    assert n > 5 or (ref[0][:, k] == -1).all() and np.isinf(ref[1][:, k]).all()
    _check_exact(gpu_pkg, base, q, (k,), dev_B=32, ref=ref)
    _check_exact(gpu_pkg, base, q, (k,), precisions=(2,), dev_B=11, ref=ref)


@pytest.mark.parametrize("batch", [1, 7, 16, 17, 32])
def test_batch_sizes_at_dim_320(gpu_pkg, batch):
    """One and two query blocks per tile, zero-padded query slots; k = 5 and 15 take the 8- and the 16-entry lane lists."""
    rng = np.random.default_rng(9000)
    base, q = D.ip_data(rng, 20000, 70, 320)
    _check_exact(gpu_pkg, base, q, (5, 15), precisions=(2,), batch=batch, dev_B=batch)


def test_threshold_exchange_of_both_precisions(gpu_pkg):
    """The shape of test_gpu_nd_u8.py::test_threshold_exchange_of_both_precisions, whose docstring derives that 270001
    rows at dim 192 make bf_launch take the in-kernel exchange on the byte rows and on the fp32 rows (the geometry does not
    depend on the metric).  The exchanged thresholds are negative here.  Batches of 32 with k = 5 and 15 are NQH = 2 with
    the 8- and 16-entry lists, batches of 16 are NQH = 1."""
    base, q = D.ip_data(np.random.default_rng(11000), 270001, 32, 192)
    ref = D.topk_ref(D.ip_int64(q, base), K1_REF)
    assert (np.delete(ref[1], D.ZERO_Q, axis=0) < 0).all()  # (the zero query's scores are -0.0)
    _check_exact(gpu_pkg, base, q, (5, 15), precisions=(2, 1), ref=ref)
    _check_exact(gpu_pkg, base, q, (5, 15), precisions=(2,), batch=16, dev_B=16, ref=ref)


@pytest.mark.parametrize("dim", [2, 100, 128])
def test_zero_products_are_negative_zero(gpu_pkg, dim):
    """The device calls return the bit pattern of -0.0 for an exactly zero product, as the fp32 scan's negation does; the
    host call returns 0.0, equal scores in ascending id.  The zero query on a large base (its k + 1 best are rows 0 .. k),
    and the disjoint supports on a base of 12 rows, where k = 15 returns every row."""
    rng = np.random.default_rng(12000 + dim)
    big, qb = D.ip_data(rng, 5000, 32, dim)
    small, qs = D.small_orth_base(rng, dim)
    zero_pairs = [(j, r) for j in D.ORTH_Q for r in (1, 2, 4, len(small) - 1)]
    for base, q, k in ((big, qb, 15), (small, qs, 15)):
        ip = D.ip_int64(q, base)
        ref = D.topk_ref(ip, K1_REF)
        with gpu_pkg.BruteForceIndex.from_u8(base, metric=gpu_pkg.METRIC_IP) as idx:
            for prec in (2, 1):
                idx.set_precision(prec)
                ids, d, flags = _check_dev(idx, q, ref, 1, len(q), k, f"(dim={dim}, n={len(base)}, precision={prec})")
                bits = d.view(np.uint32)
                live = ids >= 0
                assert np.array_equal(bits[live] == NEG_ZERO, (np.take_along_axis(ip, np.maximum(ids, 0).astype(np.int64), 1) == 0)[live])
                assert not (bits[live] == 0).any(), "+0.0 among the device scores"
                assert (bits[D.ZERO_Q][live[D.ZERO_Q]] == NEG_ZERO).all()
                assert np.array_equal(ids[D.ZERO_Q][live[D.ZERO_Q]], np.arange(live[D.ZERO_Q].sum()))
                if base is small:
                    for j, r in zero_pairs:
                        assert bits[j][ids[j] == r] == NEG_ZERO
                hi, hs = idx.search(_f32(q), min(k, len(base)))
                wi, ws = D.host_view(ref[0], ref[1], min(k, len(base)))
                assert np.array_equal(hi, wi) and np.array_equal(hs, ws)
                assert not np.signbit(hs[D.ZERO_Q]).any() and not hs[D.ZERO_Q].any()


@pytest.mark.parametrize("dim", [128, 300])
def test_non_byte_queries_are_refused_per_batch(gpu_pkg, dim):
    """Six batches of 32: batch 1 holds a value 7.5, batch 3 a value 256, batch 4 a value -1.  Under precision 0 exactly
    those batches report flags == 2 -- only the byte scan ever does: an implementation without it cannot pass -- and the
    others are exact.  The host call reruns them on the fp32 rows: every query must come back as the fp32 index over the
    same rows (BruteForceIndex(base as float, IP), code that is older than the byte scan) returns it.  All query values are
    half-integers and ||q||^2 + ||b||^2 < 2^24, so every partial sum of every product is a half-integer below 2^23:
    exactly representable, whatever the order of the chain, and the float64 product is the expected score."""
    nb, B, k = 6, 32, 5
    rng = np.random.default_rng(13000 + dim)
    base, qu = D.ip_data(rng, 6000, nb * B, dim)
    q = _f32(qu)
    q[1 * B + 4, 10] = 7.5
    q[3 * B + 0, 3] = 256.0
    q[4 * B + 31, dim - 1] = -1.0
    bad = (1 * B + 4, 3 * B, 4 * B + 31)
    assert (q.astype(np.float64) ** 2).sum(1).max() + sqnorm_max(base) < 2 ** 24
    skipped = np.zeros(nb * B, dtype=bool)
    for b in (1, 3, 4):
        skipped[b * B:(b + 1) * B] = True
    ref = D.topk_ref(D.ip_int64(qu, base), K1_REF)
    ri, rd = ref[0][:, :k + 1], ref[1][:, :k + 1]
    with gpu_pkg.BruteForceIndex.from_u8(base, metric=gpu_pkg.METRIC_IP) as idx:
        assert idx.getDim() == dim
        for prec in (0, 2):
            idx.set_precision(prec)
            ids, d, flags = _dev_multi(idx, q, nb, B, k)
            assert np.array_equal(flags == 2, skipped)
            keep = ~skipped
            assert np.array_equal(d[keep], rd[keep]) and np.array_equal(ids[keep], ri[keep])
            assert np.array_equal(flags[keep], D.tie_flags(rd)[keep])
        idx.set_precision(0)
        got = idx.search(q, k)
        idx.set_precision(1)
        ids1, d1, flags1 = _dev_multi(idx, q, nb, B, k)
        assert not (flags1 == 2).any()
    with gpu_pkg.BruteForceIndex(_f32(base), metric=gpu_pkg.METRIC_IP) as f32_idx:
        want = f32_idx.search(q, k)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    # ... which is the exact answer: the untouched queries against the int64 reference, the three others in float64
    untouched = np.ones(nb * B, dtype=bool)
    untouched[list(bad)] = False
    hi, hs = D.host_view(ref[0], ref[1], k)
    assert np.array_equal(got[0][untouched], hi[untouched]) and np.array_equal(got[1][untouched], hs[untouched])
    for i in bad:
        s = q[i].astype(np.float64) @ base.astype(np.float64).T
        o = np.lexsort((np.arange(len(base)), -s))[:k]
        assert np.array_equal(got[0][i], o) and np.array_equal(got[1][i], s[o].astype(np.float32))
        assert np.array_equal(-d1[i, :k], s[o].astype(np.float32))


def _with_sqnorm(target, dim):
    """A byte vector whose squared norm is exactly `target` (greedy: the largest square that fits, coordinate by coordinate)."""
    v = np.zeros(dim, dtype=np.uint8)
    left = target
    for i in range(dim):
        x = min(255, math.isqrt(left))
        v[i] = x
        left -= x * x
    assert left == 0 and sqnorm_max(v[None]) == target
    return v


def test_norm_rule_at_dim_2048(gpu_pkg):
    """max ||q||^2 + max ||b||^2 <= 2^24 decides per batch, to the unit: a batch exactly on the bound is scanned on bytes
    and is exact, one unit above it is refused.  The host call reruns the refused batches on the fp32 rows; one unit above
    the bound every partial sum is still below 2^24, so that batch must equal the int64 reference as well."""
    rng = np.random.default_rng(5500)
    dim, n, B, k = 2048, 5000, 32, 5
    base = rng.integers(0, 41, size=(n, dim)).astype(np.uint8)
    bmax = sqnorm_max(base)
    assert bmax < 2048 * 1600 + 1
    q = rng.integers(0, 41, size=(3 * B, dim)).astype(np.uint8)
    q[7] = _with_sqnorm(2 ** 24 - bmax, dim)               # batch 0: on the bound
    q[B + 5] = 255                                         # batch 1: far above it
    q[2 * B + 9] = _with_sqnorm(2 ** 24 - bmax + 1, dim)   # batch 2: one above it
    ref = D.topk_ref(D.ip_int64(q, base), K1_REF)
    ri, rd = ref[0][:, :k + 1], ref[1][:, :k + 1]
    with gpu_pkg.BruteForceIndex.from_u8(base, metric=gpu_pkg.METRIC_IP) as idx:
        idx.set_precision(2)
        ids, d, flags = _dev_multi(idx, _f32(q), 3, B, k)
        assert not (flags[:B] == 2).any()
        assert (flags[B:] == 2).all()
        assert np.array_equal(d[:B], rd[:B]) and np.array_equal(ids[:B], ri[:B])
        assert np.array_equal(flags[:B], D.tie_flags(rd[:B]))
        got = idx.search(_f32(q), k)
        idx.set_precision(1)
        want = idx.search(_f32(q), k)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    hi, hs = D.host_view(ref[0], ref[1], k)
    exact = np.r_[0:B, 2 * B:3 * B]
    assert np.array_equal(got[0][exact], hi[exact]) and np.array_equal(got[1][exact], hs[exact])


def test_base_norm_too_large_for_the_byte_scan(gpu_pkg):
    """One all-255 row at dim 2048 (||b||^2 = 2048 * 255^2 >= 2^24): the index is created without the byte copy, precision
    2 is refused, and precision 0 searches the fp32 rows: what precision 1 gives, and never flags == 2."""
    rng = np.random.default_rng(5600)
    dim, n = 2048, 3000
    base = rng.integers(0, 41, size=(n, dim)).astype(np.uint8)
    base[1234] = 255
    q = _f32(rng.integers(0, 41, size=(64, dim)).astype(np.uint8))
    with gpu_pkg.BruteForceIndex.from_u8(base, metric=gpu_pkg.METRIC_IP) as idx:
        assert gpu_pkg.lib().vs_set_precision(idx._h, 2) == -5
        assert "2^24" in gpu_pkg.lib().vs_last_error().decode()
        idx.set_precision(0)
        got = idx.search(q, 5)
        ids, d, flags = _dev_multi(idx, q, 2, 32, 5)
        assert not (flags == 2).any()
        idx.set_precision(1)
        want = idx.search(q, 5)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    assert (got[0][:, 0] == 1234).all()
    assert np.array_equal(-d[:, :5], got[1]) and np.array_equal(ids[:, :5], got[0])


@pytest.mark.parametrize("dim,n", [(128, 40000), (320, 20000)])
def test_l2_through_the_new_creator_is_vs_bf_create_nd_u8(gpu_pkg, dim, n):
    """Two indexes compared: vs_bf_create_nd_u8_metric(VS_METRIC_L2) against vs_bf_create_nd_u8 on the same rows -- ids,
    distances, flags, the number of scan launches and the precision semantics.  The middle batch of the device call holds a
    value 7.5 (flags == 2 under precision 2 and 0), so that a live batch follows the skipped one in the same launch: at
    dim 128 both creators give the specialised index, whose scan_kernel stages the next batch's queries itself when it
    skips a batch (test_gpu_mixed_batches.py checks those launches against exact lists), at dim 320 the general one."""
    L = gpu_pkg.lib()
    rng = np.random.default_rng(14000 + dim)
    base, q = u8_data(rng, n, 96, dim)
    qf = _f32(q)
    qf[40, 3] = 7.5  # (batch 1 of the device call is no byte batch)
    res = []
    for metric_form in (False, True):
        h = C.c_void_p(None)
        bp = base.ctypes.data_as(C.c_void_p)
        if metric_form:
            assert L.vs_bf_create_nd_u8_metric(bp, n, dim, 0, 0, 0, C.byref(h)) == 0
        else:
            assert L.vs_bf_create_nd_u8(bp, n, dim, 0, 0, C.byref(h)) == 0
        idx = gpu_pkg.BruteForceIndex.__new__(gpu_pkg.BruteForceIndex)
        gpu_pkg._Index.__init__(idx)
        idx._h, idx.n, idx.d = h, n, dim
        with idx:
            out = []
            for prec in (2, 0, 1):
                idx.set_precision(prec)
                idx.prof_enable(True)
                out.append(_dev_multi(idx, qf, 3, 32, 5))
                out.append(idx.search(qf, 5))
                out.append(idx.prof_read(0)[1])
                idx.prof_enable(False)
            res.append(out)
    for a, b in zip(*res):
        if isinstance(a, tuple) and len(a) == 3:  # a device call: the lists of a skipped batch (flags == 2) are not defined
            ran = a[2] != 2
            assert np.array_equal(a[2], b[2])
            assert np.array_equal(a[0][ran], b[0][ran]) and np.array_equal(a[1][ran], b[1][ran])
        elif isinstance(a, tuple):
            assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
        else:
            assert a == b and a > 0
    flags2 = res[1][0][2]
    assert (flags2[32:64] == 2).all() and not (flags2[:32] == 2).any() and not (flags2[64:] == 2).any()
    assert not (res[1][6][2] == 2).any()  # (precision 1)


@pytest.mark.parametrize("dim", [300, 128])
def test_refusals_leave_the_index_usable(gpu_pkg, dim):
    """The inner-product byte index is a general index at every dimension, 128 included: the virtual-shard call and the
    vs_ivf_* calls refuse it with the dimension in the message."""
    L = gpu_pkg.lib()
    rng = np.random.default_rng(15000 + dim)
    base, qu = D.ip_data(rng, 3000, 8, dim)
    q = _f32(qu)
    with gpu_pkg.BruteForceIndex.from_u8(base, metric=gpu_pkg.METRIC_IP) as idx:
        with pytest.raises(gpu_pkg.VSearchError) as e:
            gpu_pkg.BruteForceIndex.search_vshards([idx], q, 5)
        assert e.value.status == -5 and f"dim = {dim}" in str(e.value)
        ids = np.zeros((8, 5), dtype=np.int32)
        d = np.zeros((8, 5), dtype=np.float32)
        assert L.vs_ivf_search(idx._h, q.ctypes.data_as(C.c_void_p), 8, 5, 4, ids.ctypes.data_as(C.c_void_p),
                               d.ctypes.data_as(C.c_void_p), None, None) == -5
        assert f"dim = {dim}".encode() in L.vs_last_error()
        assert L.vs_ivf_set_metric(idx._h, 1) == -5
        assert f"dim = {dim}".encode() in L.vs_last_error()
        assert L.vs_ivf_search_metric(idx._h, q.ctypes.data_as(C.c_void_p), 8, 5, 4, 1, ids.ctypes.data_as(C.c_void_p),
                                      d.ctypes.data_as(C.c_void_p), None, None) == -5  # ("not an IVF index")
        ref = D.topk_ref(D.ip_int64(qu, base), K1_REF)
        _check_host(idx, qu, ref, 5, f"(dim={dim}, after the refusals)")
        _check_dev(idx, q, ref, 1, 8, 5, f"(dim={dim}, after the refusals)")


def test_wide_k_and_scores_use_the_fp32_rows(gpu_pkg):
    """k = 16 and k = 100 (vs_bf_search_topk, vs_bf_search_topk_dev_multi) and the score matrix read the fp32 rows under
    every precision setting, and equal the int64 reference."""
    import torch
    rng = np.random.default_rng(4050)
    n, B, ld = 30000, 20, 30016
    base, q = D.ip_data(rng, n, 40, 96)
    ip = D.ip_int64(q, base)
    ref = D.topk_ref(ip, 101)
    dev = torch.device("cuda:0")
    s = torch.cuda.current_stream().cuda_stream
    qd = torch.from_numpy(_f32(q[:B])).to(dev)
    with gpu_pkg.BruteForceIndex.from_u8(base, metric=gpu_pkg.METRIC_IP) as idx:
        for prec in (0, 1, 2):
            idx.set_precision(prec)
            for k in (16, 100):
                _check_host(idx, q, ref, k, f"(k={k}, precision={prec})", search="search_topk")
                ids, d, flags = _dev_multi(idx, q, 2, B, k, call="search_topk_dev_multi")
                assert np.array_equal(ids, ref[0][:2 * B, :k + 1]) and np.array_equal(d, ref[1][:2 * B, :k + 1])
                assert not (flags == 2).any()
            out = torch.full((B, ld), -1.0, dtype=torch.float32, device=dev)
            idx.scores_dev(qd.data_ptr(), B, out.data_ptr(), ld, s)
            torch.cuda.synchronize()
            sc = out.cpu().numpy()
            want = -(ip[:B].astype(np.float32))
            assert np.array_equal(sc[:, :n], want)
            assert np.array_equal(np.signbit(sc[:, :n]), np.signbit(want))  # (-0.0 for the zero products)


def test_cli_metric_ip(gpu_pkg, tmp_path):
    """vsearch_bf --metric ip on a .bvecs and on a .fvecs base: ids and scores q.v, descending, in the results grammar.
    Values under 64 at dim 200 keep every score under 10^6: the six significant digits of the grammar print them exactly."""
    import oracle
    rng = np.random.default_rng(9500)
    dim, n, nq, k = 200, 5000, 50, 5
    base = rng.integers(0, 64, size=(n, dim)).astype(np.uint8)
    q = rng.integers(0, 64, size=(nq, dim)).astype(np.uint8)
    base[n - 3] = base[17]
    q[0] = 0
    ip = D.ip_int64(q, base)
    assert ip.max() < 10 ** 6
    hi, hs = D.host_view(*D.topk_ref(ip, k), k)
    exe = os.path.join(os.path.dirname(gpu_pkg.LIB_PATH), "vsearch_bf")
    assert os.path.exists(exe), "vsearch_bf not built (make -C hai-25-rag-on-edge_amd/csrc all)"
    env = dict(os.environ)
    env["LD_LIBRARY_PATH"] = gpu_pkg.hip_runtime_dir() + os.pathsep + env.get("LD_LIBRARY_PATH", "")
    for ext in ("bvecs", "fvecs"):
        d = tmp_path / ext
        d.mkdir()
        if ext == "fvecs":
            gpu_pkg.write_fvecs(str(d / "base.fvecs"), _f32(base))
            gpu_pkg.write_fvecs(str(d / "query.fvecs"), _f32(q))
        else:
            gpu_pkg.write_bvecs(str(d / "base.bvecs"), base)
            gpu_pkg.write_bvecs(str(d / "query.bvecs"), q)
        r = subprocess.run([exe, f"base.{ext}", f"query.{ext}", str(k), "out.txt", "--metric", "ip"], cwd=d, env=env,
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        assert f"Dimension: {dim}" in r.stdout
        gi, gs = oracle.parse_results_txt(str(d / "out.txt"))
        assert np.array_equal(np.array(gi, dtype=np.int32), hi), ext
        assert np.array_equal(np.array(gs, dtype=np.float32), hs), ext
    # (refused before anything touches the GPU)
    r = subprocess.run([exe, "base.bvecs", "query.bvecs", str(k), "out2.txt", "--metric", "ip", "--gpus", "2"],
                       cwd=tmp_path / "bvecs", env=env, capture_output=True, text=True, timeout=60)
    assert r.returncode != 0
    assert "--metric ip" in r.stderr and "--gpus" in r.stderr
    assert not os.path.exists(tmp_path / "bvecs" / "out2.txt")
