"""GPU checks of the UFIXED_POINT_8 runner's top-k up to k = 128 (vs_q8_search_topk*, vs_q8_topk_scores_dev), every one
bit for bit against tests/q8_wide_ref.py (np.lexsort((ids, -scores)), padded with (-1, 0)).

The crafted matrices go through topk_scores_dev on a runner built from a dim-4 base of n rows: the matrix is a torch uint8
tensor with ld = n rounded up to 64 and the padding bytes set to 255, so that a counted padding byte shows.  Every device
call writes into buffers with guard words behind them.  tests/test_q8_wide_host.py checks the generators' preconditions."""
import os
import subprocess

import numpy as np
import pytest

import oracle
import q8_wide_ref as ref

pytestmark = pytest.mark.gpu

_runners = {}
_cases = {}


@pytest.fixture(scope="module", autouse=True)
def _close_runners():
    yield
    for r in list(_runners.values()) + [c[0] for c in _cases.values()]:
        r.close()
    _runners.clear()
    _cases.clear()


def _runner(pkg, n, dim=4):
    """One runner per row count, kept for the session: its scores do not matter, only its size."""
    if (n, dim) not in _runners:
        _runners[(n, dim)] = pkg.Q8Runner(np.ones((n, dim), dtype=np.float32), 1.0, 1.0, 0, 1.0)
    return _runners[(n, dim)]


def select(r, mat, k, stream=None, guard=64):
    """topk_scores_dev on the padded matrix: (ids, top) as numpy [B, k]; nothing may be written behind the outputs."""
    import torch

    B, n = mat.shape
    sc = torch.from_numpy(ref.padded(mat)).cuda()
    ids = torch.full((B * k + guard,), -7, dtype=torch.int32, device="cuda")
    top = torch.full((B * k + guard,), 9, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    st = stream or torch.cuda.current_stream()
    r.topk_scores_dev(sc.data_ptr(), sc.shape[1], B, k, ids.data_ptr(), top.data_ptr(), st.cuda_stream)
    st.synchronize()
    assert (ids[B * k:] == -7).all() and (top[B * k:] == 9).all()
    return ids[:B * k].cpu().numpy().reshape(B, k), top[:B * k].cpu().numpy().reshape(B, k)


def check(pkg, mat, k, runner=None):
    gi, gt = select(runner or _runner(pkg, mat.shape[1]), mat, k)
    wi, wt = ref.topk_ref(mat, k)
    assert np.array_equal(gt, wt)
    assert np.array_equal(gi, wi)
    return gi, gt


@pytest.mark.parametrize("k", [17, 32, 33, 64, 100, 128])
def test_random_bytes(gpu_pkg, k):
    check(gpu_pkg, ref.random_bytes(70001, 32), k)  # five chunks, the last with 4465 rows


def test_narrow_range(gpu_pkg):
    gi, gt = check(gpu_pkg, ref.narrow_range(70001, 4), 100)
    assert (gt == 203).all()


def test_rare_top(gpu_pkg):
    gi, gt = check(gpu_pkg, ref.rare_top(70001, 4), 100)
    assert (gt[:, :37] == 1).all() and (gt[:, 37:] == 0).all()


@pytest.mark.parametrize("value", [255, 0, 7])
def test_constant_matrix(gpu_pkg, value):
    gi, gt = check(gpu_pkg, ref.constant(32769, 3, value), 128)
    assert (gi == np.arange(128)).all() and (gt == value).all()


@pytest.mark.parametrize("n", [1, 3, 100, 127])
def test_fewer_rows_than_k(gpu_pkg, n):
    for mat in (ref.constant(n, 3, 0), ref.random_bytes(n, 3)):
        gi, gt = check(gpu_pkg, mat, 128)
        assert (gi[:, n:] == -1).all() and (gt[:, n:] == 0).all() and (np.sort(gi[:, :n], axis=1) == np.arange(n)).all()


@pytest.mark.parametrize("n", [16383, 16384, 16385, 32768, 32769])
def test_chunk_boundaries(gpu_pkg, n):
    mat, ks = ref.boundaries(n)
    for k in sorted(set(ks.values()) | {k + 1 for k in ks.values()}):  # and one row further
        check(gpu_pkg, mat, k)


def test_thread_and_wave_boundaries(gpu_pkg):
    mat = ref.inner_runs()
    for k in ref.INNER_KS:
        check(gpu_pkg, mat, k)


@pytest.mark.parametrize("k", [17, 128])
def test_all_levels(gpu_pkg, k):
    check(gpu_pkg, ref.levels_cycle(40000, 3), k)
    mat, rows = ref.spread_top()
    gi, gt = check(gpu_pkg, mat, k)
    assert np.array_equal(gi[0], rows[::-1][:k])


def test_scratch_reuse(gpu_pkg):
    """One runner at k = 128, 17, 100 on different matrices, then twice at the same k: no stale histogram or position."""
    n = 70001
    r = _runner(gpu_pkg, n)
    for mat, k in ((ref.random_bytes(n, 32), 128), (ref.narrow_range(n, 4), 17), (ref.rare_top(n, 4), 100),
                   (ref.random_bytes(n, 32, seed=1), 100), (ref.random_bytes(n, 32), 100), (ref.random_bytes(n, 32), 100)):
        check(gpu_pkg, mat, k, runner=r)


def test_large(gpu_pkg):
    n = 1000003  # 62 chunks
    assert gpu_pkg.q8_wide_plan(n, 100)[0] == 62
    check(gpu_pkg, ref.random_bytes(n, 4), 100, runner=_runner(gpu_pkg, n, dim=1))


def test_more_chunks_than_one_tile(gpu_pkg):
    """66 chunks: the cut kernel walks a value's chunk counts in register tiles of 64 chunks, and the positions of the second
    tile carry on from the first.  70 ones with at least one in every chunk: the last of them lie past chunk 63."""
    n = 65 * ref.CHUNK + 5
    assert gpu_pkg.q8_wide_plan(n, 100)[0] == 66
    r = _runner(gpu_pkg, n, dim=1)
    gi, gt = check(gpu_pkg, ref.rare_top(n, 2, ones=70), 100, runner=r)
    assert (gt[:, :70] == 1).all() and (gt[:, 70:] == 0).all() and (gi[:, 69] >= 65 * ref.CHUNK).all()
    check(gpu_pkg, ref.random_bytes(n, 2), 128, runner=r)
    check(gpu_pkg, ref.levels_cycle(n, 2), 128, runner=r)


def test_small_k_on_a_raw_buffer(gpu_pkg):
    """k <= 16 through topk_scores_dev: the existing kernels on the caller's buffer and leading dimension."""
    for mat in (ref.random_bytes(70001, 32), ref.narrow_range(70001, 4)):
        for k in (1, 16):
            check(gpu_pkg, mat, k)


def test_refusals(gpu_pkg):
    import torch

    n = 1000
    r = _runner(gpu_pkg, n)
    L = gpu_pkg.lib()
    sc = torch.zeros((4 * 1088 + 64,), dtype=torch.uint8, device="cuda")
    ids = torch.full((4 * 128,), -7, dtype=torch.int32, device="cuda")
    top = torch.full((4 * 128,), 9, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    p, i, t = sc.data_ptr(), ids.data_ptr(), top.data_ptr()
    assert p % 16 == 0
    call = lambda ptr, ld, B, k: L.vs_q8_topk_scores_dev(r._h, ptr, ld, B, k, i, t, None)
    assert call(p, 1024, 4, 100) == 0
    assert call(p, 1000, 4, 100) == -1   # not a multiple of 64
    assert call(p, 1056, 4, 100) == -1   # a multiple of 32 only
    assert call(p, 960, 4, 100) == -1    # ld < n
    assert call(p + 8, 1024, 4, 100) == -1  # misaligned
    assert call(p, 1024, 4, 0) == -1
    assert call(p, 1024, 4, 129) == -5
    assert call(p, 1024, 33, 100) == -1
    assert call(None, 1024, 4, 100) == -1
    q = np.ones((4, 4), dtype=np.float32)
    for k, status in ((0, -1), (-3, -1), (129, -5)):
        with pytest.raises(gpu_pkg.VSearchError) as e:
            r.search_topk(q, k)
        assert e.value.status == status
    assert L.vs_q8_search_topk_dev(r._h, p, 1, 33, 129, i, t, None) == -1  # B before k
    assert L.vs_q8_search_topk_dev(r._h, p, 0, 4, 100, i, t, None) == -1
    assert L.vs_q8_search_topk_dev(r._h, p, 1, 4, 129, i, t, None) == -5
    assert L.vs_q8_search_topk(r._h, p, -1, 100, i, t) == -1
    with pytest.raises(gpu_pkg.VSearchError) as e:  # vs_q8_search keeps its limit
        r.search(q, 17)
    assert e.value.status == -5
    torch.cuda.synchronize()
    assert (ids[4 * 100:] == -7).all() and (top[4 * 100:] == 9).all()


# ------------------------------------------------------------------ through the runner

def _calibrated(base, queries):
    """Min-max encodings the way a converter run with calibration inputs would choose them (as in test_gpu_q8.py)."""
    in_scale = float(queries.max()) / 255.0
    w_scale = float(base.max()) / 255.0
    ip_max = float((queries[:8].astype(np.float64) @ base[:: max(1, len(base) // 4096)].astype(np.float64).T).max())
    return in_scale, w_scale, 1.05 * ip_max / 255.0


def _case(pkg, dim):
    """(runner with id_offset 1000, 1056 queries, executeBatchRaw of all of them), once per dimension."""
    if dim not in _cases:
        if dim == 128:
            base, q = pkg.synth_sift(20037, seed=71), pkg.synth_sift(33 * 32, seed=72)
        else:
            rng = np.random.default_rng(dim)
            base = rng.integers(0, 256, size=(5000, dim)).astype(np.float32)
            base *= rng.uniform(0.1, 1.0, size=(5000, 1)).astype(np.float32)
            q = rng.integers(0, 256, size=(33 * 32, dim)).astype(np.float32)
        enc = _calibrated(base, q)
        r = pkg.Q8Runner(base, enc[0], enc[1], 0, enc[2], id_offset=1000)
        raw = np.concatenate([r.executeBatchRaw(q[i:i + 32]) for i in range(0, len(q), 32)])
        assert len(np.unique(raw)) > 16
        raw.setflags(write=False)
        _cases[dim] = (r, q, raw)
    return _cases[dim]


@pytest.mark.parametrize("dim", [128, 96])
@pytest.mark.parametrize("k", [17, 100, 128])
def test_search_topk_host(gpu_pkg, dim, k):
    r, q, raw = _case(gpu_pkg, dim)
    ids, top = r.search_topk(q[:70], k)  # two full batches and one of 6
    assert ids.dtype == np.int32 and top.dtype == np.uint8 and ids.shape == (70, k) and top.shape == (70, k)
    wi, wt = ref.topk_ref(raw[:70], k, id_offset=1000)
    assert np.array_equal(top, wt) and np.array_equal(ids, wi)


@pytest.mark.parametrize("dim", [128, 96])
@pytest.mark.parametrize("B", [1, 17, 32])
def test_search_topk_dev_on_a_stream(gpu_pkg, dim, B):
    """33 batches in one call (two quantiser groups) on a stream of the caller's own, ids with id_offset."""
    import torch

    nb, k, guard = 33, 100, 64
    r, q, raw = _case(gpu_pkg, dim)
    qd = torch.from_numpy(q[:nb * B].copy()).cuda()
    ids = torch.full((nb * B * k + guard,), -7, dtype=torch.int32, device="cuda")
    top = torch.full((nb * B * k + guard,), 9, dtype=torch.uint8, device="cuda")
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        r.search_topk_dev(qd.data_ptr(), nb, B, k, ids.data_ptr(), top.data_ptr(), stream.cuda_stream)
    stream.synchronize()
    n = nb * B * k
    assert (ids[n:] == -7).all() and (top[n:] == 9).all()
    wi, wt = ref.topk_ref(raw[:nb * B], k, id_offset=1000)
    assert np.array_equal(top[:n].cpu().numpy().reshape(-1, k), wt)
    assert np.array_equal(ids[:n].cpu().numpy().reshape(-1, k), wi)


@pytest.mark.parametrize("k", [5, 16])
def test_small_k_is_the_existing_call(gpu_pkg, k):
    import torch

    r, q, raw = _case(gpu_pkg, 96)
    ids, top = r.search_topk(q[:70], k)
    ids0, top0 = r.search(q[:70], k)
    assert np.array_equal(ids, ids0) and np.array_equal(top, top0)
    wi, wt = ref.topk_ref(raw[:70], k, id_offset=1000)
    assert np.array_equal(ids, wi) and np.array_equal(top, wt)
    qd = torch.from_numpy(q[:64].copy()).cuda()
    oi = [torch.zeros((64, k), dtype=torch.int32, device="cuda") for _ in range(2)]
    ot = [torch.zeros((64, k), dtype=torch.uint8, device="cuda") for _ in range(2)]
    torch.cuda.synchronize()
    s0 = torch.cuda.current_stream().cuda_stream
    r.search_topk_dev(qd.data_ptr(), 2, 32, k, oi[0].data_ptr(), ot[0].data_ptr(), s0)
    r.search_dev(qd.data_ptr(), 2, 32, k, oi[1].data_ptr(), ot[1].data_ptr(), s0)
    torch.cuda.synchronize()
    assert torch.equal(oi[0], oi[1]) and torch.equal(ot[0], ot[1])
    assert np.array_equal(oi[0].cpu().numpy(), ids0[:64])


def test_cli_q8_mode_at_k_100(gpu_pkg, tmp_path):
    """`vsearch_bf <ctx> <queries> <results_dir> <backend> <documents> 100 32 --q8=...` on 96-d files against the oracle."""
    rng = np.random.default_rng(51)
    base = rng.integers(0, 256, size=(5000, 96)).astype(np.float32)
    base *= rng.uniform(0.1, 1.0, size=(5000, 1)).astype(np.float32)
    q = rng.integers(0, 256, size=(70, 96)).astype(np.float32)
    i_s, w_s, o_s = (np.float32(x) for x in _calibrated(base, q))
    gpu_pkg.write_fvecs(str(tmp_path / "docs.fvecs"), base)
    gpu_pkg.write_fvecs(str(tmp_path / "queries.fvecs"), q)
    exe = os.path.join(os.path.dirname(gpu_pkg.LIB_PATH), "vsearch_bf")
    assert os.path.exists(exe), "vsearch_bf not built (make -C hai-25-rag-on-edge_amd/csrc all)"
    env = dict(os.environ)
    env["LD_LIBRARY_PATH"] = gpu_pkg.hip_runtime_dir() + os.pathsep + env.get("LD_LIBRARY_PATH", "")
    enc = f"--q8={float(i_s)!r},{float(w_s)!r},0,{float(o_s)!r}"
    args = [exe, "ctx.bin", "queries.fvecs", "out", "libQnnHtp.so", "docs.fvecs", "100", "32", enc]
    r = subprocess.run(args, cwd=tmp_path, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    raw = oracle.q8_scores(base, q, i_s, w_s, 0, o_s)
    oid, otop = oracle.q8_topk(raw, 100)
    ids, scores = oracle.parse_results_txt(str(tmp_path / "out" / "results.txt"))
    assert np.array_equal(np.array(ids), oid)
    want = np.array([[float(f"{np.float32(t) * o_s:.4f}") for t in row] for row in otop])
    assert np.array_equal(np.array(scores), want)
    m = open(tmp_path / "out" / "metrics.txt").read()
    for needle in ("UFIXED_POINT_8", "Number of queries: 70", "Number of documents: 5000", "Dimension: 96", "Top-K: 100"):
        assert needle in m, needle
    args[6] = "129"  # refused by the argument check, with a message
    r = subprocess.run(args, cwd=tmp_path, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 1 and "top_k must be in 1..128" in r.stderr
