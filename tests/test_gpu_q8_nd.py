"""GPU parity of the UFIXED_POINT_8 runner at vector dimensions other than 128 (vs_q8_create_nd): every score matrix and
every top-k bit for bit against oracle.q8_scores / oracle.q8_topk, which take the dimension as a parameter.  The
arithmetic leaves no freedom: ip is exact in int32, then one int -> float conversion (inexact above 2^24, which
2048-d reaches), one multiplication, one addition."""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle

pytestmark = pytest.mark.gpu

N0 = 4099  # 64 full groups of 64 rows and a ragged one of 3


def _calibrated(base, queries):
    """Min-max encodings the way a converter run with calibration inputs would choose them (as in test_gpu_q8.py)."""
    in_scale = float(queries.max()) / 255.0
    w_scale = float(base.max()) / 255.0
    ip_max = float((queries[:8].astype(np.float64) @ base[:: max(1, len(base) // 4096)].astype(np.float64).T).max())
    return in_scale, w_scale, 1.05 * ip_max / 255.0


def _rows(n, B, dim, seed):
    """Integer-valued rows, each scaled by a factor in [0.1, 1] of its own so that the scores spread; byte queries."""
    rng = np.random.default_rng(seed)
    base = rng.integers(0, 256, size=(n, dim)).astype(np.float32)
    base *= rng.uniform(0.1, 1.0, size=(n, 1)).astype(np.float32)
    q = rng.integers(0, 256, size=(B, dim)).astype(np.float32)
    return base, q


@functools.lru_cache(maxsize=None)
def _case(n, dim):
    """(base, 32 queries, encodings, the oracle's [32 x n] matrix), computed once per shape and never modified."""
    base, q = _rows(n, 32, dim, 1000 * dim + n)
    enc = _calibrated(base, q)
    want = oracle.q8_scores(base, q, enc[0], enc[1], 0, enc[2])
    if n >= N0:  # the encodings use the range: not a trivial comparison
        assert len(np.unique(want)) > 16 and want.max() > 128
    for a in (base, q, want):
        a.setflags(write=False)
    return base, q, enc, want


def _runner(gpu_pkg, base, enc, off=0, **kw):
    return gpu_pkg.Q8Runner(base, enc[0], enc[1], off, enc[2], **kw)


@pytest.mark.parametrize("dim", [1, 15, 17, 63, 64, 65, 127, 129, 192, 200, 256, 960, 2047, 2048])
def test_score_matrix_over_dimensions(gpu_pkg, dim):
    base, q, enc, want = _case(N0, dim)
    with _runner(gpu_pkg, base, enc) as r:
        assert (r.getNumDocs(), r.getDim(), r.getBatchSize()) == (N0, dim, 32)
        assert r.getOutputScale() == np.float32(enc[2])
        got = r.executeBatchRaw(q)
    assert got.dtype == np.uint8 and got.shape == (32, N0)
    assert np.array_equal(got, want)


@pytest.mark.parametrize("n", [1, 63, 64, 65])
def test_few_rows(gpu_pkg, n):
    base, q, enc, want = _case(n, 200)
    with _runner(gpu_pkg, base, enc) as r:
        assert np.array_equal(r.executeBatchRaw(q), want)


@pytest.mark.parametrize("dim", [200, 2048])
@pytest.mark.parametrize("B", [1, 16, 17, 31])
def test_short_batches(gpu_pkg, dim, B):
    """B <= 16 takes the kernel with one query block, B > 16 the one with two; rows past B are zero queries."""
    base, q, enc, want = _case(N0, dim)
    with _runner(gpu_pkg, base, enc) as r:
        got = r.executeBatchRaw(q[:B])
    assert got.shape == (B, N0) and np.array_equal(got, want[:B])


def test_conversion_above_2_24(gpu_pkg):
    """At 2048-d the accumulator passes 2^24, where float32(ip) rounds: the kernel must convert the complete integer once."""
    base, q, enc, want = _case(N0, 2048)
    q8 = oracle.q8_quantize(q, enc[0]).astype(np.int64)
    w8 = oracle.q8_quantize_weights(base, enc[1], 0).astype(np.int64)
    ip = q8 @ w8.T
    big = ip > 2 ** 24
    assert ip.max() < 2 ** 27 and big.any()
    inexact = big & (ip.astype(np.float32).astype(np.int64) != ip)
    assert inexact.any()
    with _runner(gpu_pkg, base, enc) as r:
        got = r.executeBatchRaw(q)
    assert np.array_equal(got[inexact], want[inexact]) and np.array_equal(got, want)


@pytest.mark.parametrize("dim", [65, 200])
def test_weight_offset_and_quantiser_lanes(gpu_pkg, dim):
    base, q, _, _ = _case(N0, dim)
    q = q[:9] * np.float32(0.4)
    q[0, :4] = [-5.0, np.nan, 1e9, 0.33]  # saturation / NaN lanes of the quantiser (QnnRunner.cpp:50-54)
    shifted = base - np.float32(40.0)     # asymmetric weights: real = scale * (q + offset), offset < 0
    w_s = float(shifted.max() - shifted.min()) / 255.0
    off = int(round(float(shifted.min()) / w_s))
    assert -255 <= off < 0
    o_s = 1.05 * float((np.nan_to_num(q[1:]).astype(np.float64) @ np.maximum(shifted, 0).astype(np.float64).T).max()) / 255.0
    want = oracle.q8_scores(shifted, q, 0.5, w_s, off, o_s)
    assert len(np.unique(want)) > 8
    with gpu_pkg.Q8Runner(shifted, 0.5, w_s, off, o_s) as r:
        assert r.encodings().weight_offset == off
        got = r.executeBatchRaw(q)
    assert np.array_equal(got, want)


def test_default_encodings_at_96(gpu_pkg):
    rng = np.random.default_rng(96)
    # unit-norm non-negative vectors scaled into the runner's hard-coded input range (0.6627451 * 255 = 169)
    base = np.abs(rng.standard_normal((N0, 96))).astype(np.float32)
    base *= 120.0 / np.linalg.norm(base, axis=1, keepdims=True)
    q = np.abs(rng.standard_normal((32, 96))).astype(np.float32) * 60.0
    with gpu_pkg.Q8Runner(base) as r:  # enc = NULL: QnnRunner.cpp:490-521 scales, weights min-max over n * dim values
        e = r.encodings()
        assert e.input_scale == oracle.Q8_INPUT_SCALE and e.output_scale == oracle.Q8_OUTPUT_SCALE
        assert e.weight_scale == np.float32(base.max()) / np.float32(255.0) and e.weight_offset == 0
        assert r.getDim() == 96
        got = r.executeBatchRaw(q)
    want = oracle.q8_scores(base, q, e.input_scale, e.weight_scale, 0, e.output_scale)
    assert np.array_equal(got, want)
    assert len(np.unique(want)) > 8


def test_execute_dev_addressing(gpu_pkg):
    """ld = n_pad: one 16-byte store per lane and query block; ld = n + 3: the byte loop.  Nothing past a row's end."""
    import torch

    base, q, enc, want = _case(N0, 200)
    B, n_pad = 17, (N0 + 63) // 64 * 64
    qd = torch.from_numpy(q[:B].copy()).cuda()
    st = torch.cuda.current_stream().cuda_stream
    with _runner(gpu_pkg, base, enc) as r:
        for ld in (n_pad, N0 + 3):
            out = torch.full((B * ld + 16,), 7, dtype=torch.uint8, device="cuda")
            r.execute_dev(qd.data_ptr(), B, out.data_ptr(), ld, st)
            torch.cuda.synchronize()
            got = out[: B * ld].view(B, ld).cpu().numpy()
            assert np.array_equal(got[:, :N0], want[:B])
            assert np.all(got[:, N0:] == 7) and np.all(out[B * ld:].cpu().numpy() == 7)


@pytest.mark.parametrize("k", [1, 5, 16])
def test_search_two_chunks(gpu_pkg, k):
    base, q, enc, want = _case(20037, 384)  # two top-k chunks, the second one short
    with _runner(gpu_pkg, base, enc, id_offset=1000) as r:
        ids, top = r.search(q, k)
    oid, otop = oracle.q8_topk(want, k)
    assert np.array_equal(top, otop) and np.array_equal(ids, oid + 1000)


def test_search_dev_many_batches(gpu_pkg):
    """33 batches of 31 queries: two quantiser groups, batch strides of B * dim floats in, B * k out."""
    import torch

    n, dim, nb, B, k = 2000, 200, 33, 31, 5
    base, q = _rows(n, nb * B, dim, 77)
    enc = _calibrated(base, q)
    want = oracle.q8_scores(base, q, enc[0], enc[1], 0, enc[2])
    oid, otop = oracle.q8_topk(want, k)
    qd = torch.from_numpy(q).cuda()
    ids = torch.full((nb * B, k), -7, dtype=torch.int32, device="cuda")
    top = torch.zeros((nb * B, k), dtype=torch.uint8, device="cuda")
    with _runner(gpu_pkg, base, enc) as r:
        r.search_dev(qd.data_ptr(), nb, B, k, ids.data_ptr(), top.data_ptr(), torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
    assert np.array_equal(top.cpu().numpy(), otop) and np.array_equal(ids.cpu().numpy(), oid)


def test_k_limits(gpu_pkg):
    base, q, enc, _ = _case(N0, 200)
    with _runner(gpu_pkg, base, enc) as r:
        with pytest.raises(gpu_pkg.VSearchError) as e:
            r.search(q, 17)
        assert e.value.status == -5
    with _runner(gpu_pkg, base[:3], enc) as r:  # fewer rows than k: the tail is (-1, 0)
        ids, top = r.search(q[:3], 5)
        raw = r.executeBatchRaw(q[:3])
    oid, otop = oracle.q8_topk(raw, 5)
    assert np.array_equal(raw, oracle.q8_scores(base[:3], q[:3], enc[0], enc[1], 0, enc[2]))
    assert np.array_equal(ids, oid) and np.array_equal(top, otop) and np.all(ids[:, 3:] == -1) and np.all(top[:, 3:] == 0)


_TOGGLE_SCRIPT = r"""
import ctypes as C, sys
import numpy as np
sys.path.insert(0, sys.argv[1])
import __graft_entry__ as ge
pkg = ge.load_package()
z = np.load(sys.argv[2])
base = np.ascontiguousarray(z["base"], dtype=np.float32)
r = pkg.Q8Runner.__new__(pkg.Q8Runner)
r._h = C.c_void_p()
enc = pkg.Q8Encodings(float(z["enc"][0]), float(z["enc"][1]), 0, float(z["enc"][2]))
rc = pkg.lib().vs_q8_create_nd(base.ctypes.data_as(C.c_void_p), base.shape[0], 128, C.byref(enc), 0, 0, C.byref(r._h))
assert rc == 0, rc
raw = r.executeBatchRaw(z["q"])
ids, top = r.search(z["q"], 5)
r.close()
np.save(sys.argv[3] + "_raw.npy", raw)
np.save(sys.argv[3] + "_ids.npy", ids)
np.save(sys.argv[3] + "_top.npy", top)
print("TOGGLE_OK")
"""


def test_toggle_at_128(gpu_pkg, tmp_path):
    """vs_q8_create_nd at dim 128 is vs_q8_create's runner; with VSEARCH_Q8_ND_FORCE=1 (a child process: the variable is
    read at creation) the general kernels run at 128, with the same bytes out."""
    base = gpu_pkg.synth_sift(N0, seed=61)
    q = gpu_pkg.synth_sift(32, seed=62)
    enc = _calibrated(base, q)
    want = oracle.q8_scores(base, q, enc[0], enc[1], 0, enc[2])
    oid, otop = oracle.q8_topk(want, 5)
    assert "VSEARCH_Q8_ND_FORCE" not in os.environ
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = str(tmp_path / "in.npz")
    np.savez(src, base=base, q=q, enc=np.array(enc, dtype=np.float64))
    for force in (None, "1"):
        e = dict(os.environ)
        if force:
            e["VSEARCH_Q8_ND_FORCE"] = force
        dst = str(tmp_path / ("forced" if force else "default"))
        r = subprocess.run([sys.executable, "-c", _TOGGLE_SCRIPT, root, src, dst], env=e, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and "TOGGLE_OK" in r.stdout, (r.stdout[-400:], r.stderr[-1200:])
    d_raw, f_raw = np.load(str(tmp_path / "default_raw.npy")), np.load(str(tmp_path / "forced_raw.npy"))
    assert np.array_equal(d_raw, f_raw) and np.array_equal(d_raw, want)
    for name, ref in (("ids", oid), ("top", otop)):
        d, f = np.load(str(tmp_path / f"default_{name}.npy")), np.load(str(tmp_path / f"forced_{name}.npy"))
        assert np.array_equal(d, f) and np.array_equal(d, ref)
    with gpu_pkg.Q8Runner(base, *enc[:2], 0, enc[2]) as r:  # vs_q8_create itself, in this process
        assert np.array_equal(r.executeBatchRaw(q), want)


def test_cli_q8_mode_at_96(gpu_pkg, tmp_path):
    """`vsearch_bf <ctx> <queries> <results_dir> <backend> <documents> <k> [batch] --q8=...` on 96-d files: results.txt holds
    the oracle's ids and score8 * output_scale with 4 decimals (main.cpp:244-246), metrics.txt the dimension."""
    base, q = _rows(5000, 70, 96, 51)
    i_s, w_s, o_s = (np.float32(x) for x in _calibrated(base, q))
    gpu_pkg.write_fvecs(str(tmp_path / "docs.fvecs"), base)
    gpu_pkg.write_fvecs(str(tmp_path / "queries.fvecs"), q)
    exe = os.path.join(os.path.dirname(gpu_pkg.LIB_PATH), "vsearch_bf")
    assert os.path.exists(exe), "vsearch_bf not built (make -C hai-25-rag-on-edge_amd/csrc all)"
    env = dict(os.environ)
    env["LD_LIBRARY_PATH"] = gpu_pkg.hip_runtime_dir() + os.pathsep + env.get("LD_LIBRARY_PATH", "")
    enc = f"--q8={float(i_s)!r},{float(w_s)!r},0,{float(o_s)!r}"
    r = subprocess.run([exe, "ctx.bin", "queries.fvecs", "out", "libQnnHtp.so", "docs.fvecs", "5", "32", enc], cwd=tmp_path, env=env,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    raw = oracle.q8_scores(base, q, i_s, w_s, 0, o_s)
    oid, otop = oracle.q8_topk(raw, 5)
    ids, scores = oracle.parse_results_txt(str(tmp_path / "out" / "results.txt"))
    assert np.array_equal(np.array(ids), oid)
    want = np.array([[float(f"{np.float32(t) * o_s:.4f}") for t in row] for row in otop])
    assert np.array_equal(np.array(scores), want)
    m = open(tmp_path / "out" / "metrics.txt").read()
    for needle in ("UFIXED_POINT_8", "Number of queries: 70", "Number of documents: 5000", "Dimension: 96", "Batch size: 32", "Top-K: 5"):
        assert needle in m, needle
