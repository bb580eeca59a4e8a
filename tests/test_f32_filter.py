"""The bf16 prefilter of the fp32 streaming scan (scan_f32f_kernel): its error bound on the CPU, and on the
GPU the same ids, distances and tie flags as scan_f32s_kernel (VSEARCH_F32_FILTER=0), bit for bit, on data where bf16
rounding matters, on ill-scaled data, and at 1 M rows against the oracle."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:  # (also run as a script: the A/B worker below)
    sys.path.insert(0, ROOT)
import oracle  # noqa: E402


# ------------------------------------------------------------------------------------------------ CPU: the bound
def _bf16(x):
    """float32 -> bf16 (round to nearest even) -> float32."""
    u = np.asarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) >> 16
    return (u << 16).astype(np.uint32).view(np.float32)


def _chain_f32(q, b):
    """scan_f32s_kernel's dot: fmaf steps in the order of its MFMA chain, k = 16 c + 4 g + i for c, i, g."""
    order = [16 * c + 4 * g + i for c in range(8) for i in range(4) for g in range(4)]
    acc = np.zeros(q.shape[0], dtype=np.float32)
    for k in order:  # fmaf: the product and sum exactly in float64 (a 24 x 24-bit product is exact there), one rounding
        acc = (q[:, k].astype(np.float64) * b[:, k].astype(np.float64) + acc.astype(np.float64)).astype(np.float32)
    return acc


def test_filter_bound_covers_bf16_error(pkg):
    """|S_fl - S'| <= E for the library's E, S' the exact sum of the bf16 products (the MFMA's own accumulation error is
    the g16 term of E, checked here against the rest of the bound's slack), on random and adversarial vectors."""
    L = pkg.lib()
    rng = np.random.default_rng(3)
    n = 4000
    cases = {
        "gauss": (rng.standard_normal((n, 128)), rng.standard_normal((n, 128))),
        "mixed": (rng.standard_normal((n, 128)) * 10.0 ** rng.uniform(-3, 3, (n, 128)),
                  rng.standard_normal((n, 128)) * 10.0 ** rng.uniform(-3, 3, (n, 128))),
        "sift": (rng.integers(0, 219, (n, 128)), rng.integers(0, 219, (n, 128))),
    }
    # adversarial: every value half an ulp of bf16 away from its rounding (the largest relative bf16 error), with the
    # signs of q and b agreeing so that the errors add up
    m = rng.uniform(1, 2, (n, 128)).astype(np.float32).view(np.uint32)
    m = ((m & np.uint32(0xFFFF0000)) | np.uint32(0x7FFF)).view(np.float32)
    s = np.sign(rng.standard_normal((n, 128)))
    cases["halfulp"] = (m * s, m[::-1] * s)
    # one large pair among tiny ones, near the ends of the well-scaled range
    big = np.full((n, 128), 2.0 ** -50)
    big[:, 7] = 2.0 ** 40 * (1 + 2.0 ** -9)
    cases["range"] = (big, big[::-1])
    for name, (q, b) in cases.items():
        q = q.astype(np.float32)
        b = b.astype(np.float32)
        qp, bp = _bf16(q), _bf16(b)
        s_fl = _chain_f32(q, b).astype(np.float64)
        s_p = (qp.astype(np.float64) * bp.astype(np.float64)).sum(1)  # exact products, float64 sum
        nq = np.linalg.norm(q.astype(np.float64), axis=1)
        nqp = np.linalg.norm(qp.astype(np.float64), axis=1)
        eq = np.linalg.norm(q.astype(np.float64) - qp, axis=1)
        nb = np.linalg.norm(b.astype(np.float64), axis=1)
        eb = np.linalg.norm(b.astype(np.float64) - bp, axis=1)
        nbp = np.linalg.norm(bp.astype(np.float64), axis=1)
        bmax, emax, bpmax = nb.max(), eb.max(), nbp.max()
        E = np.array([L.vs_f32_filter_bound(eq[i], nq[i], nqp[i], bmax, emax, bpmax) for i in range(n)])
        err = np.abs(s_fl - s_p)
        assert (err <= E).all(), (name, float((err / E).max()))
        # the bound is not vacuous: on integer data (bf16-exact) it is the rounding terms alone
        if name == "sift":
            assert (eq == 0).all() and emax == 0
            assert (E < 2.0 ** -14 * nq * bmax).all()


# ------------------------------------------------------------------------------------------------ GPU: A/B subprocesses
def _cases(n_rows):
    rng = np.random.default_rng(11)
    out = {}
    g = rng.standard_normal((n_rows, 128)).astype(np.float32)
    out["gauss"] = (g, (g[rng.integers(0, n_rows, 1024)] + 0.3 * rng.standard_normal((1024, 128))).astype(np.float32))
    mixed = (g * 10.0 ** rng.uniform(-2, 2, (n_rows, 1))).astype(np.float32)
    out["mixed"] = (mixed, (mixed[rng.integers(0, n_rows, 1024)] * 1.01).astype(np.float32))
    lb = g.view(np.uint32)
    lb = ((lb & np.uint32(0xFFFF0000)) | np.uint32(0x7FFF)).view(np.float32)  # largest bf16 rounding error
    out["lowbits"] = (lb, (lb[rng.integers(0, n_rows, 1024)] + 0.05 * rng.standard_normal((1024, 128))).astype(np.float32))
    # near-duplicates: 12 rows per query at distances spaced by 2^-20 relative, straddling its 5th / 6th best
    q = rng.standard_normal((1024, 128)).astype(np.float32)
    nd = g.copy()
    u = rng.standard_normal((1024, 128))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    for m in range(12):
        nd[1024 * m: 1024 * (m + 1)] = (q + (1.0 + m * 2.0 ** -20) * u).astype(np.float32)
    out["neardup"] = (nd, q)
    return out


def _worker(argv):
    """python test_f32_filter.py <out.npz> <n_rows> <what>: the searches of one A/B side, in a process of its own."""
    import torch
    import __graft_entry__ as ge

    pkg = ge.load_package()
    out, n_rows, what = argv[0], int(argv[1]), argv[2]
    dev = torch.device("cuda", 0)
    res = {}
    if what == "ab":
        todo = [(name, base, q, metric) for name, (base, q) in _cases(n_rows).items() for metric in (0, 1)]
    else:  # ill-scaled: rows (the shard keeps scan_f32s_kernel) or queries (+inf bound: the overflow fallback)
        rng = np.random.default_rng(5)
        base = pkg.synth_sift(n_rows, seed=9)
        q = pkg.synth_sift(1024, seed=10)
        q_tiny = q.copy()
        q_tiny[::7, 3] = 2.0 ** -70       # a non-zero magnitude below 2^-60 in every 7th query
        b_tiny = base.copy()
        b_tiny[rng.integers(0, n_rows, 5), 9] = 2.0 ** -70
        todo = [("q_tiny", base, q_tiny, 0), ("b_tiny", b_tiny, q, 0), ("q_tiny_ip", base, q_tiny, 1)]
    for name, base, q, metric in todo:
        qd = torch.from_numpy(np.ascontiguousarray(q)).to(dev)
        with pkg.BruteForceIndex(base, metric=metric) as idx:
            idx.set_precision(1)
            for nb in (4, 20, 32):
                o_d = torch.zeros((nb * 32, 6), dtype=torch.float32, device=dev)
                o_i = torch.full((nb * 32, 6), -7, dtype=torch.int32, device=dev)
                fl = torch.full((nb * 32,), -7, dtype=torch.int32, device=dev)
                idx.search_dev_multi(qd.data_ptr(), nb, 32, 5, o_i.data_ptr(), o_d.data_ptr(), fl.data_ptr(),
                                     torch.cuda.current_stream().cuda_stream)
                torch.cuda.synchronize()
                key = f"{name}_m{metric}_nb{nb}"
                res[key + "_i"] = o_i.cpu().numpy()
                res[key + "_d"] = o_d.cpu().numpy()
                res[key + "_f"] = fl.cpu().numpy()
    np.savez(out, **res)


def _run_side(tmp_path, flt, n_rows, what):
    out = str(tmp_path / f"{what}_{flt}.npz")
    env = dict(os.environ, VSEARCH_F32_FILTER=str(flt))
    subprocess.run([sys.executable, os.path.abspath(__file__), out, str(n_rows), what], env=env, check=True, timeout=900)
    return dict(np.load(out))


@pytest.mark.gpu
def test_filter_equals_fp32_kernel_bit_for_bit(gpu_pkg, tmp_path):
    """Gaussian, mixed-magnitude, worst-case-rounding and near-duplicate data, 300 K rows, 4 / 20 / 32 batches, both
    metrics: ids, distances and tie flags with the filter equal those of scan_f32s_kernel."""
    a = _run_side(tmp_path, 1, 300_000, "ab")
    b = _run_side(tmp_path, 0, 300_000, "ab")
    assert a.keys() == b.keys() and len(a) == 4 * 2 * 3 * 3
    for k in a:
        assert np.array_equal(a[k], b[k]), k


@pytest.mark.gpu
def test_filter_ill_scaled_data_exact(gpu_pkg, tmp_path):
    """Rows or queries outside [2^-60, 2^60]: exact through scan_f32s_kernel (rows) or the overflow fallback (queries)."""
    n_rows = 300_000
    a = _run_side(tmp_path, 1, n_rows, "ill")
    b = _run_side(tmp_path, 0, n_rows, "ill")
    for k in a:
        assert np.array_equal(a[k], b[k]), k
    rng = np.random.default_rng(5)
    base = gpu_pkg.synth_sift(n_rows, seed=9)
    q = gpu_pkg.synth_sift(1024, seed=10)
    q_tiny = q.copy()
    q_tiny[::7, 3] = 2.0 ** -70
    b_tiny = base.copy()
    b_tiny[rng.integers(0, n_rows, 5), 9] = 2.0 ** -70
    for name, bb, qq in (("q_tiny", base, q_tiny), ("b_tiny", b_tiny, q)):
        oi, od = oracle.search_bf(bb, qq, 5)
        gi, gd, f = a[f"{name}_m0_nb32_i"], a[f"{name}_m0_nb32_d"], a[f"{name}_m0_nb32_f"]
        keep = f == 0
        assert np.array_equal(gd[:, :5], od)
        assert np.array_equal(gi[keep, :5], oi[keep])


@pytest.mark.gpu
@pytest.mark.parametrize("nb", [32, 20])
def test_sift1m_filter_against_oracle(gpu_pkg, nb):
    """1 M synthetic SIFT rows, 32 and 20 batches of 32 queries through the prefilter: k + 1 best against the oracle."""
    import torch
    base = gpu_pkg.synth_sift(1_000_000, seed=20251205)
    q = gpu_pkg.synth_sift(nb * 32, seed=777 + nb)
    oi, od = oracle.search_bf(base, q, 5)
    dev = torch.device("cuda", 0)
    qd = torch.from_numpy(q).to(dev)
    with gpu_pkg.BruteForceIndex(base) as idx:
        idx.set_precision(1)
        o_d = torch.zeros((nb * 32, 6), dtype=torch.float32, device=dev)
        o_i = torch.full((nb * 32, 6), -7, dtype=torch.int32, device=dev)
        fl = torch.full((nb * 32,), -7, dtype=torch.int32, device=dev)
        idx.search_dev_multi(qd.data_ptr(), nb, 32, 5, o_i.data_ptr(), o_d.data_ptr(), fl.data_ptr(),
                             torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
    f = fl.cpu().numpy()
    keep = f == 0
    assert keep.mean() > 0.9
    gi, gd = o_i.cpu().numpy(), o_d.cpu().numpy()
    assert np.array_equal(gi[keep, :5], oi[keep]) and np.array_equal(gd[:, :5], od)


if __name__ == "__main__":
    _worker(sys.argv[1:])
