"""The L2 hot test of the bf16 prefilter with the row norm in the MFMA's C operand (scan_f32f_kernel): on the
CPU, that the exported bound th2 admits every (row, query) the exact scan's hot test admits, under the accumulation model
the bound assumes; on the GPU, the same ids, distances and tie flags as scan_f32s_kernel (VSEARCH_F32_FILTER=0), bit for
bit, at the sizes where the kernel takes another path, with the prefilter's counters showing that the prefilter and not
the fallback scan behind it produced them."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:  # (also run as a script: the A/B worker below)
    sys.path.insert(0, ROOT)
import oracle  # noqa: E402

F32 = np.float32


# ------------------------------------------------------------------------------------------------ CPU: the bound
def _bf16(x):
    """float32 -> bf16 (round to nearest even) -> float32."""
    u = np.asarray(x, dtype=F32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) >> 16
    return (u << 16).astype(np.uint32).view(F32)


def _chain_f32(q, b):
    """scan_f32s_kernel's dot: fmaf steps in the order of its MFMA chain, k = 16 c + 4 g + i for c, i, g."""
    order = [16 * c + 4 * g + i for c in range(8) for i in range(4) for g in range(4)]
    acc = np.zeros(q.shape[0], dtype=F32)
    for k in order:
        acc = (q[:, k].astype(np.float64) * b[:, k].astype(np.float64) + acc.astype(np.float64)).astype(F32)
    return acc


def _trunc23(x):
    """Toward zero at 23 significant bits: a relative error below 2^-22 per operation, the unit roundoff the bound's g16
    assumes for the MFMA's additions (round to nearest in fp32 is 2^-24; truncation, twice over, 2^-22)."""
    m, e = np.frexp(x)
    return np.ldexp(np.trunc(m * 2.0 ** 23) / 2.0 ** 23, e)


def _accumulate(terms, group=1):
    """Sum of the columns of `terms` left to right, every addition truncated (_trunc23); group > 1: groups of that many
    columns are summed first (truncated additions too), then accumulated."""
    n, m = terms.shape
    acc = np.zeros(n)
    for j0 in range(0, m, group):
        part = terms[:, j0].copy()
        for j in range(j0 + 1, min(j0 + group, m)):
            part = _trunc23(part + terms[:, j])
        acc = part if j0 == 0 else _trunc23(acc + part)
    return acc


# the prefilter's k order: k-step s of the MFMA holds k = 32 s + 16 (j >> 2) + 4 g + (j & 3) for lane group g, element j
_CHAIN_K = [32 * s + 16 * (j >> 2) + 4 * g + (j & 3) for s in range(4) for g in range(4) for j in range(8)]


def _families(n):
    rng = np.random.default_rng(3)
    fam = {
        "gauss": (rng.standard_normal((n, 128)), rng.standard_normal((n, 128))),
        "mixed": (rng.standard_normal((n, 128)) * 10.0 ** rng.uniform(-3, 3, (n, 128)),
                  rng.standard_normal((n, 128)) * 10.0 ** rng.uniform(-3, 3, (n, 128))),
        "sift": (rng.integers(0, 219, (n, 128)), rng.integers(0, 219, (n, 128))),
    }
    m = rng.uniform(1, 2, (n, 128)).astype(F32).view(np.uint32)
    m = ((m & np.uint32(0xFFFF0000)) | np.uint32(0x7FFF)).view(F32)
    s = np.sign(rng.standard_normal((n, 128)))
    fam["halfulp"] = (m * s, m[::-1] * s)
    big = np.full((n, 128), 2.0 ** -50)
    big[:, 7] = 2.0 ** 40 * (1 + 2.0 ** -9)
    fam["range"] = (big, big[::-1])
    # norm dominated: the C operand bn / 2 (about 160 000) is hundreds of times the spread of the sums it is added to; half
    # of the queries are perturbed rows, whose distance is hundreds of times smaller than either norm
    b = rng.standard_normal((n, 128)) + 50.0
    q = rng.standard_normal((n, 128)) + 50.0
    q[::2] = b[::2] + 0.3 * rng.standard_normal((n // 2 + n % 2, 128))
    fam["normdom"] = (q, b)
    return {k: (q.astype(F32), b.astype(F32)) for k, (q, b) in fam.items()}


def test_cnorm_test_admits_what_the_exact_test_admits(pkg):
    """Old hot test RN(bn - 2 S_fl) < thr true  =>  S'' > th2 true, for S'' accumulated from c0 = -bn / 2 and the 128 bf16
    products in five orders with every addition truncated, over a grid of tau around each pair's own distance.  No
    allowance.  And the bound is not vacuous: on integer data the distance threshold widens by less than
    2^-13 (||q|| bmax + bmax^2)."""
    L = pkg.lib()
    n = 600
    for name, (q, b) in _families(n).items():
        q64, b64 = q.astype(np.float64), b.astype(np.float64)
        qp, bp = _bf16(q).astype(np.float64), _bf16(b).astype(np.float64)
        bn = (b64 * b64).sum(1).astype(F32)  # the stored norms: fp32 numbers near ||b||^2, the same in both tests
        qn = (q64 * q64).sum(1).astype(F32)
        c0 = (F32(-0.5) * bn).astype(np.float64)
        assert np.array_equal(c0, -0.5 * bn.astype(np.float64))  # halving is exact
        prod = qp * bp  # exact: 8 x 8-bit significands
        seq = np.concatenate([c0[:, None], prod], axis=1)
        chain = prod[:, _CHAIN_K]
        s2 = {
            "exact": seq.sum(1),
            "sequential": _accumulate(seq),
            "reversed": _accumulate(seq[:, ::-1]),
            "groups4": _accumulate(seq, group=4),
            "chain_c0_first": _accumulate(np.concatenate([c0[:, None], chain], axis=1)),
            "chain_c0_last": _accumulate(np.concatenate([chain, c0[:, None]], axis=1)),
        }
        s_fl = _chain_f32(q, b)
        nq = np.linalg.norm(q64, axis=1)
        nqp = np.linalg.norm(qp, axis=1)
        eq = np.linalg.norm(q64 - qp, axis=1)
        bmax = np.linalg.norm(b64, axis=1).max()
        emax = np.linalg.norm(b64 - bp, axis=1).max()
        bpmax = np.linalg.norm(bp, axis=1).max()
        E = np.array([L.vs_f32_filter_bound(eq[i], nq[i], nqp[i], bmax, emax, bpmax) for i in range(n)], dtype=F32)
        cn = F32(L.vs_f32_filter_cnorm(float(bn.max())))
        # the exact scan's distance of the pair, and tau on a grid around it: at it, one ulp either side, further out
        d = (qn.astype(np.float64) + bn.astype(np.float64) - 2.0 * s_fl.astype(np.float64)).astype(F32)
        taus = [d, np.nextafter(d, F32(np.inf)), np.nextafter(d, F32(-np.inf))]
        for rel in (2.0 ** -22, 2.0 ** -18, 2.0 ** -12, 2.0 ** -6, 0.5):
            taus += [(d * F32(1 + rel)).astype(F32), (d * F32(1 - rel)).astype(F32)]
        old_true = 0
        for tau in taus:
            # stream_l2_thr in fp32 (any float thr serves the implication; this is the one the kernels form)
            thr = ((tau - qn) + F32(9.5367431640625e-7) * (qn + np.abs(tau))).astype(F32)
            lhs = (bn.astype(np.float64) - 2.0 * s_fl.astype(np.float64)).astype(F32)  # fmaf(-2, S_fl, bn): one rounding
            old = lhs < thr
            th2 = np.array([L.vs_f32_filter_th2(float(thr[i]), float(E[i]), float(cn)) for i in range(n)], dtype=F32)
            old_true += int(old.sum())
            for order, v in s2.items():
                new = v.astype(F32).astype(np.float64) > th2 if order != "exact" else v > th2
                assert new[old].all(), (name, order, int((old & ~new).sum()))
            if name == "sift":
                widening = -2.0 * th2.astype(np.float64) - thr.astype(np.float64)
                assert (widening > 0).all()
                assert (widening < 2.0 ** -13 * (nq * bmax + bmax * bmax)).all(), float(widening.max())
        assert old_true > n  # the grid straddles the test: it is true for a good part of it


def test_th2_masks(pkg):
    """E = +inf or an infinite bound admits everything, a bound of -inf nothing (host arithmetic of the library)."""
    L = pkg.lib()
    inf = float("inf")
    assert L.vs_f32_filter_th2(1.0, inf, 0.0) == -inf
    assert L.vs_f32_filter_th2(inf, 1.0, 1.0) == -inf
    assert L.vs_f32_filter_th2(-inf, 1.0, 1.0) == inf
    assert L.vs_f32_filter_th2(0.0, 0.0, 0.0) < 0.0
    assert L.vs_f32_filter_th2(-8.0, 1.0, 0.5) < 4.0 - 1.0 * (1 + 2.0 ** -7) - 0.5
    assert L.vs_f32_filter_th2(-8.0, 1.0, 0.5) > 2.49


# ------------------------------------------------------------------------------------------------ GPU: A/B subprocesses
N_ROWS = 70_003  # just above the 65 536 rows a seeded launch needs; no multiple of 64 or 16: the last unit and tile are partial
# The norm-dominated rows are gauss + this offset.  The error bound E of bf16 rounding grows with the norms (about 0.002 bn)
# while the distances between the rows stay those of the gaussians (256 +- 23): at an offset of 50 (and from about 8 on)
# 2 E exceeds that spread, every row is a candidate of every query and the launch overflows into the fallback scan, before
# this change and after it alike (measured at 50: 70 003 candidates per query, overflow).  At 4 the sweep writes 182 - 186
# candidates per query of which 13.3 - 13.7 survive the recheck (inner product: 39 - 40 and 19), against 2048 list entries
# per query and 1024 per wave buffer.
NORMDOM_OFFSET = 4.0
NBS = (4, 5, 17, 32)  # column blocks per wave: 1, 2 (with dead column blocks), 8, 8
BS = (32, 20)         # 20: dead columns in every second column block


def _sift(n, seed):
    return np.random.default_rng(seed).integers(0, 219, (n, 128)).astype(F32)


def _gpu_cases():
    rng = np.random.default_rng(11)
    out = {"sift": (_sift(N_ROWS, 21), _sift(1024, 22))}
    g = rng.standard_normal((N_ROWS, 128)).astype(F32)
    pick = rng.integers(0, N_ROWS, 1024)
    out["gauss"] = (g, (g[pick] + 0.3 * rng.standard_normal((1024, 128))).astype(F32))
    lb = g.view(np.uint32)
    lb = ((lb & np.uint32(0xFFFF0000)) | np.uint32(0x7FFF)).view(F32)  # largest bf16 rounding error
    out["lowbits"] = (lb, (lb[pick] + 0.05 * rng.standard_normal((1024, 128))).astype(F32))
    nd = (g + F32(NORMDOM_OFFSET)).astype(F32)
    out["normdom"] = (nd, (nd[pick] + 0.3 * rng.standard_normal((1024, 128))).astype(F32))
    # near-duplicates: 12 rows per query at distances spaced by 2^-20 relative, straddling its 5th / 6th best
    q = rng.standard_normal((1024, 128)).astype(F32)
    dup = g.copy()
    u = rng.standard_normal((1024, 128))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    for m in range(12):
        dup[1024 * m: 1024 * (m + 1)] = (q + (1.0 + m * 2.0 ** -20) * u).astype(F32)
    out["neardup"] = (dup, q)
    # the fallback: every 7th query has a component below 2^-60, so its E is +inf, every row passes, the buffers overflow
    q_tiny = out["sift"][1].copy()
    q_tiny[::7, 3] = 2.0 ** -70
    out["qtiny"] = (out["sift"][0], q_tiny)
    return out


def _worker(argv):
    """python test_f32_filter_cnorm.py <out.npz>: the searches of one A/B side, in a process of its own."""
    import torch
    import __graft_entry__ as ge

    pkg = ge.load_package()
    dev = torch.device("cuda", 0)
    res = {}
    filtered = os.environ.get("VSEARCH_F32_FILTER") != "0"
    for name, (base, q) in _gpu_cases().items():
        qd = torch.from_numpy(np.ascontiguousarray(q)).to(dev)
        for metric in (0, 1):
            if name == "qtiny" and metric == 1:
                continue
            with pkg.BruteForceIndex(base, metric=metric) as idx:
                idx.set_precision(1)
                for nb in (NBS if name != "qtiny" else (32,)):
                    for B in (BS if name != "qtiny" else (32,)):
                        o_d = torch.zeros((nb * B, 6), dtype=torch.float32, device=dev)
                        o_i = torch.full((nb * B, 6), -7, dtype=torch.int32, device=dev)
                        fl = torch.full((nb * B,), -7, dtype=torch.int32, device=dev)
                        idx.search_dev_multi(qd.data_ptr(), nb, B, 5, o_i.data_ptr(), o_d.data_ptr(), fl.data_ptr(),
                                             torch.cuda.current_stream().cuda_stream)
                        torch.cuda.synchronize()
                        key = f"{name}_m{metric}_nb{nb}_B{B}"
                        res[key + "_i"] = o_i.cpu().numpy()
                        res[key + "_d"] = o_d.cpu().numpy()
                        res[key + "_f"] = fl.cpu().numpy()
                        if filtered:
                            res[key + "_stats"] = np.array(idx.filter_stats(reset=True), dtype=np.int64)
    np.savez(argv[0], **res)


_SIDES = {}


def _side(tmp_path_factory, flt):
    if flt not in _SIDES:  # both sides once per session, shared by the tests below and left unchanged
        out = str(tmp_path_factory.mktemp("cnorm") / f"side{flt}.npz")
        env = dict(os.environ, VSEARCH_F32_FILTER=str(flt))
        subprocess.run([sys.executable, os.path.abspath(__file__), out], env=env, check=True, timeout=600)
        _SIDES[flt] = dict(np.load(out))
    return _SIDES[flt]


def _search_keys():
    keys = [f"{name}_m{metric}_nb{nb}_B{B}" for name in ("sift", "gauss", "lowbits", "normdom", "neardup")
            for metric in (0, 1) for nb in NBS for B in BS]
    return keys + ["qtiny_m0_nb32_B32"]


@pytest.mark.gpu
def test_cnorm_filter_equals_fp32_kernel_bit_for_bit(gpu_pkg, tmp_path_factory):
    """70 003 rows, 4 / 5 / 17 / 32 batches of 32 and of 20 queries, both metrics, five data sets (and the fallback's):
    ids, distances and tie flags with the prefilter equal those of scan_f32s_kernel."""
    a = _side(tmp_path_factory, 1)
    b = _side(tmp_path_factory, 0)
    keys = _search_keys()
    assert len(keys) == 5 * 2 * 4 * 2 + 1
    for k in keys:
        for s in ("_i", "_d", "_f"):
            assert np.array_equal(a[k + s], b[k + s]), k + s
        assert (a[k + "_i"][:, :5] >= 0).all(), k


@pytest.mark.gpu
def test_cnorm_results_come_from_the_prefilter(gpu_pkg, tmp_path_factory):
    """Every prefilter-side case: one prefilter launch per call, no overflow, and at least the k + 1 = 6 rows under each
    query's bound survive the recheck on average (a bound made too permissive by mistake would overflow the candidate
    buffers and let the exact fallback scan produce the results).

    The norm-dominated set was asked for at an offset of 50; there every row is a candidate of every query (70 003 written
    per query, overflow raised, 0 kept) because the bf16 error bound E alone exceeds the spread of the distances, so the
    offset is 4 (NORMDOM_OFFSET): 182 - 186 written and 13.3 - 13.7 kept per query for L2, 39 - 40 and 19 for inner
    product, no overflow.  The other sets: 13 - 22 written, 13 - 18 kept per query."""
    a = _side(tmp_path_factory, 1)
    for k in _search_keys():
        if k.startswith("qtiny"):
            continue
        launches, overflowed, written, kept = (int(x) for x in a[k + "_stats"])
        nq = a[k + "_i"].shape[0]
        print(f"{k}: launches {launches} overflowed {overflowed} written/query {written / nq:.1f} kept/query {kept / nq:.1f}")
        assert launches == 1, k
        assert overflowed == 0, k
        assert kept >= 6 * nq, (k, kept / nq)
        assert written >= kept, k


@pytest.mark.gpu
def test_cnorm_fallback_still_exact(gpu_pkg, tmp_path_factory):
    """Queries with a 2^-70 component have E = +inf: th2 = -inf, every row is a candidate, the buffers overflow
    (out[1] > 0), and the fallback scan behind the sweep gives the exact result."""
    a = _side(tmp_path_factory, 1)
    k = "qtiny_m0_nb32_B32"
    assert a[k + "_stats"][0] == 1 and a[k + "_stats"][1] > 0
    base, q = _gpu_cases()["qtiny"]
    oi, od = oracle.search_bf(base, q, 5)
    keep = a[k + "_f"] == 0
    assert np.array_equal(a[k + "_d"][:, :5], od)
    assert np.array_equal(a[k + "_i"][keep, :5], oi[keep])


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["sift", "normdom"])
def test_cnorm_against_oracle(gpu_pkg, tmp_path_factory, name):
    """The integer and the norm-dominated L2 cases at 32 batches against the CPU oracle."""
    a = _side(tmp_path_factory, 1)
    base, q = _gpu_cases()[name]
    oi, od = oracle.search_bf(base, q, 5, dot_order="chain")  # (the fp32 kernels' own order: the rows are not integers)
    k = f"{name}_m0_nb32_B32"
    keep = a[k + "_f"] == 0
    assert keep.mean() > 0.5
    assert np.array_equal(a[k + "_d"][:, :5], od)
    assert np.array_equal(a[k + "_i"][keep, :5], oi[keep])


if __name__ == "__main__":
    _worker(sys.argv[1:])
