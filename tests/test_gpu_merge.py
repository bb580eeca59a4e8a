"""vs_topk_merge_dev called directly, every output bit for bit against the numpy restatement of its contract
(tests/merge_ref.py): both merge kernels, every ranking branch of the compacting kernel and every instantiation of the
list-head kernel, on inputs the searches never hand it -- signed and zero distances of either sign, -inf, a subnormal,
ties across lists, lists of unequal length with every kind of end the contract names and winning garbage behind it,
kout != kin, padded strides.

Every call checks 64 guard words behind each output buffer and that the inputs are unchanged, and every test asserts on
the CPU the precondition of the branch it is about: the kernel through vs_topk_merge_plan, the pooled entries M counted
from the inputs, and -- where the order in which the compacting kernel pools the entries is determined (G <= 64: one
wave owns every list and its lanes append in ascending order) -- the number of entries its filter sets aside.  The
results are asserted exactly whichever branch runs."""
import functools

import numpy as np
import pytest

import merge_ref as ref

pytestmark = pytest.mark.gpu

GUARD = 64
SENT = 0x5A5A5A5A
INF = np.float32(np.inf)
# a second value set: some thousand distinct distances of either sign, so that most entries differ
WIDE = np.unique(np.concatenate([np.random.default_rng(1).standard_normal(3000).astype(np.float32),
                                 np.array([-0.0, 0.0, -np.inf], dtype=np.float32)]))


def launch(pkg, dbuf, ibuf, G, B, kin, kout, stride_g=0, want_flags=True, own_stream=False):
    """One call on flat buffers (float32 / int32).  Returns (dist bits [B, kout] uint32, ids [B, kout], flags [B] or None)."""
    import torch
    dev = torch.device("cuda:0")
    dbits = np.ascontiguousarray(dbuf, dtype=np.float32).reshape(-1).view(np.int32)  # bits: NaN payloads and zero signs travel
    ibuf = np.ascontiguousarray(ibuf, dtype=np.int32).reshape(-1)
    span = (G - 1) * (stride_g or B * kin) + B * kin
    assert len(dbits) >= span and len(ibuf) >= span  # the call reads nothing past its buffers
    dd, ii = torch.from_numpy(dbits).to(dev), torch.from_numpy(ibuf).to(dev)
    od = torch.full((B * kout + GUARD,), SENT, dtype=torch.int32, device=dev)
    oi = torch.full((B * kout + GUARD,), SENT, dtype=torch.int32, device=dev)
    fl = torch.full((B + GUARD,), SENT, dtype=torch.int32, device=dev)
    if own_stream:
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        assert s.cuda_stream != torch.cuda.current_stream().cuda_stream
    else:
        s = torch.cuda.current_stream()
    pkg.topk_merge_dev(dd.data_ptr(), ii.data_ptr(), G, B, kin, kout, od.data_ptr(), oi.data_ptr(),
                       fl.data_ptr() if want_flags else 0, s.cuda_stream, stride_g=stride_g)
    s.synchronize()
    torch.cuda.synchronize()
    od, oi, fl = od.cpu().numpy(), oi.cpu().numpy(), fl.cpu().numpy()
    for name, buf, n in (("dists", od, B * kout), ("ids", oi, B * kout), ("flags", fl, B if want_flags else 0)):
        assert np.all(buf[n:] == SENT), f"{name}: written past the output"
    assert np.array_equal(dd.cpu().numpy(), dbits) and np.array_equal(ii.cpu().numpy(), ibuf), "the inputs were written"
    return od[:B * kout].view(np.uint32).reshape(B, kout), oi[:B * kout].reshape(B, kout), fl[:B] if want_flags else None


def assert_same(got, want, what=""):
    gd, gi, gf = got
    wd, wi, wf = want[0], want[1], want[2]
    for name, g, w in (("ids", gi, wi), ("dists", gd, ref.bits(wd))):
        bad = np.argwhere(g != w)
        assert not len(bad), (f"{what}{name} differ at (query, slot) {bad[0].tolist()} (+{len(bad) - 1} more): got "
                              f"{g[tuple(bad[0])]:#x}, want {w[tuple(bad[0])]:#x}; row got {gi[bad[0][0]][:12].tolist()} want "
                              f"{wi[bad[0][0]][:12].tolist()}")
    if gf is not None:
        assert np.array_equal(gf, wf), f"{what}flags differ at queries {np.flatnonzero(gf != wf)[:8].tolist()}"


def check(pkg, d, i, kout, lpt, **kw):
    """d, i [G, B, kin] dense -> plan precondition, launch, exact comparison.  Returns (reference, M per query)."""
    G, B, kin = d.shape
    assert pkg.topk_merge_plan(G, kin, kout) == (lpt, ref.CAP, ref.TRACK)
    want = ref.merge_ref(d, i, kout)
    assert_same(launch(pkg, d, i, G, B, kin, kout, **kw), want, f"G={G} kin={kin} kout={kout}: ")
    return want


# ------------------------------------------------------------------------------------------------ the compacting kernel
FILLS = (0, 1, 63, 64, 65, 255, 256, 257, 600, 1024, 1025, 1500, 2500, 4096)
SHAPES = ((64, 64), (8, 17), (256, 16))  # (64, 64) is 4096 entries: the last shape on this kernel


@functools.lru_cache(maxsize=None)
def compact_data(G, kin):
    """Three groups of queries at every fill level the shape holds, so that the queries of one launch take different
    branches: the small value set with mixed list ends, mostly distinct distances, and one kind of end per query."""
    fills = [M for M in FILLS if M < G * kin] + [G * kin]
    kinds = ("nan", "inf", "neg", "pad")
    parts = [ref.generate(11, G, kin, fills),
             ref.generate(12, G, kin, fills, values=WIDE),
             ref.generate(13, G, kin, fills, ends=[kinds[b % 4] for b in range(len(fills))])]
    d = np.ascontiguousarray(np.concatenate([p[0] for p in parts], axis=1))
    i = np.ascontiguousarray(np.concatenate([p[1] for p in parts], axis=1))
    routes = None
    if G <= 64:
        routes = [ref.append_order(d[:, b, :], i[:, b, :]) for b in range(d.shape[1])]
    d.setflags(write=False)
    i.setflags(write=False)
    return d, i, fills * 3, routes


def required_routes(G, kin, kout):
    """The branches a launch of compact_data(G, kin) at kout must contain, from the fill levels and kout per the kernel
    source.  The lists are sorted, so the first 256 pooled entries are the heads of the lists and the filter's threshold
    is close to the true kout-th entry: about kout entries survive, one wave at 1 entry per lane (kout = 63, 64: a few
    more than 64, 4 per lane).  The larger survivor sets are built in test_compact_kernel_filter_sizes."""
    if G * kin < 4096:
        return {"epl1", "epl4"}
    if kout > 64:
        return {"epl1", "epl4", "epl16", "rounds"}
    if G > 64:
        return {"epl1", "epl4", "filter"}
    return {"epl1", "epl4", "filter-epl4" if kout >= 63 else "filter-epl1"}


@pytest.mark.parametrize("kout", [1, 5, 16, 63, 64, 65, 100, 128, 300])
@pytest.mark.parametrize("G,kin", SHAPES)
def test_compact_kernel_every_route(gpu_pkg, G, kin, kout):
    """One launch of ~40 queries at fill levels M = 0, 1, 63 .. 256 (one wave, 1 or 4 entries per lane), 257 .. 1024
    (kout <= 64: the filter; above: 16 per lane, the 64-at-a-time flush over several groups, at kout = 300 and M = 257 a
    padded tail) and 1025 .. 4096 (kout <= 64: the filter on a large set; above: the workgroup-wide rounds)."""
    d, i, fills, pooled = compact_data(G, kin)
    want = check(gpu_pkg, d, i, kout, 0)
    M = want[3]
    assert M.tolist() == fills
    seen = set()
    for b in range(d.shape[1]):
        S = None
        if pooled is not None and M[b] > 256 and kout <= 64:
            S = ref.filter_survivors(*pooled[b], kout)
        seen.add(ref.compact_route(int(M[b]), kout, S))
    assert required_routes(G, kin, kout) <= seen, sorted(seen)
    assert (kout > 1) == bool(want[2].any()) and not want[2].all()  # ties across lists are there (none at kout 1), not everywhere


def filter_data(below, short):
    """A query whose filter sets aside a chosen number of entries, for the append order of G <= 64.  64 lists of 64:
    lists 16 .. 63 hold only large values, list 0 three tiny ones, then X = +0.0, then larger ones, lists 1 .. 15 four tiny
    ones, then `below` values not above X (-0.0 with smaller ids among them: ties at the threshold), then larger ones.
    The first 256 pooled entries are the first four of every list; 63 of them are tiny and the 64th smallest is X, so
    at kout = 64 the survivors are 64 + 15 * below, and at kout = 63 the 63 tiny ones.  short: lists 16 .. 63 hold 4
    entries and lists 0 .. 15 52, 1024 entries in all (a filter that gives up then falls through to the one-wave ranking
    instead of the workgroup rounds)."""
    G, kin = 64, 64
    n_big, n_small = (4, 52) if short else (64, 64)
    d = np.full((G, 1, kin), INF, dtype=np.float32)
    i = np.full((G, 1, kin), -1, dtype=np.int32)
    ids = iter(np.random.default_rng(5).permutation(20000).tolist())
    rng = np.random.default_rng(6)
    above = np.array([1.0, 2.0], dtype=np.float32)
    for g in range(G):
        if g >= 16:
            vals = rng.choice(np.array([50.0, 60.0, 3e38], dtype=np.float32), size=n_big)
        elif g == 0:
            vals = np.concatenate([[-8.0, -8.0, -8.0, 0.0], rng.choice(above, size=n_small - 4)])
        else:  # the tiny ones tie with each other across lists; so do the values below X
            vals = np.concatenate([[-8.0] * 4, rng.choice(np.array([-4.0, -2.0, -1.0, -0.0], dtype=np.float32), size=below),
                                   rng.choice(above, size=n_small - 4 - below)])
        vals = np.sort(vals.astype(np.float32))
        own = np.array([next(ids) for _ in vals])
        for v in np.unique(vals):  # ascending ids within equal distances
            own[vals == v] = np.sort(own[vals == v])
        if g == 0:
            own[3] = 30000  # X = (+0.0, the largest id): the -0.0 entries of lists 1 .. 15 tie with it and are not above it
        d[g, 0, :len(vals)], i[g, 0, :len(vals)] = vals, own
    return d, i


@pytest.mark.parametrize("below,short,route", [(8, False, "filter-epl4"), (8, True, "filter-epl4"), (24, False, "filter-epl16"),
                                               (24, True, "filter-epl16"), (60, False, "overflow-rounds"),
                                               (48, True, "overflow-epl16")])
def test_compact_kernel_filter_sizes(gpu_pkg, below, short, route):
    """kout = 64: 184 survivors (one wave, 4 per lane), 424 (16 per lane), and 964 / 784 -- more than the filter keeps
    (512), so it gives up and the query goes to the workgroup-wide rounds (M = 4096) or to the one-wave ranking at 16
    entries per lane (short, M = 1024).  kout = 63 on the same data: the threshold is the last tiny value and exactly 63
    entries survive.  WHICH branch runs rests on the append order of the pooling (one wave owns the 64 lists and its
    lanes append in ascending order); the results asserted here are exact whatever the order."""
    d, i = filter_data(below, short)
    cd, ci = ref.append_order(d[:, 0, :], i[:, 0, :])
    lens = ref.list_lengths(d[:, 0, :], i[:, 0, :])
    first = np.sort(np.concatenate([d[g, 0, :4] for g in range(64)]))
    assert lens.min() >= 4 and np.array_equal(np.sort(cd[:256]), first)  # the first 256 pooled: four of every list
    assert first[62] == -8.0 and first[63] == 0.0 and first[64] > 0.0     # X = 0.0 is their 64th smallest
    M = len(cd)
    assert M == (1024 if short else 4096)
    S64, S63 = ref.filter_survivors(cd, ci, 64), ref.filter_survivors(cd, ci, 63)
    assert (S64, S63) == (64 + 15 * below, 63)
    assert ref.compact_route(M, 64, S64) == route and ref.compact_route(M, 63, S63) == "filter-epl1"
    for kout in (64, 63):
        want = check(gpu_pkg, d, i, kout, 0)
        assert want[3].tolist() == [M] and want[2].tolist() == [1]


# ------------------------------------------------------------------------------------------------ the list-head kernel
HEADS = ((1, 256, 17), (2, 257, 16), (4, 600, 7), (8, 1100, 4), (16, 2100, 2), (32, 4097, 1), (64, 8193, 1), (64, 16384, 1))
ONE_LIST = 137


@functools.lru_cache(maxsize=None)
def head_data(G, kin, B):
    """B = 1: one query with three quarters of the slots filled, winners spread over many lists.  B = 3: a half-filled
    query, one of 7 entries whose other lists end in (+inf, an id) with garbage behind, and an empty one.  At (256, 17)
    the first query has no -inf and list 137 holds its 17 best: that list's head advances to the list's end."""
    one = (G, kin) == (256, 17)
    if B == 1:
        d, i = ref.generate(21 + G, G, kin, [G * kin * 3 // 4], values=ref.VALUES[1:] if one else ref.VALUES)
    else:
        d0, i0 = ref.generate(31 + G, G, kin, [G * kin // 2], values=ref.VALUES[1:] if one else ref.VALUES)
        d1, i1 = ref.generate(41 + G, G, kin, [7, 0], ends=["inf", "pad"])
        d, i = np.concatenate([d0, d1], axis=1), np.concatenate([i0, i1], axis=1)
    if one:
        d[ONE_LIST, 0, :] = np.float32(-3e38) + np.float32(1e37) * (np.arange(kin) // 2)  # pairs of equal distances
        i[ONE_LIST, 0, :] = 500000 + np.arange(kin)
    d, i = np.ascontiguousarray(d), np.ascontiguousarray(i)
    d.setflags(write=False)
    i.setflags(write=False)
    return d, i


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("kout", [1, 16, 100])
@pytest.mark.parametrize("lpt,G,kin", HEADS)
def test_head_kernel_every_instantiation(gpu_pkg, lpt, G, kin, kout, B):
    """One shape per merge_kernel<LPT>, the LPT asserted through the plan: (4097, 1) is the first shape past the compacting
    kernel, (16384, 1) the last the kernel takes."""
    d, i = head_data(G, kin, B)
    assert G * kin > ref.CAP
    want = check(gpu_pkg, d, i, kout, lpt)
    od, oi, fl, M = want
    lens = ref.list_lengths(d, i)
    assert abs(M[0] - G * kin * (3 if B == 1 else 2) // 4) <= kin and lens[:, 0].min() < lens[:, 0].max()
    # winners spread over many lists, and (kout = 100 > kin) lists that run out before kout
    owner = {int(x): g for g in range(G) for x in i[g, 0, :lens[g, 0]]}
    lists_of_winners = [owner[int(x)] for x in oi[0] if x >= 0]
    if (G, kin) == (256, 17):
        assert lists_of_winners[:17] == [ONE_LIST] * min(17, kout)  # ... and past its end: the 18th comes from elsewhere
        assert kout <= 17 or lists_of_winners[17] != ONE_LIST
    else:
        assert len(set(lists_of_winners)) >= min(kout, 8)
    if B == 3:
        assert M.tolist()[1:] == [7, 0]
        assert np.all(oi[2] == -1) and np.all(od[2] == INF) and fl[2] == 0     # the empty query
        assert np.all(oi[1, 7:] == -1) and np.all(oi[1, :min(7, kout)] >= 0)   # fewer than kout entries in all


# ------------------------------------------------------------------------------------------------ addressing and options
@pytest.mark.parametrize("lpt,G,kin,B", [(0, 8, 17, 5), (0, 64, 64, 2), (2, 257, 16, 3)])
def test_padded_stride_dense_stride_null_flags_and_own_stream(gpu_pkg, lpt, G, kin, B):
    fills = [G * kin // 3, G * kin, 7, 0, G * kin // 2][:B]
    d, i = ref.generate(51 + G, G, kin, fills)
    kout = 20
    want = check(gpu_pkg, d, i, kout, lpt)  # stride_g = 0: the dense layout
    assert want[3].tolist() == fills
    assert_same(launch(gpu_pkg, d, i, G, B, kin, kout, stride_g=B * kin), want, "explicit dense stride: ")
    # groups B*kin + 37 apart, NaN and winning finite garbage in the gaps
    stride = B * kin + 37
    dbuf = np.full((G, stride), np.float32(-9e30), dtype=np.float32)
    dbuf[:, B * kin::2] = np.nan
    ibuf = (2000000 + np.arange(G * stride, dtype=np.int32)).reshape(G, stride)
    dbuf[:, :B * kin] = d.reshape(G, B * kin)
    ibuf[:, :B * kin] = i.reshape(G, B * kin)
    assert_same(launch(gpu_pkg, dbuf, ibuf, G, B, kin, kout, stride_g=stride), want, "padded stride: ")
    got = launch(gpu_pkg, d, i, G, B, kin, kout, want_flags=False)
    assert got[2] is None
    assert_same(got, want, "flags_dev = NULL: ")
    assert_same(launch(gpu_pkg, d, i, G, B, kin, kout, own_stream=True), want, "caller's stream: ")
    assert_same(launch(gpu_pkg, dbuf, ibuf, G, B, kin, kout, stride_g=stride, own_stream=True), want, "caller's stream, padded: ")


@pytest.mark.parametrize("B", [1, 1500])
def test_one_query_and_a_grid_of_1500(gpu_pkg, B):
    G, kin = 8, 17
    fills = np.random.default_rng(61).integers(0, G * kin + 1, size=B).tolist()
    fills[0] = G * kin
    d, i = ref.generate(62, G, kin, fills)
    for kout in (17, 40):
        want = check(gpu_pkg, d, i, kout, 0)
        assert want[3].tolist() == fills
    G, kin = 300, 14  # the list-head kernel on the same grid
    fills = np.random.default_rng(63).integers(0, 400, size=B).tolist()
    d, i = ref.generate(64, G, kin, fills, values=WIDE)
    assert check(gpu_pkg, d, i, 9, 2)[3].tolist() == fills


@pytest.mark.parametrize("lpt,G,kin,M", [(0, 64, 64, 400), (0, 64, 64, 1100), (2, 300, 16, 400)])
def test_flag_window_is_the_first_256_outputs(gpu_pkg, lpt, G, kin, M):
    """kout = 300, all distances distinct but one pair: a tie at outputs 270 / 271 is outside the window (flag 0), one at
    100 / 101 inside (flag 1), one at 255 / 256 straddles its end (flag 0); on the one-wave ranking (M = 400), the
    workgroup rounds (M = 1100) and the list-head kernel."""
    values = (np.arange(M, dtype=np.float32) - 50) / 4  # M distinct values, drawn without repeats below
    cases = []
    for pos in (270, 100, 255, None):
        d, i = ref.generate(71, G, kin, [M], values=values, ends="pad")
        lens = ref.list_lengths(d, i)
        live = np.arange(kin) < lens[:, :, None]
        d[live] = np.random.default_rng(72).permutation(values)  # distinct; then sorted within each list again
        for g in range(G):
            d[g, 0, :lens[g, 0]] = np.sort(d[g, 0, :lens[g, 0]])
        if pos is not None:  # the entry of rank pos + 1 takes the distance of rank pos: still ascending in its list
            rank = np.sort(d[live])
            d[d == rank[pos + 1]] = rank[pos]
            (g0, _, j0), (g1, _, j1) = np.argwhere(d == rank[pos])
            if g0 == g1 and i[g0, 0, j0] > i[g1, 0, j1]:  # both in one list: ascending ids within the tie
                i[g0, 0, j0], i[g1, 0, j1] = i[g1, 0, j1], i[g0, 0, j0]
        cases.append((d, i))
    d = np.concatenate([c[0] for c in cases], axis=1)
    i = np.concatenate([c[1] for c in cases], axis=1)
    want = check(gpu_pkg, d, i, 300, lpt)
    assert want[3].tolist() == [M] * 4 and want[2].tolist() == [0, 1, 0, 0]
    for b, pos in enumerate((270, 100, 255)):
        assert want[0][b, pos] == want[0][b, pos + 1] and len(np.unique(want[0][b])) == 299
    assert check(gpu_pkg, d, i, 257, lpt)[2].tolist() == [0, 1, 0, 0]
    assert check(gpu_pkg, d, i, 101, lpt)[2].tolist() == [0, 0, 0, 0]
    assert check(gpu_pkg, d, i, 102, lpt)[2].tolist() == [0, 1, 0, 0]
