// vs_ivf_nd_wide.hip -- wide k (17 <= k <= 128) on a general IVF index, fp32 rows, squared L2 or inner product (gfx950;
// DESIGN 4.6c).  Under inner product (IvfNdParams::metric, the IP instantiations) a distance below is the score -(q.v).
//
// A launch group first runs the list-major pipeline of vs_ivf_nd.hip at KCAP 16: part[(query * nprobe + rank) * 16] holds
// every probed list's 16 best by (distance, row).  Then
//   ivf_nd_wide_bound_kernel : per query, tau = the k-th smallest finite distance in its partial lists (+inf when there
//                     are fewer than k).  k distinct rows are at least that close, so the k best all have d <= tau.  A pair
//                     whose 16th entry is finite and <= tau is saturated -- its list may hold more such rows -- and goes
//                     to the rescan (pair_mask); any other pair has every row with d <= tau in its partial list, and
//                     those entries are appended to the query's candidate list here.
//   (the rescan plan: ivf_nd_count / ivf_nd_prefix / ivf_nd_fill of vs_ivf_nd.hip over the masked pairs, own tables)
//   ivf_scan_nd_cand_kernel : ivf_scan_nd_kernel's item loop, row and query loads and MFMA order on the rescan plan; no
//                     lane lists, no workgroup merge: a real row of a real slot with d <= tau[query] is appended to the
//                     query's list.  The distance is the same accumulation chain that tau came out of, so the comparison
//                     needs no slack.
//   ivf_nd_wide_rank_kernel : per query, the k smallest keys of its list; a query with more than kIvfNdWideCand
//                     candidates (a long list under an infinite bound, masses of equal rows) is ranked over every row of
//                     its probed lists, each distance recomputed by one thread in the MFMA's order.
//
// A candidate is the 64-bit key of vs_wide_select.h: (ordered distance bits) << 32 | reordered row -- the order the
// result is ranked by.  The lists of a query's pairs are disjoint, so its keys are unique.
#include "vs_kernels.h"
#include "vs_dev.h"
#include "vs_wide_select.h"

namespace vs {

// The key of a candidate.  Squared L2 (IP false): tw_key / tw_dist as they are.  Inner product: tw_key folds -0.0 into +0
// -- the rank the float comparisons of the other merges give it -- and tw_dist would hand +0.0 back, but a zero product
// is -0.0 in every other path and in the oracle.  The IP key keeps the folded distance word, so -0.0 still ranks above
// every negative score, below every positive one and ties with +0.0 by row, and stores (row << 1 | was -0.0) in the low
// word (rows are below 2^31; they are unique per query, so the last bit never decides an order).
template <bool IP>
__device__ __forceinline__ bool nd_wide_key(float d, int32_t row, uint64_t& key) {
    if (!tw_key(d, row, key)) return false;
    if constexpr (IP)
        key = (key & 0xffffffff00000000ull) | ((uint32_t)row << 1) | (__builtin_bit_cast(uint32_t, d) == 0x80000000u ? 1u : 0u);
    return true;
}
template <bool IP>
__device__ __forceinline__ int32_t nd_wide_row(uint64_t key) {
    return IP ? (int32_t)((uint32_t)key >> 1) : (int32_t)(uint32_t)key;
}
template <bool IP>
__device__ __forceinline__ float nd_wide_dist(uint64_t key) {
    const float d = tw_dist(key);
    return IP && (key & 1u) ? -0.0f : d;
}

constexpr int kNdWideThreads = 256;
constexpr int kNdWideSelCap = 2048;  // keys the final sort holds (16 KB of LDS)
constexpr int kNdWideTiles = 4;      // as ivf_scan_nd_kernel: 16-row tiles per wave block
constexpr int kNdWideBlockRows = kNdWideTiles * kTileRows;
static_assert(kNdWideBlockRows <= kScanPadRows, "row blocks are loaded unclamped");
static_assert(kIvfMaxProbe * 16 <= kIvfNdWideCand, "the partial lists of a query fit its candidate list");

// grid = group_q, 256 threads
template <bool IP>
__global__ __launch_bounds__(kNdWideThreads) void ivf_nd_wide_bound_kernel(const IvfNdWideParams p) {
    __shared__ WideSelLds<kNdWideSelCap> sel;
    __shared__ int s_n;
    const int q = blockIdx.x, tid = threadIdx.x;
    const int nprobe = p.r.nprobe, k = p.r.k;
    for (int i = blockIdx.x * kNdWideThreads + tid; i < 2 * p.r.nlist; i += gridDim.x * kNdWideThreads) p.r.list_cnt[i] = 0;
    const int64_t base = (int64_t)q * nprobe * 16;
    const int n = nprobe * 16;
    if (tid == 0) s_n = 0;
    const int M = wide_select<kNdWideThreads>(sel, n, k, [&](auto&& f) {
        for (int e = tid; e < n; e += kNdWideThreads) {
            uint64_t key;
            if (nd_wide_key<IP>(p.r.part_d[base + e], p.r.part_i[base + e], key)) f(key);
        }
    });  // (ends with a barrier)
    const float tau = M >= k ? tw_dist(sel.keys[k - 1]) : VS_INF;
    unsigned long long* const cand = p.cand + (int64_t)q * kIvfNdWideCand;
    for (int rank = tid; rank < nprobe; rank += kNdWideThreads) {
        const int64_t o = base + (int64_t)rank * 16;
        const float last = p.r.part_d[o + 15];
        const bool saturated = last < VS_INF && last <= tau;
        p.pair_mask[(int64_t)q * nprobe + rank] = saturated ? 1 : 0;
        if (saturated) continue;
        for (int j = 0; j < 16; ++j) {
            const float d = p.r.part_d[o + j];
            uint64_t key;
            if (d <= tau && nd_wide_key<IP>(d, p.r.part_i[o + j], key)) cand[atomicAdd(&s_n, 1)] = key;  // (at most 16 nprobe entries)
        }
    }
    __syncthreads();
    if (tid == 0) {
        p.cnt[q] = s_n;  // (left at 0 by the previous group's ranking)
        p.tau[q] = tau;
    }
}

template <bool IP>
__global__ __launch_bounds__(kScanThreads, 1) void ivf_scan_nd_cand_kernel(const IvfNdWideParams w) {
    constexpr int T = kNdWideTiles;
    const IvfNdParams& p = w.r;
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r = lane & 15, g = lane >> 4;
    const int dim_p = p.dim_p;
    const unsigned voff = (unsigned)(r * dim_p + 4 * g) * 4u;  // this lane's 16 bytes inside a 16-row tile's segment
    const unsigned tile_bytes = 64u * (unsigned)dim_p;         // 16 rows
    const int C = dim_p / 16;    // 64-byte segments per row
    const int n_pairs = C >> 1;  // full 32-float steps
    const int n_items = p.n_items[0];

#pragma clang loop unroll(disable)
    for (int item = blockIdx.x; item < n_items; item += gridDim.x) {
        const int list = p.items[2 * item], slot0 = p.items[2 * item + 1];
        const int n_slots = min(kIvfNdSlotBlock, p.list_start[list + 1] - slot0);
        const int64_t row_lo = p.offsets[list], row_end = p.offsets[list + 1];
        const int64_t last_row = row_end - 1;
        const int blocks_total = (int)((row_end - row_lo + kNdWideBlockRows - 1) / kNdWideBlockRows);
        const bool live = r < n_slots;  // (a slot past the run's end repeats the first and appends nothing)
        const int sv = p.slots[slot0 + (live ? r : 0)];
        const int qi = sv >> 8;
        float qn = 0.f;
        if constexpr (!IP) qn = p.qnorm[qi];
        const float tau = w.tau[qi];
        // this lane's 16 bytes of a 64-byte segment of its slot's padded query row
        const char* qb = reinterpret_cast<const char*>(p.qrows + (int64_t)qi * dim_p + 4 * g);
        unsigned long long* const cand = w.cand + (int64_t)qi * kIvfNdWideCand;

#pragma clang loop unroll(disable)
        for (int wb = wave; wb < blocks_total; wb += kScanWaves) {
            const int64_t row0 = row_lo + (int64_t)wb * kNdWideBlockRows;
            const char* sb = reinterpret_cast<const char*>(p.vecs + row0 * (int64_t)dim_p);
            f32x4 acc[T];
#pragma unroll
            for (int t = 0; t < T; ++t) acc[t] = (f32x4){0.f, 0.f, 0.f, 0.f};
            f32x4 a[T][2], b[2];
            auto load_pair = [&](int s, f32x4 (&av)[T][2], f32x4 (&bv)[2]) __attribute__((always_inline)) {
#pragma unroll
                for (int t = 0; t < T; ++t) {
                    av[t][0] = *(reinterpret_cast<const f32x4*>(sb + (t * tile_bytes + 128u * s) + voff));
                    av[t][1] = *(reinterpret_cast<const f32x4*>(sb + (t * tile_bytes + 128u * s + 64u) + voff));
                }
                bv[0] = *reinterpret_cast<const f32x4*>(qb + 128u * s);
                bv[1] = *reinterpret_cast<const f32x4*>(qb + 128u * s + 64u);
            };
            auto mfma_half = [&](const f32x4 (&av)[T][2], const f32x4 (&bv)[2], int u) __attribute__((always_inline)) {
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int t = 0; t < T; ++t) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[t][u][i], bv[u][i], acc[t], 0, 0, 0);
            };
            if (n_pairs > 0) load_pair(0, a, b);
            for (int s = 0; s < n_pairs; ++s) {
                f32x4 an[T][2], bn2[2];
                const bool more = s + 1 < n_pairs;
                if (more) load_pair(s + 1, an, bn2);
                mfma_half(a, b, 0);
                mfma_half(a, b, 1);
                if (more) {
#pragma unroll
                    for (int t = 0; t < T; ++t) {
                        a[t][0] = an[t][0];
                        a[t][1] = an[t][1];
                    }
                    b[0] = bn2[0];
                    b[1] = bn2[1];
                }
            }
            if (C & 1) {  // the last 16 floats of a row whose dim_p is an odd number of segments
#pragma unroll
                for (int t = 0; t < T; ++t) a[t][0] = *(reinterpret_cast<const f32x4*>(sb + (t * tile_bytes + 128u * n_pairs) + voff));
                b[0] = *reinterpret_cast<const f32x4*>(qb + 128u * n_pairs);
                mfma_half(a, b, 0);
            }
#pragma unroll
            for (int t = 0; t < T; ++t) {
                const int64_t rbase = row0 + 16 * t + 4 * g;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    float d;
                    if constexpr (IP)
                        d = -acc[t][j];
                    else
                        d = fmaf(-2.0f, acc[t][j], qn + p.vnorm[rbase + j]);  // (the norms have 64 spare entries)
                    uint64_t key;
                    // (rbase + j <= last_row: a row past the list's end never competes -- under IP it would score -0.0)
                    if (live && rbase + j <= last_row && d <= tau && nd_wide_key<IP>(d, (int32_t)(rbase + j), key)) {
                        const int pos = atomicAdd(w.cnt + qi, 1);
                        if (pos < kIvfNdWideCand) cand[pos] = key;
                    }
                }
            }
        }
    }
}

// one thread, one (row, query) dot product over the zero-padded dim_p floats in the order the MFMA chain adds them:
// segments of 16 floats ascending; inside a segment instruction i = 0..3 adds the k slices g = 0..3, element 16 c + 4 g + i
__device__ __forceinline__ float nd_dot_chain(const float* __restrict__ b, const float* __restrict__ q, const int C) {
    float dot = 0.f;
    for (int c = 0; c < C; ++c) {
        f32x4 bv[4], qv[4];
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            bv[g] = *reinterpret_cast<const f32x4*>(b + 16 * c + 4 * g);
            qv[g] = *reinterpret_cast<const f32x4*>(q + 16 * c + 4 * g);
        }
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int g = 0; g < 4; ++g) dot = __fmaf_rn(bv[g][i], qv[g][i], dot);
    }
    return dot;
}

// grid = group_q, 256 threads.  The group's last kernel.
template <bool IP>
__global__ __launch_bounds__(kNdWideThreads) void ivf_nd_wide_rank_kernel(const IvfNdWideParams w) {
    __shared__ WideSelLds<kNdWideSelCap> sel;
    __shared__ int s_upper;
    const IvfNdParams& p = w.r;
    const int q = blockIdx.x, tid = threadIdx.x;
    const int k = p.k;
    const int n = w.cnt[q];
    const bool exact = n > kIvfNdWideCand;  // (workgroup-uniform)
    int M;
    if (!exact) {
        const unsigned long long* const cand = w.cand + (int64_t)q * kIvfNdWideCand;
        M = wide_select<kNdWideThreads>(sel, n, k, [&](auto&& f) {
            for (int e = tid; e < n; e += kNdWideThreads) f((uint64_t)cand[e]);
        });
    } else {
        const int32_t* const pr = p.probes + (int64_t)q * p.nprobe;
        const float* const qv = p.qrows + (int64_t)q * p.dim_p;
        float qn = 0.f;
        if constexpr (!IP) qn = p.qnorm[q];
        const int C = p.dim_p / 16;
        if (tid == 0) s_upper = 0;
        __syncthreads();
        for (int pp = tid; pp < p.nprobe; pp += kNdWideThreads) {
            const int c = pr[pp];
            if (c >= 0 && c < p.nlist) atomicAdd(&s_upper, p.offsets[c + 1] - p.offsets[c]);
        }
        __syncthreads();
        M = wide_select<kNdWideThreads>(sel, s_upper, k, [&](auto&& f) {
            for (int pp = 0; pp < p.nprobe; ++pp) {
                const int c = pr[pp];
                if (c < 0 || c >= p.nlist) continue;
                const int s0 = p.offsets[c], s1 = p.offsets[c + 1];
                for (int row = s0 + tid; row < s1; row += kNdWideThreads) {  // (the list's own rows only: none past s1)
                    const float dot = nd_dot_chain(p.vecs + (int64_t)row * p.dim_p, qv, C);
                    float d;
                    if constexpr (IP)
                        d = -dot;
                    else
                        d = fmaf(-2.0f, dot, qn + p.vnorm[row]);
                    uint64_t key;
                    if (nd_wide_key<IP>(d, row, key)) f(key);
                }
            }
        });
    }
    const int n_out = min(M, k);
    for (int t = tid; t < k; t += kNdWideThreads) {
        float d = VS_INF;
        int32_t id = -1;
        if (t < n_out) {
            d = nd_wide_dist<IP>(sel.keys[t]);
            const int32_t row = nd_wide_row<IP>(sel.keys[t]);
            id = w.id_map ? w.id_map[row] : row;
        }
        w.out_d[(int64_t)q * k + t] = d;
        w.out_i[(int64_t)q * k + t] = id;
    }
    if (tid == 0) {
        if (exact) {
            atomicAdd(w.stats + 2, 1ull);
        } else {
            atomicAdd(w.stats + 0, (unsigned long long)n);
            atomicMax(w.stats + 1, (unsigned long long)n);
        }
        w.cnt[q] = 0;  // for the next group
    }
}

static bool nd_wide_ok(const IvfNdWideParams& p) {
    const IvfNdParams& r = p.r;
    return r.dim >= 1 && r.dim <= kNdMaxDim && r.dim_p == nd_dim_p(r.dim) && r.group_q >= 1 && r.group_q <= kIvfNdGroupQ && r.nprobe >= 1 &&
           r.nprobe <= kIvfMaxProbe && r.nlist >= 1 && (r.metric == 0 || r.metric == 1) && r.kcap == 16 && r.k > 16 && r.k <= kIvfNdWideKMax && p.tau && p.pair_mask &&
           r.pair_mask == p.pair_mask && p.cnt && p.cand && p.out_d && p.out_i && p.stats;
}

hipError_t launch_ivf_nd_wide_bound(const IvfNdWideParams& p, hipStream_t s) {
    if (!nd_wide_ok(p)) return hipErrorInvalidValue;
    if (p.r.metric)
        hipLaunchKernelGGL(ivf_nd_wide_bound_kernel<true>, dim3(p.r.group_q), dim3(kNdWideThreads), 0, s, p);
    else
        hipLaunchKernelGGL(ivf_nd_wide_bound_kernel<false>, dim3(p.r.group_q), dim3(kNdWideThreads), 0, s, p);
    return hipGetLastError();
}

hipError_t launch_ivf_nd_wide_scan(const IvfNdWideParams& p, int grid, hipStream_t s) {
    if (!nd_wide_ok(p) || grid < 1) return hipErrorInvalidValue;
    if (p.r.metric)
        hipLaunchKernelGGL(ivf_scan_nd_cand_kernel<true>, dim3(grid), dim3(kScanThreads), 0, s, p);
    else
        hipLaunchKernelGGL(ivf_scan_nd_cand_kernel<false>, dim3(grid), dim3(kScanThreads), 0, s, p);
    return hipGetLastError();
}

hipError_t launch_ivf_nd_wide_rank(const IvfNdWideParams& p, hipStream_t s) {
    if (!nd_wide_ok(p)) return hipErrorInvalidValue;
    if (p.r.metric)
        hipLaunchKernelGGL(ivf_nd_wide_rank_kernel<true>, dim3(p.r.group_q), dim3(kNdWideThreads), 0, s, p);
    else
        hipLaunchKernelGGL(ivf_nd_wide_rank_kernel<false>, dim3(p.r.group_q), dim3(kNdWideThreads), 0, s, p);
    return hipGetLastError();
}

}  // namespace vs
