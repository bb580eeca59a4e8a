// vs_scan_tail.h -- what scan_nd_kernel (vs_scan_nd.hip) and scan_nd_i8_kernel (vs_scan_nd_i8.hip) do with their
// distances in kModeTopK, whatever the rows are made of: the top-k step on a group of four distances, the in-kernel
// threshold exchange and the workgroup merge into the partial lists of merge_compact_kernel; ivf_scan_nd_kernel
// (vs_ivf_nd.hip) takes the top-k step and the merge, with its own output lists.  Device functions only;
// the kernel declares one NdTailLds and hands it to them.  tid, lane = tid & 63, wave = tid >> 6 (uniform),
// r = lane & 15 and g = lane >> 4 are the kernels' own: lane (r, g) holds queries h * 16 + r, h < NQH.
#pragma once
#include "vs_kernels.h"
#include "vs_dev.h"
#include <type_traits>

namespace vs {

constexpr int kNdMergeSmall = 64;  // entries per query of the workgroup merge's fast path
constexpr int kNdPassQ = 4;        // queries per pass of its fallback (lists full of unfiltered entries)

struct NdTailLds {
    float wmin[kScanWaves * 32];
    float tau[32];
    int cnt[32];
    float mrg_d[kMaxBatch * kNdMergeSmall];  // fast path [32][kNdMergeSmall]; fallback [kNdPassQ][32 * KCAP]
    int mrg_i[kMaxBatch * kNdMergeSmall];
};

// Four distances of one query (rows rbase .. rbase + 3) into the lane's sorted list, under the lane's bound.
template <int KCAP>
__device__ __forceinline__ void nd_topk_step(const float (&d)[4], int64_t rbase, int id_offset, float& wmin, float& tau,
                                             float (&ld)[KCAP], int (&li)[KCAP]) {
    const float dmin = fminf(fminf(d[0], d[1]), fminf(d[2], d[3]));
    wmin = fminf(wmin, dmin);
    if (dmin < tau) {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (d[j] < tau) {
                list_insert<KCAP>(ld, li, d[j], (int)(rbase + j) + id_offset);
                tau = fminf(tau, ld[KCAP - 1]);
            }
    }
}

// Threshold exchange: the first block went into the lane lists unbounded; every workgroup now publishes, per query, the
// smallest distance it has seen (wmin), reads what the others published and takes the k1-th smallest of 16 group minima
// as an upper bound of the final k1-th best distance (k1 distinct rows are at least that close).  Nobody waits for
// anybody for long: the spin is bounded and an unpublished slot reads +inf, which only loosens the bound -- the result
// does not depend on timing or residency.  Every thread of the workgroup calls it; tq gets the bound, tau its minimum
// with the bound.
template <int NQH>
__device__ __forceinline__ void xchg_bound(NdTailLds& L, float* slots, int k1, int tid, int wave, const float (&wmin)[NQH],
                                           float (&tq)[NQH], float (&tau)[NQH]) {
    constexpr int NQ = NQH * 16;
    const int lane = tid & 63, r = lane & 15, g = lane >> 4;
#pragma unroll
    for (int h = 0; h < NQH; ++h) {
        float m = wmin[h];
        m = fminf(m, __shfl_xor(m, 16));
        m = fminf(m, __shfl_xor(m, 32));
        if (g == 0) L.wmin[wave * 32 + h * 16 + r] = m;
    }
    __syncthreads();
    if (tid < NQ) {
        float m = L.wmin[tid];
#pragma unroll
        for (int w = 1; w < kScanWaves; ++w) m = fminf(m, L.wmin[w * 32 + tid]);
        __hip_atomic_store(slots + tid * kSlotStride + blockIdx.x, m, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    // DPP row g of wave w reduces query 4 w + g: lane r folds workgroups 16 r .. 16 r + 15
    const int qx = 4 * wave + g;
    const float* s0 = slots + qx * kSlotStride + 16 * r;
    const int need = (int)gridDim.x / 2;
    float m = VS_INF;
    for (int spin = 0;; ++spin) {
        int cf = 0;
        m = VS_INF;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const float v = __hip_atomic_load(s0 + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            cf += v < VS_INF;
            m = fminf(m, v);
        }
        cf += dpp_mov_i<0xB1>(cf);
        cf += dpp_mov_i<0x4E>(cf);
        cf += dpp_mov_i<0x141>(cf);
        cf += dpp_mov_i<0x140>(cf);  // row sum: workgroups that have published this row's query
        if (__all(qx >= NQ || cf >= need) || spin >= 2048) break;
        __builtin_amdgcn_s_sleep(24);
    }
    const float kth = row_kth_smallest(m, k1, r, g);
    if (r == 0) L.tau[qx] = kth < VS_INF ? next_up(kth) : VS_INF;
    __syncthreads();
#pragma unroll
    for (int h = 0; h < NQH; ++h) {
        tq[h] = L.tau[h * 16 + r];
        tau[h] = fminf(tau[h], tq[h]);
    }
}

// Workgroup merge: the entries of the lane lists that can still matter (d < tq) are compacted into LDS and ranked into
// one sorted list of KCAP entries per query (the first min(k1, KCAP) by (dist, id), then (+inf, -1)).  With a bound in
// force a query keeps a handful of entries per workgroup (fast path, one wave per query); lists full of unfiltered
// entries (small shards, list scans without a bound) go through in passes of kNdPassQ queries.  where(qq, od, oi) names
// query qq's output list, or returns false for a query without one; it is called by whole waves with qq uniform.  Every
// thread of the workgroup calls the merge; it ends with a barrier, so the LDS is free again.
template <int NQH, int KCAP, class Where>
__device__ __forceinline__ void wg_merge_lists_to(NdTailLds& L, int k1, int tid, int wave, const float (&ld)[NQH][KCAP],
                                                  const int (&li)[NQH][KCAP], const float (&tq)[NQH], Where where) {
    constexpr int NQ = NQH * 16;
    constexpr int CAP = 32 * KCAP;  // 32 lane lists per query
    static_assert(kNdPassQ * CAP <= kMaxBatch * kNdMergeSmall, "the fallback pass fits the merge buffer");
    const int lane = tid & 63, r = lane & 15;
    auto rank = [&](int qq, const float* cand_d, const int* cand_i, auto epl_tag) {
        constexpr int EPL = decltype(epl_tag)::value;
        const int M = min(L.cnt[qq], EPL * 64);
        float* od;
        int32_t* oi;
        if (!where(qq, od, oi)) return;
        const int rounds = min(min(k1, KCAP), M);
        wave_select_rounds<EPL>(cand_d, cand_i, M, rounds, lane, [&](int round, float bd, int bi) {
            if (lane == 0) {
                od[round] = bd;
                oi[round] = bi;
            }
        });
        if (lane < KCAP && lane >= rounds) {
            od[lane] = VS_INF;
            oi[lane] = -1;
        }
    };
    auto compact = [&](int q_lo, int q_n, int cap) {
#pragma unroll
        for (int h = 0; h < NQH; ++h) {
            const int qidx = h * 16 + r;
            if (qidx < q_lo || qidx >= q_lo + q_n) continue;
#pragma unroll
            for (int j = 0; j < KCAP; ++j)
                if (li[h][j] >= 0 && ld[h][j] < tq[h]) {
                    const int pos = atomicAdd(&L.cnt[qidx], 1);
                    if (pos < cap) {
                        L.mrg_d[(qidx - q_lo) * cap + pos] = ld[h][j];
                        L.mrg_i[(qidx - q_lo) * cap + pos] = li[h][j];
                    }
                }
        }
    };
    if (tid < 32) L.cnt[tid] = 0;
    __syncthreads();
    compact(0, NQ, kNdMergeSmall);
    const bool too_many = __syncthreads_or(L.cnt[tid & 31] > kNdMergeSmall);
    if (!too_many) {
        for (int qq = wave; qq < NQ; qq += kScanWaves)
            rank(qq, L.mrg_d + qq * kNdMergeSmall, L.mrg_i + qq * kNdMergeSmall, std::integral_constant<int, 1>{});
    } else {
        for (int q_lo = 0; q_lo < NQ; q_lo += kNdPassQ) {
            __syncthreads();
            if (tid < 32) L.cnt[tid] = 0;
            __syncthreads();
            compact(q_lo, kNdPassQ, CAP);
            __syncthreads();
            if (wave < kNdPassQ) rank(q_lo + wave, L.mrg_d + wave * CAP, L.mrg_i + wave * CAP, std::integral_constant<int, CAP / 64>{});
        }
    }
    __syncthreads();  // LDS is reused by the next batch
}

// The merge of the per-batch brute-force scans: the sorted per-workgroup lists go to merge_compact_kernel.
template <int NQH, int KCAP>
__device__ __forceinline__ void wg_merge_lists(NdTailLds& L, const ScanParams& p, int batch, int tid, int wave,
                                               const float (&ld)[NQH][KCAP], const int (&li)[NQH][KCAP], const float (&tq)[NQH]) {
    // partial lists are query-major: [batch][query][workgroup][KCAP] (one merge launch ranks all batches)
    wg_merge_lists_to<NQH, KCAP>(L, p.k1, tid, wave, ld, li, tq, [&](int qq, float*& od, int32_t*& oi) {
        od = p.part_d + (((int64_t)batch * kMaxBatch + qq) * kSlotStride + blockIdx.x) * KCAP;
        oi = p.part_i + (((int64_t)batch * kMaxBatch + qq) * kSlotStride + blockIdx.x) * KCAP;
        return true;
    });
}

}  // namespace vs
