// vs_one_tail.h -- what the single-call scans, scan_one_kernel (vs_scan_one.hip), scan_one_nd_kernel (vs_scan_one_nd.hip),
// scan_one_nd_i8_kernel (vs_scan_one_nd_i8.hip) and ivf_one_scan_kernel (vs_ivf_one_nd.hip), do with their lane lists without
// a second launch: the bound from the workgroup's lane minima that the scan loops take at their checkpoints, the
// workgroup merge into one partial list per query, and the merge of the partial lists by the workgroup that arrives
// last; and the LDS layout of the three of them on a general index (OneNdLds).
// Device functions only; the kernel keeps its prologue, data path and distance arithmetic and hands over its lane lists
// and its LDS (OneTailLds).  lane = tid & 63, wave = tid >> 6, r = lane & 15 and g = lane >> 4 as in the kernels: lane
// (r, g) holds queries 16 h + r, h < NQH.
#pragma once
#include "vs_kernels.h"
#include "vs_dev.h"

namespace vs {

#ifdef VS_STAMPS
#define ONE_STAMP(i)                                                                                   \
    do {                                                                                               \
        if (p.dbg && threadIdx.x == 0) p.dbg[blockIdx.x * 16 + (i)] = (int)(__builtin_amdgcn_s_memrealtime() & 0x7fffffff); \
    } while (0)
#else
#define ONE_STAMP(i)
#endif

constexpr int kOneFinalCap = 256;  // candidates per query the final merge keeps in LDS

// LDS the merges need: a query's 32 lane lists of KCAP (dist, id) entries, later per wave kOneFinalCap (dist, id)
// candidates and the numbers of the passing lists
constexpr int one_tail_bytes(int nqh, int kcap) {
    const int merge = 16 * nqh * 32 * kcap * 8, fin = kScanWaves * (2 * kOneFinalCap + kSlotStride) * 4;
    return merge > fin ? merge : fin;
}

struct OneTailLds {
    char* region;  // the kernel is done with it when the scan loop ends (the 128-d ring, the ND query fragments); 16-byte aligned
    int* cnt;      // [32]
    int* flag;     // [1]
    float* lmin;   // [16 NQH columns][33]: the lane minima of the column's 32 lanes (4 lane groups x 8 waves), rows 33 apart
};

// k smallest of M (dist, id) pairs by ascending (dist, id), read through `get(e, d, id)`; ids are unique.  One wave,
// nothing is modified: round r takes the smallest pair above round r - 1's.  emit(round, d, id, none).
template <class Get, class Emit>
__device__ __forceinline__ void wave_rank_rounds(int M, int rounds, int lane, Get get, Emit emit) {
    float last_d = -VS_INF;
    int last_i = -1;
    bool first = true;
    for (int round = 0; round < rounds; ++round) {
        float md = VS_INF;
        int mi = 0x7fffffff;
        for (int e = lane; e < M; e += 64) {
            float d;
            int id;
            get(e, d, id);
            if (id < 0) continue;
            if (!first && (d < last_d || (d == last_d && id <= last_i))) continue;  // emitted already
            if (lex_lt(d, id, md, mi)) {
                md = d;
                mi = id;
            }
        }
        float bd;
        int bi;
        wave_lexmin(md, mi, bd, bi);
        const bool none = bi == 0x7fffffff;
        emit(round, bd, bi, none);
        if (none) {
            for (int r2 = round + 1; r2 < rounds; ++r2) emit(r2, VS_INF, 0x7fffffff, true);
            return;
        }
        last_d = bd;
        last_i = bi;
        first = false;
    }
}

// The bound that makes insertions rare: the k1-th smallest of the 32 lane minima of a query column in this workgroup
// (k1 distinct rows are at least that close; a lane alone sees N / 8192 rows and would insert a fifth of them, and
// with 64 lanes deciding independently some lane inserts at nearly every value).  Taken at a few checkpoints, from
// whatever the other waves have published by then: a missing or stale minimum only loosens it.  Lane (r, g) of column
// `col` (16 h + r) reads 8 of the column's 32 minima.
// (cheap form: each of the column's 4 lanes takes the t-th smallest of its 8 minima, t = ceil(k1 / 4); the largest of
// the four has 4 t >= k1 minima at or below it.  The exact k1-th smallest of the 32 costs k1 rounds of cross-lane
// traffic and was measured at 1.5 us per call and column block)
__device__ __forceinline__ float one_shared_bound(const float* lds_lmin, int col, int g, int k1) {
    const int t = (k1 + 3) >> 2;
    float v[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) v[i] = lds_lmin[col * 33 + 8 * g + i];
    float m = VS_INF;
    for (int round = 0; round < t; ++round) {
        m = fminf(fminf(fminf(v[0], v[1]), fminf(v[2], v[3])), fminf(fminf(v[4], v[5]), fminf(v[6], v[7])));
        bool done = false;
#pragma unroll
        for (int i = 0; i < 8; ++i)
            if (!done && v[i] == m) {
                v[i] = VS_INF;
                done = true;
            }
    }
    float x = fmaxf(m, __shfl_xor(m, 16));
    x = fmaxf(x, __shfl_xor(x, 32));
    return x;  // (+inf while a lane holds fewer than t minima)
}

// The LDS of a single-call kernel on a general index: region | term [32] | counters [32] | flag [32] | lane minima
// [16][33].  The region holds the 16 query columns in MFMA B-fragment order (16 x the bytes of a padded row) while the
// rows are scanned and the merge buffers afterwards; `term` is the per-query term of the kernel's arithmetic (a float
// norm, an int32 term).
constexpr int kOneNdScratch = 8192;  // everything behind the region
constexpr int one_nd_region(int row_bytes, int kcap) {
    const int frag = 16 * row_bytes, merge = one_tail_bytes(1, kcap);
    return frag > merge ? frag : merge;
}
constexpr int one_nd_lds_bytes(int row_bytes, int kcap) { return one_nd_region(row_bytes, kcap) + kOneNdScratch; }
static_assert(one_nd_lds_bytes(4 * kNdMaxDim, 16) <= 160 * 1024, "LDS of a CU");
template <class Term>  // float or int
struct OneNdLds {
    OneTailLds tail;  // region | counters | flag | lane minima: what one_tail takes
    Term* term;       // [16]
};
template <class Term>
__device__ __forceinline__ OneNdLds<Term> one_nd_lds(char* smem, int row_bytes, int kcap) {
    static_assert(sizeof(Term) == 4, "32 words of terms");
    OneNdLds<Term> L;
    L.tail.region = smem;
    L.term = reinterpret_cast<Term*>(smem + one_nd_region(row_bytes, kcap));
    L.tail.cnt = reinterpret_cast<int*>(L.term + 32);
    L.tail.flag = L.tail.cnt + 32;
    L.tail.lmin = reinterpret_cast<float*>(L.tail.flag + 32);
    return L;
}
// no lane of the workgroup has a minimum yet; every thread calls it, the caller's next barrier publishes it
__device__ __forceinline__ void one_nd_reset_lmin(float* lds_lmin) {
    for (int i = threadIdx.x; i < 16 * 33; i += kScanThreads) lds_lmin[i] = VS_INF;  // (rows 33 apart: bank spread)
}

// the ids of the lane lists are the ids of the outputs (the brute-force scans add id_offset when they insert)
struct OneTailSameId {
    __device__ __forceinline__ int operator()(int id) const { return id; }
};

// Everything after the scan loop; every thread of the workgroup calls it, with nothing of its own outstanding on
// L.region.  REGION is the least size in bytes L.region can have in this instantiation of the kernel.  The lists are
// merged and ranked by (dist, id) on the ids the kernel inserted; an output id is id_map(that id) (the IVF single-call
// scan ranks positions in the reordered rows and writes original ids).
template <int NQH, int KCAP, int REGION, class IdMap = OneTailSameId>
__device__ __forceinline__ void one_tail(const OneParams& p, const OneTailLds& L, const float (&ld)[NQH][KCAP], const int (&li)[NQH][KCAP],
                                         const IdMap id_map = IdMap{}) {
    static_assert(one_tail_bytes(NQH, KCAP) <= REGION, "the merge buffers overlay the kernel's region");
    constexpr int NQ = NQH * 16;
    char* const smem = L.region;
    int* const lds_cnt = L.cnt;
    int* const lds_flag = L.flag;
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r = lane & 15, g = lane >> 4;
    const int G = (int)gridDim.x;

    // ---- workgroup merge.  A query's 32 lane lists (4 lane groups x 8 waves): the k1-th smallest lane minimum bounds the
    // workgroup's k1-th best (+inf with fewer than k1 rows); entries not above it are compacted into LDS (the region is
    // free now: room for every entry, so nothing can overflow) and ranked by one wave per query.
    __syncthreads();  // (every wave is done with the region; the lane minima are final)
    if (tid < 32) lds_cnt[tid] = 0;
    constexpr int CAP = 32 * KCAP;
    float* cand_d = reinterpret_cast<float*>(smem);
    int* cand_i = reinterpret_cast<int*>(smem + (size_t)NQ * CAP * sizeof(float));
    float wg_bound[NQH];
#pragma unroll
    for (int h = 0; h < NQH; ++h) wg_bound[h] = one_shared_bound(L.lmin, 16 * h + r, g, p.k1);
    __syncthreads();
#pragma unroll
    for (int h = 0; h < NQH; ++h) {
        const int qidx = 16 * h + r;
#pragma unroll
        for (int j = 0; j < KCAP; ++j)
            if (li[h][j] >= 0 && ld[h][j] <= wg_bound[h]) {
                const int pos = atomicAdd(&lds_cnt[qidx], 1);
                cand_d[qidx * CAP + pos] = ld[h][j];
                cand_i[qidx * CAP + pos] = li[h][j];
            }
    }
    __syncthreads();
    ONE_STAMP(3);
    // partial lists: part[query][workgroup][k1], sorted by (dist, id), padded with (+inf, -1); written with agent-scope
    // (write-through) stores, one per lane
    for (int qq = wave; qq < p.nq_valid; qq += kScanWaves) {
        float* od = p.part_d + ((int64_t)qq * G + blockIdx.x) * p.k1;
        int32_t* oi = p.part_i + ((int64_t)qq * G + blockIdx.x) * p.k1;
        auto put = [&](int slot, float d, int id) {
            __hip_atomic_store(od + slot, d, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(oi + slot, id, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        };
        const int M = lds_cnt[qq];
        if (M <= 64) {
            const float d = lane < M ? cand_d[qq * CAP + lane] : VS_INF;
            const int id = lane < M ? cand_i[qq * CAP + lane] : 0x7fffffff;
            const int rank = wave_rank_count(d, id, M);
            if (lane < M && rank < p.k1) put(rank, d, id);
            if (lane >= M && lane < p.k1) put(lane, VS_INF, -1);
        } else {
            wave_rank_rounds(
                M, p.k1, lane,
                [&](int e, float& d, int& id) {
                    d = cand_d[qq * CAP + e];
                    id = cand_i[qq * CAP + e];
                },
                [&](int round, float d, int id, bool none) {
                    if (lane == 0) put(round, none ? VS_INF : d, none ? -1 : id);
                });
        }
    }
    // ---- the workgroup that arrives last merges the partial lists.  Nobody waits for anybody: a workgroup that is not
    // the last one is done.  No fences: the partial lists are written with agent-scope stores that have completed
    // (vmcnt(0)) before the workgroup's arrival is counted -- a release / acquire fence pair here writes back and
    // invalidates the whole L2 of the XCD under the workgroups that are still streaming (measured: 126 instead of 100 us
    // per call at 1 M rows)
    ONE_STAMP(4);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    ONE_STAMP(5);
    if (tid == 0) lds_flag[0] = (__hip_atomic_fetch_add(p.done, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == G - 1) ? 1 : 0;
    __syncthreads();
    ONE_STAMP(6);
    if (!lds_flag[0]) return;  // workgroup-uniform
    if (tid == 0) __hip_atomic_store(p.done, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // ready for the next launch (stream ordered)
    // ONE acquire fence in ONE workgroup (every other workgroup has arrived, nobody is streaming any more): lines of the
    // partial lists this XCD's L2 may still hold from an earlier launch are dropped, plain cached loads below.  (Agent-scope
    // loads instead bypass the caches one dword at a time: 16 K of them took 35 us.)
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    ONE_STAMP(8);
    // Every memory round trip here is a microsecond or two of the call's latency, so a query costs two of them: (1) the
    // FIRST entry of each of its G partial lists (a wave reads 256 at once); their k1-th smallest bounds the k1-th best --
    // k1 distinct rows are at least that close (the lists' k1-th entries would bound it too, but a hundred times looser:
    // the smallest "sixth best of a 256th of the rows" is about the 400th best of all).  (2) the lists whose first entry
    // is not above the bound -- about k1 of them -- are read whole, all of them at once, one (list, entry) pair per lane.
    // What is not above the bound (a handful) is ranked by counting.  One wave per query; the wave's queries' first
    // entries are requested together up front.
    constexpr int QPW = NQ / kScanWaves;              // queries per wave at most: 2 per column block
    constexpr int SPL = kSlotStride / 64;             // lists per lane and query at most: 4
    constexpr int FCAP = kOneFinalCap;
    float* fin_d = reinterpret_cast<float*>(smem) + wave * FCAP;
    int* fin_i = reinterpret_cast<int*>(smem + kScanWaves * FCAP * sizeof(float)) + wave * FCAP;
    int* pl = reinterpret_cast<int*>(smem + 2 * kScanWaves * FCAP * sizeof(float)) + wave * kSlotStride;  // passing lists of the current query
    float fd[QPW][SPL];
#pragma unroll
    for (int qi = 0; qi < QPW; ++qi) {
        const int qq = wave + kScanWaves * qi;
#pragma unroll
        for (int u = 0; u < SPL; ++u) {
            const int w = lane + 64 * u;
            fd[qi][u] = VS_INF;
            if (qq < p.nq_valid && 64 * u < G) fd[qi][u] = p.part_d[((int64_t)qq * G + min(w, G - 1)) * p.k1];
            if (w >= G) fd[qi][u] = VS_INF;
        }
    }
    ONE_STAMP(9);
#pragma unroll
    for (int qi = 0; qi < QPW; ++qi) {
        const int qq = wave + kScanWaves * qi;
        if (qq >= p.nq_valid) break;  // wave-uniform
        const float* pd = p.part_d + (int64_t)qq * G * p.k1;
        const int32_t* pi = p.part_i + (int64_t)qq * G * p.k1;
        float* od = p.out_d + (int64_t)qq * p.k1;
        int32_t* oi = p.out_i + (int64_t)qq * p.k1;
        const float b = wave_kth_smallest(fd[qi][0], fd[qi][1], fd[qi][2], fd[qi][3], p.k1, lane);  // (+inf with fewer than k1 rows in all)
        // the passing lists, compacted (ballot prefix), then one (list, entry) pair per lane
        int P = 0;
#pragma unroll
        for (int u = 0; u < SPL; ++u) {
            const bool pass = fd[qi][u] < VS_INF && fd[qi][u] <= b;
            const unsigned long long mask = __ballot(pass);
            if (pass) pl[P + (int)__builtin_amdgcn_mbcnt_hi((unsigned)(mask >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)mask, 0))] = lane + 64 * u;
            P += __popcll(mask);
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        const int pairs = P * p.k1;
        int M = 0;
        for (int e0 = 0; e0 < pairs; e0 += 64) {
            const int e = e0 + lane;
            float d = VS_INF;
            int id = -1;
            if (e < pairs) {
                const int off = pl[e / p.k1] * p.k1 + e % p.k1;
                d = pd[off];
                id = pi[off];
            }
            const bool pass = id >= 0 && d <= b;
            const unsigned long long mask = __ballot(pass);
            const int pos = M + (int)__builtin_amdgcn_mbcnt_hi((unsigned)(mask >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)mask, 0));
            if (pass && pos < FCAP) {
                fin_d[pos] = d;
                fin_i[pos] = id;
            }
            M += __popcll(mask);
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
#ifdef VS_STAMPS
        if (p.dbg && lane == 0 && qq == 0) p.dbg[blockIdx.x * 16 + 11] = M;
#endif
        if (M <= 64) {
            const float d = lane < M ? fin_d[lane] : VS_INF;
            const int id = lane < M ? fin_i[lane] : 0x7fffffff;
            const int rank = wave_rank_count(d, id, M);
            if (lane < M && rank < p.k1) {
                od[rank] = d;
                oi[rank] = id_map(id);
            }
            if (lane >= M && lane < p.k1) {
                od[lane] = VS_INF;
                oi[lane] = -1;
            }
            // two of the k1 outputs at one distance (select_topk's order among them is history dependent: the caller's flag)
            bool tie = false;
            for (int j = 0; j < M; ++j) {
                const float dj = rdlane_f(d, j);
                const int rj = __builtin_amdgcn_readlane(rank, j);
                tie = tie || (j != lane && dj == d && rj < p.k1);
            }
            const bool any_tie = __any(lane < M && rank < p.k1 && tie);
            if (lane == 0 && p.flags) p.flags[qq] = any_tie ? 1 : 0;
        } else {
            float prev = VS_INF;
            int tie = 0;
            auto emit = [&](int round, float d, int id, bool none) {
                if (!none && round > 0 && d == prev) tie = 1;
                prev = none ? VS_INF : d;
                if (lane == 0) {
                    od[round] = none ? VS_INF : d;
                    oi[round] = none ? -1 : id_map(id);
                }
            };
            if (M <= FCAP) {
                wave_rank_rounds(M, p.k1, lane, [&](int e, float& d, int& id) { d = fin_d[e]; id = fin_i[e]; }, emit);
            } else {  // masses of equal distances at the bound: rank straight from the partial lists
                wave_rank_rounds(G * p.k1, p.k1, lane, [&](int e, float& d, int& id) { d = pd[e]; id = pi[e]; }, emit);
            }
            if (lane == 0 && p.flags) p.flags[qq] = tie;
        }
        __builtin_amdgcn_wave_barrier();  // (fin / pl are reused by the wave's next query)
    }
#ifdef VS_STAMPS
    __syncthreads();
    ONE_STAMP(7);
#endif
}

}  // namespace vs
