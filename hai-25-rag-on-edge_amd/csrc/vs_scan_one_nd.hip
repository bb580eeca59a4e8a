// vs_scan_one_nd.hip -- the single-call brute-force scan at any vector length 1 <= dim <= 2048 (gfx950): ONE launch per
// batch of at most 16 queries on the fp32 rows of a general index, k + 1 <= 16.
//
//   scan_one_nd_kernel<KCAP>: scan_nd_kernel's arithmetic (v_mfma_f32_16x16x4_f32, base rows = A operand, one accumulation
//   chain per distance in the (c, i) order of DESIGN 4.4c, the half step when dim_p / 16 is odd, fma(-2, dot, qn + bn) or
//   -dot) with scan_one_kernel's top-k (vs_scan_one.hip: per-lane sorted lists, a bound from the workgroup's lane minima
//   at a few checkpoints, one partial list per workgroup and query, the workgroup that arrives last merges them).  No
//   preparation launch, no memset, no merge launch, and nothing anywhere waits for another workgroup.
//
//   Queries.  Every workgroup reads the caller's unpadded [B][dim] queries itself, once: it writes them zero-padded in
//   MFMA B-fragment order into LDS (dim_p / 16 segments of 1 KB: 128 KB at dim 2048) and works out ||q||^2 in the
//   reference's order (nd_prep_kernel's code).  A K step then takes its two B fragments with two 16-byte LDS reads.
//
//   Rows.  A unit of work is a block of kOneNdTiles 16-row tiles (64 rows), dealt statically: unit (n G + workgroup) 8 +
//   wave is the wave's n-th.  The wave keeps the unit's four accumulators resident and walks the rows' K dimension in
//   steps of 32 floats (one 128-byte line per row, 8 KB per wave and step).  The steps of ALL the wave's units form one
//   stream, and the loads run kOneNdDepth steps ahead of the MFMAs in a register ring -- across unit boundaries, so a
//   short row (dim 96: three steps) keeps as many bytes in flight as a long one: 8 waves x 4 steps x 8 KB = 256 KB per
//   CU.  The row norms travel in the same stream (one float per lane and step: a load in the epilogue would be the
//   newest in the queue and waiting for it would drain the ring).  Past the wave's last step the ring is fed with
//   loads of one fixed line, so that every step issues the same number of loads and the compiler's wait counts stay
//   exact.  All loads are ordinary global loads whose waits the compiler places.
#include "vs_kernels.h"
#include "vs_dev.h"

namespace vs {

namespace {

constexpr int kOneNdTiles = 4;                              // 16-row tiles per unit
constexpr int kOneNdUnitRows = kOneNdTiles * kTileRows;     // 64 <= kScanPadRows: a unit never reads past the spare rows
static_assert(kOneNdUnitRows == kOneNdUnit, "the plan's unit");
static_assert(kOneNdUnitRows <= kScanPadRows, "units are loaded unclamped");
static_assert(kOneNdUnitRows == 64, "one row norm per lane");
constexpr int kOneNdDepth = 4;                              // K steps in flight per wave
constexpr int kOneNdQ = 16;                                 // query columns
constexpr int kOneNdScratch = 8192;                         // norms [16] | counters [32] | flag | lane minima [16][33]
constexpr int one_nd_region(int dim_p, int kcap) {          // query fragments, later the merge buffers
    const int frag = dim_p * 64, merge = kOneNdQ * 32 * kcap * 8;
    return frag > merge ? frag : merge;
}
constexpr int kOneNdMaxLds = one_nd_region(kNdMaxDim, 16) + kOneNdScratch;
static_assert(kOneNdMaxLds <= 160 * 1024, "LDS of a CU");

// (vs_scan_one.hip's) k smallest of M (dist, id) pairs by ascending (dist, id), read through `get(e, d, id)`; ids are
// unique.  One wave, nothing is modified: round r takes the smallest pair above round r - 1's.  emit(round, d, id, none).
template <class Get, class Emit>
__device__ __forceinline__ void nd_rank_rounds(int M, int rounds, int lane, Get get, Emit emit) {
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

}  // namespace

template <int KCAP>
__global__ __launch_bounds__(kScanThreads, 1) void scan_one_nd_kernel(const OneNdParams pn) {
    const OneParams& p = pn.o;
    constexpr int T = kOneNdTiles;
    constexpr int D = kOneNdDepth;
    constexpr int NQ = kOneNdQ;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int dim = pn.dim, dim_p = pn.dim_p;
    const int region = one_nd_region(dim_p, KCAP);
    f32x4* qfrag = reinterpret_cast<f32x4*>(smem);                   // [dim_p / 16][64]
    float* lds_qn = reinterpret_cast<float*>(smem + region);         // [16]
    int* lds_cnt = reinterpret_cast<int*>(lds_qn + 32);              // [32]
    int* lds_flag = lds_cnt + 32;                                    // [1]
    float* lds_lmin = reinterpret_cast<float*>(lds_flag + 32);       // [16 queries][32 lanes of the workgroup holding that column]
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r = lane & 15, g = lane >> 4;
    const int G = (int)gridDim.x;
    const int C = dim_p / 16;            // 64-byte segments per row
    const int S = (C + 1) >> 1;          // K steps per unit; the last one is a half step when C is odd
    const bool odd = (C & 1) != 0;

    // ---- the queries: B fragments into LDS, fragment (c, lane) = Q[lane & 15][16 c + 4 (lane >> 4) ..], zeros past dim
    // and past nq_valid (padding columns that nothing looks at)
    for (int e = tid; e < C * 64; e += kScanThreads) {
        const int ql = e & 63, c = e >> 6;
        const int qi = ql & 15, k0 = 16 * c + 4 * (ql >> 4);
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (qi < p.nq_valid) {
#pragma unroll
            for (int i = 0; i < 4; ++i)
                if (k0 + i < dim) v[i] = p.q[(int64_t)qi * dim + k0 + i];
        }
        qfrag[e] = v;
    }
    // ||q||^2: 8 FMA lanes over v[8 i + j], r0 + ... + r7, then the tail (nd_prep_kernel's order); waves 0 and 1
    if (wave < 2) {
        const int row = tid >> 3, j = tid & 7;
        const bool live = row < p.nq_valid;
        const float* src = p.q + (int64_t)(live ? row : 0) * dim;
        float acc = 0.f;
        const int d8 = dim & ~7;
        for (int i = 0; i < d8; i += 8) {
            const float x = src[i + j];
            acc = fmaf(x, x, acc);
        }
        const int b8 = lane & ~7;
        float sum = __shfl(acc, b8);
#pragma unroll
        for (int u = 1; u < 8; ++u) sum = sum + __shfl(acc, b8 + u);
        for (int i = d8; i < dim; ++i) sum = fmaf(src[i], src[i], sum);
        if (j == 0) lds_qn[row] = live ? sum : 0.f;
    }
    // the lanes' current minima, shared by the workgroup (see the checkpoints)
    for (int i = tid; i < NQ * 33; i += kScanThreads) lds_lmin[i] = VS_INF;  // (rows 33 apart: bank spread)
    __syncthreads();
    const float qn = lds_qn[r];
    const bool live = r < p.nq_valid;
    float tau = live ? VS_INF : -VS_INF;  // a padding column never takes a candidate
    float ld[KCAP];
    int li[KCAP];
#pragma unroll
    for (int j = 0; j < KCAP; ++j) {
        ld[j] = VS_INF;
        li[j] = -1;
    }

    // ---- the wave's units.  Run n of the base = units [n 8 G, (n + 1) 8 G): the grid reads one run at about the same
    // time.  p.reverse: the FULL runs are walked from the last to the first (calls alternate, so a call starts on the
    // rows the previous one read last: scan_one_kernel); an incomplete last run stays the wave's last unit, so a wave's
    // units are valid up to n_mine and nothing after.
    const int units_total = (int)((p.n_rows + kOneNdUnitRows - 1) / kOneNdUnitRows);
    const int per_run = G * kScanWaves;
    const int n_full = units_total / per_run;
    const int my = (int)blockIdx.x * kScanWaves + wave;
    const int n_mine = n_full + (n_full * per_run + my < units_total ? 1 : 0);
    auto unit_of = [&](int n) { return ((p.reverse && n < n_full) ? n_full - 1 - n : n) * per_run + my; };
    const int steps_total = n_mine * S;  // (<= 2^31 / 64 units x 64 steps / 2048 waves: fits)

    const unsigned voff = (unsigned)(r * dim_p + 4 * g) * 4u;  // this lane's 16 bytes inside a 16-row tile's segment
    const unsigned tile_bytes = 64u * (unsigned)dim_p;         // 16 rows
    const char* const base_c = reinterpret_cast<const char*>(p.base);
    const int last_row = (int)p.n_rows - 1;

    // the ring: D steps of T x 2 pieces of 16 bytes and one row norm per lane
    f32x4 ring[D][T][2];
    float ring_bn[D];
    int l_n = 0, l_s = 0;  // load cursor: unit l_n of the wave, step l_s
    auto issue = [&](f32x4 (&av)[T][2], float& bnv) __attribute__((always_inline)) {
        const bool have = l_n < n_mine;  // (wave-uniform) past the end: T x 2 + 1 loads of the base's first line
        const int64_t row0 = have ? (int64_t)unit_of(l_n) * kOneNdUnitRows : 0;
        const char* sb = base_c + (have ? row0 * (int64_t)dim_p * 4 + 128 * (int64_t)l_s : 0);
        const unsigned tb = have ? tile_bytes : 0u, vo = have ? voff : 0u;
        const unsigned h2 = (have && !(odd && l_s == S - 1)) ? 64u : 0u;  // a half step reads its first piece twice
#pragma unroll
        for (int t = 0; t < T; ++t) {
            av[t][0] = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(sb + (t * tb + vo)));
            av[t][1] = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(sb + (t * tb + h2 + vo)));
        }
        bnv = p.bnorm[row0 + lane];  // (the norms have 64 spare entries)
        if (++l_s == S) {
            l_s = 0;
            ++l_n;
        }
    };

    // The bound that makes insertions rare (scan_one_kernel's): each of the column's 4 lanes takes the t-th smallest of 8
    // of the column's 32 lane minima, t = ceil(k1 / 4); the largest of the four has 4 t >= k1 minima at or below it, and k1
    // distinct rows are at least that close.  A missing or stale minimum only loosens it.
    auto shared_bound = [&]() __attribute__((always_inline)) {
        const int t = (p.k1 + 3) >> 2;
        float v[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) v[i] = lds_lmin[r * 33 + 8 * g + i];
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
    };

    f32x4 acc[T];
#pragma unroll
    for (int t = 0; t < T; ++t) acc[t] = (f32x4){0.f, 0.f, 0.f, 0.f};
    float bn_cur = 0.f;
    int c_n = 0, c_s = 0;  // compute cursor
    auto compute = [&](const f32x4 (&av)[T][2], const float bnv) __attribute__((always_inline)) {
        if (c_s == 0) bn_cur = bnv;  // (every step of the unit carries it; the first one's is kept)
        const bool half = odd && c_s == S - 1;
        const f32x4 b0 = qfrag[(2 * c_s) * 64 + lane];
        const f32x4 b1 = qfrag[(half ? 2 * c_s : 2 * c_s + 1) * 64 + lane];
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int t = 0; t < T; ++t) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[t][0][i], b0[i], acc[t], 0, 0, 0);
        if (!half) {
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int t = 0; t < T; ++t) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[t][1][i], b1[i], acc[t], 0, 0, 0);
        }
        if (++c_s < S) return;
        // ---- the unit's distances
        c_s = 0;
        const int row0 = unit_of(c_n) * kOneNdUnitRows;
        ++c_n;
        const bool ragged = row0 + kOneNdUnitRows - 1 > last_row;  // wave-uniform
        bool touched = false;
#pragma unroll
        for (int t = 0; t < T; ++t) {
            const int rbase = row0 + 16 * t + 4 * g;
            float d[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float bnj = __shfl(bn_cur, 16 * t + 4 * g + j);
                // cpu_baseline.cpp:241  dist = qn + bn - 2*dot  (gcc contracts to fnmadd(2, dot, qn+bn))
                const float l2 = fmaf(-2.0f, acc[t][j], qn + bnj);
                d[j] = p.metric ? -acc[t][j] : l2;
                if (ragged && rbase + j > last_row) d[j] = VS_INF;
            }
            acc[t] = (f32x4){0.f, 0.f, 0.f, 0.f};
            const float dmin = fminf(fminf(d[0], d[1]), fminf(d[2], d[3]));
            if (dmin < tau) {
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (d[j] < tau) {
                        list_insert<KCAP>(ld, li, d[j], rbase + j + p.id_offset);
                        tau = fminf(tau, ld[KCAP - 1]);
                    }
                touched = true;
            }
        }
        if (touched) lds_lmin[r * 33 + 4 * wave + g] = ld[0];  // this lane's best so far, for the shared bound
        if (c_n == 1 || c_n == 2 || c_n == 4 || c_n == 8) {    // wave-uniform checkpoints
            const float sb = shared_bound();
            if (live && sb < VS_INF) tau = fminf(tau, next_up(sb));
        }
    };

    // (the ring slots are named by constants, one statement each: left to the unroller the KCAP = 16 form kept the ring
    // as an indexed array in scratch memory)
    static_assert(D == 4, "the ring is walked slot by slot below");
#define VS_ONE_ND_STEP(u)                                              \
    do {                                                               \
        if (s0 + (u) < steps_total) compute(ring[u], ring_bn[u]);      \
        issue(ring[u], ring_bn[u]);                                    \
    } while (0)
    issue(ring[0], ring_bn[0]);
    issue(ring[1], ring_bn[1]);
    issue(ring[2], ring_bn[2]);
    issue(ring[3], ring_bn[3]);
    for (int s0 = 0; s0 < steps_total; s0 += D) {
        VS_ONE_ND_STEP(0);
        VS_ONE_ND_STEP(1);
        VS_ONE_ND_STEP(2);
        VS_ONE_ND_STEP(3);
    }
#undef VS_ONE_ND_STEP

    // ---- workgroup merge (scan_one_kernel's).  A query's 32 lane lists (4 lane groups x 8 waves): the bound from the
    // lane minima bounds the workgroup's k1-th best (+inf with fewer than k1 rows); entries not above it are compacted into
    // LDS (the query fragments are done with: room for every entry, so nothing can overflow) and ranked by one wave per
    // query.
    __syncthreads();  // (every wave is done with the fragments; the lane minima are final)
    if (tid < 32) lds_cnt[tid] = 0;
    constexpr int CAP = 32 * KCAP;
    float* cand_d = reinterpret_cast<float*>(smem);
    int* cand_i = reinterpret_cast<int*>(smem + (size_t)NQ * CAP * sizeof(float));
    const float wg_bound = shared_bound();
    __syncthreads();
#pragma unroll
    for (int j = 0; j < KCAP; ++j)
        if (li[j] >= 0 && ld[j] <= wg_bound) {
            const int pos = atomicAdd(&lds_cnt[r], 1);
            cand_d[r * CAP + pos] = ld[j];
            cand_i[r * CAP + pos] = li[j];
        }
    __syncthreads();
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
            nd_rank_rounds(
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
    // ---- the workgroup that arrives last merges the partial lists (scan_one_kernel's: no fences while others stream --
    // the partial lists are written with agent-scope stores that have completed before the arrival is counted).  Nobody
    // waits for anybody: a workgroup that is not the last one is done.
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (tid == 0) lds_flag[0] = (__hip_atomic_fetch_add(p.done, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == G - 1) ? 1 : 0;
    __syncthreads();
    if (!lds_flag[0]) return;  // workgroup-uniform
    if (tid == 0) __hip_atomic_store(p.done, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // ready for the next launch (stream ordered)
    // ONE acquire fence in ONE workgroup (every other workgroup has arrived): lines of the partial lists this XCD's L2 may
    // still hold from an earlier launch are dropped, plain cached loads below.
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    // Per query two memory round trips: (1) the FIRST entry of each of its G partial lists; their k1-th smallest bounds
    // the k1-th best.  (2) the lists whose first entry is not above the bound are read whole, one (list, entry) pair per
    // lane; what is not above the bound is ranked by counting.  One wave per query.
    constexpr int QPW = kOneNdQ / kScanWaves;         // queries per wave at most: 2
    constexpr int SPL = kSlotStride / 64;             // lists per lane and query at most: 4
    constexpr int FCAP = 256;                         // candidates per query kept in LDS
    float* fin_d = reinterpret_cast<float*>(smem) + wave * FCAP;
    int* fin_i = reinterpret_cast<int*>(smem + kScanWaves * FCAP * sizeof(float)) + wave * FCAP;
    int* pl = reinterpret_cast<int*>(smem + 2 * kScanWaves * FCAP * sizeof(float)) + wave * kSlotStride;  // passing lists of the current query
    static_assert(2 * kScanWaves * FCAP * 4 + kScanWaves * kSlotStride * 4 <= kOneNdQ * 32 * 8 * 8, "the final merge's buffers fit the region");
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
        if (M <= 64) {
            const float d = lane < M ? fin_d[lane] : VS_INF;
            const int id = lane < M ? fin_i[lane] : 0x7fffffff;
            const int rank = wave_rank_count(d, id, M);
            if (lane < M && rank < p.k1) {
                od[rank] = d;
                oi[rank] = id;
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
                    oi[round] = none ? -1 : id;
                }
            };
            if (M <= FCAP) {
                nd_rank_rounds(M, p.k1, lane, [&](int e, float& d, int& id) { d = fin_d[e]; id = fin_i[e]; }, emit);
            } else {  // masses of equal distances at the bound: rank straight from the partial lists
                nd_rank_rounds(G * p.k1, p.k1, lane, [&](int e, float& d, int& id) { d = pd[e]; id = pi[e]; }, emit);
            }
            if (lane == 0 && p.flags) p.flags[qq] = tie;
        }
        __builtin_amdgcn_wave_barrier();  // (fin / pl are reused by the wave's next query)
    }
}

void scan_one_nd_geometry(int64_t n_rows, int num_cus, int64_t* grid, int64_t* units_per_wave) {
    const int64_t units = (n_rows + kOneNdUnit - 1) / kOneNdUnit;
    const int64_t g = std::max<int64_t>(1, std::min<int64_t>(std::min(num_cus, kSlotStride), (units + kScanWaves - 1) / kScanWaves));
    *grid = g;
    *units_per_wave = (units + g * kScanWaves - 1) / (g * kScanWaves);
}

template <int KCAP>
static hipError_t launch_one_nd_t(const OneNdParams& p, int grid, hipStream_t s) {
    auto kfn = scan_one_nd_kernel<KCAP>;
    static bool attr_set[64] = {};
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) dev = 0;
    if (!attr_set[dev]) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kfn), hipFuncAttributeMaxDynamicSharedMemorySize, kOneNdMaxLds);
        if (e != hipSuccess) return e;
        attr_set[dev] = true;
    }
    hipLaunchKernelGGL(kfn, dim3(grid), dim3(kScanThreads), one_nd_region(p.dim_p, KCAP) + kOneNdScratch, s, p);
    return hipGetLastError();
}

hipError_t launch_scan_one_nd(const OneNdParams& p, int grid, hipStream_t s) {
    if (p.o.nq_valid < 1 || p.o.nq_valid > kOneNdQ || p.o.k1 < 1 || p.o.k1 > 16 || grid < 1 || grid > kSlotStride || p.o.n_rows < 1 ||
        p.dim < 1 || p.dim > kNdMaxDim || p.dim_p != nd_dim_p(p.dim) || p.o.n_rows > 0x7fffffff - 2 * kOneNdUnit)
        return hipErrorInvalidValue;
    return p.o.k1 <= 8 ? launch_one_nd_t<8>(p, grid, s) : launch_one_nd_t<16>(p, grid, s);
}

}  // namespace vs
