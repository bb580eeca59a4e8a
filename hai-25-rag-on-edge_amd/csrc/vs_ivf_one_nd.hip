// vs_ivf_one_nd.hip -- the single-call IVF search of a general index, 1 <= dim <= 2048, fp32 rows, squared L2 or inner
// product (gfx950): TWO launches per batch of at most 16 queries, k <= 16, nlist <= kIvfOneMaxNlist.
//
//   ivf_one_coarse_kernel<IP>      : every workgroup stages the caller's queries itself (vs_one_nd_queries.h), the
//                     workgroups deal the centroid table's 64-row blocks among themselves and score them with
//                     scan_nd_kernel's chain into a [16][ld] scratch; release fence, ticket; the workgroup that arrives
//                     last picks every query's nprobe smallest by (score, list id) (pick_probes_kernel's method), builds the per-list column masks and
//                     the unit table, counts the candidates, and resets the ticket.
//   ivf_one_coarse_kernel<IP, IvfOneU8Params> : its byte-index mode, for an index that keeps a byte copy of its rows (DESIGN
//                     4.6e): the same scores and probes; the last workgroup also applies the exactness rule to every
//                     query and cuts the probed lists into byte units and fp32 units for ivf_one_scan_u8_kernel
//                     (vs_ivf_one_nd_i8.hip).  The fp32 instantiations compile to the code they had without it.
//   ivf_one_scan_kernel<KCAP, IP>  : a fixed grid loops over the unit table.  A unit is at most kIvfOneUnitRows rows of
//                     one probed list, counted in 64-row blocks from the list's first row as ivf_scan_nd_kernel counts
//                     them; the 8 waves take its blocks round-robin, four 16-row tiles against the 16 query columns,
//                     K walked as ivf_scan_nd_kernel walks it (one step ahead, unclamped, no nontemporal hint: a probed
//                     list is read again by the next call).  Lane (r, g) keeps ONE sorted list for query column r across
//                     all the workgroup's units; a column takes a candidate only when r < B and the unit's list mask has
//                     bit r.  Ids are positions in the reordered rows.  Everything after the loop is vs_one_tail.h with
//                     the index's position -> original id map.
//
// Nothing waits for another workgroup: the only hand-over between workgroups is the ticket of the last arriver, in both
// launches.  Neither launch needs a preparation launch or a memset: both tickets are left at zero.
//
// Kernel contract: a coarse score is bit for bit the number launch_scan_nd (kModeStore) writes for that centroid and
// query, and a row's distance is ivf_scan_nd_kernel's -- the same accumulation chain (the (c, i) order of DESIGN 4.4c,
// the half step when dim_p / 16 is odd), then fma(-2, dot, qn + norm) or -dot.  The probes are pick_probes_kernel's, so
// ids, distance bits, empty slots and the candidate count of a call are those of ivf_group_nd_dev's launches.
#include "vs_ivf_one_scan.h"

namespace vs {

namespace {

constexpr int kIvfOnePickVPL = 16;                             // scores per lane of the selection
static_assert(64 * kIvfOnePickVPL == kIvfOneMaxNlist, "the selection keeps a query's scores in one wave's registers");

// The unit table of the byte-index mode, by the last workgroup: a probed list with column mask m gives byte units
// (unit_rows8 rows, mask m & V) and fp32 units (unit_rows rows, mask m & ~V), each kind only when its mask is non-zero;
// all byte units first.  Thread t owns lists [lo, hi).  Two prefix scans side by side: lds_scan8 [kScanThreads] overlays
// the winners, which every wave is done with (the caller's barrier).
__device__ __forceinline__ void ivf_one_unit_table_u8(const IvfOneU8Params& p, const int V, const int lo, const int hi, const int* lds_mask,
                                                      int* lds_scan, int* lds_scan8) {
    const int tid = threadIdx.x;
    const int U = p.unit_rows, U8R = p.unit_rows8;
    int nu = 0, nu8 = 0;
    for (int c = lo; c < hi; ++c) {
        const int m = lds_mask[c], rows = p.offsets[c + 1] - p.offsets[c];
        if (m & V) nu8 += (rows + U8R - 1) / U8R;
        if (m & ~V) nu += (rows + U - 1) / U;
    }
    lds_scan[tid] = nu;
    lds_scan8[tid] = nu8;
    __syncthreads();
    for (int o = 1; o < kScanThreads; o <<= 1) {  // inclusive scans
        const int a = tid >= o ? lds_scan[tid - o] : 0;
        const int a8 = tid >= o ? lds_scan8[tid - o] : 0;
        __syncthreads();
        lds_scan[tid] += a;
        lds_scan8[tid] += a8;
        __syncthreads();
    }
    const int total8 = lds_scan8[kScanThreads - 1];
    int unit8 = lds_scan8[tid] - nu8;
    int unit = total8 + lds_scan[tid] - nu;
    for (int c = lo; c < hi; ++c) {
        const int m = lds_mask[c];
        if (!m) continue;
        const int row_lo = p.offsets[c], row_end = p.offsets[c + 1];
        if (m & V)
            for (int r0 = row_lo; r0 < row_end; r0 += U8R, ++unit8)
                if (unit8 < p.units_cap) reinterpret_cast<i32x4*>(p.units)[unit8] = (i32x4){r0, min(r0 + U8R, row_end), m & V, c};
        if (m & ~V)
            for (int r0 = row_lo; r0 < row_end; r0 += U, ++unit)
                if (unit < p.units_cap) reinterpret_cast<i32x4*>(p.units)[unit] = (i32x4){r0, min(r0 + U, row_end), m & ~V, c};
    }
    if (tid == kScanThreads - 1) {
        const int n8 = min(total8, p.units_cap), n = min(total8 + lds_scan[tid], p.units_cap);
        p.n_units8[0] = n8;
        p.n_units[0] = n;
        p.counters[0] += 1ull;  // (one writer at a time: the launches of an index are stream ordered)
        if (n8 > 0 && n > n8) p.counters[1] += 1ull;
        if ((unsigned long long)n > p.counters[2]) p.counters[2] = (unsigned long long)n;
    }
}

}  // namespace

// The coarse launch.  U8 (P is IvfOneU8Params): the byte-index mode -- the last workgroup also reaches the exactness
// rule's verdict per query (ivf_nd_prep_i8's, in integers: the 16-bit mask V) from the staged queries, counts a pair on
// the byte rows or on the fp32 rows by its query's bit in V, and cuts every probed list that holds rows into byte units
// (column mask m & V) and fp32 units (m & ~V), the byte units first.  Without U8 none of that is compiled.

template <bool IP, class P = IvfOneParams>
__global__ __launch_bounds__(kScanThreads, 1) void ivf_one_coarse_kernel(const P p) {
    constexpr bool U8 = std::is_same_v<P, IvfOneU8Params>;
    constexpr int T = kIvfOneTiles;
    constexpr int NL = kIvfOneMaxNlist;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int dim = p.dim, dim_p = p.dim_p, nlist = p.nlist, B = p.o.nq_valid;
    const int region = ivf_one_coarse_region(dim_p);
    f32x4* qfrag = reinterpret_cast<f32x4*>(smem);               // [dim_p / 16][64]
    float* lds_qn = reinterpret_cast<float*>(smem + region);     // [16]
    int* lds_flag = reinterpret_cast<int*>(lds_qn + 32);         // [1]
    int* lds_mask = lds_flag + 32;                               // [NL]
    int* lds_scan = lds_mask + NL;                               // [kScanThreads]
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r = lane & 15, g = lane >> 4;
    const int G = (int)gridDim.x;
    const int C = dim_p / 16;

    one_nd_stage_queries(p.o.q, B, dim, dim_p, qfrag, lds_qn);
    __syncthreads();
    const float qn = lds_qn[r];

    // ---- the centroid table's 64-row blocks: block (n 8 + wave) G + workgroup is the wave's n-th
    const unsigned voff = (unsigned)(r * dim_p + 4 * g) * 4u;
    const unsigned tile_bytes = 64u * (unsigned)dim_p;
    const int blocks_total = (nlist + kIvfOneBlockRows - 1) / kIvfOneBlockRows;
#pragma clang loop unroll(disable)
    for (int wb = wave * G + (int)blockIdx.x; wb < blocks_total; wb += kScanWaves * G) {
        const int row0 = wb * kIvfOneBlockRows;
        const char* sb = reinterpret_cast<const char*>(p.cents + (int64_t)row0 * dim_p);
        f32x4 acc[T];
        ivf_one_block_dots(sb, voff, tile_bytes, C, qfrag, lane, acc);
#pragma unroll
        for (int t = 0; t < T; ++t) {
            const int rbase = row0 + 16 * t + 4 * g;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                float d;
                if constexpr (IP)
                    d = -acc[t][j];
                else
                    d = fmaf(-2.0f, acc[t][j], qn + p.cnorm[rbase + j]);  // (the norms have 64 spare entries)
                if (r < B && rbase + j < nlist) p.scores[(int64_t)r * p.ld + rbase + j] = d;
            }
        }
    }

    // ---- the workgroup that arrives last selects.  Nobody waits for anybody: every other workgroup is done here.
    if constexpr (U8) {
        if (tid < 17) lds_scan[tid] = 0;  // (the last arriver's per-query sums, below)
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    __syncthreads();
    if (tid == 0) lds_flag[0] = (__hip_atomic_fetch_add(p.ticket, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == G - 1) ? 1 : 0;
    __syncthreads();
    if (!lds_flag[0]) return;  // workgroup-uniform
    if (tid == 0) __hip_atomic_store(p.ticket, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // ready for the next launch (stream ordered)
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");

    for (int c = tid; c < NL; c += kScanThreads) lds_mask[c] = 0;
    if constexpr (U8) {
        // ivf_nd_prep_i8's verdict per query, in integers (n2 <= 2048 * 255^2, 0 <= bmax < 2^24), from the query fragments
        // in LDS before the winners overlay them: floats in MFMA order, and the zeros past dim and past B are bytes.
        // Fragment e belongs to query e & 15 = tid & 15 in every round of a thread; lanes r, r + 16, r + 32, r + 48 of a wave
        // add up by shuffle, the 8 waves in LDS (lds_scan [0, 16): ||q||^2, [16]: the queries with a value that is no
        // byte; cleared ahead of the ticket's barrier, used again by the unit table behind the next barrier but one).
        // No global memory is read for it: a dependent round trip in the one workgroup everybody waits for is a
        // microsecond or two of every call.
        int n2 = 0, bad = 0;
        for (int e = tid; e < C * 64; e += kScanThreads) {
            const f32x4 v = qfrag[e];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                int xi;
                if (byte_value(v[i], xi))
                    n2 += xi * xi;
                else
                    bad = 1;
            }
        }
        n2 += __shfl_xor(n2, 16);
        bad |= __shfl_xor(bad, 16);
        n2 += __shfl_xor(n2, 32);
        bad |= __shfl_xor(bad, 32);
        if (lane < 16) {
            atomicAdd(&lds_scan[lane], n2);
            if (bad) atomicOr(&lds_scan[16], 1 << lane);
        }
    }
    __syncthreads();
    int V = 0;  // byte-index mode: bit q set when query q runs on the byte rows
    if constexpr (U8) {
        const int not_bytes = lds_scan[16];
        for (int qq = 0; qq < B; ++qq)
            if (!((not_bytes >> qq) & 1) && lds_scan[qq] <= kNd8NormLimit - p.bmax) V |= 1 << qq;
    }

    // per query, one wave: the nprobe smallest by (score, list id); a NaN never competes.  pick_probes_kernel's method:
    // every lane sorts its 16 strided scores once in registers (bitonic network, static indices); a round is then one
    // wave-wide (score, id) argmin over the lanes' heads, and the winning lane shifts its run down by one -- no memory
    // traffic inside a round.  The winners are parked in LDS (the query fragments are done with) and written out, with
    // their lists' masks and row counts, by all lanes at once afterwards.
    //   (measured, 1 M rows, nlist 1024: a first form that re-read the query's scores from LDS in every round and had
    //   lane 0 look up each winner's list length before the next round cost 2.3 us per round: the coarse launch took 216 us
    //   at B = 16, nprobe 32, 96-d, and that shape was slower than the group route, 325 against 293 us)
    int* won = reinterpret_cast<int*>(smem) + wave * kIvfMaxProbe;  // [8 waves][256]
    unsigned long long rows_sum = 0, pairs_sum = 0;
    unsigned long long pairs8_sum = 0;  // byte-index mode: the pairs of the queries in V (pairs_sum: the others')
    for (int qq = wave; qq < B; qq += kScanWaves) {
        float v[kIvfOnePickVPL];
        int id[kIvfOnePickVPL];
#pragma unroll
        for (int i = 0; i < kIvfOnePickVPL; ++i) {
            const int c = i * 64 + lane;
            const float x = c < nlist ? p.scores[(int64_t)qq * p.ld + c] : VS_INF;
            const bool ok = c < nlist && x == x;
            v[i] = ok ? x : VS_INF;
            id[i] = ok ? c : 0x7fffffff;
        }
#pragma unroll
        for (int k = 2; k <= kIvfOnePickVPL; k <<= 1)
#pragma unroll
            for (int j = k >> 1; j > 0; j >>= 1)
#pragma unroll
                for (int i = 0; i < kIvfOnePickVPL; ++i) {
                    const int l = i ^ j;
                    if (l > i) {
                        const bool up = (i & k) == 0;
                        const bool sw = up ? lex_lt(v[l], id[l], v[i], id[i]) : lex_lt(v[i], id[i], v[l], id[l]);
                        const float tv = sw ? v[l] : v[i];
                        const int ti = sw ? id[l] : id[i];
                        v[l] = sw ? v[i] : v[l];
                        id[l] = sw ? id[i] : id[l];
                        v[i] = tv;
                        id[i] = ti;
                    }
                }
        for (int round = 0; round < p.nprobe; ++round) {
            float bd;
            int bi;
            wave_lexmin(v[0], id[0], bd, bi);
            if (lane == 0) won[round] = bi == 0x7fffffff ? -1 : bi;
            if (id[0] == bi && bi != 0x7fffffff) {  // (ids are unique: one lane) its run moves down by one
#pragma unroll
                for (int i = 0; i + 1 < kIvfOnePickVPL; ++i) {
                    v[i] = v[i + 1];
                    id[i] = id[i + 1];
                }
                v[kIvfOnePickVPL - 1] = VS_INF;
                id[kIvfOnePickVPL - 1] = 0x7fffffff;
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        for (int e = lane; e < p.nprobe; e += 64) {
            const int c = won[e];
            p.probes[(int64_t)qq * p.nprobe + e] = c;
            if (c < 0) continue;
            const int rows = p.offsets[c + 1] - p.offsets[c];
            if (rows > 0) {
                atomicOr(&lds_mask[c], 1 << qq);
                rows_sum += (unsigned long long)rows;
                if (U8 && ((V >> qq) & 1))
                    ++pairs8_sum;
                else
                    ++pairs_sum;
            }
        }
        __builtin_amdgcn_wave_barrier();  // (won is reused by the wave's next query)
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        rows_sum += __shfl_xor(rows_sum, o);
        pairs_sum += __shfl_xor(pairs_sum, o);
        if constexpr (U8) pairs8_sum += __shfl_xor(pairs8_sum, o);
    }
    if (lane == 0 && rows_sum && p.cand_count) atomicAdd(p.cand_count, rows_sum);
    if (lane == 0 && pairs_sum && p.pair_count) atomicAdd(p.pair_count, pairs_sum);
    if constexpr (U8) {
        if (lane == 0 && pairs8_sum && p.pair_count8) atomicAdd(p.pair_count8, pairs8_sum);
    }
    __syncthreads();

    // the unit table: every probed list that holds rows, cut into units of unit_rows rows.  Thread t owns lists
    // [t per, (t + 1) per).
    const int U = p.unit_rows;
    const int per = (nlist + kScanThreads - 1) / kScanThreads;
    const int lo = min(tid * per, nlist), hi = min(lo + per, nlist);
    if constexpr (U8) {
        ivf_one_unit_table_u8(p, V, lo, hi, lds_mask, lds_scan, reinterpret_cast<int*>(smem));
        return;
    }
    int nu = 0;
    for (int c = lo; c < hi; ++c)
        if (lds_mask[c]) nu += (p.offsets[c + 1] - p.offsets[c] + U - 1) / U;
    lds_scan[tid] = nu;
    __syncthreads();
    for (int o = 1; o < kScanThreads; o <<= 1) {  // inclusive scan
        const int a = tid >= o ? lds_scan[tid - o] : 0;
        __syncthreads();
        lds_scan[tid] += a;
        __syncthreads();
    }
    int unit = lds_scan[tid] - nu;
    for (int c = lo; c < hi; ++c) {
        const int m = lds_mask[c];
        if (!m) continue;
        const int row_lo = p.offsets[c], row_end = p.offsets[c + 1];
        for (int r0 = row_lo; r0 < row_end; r0 += U, ++unit)
            if (unit < p.units_cap) reinterpret_cast<i32x4*>(p.units)[unit] = (i32x4){r0, min(r0 + U, row_end), m, c};
    }
    if (tid == kScanThreads - 1) {
        const int n = min(lds_scan[tid], p.units_cap);
        p.n_units[0] = n;
        p.counters[0] += 1ull;  // (one writer at a time: the launches of an index are stream ordered)
        if ((unsigned long long)n > p.counters[1]) p.counters[1] = (unsigned long long)n;
    }
}

template <int KCAP, bool IP>
__global__ __launch_bounds__(kScanThreads, 1) void ivf_one_scan_kernel(const IvfOneParams p) {
    constexpr int T = kIvfOneTiles;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int dim_p = p.dim_p, B = p.o.nq_valid;
    const auto L = one_nd_lds<float>(smem, 4 * dim_p, KCAP);
    f32x4* qfrag = reinterpret_cast<f32x4*>(L.tail.region);  // [dim_p / 16][64]
    float* lds_qn = L.term;        // [16]
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r = lane & 15, g = lane >> 4;
    const int C = dim_p / 16;
    const int n_units = p.n_units[0];  // (the coarse launch's, stream ordered)
    const bool has_units = (int)blockIdx.x < n_units;  // a workgroup without units goes straight to the ticket

    if (has_units) one_nd_stage_queries(p.o.q, B, p.dim, dim_p, qfrag, lds_qn);
    one_nd_reset_lmin(L.tail.lmin);
    __syncthreads();
    float qn = 0.f;
    if constexpr (!IP) qn = has_units ? lds_qn[r] : 0.f;
    const bool live = r < B;
    float tau = VS_INF;  // the column's bound
    float ld[1][KCAP];
    int li[1][KCAP];
#pragma unroll
    for (int j = 0; j < KCAP; ++j) {
        ld[0][j] = VS_INF;
        li[0][j] = -1;
    }
    const unsigned voff = (unsigned)(r * dim_p + 4 * g) * 4u;  // this lane's 16 bytes inside a 16-row tile's segment
    const unsigned tile_bytes = 64u * (unsigned)dim_p;         // 16 rows
    int c_n = 0;  // blocks this wave has done (wave-uniform): the checkpoints of the shared bound

    VS_IVF_ONE_UNITS_F32(blockIdx.x)

    // (the query fragments are done with: the merges overlay them)
    one_tail<1, KCAP, one_nd_region(64, KCAP)>(p.o, L.tail, ld, li, IvfOneIdMap{p.id_map});  // (64: the shortest row, dim_p = 16)
}

int ivf_one_coarse_grid(int nlist, int num_cus) {
    const int blocks = (nlist + kIvfOneBlockRows - 1) / kIvfOneBlockRows;
    return std::max(1, std::min(std::min(num_cus, kSlotStride), blocks));
}

int ivf_one_scan_grid(int num_cus) { return std::max(1, std::min(num_cus, kSlotStride)); }

bool ivf_one_params_ok(const IvfOneParams& p) {
    return p.dim >= 1 && p.dim <= kNdMaxDim && p.dim_p == nd_dim_p(p.dim) && p.nlist >= 1 && p.nlist <= kIvfOneMaxNlist && p.o.nq_valid >= 1 &&
           p.o.nq_valid <= kIvfOneQ && p.o.k1 >= 1 && p.o.k1 <= 16 && p.nprobe >= 1 && p.nprobe <= kIvfMaxProbe && p.nprobe <= p.nlist &&
           p.unit_rows >= kIvfOneBlockRows && p.unit_rows % kIvfOneBlockRows == 0 && p.units_cap >= 1 && p.ld >= p.nlist &&
           (p.metric == 0 || p.metric == 1);
}

hipError_t launch_ivf_one_coarse(const IvfOneParams& p, int grid, hipStream_t s) {
    if (!ivf_one_params_ok(p) || grid < 1 || grid > kSlotStride) return hipErrorInvalidValue;
    const int lds = ivf_one_coarse_region(p.dim_p) + kIvfOneCoarseScratch;
    return p.metric ? launch_big_lds<ivf_one_coarse_kernel<true>, kIvfOneMaxLds>(p, grid, lds, s) : launch_big_lds<ivf_one_coarse_kernel<false>, kIvfOneMaxLds>(p, grid, lds, s);
}

hipError_t launch_ivf_one_coarse_u8(const IvfOneU8Params& p, int grid, hipStream_t s) {
    if (!ivf_one_params_ok(p) || grid < 1 || grid > kSlotStride || p.dim_b != nd_dim_b(p.dim) || p.bmax < 0 || p.bmax >= kNd8NormLimit ||
        p.unit_rows8 < kIvfOneBlockRows || p.unit_rows8 % kIvfOneBlockRows || !p.n_units8)
        return hipErrorInvalidValue;
    const int lds = ivf_one_coarse_region(p.dim_p) + kIvfOneCoarseScratch;
    return p.metric ? launch_big_lds<ivf_one_coarse_kernel<true, IvfOneU8Params>, kIvfOneMaxLds>(p, grid, lds, s)
                      : launch_big_lds<ivf_one_coarse_kernel<false, IvfOneU8Params>, kIvfOneMaxLds>(p, grid, lds, s);
}

hipError_t launch_ivf_one_scan(const IvfOneParams& p, int grid, hipStream_t s) {
    if (!ivf_one_params_ok(p) || grid < 1 || grid > kSlotStride) return hipErrorInvalidValue;
    const int kcap = p.o.k1 <= 8 ? 8 : 16;
    const int lds = one_nd_lds_bytes(4 * p.dim_p, kcap);
    if (kcap == 8)
        return p.metric ? launch_big_lds<ivf_one_scan_kernel<8, true>, kIvfOneMaxLds>(p, grid, lds, s) : launch_big_lds<ivf_one_scan_kernel<8, false>, kIvfOneMaxLds>(p, grid, lds, s);
    return p.metric ? launch_big_lds<ivf_one_scan_kernel<16, true>, kIvfOneMaxLds>(p, grid, lds, s) : launch_big_lds<ivf_one_scan_kernel<16, false>, kIvfOneMaxLds>(p, grid, lds, s);
}

}  // namespace vs
