// vs_ivf_one_nd.hip -- the single-call IVF search of a general index, 1 <= dim <= 2048, fp32 rows, squared L2 or inner
// product (gfx950): TWO launches per batch of at most 16 queries, k <= 16, nlist <= kIvfOneMaxNlist.
//
//   ivf_one_coarse_kernel<IP>      : every workgroup stages the caller's queries itself (vs_one_nd_queries.h), the
//                     workgroups deal the centroid table's 64-row blocks among themselves and score them with
//                     scan_nd_kernel's chain into a [16][ld] scratch; release fence, ticket; the workgroup that arrives
//                     last picks every query's nprobe smallest by (score, list id) (pick_probes_kernel's method), builds the per-list column masks and
//                     the unit table, counts the candidates, and resets the ticket.
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
#include "vs_kernels.h"
#include "vs_dev.h"
#include "vs_one_tail.h"
#include "vs_one_nd_queries.h"

namespace vs {

namespace {

constexpr int kIvfOneTiles = 4;                                // 16-row tiles per wave block
constexpr int kIvfOneBlockRows = kIvfOneTiles * kTileRows;     // 64 <= kScanPadRows: a block never reads past the spare rows
static_assert(kIvfOneBlockRows <= kScanPadRows, "row blocks are loaded unclamped");
static_assert(kIvfOneUnitRows % kIvfOneBlockRows == 0, "a unit is whole blocks, counted from the list's first row");
constexpr int kIvfOneQ = 16;                                   // query columns
constexpr int kIvfOnePickVPL = 16;                             // scores per lane of the selection
static_assert(64 * kIvfOnePickVPL == kIvfOneMaxNlist, "the selection keeps a query's scores in one wave's registers");
// (the scan's LDS is OneNdLds of vs_one_tail.h over rows of 4 dim_p bytes)
// coarse: query fragments, later the last arriver's winners [8 waves][kIvfMaxProbe]; behind them norms [32] | flag [32] |
// masks [kIvfOneMaxNlist] | prefix scan [kScanThreads]
constexpr int kIvfOneCoarseScratch = (32 + 32 + kIvfOneMaxNlist + kScanThreads) * 4;
constexpr int ivf_one_coarse_region(int dim_p) {
    const int frag = dim_p * 64, sel = kScanWaves * kIvfMaxProbe * 4;
    return frag > sel ? frag : sel;
}
constexpr int kIvfOneCoarseMaxLds = ivf_one_coarse_region(kNdMaxDim) + kIvfOneCoarseScratch;
constexpr int kIvfOneMaxLds = kIvfOneCoarseMaxLds > one_nd_lds_bytes(4 * kNdMaxDim, 16) ? kIvfOneCoarseMaxLds : one_nd_lds_bytes(4 * kNdMaxDim, 16);
static_assert(kIvfOneMaxLds <= 160 * 1024, "LDS of a CU");

// The dot products of one 64-row block (four 16-row tiles at sb) with the 16 staged query columns: scan_nd_kernel's chain,
// the B fragments from LDS.  Row loads run one K step ahead of the MFMAs.
__device__ __forceinline__ void ivf_one_block_dots(const char* sb, unsigned voff, unsigned tile_bytes, int C, const f32x4* qfrag, int lane,
                                                   f32x4 (&acc)[kIvfOneTiles]) {
    constexpr int T = kIvfOneTiles;
    const int n_pairs = C >> 1;  // full 32-float steps
#pragma unroll
    for (int t = 0; t < T; ++t) acc[t] = (f32x4){0.f, 0.f, 0.f, 0.f};
    f32x4 a[T][2];
    auto load_pair = [&](int s, f32x4 (&av)[T][2]) __attribute__((always_inline)) {
#pragma unroll
        for (int t = 0; t < T; ++t) {
            av[t][0] = *(reinterpret_cast<const f32x4*>(sb + (t * tile_bytes + 128u * s) + voff));
            av[t][1] = *(reinterpret_cast<const f32x4*>(sb + (t * tile_bytes + 128u * s + 64u) + voff));
        }
    };
    auto mfma_half = [&](const f32x4 (&av)[T][2], const f32x4 bv, int u) __attribute__((always_inline)) {
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int t = 0; t < T; ++t) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[t][u][i], bv[i], acc[t], 0, 0, 0);
    };
    if (n_pairs > 0) load_pair(0, a);
    for (int s = 0; s < n_pairs; ++s) {
        f32x4 an[T][2];
        const bool more = s + 1 < n_pairs;
        if (more) load_pair(s + 1, an);
        const f32x4 b0 = qfrag[(2 * s) * 64 + lane], b1 = qfrag[(2 * s + 1) * 64 + lane];
        mfma_half(a, b0, 0);
        mfma_half(a, b1, 1);
        if (more) {
#pragma unroll
            for (int t = 0; t < T; ++t) {
                a[t][0] = an[t][0];
                a[t][1] = an[t][1];
            }
        }
    }
    if (C & 1) {  // the last 16 floats of a row whose dim_p is an odd number of segments
#pragma unroll
        for (int t = 0; t < T; ++t) a[t][0] = *(reinterpret_cast<const f32x4*>(sb + (t * tile_bytes + 128u * n_pairs) + voff));
        mfma_half(a, qfrag[(2 * n_pairs) * 64 + lane], 0);
    }
}

// position in the reordered rows -> the caller's id
struct IvfOneIdMap {
    const int32_t* map;  // null: identity
    __device__ __forceinline__ int operator()(int id) const { return map ? map[id] : id; }
};

}  // namespace

template <bool IP>
__global__ __launch_bounds__(kScanThreads, 1) void ivf_one_coarse_kernel(const IvfOneParams p) {
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
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    __syncthreads();
    if (tid == 0) lds_flag[0] = (__hip_atomic_fetch_add(p.ticket, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == G - 1) ? 1 : 0;
    __syncthreads();
    if (!lds_flag[0]) return;  // workgroup-uniform
    if (tid == 0) __hip_atomic_store(p.ticket, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // ready for the next launch (stream ordered)
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");

    for (int c = tid; c < NL; c += kScanThreads) lds_mask[c] = 0;
    __syncthreads();

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
                ++pairs_sum;
            }
        }
        __builtin_amdgcn_wave_barrier();  // (won is reused by the wave's next query)
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        rows_sum += __shfl_xor(rows_sum, o);
        pairs_sum += __shfl_xor(pairs_sum, o);
    }
    if (lane == 0 && rows_sum && p.cand_count) atomicAdd(p.cand_count, rows_sum);
    if (lane == 0 && pairs_sum && p.pair_count) atomicAdd(p.pair_count, pairs_sum);
    __syncthreads();

    // the unit table: every probed list that holds rows, cut into units of unit_rows rows.  Thread t owns lists
    // [t per, (t + 1) per).
    const int U = p.unit_rows;
    const int per = (nlist + kScanThreads - 1) / kScanThreads;
    const int lo = min(tid * per, nlist), hi = min(lo + per, nlist);
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

#pragma clang loop unroll(disable)
    for (int unit = blockIdx.x; unit < n_units; unit += gridDim.x) {
        const i32x4 u = reinterpret_cast<const i32x4*>(p.units)[unit];
        const int row_lo = u[0], row_end = u[1];  // (a unit that is not its list's last ends on a block boundary)
        const int last_row = row_end - 1;
        const bool mine = live && ((u[2] >> r) & 1);
        const int blocks_total = (row_end - row_lo + kIvfOneBlockRows - 1) / kIvfOneBlockRows;
#pragma clang loop unroll(disable)
        for (int wb = wave; wb < blocks_total; wb += kScanWaves) {
            const int row0 = row_lo + wb * kIvfOneBlockRows;
            const char* sb = reinterpret_cast<const char*>(p.vecs + (int64_t)row0 * dim_p);
            f32x4 acc[T];
            ivf_one_block_dots(sb, voff, tile_bytes, C, qfrag, lane, acc);
            const bool ragged = row0 + kIvfOneBlockRows - 1 > last_row;  // wave-uniform
            bool touched = false;
#pragma unroll
            for (int t = 0; t < T; ++t) {
                const int rbase = row0 + 16 * t + 4 * g;
                float d[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    if constexpr (IP)
                        d[j] = -acc[t][j];  // (an exactly zero product is +0 out of the chain: -0.0)
                    else
                        d[j] = fmaf(-2.0f, acc[t][j], qn + p.vnorm[rbase + j]);  // (the norms have 64 spare entries)
                    if (ragged && rbase + j > last_row) d[j] = VS_INF;  // (under IP a spare row's -0.0 must never compete)
                }
                const float dmin = fminf(fminf(d[0], d[1]), fminf(d[2], d[3]));
                if (dmin < (mine ? tau : -VS_INF)) {  // (a column outside the mask: its bound is -inf)
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        if (d[j] < tau) {
                            list_insert<KCAP>(ld[0], li[0], d[j], rbase + j);
                            tau = fminf(tau, ld[0][KCAP - 1]);
                        }
                    touched = true;
                }
            }
            if (touched) L.tail.lmin[r * 33 + 4 * wave + g] = ld[0][0];  // this lane's best so far, for the shared bound
            ++c_n;
            if (c_n == 1 || c_n == 2 || c_n == 4 || c_n == 8 || c_n == 16) {  // wave-uniform checkpoints
                // the k-th smallest of the column's lane minima: k distinct rows of the column's probed lists are at
                // least that close (vs_one_tail.h); whatever the other waves have published by now, stale only loosens it
                const float sbound = one_shared_bound(L.tail.lmin, r, g, p.o.k1);
                if (live && sbound < VS_INF) tau = fminf(tau, next_up(sbound));
            }
        }
    }

    // (the query fragments are done with: the merges overlay them)
    one_tail<1, KCAP, one_nd_region(64, KCAP)>(p.o, L.tail, ld, li, IvfOneIdMap{p.id_map});  // (64: the shortest row, dim_p = 16)
}

int ivf_one_coarse_grid(int nlist, int num_cus) {
    const int blocks = (nlist + kIvfOneBlockRows - 1) / kIvfOneBlockRows;
    return std::max(1, std::min(std::min(num_cus, kSlotStride), blocks));
}

int ivf_one_scan_grid(int num_cus) { return std::max(1, std::min(num_cus, kSlotStride)); }

static bool ivf_one_params_ok(const IvfOneParams& p) {
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

hipError_t launch_ivf_one_scan(const IvfOneParams& p, int grid, hipStream_t s) {
    if (!ivf_one_params_ok(p) || grid < 1 || grid > kSlotStride) return hipErrorInvalidValue;
    const int kcap = p.o.k1 <= 8 ? 8 : 16;
    const int lds = one_nd_lds_bytes(4 * p.dim_p, kcap);
    if (kcap == 8)
        return p.metric ? launch_big_lds<ivf_one_scan_kernel<8, true>, kIvfOneMaxLds>(p, grid, lds, s) : launch_big_lds<ivf_one_scan_kernel<8, false>, kIvfOneMaxLds>(p, grid, lds, s);
    return p.metric ? launch_big_lds<ivf_one_scan_kernel<16, true>, kIvfOneMaxLds>(p, grid, lds, s) : launch_big_lds<ivf_one_scan_kernel<16, false>, kIvfOneMaxLds>(p, grid, lds, s);
}

}  // namespace vs
