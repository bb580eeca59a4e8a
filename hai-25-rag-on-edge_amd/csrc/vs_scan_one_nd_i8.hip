// vs_scan_one_nd_i8.hip -- the single-call byte scan of a general index made from uint8 rows (gfx950): ONE launch per batch
// of at most 16 queries on the int8 rows (x - 128, padded to dim_b) of a vs_bf_create_nd_u8* index, k + 1 <= 16, squared
// L2 and inner product.
//
//   scan_one_nd_i8_kernel<KCAP, IP>: scan_nd_i8_kernel's arithmetic (v_mfma_i32_16x16x64_i8, base rows = A operand, one
//   query block = B; (float)(qterm + rterm - 2 acc), or -(float)(qt_ip + 128 rsum + acc) under inner product) in
//   scan_one_nd_kernel's organisation: per-lane sorted lists, a bound from the workgroup's lane minima at a few
//   checkpoints, one partial list per workgroup and query, the workgroup that arrives last merges them (vs_one_tail.h).
//   No preparation launch, no memset, no merge launch, and nothing anywhere waits for another workgroup.
//
//   Queries and the verdict.  Every workgroup reads the caller's unpadded [B][dim] floats itself, once: it writes them as
//   bytes (x - 128), zero-padded, in MFMA B-fragment order into LDS (dim_b / 64 fragments of 1 KB: 32 KB at dim 2048),
//   works out the per-query term in integers and reaches nd_prep_i8_kernel's verdict (vs_one_nd_queries.h).  The verdict
//   is a pure function of the queries and bmax, so every workgroup reaches the same one by itself.  A refused batch
//   scans nothing: the tail runs on empty lane lists (ids -1, distances +inf) and the workgroup that arrives last leaves
//   flags = 2 for all the batch's queries -- the contract of scan_nd_i8_kernel's merge, which the host calls rerun on.
//
//   Rows.  scan_one_nd_kernel's: a unit is kOneNd8Tiles 16-row tiles (64 rows), unit (n G + workgroup) 8 + wave is the
//   wave's n-th.  A K step is 128 bytes per row (two 16-byte pieces per lane and tile: the fp32 kernel's 8 loads of 16
//   bytes, the same 128 VGPRs of ring), with a 64-byte half step when dim_b / 64 is odd.  The steps of ALL the wave's
//   units form one stream, kOneNd8Depth steps ahead of the MFMAs in a register ring, across unit boundaries.  The row's
//   int32 term rides in the ring (one int per lane and step).  Past the wave's last step the ring is fed with loads of
//   one fixed line, so that every step issues the same number of loads.  All loads are ordinary global loads whose
//   waits the compiler places.
#include "vs_kernels.h"
#include "vs_dev.h"
#include "vs_one_tail.h"
#include "vs_one_nd_queries.h"

namespace vs {

namespace {

constexpr int kOneNd8Tiles = 4;                               // 16-row tiles per unit
constexpr int kOneNd8UnitRows = kOneNd8Tiles * kTileRows;     // 64 <= kScanPadRows: a unit never reads past the spare rows
static_assert(kOneNd8UnitRows == kOneNdUnit, "the plan's unit");
static_assert(kOneNd8UnitRows <= kScanPadRows, "units are loaded unclamped");
static_assert(kOneNd8UnitRows == 64, "one row term per lane");
constexpr int kOneNd8Depth = 4;                               // K steps in flight per wave
constexpr int kOneNd8Q = 16;                                  // query columns
constexpr int kOneNd8MaxLds = one_nd_lds_bytes(kNdMaxDim, 16);  // (OneNdLds of vs_one_tail.h over rows of dim_b bytes)

}  // namespace

template <int KCAP, bool IP>
__global__ __launch_bounds__(kScanThreads, 1) void scan_one_nd_i8_kernel(const OneNdI8Params pn) {
    const OneParams& p = pn.o;
    constexpr int T = kOneNd8Tiles;
    constexpr int D = kOneNd8Depth;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int dim_b = pn.dim_b;
    const auto L = one_nd_lds<int>(smem, dim_b, KCAP);
    i32x4* qfrag = reinterpret_cast<i32x4*>(L.tail.region);  // [dim_b / 64][64]
    int* lds_qt = L.term;                                    // [16]
    int* lds_flag = L.tail.flag;
    float* lds_lmin = L.tail.lmin;
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r = lane & 15, g = lane >> 4;
    const int G = (int)gridDim.x;
    const int C = dim_b / 64;            // 64-byte segments per row
    const int S = (C + 1) >> 1;          // K steps per unit; the last one is a half step when C is odd
    const bool odd = (C & 1) != 0;

    // the lanes' current minima, shared by the workgroup (see the checkpoints)
    one_nd_reset_lmin(lds_lmin);
    // ---- the queries: byte B fragments into LDS, their terms, and the batch verdict (vs_one_nd_queries.h; ends with a barrier)
    const bool run = one_nd_stage_queries_i8<IP>(p.q, p.nq_valid, pn.dim, dim_b, pn.bmax, qfrag, lds_qt);  // workgroup-uniform
    const int qt = lds_qt[r];
    const bool live = r < p.nq_valid;
    float tau = live ? VS_INF : -VS_INF;  // a padding column never takes a candidate
    float ld[1][KCAP];  // (one column block: the shared tail's shape)
    int li[1][KCAP];
#pragma unroll
    for (int j = 0; j < KCAP; ++j) {
        ld[0][j] = VS_INF;
        li[0][j] = -1;
    }

    // ---- the wave's units, dealt and walked as in scan_one_nd_kernel: run n of the base = units [n 8 G, (n + 1) 8 G);
    // p.reverse walks the FULL runs from the last to the first, an incomplete last run stays the wave's last unit.  A
    // refused batch has no units: the loop below does not run and the lane lists stay empty.
    const int units_total = (int)((p.n_rows + kOneNd8UnitRows - 1) / kOneNd8UnitRows);
    const int per_run = G * kScanWaves;
    const int n_full = units_total / per_run;
    const int my = (int)blockIdx.x * kScanWaves + wave;
    const int n_mine = run ? n_full + (n_full * per_run + my < units_total ? 1 : 0) : 0;
    auto unit_of = [&](int n) { return ((p.reverse && n < n_full) ? n_full - 1 - n : n) * per_run + my; };
    const int steps_total = n_mine * S;  // (<= 2^25 units / 8 waves x 16 steps: fits)

    const unsigned voff = (unsigned)(r * dim_b + 16 * g);  // this lane's 16 bytes inside a 16-row tile's 64-byte segment
    const unsigned tile_bytes = 16u * (unsigned)dim_b;     // 16 rows
    const char* const base_c = reinterpret_cast<const char*>(pn.base_u8);
    const int32_t* const row_term = IP ? pn.rsum : pn.rterm;
    const int last_row = (int)p.n_rows - 1;

    // the ring: D steps of T x 2 pieces of 16 bytes and one row term per lane
    i32x4 ring[D][T][2];
    int ring_rt[D];
    int l_n = 0, l_s = 0;  // load cursor: unit l_n of the wave, step l_s
    auto issue = [&](i32x4 (&av)[T][2], int& rtv) __attribute__((always_inline)) {
        const bool have = l_n < n_mine;  // (wave-uniform) past the end: T x 2 + 1 loads of the base's first line
        const int64_t row0 = have ? (int64_t)unit_of(l_n) * kOneNd8UnitRows : 0;
        const char* sb = base_c + (have ? row0 * (int64_t)dim_b + 128 * (int64_t)l_s : 0);
        const unsigned tb = have ? tile_bytes : 0u, vo = have ? voff : 0u;
        const unsigned h2 = (have && !(odd && l_s == S - 1)) ? 64u : 0u;  // a half step reads its first piece twice
#pragma unroll
        for (int t = 0; t < T; ++t) {
            av[t][0] = __builtin_nontemporal_load(reinterpret_cast<const i32x4*>(sb + (t * tb + vo)));
            av[t][1] = __builtin_nontemporal_load(reinterpret_cast<const i32x4*>(sb + (t * tb + h2 + vo)));
        }
        rtv = row_term[row0 + lane];  // (the terms have 64 spare entries)
        if (++l_s == S) {
            l_s = 0;
            ++l_n;
        }
    };

    i32x4 acc[T];
#pragma unroll
    for (int t = 0; t < T; ++t) acc[t] = (i32x4){0, 0, 0, 0};
    int rt_cur = 0;
    int c_n = 0, c_s = 0;  // compute cursor
    auto compute = [&](const i32x4 (&av)[T][2], const int rtv) __attribute__((always_inline)) {
        if (c_s == 0) rt_cur = rtv;  // (every step of the unit carries it; the first one's is kept)
        const bool half = odd && c_s == S - 1;
        const i32x4 b0 = qfrag[(2 * c_s) * 64 + lane];
        const i32x4 b1 = qfrag[(half ? 2 * c_s : 2 * c_s + 1) * 64 + lane];
#pragma unroll
        for (int t = 0; t < T; ++t) acc[t] = __builtin_amdgcn_mfma_i32_16x16x64_i8(av[t][0], b0, acc[t], 0, 0, 0);
        if (!half) {
#pragma unroll
            for (int t = 0; t < T; ++t) acc[t] = __builtin_amdgcn_mfma_i32_16x16x64_i8(av[t][1], b1, acc[t], 0, 0, 0);
        }
        if (++c_s < S) return;
        // ---- the unit's distances
        c_s = 0;
        const int row0 = unit_of(c_n) * kOneNd8UnitRows;
        ++c_n;
        const bool ragged = row0 + kOneNd8UnitRows - 1 > last_row;  // wave-uniform
        bool touched = false;
#pragma unroll
        for (int t = 0; t < T; ++t) {
            const int rbase = row0 + 16 * t + 4 * g;
            float d[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int rtj = __shfl(rt_cur, 16 * t + 4 * g + j);
                // scan_nd_i8_kernel's: the integer the fp32 path computes exactly, ||q||^2 + ||b||^2 - 2 q.b, or -(q.b) with
                // q.b = q'.b' + 128 (sum q' + sum b') + 128^2 dim (a zero product gives -0.0 like the fp32 scan's negation)
                if constexpr (IP)
                    d[j] = -(float)(qt + 128 * rtj + acc[t][j]);
                else
                    d[j] = (float)(qt + rtj - 2 * acc[t][j]);
                if (ragged && rbase + j > last_row) d[j] = VS_INF;
            }
            acc[t] = (i32x4){0, 0, 0, 0};
            const float dmin = fminf(fminf(d[0], d[1]), fminf(d[2], d[3]));
            if (dmin < tau) {
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (d[j] < tau) {
                        list_insert<KCAP>(ld[0], li[0], d[j], rbase + j + p.id_offset);
                        tau = fminf(tau, ld[0][KCAP - 1]);
                    }
                touched = true;
            }
        }
        if (touched) lds_lmin[r * 33 + 4 * wave + g] = ld[0][0];  // this lane's best so far, for the shared bound
        if (c_n == 1 || c_n == 2 || c_n == 4 || c_n == 8) {    // wave-uniform checkpoints
            const float sb = one_shared_bound(lds_lmin, r, g, p.k1);
            if (live && sb < VS_INF) tau = fminf(tau, next_up(sb));
        }
    };

    // (the ring slots are named by constants, one statement each, as in scan_one_nd_kernel: an indexed ring goes to
    // scratch memory)
    static_assert(D == 4, "the ring is walked slot by slot below");
#define VS_ONE_ND8_STEP(u)                                             \
    do {                                                               \
        if (s0 + (u) < steps_total) compute(ring[u], ring_rt[u]);      \
        issue(ring[u], ring_rt[u]);                                    \
    } while (0)
    issue(ring[0], ring_rt[0]);
    issue(ring[1], ring_rt[1]);
    issue(ring[2], ring_rt[2]);
    issue(ring[3], ring_rt[3]);
    for (int s0 = 0; s0 < steps_total; s0 += D) {
        VS_ONE_ND8_STEP(0);
        VS_ONE_ND8_STEP(1);
        VS_ONE_ND8_STEP(2);
        VS_ONE_ND8_STEP(3);
    }
#undef VS_ONE_ND8_STEP

    // (the query fragments are done with: the merges overlay them)
    one_tail<1, KCAP, one_nd_region(64, KCAP)>(p, L.tail, ld, li);  // (64: the shortest padded row)
    // a refused batch: the workgroup that arrived last (the only one whose flag word is set) overwrites the tail's
    // flags with the verdict -- the lanes that wrote them there (lane 0 of wave q & 7), after a barrier
    if (!run) {  // workgroup-uniform
        __syncthreads();
        if (lds_flag[0] && lane == 0 && p.flags)
            for (int qq = wave; qq < p.nq_valid; qq += kScanWaves) p.flags[qq] = 2;
    }
}

template <int KCAP, bool IP>
static hipError_t launch_one_nd_i8_t(const OneNdI8Params& p, int grid, hipStream_t s) {
    return launch_big_lds<scan_one_nd_i8_kernel<KCAP, IP>, kOneNd8MaxLds>(p, grid, one_nd_lds_bytes(p.dim_b, KCAP), s);
}

hipError_t launch_scan_one_nd_i8(const OneNdI8Params& p, int grid, hipStream_t s) {
    if (p.o.nq_valid < 1 || p.o.nq_valid > kOneNd8Q || p.o.k1 < 1 || p.o.k1 > 16 || grid < 1 || grid > kSlotStride || p.o.n_rows < 1 ||
        p.dim < 1 || p.dim > kNdMaxDim || p.dim_b != nd_dim_b(p.dim) || p.o.n_rows > 0x7fffffff - 2 * kOneNdUnit || !p.base_u8 ||
        (p.o.metric != 0 && p.o.metric != 1) || !(p.o.metric ? p.rsum : p.rterm) || p.bmax < 0 || p.bmax >= kNd8NormLimit)
        return hipErrorInvalidValue;
    if (p.o.metric) return p.o.k1 <= 8 ? launch_one_nd_i8_t<8, true>(p, grid, s) : launch_one_nd_i8_t<16, true>(p, grid, s);
    return p.o.k1 <= 8 ? launch_one_nd_i8_t<8, false>(p, grid, s) : launch_one_nd_i8_t<16, false>(p, grid, s);
}

}  // namespace vs
