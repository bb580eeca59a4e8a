// vs_scan_one_nd.hip -- the single-call brute-force scan at any vector length 1 <= dim <= 2048 (gfx950): ONE launch per
// batch of at most 16 queries on the fp32 rows of a general index, k + 1 <= 16.
//
//   scan_one_nd_kernel<KCAP>: scan_nd_kernel's arithmetic (v_mfma_f32_16x16x4_f32, base rows = A operand, one accumulation
//   chain per distance in the (c, i) order of DESIGN 4.4c, the half step when dim_p / 16 is odd, fma(-2, dot, qn + bn) or
//   -dot) with scan_one_kernel's top-k (per-lane sorted lists, a bound from the workgroup's lane minima at a few
//   checkpoints, one partial list per workgroup and query, the workgroup that arrives last merges them: the bound and
//   everything after the scan loop are vs_one_tail.h, shared with vs_scan_one.hip).  No preparation launch, no memset, no merge launch, and nothing anywhere waits for another workgroup.
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
#include "vs_one_tail.h"
#include "vs_one_nd_queries.h"

namespace vs {

namespace {

constexpr int kOneNdTiles = 4;                              // 16-row tiles per unit
constexpr int kOneNdUnitRows = kOneNdTiles * kTileRows;     // 64 <= kScanPadRows: a unit never reads past the spare rows
static_assert(kOneNdUnitRows == kOneNdUnit, "the plan's unit");
static_assert(kOneNdUnitRows <= kScanPadRows, "units are loaded unclamped");
static_assert(kOneNdUnitRows == 64, "one row norm per lane");
constexpr int kOneNdDepth = 4;                              // K steps in flight per wave
constexpr int kOneNdQ = 16;                                 // query columns
constexpr int kOneNdMaxLds = one_nd_lds_bytes(4 * kNdMaxDim, 16);  // (OneNdLds of vs_one_tail.h over rows of 4 dim_p bytes)

}  // namespace

template <int KCAP>
__global__ __launch_bounds__(kScanThreads, 1) void scan_one_nd_kernel(const OneNdParams pn) {
    const OneParams& p = pn.o;
    constexpr int T = kOneNdTiles;
    constexpr int D = kOneNdDepth;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int dim = pn.dim, dim_p = pn.dim_p;
    const auto L = one_nd_lds<float>(smem, 4 * dim_p, KCAP);
    f32x4* qfrag = reinterpret_cast<f32x4*>(L.tail.region);  // [dim_p / 16][64]
    float* lds_qn = L.term;                                  // [16]
    float* lds_lmin = L.tail.lmin;
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r = lane & 15, g = lane >> 4;
    const int G = (int)gridDim.x;
    const int C = dim_p / 16;            // 64-byte segments per row
    const int S = (C + 1) >> 1;          // K steps per unit; the last one is a half step when C is odd
    const bool odd = (C & 1) != 0;

    // ---- the queries: B fragments into LDS and their squared norms (vs_one_nd_queries.h)
    one_nd_stage_queries(p.q, p.nq_valid, dim, dim_p, qfrag, lds_qn);
    // the lanes' current minima, shared by the workgroup (see the checkpoints)
    one_nd_reset_lmin(lds_lmin);
    __syncthreads();
    const float qn = lds_qn[r];
    const bool live = r < p.nq_valid;
    float tau = live ? VS_INF : -VS_INF;  // a padding column never takes a candidate
    float ld[1][KCAP];  // (one column block: the shared tail's shape)
    int li[1][KCAP];
#pragma unroll
    for (int j = 0; j < KCAP; ++j) {
        ld[0][j] = VS_INF;
        li[0][j] = -1;
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

    // (the query fragments are done with: the merges overlay them)
    one_tail<1, KCAP, one_nd_region(64, KCAP)>(p, L.tail, ld, li);  // (64: the shortest padded row, dim_p = 16)
}

void scan_one_nd_geometry(int64_t n_rows, int num_cus, int64_t* grid, int64_t* units_per_wave) {
    const int64_t units = (n_rows + kOneNdUnit - 1) / kOneNdUnit;
    const int64_t g = std::max<int64_t>(1, std::min<int64_t>(std::min(num_cus, kSlotStride), (units + kScanWaves - 1) / kScanWaves));
    *grid = g;
    *units_per_wave = (units + g * kScanWaves - 1) / (g * kScanWaves);
}

template <int KCAP>
static hipError_t launch_one_nd_t(const OneNdParams& p, int grid, hipStream_t s) {
    return launch_big_lds<scan_one_nd_kernel<KCAP>, kOneNdMaxLds>(p, grid, one_nd_lds_bytes(4 * p.dim_p, KCAP), s);
}

hipError_t launch_scan_one_nd(const OneNdParams& p, int grid, hipStream_t s) {
    if (p.o.nq_valid < 1 || p.o.nq_valid > kOneNdQ || p.o.k1 < 1 || p.o.k1 > 16 || grid < 1 || grid > kSlotStride || p.o.n_rows < 1 ||
        p.dim < 1 || p.dim > kNdMaxDim || p.dim_p != nd_dim_p(p.dim) || p.o.n_rows > 0x7fffffff - 2 * kOneNdUnit)
        return hipErrorInvalidValue;
    return p.o.k1 <= 8 ? launch_one_nd_t<8>(p, grid, s) : launch_one_nd_t<16>(p, grid, s);
}

}  // namespace vs
