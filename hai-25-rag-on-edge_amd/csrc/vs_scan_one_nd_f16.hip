// vs_scan_one_nd_f16.hip -- the single-call brute-force scan on the half rows of a vs_bf_create_nd_f16 index (gfx950): ONE
// launch per batch of at most 16 queries, k + 1 <= 16, at any vector length 1 <= dim <= 2048.
//
//   scan_one_nd_f16_kernel<KCAP>: scan_one_nd_kernel's organisation (per-lane sorted lists, a bound from the workgroup's
//   lane minima at a few checkpoints, one partial list per workgroup and query, the workgroup that arrives last merges
//   them: vs_one_tail.h) on scan_nd_f16_kernel's row side (rows stored as halves in the permuted layout of DESIGN 4.4g,
//   widened in registers, v_mfma_f32_16x16x4_f32 in that kernel's order: segment 2 s then 2 s + 1, inside a segment i
//   outer and tile inner -- one accumulation chain per distance, scan_nd_kernel's on the widened rows).  No preparation
//   launch, no memset, no merge launch, and nothing anywhere waits for another workgroup.
//
//   Queries.  Every workgroup stages the caller's unpadded [B][dim] fp32 queries itself (vs_one_nd_queries.h), zero-padded
//   to dim_h = nd_dim_h(dim) floats per query: dim_h / 16 fragments of 1 KB, 128 KB at dim 2048.  The zero segment that
//   dim_h may add over dim_p leaves every chain unchanged (launch_scan_nd_f16 relies on the same).
//
//   Rows.  A unit of work is kOneNdhTiles 16-row tiles (64 rows), unit (n G + workgroup) 8 + wave is the wave's n-th.  A K
//   step is 32 elements = one 64-byte segment per row: ONE 16-byte load per lane and tile delivers the lane's 4 halves of
//   segment 2 s and its 4 of segment 2 s + 1 (4 KB per wave and step; dim_h is a multiple of 32, so there is no half
//   step).  The steps of ALL the wave's units form one stream, and the loads run kOneNdhDepth steps ahead of the MFMAs in
//   a register ring, across unit boundaries.  A step is 16 VGPRs per lane where scan_one_nd_kernel spends 32; the saving
//   goes into depth: 8 steps in flight, 8 waves x 8 steps x 4 KB = the same 256 KB per CU.  The row norms travel in the
//   same stream (one float per lane and step).  Past the wave's last step the ring is fed with loads of one fixed line,
//   so that every step issues the same number of loads and the compiler's wait counts stay exact.  All loads are
//   ordinary nontemporal global loads whose waits the compiler places.
#include "vs_kernels.h"
#include "vs_dev.h"
#include "vs_one_tail.h"
#include "vs_one_nd_queries.h"

namespace vs {

namespace {

constexpr int kOneNdhTiles = 4;                               // 16-row tiles per unit
constexpr int kOneNdhUnitRows = kOneNdhTiles * kTileRows;     // 64 <= kScanPadRows: a unit never reads past the spare rows
static_assert(kOneNdhUnitRows == kOneNdUnit, "the plan's unit");
static_assert(kOneNdhUnitRows <= kScanPadRows, "units are loaded unclamped");
static_assert(kOneNdhUnitRows == 64, "one row norm per lane");
constexpr int kOneNdhDepth = 8;                               // K steps in flight per wave
constexpr int kOneNdhQ = 16;                                  // query columns
constexpr int kOneNdhMaxLds = one_nd_lds_bytes(4 * nd_dim_h(kNdMaxDim), 16);  // (OneNdLds over rows of 4 dim_h bytes)
static_assert(kOneNdhMaxLds == one_nd_lds_bytes(4 * kNdMaxDim, 16), "scan_one_nd_kernel's ceiling");

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));

}  // namespace

template <int KCAP>
__global__ __launch_bounds__(kScanThreads, 1) void scan_one_nd_f16_kernel(const OneNdF16Params pn) {
    const OneParams& p = pn.o;
    constexpr int T = kOneNdhTiles;
    constexpr int D = kOneNdhDepth;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int dim = pn.dim, dim_h = pn.dim_h;
    const auto L = one_nd_lds<float>(smem, 4 * dim_h, KCAP);
    f32x4* qfrag = reinterpret_cast<f32x4*>(L.tail.region);  // [dim_h / 16][64]
    float* lds_qn = L.term;                                  // [16]
    float* lds_lmin = L.tail.lmin;
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r = lane & 15, g = lane >> 4;
    const int G = (int)gridDim.x;
    const int S = dim_h >> 5;  // K steps per unit (>= 1): two 16-float segments each

    // ---- the queries: B fragments into LDS, padded to dim_h, and their squared norms (vs_one_nd_queries.h)
    one_nd_stage_queries(p.q, p.nq_valid, dim, dim_h, qfrag, lds_qn);
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

    // ---- the wave's units, dealt and walked as in scan_one_nd_kernel: run n of the base = units [n 8 G, (n + 1) 8 G);
    // p.reverse walks the FULL runs from the last to the first, an incomplete last run stays the wave's last unit, so a
    // wave's units are valid up to n_mine and nothing after.
    const int units_total = (int)((p.n_rows + kOneNdhUnitRows - 1) / kOneNdhUnitRows);
    const int per_run = G * kScanWaves;
    const int n_full = units_total / per_run;
    const int my = (int)blockIdx.x * kScanWaves + wave;
    const int n_mine = n_full + (n_full * per_run + my < units_total ? 1 : 0);
    auto unit_of = [&](int n) { return ((p.reverse && n < n_full) ? n_full - 1 - n : n) * per_run + my; };
    const int steps_total = n_mine * S;  // (<= 2^31 / 64 units x 64 steps / 8 waves: fits)

    const unsigned voff = (unsigned)(r * dim_h + 8 * g) * 2u;  // this lane's 16 bytes inside a 16-row tile's 64-byte segment
    const unsigned tile_bytes = 32u * (unsigned)dim_h;         // 16 rows
    const char* const base_c = reinterpret_cast<const char*>(pn.base_f16);
    const int last_row = (int)p.n_rows - 1;

    // the ring: D steps of T pieces of 16 bytes (8 halves: 4 of segment 2 s, 4 of segment 2 s + 1) and one row norm per lane
    f16x8 ring[D][T];
    float ring_bn[D];
    int l_n = 0, l_s = 0;  // load cursor: unit l_n of the wave, step l_s
    auto issue = [&](f16x8 (&av)[T], float& bnv) __attribute__((always_inline)) {
        const bool have = l_n < n_mine;  // (wave-uniform) past the end: T + 1 loads of the base's first line
        const int64_t row0 = have ? (int64_t)unit_of(l_n) * kOneNdhUnitRows : 0;
        const char* sb = base_c + (have ? row0 * (int64_t)dim_h * 2 + 64 * (int64_t)l_s : 0);
        const unsigned tb = have ? tile_bytes : 0u, vo = have ? voff : 0u;
#pragma unroll
        for (int t = 0; t < T; ++t) av[t] = __builtin_nontemporal_load(reinterpret_cast<const f16x8*>(sb + (t * tb + vo)));
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
    auto compute = [&](const f16x8 (&av)[T], const float bnv) __attribute__((always_inline)) {
        if (c_s == 0) bn_cur = bnv;  // (every step of the unit carries it; the first one's is kept)
        // segment 2 s, then 2 s + 1; inside a segment scan_nd_f16_kernel's order (i, tile): four independent chains
        // between two MFMAs of one chain.  A half widens exactly (fp16 denormals are on: a subnormal half becomes the
        // normal float it names)
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const f32x4 b = qfrag[(2 * c_s + u) * 64 + lane];
            float w[T][4];
#pragma unroll
            for (int t = 0; t < T; ++t)
#pragma unroll
                for (int i = 0; i < 4; ++i) w[t][i] = (float)av[t][4 * u + i];
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int t = 0; t < T; ++t) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(w[t][i], b[i], acc[t], 0, 0, 0);
        }
        if (++c_s < S) return;
        // ---- the unit's distances
        c_s = 0;
        const int row0 = unit_of(c_n) * kOneNdhUnitRows;
        ++c_n;
        const bool ragged = row0 + kOneNdhUnitRows - 1 > last_row;  // wave-uniform
        bool touched = false;
#pragma unroll
        for (int t = 0; t < T; ++t) {
            const int rbase = row0 + 16 * t + 4 * g;
            float d[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float bnj = __shfl(bn_cur, 16 * t + 4 * g + j);
                const float l2 = fmaf(-2.0f, acc[t][j], qn + bnj);  // scan_nd_kernel's epilogue
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

    // (the ring slots are named by constants, one statement each, as in scan_one_nd_kernel: an indexed ring goes to
    // scratch memory)
    static_assert(D == 8, "the ring is walked slot by slot below");
#define VS_ONE_NDH_STEP(u)                                             \
    do {                                                               \
        if (s0 + (u) < steps_total) compute(ring[u], ring_bn[u]);      \
        issue(ring[u], ring_bn[u]);                                    \
    } while (0)
    issue(ring[0], ring_bn[0]);
    issue(ring[1], ring_bn[1]);
    issue(ring[2], ring_bn[2]);
    issue(ring[3], ring_bn[3]);
    issue(ring[4], ring_bn[4]);
    issue(ring[5], ring_bn[5]);
    issue(ring[6], ring_bn[6]);
    issue(ring[7], ring_bn[7]);
    for (int s0 = 0; s0 < steps_total; s0 += D) {
        VS_ONE_NDH_STEP(0);
        VS_ONE_NDH_STEP(1);
        VS_ONE_NDH_STEP(2);
        VS_ONE_NDH_STEP(3);
        VS_ONE_NDH_STEP(4);
        VS_ONE_NDH_STEP(5);
        VS_ONE_NDH_STEP(6);
        VS_ONE_NDH_STEP(7);
    }
#undef VS_ONE_NDH_STEP

    // (the query fragments are done with: the merges overlay them)
    one_tail<1, KCAP, one_nd_region(128, KCAP)>(p, L.tail, ld, li);  // (128: the shortest padded row, dim_h = 32 floats)
}

template <int KCAP>
static hipError_t launch_one_nd_f16_t(const OneNdF16Params& p, int grid, hipStream_t s) {
    return launch_big_lds<scan_one_nd_f16_kernel<KCAP>, kOneNdhMaxLds>(p, grid, one_nd_lds_bytes(4 * p.dim_h, KCAP), s);
}

hipError_t launch_scan_one_nd_f16(const OneNdF16Params& p, int grid, hipStream_t s) {
    if (p.o.nq_valid < 1 || p.o.nq_valid > kOneNdhQ || p.o.k1 < 1 || p.o.k1 > 16 || grid < 1 || grid > kSlotStride || p.o.n_rows < 1 ||
        p.dim < 1 || p.dim > kNdMaxDim || p.dim_h != nd_dim_h(p.dim) || p.o.n_rows > 0x7fffffff - 2 * kOneNdUnit || !p.base_f16)
        return hipErrorInvalidValue;
    return p.o.k1 <= 8 ? launch_one_nd_f16_t<8>(p, grid, s) : launch_one_nd_f16_t<16>(p, grid, s);
}

}  // namespace vs
