// vs_ivf_one_scan.h -- what the two scan launches of the single-call IVF search of a general index share (gfx950; DESIGN
// 4.6d, 4.6e): ivf_one_scan_kernel (vs_ivf_one_nd.hip, fp32 rows) and ivf_one_scan_u8_kernel (vs_ivf_one_nd_i8.hip, byte
// rows first, then the fp32 rows for the queries that do not qualify).  The block geometry, the dot products of one 64-row
// block of fp32 rows with the 16 staged query columns, the loop over a workgroup's fp32 units, and the position -> id map.
// Device functions only; lane = tid & 63, wave = tid >> 6, r = lane & 15 and g = lane >> 4 as in the kernels.
#pragma once
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
static_assert(kIvfOneU8UnitRows % kIvfOneBlockRows == 0, "a unit is whole blocks, counted from the list's first row");
constexpr int kIvfOneQ = 16;                                   // query columns
// (the scan's LDS is OneNdLds of vs_one_tail.h over rows of 4 dim_p bytes, in both kernels)
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

// (ivf_one_take and ivf_one_checkpoint below are the byte phase's; the same statements stand as text in
// VS_IVF_ONE_UNITS_F32 for the reason given there.  A change to one goes into the other by hand.)
// What a lane does with the four distances of rows rbase .. rbase + 3 of one tile: into its sorted list when the column is
// in the unit's mask (a column outside the mask: its bound is -inf).  Returns whether the list changed.
template <int KCAP>
__device__ __forceinline__ bool ivf_one_take(const float (&d)[4], int rbase, bool mine, float& tau, float (&ld)[KCAP], int (&li)[KCAP]) {
    const float dmin = fminf(fminf(d[0], d[1]), fminf(d[2], d[3]));
    if (dmin < (mine ? tau : -VS_INF)) {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (d[j] < tau) {
                list_insert<KCAP>(ld, li, d[j], rbase + j);
                tau = fminf(tau, ld[KCAP - 1]);
            }
        return true;
    }
    return false;
}

// After a block: the lane's best so far for the shared bound, and the bound itself at the wave's 1st, 2nd, 4th, 8th and
// 16th block (c_n counts the wave's blocks, wave-uniform).
__device__ __forceinline__ void ivf_one_checkpoint(const OneTailLds& tail, bool touched, float best, int wave, int r, int g, bool live, int k1, int& c_n,
                                                   float& tau) {
    if (touched) tail.lmin[r * 33 + 4 * wave + g] = best;  // this lane's best so far, for the shared bound
    ++c_n;
    if (c_n == 1 || c_n == 2 || c_n == 4 || c_n == 8 || c_n == 16) {  // wave-uniform checkpoints
        // the k-th smallest of the column's lane minima: k distinct rows of the column's probed lists are at
        // least that close (vs_one_tail.h); whatever the other waves have published by now, stale only loosens it
        const float sbound = one_shared_bound(tail.lmin, r, g, k1);
        if (live && sbound < VS_INF) tau = fminf(tau, next_up(sbound));
    }
}

// The workgroup's fp32 units: units FIRST, FIRST + gridDim.x, ... below n_units of the unit table, the 8 waves taking a
// unit's 64-row blocks round-robin.  Expands inside a kernel that has, under these names: p (IvfOneParams), L (OneNdLds),
// qfrag and qn (the staged fp32 queries, one_nd_stage_queries), live, dim_p, C, voff, tile_bytes, n_units, wave, lane, r, g,
// and the lane's state tau, ld, li, c_n; T = kIvfOneTiles.
//   Text and not a function on purpose: ivf_one_scan_kernel has to stay, instruction for instruction, the kernel that was
//   measured.  The compiler simplifies a function by itself before it inlines it; with the lane's state behind references
//   it settles there for branches where the kernel's own locals gave it selects (300 to 500 instructions more per
//   kernel), and with the state copied into locals of the function the kernel still came out 3 to 57 instructions apart.
#define VS_IVF_ONE_UNITS_F32(FIRST)                                                                                          \
    _Pragma("clang loop unroll(disable)")                                                                                    \
    for (int unit = (FIRST); unit < n_units; unit += gridDim.x) {                                                            \
        const i32x4 u = reinterpret_cast<const i32x4*>(p.units)[unit];                                                       \
        const int row_lo = u[0], row_end = u[1]; /* (a unit that is not its list's last ends on a block boundary) */         \
        const int last_row = row_end - 1;                                                                                    \
        const bool mine = live && ((u[2] >> r) & 1);                                                                         \
        const int blocks_total = (row_end - row_lo + kIvfOneBlockRows - 1) / kIvfOneBlockRows;                               \
        _Pragma("clang loop unroll(disable)")                                                                                \
        for (int wb = wave; wb < blocks_total; wb += kScanWaves) {                                                           \
            const int row0 = row_lo + wb * kIvfOneBlockRows;                                                                 \
            const char* sb = reinterpret_cast<const char*>(p.vecs + (int64_t)row0 * dim_p);                                  \
            f32x4 acc[T];                                                                                                    \
            ivf_one_block_dots(sb, voff, tile_bytes, C, qfrag, lane, acc);                                                   \
            const bool ragged = row0 + kIvfOneBlockRows - 1 > last_row; /* wave-uniform */                                   \
            bool touched = false;                                                                                            \
            _Pragma("unroll")                                                                                                \
            for (int t = 0; t < T; ++t) {                                                                                    \
                const int rbase = row0 + 16 * t + 4 * g;                                                                     \
                float d[4];                                                                                                  \
                _Pragma("unroll")                                                                                            \
                for (int j = 0; j < 4; ++j) {                                                                                \
                    if constexpr (IP)                                                                                        \
                        d[j] = -acc[t][j]; /* (an exactly zero product is +0 out of the chain: -0.0) */                      \
                    else                                                                                                     \
                        d[j] = fmaf(-2.0f, acc[t][j], qn + p.vnorm[rbase + j]); /* (the norms have 64 spare entries) */      \
                    if (ragged && rbase + j > last_row) d[j] = VS_INF; /* (under IP a spare row's -0.0 must never compete) */ \
                }                                                                                                            \
                const float dmin = fminf(fminf(d[0], d[1]), fminf(d[2], d[3]));                                              \
                if (dmin < (mine ? tau : -VS_INF)) { /* (a column outside the mask: its bound is -inf) */                    \
                    _Pragma("unroll")                                                                                        \
                    for (int j = 0; j < 4; ++j)                                                                              \
                        if (d[j] < tau) {                                                                                    \
                            list_insert<KCAP>(ld[0], li[0], d[j], rbase + j);                                                \
                            tau = fminf(tau, ld[0][KCAP - 1]);                                                               \
                        }                                                                                                    \
                    touched = true;                                                                                          \
                }                                                                                                            \
            }                                                                                                                \
            if (touched) L.tail.lmin[r * 33 + 4 * wave + g] = ld[0][0]; /* this lane's best so far, for the shared bound */  \
            ++c_n;                                                                                                           \
            if (c_n == 1 || c_n == 2 || c_n == 4 || c_n == 8 || c_n == 16) { /* wave-uniform checkpoints */                  \
                /* the k-th smallest of the column's lane minima: k distinct rows of the column's probed lists are at least  \
                   that close (vs_one_tail.h); whatever the other waves have published by now, stale only loosens it */      \
                const float sbound = one_shared_bound(L.tail.lmin, r, g, p.o.k1);                                            \
                if (live && sbound < VS_INF) tau = fminf(tau, next_up(sbound));                                              \
            }                                                                                                                \
        }                                                                                                                    \
    }

}  // namespace

}  // namespace vs
