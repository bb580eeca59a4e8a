// vs_ivf_nd_wide_i8.hip -- the candidate scan of a wide-k group (17 <= k <= 128) of a general IVF index on the byte copy of
// its rows (vs_ivf_create_nd_u8; gfx950).
//
// A wide group on such an index runs its first scan on two plans, as a k <= 16 group does (vs_ivf_nd_i8.hip): a query
// that qualifies for the byte rows -- every value an integer in [0, 255] and ||q||^2 + bmax <= 2^24, ivf_nd_prep_i8's
// verdict -- has every one of its pairs scored by ivf_scan_nd_i8_kernel<16>, so every entry of its partial lists, and the
// bound tau that ivf_nd_wide_bound_kernel takes out of them, is an exact integer (or tau is +inf).  The saturated pairs
// are planned twice as well, and this file scans the byte plan:
//
//   ivf_scan_nd_cand_i8_kernel<IP> : ivf_scan_nd_i8_kernel's item loop, row and query loads and MFMAs (512-thread
//                     workgroups loop over the item table, the 8 waves take a list's 64-row blocks round-robin, four
//                     16-row tiles per wave block, 128-byte steps of two v_mfma_i32_16x16x64_i8 per tile and a 64-byte
//                     tail step when dim_b / 64 is odd; rows one step ahead and unclamped into the 64 spare rows, the B
//                     operand gathered from the byte row of the query in slot r).  No lane lists, no workgroup merge, no
//                     LDS.  The epilogue stays in integers: a row is tested as d = qterm + rterm - 2 q'.b' <= floor(tau)
//                     (squared L2) or q.b >= -tau (inner product), and only a row that passes is converted -- (float)d or
//                     -(float)(q.b), the bits the fp32 candidate scan computes for it, -0.0 for a zero product -- keyed
//                     and appended through the atomic on cnt[query], as ivf_scan_nd_cand_kernel appends.
//
// Why the integer test is the float test.  Squared L2: for a qualifying query 0 <= d <= ||q||^2 + ||b||^2 <= 2^24 (q.b >=
// 0: no value is negative), so (float)d is exact; tau is one of those floats, so d <= (int)tau is (float)d <= tau.  An
// infinite tau becomes INT_MAX and admits every row.  Inner product: 0 <= q.b <= (||q||^2 + ||b||^2) / 2 <= 2^23, exact
// as a float; tau is -(q.b) of some row (+0.0 for a zero product: tw_dist of the folded key), so q.b >= (int)(-tau) is
// -(float)(q.b) <= tau, and an infinite tau becomes INT_MIN.
//
// No int32 overflow, for any stored bytes (so also for the spare rows and for the repeated slot of a ragged item, which
// are masked afterwards by row number and slot): |q'.b'| <= 128 * 128 * 2048 = 2^25.  Squared L2: qterm, rterm <= 128^2 *
// 2048 = 2^25 each, |2 q'.b'| <= 2^26, |d| <= 2^27.  Inner product: |sum q'|, |sum b'| <= 128 * 2048 = 2^18 each, |128 (sum
// q' + sum b')| <= 2^26, 128^2 dim <= 2^25, |q.b| <= 2^27.
#include "vs_kernels.h"
#include "vs_dev.h"
#include "vs_wide_select.h"

namespace vs {

constexpr int kNdWide8Tiles = 4;                              // 16-row tiles per wave block
constexpr int kNdWide8BlockRows = kNdWide8Tiles * kTileRows;  // 64 <= kScanPadRows: a block never reads past the spare rows
static_assert(kNdWide8BlockRows <= kScanPadRows, "row blocks are loaded unclamped");
static_assert(kIvfNdSlotBlock == kTileRows, "an item is one MFMA column block");

template <bool IP>
__global__ __launch_bounds__(kScanThreads, 1) void ivf_scan_nd_cand_i8_kernel(const IvfNdWideI8Params pb) {
    constexpr int T = kNdWide8Tiles;
    const IvfNdWideParams& w = pb.w;
    const IvfNdParams& p = w.r;
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r = lane & 15, g = lane >> 4;
    const int dim_b = pb.dim_b;
    const unsigned voff = (unsigned)(r * dim_b + 16 * g);  // this lane's 16 bytes inside a 16-row tile's 64-byte step
    const unsigned tile_bytes = 16u * (unsigned)dim_b;     // 16 rows
    const int S = dim_b / 64;    // 64-byte steps per row
    const int n_pairs = S >> 1;  // full 128-byte steps
    const int n_items = p.n_items[0];

#pragma clang loop unroll(disable)
    for (int item = blockIdx.x; item < n_items; item += gridDim.x) {
        const int list = p.items[2 * item], slot0 = p.items[2 * item + 1];
        const int n_slots = min(kIvfNdSlotBlock, p.list_start[list + 1] - slot0);
        const int64_t row_lo = p.offsets[list], row_end = p.offsets[list + 1];
        const int64_t last_row = row_end - 1;
        const int blocks_total = (int)((row_end - row_lo + kNdWide8BlockRows - 1) / kNdWide8BlockRows);
        const bool live = r < n_slots;  // (a slot past the run's end repeats the first and appends nothing)
        const int sv = p.slots[slot0 + (live ? r : 0)];
        const int qi = sv >> 8;
        const float tau = w.tau[qi];
        // qt: the query's term of the integer; lim: the bound as an integer (see the file's header)
        int qt, lim;
        if constexpr (IP) {
            qt = 128 * pb.qsum[qi] + 16384 * p.dim;  // q.b = q'.b' + 128 (sum q' + sum b') + 128^2 dim
            lim = tau < VS_INF ? (int)(-tau) : INT32_MIN;
        } else {
            qt = pb.qterm[qi];
            lim = tau < VS_INF ? (int)tau : INT32_MAX;
        }
        // this lane's 16 bytes of a 64-byte step of its slot's byte query row
        const char* qb = reinterpret_cast<const char*>(pb.q8rows) + (int64_t)qi * dim_b + 16 * g;
        unsigned long long* const cand = w.cand + (int64_t)qi * kIvfNdWideCand;

#pragma clang loop unroll(disable)
        for (int wb = wave; wb < blocks_total; wb += kScanWaves) {
            const int64_t row0 = row_lo + (int64_t)wb * kNdWide8BlockRows;
            const char* sb = reinterpret_cast<const char*>(pb.vecs_u8) + row0 * (int64_t)dim_b;
            i32x4 acc[T];
#pragma unroll
            for (int t = 0; t < T; ++t) acc[t] = (i32x4){0, 0, 0, 0};
            i32x4 a[T][2], b[2];
            auto load_pair = [&](int s, i32x4 (&av)[T][2], i32x4 (&bv)[2]) __attribute__((always_inline)) {
#pragma unroll
                for (int t = 0; t < T; ++t) {
                    av[t][0] = *(reinterpret_cast<const i32x4*>(sb + (t * tile_bytes + 128u * s) + voff));
                    av[t][1] = *(reinterpret_cast<const i32x4*>(sb + (t * tile_bytes + 128u * s + 64u) + voff));
                }
                bv[0] = *reinterpret_cast<const i32x4*>(qb + 128u * s);
                bv[1] = *reinterpret_cast<const i32x4*>(qb + 128u * s + 64u);
            };
            auto mfma_half = [&](const i32x4 (&av)[T][2], const i32x4 (&bv)[2], int u) __attribute__((always_inline)) {
#pragma unroll
                for (int t = 0; t < T; ++t) acc[t] = __builtin_amdgcn_mfma_i32_16x16x64_i8(av[t][u], bv[u], acc[t], 0, 0, 0);
            };
            if (n_pairs > 0) load_pair(0, a, b);
            for (int s = 0; s < n_pairs; ++s) {
                i32x4 an[T][2], bn2[2];
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
            if (S & 1) {  // the last 64 bytes of a row whose dim_b is an odd number of steps
#pragma unroll
                for (int t = 0; t < T; ++t) a[t][0] = *(reinterpret_cast<const i32x4*>(sb + (t * tile_bytes + 128u * n_pairs) + voff));
                b[0] = *reinterpret_cast<const i32x4*>(qb + 128u * n_pairs);
                mfma_half(a, b, 0);
            }
#pragma unroll
            for (int t = 0; t < T; ++t) {
                const int64_t rbase = row0 + 16 * t + 4 * g;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    // (the row terms have 64 spare entries)
                    int v;
                    bool pass;
                    if constexpr (IP) {
                        v = qt + 128 * pb.rsum[rbase + j] + acc[t][j];
                        pass = v >= lim;
                    } else {
                        v = qt + pb.rterm[rbase + j] - 2 * acc[t][j];
                        pass = v <= lim;
                    }
                    // (rbase + j <= last_row: a row past the list's end never competes -- under IP it would score -0.0)
                    if (live && rbase + j <= last_row && pass) {
                        const float d = IP ? -(float)v : (float)v;  // (-(float)0 = -0.0)
                        uint64_t key;
                        if (nd_wide_key<IP>(d, (int32_t)(rbase + j), key)) {
                            const int pos = atomicAdd(w.cnt + qi, 1);
                            if (pos < kIvfNdWideCand) cand[pos] = key;
                        }
                    }
                }
            }
        }
    }
}

hipError_t launch_ivf_nd_wide_i8_scan(const IvfNdWideI8Params& pb, int grid, hipStream_t s) {
    const IvfNdWideParams& w = pb.w;
    const IvfNdParams& r = w.r;
    if (grid < 1 || r.dim < 1 || r.dim > kNdMaxDim || pb.dim_b != nd_dim_b(r.dim) || r.group_q < 1 || r.group_q > kIvfNdGroupQ || r.nprobe < 1 ||
        r.nprobe > kIvfMaxProbe || r.nlist < 1 || (r.metric != 0 && r.metric != 1) || r.k <= 16 || r.k > kIvfNdWideKMax || !pb.vecs_u8 ||
        !pb.rterm || !pb.q8rows || !pb.qterm || (r.metric == 1 && (!pb.rsum || !pb.qsum)) || !w.tau || !w.cnt || !w.cand || !r.pair_mask ||
        !r.route || r.route_want != 1)
        return hipErrorInvalidValue;
    if (r.metric)
        hipLaunchKernelGGL(ivf_scan_nd_cand_i8_kernel<true>, dim3(grid), dim3(kScanThreads), 0, s, pb);
    else
        hipLaunchKernelGGL(ivf_scan_nd_cand_i8_kernel<false>, dim3(grid), dim3(kScanThreads), 0, s, pb);
    return hipGetLastError();
}

}  // namespace vs
