// vs_scan_nd_i8_wide.hip -- the two bulk passes of wide-k brute force (k >= 16, topw_launch) on the byte copy of a
// general index made from uint8 rows (gfx950).
//
//   scan_nd_i8_wide_kernel<NQH, MODE, IP> : scan_nd_kernel's kModeStore contract (the distances of one batch to rows
//                          [row_begin, row_end) as a matrix [nq_valid][store_ld]) and its kModeFilter contract (every
//                          (row, d) with d < tau0[query] appended to the query's candidate list, counted past f_cap) on
//                          rows stored as int8 (x - 128), with v_mfma_i32_16x16x64_i8.  A quarter of scan_nd_kernel's
//                          row bytes and, under the exactness rule of vs_scan_nd_i8.hip, the same distance bits, so that
//                          the selections around the passes see what they would see behind the fp32 passes.
//
// The batch is batch wide_batch of the scratch nd_prep_i8_kernel prepared (fragments, per-query term, verdict).  A
// batch whose verdict word is set is not a byte batch: the launch returns at once, and the fp32 launch the caller
// enqueued behind it with run_if on that word writes the same outputs instead.
//
// Organisation and load schedule: scan_nd_i8_kernel's.  A wave owns 64-row blocks dealt round-robin and keeps their
// kNd8Tiles x NQH int32 accumulators resident while it walks the rows in steps of 128 bytes, one step ahead, with a
// 64-byte tail step when dim_b / 64 is odd; "uniform base + 32-bit lane offset" addressing; ordinary global loads and
// stores whose waits the compiler places.  There are no lane lists, no threshold exchange and no workgroup merge, hence
// no LDS and no barrier.
#include "vs_kernels.h"
#include "vs_dev.h"

namespace vs {

template <int NQH, int MODE, bool IP>
__global__ __launch_bounds__(kScanThreads, 1) void scan_nd_i8_wide_kernel(const ScanNdI8Params pn) {
    static_assert(MODE == kModeStore || MODE == kModeFilter, "the two bulk passes of topw_launch");
    const ScanParams& p = pn.s;
    constexpr int T = kNd8Tiles;
    const int batch = pn.wide_batch;
    const int bad = p.invalid[batch];  // (uniform over the launch)
    // the store pass opens every wide batch of the byte route, the one whose prefix is the whole base included: it counts
    if (MODE == kModeStore && pn.wide_cnt && blockIdx.x == 0 && threadIdx.x == 0) atomicAdd(pn.wide_cnt + (bad ? 1 : 0), 1ull);
    if (bad) return;

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r = lane & 15, g = lane >> 4;
    const int dim_b = pn.dim_b;
    const unsigned voff = (unsigned)(r * dim_b + 16 * g);  // this lane's 16 bytes inside a 16-row tile's 64-byte step
    const int S = dim_b / 64;          // 64-byte steps per row
    const int n_pairs = S >> 1;        // full 128-byte lines
    const int64_t n_rows = p.row_end - p.row_begin;
    const int64_t last_row = p.row_end - 1;
    const int blocks_total = (int)((n_rows + kNd8BlockRows - 1) / kNd8BlockRows);
    // blocks are dealt round-robin: block (n * G + workgroup) * 8 + wave -- workgroups in lock-step read consecutive rows
    const int wb0 = blockIdx.x * kScanWaves + wave;
    const int wb_step = gridDim.x * kScanWaves;

    const i32x4* qf_b = reinterpret_cast<const i32x4*>(pn.q8frag) + (int64_t)batch * S * 128;
    int qt[NQH];
    float tau[NQH];
#pragma unroll
    for (int h = 0; h < NQH; ++h) {
        qt[h] = pn.qterm[batch * kMaxBatch + h * 16 + r];
        tau[h] = MODE == kModeFilter ? p.tau0[h * 16 + r] : VS_INF;  // (the bounds of this one batch: [32])
    }

#pragma clang loop unroll(disable)
    for (int wb = wb0; wb < blocks_total; wb += wb_step) {
        const int64_t row0 = p.row_begin + (int64_t)wb * kNd8BlockRows;
        // one address register serves every load of the block
        const char* sb = reinterpret_cast<const char*>(p.base_u8) + row0 * (int64_t)dim_b;
        const unsigned tile_bytes = 16u * (unsigned)dim_b;  // 16 rows
        i32x4 acc[T][NQH];
#pragma unroll
        for (int t = 0; t < T; ++t)
#pragma unroll
            for (int h = 0; h < NQH; ++h) acc[t][h] = (i32x4){0, 0, 0, 0};
        i32x4 a[T][2], b[NQH][2];
        auto load_a = [&](int s, i32x4 (&av)[T][2]) __attribute__((always_inline)) {
#pragma unroll
            for (int t = 0; t < T; ++t) {
                av[t][0] = __builtin_nontemporal_load(reinterpret_cast<const i32x4*>(sb + (t * tile_bytes + 128u * s) + voff));
                av[t][1] = __builtin_nontemporal_load(reinterpret_cast<const i32x4*>(sb + (t * tile_bytes + 128u * s + 64u) + voff));
            }
        };
        auto load_b = [&](int s, i32x4 (&bv)[NQH][2]) __attribute__((always_inline)) {
#pragma unroll
            for (int h = 0; h < NQH; ++h) {
                bv[h][0] = qf_b[((2 * s) * 2 + h) * 64 + lane];
                bv[h][1] = qf_b[((2 * s + 1) * 2 + h) * 64 + lane];
            }
        };
        auto mfma_half = [&](const i32x4 (&av)[T][2], const i32x4 (&bv)[NQH][2], int u) __attribute__((always_inline)) {
#pragma unroll
            for (int t = 0; t < T; ++t)
#pragma unroll
                for (int h = 0; h < NQH; ++h)
                    acc[t][h] = __builtin_amdgcn_mfma_i32_16x16x64_i8(av[t][u], bv[h][u], acc[t][h], 0, 0, 0);
        };
        if (n_pairs > 0) {
            load_a(0, a);
            load_b(0, b);
        }
        for (int s = 0; s < n_pairs; ++s) {
            i32x4 an[T][2], bn2[NQH][2];
            const bool more = s + 1 < n_pairs;
            if (more) {
                load_a(s + 1, an);
                load_b(s + 1, bn2);
            }
            mfma_half(a, b, 0);
            mfma_half(a, b, 1);
            if (more) {
#pragma unroll
                for (int t = 0; t < T; ++t) {
                    a[t][0] = an[t][0];
                    a[t][1] = an[t][1];
                }
#pragma unroll
                for (int h = 0; h < NQH; ++h) {
                    b[h][0] = bn2[h][0];
                    b[h][1] = bn2[h][1];
                }
            }
        }
        if (S & 1) {  // the last 64 bytes of a row whose dim_b is an odd number of steps
#pragma unroll
            for (int t = 0; t < T; ++t) a[t][0] = __builtin_nontemporal_load(reinterpret_cast<const i32x4*>(sb + (t * tile_bytes + 128u * n_pairs) + voff));
#pragma unroll
            for (int h = 0; h < NQH; ++h) b[h][0] = qf_b[((2 * n_pairs) * 2 + h) * 64 + lane];
            mfma_half(a, b, 0);
        }
        const bool ragged = row0 + kNd8BlockRows - 1 > last_row;  // wave-uniform
#pragma unroll
        for (int t = 0; t < T; ++t) {
            const int64_t rbase = row0 + 16 * t + 4 * g;
            int rt[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) rt[j] = IP ? pn.rsum[rbase + j] : p.rterm[rbase + j];  // (the terms have 64 spare entries)
#pragma unroll
            for (int h = 0; h < NQH; ++h) {
                const int qidx = h * 16 + r;
                f32x4 d;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    // scan_nd_i8_kernel's epilogue: the integer the fp32 chain computes exactly, -0.0 for a zero product
                    if constexpr (IP)
                        d[j] = -(float)(qt[h] + 128 * rt[j] + acc[t][h][j]);
                    else
                        d[j] = (float)(qt[h] + rt[j] - 2 * acc[t][h][j]);
                    if (ragged && rbase + j > last_row) d[j] = VS_INF;
                }
                if (MODE == kModeStore) {
                    // a lane holds 4 consecutive rows of one query: one 16-byte store (store_ld and rbase - row_begin are
                    // multiples of 4 floats), or, where the block overhangs the last row, the rows that exist one by one
                    if (qidx < p.nq_valid) {
                        float* dst = p.store + (int64_t)qidx * p.store_ld + (rbase - p.row_begin);
                        if (!ragged || rbase + 3 <= last_row) {
                            *reinterpret_cast<f32x4*>(dst) = d;
                        } else {
#pragma unroll
                            for (int j = 0; j < 4; ++j)
                                if (rbase + j <= last_row) dst[j] = d[j];
                        }
                    }
                } else {
                    // scan_nd_kernel's filter branch: everything under the query's bound, the count running on past the cap
                    const float dmin = fminf(fminf(d[0], d[1]), fminf(d[2], d[3]));
                    if (dmin < tau[h]) {
#pragma unroll
                        for (int j = 0; j < 4; ++j)
                            if (d[j] < tau[h]) {
                                const int pos = atomicAdd(p.f_cnt + qidx, 1);
                                if (pos < p.f_cap) {
                                    p.f_row[(int64_t)qidx * p.f_cap + pos] = (int)(rbase + j);
                                    p.f_d[(int64_t)qidx * p.f_cap + pos] = d[j];
                                }
                            }
                    }
                }
            }
        }
    }
}

template <int NQH, int MODE>
static hipError_t launch_wide_t(const ScanNdI8Params& p, int grid, hipStream_t s) {
    if (p.s.metric)
        hipLaunchKernelGGL((scan_nd_i8_wide_kernel<NQH, MODE, true>), dim3(grid), dim3(kScanThreads), 0, s, p);
    else
        hipLaunchKernelGGL((scan_nd_i8_wide_kernel<NQH, MODE, false>), dim3(grid), dim3(kScanThreads), 0, s, p);
    return hipGetLastError();
}

hipError_t launch_scan_nd_i8_wide(const ScanNdI8Params& p, int grid, int nqh, int mode, hipStream_t s) {
    if ((nqh != 1 && nqh != 2) || p.s.nq_valid > 16 * nqh || p.wide_batch < 0 || p.wide_batch >= p.s.n_batches || p.s.run_if ||
        p.s.row_end <= p.s.row_begin || p.s.row_end - p.s.row_begin > (int64_t)0x7fffffff - kNd8BlockRows)
        return hipErrorInvalidValue;
    if (mode == kModeStore) {
        if (!p.s.store || (reinterpret_cast<uintptr_t>(p.s.store) & 15) || p.s.store_ld < p.s.row_end - p.s.row_begin || (p.s.store_ld & 15))
            return hipErrorInvalidValue;
    } else if (mode == kModeFilter) {
        if (!p.s.tau0 || !p.s.f_cnt || !p.s.f_row || !p.s.f_d || p.s.f_cap < 1) return hipErrorInvalidValue;
    } else {
        return hipErrorInvalidValue;
    }
    if (!scan_nd_i8_params_ok(p, grid)) return hipErrorInvalidValue;
    if (!p.wide_prepared) {
        hipError_t e = launch_nd_prep_i8(p, grid, s);
        if (e != hipSuccess) return e;
    }
    if (mode == kModeStore) return nqh == 1 ? launch_wide_t<1, kModeStore>(p, grid, s) : launch_wide_t<2, kModeStore>(p, grid, s);
    return nqh == 1 ? launch_wide_t<1, kModeFilter>(p, grid, s) : launch_wide_t<2, kModeFilter>(p, grid, s);
}

}  // namespace vs
