// vs_scan_nd.hip -- the brute-force scan for any vector length 1 <= dim <= 2048 (gfx950).
//
//   scan_nd_kernel<NQH, KCAP, MODE> : the general-dimension sibling of scan_kernel (vs_scan.hip): the same ScanParams
//                          contract (kModeTopK partial lists + threshold exchange, kModeStore score matrix, kModeFilter
//                          candidate lists, kModeAssign nearest centroid of every row for the index builder), the same
//                          arithmetic (v_mfma_f32_16x16x4_f32, base rows = A operand, one accumulation chain per
//                          distance in the k order of scan_kernel, fma(-2, dot, qn + bn) epilogue), so that at dim = 128
//                          it gives scan_kernel's distances to the bit.
//   nd_prep_kernel       : per batch, the queries zero-padded to dim_p and laid out in MFMA B-fragment order, and their
//                          squared norms in the reference's summation order (cpu_baseline.cpp:95-114).
//
// Rows are stored [n_rows + pad][dim_p] with dim_p = dim rounded up to 16 floats (one 64-byte segment); the padding is
// zero, so it adds exact zeros to every chain.
//
// Organisation.  Nothing in a wave grows with dim: a wave owns a block of kNdTiles 16-row tiles and keeps
// their kNdTiles x NQH accumulators resident while it walks the rows' K dimension in steps of 32 floats (one 128-byte
// line per row).  Per step a lane loads, for every tile, the two 16-byte pieces of its row (lanes g = 0..3 of a row
// cover a whole 64-byte segment) and, for every query block, the two 16-byte pieces of the prepared fragments (1 KB per
// load instruction, contiguous, L2 resident: 128 B x dim_p per batch), one step ahead of the MFMAs that use them.  All
// loads are ordinary global loads whose waits the compiler places: there is no hand-counted queue in this kernel.
#include "vs_kernels.h"
#include "vs_dev.h"
#include "vs_scan_tail.h"

namespace vs {

constexpr int kNdTiles = 4;                        // 16-row tiles per wave block
constexpr int kNdBlockRows = kNdTiles * kTileRows;  // 64 <= kScanPadRows: a block never reads past the spare rows
static_assert(kNdBlockRows <= kScanPadRows, "row blocks are loaded unclamped");

// grid = n_batches, 256 threads
__global__ __launch_bounds__(256) void nd_prep_kernel(const float* __restrict__ q, int64_t q_batch_stride, int nq_valid, int dim,
                                                      int dim_p, float* __restrict__ qfrag, float* __restrict__ qnorm,
                                                      const int32_t* run_if) {
    if (run_if && !run_if[0]) return;
    const int batch = blockIdx.x;
    const float* qb = q + (int64_t)batch * q_batch_stride;
    const int C = dim_p / 16;
    f32x4* out = reinterpret_cast<f32x4*>(qfrag) + (int64_t)batch * C * 128;
    // fragment (c, h, lane) = Q[16 h + (lane & 15)][16 c + 4 (lane >> 4) ..], zeros past dim and past nq_valid
    for (int e = threadIdx.x; e < C * 128; e += 256) {
        const int lane = e & 63, h = (e >> 6) & 1, c = e >> 7;
        const int qi = 16 * h + (lane & 15), k0 = 16 * c + 4 * (lane >> 4);
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (qi < nq_valid) {
#pragma unroll
            for (int i = 0; i < 4; ++i)
                if (k0 + i < dim) v[i] = qb[(int64_t)qi * dim + k0 + i];
        }
        out[e] = v;
    }
    // squared norms: 8 FMA lanes, r0 + ... + r7, then the tail (row_sqnorm_kernel's order)
    const int row = threadIdx.x >> 3, j = threadIdx.x & 7;
    const bool live = row < nq_valid;
    const float* src = qb + (int64_t)(live ? row : 0) * dim;
    float acc = 0.f;
    const int d8 = dim & ~7;
    for (int i = 0; i < d8; i += 8) {
        const float x = src[i + j];
        acc = fmaf(x, x, acc);
    }
    const int b8 = (threadIdx.x & 63) & ~7;
    float sum = __shfl(acc, b8);
#pragma unroll
    for (int u = 1; u < 8; ++u) sum = sum + __shfl(acc, b8 + u);
    for (int i = d8; i < dim; ++i) sum = fmaf(src[i], src[i], sum);
    if (j == 0) qnorm[batch * kMaxBatch + row] = live ? sum : 0.f;
}

template <int NQH, int KCAP, int MODE>
__global__ __launch_bounds__(kScanThreads, 1) void scan_nd_kernel(const ScanNdParams pn) {
    const ScanParams& p = pn.s;
    constexpr int T = kNdTiles;
    __shared__ NdTailLds tail;
    if (p.run_if && !p.run_if[0]) return;

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r = lane & 15, g = lane >> 4;
    const int dim_p = pn.dim_p;
    const unsigned voff = (unsigned)(r * dim_p + 4 * g) * 4u;  // this lane's 16 bytes inside a 16-row tile's segment
    const int C = dim_p / 16;          // 64-byte segments per row
    const int n_pairs = C >> 1;        // full 32-float steps
    const int64_t n_rows = p.row_end - p.row_begin;
    const int64_t last_row = p.row_end - 1;
    const int blocks_total = (int)((n_rows + kNdBlockRows - 1) / kNdBlockRows);
    // blocks are dealt round-robin: block (n * G + workgroup) * 8 + wave -- workgroups in lock-step read consecutive rows
    const int wb0 = blockIdx.x * kScanWaves + wave;
    const int wb_step = gridDim.x * kScanWaves;

#pragma clang loop unroll(disable)
    for (int batch = 0; batch < p.n_batches; ++batch) {
        const f32x4* qf_b = reinterpret_cast<const f32x4*>(pn.qfrag) + (int64_t)batch * C * 128;
        float* slots = p.slots_cur ? p.slots_cur + (int64_t)batch * 32 * kSlotStride : nullptr;
        float qn[NQH], tau[NQH], tq[NQH], wmin[NQH];
#pragma unroll
        for (int h = 0; h < NQH; ++h) {
            qn[h] = pn.qnorm[batch * kMaxBatch + h * 16 + r];
            tau[h] = tq[h] = VS_INF;
            wmin[h] = VS_INF;
        }
        if ((MODE == kModeTopK || MODE == kModeFilter) && p.tau0) {
#pragma unroll
            for (int h = 0; h < NQH; ++h) tau[h] = tq[h] = p.tau0[batch * kMaxBatch + h * 16 + r];
        }
        float ld[NQH][KCAP];
        int li[NQH][KCAP];
#pragma unroll
        for (int h = 0; h < NQH; ++h)
#pragma unroll
            for (int j = 0; j < KCAP; ++j) {
                ld[h][j] = VS_INF;
                li[h][j] = -1;
            }

        // one block of T tiles: distances, then what the mode does with them
        auto do_block = [&](int wb) __attribute__((always_inline)) {
            const int64_t row0 = p.row_begin + (int64_t)wb * kNdBlockRows;
            // "uniform base + 32-bit lane offset" addressing: one address register serves every load of the block
            const char* sb = reinterpret_cast<const char*>(p.base + row0 * (int64_t)dim_p);
            const unsigned tile_bytes = 64u * (unsigned)dim_p;  // 16 rows
            f32x4 acc[T][NQH];
#pragma unroll
            for (int t = 0; t < T; ++t)
#pragma unroll
                for (int h = 0; h < NQH; ++h) acc[t][h] = (f32x4){0.f, 0.f, 0.f, 0.f};
            f32x4 a[T][2], b[NQH][2];
            auto load_pair = [&](int s, f32x4 (&av)[T][2], f32x4 (&bv)[NQH][2]) __attribute__((always_inline)) {
#pragma unroll
                for (int t = 0; t < T; ++t) {
                    av[t][0] = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(sb + (t * tile_bytes + 128u * s) + voff));
                    av[t][1] = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(sb + (t * tile_bytes + 128u * s + 64u) + voff));
                }
#pragma unroll
                for (int h = 0; h < NQH; ++h) {
                    bv[h][0] = qf_b[((2 * s) * 2 + h) * 64 + lane];
                    bv[h][1] = qf_b[((2 * s + 1) * 2 + h) * 64 + lane];
                }
            };
            auto mfma_half = [&](const f32x4 (&av)[T][2], const f32x4 (&bv)[NQH][2], int u) __attribute__((always_inline)) {
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int t = 0; t < T; ++t)
#pragma unroll
                        for (int h = 0; h < NQH; ++h)
                            acc[t][h] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[t][u][i], bv[h][u][i], acc[t][h], 0, 0, 0);
            };
            if (n_pairs > 0) load_pair(0, a, b);
            for (int s = 0; s < n_pairs; ++s) {
                f32x4 an[T][2], bn2[NQH][2];
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
#pragma unroll
                    for (int h = 0; h < NQH; ++h) {
                        b[h][0] = bn2[h][0];
                        b[h][1] = bn2[h][1];
                    }
                }
            }
            if (C & 1) {  // the last 16 floats of a row whose dim_p is an odd number of segments
#pragma unroll
                for (int t = 0; t < T; ++t) a[t][0] = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(sb + (t * tile_bytes + 128u * n_pairs) + voff));
#pragma unroll
                for (int h = 0; h < NQH; ++h) b[h][0] = qf_b[((2 * n_pairs) * 2 + h) * 64 + lane];
                mfma_half(a, b, 0);
            }
            const bool ragged = row0 + kNdBlockRows - 1 > last_row;  // wave-uniform
#pragma unroll
            for (int t = 0; t < T; ++t) {
                const int64_t rbase = row0 + 16 * t + 4 * g;
                float bnv[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) bnv[j] = p.bnorm[rbase + j];  // (the norms have 64 spare entries)
                float d[NQH][4];
#pragma unroll
                for (int h = 0; h < NQH; ++h)
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        // cpu_baseline.cpp:241  dist = qn + bn - 2*dot  (gcc contracts to fnmadd(2, dot, qn+bn))
                        const float l2 = fmaf(-2.0f, acc[t][h][j], qn[h] + bnv[j]);
                        d[h][j] = p.metric ? -acc[t][h][j] : l2;
                        if (ragged && rbase + j > last_row) d[h][j] = VS_INF;
                    }
                if (MODE == kModeTopK) {
#pragma unroll
                    for (int h = 0; h < NQH; ++h) nd_topk_step<KCAP>(d[h], rbase, p.id_offset, wmin[h], tau[h], ld[h], li[h]);
                } else if (MODE == kModeFilter) {
                    // candidate rows for the exact replay of select_topk: everything under the query's bound
#pragma unroll
                    for (int h = 0; h < NQH; ++h) {
                        const float dmin = fminf(fminf(d[h][0], d[h][1]), fminf(d[h][2], d[h][3]));
                        if (dmin < tau[h]) {
                            const int qidx = h * 16 + r;
#pragma unroll
                            for (int j = 0; j < 4; ++j)
                                if (d[h][j] < tau[h]) {
                                    const int pos = atomicAdd(p.f_cnt + qidx, 1);
                                    if (pos < p.f_cap) {
                                        p.f_row[(int64_t)qidx * p.f_cap + pos] = (int)(rbase + j);
                                        p.f_d[(int64_t)qidx * p.f_cap + pos] = d[h][j];
                                    }
                                }
                        }
                    }
                } else if (MODE == kModeAssign) {
                    // k-means assignment (scan_kernel's assign branch): the "queries" are a block of 32 centroids, and
                    // every base row keeps its nearest centroid so far in best_d / best_i.  A lane holds rows rbase ..
                    // rbase + 3 for columns r and 16 + r: fold its columns, then the 16 lanes of the DPP row (the same
                    // rows, other columns).  No atomics: a wave owns the same row blocks in every batch (wb0 and wb_step
                    // do not depend on the batch), and the launches of one pass are ordered by their stream.
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        float bd = VS_INF;
                        int bi = 0x7fffffff;
#pragma unroll
                        for (int h = 0; h < NQH; ++h) {
                            const int cid = p.assign_base + batch * kMaxBatch + h * 16 + r;
                            if (h * 16 + r < p.nq_valid && lex_lt(d[h][j], cid, bd, bi)) {
                                bd = d[h][j];
                                bi = cid;
                            }
                        }
                        float od;
                        int oi;
                        od = dpp_mov_f<0xB1>(bd); oi = dpp_mov_i<0xB1>(bi);
                        if (lex_lt(od, oi, bd, bi)) { bd = od; bi = oi; }
                        od = dpp_mov_f<0x4E>(bd); oi = dpp_mov_i<0x4E>(bi);
                        if (lex_lt(od, oi, bd, bi)) { bd = od; bi = oi; }
                        od = dpp_mov_f<0x141>(bd); oi = dpp_mov_i<0x141>(bi);
                        if (lex_lt(od, oi, bd, bi)) { bd = od; bi = oi; }
                        od = dpp_mov_f<0x140>(bd); oi = dpp_mov_i<0x140>(bi);
                        if (lex_lt(od, oi, bd, bi)) { bd = od; bi = oi; }
                        const int64_t row = rbase + j;
                        if (r == 0 && row <= last_row && bi != 0x7fffffff) {
                            const float cur_d = p.best_d[row];
                            const int cur_i = p.best_i[row];
                            if (lex_lt(bd, bi, cur_d, cur_i < 0 ? 0x7fffffff : cur_i)) {
                                p.best_d[row] = bd;
                                p.best_i[row] = bi;
                            }
                        }
                    }
                } else {  // kModeStore
#pragma unroll
                    for (int h = 0; h < NQH; ++h) {
                        const int qidx = h * 16 + r;
                        if (qidx < p.nq_valid) {
                            float* dst = p.store + (int64_t)qidx * p.store_ld + (rbase - p.row_begin);
#pragma unroll
                            for (int j = 0; j < 4; ++j)
                                if (rbase + j <= last_row) dst[j] = d[h][j];
                        }
                    }
                }
            }
        };

        bool xchg = MODE == kModeTopK && slots != nullptr;  // (workgroup-uniform)
        for (int wb = wb0; wb < blocks_total || xchg; wb += wb_step) {
        if (wb < blocks_total) do_block(wb);
        if (xchg) {
            xchg = false;
            xchg_bound<NQH>(tail, slots, p.k1, tid, wave, wmin, tq, tau);  // (after the first block: vs_scan_tail.h)
        }
        }
        if (MODE == kModeAssign) continue;  // the next 32 centroids: nothing is shared between waves, so no barrier
        if (MODE != kModeTopK) return;
        wg_merge_lists<NQH, KCAP>(tail, p, batch, tid, wave, ld, li, tq);  // (ends with a barrier)
    }
}

template <int NQH, int KCAP, int MODE>
static hipError_t launch_scan_nd_t(const ScanNdParams& p, int grid, hipStream_t s) {
    hipLaunchKernelGGL((scan_nd_kernel<NQH, KCAP, MODE>), dim3(grid), dim3(kScanThreads), 0, s, p);
    return hipGetLastError();
}

hipError_t launch_scan_nd(const ScanNdParams& p, int grid, int kcap, int nqh, int mode, hipStream_t s) {
    if (p.dim < 1 || p.dim > kNdMaxDim || p.dim_p != nd_dim_p(p.dim) || !p.qfrag || !p.qnorm || grid < 1 || grid > kSlotStride ||
        (p.s.row_begin & 15) || p.s.n_batches < 1 || (mode == kModeAssign && (!p.s.best_d || !p.s.best_i || nqh != 2)))
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(nd_prep_kernel, dim3(p.s.n_batches), dim3(256), 0, s, p.s.q, p.s.q_batch_stride, p.s.nq_valid, p.dim, p.dim_p,
                       p.qfrag, p.qnorm, p.s.run_if);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    if (mode == kModeStore) return nqh == 1 ? launch_scan_nd_t<1, 8, kModeStore>(p, grid, s) : launch_scan_nd_t<2, 8, kModeStore>(p, grid, s);
    if (mode == kModeAssign) return launch_scan_nd_t<2, 8, kModeAssign>(p, grid, s);  // (the builder's batches are 32 centroids wide)
    if (mode == kModeFilter) return nqh == 1 ? launch_scan_nd_t<1, 8, kModeFilter>(p, grid, s) : launch_scan_nd_t<2, 8, kModeFilter>(p, grid, s);
    if (mode != kModeTopK) return hipErrorInvalidValue;
    if (kcap == 8) return nqh == 1 ? launch_scan_nd_t<1, 8, kModeTopK>(p, grid, s) : launch_scan_nd_t<2, 8, kModeTopK>(p, grid, s);
    if (kcap == 16) return nqh == 1 ? launch_scan_nd_t<1, 16, kModeTopK>(p, grid, s) : launch_scan_nd_t<2, 16, kModeTopK>(p, grid, s);
    return hipErrorInvalidValue;
}

}  // namespace vs
