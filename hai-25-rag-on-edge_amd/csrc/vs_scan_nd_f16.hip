// vs_scan_nd_f16.hip -- the brute-force scan of a general index whose rows are IEEE binary16 (vs_bf_create_nd_f16, gfx950).
//
//   scan_nd_f16_kernel<NQH, KCAP, MODE> : scan_nd_kernel's ScanParams contract (kModeTopK, kModeStore, kModeFilter) and its
//                          arithmetic -- v_mfma_f32_16x16x4_f32, base rows = A operand, one accumulation chain per distance,
//                          segment c of 16 floats, lane group g supplying floats 16 c + 4 g + i to step (c, i), the
//                          fma(-2, dot, qn + bn) / -dot epilogue -- on rows stored as halves.  A half widens to fp32
//                          exactly (v_cvt_f32_f16; the kernel runs with fp16 denormals on, the target's default, so a
//                          subnormal half becomes the normal float it names), so every chain sees the operands
//                          scan_nd_kernel sees on the widened rows and returns its bits.  The queries come prepared by
//                          nd_prep_kernel (fp32 fragments and norms); the threshold exchange and the workgroup merge are
//                          vs_scan_tail.h's.  Only the row side is new.
//   nd_f16_layout_kernel : the creator's pass over one chunk of rows in row order: the stored layout below, and the rows'
//                          squared norms from the widened values in row_sqnorm_kernel's summation order.
//
// Row layout.  Rows are stored [n_rows + pad][dim_h], dim_h = dim rounded up to 32 halves (one 64-byte
// segment per 32 elements), zero padded.  Per 32-float K step a lane (r, g) needs floats 16 c + 4 g .. + 3 of the two
// segments c = 2 s and 2 s + 1: in row-major halves two separate 8-byte pieces.  Inside every 32-half block the halves are
// therefore permuted at creation: stored position 8 g + e holds element 4 g + e of the block for e < 4 and element
// 16 + 4 g + (e - 4) for e >= 4.  One 16-byte load per lane, tile and K step then delivers both pieces (4 VGPRs where
// scan_nd_kernel spends 8), and the four lanes of a row still cover one whole 64-byte segment per load instruction.
//
// Organisation.  scan_nd_kernel's: a wave owns a block of kNdhTiles 16-row tiles, keeps their kNdhTiles x NQH
// accumulators resident and walks K in steps of 32 elements; blocks are dealt round-robin; loads are unclamped (spare
// zero rows behind the last row).  The registers the narrower rows free go into depth: a ring of three row sets, filled
// TWO K steps ahead of the MFMAs that read them (scan_nd_kernel: one), i.e. twice the K extent in flight per wave at half
// the bytes per row (3 x 16 row VGPRs where scan_nd_kernel holds 2 x 32).  The ring is unrolled by three, so no row set is
// ever copied (a copy would wait for the load it moves).  All loads are ordinary global loads whose waits the compiler places.
#include "vs_kernels.h"
#include "vs_dev.h"
#include "vs_scan_tail.h"

namespace vs {

constexpr int kNdhTiles = 4;                          // 16-row tiles per wave block
constexpr int kNdhBlockRows = kNdhTiles * kTileRows;  // 64 <= kScanPadRows: a block never reads past the spare rows
static_assert(kNdhBlockRows <= kScanPadRows, "row blocks are loaded unclamped");

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));

// 8 threads per row (row_sqnorm_kernel's geometry and summation order); grid = ceil(rows * 8 / 256)
__global__ __launch_bounds__(256) void nd_f16_layout_kernel(const _Float16* __restrict__ src, int64_t rows, int dim, int dim_h,
                                                            _Float16* __restrict__ dst, float* __restrict__ norm) {
    const int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t row = gid >> 3;
    const int j = (int)(gid & 7);
    const bool ok = row < rows;
    const _Float16* s = src + (ok ? row : 0) * (int64_t)dim;
    float acc = 0.f;
    const int d8 = dim & ~7;
    for (int i = 0; i < d8; i += 8) {
        const float x = (float)s[i + j];
        acc = fmaf(x, x, acc);
    }
    const int b = (threadIdx.x & 63) & ~7;
    float sum = __shfl(acc, b);
#pragma unroll
    for (int u = 1; u < 8; ++u) sum = sum + __shfl(acc, b + u);
    for (int i = d8; i < dim; ++i) {
        const float x = (float)s[i];
        sum = fmaf(x, x, sum);
    }
    if (!ok) return;
    if (j == 0) norm[row] = sum;
    _Float16* d = dst + row * (int64_t)dim_h;
    for (int pos = j; pos < dim_h; pos += 8) {
        const int k = (pos & ~31) + nd_f16_elem_at(pos & 31);
        d[pos] = k < dim ? s[k] : (_Float16)0.f;
    }
}

template <int NQH, int KCAP, int MODE>
__global__ __launch_bounds__(kScanThreads, 1) void scan_nd_f16_kernel(const ScanNdF16Params pn) {
    const ScanParams& p = pn.s;
    constexpr int T = kNdhTiles;
    // K steps the row loads run ahead of their MFMAs.  Two everywhere but in the widest top-k shape (two query blocks, lists
    // of 16): its lane lists hold 64 VGPRs, and the third row set would not fit the 256 of an 8-wave workgroup.
    constexpr int D = (MODE == kModeTopK && NQH == 2 && KCAP == 16) ? 1 : 2;
    __shared__ NdTailLds tail;
    if (p.run_if && !p.run_if[0]) return;

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r = lane & 15, g = lane >> 4;
    const int dim_h = pn.dim_h;
    const unsigned voff = (unsigned)(r * dim_h + 8 * g) * 2u;  // this lane's 16 bytes inside a 16-row tile's 64-byte segment
    const int n_steps = dim_h >> 5;                            // K steps of 32 elements (>= 1)
    const int64_t n_rows = p.row_end - p.row_begin;
    const int64_t last_row = p.row_end - 1;
    const int blocks_total = (int)((n_rows + kNdhBlockRows - 1) / kNdhBlockRows);
    // blocks are dealt round-robin: block (n * G + workgroup) * 8 + wave -- workgroups in lock-step read consecutive rows
    const int wb0 = blockIdx.x * kScanWaves + wave;
    const int wb_step = gridDim.x * kScanWaves;

#pragma clang loop unroll(disable)
    for (int batch = 0; batch < p.n_batches; ++batch) {
        // nd_prep_kernel's fragments with dim_p = dim_h: (c, h, lane), c < dim_h / 16
        const f32x4* qf_b = reinterpret_cast<const f32x4*>(pn.qfrag) + (int64_t)batch * (dim_h >> 4) * 128;
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
            const int64_t row0 = p.row_begin + (int64_t)wb * kNdhBlockRows;
            // "uniform base + 32-bit lane offset" addressing: one address register serves every load of the block
            const char* sb = reinterpret_cast<const char*>(p.base_f16 + row0 * (int64_t)dim_h);
            const unsigned tile_bytes = 32u * (unsigned)dim_h;  // 16 rows
            f32x4 acc[T][NQH];
#pragma unroll
            for (int t = 0; t < T; ++t)
#pragma unroll
                for (int h = 0; h < NQH; ++h) acc[t][h] = (f32x4){0.f, 0.f, 0.f, 0.f};
            // the ring: set (s % 3) holds the rows of K step s -- per tile the lane's 8 halves (both segments).  The query
            // fragments (fp32, L2 resident) stay one step ahead, as in scan_nd_kernel, and are issued BEFORE the rows two
            // steps ahead: the wait for them then leaves those row loads in flight.
            f16x8 a0[T], a1[T], a2[T];
            f32x4 b[NQH][2], bn2[NQH][2];
            auto load_a = [&](int s, f16x8 (&av)[T]) __attribute__((always_inline)) {
#pragma unroll
                for (int t = 0; t < T; ++t)
                    av[t] = __builtin_nontemporal_load(reinterpret_cast<const f16x8*>(sb + (t * tile_bytes + 64u * s) + voff));
            };
            auto load_b = [&](int s, f32x4 (&bv)[NQH][2]) __attribute__((always_inline)) {
#pragma unroll
                for (int h = 0; h < NQH; ++h) {
                    bv[h][0] = qf_b[((2 * s) * 2 + h) * 64 + lane];
                    bv[h][1] = qf_b[((2 * s + 1) * 2 + h) * 64 + lane];
                }
            };
            // K step s on set `cur`; `fill` is the set of step s + D.  AHEAD: steps s + 1 .. s + D exist, so the loads are
            // issued without a test (a conditional load makes the compiler wait for everything in flight where the paths
            // join).  Segment 2 s, then 2 s + 1; inside a segment scan_nd_kernel's order (i, tile, query block): eight
            // independent chains between two MFMAs of one chain
            auto k_step = [&](int s, const f16x8 (&cur)[T], f16x8 (&fill)[T], auto ahead) __attribute__((always_inline)) {
                constexpr bool AHEAD = decltype(ahead)::value;
                const bool more = AHEAD || s + 1 < n_steps;
                if (more) load_b(s + 1, bn2);
                if (AHEAD || s + D < n_steps) load_a(s + D, fill);
                __builtin_amdgcn_sched_barrier(0);  // the loads stay in front of this step's MFMAs, in this order
#pragma unroll
                for (int u = 0; u < 2; ++u) {
                    float w[T][4];
#pragma unroll
                    for (int t = 0; t < T; ++t)
#pragma unroll
                        for (int i = 0; i < 4; ++i) w[t][i] = (float)cur[t][4 * u + i];  // exact
#pragma unroll
                    for (int i = 0; i < 4; ++i)
#pragma unroll
                        for (int t = 0; t < T; ++t)
#pragma unroll
                            for (int h = 0; h < NQH; ++h)
                                acc[t][h] = __builtin_amdgcn_mfma_f32_16x16x4f32(w[t][i], b[h][u][i], acc[t][h], 0, 0, 0);
                }
                if (more) {
#pragma unroll
                    for (int h = 0; h < NQH; ++h) {
                        b[h][0] = bn2[h][0];
                        b[h][1] = bn2[h][1];
                    }
                }
            };
            constexpr std::true_type kAhead{};
            constexpr std::false_type kTail{};
            load_b(0, b);
            load_a(0, a0);
            if (D == 2 && n_steps > 1) load_a(1, a1);
            int s = 0;
            // (unrolled by the ring's length: no row set is ever copied; set (s + D) % 3 is filled at step s)
            if constexpr (D == 2) {
#pragma clang loop unroll(disable)
                for (; s + 4 < n_steps; s += 3) {
                    k_step(s, a0, a2, kAhead);
                    k_step(s + 1, a1, a0, kAhead);
                    k_step(s + 2, a2, a1, kAhead);
                }
                // the last 1 .. 4 steps
                k_step(s, a0, a2, kTail);
                if (s + 1 < n_steps) {
                    k_step(s + 1, a1, a0, kTail);
                    if (s + 2 < n_steps) {
                        k_step(s + 2, a2, a1, kTail);
                        if (s + 3 < n_steps) k_step(s + 3, a0, a2, kTail);
                    }
                }
            } else {
#pragma clang loop unroll(disable)
                for (; s + 3 < n_steps; s += 3) {
                    k_step(s, a0, a1, kAhead);
                    k_step(s + 1, a1, a2, kAhead);
                    k_step(s + 2, a2, a0, kAhead);
                }
                // the last 1 .. 3 steps
                k_step(s, a0, a1, kTail);
                if (s + 1 < n_steps) {
                    k_step(s + 1, a1, a2, kTail);
                    if (s + 2 < n_steps) k_step(s + 2, a2, a0, kTail);
                }
            }
            const bool ragged = row0 + kNdhBlockRows - 1 > last_row;  // wave-uniform
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
                        const float l2 = fmaf(-2.0f, acc[t][h][j], qn[h] + bnv[j]);  // scan_nd_kernel's epilogue
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
        if (MODE != kModeTopK) return;
        wg_merge_lists<NQH, KCAP>(tail, p, batch, tid, wave, ld, li, tq);  // (ends with a barrier)
    }
}

template <int NQH, int KCAP, int MODE>
static hipError_t launch_scan_nd_f16_t(const ScanNdF16Params& p, int grid, hipStream_t s) {
    hipLaunchKernelGGL((scan_nd_f16_kernel<NQH, KCAP, MODE>), dim3(grid), dim3(kScanThreads), 0, s, p);
    return hipGetLastError();
}

hipError_t launch_scan_nd_f16(const ScanNdF16Params& p, int grid, int kcap, int nqh, int mode, hipStream_t s) {
    if (p.dim < 1 || p.dim > kNdMaxDim || p.dim_h != nd_dim_h(p.dim) || !p.s.base_f16 || !p.qfrag || !p.qnorm || grid < 1 ||
        grid > kSlotStride || (p.s.row_begin & 15) || p.s.n_batches < 1 || (nqh != 1 && nqh != 2))
        return hipErrorInvalidValue;
    // the queries as for launch_scan_nd, zero padded to dim_h: a step of zeros leaves a chain unchanged
    hipError_t e = launch_nd_prep(p.s.q, p.s.q_batch_stride, p.s.nq_valid, p.dim, p.dim_h, p.qfrag, p.qnorm, p.s.run_if, p.s.n_batches, s);
    if (e != hipSuccess) return e;
    if (mode == kModeStore) return nqh == 1 ? launch_scan_nd_f16_t<1, 8, kModeStore>(p, grid, s) : launch_scan_nd_f16_t<2, 8, kModeStore>(p, grid, s);
    if (mode == kModeFilter) return nqh == 1 ? launch_scan_nd_f16_t<1, 8, kModeFilter>(p, grid, s) : launch_scan_nd_f16_t<2, 8, kModeFilter>(p, grid, s);
    if (mode != kModeTopK) return hipErrorInvalidValue;
    if (kcap == 8) return nqh == 1 ? launch_scan_nd_f16_t<1, 8, kModeTopK>(p, grid, s) : launch_scan_nd_f16_t<2, 8, kModeTopK>(p, grid, s);
    if (kcap == 16) return nqh == 1 ? launch_scan_nd_f16_t<1, 16, kModeTopK>(p, grid, s) : launch_scan_nd_f16_t<2, 16, kModeTopK>(p, grid, s);
    return hipErrorInvalidValue;
}

hipError_t launch_nd_f16_layout(const uint16_t* src, int64_t rows, int dim, uint16_t* dst, float* norm, hipStream_t s) {
    if (rows <= 0) return hipSuccess;
    if (!src || !dst || !norm || dim < 1 || dim > kNdMaxDim) return hipErrorInvalidValue;
    const int grid = (int)((rows * 8 + 255) / 256);
    hipLaunchKernelGGL(nd_f16_layout_kernel, dim3(grid), dim3(256), 0, s, reinterpret_cast<const _Float16*>(src), rows, dim,
                       nd_dim_h(dim), reinterpret_cast<_Float16*>(dst), norm);
    return hipGetLastError();
}

}  // namespace vs
