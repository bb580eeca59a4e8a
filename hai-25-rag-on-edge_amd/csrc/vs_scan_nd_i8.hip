// vs_scan_nd_i8.hip -- the byte scan of a general-dimension index made from uint8 rows (vs_bf_create_nd_u8; gfx950).
//
//   scan_nd_i8_kernel<NQH, KCAP, IP> : scan_nd_kernel's kModeTopK contract (vs_scan_nd.hip: partial lists
//                          [batch*32+q][workgroup][kcap], threshold exchange through slots_cur, tau0, run_if, id_offset) on
//                          rows stored as int8 (x - 128), with v_mfma_i32_16x16x64_i8 (base rows = A operand).  A quarter
//                          of scan_nd_kernel's row bytes, the same distances.
//   nd_prep_i8_kernel    : per batch, the queries as bytes (x - 128) zero-padded to dim_b and to 32 queries in MFMA
//                          B-fragment order, the per-query term, and the verdict whether the batch may run on bytes.
//
// Rows are [n_rows + kScanPadRows][dim_b] with dim_b = dim rounded up to 64 bytes; padding bytes and spare rows are
// zero, so they add nothing to any dot product.
//
// Terms.  With q' = q - 128, b' = b - 128 (both in [-128, 127]) and zero padding,
//     ||q - b||^2 = sum (q' - b')^2 = qterm + rterm - 2 q'.b',   qterm = sum q'^2, rterm = sum b'^2 over the real dim.
// Both terms are <= 2048 * 128^2 = 2^25, |q'.b'| <= 2^25 and the distance is <= 2048 * 255^2 < 2^27: every int32
// intermediate fits in any order of evaluation.
//
// Exactness rule.  The fp32 path's distance fma(-2, dot, qn + bn) is the exact integer when all values are
// integers and ||q||^2 + ||b||^2 <= 2^24 (both norms, every partial sum of q.b <= (||q||^2 + ||b||^2) / 2 and the epilogue
// are then exactly representable, in any summation order).  A batch runs here only when every query value is an integer in
// [0, 255] and max over the batch of ||q||^2 + max over the base of ||b||^2 <= 2^24; the int32 distance is then that
// same integer (< 2^24, so the conversion to float is exact).  Any other batch gets invalid[batch] = 1 and is skipped:
// the merge reports flags = 2 and the host calls rerun it on the fp32 rows.
//
// Inner product (ScanParams::metric == 1, the IP instantiations; vs_bf_create_nd_u8_metric).  The rule is the same: under
// it every partial sum of q.b is at most (||q||^2 + ||b||^2) / 2 <= 2^23, so the fp32 chain is exact in any order (as in
// vs_ivf_nd_i8.hip) and equals the int32 product rebuilt from the stored bytes,
//     q.b = q'.b' + 128 (sum q' + sum b') + 128^2 dim,
// with qt_ip = 128 sum q' + 128^2 dim per query from the preparation launch (in the qterm buffer) and rsum = sum b' per
// row (launch_ivf_nd_i8_rowsum).  The scan writes -(float)(q.b): the fp32 scan's bits, -0.0 for a zero product included.
//
// Organisation: scan_nd_kernel's.  Nothing in a wave grows with dim: a wave owns a block of kNd8Tiles 16-row tiles and
// keeps their kNd8Tiles x NQH int32 accumulators resident while it walks the rows in steps of 128 bytes (one line per
// row, two 16x16x64 MFMAs per tile and query block), with a 64-byte tail step when dim_b / 64 is odd.  Rows and
// fragments are loaded one step ahead with ordinary global loads whose waits the compiler places.  The top-k step, the
// threshold exchange and the workgroup merge are the ones scan_nd_kernel uses (vs_scan_tail.h).
#include "vs_kernels.h"
#include "vs_dev.h"
#include "vs_scan_tail.h"

namespace vs {

// (kNd8Tiles and kNd8BlockRows are in vs_kernels.h: the wide-k passes, vs_scan_nd_i8_wide.hip, share them; byte_value and
// kNd8NormLimit, the exactness rule's pieces, are in vs_dev.h: the IVF byte scan shares them)

// grid = n_batches, 256 threads.  IP: the per-query term is qt_ip = 128 sum q' + 128^2 dim instead of sum q'^2 (same buffer)
template <bool IP>
__global__ __launch_bounds__(256) void nd_prep_i8_kernel(const float* __restrict__ q, int64_t q_batch_stride, int nq_valid, int dim,
                                                         int dim_b, int bmax, int8_t* __restrict__ q8frag,
                                                         int32_t* __restrict__ qterm, int32_t* __restrict__ invalid,
                                                         const int32_t* run_if) {
    if (run_if && !run_if[0]) return;
    const int batch = blockIdx.x;
    const float* qb = q + (int64_t)batch * q_batch_stride;
    const int S = dim_b / 64;
    i32x4* out = reinterpret_cast<i32x4*>(q8frag) + (int64_t)batch * S * 128;
    bool bad = false;
    // fragment (s, h, lane) = bytes Q'[16 h + (lane & 15)][64 s + 16 (lane >> 4) ..], zeros past dim and past nq_valid
    for (int e = threadIdx.x; e < S * 128; e += 256) {
        const int lane = e & 63, h = (e >> 6) & 1, s = e >> 7;
        const int qi = 16 * h + (lane & 15), k0 = 64 * s + 16 * (lane >> 4);
        i32x4 v = {0, 0, 0, 0};
        if (qi < nq_valid) {
#pragma unroll
            for (int w = 0; w < 4; ++w) {
                unsigned word = 0;
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int k = k0 + 4 * w + i;
                    if (k < dim) {
                        int xi;
                        bad |= !byte_value(qb[(int64_t)qi * dim + k], xi);
                        word |= ((unsigned)((xi - 128) & 0xff)) << (8 * i);
                    }
                }
                v[w] = (int)word;
            }
        }
        out[e] = v;
    }
    // per query (8 lanes each): qterm = sum (q - 128)^2 and ||q||^2, in integers; absent queries are zero and never
    // invalidate a batch
    const int row = threadIdx.x >> 3, j = threadIdx.x & 7;
    const bool live = row < nq_valid;
    const float* src = qb + (int64_t)(live ? row : 0) * dim;
    int t = 0, n2 = 0;
    if (live) {
        for (int i = j; i < dim; i += 8) {
            int xi;
            if (byte_value(src[i], xi)) {
                t += IP ? xi - 128 : (xi - 128) * (xi - 128);
                n2 += xi * xi;
            }
        }
    }
#pragma unroll
    for (int m = 1; m < 8; m <<= 1) {
        t += __shfl_xor(t, m);
        n2 += __shfl_xor(n2, m);
    }
    if (IP) t = 128 * t + 16384 * dim;  // (|128 sum q'| <= 2^25, 128^2 dim <= 2^25; an absent query's term is never ranked)
    if (j == 0) qterm[batch * kMaxBatch + row] = t;
    if (live && n2 > kNd8NormLimit - bmax) bad = true;  // (n2 <= 2048 * 255^2, 0 <= bmax < 2^24: no overflow)
    const int any = __syncthreads_or(bad ? 1 : 0);
    if (threadIdx.x == 0) invalid[batch] = any ? 1 : 0;  // written as 0 or 1: nobody has to clear it before
}

// IP: the inner-product instantiation -- the same loads and MFMAs; the epilogue rebuilds q.b from the shifted bytes
template <int NQH, int KCAP, bool IP>
__global__ __launch_bounds__(kScanThreads, 1) void scan_nd_i8_kernel(const ScanNdI8Params pn) {
    const ScanParams& p = pn.s;
    constexpr int T = kNd8Tiles;
    // the fragments of a step are loaded one step ahead like its rows, except in the largest instantiation (two query
    // blocks, 16-entry lists), which has no registers left for the second set: there they are loaded in their own step
    constexpr bool BAHEAD = NQH * KCAP < 32;
    __shared__ NdTailLds tail;
    if (p.run_if && !p.run_if[0]) return;

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

#pragma clang loop unroll(disable)
    for (int batch = 0; batch < p.n_batches; ++batch) {
        if (p.invalid[batch]) continue;  // (workgroup-uniform) not a byte batch: flags = 2, the caller reruns it in fp32
        const i32x4* qf_b = reinterpret_cast<const i32x4*>(pn.q8frag) + (int64_t)batch * S * 128;
        float* slots = p.slots_cur ? p.slots_cur + (int64_t)batch * 32 * kSlotStride : nullptr;
        int qt[NQH];
        float tau[NQH], tq[NQH], wmin[NQH];
#pragma unroll
        for (int h = 0; h < NQH; ++h) {
            qt[h] = pn.qterm[batch * kMaxBatch + h * 16 + r];
            tau[h] = tq[h] = VS_INF;
            wmin[h] = VS_INF;
        }
        if (p.tau0) {
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

        // one block of T tiles: distances into the lane lists
        auto do_block = [&](int wb) __attribute__((always_inline)) {
            const int64_t row0 = p.row_begin + (int64_t)wb * kNd8BlockRows;
            // "uniform base + 32-bit lane offset" addressing: one address register serves every load of the block
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
                if (BAHEAD) load_b(0, b);
            }
            for (int s = 0; s < n_pairs; ++s) {
                i32x4 an[T][2], bn2[NQH][2];
                const bool more = s + 1 < n_pairs;
                if (!BAHEAD) load_b(s, b);  // (issued before the rows of the next step: its wait leaves those in flight)
                if (more) {
                    load_a(s + 1, an);
                    if (BAHEAD) load_b(s + 1, bn2);
                }
                mfma_half(a, b, 0);
                mfma_half(a, b, 1);
                if (more) {
#pragma unroll
                    for (int t = 0; t < T; ++t) {
                        a[t][0] = an[t][0];
                        a[t][1] = an[t][1];
                    }
                    if (BAHEAD) {
#pragma unroll
                        for (int h = 0; h < NQH; ++h) {
                            b[h][0] = bn2[h][0];
                            b[h][1] = bn2[h][1];
                        }
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
                    float d[4];
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        // the integer the fp32 path computes exactly: ||q||^2 + ||b||^2 - 2 q.b, or -(q.b) with
                        // q.b = q'.b' + 128 (sum q' + sum b') + 128^2 dim (|q'.b'| <= 2^25, |128 (...)| <= 2^26, 128^2 dim <= 2^25;
                        // a zero product gives -0.0 like the fp32 scan's negation)
                        if constexpr (IP)
                            d[j] = -(float)(qt[h] + 128 * rt[j] + acc[t][h][j]);
                        else
                            d[j] = (float)(qt[h] + rt[j] - 2 * acc[t][h][j]);
                        if (ragged && rbase + j > last_row) d[j] = VS_INF;
                    }
                    nd_topk_step<KCAP>(d, rbase, p.id_offset, wmin[h], tau[h], ld[h], li[h]);
                }
            }
        };

        bool xchg = slots != nullptr;  // (workgroup-uniform)
        for (int wb = wb0; wb < blocks_total || xchg; wb += wb_step) {
        if (wb < blocks_total) do_block(wb);
        if (xchg) {
            xchg = false;
            xchg_bound<NQH>(tail, slots, p.k1, tid, wave, wmin, tq, tau);  // (after the first block: vs_scan_tail.h)
        }
        }
        wg_merge_lists<NQH, KCAP>(tail, p, batch, tid, wave, ld, li, tq);  // (ends with a barrier)
    }
}

template <int NQH, int KCAP>
static hipError_t launch_scan_nd_i8_t(const ScanNdI8Params& p, int grid, hipStream_t s) {
    if (p.s.metric)
        hipLaunchKernelGGL((scan_nd_i8_kernel<NQH, KCAP, true>), dim3(grid), dim3(kScanThreads), 0, s, p);
    else
        hipLaunchKernelGGL((scan_nd_i8_kernel<NQH, KCAP, false>), dim3(grid), dim3(kScanThreads), 0, s, p);
    return hipGetLastError();
}

bool scan_nd_i8_params_ok(const ScanNdI8Params& p, int grid) {
    if (p.dim < 1 || p.dim > kNdMaxDim || p.dim_b != nd_dim_b(p.dim) || !p.q8frag || !p.qterm || !p.s.base_u8 ||
        (p.s.metric != 0 && p.s.metric != 1) || !(p.s.metric ? p.rsum : p.s.rterm) ||
        !p.s.invalid || p.bmax < 0 || p.bmax >= kNd8NormLimit || grid < 1 || grid > kSlotStride ||
        (p.s.row_begin & 15) || p.s.n_batches < 1 || p.s.nq_valid < 1 || p.s.nq_valid > kMaxBatch)
        return false;
    return true;
}

hipError_t launch_nd_prep_i8(const ScanNdI8Params& p, int grid, hipStream_t s) {
    if (!scan_nd_i8_params_ok(p, grid)) return hipErrorInvalidValue;
    if (p.s.metric)
        hipLaunchKernelGGL(nd_prep_i8_kernel<true>, dim3(p.s.n_batches), dim3(256), 0, s, p.s.q, p.s.q_batch_stride, p.s.nq_valid, p.dim,
                           p.dim_b, p.bmax, p.q8frag, p.qterm, p.s.invalid, p.s.run_if);
    else
        hipLaunchKernelGGL(nd_prep_i8_kernel<false>, dim3(p.s.n_batches), dim3(256), 0, s, p.s.q, p.s.q_batch_stride, p.s.nq_valid, p.dim,
                           p.dim_b, p.bmax, p.q8frag, p.qterm, p.s.invalid, p.s.run_if);
    return hipGetLastError();
}

hipError_t launch_scan_nd_i8(const ScanNdI8Params& p, int grid, int kcap, int nqh, hipStream_t s) {
    hipError_t e = launch_nd_prep_i8(p, grid, s);
    if (e != hipSuccess) return e;
    if (kcap == 8) return nqh == 1 ? launch_scan_nd_i8_t<1, 8>(p, grid, s) : launch_scan_nd_i8_t<2, 8>(p, grid, s);
    if (kcap == 16) return nqh == 1 ? launch_scan_nd_i8_t<1, 16>(p, grid, s) : launch_scan_nd_i8_t<2, 16>(p, grid, s);
    return hipErrorInvalidValue;
}

}  // namespace vs
