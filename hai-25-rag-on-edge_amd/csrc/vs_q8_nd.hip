// vs_q8_nd.hip -- the UFIXED_POINT_8 score path (vs_q8.hip) at any vector dimension from 1 to 2048 (gfx950).
//
// Layout.  The database is int8 (w8 - 128), [n_pad][dim_b] with dim_b = dim rounded up to 64 bytes and n_pad a multiple
// of 64 rows; wterm[row] = 128 * sum(w8) over the real dim.  Padding bytes and padding rows are stored as 0 (not as
// -128), and so are the padding bytes of the quantised queries: they add nothing to the MFMA dot, and
//     sum q (w + off) = dot(q - 128, w - 128) + 128 sum(w) + [128 sum(q) - 128 * 128 * dim + off * sum(q)]
// holds with the real dim in the constant.  At dim 2048 every term is below 2^28 in magnitude (|dot| <= 2^25,
// 128 sum(w) < 2^26, the bracket between -255 * 255 * 2048 - 2^25 and 2^26), and so is every partial sum in the order
// the epilogue adds them: (dot + bracket) + 128 sum(w).
//
//   q8_quantize_queries_nd_kernel  one wave per query: the quantiser of vs_q8.hip for B real queries and zero rows
//                                  up to 32, written as the 16-byte B fragments the score kernel loads, fragment
//                                  (step s, query block h, lane) = bytes Q'[16 h + (lane & 15)][64 s + 16 (lane >> 4) ..];
//                                  the per-query bracket above goes to cq
//   q8_scores_nd_kernel<NQH>       q8_scores_kernel with a K loop.  Nothing in a wave grows with dim: a wave owns 64 rows,
//                                  keeps their 4 x NQH i32x4 accumulators resident and walks the rows in steps of 128
//                                  bytes (two 16x16x64 MFMAs per tile and query block), with a 64-byte tail step when
//                                  dim_b / 64 is odd.  Rows and query fragments are loaded one step ahead.  The
//                                  fragments come from the fragment buffer with ordinary global loads: at most 64 KB per
//                                  batch, read by every wave, so they stay in L2.  The epilogue is
//                                  q8_scores_kernel's: the same row -> MFMA-row assignment, one 16-byte store per lane
//                                  and query block.  (float)ip is the one round-to-nearest conversion of the complete
//                                  integer (v_cvt_f32_i32); above 2^24 it is no longer exact, and the oracle's is the same.
#include <algorithm>

#include "vs_q8_nd.h"

namespace vs {

namespace {

typedef int i32x4 __attribute__((ext_vector_type(4)));

// grid = n_batches * 32 (batch, row of the batch), one wave each: the lane's 16-value pieces of the query go to the
// fragment slots the score kernel's lanes load them from
__global__ __launch_bounds__(64) void q8_quantize_queries_nd_kernel(const float* __restrict__ q, int B, int dim, int dim_b, float inv_scale,
                                                                   int w_off, int8_t* __restrict__ q8frag, int32_t* __restrict__ cq) {
    const int nb = blockIdx.x >> 5, qi = blockIdx.x & 31, S = dim_b / 64;
    const float* src = q + ((size_t)nb * B + qi) * dim;  // (read only when qi < B)
    i32x4* out = reinterpret_cast<i32x4*>(q8frag) + (size_t)nb * S * 128;
    int sum = 0;
    for (int j = threadIdx.x; j < 4 * S; j += 64) {  // piece j: values 16 j .. 16 j + 15
        i32x4 v = {0, 0, 0, 0};
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            unsigned word = 0;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int k = 16 * j + 4 * w + i;
                if (k < dim) {
                    const float x = qi < B ? src[k] : 0.0f;  // rows past B: the zero padding of main.cpp:206-211
                    const unsigned u = q8_sat(__fadd_rn(__fmul_rn(x, inv_scale), 0.5f));  // two roundings (vs_q8.hip)
                    sum += (int)u;
                    word |= ((u - 128u) & 0xffu) << (8 * i);
                }
            }
            v[w] = (int)word;
        }
        out[(((j >> 2) * 2 + (qi >> 4)) * 64) + 16 * (j & 3) + (qi & 15)] = v;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o);
    if (threadIdx.x == 0) cq[nb * kQ8Batch + qi] = 128 * sum - 128 * 128 * dim + w_off * sum;  // (sum <= 255 * 2048)
}

template <int NQH>
__global__ __launch_bounds__(256) void q8_scores_nd_kernel(const int8_t* __restrict__ wq, const int32_t* __restrict__ wterm,
                                                           const int8_t* __restrict__ q8frag, const int32_t* __restrict__ cq, int dim_b,
                                                           int64_t n_rows, int64_t n_groups, int B, float mult,
                                                           uint8_t* __restrict__ out, int64_t ld, int aligned) {
    constexpr int T = 4;  // 16-row tiles of a wave's 64 rows
    const int lane = threadIdx.x & 63, g = lane >> 4, c = lane & 15;
    const int64_t wave0 = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6), waves = (int64_t)gridDim.x * 4;
    const i32x4* qf = reinterpret_cast<const i32x4*>(q8frag);
    const int S = dim_b / 64;    // 64-byte steps per row
    const int n_pairs = S >> 1;  // full 128-byte lines
    int cqv[NQH];
#pragma unroll
    for (int h = 0; h < NQH; ++h) cqv[h] = cq[16 * h + c];
    // MFMA row m of tile t <- database row 16*(m/4) + 4*t + (m%4), as in q8_scores_kernel: over the four tiles the C
    // fragments of lane group g hold the 16 consecutive rows 16g .. 16g+15
    const unsigned voff = (unsigned)((16 * (c >> 2) + (c & 3)) * dim_b + 16 * g);  // this lane's 16 bytes of tile 0's step
    const unsigned tile_bytes = 4u * (unsigned)dim_b;                             // tile t starts 4 t rows further
    for (int64_t grp = wave0; grp < n_groups; grp += waves) {
        const int64_t row0 = grp * kQ8GroupRows;
        const char* sb = reinterpret_cast<const char*>(wq) + row0 * (int64_t)dim_b;  // uniform base + 32-bit lane offset
        i32x4 acc[T][NQH];
#pragma unroll
        for (int t = 0; t < T; ++t)
#pragma unroll
            for (int h = 0; h < NQH; ++h) acc[t][h] = (i32x4){0, 0, 0, 0};
        i32x4 a[T][2], b[NQH][2];
        auto load_a = [&](int s, i32x4 (&av)[T][2]) __attribute__((always_inline)) {
#pragma unroll
            for (int t = 0; t < T; ++t) {
                av[t][0] = *reinterpret_cast<const i32x4*>(sb + (t * tile_bytes + 128u * s) + voff);
                av[t][1] = *reinterpret_cast<const i32x4*>(sb + (t * tile_bytes + 128u * s + 64u) + voff);
            }
        };
        auto load_b = [&](int s, i32x4 (&bv)[NQH][2]) __attribute__((always_inline)) {
#pragma unroll
            for (int h = 0; h < NQH; ++h) {
                bv[h][0] = qf[((2 * s) * 2 + h) * 64 + lane];
                bv[h][1] = qf[((2 * s + 1) * 2 + h) * 64 + lane];
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
            i32x4 an[T][2], bn[NQH][2];
            const bool more = s + 1 < n_pairs;
            if (more) {
                load_a(s + 1, an);
                load_b(s + 1, bn);
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
                    b[h][0] = bn[h][0];
                    b[h][1] = bn[h][1];
                }
            }
        }
        if (S & 1) {  // the last 64 bytes of a row whose dim_b is an odd number of steps
#pragma unroll
            for (int t = 0; t < T; ++t) a[t][0] = *reinterpret_cast<const i32x4*>(sb + (t * tile_bytes + 128u * n_pairs) + voff);
#pragma unroll
            for (int h = 0; h < NQH; ++h) b[h][0] = qf[((2 * n_pairs) * 2 + h) * 64 + lane];
            mfma_half(a, b, 0);
        }
        i32x4 rw[T];
#pragma unroll
        for (int t = 0; t < T; ++t) rw[t] = *reinterpret_cast<const i32x4*>(wterm + row0 + 16 * g + 4 * t);
#pragma unroll
        for (int h = 0; h < NQH; ++h) {
            i32x4 word;
#pragma unroll
            for (int t = 0; t < T; ++t) {
                unsigned w = 0;
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int ip = acc[t][h][i] + cqv[h] + rw[t][i];
                    w |= q8_sat(__fadd_rn(__fmul_rn((float)ip, mult), 0.5f)) << (8 * i);
                }
                word[t] = (int)w;
            }
            const int qi = 16 * h + c;
            const int64_t r = row0 + 16 * g;
            if (qi < B && r < n_rows) {
                uint8_t* dst = out + (size_t)qi * ld + r;
                if (aligned && r + 16 <= n_rows) {
                    *reinterpret_cast<i32x4*>(dst) = word;
                } else {
                    const int n = n_rows - r < 16 ? (int)(n_rows - r) : 16;
                    for (int j = 0; j < n; ++j) dst[j] = (uint8_t)(((unsigned)word[j >> 2] >> (8 * (j & 3))) & 0xffu);
                }
            }
        }
    }
}

}  // namespace

hipError_t launch_q8_quantize_nd(const float* q, int n_batches, int B, int dim, float inv_scale, int w_off, int8_t* q8frag, int32_t* cq,
                                 hipStream_t s) {
    if (!q || !q8frag || !cq || n_batches < 1 || B < 1 || B > kQ8Batch || dim < 1 || dim > kQ8MaxDim) return hipErrorInvalidValue;
    hipLaunchKernelGGL(q8_quantize_queries_nd_kernel, dim3(n_batches * kQ8Batch), dim3(64), 0, s, q, B, dim, q8_dim_b(dim), inv_scale, w_off, q8frag, cq);
    return hipGetLastError();
}

hipError_t launch_q8_scores_nd(const int8_t* wq, const int32_t* wterm, const int8_t* q8frag, const int32_t* cq, int dim, int64_t n_rows,
                               int64_t n_pad, int B, float mult, uint8_t* out, int64_t ld, int num_cus, hipStream_t s) {
    if (!wq || !wterm || !q8frag || !cq || !out || dim < 1 || dim > kQ8MaxDim || n_rows < 1 || n_pad < n_rows || n_pad % kQ8GroupRows ||
        B < 1 || B > kQ8Batch || ld < n_rows || num_cus < 1)
        return hipErrorInvalidValue;
    const int64_t n_groups = n_pad / kQ8GroupRows;
    // 3 workgroups = 12 waves per CU, what the registers allow; a wave strides over the groups.  (Measured against one
    // workgroup per four groups: 14 % slower at 128-d, 6 % faster at 384-d, the same at 2048-d.  Non-temporal row loads:
    // 10 to 30 % slower at every dimension -- DESIGN.md 4.9.)
    const int grid = (int)std::max<int64_t>(1, std::min<int64_t>((n_groups + 3) / 4, (int64_t)num_cus * 3));
    const int aligned = (ld % 16 == 0) && (reinterpret_cast<uintptr_t>(out) % 16 == 0);
    if (B <= 16)
        hipLaunchKernelGGL(q8_scores_nd_kernel<1>, dim3(grid), dim3(256), 0, s, wq, wterm, q8frag, cq, q8_dim_b(dim), n_rows, n_groups, B, mult,
                           out, ld, aligned);
    else
        hipLaunchKernelGGL(q8_scores_nd_kernel<2>, dim3(grid), dim3(256), 0, s, wq, wterm, q8frag, cq, q8_dim_b(dim), n_rows, n_groups, B, mult,
                           out, ld, aligned);
    return hipGetLastError();
}

}  // namespace vs
