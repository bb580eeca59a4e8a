// vs_one_nd_queries.h -- how a single-call kernel on a general index (scan_one_nd_kernel in vs_scan_one_nd.hip, the two
// kernels of vs_ivf_one_nd.hip) takes the caller's queries without a preparation launch: every workgroup reads the
// unpadded [nq_valid][dim] queries itself, writes them zero-padded in MFMA B-fragment order into LDS (dim_p / 16 segments
// of 1 KB: 128 KB at dim 2048) and works out ||q||^2 in the reference's order (nd_prep_kernel's code).  Device function
// only; every thread of a kScanThreads workgroup calls it, and the caller's next barrier publishes what it wrote.  The byte
// form below does the same for scan_one_nd_i8_kernel (vs_scan_one_nd_i8.hip): byte fragments, integer terms and the batch
// verdict of the exactness rule.
#pragma once
#include "vs_kernels.h"
#include "vs_dev.h"

namespace vs {

// qfrag [dim_p / 16][64]: fragment (c, lane) = Q[lane & 15][16 c + 4 (lane >> 4) ..], zeros past dim and past nq_valid
// (padding columns that nothing looks at); lds_qn [16]: the squared norms, 0 past nq_valid (waves 0 and 1 write them)
__device__ __forceinline__ void one_nd_stage_queries(const float* q, int nq_valid, int dim, int dim_p, f32x4* qfrag, float* lds_qn) {
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int C = dim_p / 16;
    for (int e = tid; e < C * 64; e += kScanThreads) {
        const int ql = e & 63, c = e >> 6;
        const int qi = ql & 15, k0 = 16 * c + 4 * (ql >> 4);
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (qi < nq_valid) {
#pragma unroll
            for (int i = 0; i < 4; ++i)
                if (k0 + i < dim) v[i] = q[(int64_t)qi * dim + k0 + i];
        }
        qfrag[e] = v;
    }
    // ||q||^2: 8 FMA lanes over v[8 i + j], r0 + ... + r7, then the tail (nd_prep_kernel's order); waves 0 and 1
    if (wave < 2) {
        const int row = tid >> 3, j = tid & 7;
        const bool live = row < nq_valid;
        const float* src = q + (int64_t)(live ? row : 0) * dim;
        float acc = 0.f;
        const int d8 = dim & ~7;
        for (int i = 0; i < d8; i += 8) {
            const float x = src[i + j];
            acc = fmaf(x, x, acc);
        }
        const int b8 = lane & ~7;
        float sum = __shfl(acc, b8);
#pragma unroll
        for (int u = 1; u < 8; ++u) sum = sum + __shfl(acc, b8 + u);
        for (int i = d8; i < dim; ++i) sum = fmaf(src[i], src[i], sum);
        if (j == 0) lds_qn[row] = live ? sum : 0.f;
    }
}

// The byte form (scan_one_nd_i8_kernel in vs_scan_one_nd_i8.hip): nd_prep_i8_kernel's work for one batch, done by every
// workgroup for itself.  q8frag [dim_b / 64][64]: fragment (s, lane) = bytes Q'[lane & 15][64 s + 16 (lane >> 4) ..] with
// Q' = Q - 128, zeros past dim and past nq_valid; lds_qt [16]: per query sum (q - 128)^2, or under IP 128 sum (q - 128) +
// 128^2 dim, 0 past nq_valid (waves 0 and 1 write them).  Returns the batch verdict, the same in every thread of every
// workgroup (a pure function of the queries and bmax): true when every value of every live query is an integer in
// [0, 255] and max ||q||^2 <= kNd8NormLimit - bmax.  All sums are integers: their order does not matter.  Holds a
// barrier, which also publishes what it wrote.
template <bool IP>
__device__ __forceinline__ bool one_nd_stage_queries_i8(const float* q, int nq_valid, int dim, int dim_b, int bmax, i32x4* q8frag, int* lds_qt) {
    const int tid = threadIdx.x;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int S = dim_b / 64;
    bool bad = false;
    for (int e = tid; e < S * 64; e += kScanThreads) {
        const int ql = e & 63, s = e >> 6;
        const int qi = ql & 15, k0 = 64 * s + 16 * (ql >> 4);
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
                        bad |= !byte_value(q[(int64_t)qi * dim + k], xi);
                        word |= ((unsigned)((xi - 128) & 0xff)) << (8 * i);
                    }
                }
                v[w] = (int)word;
            }
        }
        q8frag[e] = v;
    }
    // per query (8 lanes each, waves 0 and 1): the term and ||q||^2
    if (wave < 2) {
        const int row = tid >> 3, j = tid & 7;
        const bool live = row < nq_valid;
        const float* src = q + (int64_t)(live ? row : 0) * dim;
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
        if (IP) t = 128 * t + 16384 * dim;  // (|128 sum q'| <= 2^25, 128^2 dim <= 2^25)
        if (j == 0) lds_qt[row] = live ? t : 0;
        if (live && n2 > kNd8NormLimit - bmax) bad = true;  // (n2 <= 2048 * 255^2, 0 <= bmax < 2^24: no overflow)
    }
    return __syncthreads_or(bad ? 1 : 0) == 0;
}

}  // namespace vs
