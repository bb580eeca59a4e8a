// vs_one_nd_queries.h -- how a single-call kernel on a general index (scan_one_nd_kernel in vs_scan_one_nd.hip, the two
// kernels of vs_ivf_one_nd.hip) takes the caller's queries without a preparation launch: every workgroup reads the
// unpadded [nq_valid][dim] queries itself, writes them zero-padded in MFMA B-fragment order into LDS (dim_p / 16 segments
// of 1 KB: 128 KB at dim 2048) and works out ||q||^2 in the reference's order (nd_prep_kernel's code).  Device function
// only; every thread of a kScanThreads workgroup calls it, and the caller's next barrier publishes what it wrote.
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

}  // namespace vs
