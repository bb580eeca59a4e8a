// vs_topk_wide.hip -- selection of the k1 <= 129 best (dist, id) per query out of a dense score block and / or candidate
// lists (topk_wide_kernel, see TopkWideParams in vs_kernels.h): the selection stage of the wide-k brute-force launcher.
#include "vs_kernels.h"
#include "vs_dev.h"
#include "vs_wide_select.h"

namespace vs {

namespace {

constexpr int kTwThreads = 1024;
constexpr int kTwCap = 2048;  // keys the final sort holds (16 KB of LDS)

// every valid entry of query q -> f(key), entries dealt over the workgroup's threads
template <class F>
__device__ __forceinline__ void tw_for_each(const TopkWideParams& p, int q, const int (&len)[2], F&& f) {
    if (p.dense) {
        const float* row = p.dense + (int64_t)q * p.dense_ld;
        const int64_t nv = (p.n_dense + 3) >> 2;
        for (int64_t v = threadIdx.x; v < nv; v += kTwThreads) {
            const f32x4 x = *reinterpret_cast<const f32x4*>(row + 4 * v);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                uint64_t key;
                if (4 * v + j < p.n_dense && tw_key(x[j], p.dense_id0 + (int32_t)(4 * v + j), key)) f(key);
            }
        }
    }
    for (int l = 0; l < p.n_list; ++l) {
        const TopkList& L = p.list[l];
        for (int e = threadIdx.x; e < len[l]; e += kTwThreads) {
            const int64_t o = (int64_t)q * L.stride_q + e;
            const int32_t id = L.i[o];
            uint64_t key;
            if (id >= 0 && tw_key(L.d[o], id + L.id_add, key)) f(key);
        }
    }
}

}  // namespace

__global__ __launch_bounds__(kTwThreads) void topk_wide_kernel(const TopkWideParams p) {
    __shared__ WideSelLds<kTwCap> sel;
    const int q = blockIdx.x, tid = threadIdx.x;
    if (p.run_if && !p.run_if[0]) return;
    if (p.zero && q == 0)
        for (int w = tid; w < p.zero_words; w += kTwThreads) p.zero[w] = 0;
    if (q >= p.nq) {
        if (tid == 0 && p.tau_out) p.tau_out[q] = -VS_INF;  // padding query: a filter pass under this bound emits nothing
        return;
    }
    const int qin = p.grp_out > 0 ? (q / p.grp_out) * p.grp_in + q % p.grp_out : q;  // (see TopkWideParams)
    int len[2] = {0, 0};
    int64_t upper = p.dense ? p.n_dense : 0;  // entries at most
    for (int l = 0; l < p.n_list; ++l) {
        int c = p.list[l].cap;
        if (p.list[l].cnt) {
            const int n = p.list[l].cnt[qin];
            if (n > c) {
                if (tid == 0 && p.overflow) p.overflow[p.grp_out > 0 ? q / p.grp_out : 0] = 1;
            } else {
                c = n > 0 ? n : 0;
            }
        }
        len[l] = c;
        upper += c;
    }
    const int M = wide_select<kTwThreads>(sel, upper, p.k1, [&](auto&& f) { tw_for_each(p, qin, len, f); });
    const uint64_t* keys = sel.keys;

    const int n_out = min(M, p.k1);
    int tie = 0;
    for (int t = tid; t < p.k1; t += kTwThreads) {
        float d = VS_INF;
        int32_t id = -1;
        if (t < n_out) {
            d = tw_dist(keys[t]);
            id = (int32_t)(uint32_t)keys[t];
            if (t + 1 < n_out && tw_dist(keys[t + 1]) == d) tie = 1;
        }
        p.out_d[(int64_t)q * p.out_ld + t] = d;
        p.out_i[(int64_t)q * p.out_ld + t] = id;
    }
    tie = __syncthreads_or(tie);
    if (tid == 0) {
        if (p.flags) p.flags[q] = tie;
        if (p.tau_out) {
            const float kth = M >= p.k1 ? tw_dist(keys[p.k1 - 1]) : VS_INF;
            p.tau_out[q] = kth < VS_INF ? next_up(kth) : VS_INF;
        }
    }
}

hipError_t launch_topk_wide(const TopkWideParams& p, int grid, hipStream_t s) {
    if (p.k1 < 1 || p.k1 > kTopkWideMax || p.nq < 0 || grid < p.nq || grid < 1 || p.n_list < 0 || p.n_list > 2 || p.grp_out < 0 ||
        (p.dense && (p.dense_ld & 3)))
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(topk_wide_kernel, dim3(grid), dim3(kTwThreads), 0, s, p);
    return hipGetLastError();
}

}  // namespace vs
