// vs_topk_wide.hip -- selection of the k1 <= 129 best (dist, id) per query out of a dense score block and / or candidate
// lists (topk_wide_kernel, see TopkWideParams in vs_kernels.h): the selection stage of the wide-k brute-force launcher.
#include "vs_kernels.h"
#include "vs_dev.h"

namespace vs {

namespace {

constexpr int kTwThreads = 1024;
constexpr int kTwCap = 2048;  // keys the final sort holds (16 KB of LDS)

// (dist, id) -> 64-bit key whose unsigned order is the (dist, id) order; false for entries that never enter an output
__device__ __forceinline__ bool tw_key(float d, int32_t id, uint64_t& key) {
    if (!(d < VS_INF) || id < 0) return false;  // +inf, NaN, padding
    uint32_t u = __builtin_bit_cast(uint32_t, d);
    if (u == 0x80000000u) u = 0u;  // -0 ranks with +0, as the float comparisons of the other merges have it
    u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
    key = ((uint64_t)u << 32) | (uint32_t)id;
    return true;
}

__device__ __forceinline__ float tw_dist(uint64_t key) {
    const uint32_t u = (uint32_t)(key >> 32);
    return __builtin_bit_cast(float, (u & 0x80000000u) ? (u & 0x7fffffffu) : ~u);
}

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
    __shared__ uint64_t keys[kTwCap];
    __shared__ int hist[256];
    __shared__ int s_n, s_total, s_bin, s_below, s_at;
    const int q = blockIdx.x, tid = threadIdx.x;
    if (p.run_if && !p.run_if[0]) return;
    if (p.zero && q == 0)
        for (int w = tid; w < p.zero_words; w += kTwThreads) p.zero[w] = 0;
    if (q >= p.nq) {
        if (tid == 0 && p.tau_out) p.tau_out[q] = -VS_INF;  // padding query: a filter pass under this bound emits nothing
        return;
    }
    int len[2] = {0, 0};
    int64_t upper = p.dense ? p.n_dense : 0;  // entries at most
    for (int l = 0; l < p.n_list; ++l) {
        int c = p.list[l].cap;
        if (p.list[l].cnt) {
            const int n = p.list[l].cnt[q];
            if (n > c) {
                if (tid == 0 && p.overflow) p.overflow[0] = 1;
            } else {
                c = n > 0 ? n : 0;
            }
        }
        len[l] = c;
        upper += c;
    }

    // Radix select: `prefix` = the leading 64 - shift bits of the k1-th smallest key, `below` = keys under that prefix.
    // Stops as soon as every key at or under the prefix fits in LDS.
    bool all = upper <= kTwCap;  // nothing to select: collect every entry
    uint64_t prefix = 0;
    int shift = 64, kr = p.k1, below = 0;
    while (!all) {
        shift -= 8;
        const bool first = shift == 56;
        for (int b = tid; b < 256; b += kTwThreads) hist[b] = 0;
        __syncthreads();
        const int sh = shift;
        const uint64_t pre = prefix;
        tw_for_each(p, q, len, [&](uint64_t key) {
            if (first || (key >> (sh + 8)) == pre) atomicAdd(&hist[(key >> sh) & 255], 1);
        });
        __syncthreads();
        if (tid < 64) {  // wave 0: prefix sums over the 256 bins (4 per lane), the bin that holds rank kr
            const int h0 = hist[4 * tid], h1 = hist[4 * tid + 1], h2 = hist[4 * tid + 2], h3 = hist[4 * tid + 3];
            const int s = h0 + h1 + h2 + h3;
            int inc = s;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const int t = __shfl_up(inc, o);
                if (tid >= o) inc += t;
            }
            const int total = __shfl(inc, 63);
            const int kt = first ? min(kr, total) : kr;
            const int exc = inc - s;
            if (kt > 0 && exc < kt && kt <= inc) {
                int c = exc, b = 4 * tid;
                if (c + h0 < kt) {
                    c += h0;
                    ++b;
                    if (c + h1 < kt) {
                        c += h1;
                        ++b;
                        if (c + h2 < kt) {
                            c += h2;
                            ++b;
                        }
                    }
                }
                s_bin = b;
                s_below = c;
                s_at = hist[b];
            }
            if (tid == 0) s_total = total;
        }
        __syncthreads();
        if (first) {
            const int total = s_total;
            if (total <= kTwCap) {  // (also total == 0: no valid entry at all)
                all = true;
                break;
            }
            kr = min(kr, total);
        }
        prefix = (prefix << 8) | (uint64_t)s_bin;
        below += s_below;
        kr -= s_below;
        if (below + s_at <= kTwCap) break;  // (keys are unique: at shift 0 s_at == 1 and below < k1)
        __syncthreads();  // hist / s_* are rewritten by the next pass
    }

    // compaction of the keys at or under the prefix (all of them when `all`), then a bitonic sort in LDS
    if (tid == 0) s_n = 0;
    __syncthreads();
    {
        const int sh = shift;
        const uint64_t pre = prefix;
        const bool take_all = all;
        tw_for_each(p, q, len, [&](uint64_t key) {
            if (take_all || (key >> sh) <= pre) keys[atomicAdd(&s_n, 1)] = key;
        });
    }
    __syncthreads();
    const int M = s_n;
    int P = 2;
    while (P < M) P <<= 1;
    for (int i = M + tid; i < P; i += kTwThreads) keys[i] = ~0ull;
    __syncthreads();
    for (int k = 2; k <= P; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = tid; i < P; i += kTwThreads) {
                const int x = i ^ j;
                if (x > i) {
                    const uint64_t a = keys[i], b = keys[x];
                    if (((i & k) == 0) == (a > b)) {
                        keys[i] = b;
                        keys[x] = a;
                    }
                }
            }
            __syncthreads();
        }
    }

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
    if (p.k1 < 1 || p.k1 > kTopkWideMax || p.nq < 0 || grid < p.nq || grid < 1 || p.n_list < 0 || p.n_list > 2 ||
        (p.dense && (p.dense_ld & 3)))
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(topk_wide_kernel, dim3(grid), dim3(kTwThreads), 0, s, p);
    return hipGetLastError();
}

}  // namespace vs
