// vs_wide_select.h -- the k1 smallest 64-bit (ordered distance bits) << 32 | id keys of one query, one workgroup: a radix
// select with LDS histograms (8-bit digits, most significant first) until every key at or under the selected prefix fits
// in LDS, then one compaction and a bitonic sort of those.  Shared by topk_wide_kernel (dense block / two lists) and the
// wide-k IVF ranking (sixteen candidate sub-lists, or every row of the probed lists).
#pragma once
#include "vs_dev.h"

namespace vs {

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

// LDS of one selection: CAP keys for the final sort
template <int CAP>
struct WideSelLds {
    uint64_t keys[CAP];
    int hist[256];
    int n, total, bin, below, at;
};

// The k1 smallest keys of a query, ascending, in s.keys[0 .. min(M, k1)); returns M (keys sorted, M >= min(k1, keys)).
// `each(f)` calls f(key) for this thread's share of the query's keys -- the same keys on every call (it is called once
// per radix pass and once for the compaction); `upper` bounds their count.  Keys are unique.  Ends with a barrier.
template <int THREADS, int CAP, class Each>
__device__ __forceinline__ int wide_select(WideSelLds<CAP>& s, const int64_t upper, const int k1, Each&& each) {
    const int tid = threadIdx.x;
    bool all = upper <= CAP;  // nothing to select: collect every entry
    uint64_t prefix = 0;
    int shift = 64, kr = k1, below = 0;
    while (!all) {
        shift -= 8;
        const bool first = shift == 56;
        for (int b = tid; b < 256; b += THREADS) s.hist[b] = 0;
        __syncthreads();
        const int sh = shift;
        const uint64_t pre = prefix;
        each([&](uint64_t key) {
            if (first || (key >> (sh + 8)) == pre) atomicAdd(&s.hist[(key >> sh) & 255], 1);
        });
        __syncthreads();
        if (tid < 64) {  // wave 0: prefix sums over the 256 bins (4 per lane), the bin that holds rank kr
            const int h0 = s.hist[4 * tid], h1 = s.hist[4 * tid + 1], h2 = s.hist[4 * tid + 2], h3 = s.hist[4 * tid + 3];
            const int sum = h0 + h1 + h2 + h3;
            int inc = sum;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const int t = __shfl_up(inc, o);
                if (tid >= o) inc += t;
            }
            const int total = __shfl(inc, 63);
            const int kt = first ? min(kr, total) : kr;
            const int exc = inc - sum;
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
                s.bin = b;
                s.below = c;
                s.at = s.hist[b];
            }
            if (tid == 0) s.total = total;
        }
        __syncthreads();
        if (first) {
            const int total = s.total;
            if (total <= CAP) {  // (also total == 0: no valid entry at all)
                all = true;
                break;
            }
            kr = min(kr, total);
        }
        prefix = (prefix << 8) | (uint64_t)s.bin;
        below += s.below;
        kr -= s.below;
        if (below + s.at <= CAP) break;  // (keys are unique: at shift 0 s.at == 1 and below < k1)
        __syncthreads();  // hist / bin / below / at are rewritten by the next pass
    }

    // compaction of the keys at or under the prefix (all of them when `all`), then a bitonic sort in LDS
    if (tid == 0) s.n = 0;
    __syncthreads();
    {
        const int sh = shift;
        const uint64_t pre = prefix;
        const bool take_all = all;
        each([&](uint64_t key) {
            if (take_all || (key >> sh) <= pre) s.keys[atomicAdd(&s.n, 1)] = key;
        });
    }
    __syncthreads();
    const int M = s.n;
    int P = 2;
    while (P < M) P <<= 1;
    for (int i = M + tid; i < P; i += THREADS) s.keys[i] = ~0ull;
    __syncthreads();
    for (int k = 2; k <= P; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = tid; i < P; i += THREADS) {
                const int x = i ^ j;
                if (x > i) {
                    const uint64_t a = s.keys[i], b = s.keys[x];
                    if (((i & k) == 0) == (a > b)) {
                        s.keys[i] = b;
                        s.keys[x] = a;
                    }
                }
            }
            __syncthreads();
        }
    }
    return M;
}

}  // namespace vs
