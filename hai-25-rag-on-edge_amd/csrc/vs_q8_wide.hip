// vs_q8_wide.hip -- exact top-k for 17 <= k <= 128 over the uint8 score matrix of the UFIXED_POINT_8 runner: a counting
// select.  256 score levels over up to 2^31 rows: equal scores at the cut are the rule, so nothing is sorted and no
// candidate list is kept.  Per batch, on the materialised matrix scores [B][ld] (vs_q8.hip, both runners):
//   q8_hist_kernel     (n_chunks, B)  the 256-bin histogram of every 16384-row chunk, hist [B][n_chunks][256]
//   q8_cut_kernel      (B)            one thread per score value v: total[v] over the chunks, ge[v] = rows at or above v by
//                                     a block scan, the cut t = the largest v with ge[v] >= kk (kk = min(k, n_rows)); for
//                                     every v >= t the chunk counts become output positions IN PLACE:
//                                     hist[b][c][v] <- (ge[v] - total[v]) + sum over c' < c of the old hist[b][c'][v]
//                                     (values below t keep their counts, nobody reads them); t per query; per (query,
//                                     chunk) whether the chunk holds a row that lands below kk; (-1, 0) into slots kk .. k-1
//   q8_scatter_kernel  (n_chunks, B)  a chunk with nothing to write leaves at once; the others reload their scores, and a
//                                     row r of value v >= t goes to position hist[b][c][v] + (rows before r in the chunk
//                                     with the same value), written iff that is below kk: always for v > t, for v = t
//                                     exactly the lowest-numbered rows
// Every slot of [0, kk) is written exactly once by a plain store, whatever the score distribution: no atomics on global
// memory, no order dependence, the same bits on every run.  Bytes at or past n_rows are never counted (a padding byte is
// not a row of score 0).  Order: score descending, equal scores in ascending row number, as the k <= 16 kernels.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "vs_q8_nd.h"

namespace {

constexpr int kChunkRows = vs::kQ8ChunkRows;
constexpr int kWideK = vs::kQ8WideK;
// LDS bins of q8_hist_kernel: kCopies copies per wave, lane l adds into copy l % kCopies, so that the 64 lanes of an
// instruction that all hold one value (saturated or coarse encodings) meet on kCopies addresses, not on one; copy c starts
// 4 banks after copy c - 1, which puts those addresses on different banks
constexpr int kCopies = 8;
constexpr int kCopyStride = 256 + 4;
constexpr int kBins = 4 * kCopies * kCopyStride;

// the thread's 64 consecutive scores as 16 words (four 16-byte loads; ld is a multiple of 64, so whole pieces exist);
// bytes past the last row read as 0.  Returns the number of the thread's bytes that are rows.
__device__ __forceinline__ int load_scores(const uint8_t* __restrict__ row, int64_t n_rows, int chunk, int tid, unsigned (&w)[16]) {
    const int64_t r0 = (int64_t)chunk * kChunkRows + (int64_t)tid * 64;
    const int64_t left = n_rows - r0;
    const int nvalid = left <= 0 ? 0 : (left < 64 ? (int)left : 64);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        uint4 v = make_uint4(0, 0, 0, 0);
        if (16 * j < nvalid) v = *reinterpret_cast<const uint4*>(row + r0 + 16 * j);
        w[4 * j] = v.x, w[4 * j + 1] = v.y, w[4 * j + 2] = v.z, w[4 * j + 3] = v.w;
    }
    if (nvalid < 64) {
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const int rem = nvalid - 4 * j;
            if (rem < 4) w[j] = rem <= 0 ? 0u : (w[j] & ((1u << (8 * rem)) - 1u));
        }
    }
    return nvalid;
}

// inclusive prefix sum of v over the 256 threads in thread order; sh[0..4) receives the four wave totals
__device__ __forceinline__ unsigned block_scan_256(unsigned v, unsigned* sh) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const unsigned up = __shfl_up(v, o);
        if (lane >= o) v += up;
    }
    if (lane == 63) sh[wave] = v;
    __syncthreads();
    for (int wv = 0; wv < wave; ++wv) v += sh[wv];
    return v;
}

__global__ __launch_bounds__(256) void q8_hist_kernel(const uint8_t* __restrict__ scores, int64_t ld, int64_t n_rows, int n_chunks,
                                                      uint32_t* __restrict__ hist) {
    __shared__ unsigned bins[kBins];
    const int chunk = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
    unsigned w[16];
    const int nvalid = load_scores(scores + (size_t)b * ld, n_rows, chunk, tid, w);
    for (int i = tid; i < kBins; i += 256) bins[i] = 0;
    __syncthreads();
    unsigned* mine = bins + ((tid >> 6) * kCopies + (tid & (kCopies - 1))) * kCopyStride;
    unsigned diff = 0;
#pragma unroll
    for (int j = 1; j < 16; ++j) diff |= w[j] ^ w[0];
    if (nvalid == 64 && diff == 0 && w[0] == (w[0] & 0xffu) * 0x01010101u) {
        atomicAdd(&mine[w[0] & 0xffu], 64u);  // 64 equal scores: one addition (constant stretches of a saturated matrix)
    } else if (nvalid == 64) {
#pragma unroll
        for (int j = 0; j < 16; ++j)
#pragma unroll
            for (int i = 0; i < 4; ++i) atomicAdd(&mine[(w[j] >> (8 * i)) & 0xffu], 1u);
    } else {
#pragma unroll
        for (int j = 0; j < 16; ++j)
#pragma unroll
            for (int i = 0; i < 4; ++i)
                if (4 * j + i < nvalid) atomicAdd(&mine[(w[j] >> (8 * i)) & 0xffu], 1u);
    }
    __syncthreads();
    unsigned sum = 0;
#pragma unroll 8
    for (int c = 0; c < 4 * kCopies; ++c) sum += bins[c * kCopyStride + tid];
    hist[((size_t)b * n_chunks + chunk) * 256 + tid] = sum;
}

// The chunk counts of one value are walked in tiles of kCutTile chunks held in registers: the loads of a tile are all in
// flight together (a loop of dependent load / store pairs over 62 chunks made this kernel as slow as the histogram), and
// up to kCutTile chunks (1 M rows) the second walk reuses the registers of the first.
constexpr int kCutTile = 64;
__global__ __launch_bounds__(256) void q8_cut_kernel(uint32_t* __restrict__ hist, int64_t n_rows, int n_chunks, int k,
                                                     int32_t* __restrict__ cut, uint32_t* __restrict__ flag, int32_t* __restrict__ ids,
                                                     uint8_t* __restrict__ top) {
    __shared__ unsigned s_wave[4];
    __shared__ unsigned s_flag[kCutTile];
    __shared__ int s_t;
    const int b = blockIdx.x, tid = threadIdx.x, v = 255 - tid;  // thread order = descending value: the scan gives ge[v]
    const unsigned kk = n_rows < k ? (unsigned)n_rows : (unsigned)k;
    uint32_t* hb = hist + (size_t)b * n_chunks * 256 + v;
    unsigned h[kCutTile];
    unsigned total = 0;
    for (int c0 = 0; c0 < n_chunks; c0 += kCutTile) {
#pragma unroll
        for (int u = 0; u < kCutTile; ++u) h[u] = c0 + u < n_chunks ? hb[(size_t)(c0 + u) * 256] : 0u;
#pragma unroll
        for (int u = 0; u < kCutTile; ++u) total += h[u];
    }
    const unsigned ge = block_scan_256(total, s_wave);  // <= n_rows < 2^31
    const unsigned above = ge - total;
    if (ge >= kk && above < kk) s_t = v;  // one thread: ge[0] = n_rows >= kk >= 1 and ge falls with v
    __syncthreads();
    const int t = s_t;
    if (tid == 0) cut[b] = t;
    if ((unsigned)tid >= kk && tid < k) {  // slots past the rows
        ids[(size_t)b * k + tid] = -1;
        top[(size_t)b * k + tid] = 0;
    }
    unsigned run = above;
    for (int c0 = 0; c0 < n_chunks; c0 += kCutTile) {
        if (n_chunks > kCutTile) {  // (a single tile is still in h)
#pragma unroll
            for (int u = 0; u < kCutTile; ++u) h[u] = c0 + u < n_chunks ? hb[(size_t)(c0 + u) * 256] : 0u;
        }
        if (tid < kCutTile) s_flag[tid] = 0;
        __syncthreads();
        if (v >= t) {
#pragma unroll
            for (int u = 0; u < kCutTile; ++u)
                if (c0 + u < n_chunks) {
                    hb[(size_t)(c0 + u) * 256] = run;
                    if (h[u] && run < kk) s_flag[u] = 1;  // (several threads may store the same 1)
                    run += h[u];
                }
        }
        __syncthreads();
        if (tid < kCutTile && c0 + tid < n_chunks) flag[(size_t)b * n_chunks + c0 + tid] = s_flag[tid];
    }
}

__global__ __launch_bounds__(256) void q8_scatter_kernel(const uint8_t* __restrict__ scores, int64_t ld, int64_t n_rows, int n_chunks,
                                                         int k, int32_t id_offset, const uint32_t* __restrict__ base,
                                                         const int32_t* __restrict__ cut, const uint32_t* __restrict__ flag,
                                                         int32_t* __restrict__ ids, uint8_t* __restrict__ top) {
    __shared__ unsigned s_wave[4];
    __shared__ unsigned above_list[kWideK];  // value << 16 | row in chunk of the entries above the cut, in row order
    const int chunk = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
    if (!flag[(size_t)b * n_chunks + chunk]) return;  // the whole workgroup
    const int t = cut[b];
    const unsigned kk = n_rows < k ? (unsigned)n_rows : (unsigned)k;
    unsigned w[16];
    const int nvalid = load_scores(scores + (size_t)b * ld, n_rows, chunk, tid, w);
    const int c_ge = t > 0 ? vs::count_ge(w, t) : nvalid;  // padding bytes read as 0 and are rows of no value
    const int c_gt = t < 255 ? vs::count_ge(w, t + 1) : 0;
    const int c_eq = c_ge - c_gt;
    // one scan for both counts: entries at the cut (at most 16384) in the low half, above it (fewer than 128) in the high
    const unsigned mine = (unsigned)c_eq | ((unsigned)c_gt << 16);
    const unsigned before = block_scan_256(mine, s_wave) - mine;
    const unsigned n_gt = (s_wave[0] + s_wave[1] + s_wave[2] + s_wave[3]) >> 16;
    const uint32_t* bb = base + ((size_t)b * n_chunks + chunk) * 256;
    const int32_t id0 = (int32_t)((int64_t)chunk * kChunkRows) + id_offset;
    int32_t* oi = ids + (size_t)b * k;
    uint8_t* ot = top + (size_t)b * k;
    if (c_eq) {
        unsigned pos = bb[t] + (before & 0xffffu);
        if (pos < kk) {  // the lowest-numbered rows at the cut
#pragma unroll
            for (int j = 0; j < 16; ++j)
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    if ((int)((w[j] >> (8 * i)) & 0xffu) == t && 4 * j + i < nvalid && pos < kk) {
                        oi[pos] = id0 + tid * 64 + 4 * j + i;
                        ot[pos] = (uint8_t)t;
                        ++pos;
                    }
        }
    }
    if (c_gt) {
        unsigned g = before >> 16;
#pragma unroll
        for (int j = 0; j < 16; ++j)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const unsigned v = (w[j] >> (8 * i)) & 0xffu;
                if ((int)v > t && g < (unsigned)kWideK) above_list[g++] = (v << 16) | (unsigned)(tid * 64 + 4 * j + i);
            }
    }
    __syncthreads();
    if ((unsigned)tid < n_gt && tid < kWideK) {
        const unsigned key = above_list[tid], v = key >> 16;
        unsigned pos = bb[v];
        for (int j = 0; j < tid; ++j) pos += (above_list[j] >> 16) == v;
        if (pos < kk) {  // always: fewer than kk rows lie above the cut
            oi[pos] = id0 + (int32_t)(key & 0xffffu);
            ot[pos] = (uint8_t)v;
        }
    }
}

}  // namespace

namespace vs {

hipError_t launch_q8_hist(const uint8_t* scores, int64_t ld, int64_t n_rows, int n_chunks, int B, uint32_t* hist, hipStream_t s) {
    hipLaunchKernelGGL(q8_hist_kernel, dim3(n_chunks, B), dim3(256), 0, s, scores, ld, n_rows, n_chunks, hist);
    return hipGetLastError();
}

hipError_t launch_q8_cut(uint32_t* hist, int64_t n_rows, int n_chunks, int B, int k, int32_t* cut, uint32_t* flag, int32_t* ids,
                         uint8_t* top, hipStream_t s) {
    hipLaunchKernelGGL(q8_cut_kernel, dim3(B), dim3(256), 0, s, hist, n_rows, n_chunks, k, cut, flag, ids, top);
    return hipGetLastError();
}

hipError_t launch_q8_scatter(const uint8_t* scores, int64_t ld, int64_t n_rows, int n_chunks, int B, int k, int32_t id_offset,
                             const uint32_t* base, const int32_t* cut, const uint32_t* flag, int32_t* ids, uint8_t* top, hipStream_t s) {
    hipLaunchKernelGGL(q8_scatter_kernel, dim3(n_chunks, B), dim3(256), 0, s, scores, ld, n_rows, n_chunks, k, id_offset, base, cut, flag,
                       ids, top);
    return hipGetLastError();
}

}  // namespace vs
