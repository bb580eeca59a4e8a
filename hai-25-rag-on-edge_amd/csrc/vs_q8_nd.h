// vs_q8_nd.h -- the general-dimension kernels of the UFIXED_POINT_8 runner (vs_q8_nd.hip), as vs_q8.hip launches them.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace vs {

constexpr int kQ8Batch = 32;       // queries of a batch (QnnRunner::getBatchSize)
constexpr int kQ8GroupRows = 64;   // rows a wave scores at a time
constexpr int kQ8MaxDim = 2048;

// dim rounded up to whole 64-byte MFMA steps
inline int q8_dim_b(int dim) { return (dim + 63) / 64 * 64; }

// sat_u8(trunc(v)) for a value that already carries its +0.5: NaN and negatives -> 0 (QnnRunner.cpp:52-53)
__device__ __forceinline__ unsigned q8_sat(float v) {
    v = fminf(fmaxf(v, 0.0f), 255.0f);
    return (unsigned)(int)v;
}

// 128 * (number of bytes of x that are >= the byte replicated in m4), added to acc.  m7 = m4 & 0x7f7f7f7f, nm = ~m4.
__device__ __forceinline__ unsigned ge_bytes_acc(unsigned x, unsigned m4, unsigned m7, unsigned nm, unsigned acc) {
    const unsigned H = 0x80808080u;
    const unsigned t = (x | H) - m7;                    // per byte (x | 0x80) - (m & 0x7f): no borrow crosses bytes
    const unsigned ge = ((x & nm) | (~(x ^ m4) & t)) & H;  // bit 7 of a byte: x >= m (unsigned)
    return __builtin_amdgcn_udot4(ge, 0x01010101u, acc, false);
}

// bytes of the thread's 16 words that are >= mid (mid in 1..255)
__device__ __forceinline__ int count_ge(const unsigned (&w)[16], int mid) {
    const unsigned m4 = 0x01010101u * (unsigned)mid, m7 = m4 & 0x7f7f7f7fu, nm = ~m4;
    unsigned a = 0;
#pragma unroll
    for (int j = 0; j < 16; ++j) a = ge_bytes_acc(w[j], m4, m7, nm, a);
    return (int)(a >> 7);
}

// n_batches batches of B queries, [n_batches * B][dim] floats -> q8frag [n_batches][dim_b / 64][2][64] 16-byte fragments
// and cq [n_batches][32]
hipError_t launch_q8_quantize_nd(const float* q, int n_batches, int B, int dim, float inv_scale, int w_off, int8_t* q8frag, int32_t* cq,
                                 hipStream_t s);

// one batch: wq [n_pad][dim_b] bytes (w8 - 128, zero padding), wterm [n_pad], q8frag / cq of that batch -> out [B][ld]
hipError_t launch_q8_scores_nd(const int8_t* wq, const int32_t* wterm, const int8_t* q8frag, const int32_t* cq, int dim, int64_t n_rows,
                               int64_t n_pad, int B, float mult, uint8_t* out, int64_t ld, int num_cus, hipStream_t s);

// The counting select of vs_q8_wide.hip (17 <= k <= 128) on a score matrix scores [B][ld] (ld a multiple of 64, the buffer
// 16-byte aligned, only the first n_rows bytes of a row are scores), n_chunks = ceil(n_rows / kQ8ChunkRows):
//   hist  -> hist [B][n_chunks][256] counts per (query, chunk, score value)
//   cut   -> cut [B] the k-th largest value per query; hist turned in place into output positions for every value at or
//            above it; flag [B][n_chunks] chunks with something to write; (-1, 0) into the slots past the rows
//   scatter -> ids / top [B][k], every slot below min(k, n_rows) written once
constexpr int kQ8ChunkRows = 16384;  // rows per top-k chunk (256 threads x 64 bytes)
constexpr int kQ8WideK = 128;
hipError_t launch_q8_hist(const uint8_t* scores, int64_t ld, int64_t n_rows, int n_chunks, int B, uint32_t* hist, hipStream_t s);
hipError_t launch_q8_cut(uint32_t* hist, int64_t n_rows, int n_chunks, int B, int k, int32_t* cut, uint32_t* flag, int32_t* ids,
                         uint8_t* top, hipStream_t s);
hipError_t launch_q8_scatter(const uint8_t* scores, int64_t ld, int64_t n_rows, int n_chunks, int B, int k, int32_t id_offset,
                             const uint32_t* base, const int32_t* cut, const uint32_t* flag, int32_t* ids, uint8_t* top, hipStream_t s);

}  // namespace vs
