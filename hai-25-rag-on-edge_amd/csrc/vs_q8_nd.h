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

// n_batches batches of B queries, [n_batches * B][dim] floats -> q8frag [n_batches][dim_b / 64][2][64] 16-byte fragments
// and cq [n_batches][32]
hipError_t launch_q8_quantize_nd(const float* q, int n_batches, int B, int dim, float inv_scale, int w_off, int8_t* q8frag, int32_t* cq,
                                 hipStream_t s);

// one batch: wq [n_pad][dim_b] bytes (w8 - 128, zero padding), wterm [n_pad], q8frag / cq of that batch -> out [B][ld]
hipError_t launch_q8_scores_nd(const int8_t* wq, const int32_t* wterm, const int8_t* q8frag, const int32_t* cq, int dim, int64_t n_rows,
                               int64_t n_pad, int B, float mult, uint8_t* out, int64_t ld, int num_cus, hipStream_t s);

}  // namespace vs
