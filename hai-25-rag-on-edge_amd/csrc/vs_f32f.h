// vs_f32f.h -- what the two prefilter sweeps of the fp32 streaming scan share (scan_f32f_kernel in vs_scan.hip: bf16 image;
// scan_f32f_i8_kernel in vs_scan_f32f_i8.hip: byte copy): the unit of the sweep, the exact recheck behind either, the
// batches' verdict, and the measured launch rules.  Device code only.
#pragma once
#include "vs_kernels.h"
#include "vs_dev.h"
#include <hip/hip_runtime.h>

namespace vs {

constexpr int kUnitRows = 64;                         // rows per ring slot: four 16-row tiles
constexpr int kUnitTiles = kUnitRows / kTileRows;
static_assert(kUnitRows <= kScanPadRows, "units are fetched unclamped: every row array of a sweep has kScanPadRows spare rows");

// L2 bound of the streaming fp32 scan's hot test fma(-2, dot, bn) < thr: d = RN(RN(qn + bn) - 2 dot) < tau implies
// RN(bn - 2 dot) < tau - qn + slack: the three roundings together move the comparison by less than 2^-24 * 8 (qn + |tau|)
// (a row under the bound has bn < 2 (qn + tau)); the slack is 16 times that.  (One function: the exact recheck of the
// prefilters must form the same bits.)
__device__ __forceinline__ float stream_l2_thr(float tau, float qn) {
    return (tau - qn) + 9.5367431640625e-7f * (qn + fabsf(tau));
}

// the exact recheck: scan_f32s_kernel's dot of (row, query), its distance and both of its tests, or a dropped entry
struct RecheckF32 {
    const float* base;
    const float* bnorm;
    const float* q;
    int64_t q_batch_stride;
    const float* qnorm;
    const float* tau0;
    int metric;
    int32_t id_offset;
    __device__ __forceinline__ int4 operator()(const int4& c) const {
        const int qg = c.x;
        const int64_t row = (int64_t)c.z - id_offset;
        const float* b = base + row * kDim;
        const float* qq = q + (int64_t)(qg / kMaxBatch) * q_batch_stride + (int64_t)(qg % kMaxBatch) * kDim;
        // the MFMA chain of scan_f32s_kernel: step (c, i) of v_mfma_f32_16x16x4_f32 adds the four products of k = 16 c +
        // 4 g + i, g = 0..3 in order, each rounded like an fmaf
        float dot = 0.f;
#pragma unroll
        for (int cc = 0; cc < 8; ++cc) {
            f32x4 bv[4], qv[4];
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                bv[g] = *reinterpret_cast<const f32x4*>(b + 16 * cc + 4 * g);
                qv[g] = *reinterpret_cast<const f32x4*>(qq + 16 * cc + 4 * g);
            }
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int g = 0; g < 4; ++g) dot = fmaf(bv[g][i], qv[g][i], dot);
        }
        const float qn = qnorm[qg], tau = tau0[qg], bn = bnorm[row];
        bool keep;
        float d;
        if (!metric) {
            d = fmaf(-2.0f, dot, qn + bn);
            keep = fmaf(-2.0f, dot, bn) < stream_l2_thr(tau, qn) && d < tau;
        } else {
            d = -dot;
            keep = dot > -tau && d < tau;
        }
        return keep ? make_int4(qg, __builtin_bit_cast(int, d), c.z, 0) : make_int4(-1, 0, 0, 0);
    }
};

// StreamParams::invalid: whether some batch of the launch group is not byte valued (kernel-uniform: every wave reads the
// same n_batches <= 32 words, which seed_qnorm_kernel wrote earlier in the stream).  The byte sweep leaves when it is
// set, the bf16 sweep enqueued behind it when it is clear: one of the two answers the whole group.
__device__ __forceinline__ bool f32f_some_batch_not_bytes(const int32_t* invalid, const int n_batches, const int lane) {
    return __ballot(lane < n_batches && invalid[lane] != 0) != 0;
}

// Steps of every eight on which the second 4-wave workgroup of a CU raises its priority, where the caller does not
// force a count (StreamParams::f32f_prio < 0), by units per workgroup: the choice measured per shard size (DESIGN 4.2b,
// profiles/r09a_sizes_ab.txt).  Four of eight pay from about 60 units per workgroup on (1 M rows: - 4 % at 32 batches,
// - 1 % at 16); at 30 units and fewer (500 K rows and below) a block of four steps is too large a part of the sweep, and
// the launch group measured 3 - 5 % longer with it.
inline int f32f_prio_default(int64_t units_per_wg) { return units_per_wg >= 48 ? 4 : 0; }

// Waves per workgroup of the prefilter sweeps where the caller does not force one (StreamParams::f32f_waves), by column
// blocks per wave: the choice measured per launch size.
inline int f32f_waves_default(int cbw) { return cbw >= 4 ? 4 : 8; }

// the byte sweep for a launch group that launch_scan_f32_stream has checked (vs_scan_f32f_i8.hip)
hipError_t launch_scan_f32f_i8(const StreamParams& p, int cbw, int grid, hipStream_t s);

}  // namespace vs
