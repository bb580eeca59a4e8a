// vs_i16_quant.h -- the int16 cosine quantiser (include/vsearch.h, "int16 cosine score path"), one definition for the
// host (vs_i16_quantize, vs_host.cpp) and the device (i16_quantize_kernel, vs_i16.hip).
//
// The element-wise steps and the split rule of the pairwise sum are the functions below, compiled for both sides.  The
// host walks the tree of P(s, n) by recursion; the device kernel sums its leaves (at most 128 elements each) on different
// lanes and folds them with the same split rule, so both form the same tree: it is fixed by n alone.
// Every product, sum, quotient and root is rounded once to fp32: contraction into fused multiply-adds is switched off.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define VS_I16_HD __host__ __device__ inline
#else
#define VS_I16_HD inline
#endif

namespace vs {

constexpr int kI16MaxDim = 2048;
constexpr int kI16Leaf = 128;      // the longest run P sums without splitting (numpy's PW_BLOCKSIZE)
constexpr int kI16MaxLeaves = 32;  // a split run is longer than 128, so its halves hold at least 64: 2048 / 64 leaves

VS_I16_HD float i16_mul(float a, float b) {
#pragma clang fp contract(off)
    return a * b;
}
VS_I16_HD float i16_add(float a, float b) {
#pragma clang fp contract(off)
    return a + b;
}
// length of the left half of a run of n > 128 elements: n / 2 rounded down to a multiple of 8
VS_I16_HD int i16_split(int n) { return (n / 2) & ~7; }

// den = RN(sqrt_rn(S) + (float)1e-8)
VS_I16_HD float i16_den(float S) {
#pragma clang fp contract(off)
    return __builtin_sqrtf(S) + 1e-8f;
}
// q = (int16) trunc(RN(RN(x / den) * scale)), a NaN gives 0.  |v| <= scale (1 + 2^-22) <= 2048: the conversion fits.
VS_I16_HD int i16_quant1(float x, float den, float scale) {
#pragma clang fp contract(off)
    const float u = x / den;
    const float v = u * scale;
    return v == v ? (int)v : 0;
}

// a leaf of P: n <= 128 squares of x[0..n), numpy's eight-lane order
VS_I16_HD float i16_leaf(const float* x, int n) {
    if (n < 8) {
        float res = 0.f;
        for (int i = 0; i < n; ++i) res = i16_add(res, i16_mul(x[i], x[i]));
        return res;
    }
    float r[8];
    for (int j = 0; j < 8; ++j) r[j] = i16_mul(x[j], x[j]);
    int i = 8;
    for (; i + 8 <= n; i += 8)
        for (int j = 0; j < 8; ++j) r[j] = i16_add(r[j], i16_mul(x[i + j], x[i + j]));
    float res = i16_add(i16_add(i16_add(r[0], r[1]), i16_add(r[2], r[3])), i16_add(i16_add(r[4], r[5]), i16_add(r[6], r[7])));
    for (; i < n; ++i) res = i16_add(res, i16_mul(x[i], x[i]));
    return res;
}

// The device image stores a quantised value as the float16 of the same integer (|q| <= 2048: exact).  Back to the integer:
VS_I16_HD int i16_from_f16_bits(uint16_t h) {
    const int e = (h >> 10) & 31;
    if (e < 15) return 0;  // (the image holds integers: anything below 1 is 0)
    const int a = (int)((0x400u | (h & 0x3ffu)) << 1) >> (26 - e);  // (1.m * 2^11) >> (11 - (e - 15))
    return (h & 0x8000u) ? -a : a;
}

}  // namespace vs
