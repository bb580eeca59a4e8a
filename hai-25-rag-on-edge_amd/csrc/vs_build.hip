// vs_build.hip -- index builder kernels: compute_norms (cpu_baseline.cpp:95-125), Lloyd update and k-means++ seeding
// (create_ivf_model_reordered.py:88-118); see vs_kernels.h.
#include "vs_kernels.h"
#include "vs_dev.h"
#include <type_traits>
#include <algorithm>

namespace vs {

// ------------------------------------------------------------------------------------------------
// Row norms in the reference's order: 8 FMA lanes over v[8 i + j], then r0+r1+...+r7 left to
// right, then the scalar tail (cpu_baseline.cpp:95-114).  8 threads per row.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void row_sqnorm_kernel(const float* __restrict__ v, int64_t rows, int dim,
                                                         int64_t ld, float* __restrict__ out) {
    const int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t row = gid >> 3;
    const int j = (int)(gid & 7);
    const bool ok = row < rows;
    const float* src = v + (ok ? row : 0) * ld;
    float acc = 0.f;
    const int d8 = dim & ~7;
    for (int i = 0; i < d8; i += 8) {
        const float x = src[i + j];
        acc = fmaf(x, x, acc);
    }
    const int lane = threadIdx.x & 63;
    const int b = lane & ~7;
    float sum = __shfl(acc, b);
#pragma unroll
    for (int u = 1; u < 8; ++u) sum = sum + __shfl(acc, b + u);
    for (int i = d8; i < dim; ++i) sum = fmaf(src[i], src[i], sum);
    if (ok && j == 0) out[row] = sum;
}

hipError_t launch_row_sqnorm(const float* v, int64_t rows, int dim, float* out, hipStream_t s) {
    return launch_row_sqnorm_ld(v, rows, dim, dim, out, s);
}

hipError_t launch_row_sqnorm_ld(const float* v, int64_t rows, int dim, int64_t ld, float* out, hipStream_t s) {
    if (rows <= 0) return hipSuccess;
    const int64_t threads = rows * 8;
    const int grid = (int)((threads + 255) / 256);
    hipLaunchKernelGGL(row_sqnorm_kernel, dim3(grid), dim3(256), 0, s, v, rows, dim, ld, out);
    return hipGetLastError();
}

// Shard constants of the bf16 prefilter (FilterStats) and the rows' bf16 image for scan_f32f_kernel, in one pass over the
// rows.  A workgroup takes 32 rows through LDS (whole 512-byte rows per load instruction; rows 136 floats apart, so that
// the strided reads below spread over the banks).  The statistics keep the arithmetic they always had: 8 threads per
// row, thread j over v[8 i + j] in double (exact squares of the rounding residuals, which in float could fall below the
// normal range), a butterfly over the 8, maxima by integer atomics on the bits of non-negative doubles (their order is
// the integers' order).  The image is written from the same tile, a 16-byte chunk per thread and store: chunk 4 s + g of
// a row = bf16 of floats 32 s + 4 g .. + 3 and 32 s + 16 + 4 g .. + 3 (vs_kernels.h), rounded as the statistics assume.
__device__ __forceinline__ bool filter_scaled(float x) {
    const float a = fabsf(x);
    return a == 0.f || (a >= (float)kFiltLo && a <= (float)kFiltHi);  // (false for inf and NaN)
}
constexpr int kImgBlockRows = 32;
constexpr int kImgLd = kDim + 8;  // 8 lanes per row x 8 banks: the 8 rows of a wave's strided read meet 64 different banks
__global__ __launch_bounds__(256) void row_filter_image_kernel(const float* __restrict__ v, const float* __restrict__ bnorm, int64_t rows,
                                                               unsigned long long* __restrict__ out, uint16_t* __restrict__ img) {
    __shared__ __attribute__((aligned(16))) float tile[kImgBlockRows * kImgLd];
    const int tid = threadIdx.x;
    const int64_t row0 = (int64_t)blockIdx.x * kImgBlockRows;
#pragma unroll
    for (int m = 0; m < kImgBlockRows * (kDim / 4) / 256; ++m) {
        const int idx = tid + 256 * m, rr = idx >> 5, c4 = idx & 31;
        float4 x = make_float4(0.f, 0.f, 0.f, 0.f);
        if (row0 + rr < rows) x = *reinterpret_cast<const float4*>(v + (row0 + rr) * kDim + 4 * c4);
        *reinterpret_cast<float4*>(tile + rr * kImgLd + 4 * c4) = x;
    }
    __syncthreads();
    const int j = tid & 7;
    const bool ok = row0 + (tid >> 3) < rows;
    const float* src = tile + (tid >> 3) * kImgLd;
    double n2 = 0.0, e2 = 0.0, p2 = 0.0;
    bool bad = false;
    for (int i = 0; i < kDim; i += 8) {
        const float x = src[i + j];
        const float xp = (float)(__bf16)x;
        bad = bad || !filter_scaled(x);
        const double d = (double)x - (double)xp;
        n2 = fma((double)x, (double)x, n2);
        e2 = fma(d, d, e2);
        p2 = fma((double)xp, (double)xp, p2);
    }
#pragma unroll
    for (int u = 1; u < 8; u <<= 1) {
        n2 += __shfl_xor(n2, u);
        e2 += __shfl_xor(e2, u);
        p2 += __shfl_xor(p2, u);
    }
    const bool any_bad = __any(ok && bad);
    if (ok && j == 0) {
        atomicMax(out + 0, (unsigned long long)__double_as_longlong(n2));
        atomicMax(out + 1, (unsigned long long)__double_as_longlong(e2));
        atomicMax(out + 2, (unsigned long long)__double_as_longlong(p2));
        // the largest STORED norm (what the scans read; a non-negative float, widened exactly): filter_cnorm
        if (bnorm) atomicMax(out + 4, (unsigned long long)__double_as_longlong((double)bnorm[row0 + (tid >> 3)]));
    }
    if (any_bad && (threadIdx.x & 63) == 0) atomicMax(out + 3, 1ull);
    if (!img) return;
#pragma unroll
    for (int m = 0; m < kImgBlockRows * 16 / 256; ++m) {
        const int c = tid + 256 * m, rr = c >> 4, ch = c & 15;
        if (row0 + rr >= rows) continue;
        const float* lo = tile + rr * kImgLd + 32 * (ch >> 2) + 4 * (ch & 3);
        unsigned w[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float x0 = lo[16 * (e >> 1) + 2 * (e & 1)], x1 = lo[16 * (e >> 1) + 2 * (e & 1) + 1];
            w[e] = (unsigned)__builtin_bit_cast(uint16_t, (__bf16)x0) | ((unsigned)__builtin_bit_cast(uint16_t, (__bf16)x1) << 16);
        }
        *reinterpret_cast<uint4*>(img + (row0 + rr) * kDim + 8 * ch) = make_uint4(w[0], w[1], w[2], w[3]);
    }
}

hipError_t launch_row_filter_image(const float* v, const float* bnorm, int64_t rows, unsigned long long* out, uint16_t* img, hipStream_t s) {
    if (rows <= 0) return hipSuccess;
    const int grid = (int)((rows + kImgBlockRows - 1) / kImgBlockRows);
    hipLaunchKernelGGL(row_filter_image_kernel, dim3(grid), dim3(256), 0, s, v, bnorm, rows, out, img);
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------
// k-means update (index builder, create_ivf_model_reordered.py:96-105): cluster sums are accumulated
// in 44.20 fixed point with 64-bit integer atomics, so the result does not depend on the order in
// which rows arrive (float atomics would make the index differ from run to run).
// ------------------------------------------------------------------------------------------------
constexpr double kFix = 1048576.0;  // 2^20

__global__ __launch_bounds__(256) void kmeans_accum_kernel(const float* __restrict__ x, const int32_t* __restrict__ assign,
                                                           int64_t rows, unsigned long long* __restrict__ acc,
                                                           int32_t* __restrict__ counts) {
    // 128 threads per row, 2 rows per workgroup pass
    const int t = threadIdx.x & 127;
    for (int64_t row = (int64_t)blockIdx.x * 2 + (threadIdx.x >> 7); row < rows; row += (int64_t)gridDim.x * 2) {
        const int c = assign[row];
        if (c < 0) continue;
        const long long v = __double2ll_rn((double)x[row * kDim + t] * kFix);
        atomicAdd(acc + (int64_t)c * kDim + t, (unsigned long long)v);
        if (t == 0) atomicAdd(counts + c, 1);
    }
}

__global__ __launch_bounds__(128) void kmeans_finalize_kernel(float* __restrict__ cents, const unsigned long long* __restrict__ acc,
                                                              const int32_t* __restrict__ counts, double* __restrict__ shift) {
    const int c = blockIdx.x, t = threadIdx.x;
    const int n = counts[c];
    float delta2 = 0.f;
    if (n > 0) {
        const double mean = (double)(long long)acc[(int64_t)c * kDim + t] / kFix / (double)n;
        const float nv = (float)mean;
        const float ov = cents[c * kDim + t];
        cents[c * kDim + t] = nv;
        delta2 = (nv - ov) * (nv - ov);
    }  // an empty cluster keeps its centroid
    __shared__ float red[128];
    red[t] = delta2;
    __syncthreads();
    for (int sft = 64; sft > 0; sft >>= 1) {
        if (t < sft) red[t] += red[t + sft];
        __syncthreads();
    }
    if (t == 0) shift[c] = (double)red[0];
}

hipError_t launch_kmeans_update(const float* x, const int32_t* assign, int64_t rows, int nlist, float* cents,
                                unsigned long long* acc, int32_t* counts, double* shift, hipStream_t s) {
    hipError_t e = hipMemsetAsync(acc, 0, (size_t)nlist * kDim * sizeof(unsigned long long), s);
    if (e != hipSuccess) return e;
    e = hipMemsetAsync(counts, 0, (size_t)nlist * sizeof(int32_t), s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(kmeans_accum_kernel, dim3(4096), dim3(256), 0, s, x, assign, rows, acc, counts);
    hipLaunchKernelGGL(kmeans_finalize_kernel, dim3(nlist), dim3(128), 0, s, cents, acc, counts, shift);
    return hipGetLastError();
}

// The same update at any dimension: rows ld floats apart, accumulators and centroids [nlist][dim].  One thread per
// (row, column) element; the integer sums do not depend on how the elements are dealt out.
__global__ __launch_bounds__(256) void kmeans_accum_nd_kernel(const float* __restrict__ x, int64_t ld, int dim,
                                                              const int32_t* __restrict__ assign, int64_t rows,
                                                              unsigned long long* __restrict__ acc, int32_t* __restrict__ counts) {
    if (dim <= 256) {  // whole rows per workgroup pass: 256 / dim of them (a row is never split between passes)
        const int rpp = 256 / dim;
        const int rr = threadIdx.x / dim, t = threadIdx.x - rr * dim;
        if (rr >= rpp) return;
        for (int64_t row = (int64_t)blockIdx.x * rpp + rr; row < rows; row += (int64_t)gridDim.x * rpp) {
            const int c = assign[row];
            if (c < 0) continue;
            const long long v = __double2ll_rn((double)x[row * ld + t] * kFix);
            atomicAdd(acc + (int64_t)c * dim + t, (unsigned long long)v);
            if (t == 0) atomicAdd(counts + c, 1);
        }
        return;
    }
    for (int64_t row = blockIdx.x; row < rows; row += gridDim.x) {
        const int c = assign[row];
        if (c < 0) continue;
        for (int t = threadIdx.x; t < dim; t += 256) {
            const long long v = __double2ll_rn((double)x[row * ld + t] * kFix);
            atomicAdd(acc + (int64_t)c * dim + t, (unsigned long long)v);
        }
        if (threadIdx.x == 0) atomicAdd(counts + c, 1);
    }
}

// One workgroup per centroid.  shift[c]: thread t adds the squared shifts of columns t, t + 128, ... in that order, then
// kmeans_finalize_kernel's tree over the 128 threads (at dim 128 that is its sum).
__global__ __launch_bounds__(128) void kmeans_finalize_nd_kernel(float* __restrict__ cents, int dim,
                                                                 const unsigned long long* __restrict__ acc,
                                                                 const int32_t* __restrict__ counts, double* __restrict__ shift) {
    const int c = blockIdx.x, t = threadIdx.x;
    const int n = counts[c];
    float delta2 = 0.f;
    if (n > 0) {
        for (int col = t; col < dim; col += 128) {
            const double mean = (double)(long long)acc[(int64_t)c * dim + col] / kFix / (double)n;
            const float nv = (float)mean;
            const float ov = cents[(int64_t)c * dim + col];
            cents[(int64_t)c * dim + col] = nv;
            delta2 += (nv - ov) * (nv - ov);
        }
    }  // an empty cluster keeps its centroid
    __shared__ float red[128];
    red[t] = delta2;
    __syncthreads();
    for (int sft = 64; sft > 0; sft >>= 1) {
        if (t < sft) red[t] += red[t + sft];
        __syncthreads();
    }
    if (t == 0) shift[c] = (double)red[0];
}

hipError_t launch_kmeans_update_nd(const float* x, int64_t ld, int dim, const int32_t* assign, int64_t rows, int nlist, float* cents,
                                   unsigned long long* acc, int32_t* counts, double* shift, hipStream_t s) {
    if (dim < 1 || dim > kNdMaxDim || ld < dim) return hipErrorInvalidValue;
    hipError_t e = hipMemsetAsync(acc, 0, (size_t)nlist * dim * sizeof(unsigned long long), s);
    if (e != hipSuccess) return e;
    e = hipMemsetAsync(counts, 0, (size_t)nlist * sizeof(int32_t), s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(kmeans_accum_nd_kernel, dim3(4096), dim3(256), 0, s, x, ld, dim, assign, rows, acc, counts);
    hipLaunchKernelGGL(kmeans_finalize_nd_kernel, dim3(nlist), dim3(128), 0, s, cents, dim, acc, counts, shift);
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------
// k-means++ seeding.  kpp_update_kernel: one workgroup per kKppBlockRows rows, 8 lanes per row (as in the IVF
// scans); kpp_pick_kernel: one workgroup finds the block, then the row, where the running sum passes u * total.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void kpp_update_kernel(const float* __restrict__ x, const float* __restrict__ xnorm, int64_t rows,
                                                         const float* __restrict__ centre, float* __restrict__ d2,
                                                         double* __restrict__ block_sums) {
    __shared__ double wsum[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int rr = lane >> 3, s8 = lane & 7;
    f32x4 cf[4];
    float cn = 0.f;
#pragma unroll
    for (int m = 0; m < 4; ++m) {
        cf[m] = *reinterpret_cast<const f32x4*>(centre + 4 * (s8 + 8 * m));
#pragma unroll
        for (int i = 0; i < 4; ++i) cn = fmaf(cf[m][i], cf[m][i], cn);
    }
    cn = dpp_add_xor1(cn);
    cn = dpp_add_xor2(cn);
    cn = dpp_add_half_mirror(cn);
    const int64_t row_begin = (int64_t)blockIdx.x * kKppBlockRows;
    double acc = 0.0;
    for (int r0 = wave * 8; r0 < kKppBlockRows; r0 += 32) {
        const int64_t row = row_begin + r0 + rr;
        const bool ok = row < rows;
        const float* src = x + (ok ? row : 0) * kDim + 4 * s8;
        float dot = 0.f;
#pragma unroll
        for (int m = 0; m < 4; ++m) {
            const f32x4 v = *reinterpret_cast<const f32x4*>(src + 32 * m);
#pragma unroll
            for (int i = 0; i < 4; ++i) dot = fmaf(v[i], cf[m][i], dot);
        }
        dot = dpp_add_xor1(dot);
        dot = dpp_add_xor2(dot);
        dot = dpp_add_half_mirror(dot);
        if (ok && s8 == 0) {
            const float d = fmaxf(fmaf(-2.0f, dot, xnorm[row] + cn), 0.f);
            const float nd = fminf(d2[row], d);
            d2[row] = nd;
            acc += (double)nd;
        }
    }
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) acc += __shfl_xor(acc, m);
    if (lane == 0) wsum[wave] = acc;
    __syncthreads();
    if (tid == 0) block_sums[blockIdx.x] = wsum[0] + wsum[1] + wsum[2] + wsum[3];
}

__global__ __launch_bounds__(1024) void kpp_pick_kernel(const float* __restrict__ x, int64_t rows, const float* __restrict__ d2,
                                                        const double* __restrict__ block_sums, int n_blocks, double u,
                                                        float* __restrict__ out_centre, int dim, int64_t ld) {
    __shared__ double s_part[1024];
    __shared__ double s_target, s_before;
    __shared__ int s_block;
    __shared__ long long s_row;
    const int tid = threadIdx.x;
    // total and the block where the running sum passes the target: block sums through LDS, 1024 at a time
    if (tid == 0) {
        s_before = 0.0;
        s_block = -1;
    }
    __syncthreads();
    double total = 0.0;
    for (int b0 = 0; b0 < n_blocks; b0 += 1024) {
        s_part[tid] = b0 + tid < n_blocks ? block_sums[b0 + tid] : 0.0;
        __syncthreads();
        for (int t = 0; t < 1024 && b0 + t < n_blocks; ++t) total += s_part[t];  // every thread: the same order, the same sum
        __syncthreads();
    }
    const double target = u * total;
    for (int b0 = 0; b0 < n_blocks; b0 += 1024) {
        s_part[tid] = b0 + tid < n_blocks ? block_sums[b0 + tid] : 0.0;
        __syncthreads();
        if (tid == 0 && s_block < 0) {
            double run = s_before;
            for (int t = 0; t < 1024 && b0 + t < n_blocks; ++t) {
                if (run + s_part[t] > target) {
                    s_block = b0 + t;
                    break;
                }
                run += s_part[t];
            }
            s_before = run;
        }
        __syncthreads();
    }
    if (tid == 0) {
        if (s_block < 0) s_block = n_blocks - 1;
        s_target = target;
        s_row = -1;
    }
    __syncthreads();
    const int64_t row = (int64_t)s_block * kKppBlockRows + tid;  // kKppBlockRows == blockDim.x
    s_part[tid] = row < rows ? (double)d2[row] : 0.0;
    __syncthreads();
    if (tid == 0) {
        double run = s_before;
        long long pick = -1;
        const int64_t last = min<int64_t>(rows, ((int64_t)s_block + 1) * kKppBlockRows) - 1;
        for (int t = 0; t < 1024; ++t) {
            run += s_part[t];
            if (run > s_target && s_part[t] > 0.0) {
                pick = (long long)s_block * kKppBlockRows + t;
                break;
            }
        }
        if (pick < 0) {  // rounding at the very end of the range (or an all-zero block): last row with d2 > 0, else the last row
            pick = last;
            for (int t = 1023; t >= 0; --t)
                if (s_part[t] > 0.0) {
                    pick = (long long)s_block * kKppBlockRows + t;
                    break;
                }
        }
        s_row = pick;
    }
    __syncthreads();
    for (int t = tid; t < dim; t += 1024) out_centre[t] = x[s_row * ld + t];  // rows ld floats apart, centres dim apart
}

hipError_t launch_kpp_step(const float* x, const float* xnorm, int64_t rows, float* cents, int c, float* d2, double* block_sums,
                           int n_blocks, double u, hipStream_t s) {
    hipLaunchKernelGGL(kpp_update_kernel, dim3(n_blocks), dim3(256), 0, s, x, xnorm, rows, cents + (size_t)(c - 1) * kDim, d2, block_sums);
    hipLaunchKernelGGL(kpp_pick_kernel, dim3(1), dim3(1024), 0, s, x, rows, d2, block_sums, n_blocks, u, cents + (size_t)c * kDim,
                       kDim, (int64_t)kDim);
    return hipGetLastError();
}

// The same step at any dimension (index builder of a general IVF index): rows [rows][ld] with ld = nd_dim_p(dim), zero
// padded; centres [nlist][dim], unpadded.  The centre goes through LDS (at 2048-d its 8 lanes x 64 f32x4 would not fit in
// registers), zero padded to ld.  Summation order of D^2, stated in vsearch.h at vs_ivf_build_nd: 8 lanes per row, lane s
// chains fmaf over the 16-byte chunks s, s + 8, s + 16, ... of the padded row (four elements each, in order), then the 8
// partial sums are added as (((p0+p1)+(p2+p3)) + ((p7+p6)+(p5+p4))) -- dpp_add_xor1 / xor2 / half_mirror, which at dim
// 128 is kpp_update_kernel's order.  ||c||^2 takes the same order; ||x||^2 is row_sqnorm_kernel's.  Everything else
// (d2 = min(d2, max(fma(-2, x.c, xn + cn), 0)), the double sums per kKppBlockRows rows) is kpp_update_kernel's.
__global__ __launch_bounds__(256) void kpp_update_nd_kernel(const float* __restrict__ x, int64_t ld, const float* __restrict__ xnorm,
                                                            int64_t rows, const float* __restrict__ centre, int dim,
                                                            float* __restrict__ d2, double* __restrict__ block_sums) {
    __shared__ __attribute__((aligned(16))) float cs[kNdMaxDim];
    __shared__ double wsum[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int rr = lane >> 3, s8 = lane & 7;
    const int n_chunks = (int)(ld >> 2);
    for (int t = tid; t < (int)ld; t += 256) cs[t] = t < dim ? centre[t] : 0.f;
    __syncthreads();
    float cn = 0.f;
    for (int ch = s8; ch < n_chunks; ch += 8) {
        const f32x4 c4 = *reinterpret_cast<const f32x4*>(cs + 4 * ch);
#pragma unroll
        for (int i = 0; i < 4; ++i) cn = fmaf(c4[i], c4[i], cn);
    }
    cn = dpp_add_xor1(cn);
    cn = dpp_add_xor2(cn);
    cn = dpp_add_half_mirror(cn);
    const int64_t row_begin = (int64_t)blockIdx.x * kKppBlockRows;
    double acc = 0.0;
    for (int r0 = wave * 8; r0 < kKppBlockRows; r0 += 32) {
        const int64_t row = row_begin + r0 + rr;
        const bool ok = row < rows;
        const float* src = x + (ok ? row : 0) * ld;
        float dot = 0.f;
        for (int ch = s8; ch < n_chunks; ch += 8) {
            const f32x4 v = *reinterpret_cast<const f32x4*>(src + 4 * ch);
            const f32x4 c4 = *reinterpret_cast<const f32x4*>(cs + 4 * ch);
#pragma unroll
            for (int i = 0; i < 4; ++i) dot = fmaf(v[i], c4[i], dot);
        }
        dot = dpp_add_xor1(dot);
        dot = dpp_add_xor2(dot);
        dot = dpp_add_half_mirror(dot);
        if (ok && s8 == 0) {
            const float d = fmaxf(fmaf(-2.0f, dot, xnorm[row] + cn), 0.f);
            const float nd = fminf(d2[row], d);
            d2[row] = nd;
            acc += (double)nd;
        }
    }
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) acc += __shfl_xor(acc, m);
    if (lane == 0) wsum[wave] = acc;
    __syncthreads();
    if (tid == 0) block_sums[blockIdx.x] = wsum[0] + wsum[1] + wsum[2] + wsum[3];
}

hipError_t launch_kpp_step_nd(const float* x, int64_t ld, const float* xnorm, int64_t rows, int dim, float* cents, int c, float* d2,
                              double* block_sums, int n_blocks, double u, hipStream_t s) {
    if (dim < 1 || dim > kNdMaxDim || ld != nd_dim_p(dim)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(kpp_update_nd_kernel, dim3(n_blocks), dim3(256), 0, s, x, ld, xnorm, rows, cents + (size_t)(c - 1) * dim, dim, d2,
                       block_sums);
    hipLaunchKernelGGL(kpp_pick_kernel, dim3(1), dim3(1024), 0, s, x, rows, d2, block_sums, n_blocks, u, cents + (size_t)c * dim, dim, ld);
    return hipGetLastError();
}

}  // namespace vs
