// vs_scan_nd_f32f.hip -- bf16 prefilter of the fp32 rows of a general index (any dim 1..2048), DESIGN 4.4f.
//
//   nd_filter_image_kernel      : at index creation, the rows once more as bf16 (RNE) in the A-fragment order of
//                                 v_mfma_f32_16x16x32_bf16, and the shard constants of FilterStats.
//   ndf_prep_kernel             : per launch group, the queries as bf16 B fragments in the matching k order, and per query
//                                 ||q'|| and the error bound E (filter_bound_nd); clears the group's counters.
//   scan_nd_f32f_kernel<CBW, IP>: ONE sweep over the image for up to 8 * CBW 16-query column blocks: ndf_sweep (vs_ndf_sweep.h,
//                                 where the organisation is described) on NdfImageSrc.  What passes is recomputed from the
//                                 fp32 rows by RecheckNd (scan_nd_kernel's chain, bit for bit) when the wave bins its buffer,
//                                 so every id, distance bit and flag is decided as scan_nd_kernel decides it.
//
// Image layout.  dim32 = dim rounded up to 32 elements, S = dim32 / 32 slabs.  A unit is 64 rows (four 16-row tiles); its
// image is S slabs of 4 KB, unit major:  img[((unit * S + s) * 4 + t) * 64 + lane][j], j < 8, lane = 16 g + r, holds
// bf16(row 64 unit + 16 t + r, element 32 s + 8 g + j): the 16 bytes of lane (r, g) are its A operand of tile t for
// K-slab s, so a slab is moved by four 1 KB LDS-DMA pieces and read back lane-linear (ds_read_b128 at 16 lane: no bank
// conflict, no swizzle).  Rows past n_rows and elements past dim are zero; there is one spare unit of zero rows.
// The prepared queries use the same k order: qb16[(cb * S + s) * 64 + lane][j] = bf16(Q[16 cb + r][32 s + 8 g + j]).
#include "vs_kernels.h"
#include "vs_dev.h"
#include "vs_ndf_sweep.h"

namespace vs {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

__device__ __forceinline__ bool ndf_scaled(float x) {
    const float a = fabsf(x);
    return a == 0.f || (a >= (float)kFiltLo && a <= (float)kFiltHi);  // (false for inf and NaN)
}
__device__ __forceinline__ unsigned ndf_pack2(float x0, float x1) {
    return (unsigned)__builtin_bit_cast(uint16_t, (__bf16)x0) | ((unsigned)__builtin_bit_cast(uint16_t, (__bf16)x1) << 16);
}

// grid = units (of real rows), 256 threads: wave t takes tile t of the unit, lane (r, g) the elements 8 g .. 8 g + 7 of
// every slab of row 16 t + r.  Statistics in double (exact squares of the rounding residuals), maxima by integer atomics
// on the bits of non-negative doubles.
__global__ __launch_bounds__(256) void nd_filter_image_kernel(const float* __restrict__ v, const float* __restrict__ bnorm, int64_t rows,
                                                              int dim_p, int slabs, unsigned long long* __restrict__ out,
                                                              uint16_t* __restrict__ img) {
    const int tid = threadIdx.x, lane = tid & 63, r = lane & 15, g = lane >> 4;
    const int64_t row = (int64_t)blockIdx.x * kNdfUnitRows + 16 * (tid >> 6) + r;
    const bool ok = row < rows;
    const float* src = v + (ok ? row : 0) * (int64_t)dim_p;
    double n2 = 0.0, e2 = 0.0, p2 = 0.0;
    bool bad = false;
    for (int s = 0; s < slabs; ++s) {
        const int k0 = 32 * s + 8 * g;
        float x[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) x[j] = 0.f;
        if (ok && k0 < dim_p) {  // (dim_p is a multiple of 16: eight floats are inside or outside together)
            const f32x4 lo = *reinterpret_cast<const f32x4*>(src + k0), hi = *reinterpret_cast<const f32x4*>(src + k0 + 4);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                x[j] = lo[j];
                x[4 + j] = hi[j];
            }
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const float xp = (float)(__bf16)x[j];
            bad = bad || !ndf_scaled(x[j]);
            const double d = (double)x[j] - (double)xp;
            n2 = fma((double)x[j], (double)x[j], n2);
            e2 = fma(d, d, e2);
            p2 = fma((double)xp, (double)xp, p2);
        }
        if (img)
            *reinterpret_cast<uint4*>(img + (((int64_t)blockIdx.x * slabs + s) * 256 + tid) * 8) =
                make_uint4(ndf_pack2(x[0], x[1]), ndf_pack2(x[2], x[3]), ndf_pack2(x[4], x[5]), ndf_pack2(x[6], x[7]));
    }
    // the four lanes (r, g = 0..3) of a row
    n2 += __shfl_xor(n2, 16), e2 += __shfl_xor(e2, 16), p2 += __shfl_xor(p2, 16);
    n2 += __shfl_xor(n2, 32), e2 += __shfl_xor(e2, 32), p2 += __shfl_xor(p2, 32);
    const bool any_bad = __any(ok && bad);
    if (ok && g == 0) {
        atomicMax(out + 0, (unsigned long long)__double_as_longlong(n2));
        atomicMax(out + 1, (unsigned long long)__double_as_longlong(e2));
        atomicMax(out + 2, (unsigned long long)__double_as_longlong(p2));
        atomicMax(out + 4, (unsigned long long)__double_as_longlong((double)bnorm[row]));  // the largest STORED norm
    }
    if (any_bad && lane == 0) atomicMax(out + 3, 1ull);
}

hipError_t launch_nd_filter_image(const float* v, const float* bnorm, int64_t rows, int dim_p, unsigned long long* out, uint16_t* img,
                                  hipStream_t s) {
    if (rows <= 0) return hipSuccess;
    const int64_t units = (rows + kNdfUnitRows - 1) / kNdfUnitRows;
    hipLaunchKernelGGL(nd_filter_image_kernel, dim3((unsigned)units), dim3(256), 0, s, v, bnorm, rows, dim_p, ndf_slabs(dim_p), out, img);
    return hipGetLastError();
}

// the compact copy of the sample rows (row i * stride, i < n) and of their stored norms; grid = n, 256 threads
__global__ __launch_bounds__(256) void ndf_sample_kernel(const float* __restrict__ v, const float* __restrict__ bnorm, int64_t stride, int dim_p,
                                                         float* __restrict__ out, float* __restrict__ out_norm) {
    const int64_t i = blockIdx.x, row = i * stride;
    for (int c = threadIdx.x; c < dim_p; c += 256) out[i * dim_p + c] = v[row * dim_p + c];
    if (threadIdx.x == 0) out_norm[i] = bnorm[row];
}
hipError_t launch_nd_filter_sample(const float* v, const float* bnorm, int64_t n, int64_t stride, int dim_p, float* out, float* out_norm,
                                   hipStream_t s) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(ndf_sample_kernel, dim3((unsigned)n), dim3(256), 0, s, v, bnorm, stride, dim_p, out, out_norm);
    return hipGetLastError();
}

// grid = n_batches, 256 threads
__global__ __launch_bounds__(256) void ndf_prep_kernel(const NdFilterParams p) {
    const int batch = blockIdx.x, tid = threadIdx.x;
    for (int i = batch * 256 + tid; i < p.zero_words; i += gridDim.x * 256) p.zero[i] = 0;
    const float* qb = p.q + (int64_t)batch * p.q_batch_stride;
    const int S = p.slabs, dim = p.dim;
    uint4* out = reinterpret_cast<uint4*>(p.qb16) + (int64_t)batch * 2 * S * 64;
    for (int e = tid; e < 2 * S * 64; e += 256) {
        const int lane = e & 63, s = (e >> 6) % S, h = (e >> 6) / S;
        const int qi = 16 * h + (lane & 15), k0 = 32 * s + 8 * (lane >> 4);
        float x[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) x[j] = (qi < p.nq_valid && k0 + j < dim) ? qb[(int64_t)qi * dim + k0 + j] : 0.f;
        out[e] = make_uint4(ndf_pack2(x[0], x[1]), ndf_pack2(x[2], x[3]), ndf_pack2(x[4], x[5]), ndf_pack2(x[6], x[7]));
    }
    // ||q||, ||q'||, ||q - q'|| in double, 8 threads per query
    const int row = tid >> 3, j = tid & 7;
    const bool live = row < p.nq_valid;
    const float* src = qb + (int64_t)(live ? row : 0) * dim;
    double n2 = 0.0, e2 = 0.0, p2 = 0.0;
    int ok_q = 1;
    for (int i = j; i < dim; i += 8) {
        const float x = src[i], xp = (float)(__bf16)x;
        ok_q &= ndf_scaled(x) ? 1 : 0;
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
        ok_q &= __shfl_xor(ok_q, u);
    }
    if (j == 0) {
        const int qg = batch * kMaxBatch + row;
        p.qbound[qg] = !live ? 0.f : ok_q ? filter_bound_nd(dim, sqrt(e2), sqrt(n2), sqrt(p2), p.fstats) : __builtin_inff();
        p.qnp[qg] = live ? (float)(sqrt(p2) * (1.0 + 1.0 / 1048576.0)) : 0.f;
    }
}

// the exact recheck: scan_nd_kernel's dot of (row, query) -- segment c of 16 floats, step i, lane group g adds element
// 16 c + 4 g + i, each product rounded like an fmaf -- from the fp32 row and the zero-padded fp32 query fragments
// that nd_prep_kernel wrote, its distance, and the exact test against tau0
struct RecheckNd {
    const float* base;
    const float* bnorm;
    const float* qfrag;  // ScanNdParams::qfrag
    const float* qnorm;
    const float* tau0;
    int dim_p, metric;
    int32_t id_offset;
    __device__ __forceinline__ int4 operator()(const int4& c) const {
        const int qg = c.x, batch = qg / kMaxBatch, qi = qg % kMaxBatch;
        const int64_t row = (int64_t)c.z - id_offset;
        const int C = dim_p / 16;
        const f32x4* b = reinterpret_cast<const f32x4*>(base + row * dim_p);
        // fragment (c, h, lane = 16 g + r) = Q[16 h + r][16 c + 4 g ..]
        const f32x4* qf = reinterpret_cast<const f32x4*>(qfrag) + (int64_t)batch * C * 128 + (qi >> 4) * 64 + (qi & 15);
        float dot = 0.f;
        for (int cc = 0; cc < C; ++cc) {
            f32x4 bv[4], qv[4];
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                bv[g] = b[4 * cc + g];
                qv[g] = qf[cc * 128 + 16 * g];
            }
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int g = 0; g < 4; ++g) dot = fmaf(bv[g][i], qv[g][i], dot);
        }
        const float d = metric ? -dot : fmaf(-2.0f, dot, qnorm[qg] + bnorm[row]);
        return d < tau0[qg] ? make_int4(qg, __builtin_bit_cast(int, d), c.z, 0) : make_int4(-1, 0, 0, 0);
    }
};

template <int CBW, bool IP>
__global__ __launch_bounds__(kNdfWaves * 64, 1) void scan_nd_f32f_kernel(const NdFilterParams p);

// the image as the sweep's source of rows (vs_ndf_sweep.h)
struct NdfImageSrc {
    using Params = NdFilterParams;
    const char* img;
    int S;
    unsigned voff;  // a slab's piece of a tile is lane-linear in the image
    __device__ __forceinline__ NdfImageSrc(const Params& p, int lane)
        : img(reinterpret_cast<const char*>(p.img)), S(p.slabs), voff((unsigned)lane * 16u) {}
    __device__ __forceinline__ const char* row_piece(int64_t unit, int s, int wave) const {
        return img + (unit * S + s) * kNdfSlabBytes + wave * 1024;
    }
    static __device__ __forceinline__ f32x4 mfma(const i32x4& a, const i32x4& b, const f32x4& c) {
        return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
    }
    // filter_nd_th; a query outside the well-scaled range has E = +inf, which leaves the threshold at -inf: everything passes
    static __device__ __forceinline__ float threshold(const Params& p, int ip, int qg, bool) {
        return filter_nd_th(ip, p.tau0[qg], p.qnorm[qg], p.qbound[qg], p.qnp[qg], p.bnmax, p.fstats.bpmax);
    }
    static __device__ __forceinline__ RecheckNd recheck(const Params& p, int ip) {
        return RecheckNd{p.base, p.bnorm, p.qfrag, p.qnorm, p.tau0, p.dim_p, ip, p.id_offset};
    }
    template <int CBW, bool IP>
    static auto kernel() { return scan_nd_f32f_kernel<CBW, IP>; }
};

template <int CBW, bool IP>
__global__ __launch_bounds__(kNdfWaves * 64, 1) void scan_nd_f32f_kernel(const NdFilterParams p) { ndf_sweep<NdfImageSrc, CBW, IP>(p); }

hipError_t launch_scan_nd_f32f(const NdFilterParams& p, const NdFilterPlan& g, hipStream_t s) {
    if (!ndf_sweep_args_ok(p, g) || p.dim_p != nd_dim_p(p.dim) || p.slabs != ndf_slabs(p.dim_p) || !p.img) return hipErrorInvalidValue;
    hipLaunchKernelGGL(ndf_prep_kernel, dim3(p.n_batches), dim3(256), 0, s, p);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    return launch_ndf_sweep<NdfImageSrc>(p, g, s);
}

}  // namespace vs
