// vs_scan_nd_f16f.hip -- f16 MFMA prefilter on the half rows of a vs_bf_create_nd_f16 index (any dim 1..2048), DESIGN 4.4h.
//
//   nd_f16_stats_kernel         : at index creation, the shard constants of F16FilterStats from the stored half rows.
//   ndf16_sample_kernel         : at index creation, the compact copy of the sample rows (whole stored rows, unchanged).
//   ndf16_prep_kernel           : per launch group, the queries rounded to f16 (RNE, subnormals to zero) as B fragments in the
//                                 STORED k order of the rows, and per query ||q'|| and the error bound E (filter_bound_nd_f16);
//                                 clears the group's counters.
//   scan_nd_f16f_kernel<CBW, IP>: ONE sweep over the stored half rows for up to 8 * CBW 16-query column blocks with
//                                 v_mfma_f32_16x16x32_f16: ndf_sweep (vs_ndf_sweep.h, where the organisation is described) on
//                                 NdfHalfRowsSrc.  What passes is recomputed from the half rows by RecheckNdF16
//                                 (scan_nd_f16_kernel's chain, bit for bit) when the wave bins its buffer, so every id,
//                                 distance bit and flag is decided as scan_nd_f16_kernel decides it.
//
// No image.  The stored rows are [n_rows + 64][dim_h] halves, every 32-half block permuted: stored position w holds element
// nd_f16_elem_at(w) of the block (vs_scan_nd_f16.hip).  The 16 bytes at stored positions 8 g .. 8 g + 7 of block s of row r
// -- what lane (r, g) of scan_nd_f16_kernel loads -- are eight elements of K slab s, each element of the slab in exactly one
// lane group: a valid A operand of one 32-element MFMA step.  The permutation is only an order of the k index, and a dot
// product does not depend on it as long as B uses the same one: qb16[(cb * S + s) * 64 + lane][j] =
// f16(Q[16 cb + r][32 s + nd_f16_elem_at(8 g + j)]), S = dim_h / 32.
//
// The sweep's piece of row tile t of (unit, slab s) is therefore read in place: scalar base rows + ((64 unit + 16 t) dim_h +
// 32 s) 2 bytes, lane offset (r dim_h + 8 g) 2 bytes, so one LDS-DMA instruction covers 16 rows x one 64-byte segment.
#include "vs_kernels.h"
#include "vs_dev.h"
#include "vs_ndf_sweep.h"

namespace vs {

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));

// ---- creation ----
// one wave per row, four rows per workgroup; maxima by integer atomics on the bits of non-negative doubles
__global__ __launch_bounds__(256) void nd_f16_stats_kernel(const uint16_t* __restrict__ rows, const float* __restrict__ bnorm, int64_t n_rows,
                                                           int dim_h, unsigned long long* __restrict__ out) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= n_rows) return;  // (wave-uniform)
    const uint16_t* src = rows + row * dim_h;
    double n2 = 0.0;
    bool sub = false, bad = false;
    for (int c = lane; c < dim_h; c += 64) {
        const uint16_t b = src[c];
        const int ex = (b >> 10) & 31;
        sub = sub || (ex == 0 && (b & 0x3ff) != 0);
        bad = bad || ex == 31;
        const double x = (double)(float)__builtin_bit_cast(_Float16, b);  // (the order of the sum does not matter to a bound: rounded up below)
        n2 = fma(x, x, n2);
    }
#pragma unroll
    for (int u = 32; u >= 1; u >>= 1) n2 += __shfl_xor(n2, u);
    const bool any_sub = __any(sub), any_bad = __any(bad);
    if (lane == 0) {
        if (!any_bad) {
            atomicMax(out + 0, (unsigned long long)__double_as_longlong(n2));
            atomicMax(out + 1, (unsigned long long)__double_as_longlong((double)fabsf(bnorm[row])));  // the largest STORED norm
        }
        if (any_sub) atomicMax(out + 2, 1ull);
        if (any_bad || !(bnorm[row] < __builtin_inff())) atomicMax(out + 3, 1ull);
    }
}
hipError_t launch_nd_f16_stats(const uint16_t* rows, const float* bnorm, int64_t n_rows, int dim_h, unsigned long long* out, hipStream_t s) {
    if (n_rows <= 0) return hipSuccess;
    hipLaunchKernelGGL(nd_f16_stats_kernel, dim3((unsigned)((n_rows + 3) / 4)), dim3(256), 0, s, rows, bnorm, n_rows, dim_h, out);
    return hipGetLastError();
}

// rows i * stride, i < n, as they are stored, and their norms; grid = n, 256 threads
__global__ __launch_bounds__(256) void ndf16_sample_kernel(const uint16_t* __restrict__ rows, const float* __restrict__ bnorm, int64_t stride,
                                                           int dim_h, uint16_t* __restrict__ out, float* __restrict__ out_norm) {
    const int64_t i = blockIdx.x, row = i * stride;
    for (int c = threadIdx.x; c < dim_h; c += 256) out[i * dim_h + c] = rows[row * dim_h + c];
    if (threadIdx.x == 0) out_norm[i] = bnorm[row];
}
hipError_t launch_nd_f16_sample(const uint16_t* rows, const float* bnorm, int64_t n, int64_t stride, int dim_h, uint16_t* out, float* out_norm,
                                hipStream_t s) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(ndf16_sample_kernel, dim3((unsigned)n), dim3(256), 0, s, rows, bnorm, stride, dim_h, out, out_norm);
    return hipGetLastError();
}

// ---- query preparation ----
// the half that B holds for the query value x: f16(x) by RNE; an f16 subnormal is written as zero (B never holds a
// subnormal), and so is a value that rounds to +-inf or is NaN, whose query gets E = +inf (`bad`)
__device__ __forceinline__ uint16_t ndf16_round(float x, bool& bad) {
    const uint16_t b = __builtin_bit_cast(uint16_t, (_Float16)x);
    const int ex = (b >> 10) & 31;
    if (ex == 31) bad = true;
    return (ex == 0 || ex == 31) ? (uint16_t)0 : b;
}

// grid = n_batches, 256 threads
__global__ __launch_bounds__(256) void ndf16_prep_kernel(const NdF16FilterParams p) {
    const int batch = blockIdx.x, tid = threadIdx.x;
    for (int i = batch * 256 + tid; i < p.zero_words; i += gridDim.x * 256) p.zero[i] = 0;
    const float* qb = p.q + (int64_t)batch * p.q_batch_stride;
    const int S = p.slabs, dim = p.dim;
    uint4* out = reinterpret_cast<uint4*>(p.qb16) + (int64_t)batch * 2 * S * 64;
    for (int e = tid; e < 2 * S * 64; e += 256) {
        const int lane = e & 63, s = (e >> 6) % S, h = (e >> 6) / S;
        const int qi = 16 * h + (lane & 15), g = lane >> 4;
        unsigned w[4];
        bool bad = false;
#pragma unroll
        for (int j = 0; j < 8; j += 2) {
            const int k0 = 32 * s + nd_f16_elem_at(8 * g + j), k1 = 32 * s + nd_f16_elem_at(8 * g + j + 1);
            const float x0 = (qi < p.nq_valid && k0 < dim) ? qb[(int64_t)qi * dim + k0] : 0.f;
            const float x1 = (qi < p.nq_valid && k1 < dim) ? qb[(int64_t)qi * dim + k1] : 0.f;
            w[j >> 1] = (unsigned)ndf16_round(x0, bad) | ((unsigned)ndf16_round(x1, bad) << 16);
        }
        out[e] = make_uint4(w[0], w[1], w[2], w[3]);
    }
    // ||q||, ||q'||, ||q - q'|| and ||q'||_1 in double from the values written, 8 threads per query
    const int row = tid >> 3, j = tid & 7;
    const bool live = row < p.nq_valid;
    const float* src = qb + (int64_t)(live ? row : 0) * dim;
    double n2 = 0.0, e2 = 0.0, p2 = 0.0, l1 = 0.0;
    bool bad = false;
    for (int i = j; i < dim; i += 8) {
        const float x = src[i];
        const double xp = (double)(float)__builtin_bit_cast(_Float16, ndf16_round(x, bad));
        const double d = (double)x - xp;
        n2 = fma((double)x, (double)x, n2);
        e2 = fma(d, d, e2);
        p2 = fma(xp, xp, p2);
        l1 += fabs(xp);
    }
    int ok_q = bad ? 0 : 1;
#pragma unroll
    for (int u = 1; u < 8; u <<= 1) {
        n2 += __shfl_xor(n2, u);
        e2 += __shfl_xor(e2, u);
        p2 += __shfl_xor(p2, u);
        l1 += __shfl_xor(l1, u);
        ok_q &= __shfl_xor(ok_q, u);
    }
    if (j == 0) {
        const int qg = batch * kMaxBatch + row;
        p.qbound[qg] = !live ? 0.f : ok_q ? filter_bound_nd_f16(dim, sqrt(e2), sqrt(n2), sqrt(p2), l1, p.fstats) : __builtin_inff();
        p.qnp[qg] = live ? (float)(sqrt(p2) * (1.0 + 1.0 / 1048576.0)) : 0.f;
    }
}

// the exact recheck: scan_nd_f16_kernel's dot of (row, query) -- scan_nd_kernel's chain at dim_p = dim_h: segment c of 16
// floats, step i, lane group g adds element 16 c + 4 g + i, each product rounded like an fmaf -- from the stored half row
// widened with (float) and the zero-padded fp32 query fragments that nd_prep_kernel wrote, its distance, and the exact
// test against tau0.  The stored permutation is undone by address: element 16 c + 4 g + i of the row sits at stored
// position 32 (c >> 1) + 8 g + 4 (c & 1) + i, i.e. in half 4 (c & 1) + i of the 16 bytes of lane group g in block c >> 1.
struct RecheckNdF16 {
    const uint16_t* rows;
    const float* bnorm;
    const float* qfrag;  // ScanNdF16Params::qfrag
    const float* qnorm;
    const float* tau0;
    int dim_h, metric;
    int32_t id_offset;
    __device__ __forceinline__ int4 operator()(const int4& c) const {
        const int qg = c.x, batch = qg / kMaxBatch, qi = qg % kMaxBatch;
        const int64_t row = (int64_t)c.z - id_offset;
        const int S = dim_h / 32;
        const f16x8* b = reinterpret_cast<const f16x8*>(rows + row * dim_h);
        // fragment (c, h, lane = 16 g + r) = Q[16 h + r][16 c + 4 g ..]
        const f32x4* qf = reinterpret_cast<const f32x4*>(qfrag) + (int64_t)batch * (2 * S) * 128 + (qi >> 4) * 64 + (qi & 15);
        float dot = 0.f;
        for (int s = 0; s < S; ++s) {
            f16x8 bv[4];
#pragma unroll
            for (int g = 0; g < 4; ++g) bv[g] = b[4 * s + g];
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                f32x4 qv[4];
#pragma unroll
                for (int g = 0; g < 4; ++g) qv[g] = qf[(2 * s + u) * 128 + 16 * g];
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int g = 0; g < 4; ++g) dot = fmaf((float)bv[g][4 * u + i], qv[g][i], dot);
            }
        }
        const float d = metric ? -dot : fmaf(-2.0f, dot, qnorm[qg] + bnorm[row]);
        return d < tau0[qg] ? make_int4(qg, __builtin_bit_cast(int, d), c.z, 0) : make_int4(-1, 0, 0, 0);
    }
};

template <int CBW, bool IP>
__global__ __launch_bounds__(kNdfWaves * 64, 1) void scan_nd_f16f_kernel(const NdF16FilterParams p);

// the stored half rows as the sweep's source of rows (vs_ndf_sweep.h): no image.  The 64 spare rows behind the base serve
// as the spare unit.
struct NdfHalfRowsSrc {
    using Params = NdF16FilterParams;
    const char* rows;
    int64_t unit_bytes, tile_bytes;
    unsigned voff;  // scan_nd_f16_kernel's voff: this lane's 16 bytes of a tile's segment
    __device__ __forceinline__ NdfHalfRowsSrc(const Params& p, int lane)
        : rows(reinterpret_cast<const char*>(p.rows)), unit_bytes((int64_t)kNdfUnitRows * p.dim_h * 2), tile_bytes((int64_t)16 * p.dim_h * 2),
          voff((unsigned)((lane & 15) * p.dim_h + 8 * (lane >> 4)) * 2u) {}
    // row tile `wave` of the unit, slab s: 16 rows x one 64-byte segment, straight from the stored rows (LDS-DMA with
    // per-lane addresses: one instruction covers the tile's piece and lands lane-linear)
    __device__ __forceinline__ const char* row_piece(int64_t unit, int s, int wave) const {
        return rows + unit * unit_bytes + wave * tile_bytes + s * 64;
    }
    static __device__ __forceinline__ f32x4 mfma(const i32x4& a, const i32x4& b, const f32x4& c) {
        return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
    }
    // filter_nd_th with ||b'||max = ||b||max: the rows are not rounded.  A query without a bound (E = +inf: a value that f16
    // cannot hold) sends the group to the per-batch scan behind at once: the overflow word is raised here, by the first
    // workgroup of the pass, and nothing of that query is written (what the sweep finds is not ranked once the word is set)
    static __device__ __forceinline__ float threshold(const Params& p, int ip, int qg, bool herald) {
        const float e = p.qbound[qg];
        if (e < VS_INF) return filter_nd_th(ip, p.tau0[qg], p.qnorm[qg], e, p.qnp[qg], p.bnmax, p.fstats.bmax);
        if (herald) sink_raise_overflow(p.sink);
        return VS_INF;
    }
    static __device__ __forceinline__ RecheckNdF16 recheck(const Params& p, int ip) {
        return RecheckNdF16{p.rows, p.bnorm, p.qfrag, p.qnorm, p.tau0, p.dim_h, ip, p.id_offset};
    }
    template <int CBW, bool IP>
    static auto kernel() { return scan_nd_f16f_kernel<CBW, IP>; }
};

template <int CBW, bool IP>
__global__ __launch_bounds__(kNdfWaves * 64, 1) void scan_nd_f16f_kernel(const NdF16FilterParams p) { ndf_sweep<NdfHalfRowsSrc, CBW, IP>(p); }

hipError_t launch_scan_nd_f16f(const NdF16FilterParams& p, const NdFilterPlan& g, hipStream_t s) {
    if (!ndf_sweep_args_ok(p, g) || p.dim_h != nd_dim_h(p.dim) || p.slabs != p.dim_h / 32 || p.nq_valid < 1 || p.nq_valid > kMaxBatch || !p.rows ||
        !p.bnorm || p.sink.wcap < 1)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(ndf16_prep_kernel, dim3(p.n_batches), dim3(256), 0, s, p);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    return launch_ndf_sweep<NdfHalfRowsSrc>(p, g, s);
}

}  // namespace vs
