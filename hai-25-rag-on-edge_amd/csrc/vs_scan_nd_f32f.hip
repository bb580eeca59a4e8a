// vs_scan_nd_f32f.hip -- bf16 prefilter of the fp32 rows of a general index (any dim 1..2048), DESIGN 4.4f.
//
//   nd_filter_image_kernel      : at index creation, the rows once more as bf16 (RNE) in the A-fragment order of
//                                 v_mfma_f32_16x16x32_bf16, and the shard constants of FilterStats.
//   ndf_prep_kernel             : per launch group, the queries as bf16 B fragments in the matching k order, and per query
//                                 ||q'|| and the error bound E (filter_bound_nd); clears the group's counters.
//   scan_nd_f32f_kernel<CBW, IP>: ONE sweep over the image for up to 8 * CBW 16-query column blocks: a tiled product with a
//                                 threshold epilogue.  What passes is recomputed from the fp32 rows by RecheckNd (scan_nd_kernel's
//                                 chain, bit for bit) when the wave bins its buffer, so every id, distance bit and flag is
//                                 decided as scan_nd_kernel decides it.
//
// Image layout.  dim32 = dim rounded up to 32 elements, S = dim32 / 32 slabs.  A unit is 64 rows (four 16-row tiles); its
// image is S slabs of 4 KB, unit major:  img[((unit * S + s) * 4 + t) * 64 + lane][j], j < 8, lane = 16 g + r, holds
// bf16(row 64 unit + 16 t + r, element 32 s + 8 g + j): the 16 bytes of lane (r, g) are its A operand of tile t for
// K-slab s, so a slab is moved by four 1 KB LDS-DMA pieces and read back lane-linear (ds_read_b128 at 16 lane: no bank
// conflict, no swizzle).  Rows past n_rows and elements past dim are zero; there is one spare unit of zero rows.
// The prepared queries use the same k order: qbf[(cb * S + s) * 64 + lane][j] = bf16(Q[16 cb + r][32 s + 8 g + j]).
//
// Organisation.  Workgroup x of gridDim.x sweeps units x + n G; gridDim.y = passes, pass y serves column blocks
// [64 y CBW / 8 ...): wave w owns column blocks cb0 + w + 8 h, h < CBW, and keeps their accumulators for the unit's four
// row tiles (4 CBW f32x4) resident while K walks in slabs.  A step is one (unit, slab): every wave issues 1 + CBW LDS-DMA
// pieces for step j + D - 1 -- waves 0..3 one of the slab's four row pieces, waves 4..7 the unit's 64 stored norms (256
// bytes, the same piece four times), and every wave the CBW 1 KB B pieces of its own column blocks, which only it reads --
// waits for its own pieces of step j by a constant vmcnt, passes one raw s_barrier (which publishes the row pieces of
// step j and frees the slot of step j - 1), and feeds 4 CBW MFMAs from LDS.  The loop contains no other vector-memory
// instruction than these pieces and the (rare) candidate stores, which only make the counted wait stricter.
// Each unit of the image leaves HBM once per pass: ceil(n_cb / (8 CBW)) times per launch group, i.e. once up to 16
// batches and twice from 17 to 32 (CBW <= 4: the accumulators, not LDS, set that limit).
#include "vs_kernels.h"
#include "vs_dev.h"
#include "vs_sink.h"
#include "vs_ring.h"
#include <algorithm>

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
    uint4* out = reinterpret_cast<uint4*>(p.qbf) + (int64_t)batch * 2 * S * 64;
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

constexpr int kNdfWaves = 8;
constexpr int kNdfSlabBytes = kNdfUnitRows * 64;             // 4 KB: 64 rows x 32 bf16
constexpr int kNdfNormOff = kNdfSlabBytes;                   // the unit's 64 stored norms behind the rows
constexpr int kNdfBOff = kNdfSlabBytes + kNdfUnitRows * 4;   // the waves' B pieces behind those
constexpr int ndf_slot_bytes(int cbw) { return kNdfBOff + kNdfWaves * cbw * 1024; }
constexpr int ndf_depth(int cbw) { return std::min(8, (160 * 1024) / ndf_slot_bytes(cbw)); }  // slots of the ring

template <int CBW, bool IP>
__global__ __launch_bounds__(kNdfWaves * 64, 1) void scan_nd_f32f_kernel(const NdFilterParams p) {
    constexpr int NW = kNdfWaves;
    constexpr int D = ndf_depth(CBW);
    constexpr int kSlot = ndf_slot_bytes(CBW);
    constexpr int kStepVmem = 1 + CBW;  // vector-memory instructions per wave and step
    static_assert(D >= 3 && D * kSlot <= 160 * 1024, "the ring: one slot being read, one being filled, >= 1 in flight");
    static_assert((D - 2) * kStepVmem <= 63, "vmcnt is a 6-bit count");
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int r = lane & 15, g = lane >> 4;
    const int G = (int)gridDim.x, bx = (int)blockIdx.x;
    const int units_total = (int)((p.n_rows + kNdfUnitRows - 1) / kNdfUnitRows);
    const int T = (units_total - bx + G - 1) / G;  // units of this workgroup (G <= units_total: T >= 1)
    const int S = p.slabs;
    const int steps = T * S;
    const int n_cb = 2 * p.n_batches;
    const int cb0 = (int)blockIdx.y * NW * CBW;  // (cb0 < n_cb: the launcher's passes)

    // per (h, lane): the hot test's threshold of query 16 cb + r (filter_nd_th); +inf for a dead block or a padding query
    float th[CBW];
#pragma unroll
    for (int h = 0; h < CBW; ++h) {
        const int cb = cb0 + wave + NW * h;
        const int qrow = 16 * (cb & 1) + r;
        th[h] = VS_INF;
        if (cb < n_cb && qrow < p.nq_valid) {
            const int qg = (cb >> 1) * kMaxBatch + qrow;
            th[h] = filter_nd_th(IP ? 1 : 0, p.tau0[qg], p.qnorm[qg], p.qbound[qg], p.qnp[qg], p.bnmax, p.fstats.bpmax);
        }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // (the loads above are the compiler's; the counted queue starts empty)

    const unsigned ring_lds = __builtin_amdgcn_readfirstlane((unsigned)(size_t)(__attribute__((address_space(3))) char*)smem);
    const unsigned voff16 = (unsigned)lane * 16u, voff4 = (unsigned)lane * 4u;
    const char* const img = reinterpret_cast<const char*>(p.img);
    const char* qsrc[CBW];  // this wave's column blocks in the prepared queries (a block past the launch's: the last one)
#pragma unroll
    for (int h = 0; h < CBW; ++h) qsrc[h] = reinterpret_cast<const char*>(p.qbf) + (int64_t)min(cb0 + wave + NW * h, n_cb - 1) * S * 1024;
    // (an "s" operand must be in scalar registers whatever the compiler thinks of its divergence: every value here is wave-uniform)
    auto uni = [](const char* ptr) __attribute__((always_inline)) -> const char* {
        const unsigned long long v = (unsigned long long)ptr;
        const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)v), hi = __builtin_amdgcn_readfirstlane((unsigned)(v >> 32));
        return reinterpret_cast<const char*>(((unsigned long long)hi << 32) | lo);
    };
    // step (n, s) of the workgroup into ring slot `slot`: kStepVmem instructions; M0 saved and restored in the statement
    auto issue = [&](const int n, const int s, const int slot) __attribute__((always_inline)) {
        const int64_t unit = (int64_t)bx + (int64_t)n * G;
        const unsigned sbase = __builtin_amdgcn_readfirstlane(ring_lds + (unsigned)(slot * kSlot));
        unsigned keep;
        if (wave < 4) {
            const char* src = uni(img + (unit * S + s) * kNdfSlabBytes + wave * 1024);
            const unsigned dst = sbase + (unsigned)wave * 1024u;
            asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2 nt\n\ts_mov_b32 m0, %0"
                         : "=&s"(keep) : "v"(voff16), "s"(src), "s"(dst) : "memory");
        } else {
            const char* src = uni(reinterpret_cast<const char*>(p.bnorm + unit * kNdfUnitRows));
            const unsigned dst = sbase + (unsigned)kNdfNormOff;
            asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\tglobal_load_lds_dword %1, %2\n\ts_mov_b32 m0, %0"
                         : "=&s"(keep) : "v"(voff4), "s"(src), "s"(dst) : "memory");
        }
#pragma unroll
        for (int h = 0; h < CBW; ++h) {
            const char* src = uni(qsrc[h] + s * 1024);
            const unsigned dst = sbase + (unsigned)(kNdfBOff + (wave * CBW + h) * 1024);
            asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2\n\ts_mov_b32 m0, %0"
                         : "=&s"(keep) : "v"(voff16), "s"(src), "s"(dst) : "memory");
        }
    };

    int4* wbuf = p.sink.wbuf + ((int64_t)((int)blockIdx.y * G + bx) * NW + wave) * p.sink.wcap;
    int wbase = 0;  // wave-uniform fill of the private candidate buffer

    // the issue cursor runs D - 1 steps ahead of the read cursor; past the end it stays on the last step (a slot nobody reads)
    int ni = 0, si = 0;
    auto advance_issue = [&]() __attribute__((always_inline)) {
        if (ni * S + si + 1 < steps) {
            if (++si == S) si = 0, ++ni;
        }
    };
#pragma unroll
    for (int j = 0; j < D - 1; ++j) {
        issue(ni, si, j);
        advance_issue();
    }

    f32x4 acc[4][CBW];
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int h = 0; h < CBW; ++h) acc[t][h] = (f32x4){0.f, 0.f, 0.f, 0.f};
    int sl = 0, nc = 0, sc = 0;
#pragma clang loop unroll(disable)
    for (int j = 0; j < steps; ++j) {
        // this wave's pieces of step j have landed; behind the barrier so have everyone's, and step j - 1's slot is free
        wait_vm<(D - 2) * kStepVmem>();
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
        issue(ni, si, sl == 0 ? D - 1 : sl - 1);
        advance_issue();
        const char* slot = smem + sl * kSlot;
        i32x4 a[4], b[CBW];
#pragma unroll
        for (int t = 0; t < 4; ++t) a[t] = *reinterpret_cast<const i32x4*>(slot + t * 1024 + lane * 16);
#pragma unroll
        for (int h = 0; h < CBW; ++h) b[h] = *reinterpret_cast<const i32x4*>(slot + kNdfBOff + (wave * CBW + h) * 1024 + lane * 16);
#pragma unroll
        for (int h = 0; h < CBW; ++h)
#pragma unroll
            for (int t = 0; t < 4; ++t)
                acc[t][h] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a[t]), __builtin_bit_cast(bf16x8, b[h]), acc[t][h], 0, 0, 0);
        if (sc == S - 1) {  // (workgroup-uniform) the unit's last slab: the threshold epilogue
            const int row_u = (bx + nc * G) * kNdfUnitRows + 4 * g;
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                const f32x4 bn = *reinterpret_cast<const f32x4*>(slot + kNdfNormOff + (16 * t + 4 * g) * 4);
#pragma unroll
                for (int h = 0; h < CBW; ++h) {
                    f32x4 v;
#pragma unroll
                    for (int i = 0; i < 4; ++i) v[i] = IP ? acc[t][h][i] : fmaf(2.0f, acc[t][h][i], -bn[i]);
                    const float vmax = fmaxf(fmaxf(v[0], v[1]), fmaxf(v[2], v[3]));
                    if (__builtin_expect(__ballot(vmax > th[h]) != 0, 0)) {  // rare: a few hundred rows per query per million
#pragma unroll
                        for (int i = 0; i < 4; ++i) {
                            const int row = row_u + 16 * t + i;
                            const bool pass = v[i] > th[h] && row < (int)p.n_rows;
                            const unsigned long long mask = __ballot(pass);
                            if (mask) {  // wave-uniform
                                const int pos = wbase + (int)__builtin_amdgcn_mbcnt_hi((unsigned)(mask >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)mask, 0));
                                // (query, value, id): the value is replaced by RecheckNd's
                                if (pass && pos < p.sink.wcap)
                                    wbuf[pos] = make_int4(16 * (cb0 + wave + NW * h) + r, __builtin_bit_cast(int, v[i]), row + p.id_offset, 0);
                                wbase += __popcll(mask);
                            }
                        }
                    }
                    acc[t][h] = (f32x4){0.f, 0.f, 0.f, 0.f};
                }
            }
            sc = 0, ++nc;
        } else {
            ++sc;
            // the step's chains have issued, so its fragments have arrived: the barrier behind which the slot is refilled
            // follows the LDS reads
#pragma unroll
            for (int t = 0; t < 4; ++t)
#pragma unroll
                for (int h = 0; h < CBW; ++h) asm volatile("" : "+v"(acc[t][h]));
        }
        sl = sl + 1 == D ? 0 : sl + 1;
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // retire the tail prefetches before the wave ends
    const RecheckNd fix{p.base, p.bnorm, p.qfrag, p.qnorm, p.tau0, p.dim_p, IP ? 1 : 0, p.id_offset};
    int kept = sink_bin_wave<RecheckNd, true>(p.sink, ((int)blockIdx.y * G + bx) * NW + wave, wbase, lane, fix);
    if (p.sink.stats && wbase > 0) {  // (wave-uniform) one atomic instruction: lane 0 adds the sweep's count, lane 1 the survivors
#pragma unroll
        for (int u = 32; u >= 1; u >>= 1) kept += __shfl_xor(kept, u);
        if (lane < 2) atomicAdd(p.sink.stats + 2 + lane, (unsigned long long)(lane == 0 ? wbase : kept));
    }
}

template <int CBW, bool IP>
static hipError_t launch_ndf_t(const NdFilterParams& p, int grid, int passes, hipStream_t s) {
    constexpr int kLds = ndf_depth(CBW) * ndf_slot_bytes(CBW);
    auto kfn = scan_nd_f32f_kernel<CBW, IP>;
    static bool attr_set[64] = {};
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) dev = 0;
    if (!attr_set[dev]) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kfn), hipFuncAttributeMaxDynamicSharedMemorySize, kLds);
        if (e != hipSuccess) return e;
        attr_set[dev] = true;
    }
    hipLaunchKernelGGL(kfn, dim3(grid, passes), dim3(kNdfWaves * 64), kLds, s, p);
    return hipGetLastError();
}

hipError_t launch_scan_nd_f32f(const NdFilterParams& p, const NdFilterPlan& g, hipStream_t s) {
    const int64_t units = (p.n_rows + kNdfUnitRows - 1) / kNdfUnitRows;
    if (p.n_batches < 1 || p.n_batches > 32 || p.dim < 1 || p.dim > kNdMaxDim || p.dim_p != nd_dim_p(p.dim) || p.slabs != ndf_slabs(p.dim_p) ||
        g.grid < 1 || g.grid > units || g.passes < 1 || g.cbw < 1 || g.cbw > 4 || g.passes * kNdfWaves * g.cbw < 2 * p.n_batches ||
        (g.passes - 1) * kNdfWaves * g.cbw >= 2 * p.n_batches || (int64_t)g.grid * g.passes > kSlotStride || p.n_rows > 0x7fffffff - 2 * kNdfUnitRows ||
        !p.img || !p.qbf || !p.qfrag || !p.zero)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(ndf_prep_kernel, dim3(p.n_batches), dim3(256), 0, s, p);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    const bool ip = p.metric != 0;
    switch (g.cbw) {
    case 1: return ip ? launch_ndf_t<1, true>(p, g.grid, g.passes, s) : launch_ndf_t<1, false>(p, g.grid, g.passes, s);
    case 2: return ip ? launch_ndf_t<2, true>(p, g.grid, g.passes, s) : launch_ndf_t<2, false>(p, g.grid, g.passes, s);
    case 3: return ip ? launch_ndf_t<3, true>(p, g.grid, g.passes, s) : launch_ndf_t<3, false>(p, g.grid, g.passes, s);
    default: return ip ? launch_ndf_t<4, true>(p, g.grid, g.passes, s) : launch_ndf_t<4, false>(p, g.grid, g.passes, s);
    }
}

}  // namespace vs
