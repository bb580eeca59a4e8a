// vs_scan_nd_f16f.hip -- f16 MFMA prefilter on the half rows of a vs_bf_create_nd_f16 index (any dim 1..2048), DESIGN 4.4h.
//
//   nd_f16_stats_kernel         : at index creation, the shard constants of F16FilterStats from the stored half rows.
//   ndf16_sample_kernel         : at index creation, the compact copy of the sample rows (whole stored rows, unchanged).
//   ndf16_prep_kernel           : per launch group, the queries rounded to f16 (RNE, subnormals to zero) as B fragments in the
//                                 STORED k order of the rows, and per query ||q'|| and the error bound E (filter_bound_nd_f16);
//                                 clears the group's counters.
//   scan_nd_f16f_kernel<CBW, IP>: ONE sweep over the stored half rows for up to 8 * CBW 16-query column blocks with
//                                 v_mfma_f32_16x16x32_f16: a tiled product with a threshold epilogue.  What passes is recomputed
//                                 from the half rows by RecheckNdF16 (scan_nd_f16_kernel's chain, bit for bit) when the wave
//                                 bins its buffer, so every id, distance bit and flag is decided as scan_nd_f16_kernel decides it.
//
// No image.  The stored rows are [n_rows + 64][dim_h] halves, every 32-half block permuted: stored position w holds element
// nd_f16_elem_at(w) of the block (vs_scan_nd_f16.hip).  The 16 bytes at stored positions 8 g .. 8 g + 7 of block s of row r
// -- what lane (r, g) of scan_nd_f16_kernel loads -- are eight elements of K slab s, each element of the slab in exactly one
// lane group: a valid A operand of one 32-element MFMA step.  The permutation is only an order of the k index, and a dot
// product does not depend on it as long as B uses the same one: qh[(cb * S + s) * 64 + lane][j] =
// f16(Q[16 cb + r][32 s + nd_f16_elem_at(8 g + j)]), S = dim_h / 32.
//
// Organisation: scan_nd_f32f_kernel's.  A unit is 64 rows (four 16-row tiles; the 64 spare rows behind the
// base serve as the spare unit).  Workgroup x of gridDim.x sweeps units x + n G; gridDim.y = passes; wave w owns column
// blocks cb0 + w + 8 h, h < CBW, and keeps their 4 CBW f32x4 accumulators resident while K walks in 32-element slabs.  A
// step is one (unit, slab): waves 0..3 issue the slab's piece of row tile `wave` -- LDS-DMA with per-lane addresses, scalar
// base rows + ((64 unit + 16 t) dim_h + 32 s) 2 bytes, lane offset (r dim_h + 8 g) 2 bytes, so one instruction covers 16 rows
// x one 64-byte segment and lands lane-linear (1 KB per tile and slab, read back with one ds_read_b128 at 16 lane, no
// swizzle) -- waves 4..7 the unit's 64 stored norms, and every wave the CBW 1 KB B pieces of its own column blocks.  Waits
// use one constant vmcnt, one raw s_barrier per step; the loop holds no other vector-memory instruction than these pieces
// and the (rare) candidate stores.
#include "vs_kernels.h"
#include "vs_dev.h"
#include "vs_sink.h"
#include "vs_ring.h"
#include <algorithm>

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
    uint4* out = reinterpret_cast<uint4*>(p.qh) + (int64_t)batch * 2 * S * 64;
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

constexpr int kNdhfWaves = 8;
constexpr int kNdhfSlabBytes = kNdfUnitRows * 64;              // 4 KB: 64 rows x 32 halves
constexpr int kNdhfNormOff = kNdhfSlabBytes;                   // the unit's 64 stored norms behind the rows
constexpr int kNdhfBOff = kNdhfSlabBytes + kNdfUnitRows * 4;   // the waves' B pieces behind those
constexpr int ndhf_slot_bytes(int cbw) { return kNdhfBOff + kNdhfWaves * cbw * 1024; }
constexpr int ndhf_depth(int cbw) { return std::min(8, (160 * 1024) / ndhf_slot_bytes(cbw)); }  // slots of the ring

template <int CBW, bool IP>
__global__ __launch_bounds__(kNdhfWaves * 64, 1) void scan_nd_f16f_kernel(const NdF16FilterParams p) {
    constexpr int NW = kNdhfWaves;
    constexpr int D = ndhf_depth(CBW);
    constexpr int kSlot = ndhf_slot_bytes(CBW);
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

    // per (h, lane): the hot test's threshold of query 16 cb + r (filter_nd_th with ||b'||max = ||b||max: the rows are not
    // rounded); +inf for a dead block or a padding query.  A query without a bound (E = +inf: a value that f16 cannot
    // hold) sends the group to the per-batch scan behind at once: the overflow word is raised here, by the first workgroup
    // of the pass, and nothing of that query is written (what the sweep finds is not ranked once the word is set)
    float th[CBW];
#pragma unroll
    for (int h = 0; h < CBW; ++h) {
        const int cb = cb0 + wave + NW * h;
        const int qrow = 16 * (cb & 1) + r;
        th[h] = VS_INF;
        if (cb < n_cb && qrow < p.nq_valid) {
            const int qg = (cb >> 1) * kMaxBatch + qrow;
            const float e = p.qbound[qg];
            if (e < VS_INF) th[h] = filter_nd_th(IP ? 1 : 0, p.tau0[qg], p.qnorm[qg], e, p.qnp[qg], p.bnmax, p.fstats.bmax);
            else if (bx == 0 && g == 0) sink_raise_overflow(p.sink);
        }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // (the accesses above are the compiler's; the counted queue starts empty)

    const unsigned ring_lds = __builtin_amdgcn_readfirstlane((unsigned)(size_t)(__attribute__((address_space(3))) char*)smem);
    const unsigned voff16 = (unsigned)lane * 16u, voff4 = (unsigned)lane * 4u;
    const unsigned voff_row = (unsigned)(r * p.dim_h + 8 * g) * 2u;  // scan_nd_f16_kernel's voff: this lane's 16 bytes of a tile's segment
    const int64_t unit_bytes = (int64_t)kNdfUnitRows * p.dim_h * 2, tile_bytes = (int64_t)16 * p.dim_h * 2;
    const char* const rows = reinterpret_cast<const char*>(p.rows);
    const char* qsrc[CBW];  // this wave's column blocks in the prepared queries (a block past the launch's: the last one)
#pragma unroll
    for (int h = 0; h < CBW; ++h) qsrc[h] = reinterpret_cast<const char*>(p.qh) + (int64_t)min(cb0 + wave + NW * h, n_cb - 1) * S * 1024;
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
        if (wave < 4) {  // row tile `wave` of the unit, slab s: 16 rows x one 64-byte segment, straight from the stored rows
            const char* src = uni(rows + unit * unit_bytes + wave * tile_bytes + s * 64);
            const unsigned dst = sbase + (unsigned)wave * 1024u;
            asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2 nt\n\ts_mov_b32 m0, %0"
                         : "=&s"(keep) : "v"(voff_row), "s"(src), "s"(dst) : "memory");
        } else {
            const char* src = uni(reinterpret_cast<const char*>(p.bnorm + unit * kNdfUnitRows));
            const unsigned dst = sbase + (unsigned)kNdhfNormOff;
            asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\tglobal_load_lds_dword %1, %2\n\ts_mov_b32 m0, %0"
                         : "=&s"(keep) : "v"(voff4), "s"(src), "s"(dst) : "memory");
        }
#pragma unroll
        for (int h = 0; h < CBW; ++h) {
            const char* src = uni(qsrc[h] + s * 1024);
            const unsigned dst = sbase + (unsigned)(kNdhfBOff + (wave * CBW + h) * 1024);
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
        for (int h = 0; h < CBW; ++h) b[h] = *reinterpret_cast<const i32x4*>(slot + kNdhfBOff + (wave * CBW + h) * 1024 + lane * 16);
#pragma unroll
        for (int h = 0; h < CBW; ++h)
#pragma unroll
            for (int t = 0; t < 4; ++t)
                acc[t][h] = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, a[t]), __builtin_bit_cast(f16x8, b[h]), acc[t][h], 0, 0, 0);
        if (sc == S - 1) {  // (workgroup-uniform) the unit's last slab: the threshold epilogue
            const int row_u = (bx + nc * G) * kNdfUnitRows + 4 * g;
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                const f32x4 bn = *reinterpret_cast<const f32x4*>(slot + kNdhfNormOff + (16 * t + 4 * g) * 4);
#pragma unroll
                for (int h = 0; h < CBW; ++h) {
                    f32x4 v;
#pragma unroll
                    for (int i = 0; i < 4; ++i) v[i] = IP ? acc[t][h][i] : fmaf(2.0f, acc[t][h][i], -bn[i]);
                    const float vmax = fmaxf(fmaxf(v[0], v[1]), fmaxf(v[2], v[3]));
                    if (__builtin_expect(__ballot(vmax > th[h]) != 0, 0)) {  // rare
#pragma unroll
                        for (int i = 0; i < 4; ++i) {
                            const int row = row_u + 16 * t + i;
                            const bool pass = v[i] > th[h] && row < (int)p.n_rows;
                            const unsigned long long mask = __ballot(pass);
                            if (mask) {  // wave-uniform
                                const int pos = wbase + (int)__builtin_amdgcn_mbcnt_hi((unsigned)(mask >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)mask, 0));
                                // (query, value, id): the value is replaced by RecheckNdF16's
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
    const RecheckNdF16 fix{p.rows, p.bnorm, p.qfrag, p.qnorm, p.tau0, p.dim_h, IP ? 1 : 0, p.id_offset};
    int kept = sink_bin_wave<RecheckNdF16, true>(p.sink, ((int)blockIdx.y * G + bx) * NW + wave, wbase, lane, fix);
    if (p.sink.stats && wbase > 0) {  // (wave-uniform) one atomic instruction: lane 0 adds the sweep's count, lane 1 the survivors
#pragma unroll
        for (int u = 32; u >= 1; u >>= 1) kept += __shfl_xor(kept, u);
        if (lane < 2) atomicAdd(p.sink.stats + 2 + lane, (unsigned long long)(lane == 0 ? wbase : kept));
    }
}

template <int CBW, bool IP>
static hipError_t launch_ndhf_t(const NdF16FilterParams& p, int grid, int passes, hipStream_t s) {
    constexpr int kLds = ndhf_depth(CBW) * ndhf_slot_bytes(CBW);
    auto kfn = scan_nd_f16f_kernel<CBW, IP>;
    static bool attr_set[64] = {};
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) dev = 0;
    if (!attr_set[dev]) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kfn), hipFuncAttributeMaxDynamicSharedMemorySize, kLds);
        if (e != hipSuccess) return e;
        attr_set[dev] = true;
    }
    hipLaunchKernelGGL(kfn, dim3(grid, passes), dim3(kNdhfWaves * 64), kLds, s, p);
    return hipGetLastError();
}

hipError_t launch_scan_nd_f16f(const NdF16FilterParams& p, const NdFilterPlan& g, hipStream_t s) {
    const int64_t units = (p.n_rows + kNdfUnitRows - 1) / kNdfUnitRows;
    if (p.n_batches < 1 || p.n_batches > 32 || p.dim < 1 || p.dim > kNdMaxDim || p.dim_h != nd_dim_h(p.dim) || p.slabs != p.dim_h / 32 ||
        g.grid < 1 || g.grid > units || g.passes < 1 || g.cbw < 1 || g.cbw > 4 || g.passes * kNdhfWaves * g.cbw < 2 * p.n_batches ||
        (g.passes - 1) * kNdhfWaves * g.cbw >= 2 * p.n_batches || (int64_t)g.grid * g.passes > kSlotStride || p.n_rows > 0x7fffffff - 2 * kNdfUnitRows ||
        p.nq_valid < 1 || p.nq_valid > kMaxBatch || !p.rows || !p.bnorm || !p.qh || !p.qfrag || !p.zero || p.sink.wcap < 1)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(ndf16_prep_kernel, dim3(p.n_batches), dim3(256), 0, s, p);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    const bool ip = p.metric != 0;
    switch (g.cbw) {
    case 1: return ip ? launch_ndhf_t<1, true>(p, g.grid, g.passes, s) : launch_ndhf_t<1, false>(p, g.grid, g.passes, s);
    case 2: return ip ? launch_ndhf_t<2, true>(p, g.grid, g.passes, s) : launch_ndhf_t<2, false>(p, g.grid, g.passes, s);
    case 3: return ip ? launch_ndhf_t<3, true>(p, g.grid, g.passes, s) : launch_ndhf_t<3, false>(p, g.grid, g.passes, s);
    default: return ip ? launch_ndhf_t<4, true>(p, g.grid, g.passes, s) : launch_ndhf_t<4, false>(p, g.grid, g.passes, s);
    }
}

}  // namespace vs
