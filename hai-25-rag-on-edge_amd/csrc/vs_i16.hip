// vs_i16.hip -- the int16 cosine score path of the reference (AMD_npu/), at any vector dimension from 1 to 2048 (gfx950).
//
// What the reference does around its NPU kernel:
//   Codes/preprocess.py:24-42        L2-normalise every base row and every query, multiply by 1000, truncate to int16
//   Codes/test.cpp:32-43, 285-311    the int16 x int16 -> int32 matrix C = A B^T, row-major
// XRT, the xclbin and the AIE tile-major output layout are not restated; the quantiser (contract in vsearch.h, arithmetic
// in vs_i16_quant.h) and the integer score matrix are, exactly.
//
// Layout.  A quantised value is stored as the float16 of the same integer (|q| <= 2047 < 2048: exact), 2 bytes per
// element: rows are [n_rows + 64][dim_b] bytes with dim_b = 2 dim rounded up to 64; padding bytes and the 64 spare rows
// are zero, so tile loads need no clamp and add nothing to a dot product.
//
// Arithmetic.  v_mfma_f32_16x16x32_f16 on those rows: per lane and step the same 16 bytes q8_scores_nd_kernel feeds its
// int8 MFMA.  Every partial sum of q'.b', over any subset of the terms, is an integer of magnitude at most
// ||q'|| ||b'|| <= scale^2 (1 + 2^-20) < 2^23 (Cauchy-Schwarz on the sub-vectors; truncation towards zero only shrinks a
// vector), so an fp32 accumulation is exact in any order: (int)acc is the int32 product and -acc an exact top-k key.
//
// Kernels:
//   i16_quantize_kernel         a workgroup per row.  The leaves of the pairwise sum P (at most 128 elements each, at most
//                               32 of them) are summed by eight lanes each, numpy's eight partial sums; one thread folds
//                               them in the order the split rule fixes.  Base rows go out row-major, queries as the
//                               16-byte B fragments the scans load: fragment (step s, query block h, lane) = the eight
//                               values Q'[16 h + (lane & 15)][32 s + 8 (lane >> 4) ..]; rows past B are zero queries.
//   i16_scores_kernel<NQH>      q8_scores_nd_kernel's walk: a wave owns 64 rows, keeps their 4 x NQH accumulators
//                               resident, 128-byte steps with a 64-byte tail step, rows and fragments loaded one step
//                               ahead; a lane ends with 16 consecutive rows of one query: four 16-byte stores.
//   i16_topk_kernel<NQH, KCAP>  scan_nd_i8_kernel's organisation with the top-k fused in (vs_scan_tail.h: lane lists
//                               under key -acc, threshold exchange, workgroup merge); merge_compact_kernel ranks the
//                               partial lists and i16_finish_kernel turns the keys into int32 scores.  The score matrix is
//                               never written.
//   i16_keys_kernel<NQH>        the walk of i16_scores_kernel (both are i16_walk_kernel) over chosen 64-row groups, float
//                               keys out: the sample and the fallback chunks of the wide-k pipeline
//   i16_filter_kernel<NQH>      i16_topk_kernel's scan without lists: rows under a per-query bound go to candidate lists
//                               (17 <= k <= 128: wide_enqueue, ranked by topk_wide_kernel)
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <memory>
#include <new>
#include <string>
#include <type_traits>
#include <vector>

#include "../../include/vsearch.h"
#include "vs_dev.h"
#include "vs_host.h"
#include "vs_i16_quant.h"
#include "vs_kernels.h"
#include "vs_res.h"
#include "vs_scan_tail.h"

using vs::set_error;

#define HIPCHK(expr)                                                                                   \
    do {                                                                                               \
        hipError_t _e = (expr);                                                                        \
        if (_e != hipSuccess) {                                                                        \
            set_error(std::string(#expr) + ": " + hipGetErrorString(_e));                              \
            return VS_ERR_DEVICE;                                                                      \
        }                                                                                              \
    } while (0)

namespace {

using vs::f32x4;
using vs::i32x4;
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));

constexpr int kBatch = 32;
constexpr int kGroup = 16;       // batches one quantiser launch and one fused scan launch serve
constexpr int kGroupRows = 64;   // rows a wave scores per step
constexpr int kMaxK = 16;
constexpr int kWideMaxK = 128;             // vs_i16_search_topk*
constexpr int kWideCap = 8192;             // candidates kept per query
constexpr int64_t kWideChunk = 1 << 20;    // rows per chunk of the dense fallback
constexpr int kPadRows = vs::kScanPadRows;
static_assert(kGroupRows <= kPadRows, "row groups are loaded unclamped");

inline int i16_dim_b(int dim) { return (2 * dim + 63) / 64 * 64; }

__device__ __forceinline__ f32x4 mfma_f16(i32x4 a, i32x4 b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
}

// B == 0: grid = rows, src [rows][dim] -> dst [rows][dim_b] bytes.  B >= 1: grid = n_batches * 32 (batch, row of the
// batch), src [n_batches * B][dim] -> dst [n_batches][dim_b / 64][2][64] 16-byte fragments.
__global__ __launch_bounds__(256) void i16_quantize_kernel(const float* __restrict__ src, int B, int dim, int dim_b, float scale,
                                                           i32x4* __restrict__ dst) {
    __shared__ int s_off[vs::kI16MaxLeaves], s_n[vs::kI16MaxLeaves], s_depth[vs::kI16MaxLeaves];
    __shared__ float s_sum[vs::kI16MaxLeaves];
    __shared__ int st_off[16], st_n[16], st_d[16];  // the walk's pending runs / the fold's pending sums (depth <= 6)
    __shared__ float st_sum[16];
    __shared__ int s_leaves;
    __shared__ float s_den;
    const int tid = threadIdx.x;
    const int pieces = dim_b / 16;  // 16-byte pieces of eight values
    const bool frag = B > 0;
    const int nb = blockIdx.x >> 5, qi = blockIdx.x & 31;
    const int64_t row = frag ? (int64_t)nb * B + qi : (int64_t)blockIdx.x;
    const float* x = src + row * dim;  // (read only for a real row)
    i32x4* out = frag ? dst + (int64_t)nb * (dim_b / 64) * 128 : dst + (int64_t)blockIdx.x * pieces;
    auto slot_of = [&](int p) { return frag ? ((p >> 2) * 2 + (qi >> 4)) * 64 + 16 * (p & 3) + (qi & 15) : p; };
    if (frag && qi >= B) {  // (workgroup-uniform) a zero query
        for (int p = tid; p < pieces; p += 256) out[slot_of(p)] = (i32x4){0, 0, 0, 0};
        return;
    }
    if (tid == 0) {  // the leaves of P(s, dim), left to right, with their depth in the tree
        int top = 1, nl = 0;
        st_off[0] = 0, st_n[0] = dim, st_d[0] = 0;
        while (top > 0) {
            --top;
            const int off = st_off[top], n = st_n[top], d = st_d[top];
            if (n <= vs::kI16Leaf) {
                s_off[nl] = off, s_n[nl] = n, s_depth[nl] = d;
                ++nl;
            } else {
                const int n2 = vs::i16_split(n);
                st_off[top] = off + n2, st_n[top] = n - n2, st_d[top] = d + 1;
                ++top;
                st_off[top] = off, st_n[top] = n2, st_d[top] = d + 1;
                ++top;
            }
        }
        s_leaves = nl;
    }
    __syncthreads();
    {  // leaf `leaf` on lanes 8 leaf .. 8 leaf + 7: lane j keeps numpy's partial sum r_j
        const int leaf = tid >> 3, j = tid & 7;
        const bool has = leaf < s_leaves;
        const int off = has ? s_off[leaf] : 0, n = has ? s_n[leaf] : 0;
        float xv[vs::kI16Leaf / 8];  // the lane's values, fetched together: one memory round trip, not one per step
#pragma unroll
        for (int u = 0; u < vs::kI16Leaf / 8; ++u) xv[u] = 8 * u + 8 <= n ? x[off + 8 * u + j] : 0.f;
        float r = vs::i16_mul(xv[0], xv[0]);
#pragma unroll
        for (int u = 1; u < vs::kI16Leaf / 8; ++u)
            if (8 * u + 8 <= n) r = vs::i16_add(r, vs::i16_mul(xv[u], xv[u]));
        r = vs::i16_add(r, __shfl_xor(r, 1));  // (r0+r1), (r2+r3), ...
        r = vs::i16_add(r, __shfl_xor(r, 2));  // ((r0+r1)+(r2+r3)), ...
        r = vs::i16_add(r, __shfl_xor(r, 4));
        if (has && j == 0) {
            float res = n >= 8 ? r : 0.f;
            for (int i = n >= 8 ? (n & ~7) : 0; i < n; ++i) res = vs::i16_add(res, vs::i16_mul(x[off + i], x[off + i]));
            s_sum[leaf] = res;
        }
    }
    __syncthreads();
    if (tid == 0) {  // two pending sums of the same depth are the halves of one run
        int top = 0;
        for (int l = 0; l < s_leaves; ++l) {
            float v = s_sum[l];
            int d = s_depth[l];
            while (top > 0 && st_d[top - 1] == d) {
                v = vs::i16_add(st_sum[top - 1], v);
                --d;
                --top;
            }
            st_sum[top] = v, st_d[top] = d;
            ++top;
        }
        s_den = vs::i16_den(st_sum[0]);
    }
    __syncthreads();
    const float den = s_den;
    for (int p = tid; p < pieces; p += 256) {
        i32x4 v;
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            unsigned word = 0;
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const int k = 8 * p + 2 * w + i;
                const int q = k < dim ? vs::i16_quant1(x[k], den, scale) : 0;
                word |= (unsigned)__builtin_bit_cast(unsigned short, (_Float16)(float)q) << (16 * i);
            }
            v[w] = (int)word;
        }
        out[slot_of(p)] = v;
    }
}

// Which 64-row groups a score walk visits: all of them (the score matrix: column = row) ...
struct AllGroups {
    __device__ __forceinline__ bool idle() const { return false; }
    __device__ __forceinline__ int64_t group(int64_t j) const { return j; }
    __device__ __forceinline__ int64_t column(int64_t, int64_t row) const { return row; }
};
// ... or the groups first + j stride (a sample, a chunk), and nothing at all unless *run_if != 0 when run_if is given
struct SomeGroups {
    int64_t first, stride;
    const int32_t* run_if;
    __device__ __forceinline__ bool idle() const { return run_if && !run_if[0]; }
    __device__ __forceinline__ int64_t group(int64_t j) const { return first + j * stride; }
    __device__ __forceinline__ int64_t column(int64_t j, int64_t row) const { return row - (group(j) - j) * kGroupRows; }
};

// rows: [n_pad][dim_b] bytes, n_pad a multiple of 64 inside the image.  The j-th group visited, j < n_groups, goes to
// columns 64 j .. of out ([B][ld]): Out = int32_t the scores (i16_scores_kernel), Out = float the top-k keys -(q'.b')
// (i16_keys_kernel)
template <int NQH, class Out, class Groups>
__global__ __launch_bounds__(256) void i16_walk_kernel(const char* __restrict__ rows, const i32x4* __restrict__ qf, int dim_b,
                                                       int64_t n_rows, int64_t n_groups, int B, Out* __restrict__ out, int64_t ld,
                                                       int aligned, const Groups groups) {
    constexpr int T = 4;  // 16-row tiles of a wave's 64 rows
    constexpr bool KEYS = std::is_floating_point<Out>::value;
    if (groups.idle()) return;
    const int lane = threadIdx.x & 63, g = lane >> 4, c = lane & 15;
    const int64_t wave0 = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6), waves = (int64_t)gridDim.x * 4;
    const int S = dim_b / 64;    // 64-byte steps per row
    const int n_pairs = S >> 1;  // full 128-byte lines
    // MFMA row m of tile t <- row 16*(m/4) + 4*t + (m%4), as in q8_scores_kernel: over the four tiles the C fragments of
    // lane group g hold the 16 consecutive rows 16g .. 16g+15
    const unsigned voff = (unsigned)((16 * (c >> 2) + (c & 3)) * dim_b + 16 * g);
    const unsigned tile_bytes = 4u * (unsigned)dim_b;
    for (int64_t grp = wave0; grp < n_groups; grp += waves) {
        const int64_t row0 = groups.group(grp) * kGroupRows;
        const char* sb = rows + row0 * (int64_t)dim_b;  // uniform base + 32-bit lane offset
        f32x4 acc[T][NQH];
#pragma unroll
        for (int t = 0; t < T; ++t)
#pragma unroll
            for (int h = 0; h < NQH; ++h) acc[t][h] = (f32x4){0.f, 0.f, 0.f, 0.f};
        i32x4 a[T][2], b[NQH][2];
        auto load_a = [&](int s, i32x4 (&av)[T][2]) __attribute__((always_inline)) {
#pragma unroll
            for (int t = 0; t < T; ++t) {
                av[t][0] = *reinterpret_cast<const i32x4*>(sb + (t * tile_bytes + 128u * s) + voff);
                av[t][1] = *reinterpret_cast<const i32x4*>(sb + (t * tile_bytes + 128u * s + 64u) + voff);
            }
        };
        auto load_b = [&](int s, i32x4 (&bv)[NQH][2]) __attribute__((always_inline)) {
#pragma unroll
            for (int h = 0; h < NQH; ++h) {
                bv[h][0] = qf[((2 * s) * 2 + h) * 64 + lane];
                bv[h][1] = qf[((2 * s + 1) * 2 + h) * 64 + lane];
            }
        };
        auto mfma_half = [&](const i32x4 (&av)[T][2], const i32x4 (&bv)[NQH][2], int u) __attribute__((always_inline)) {
#pragma unroll
            for (int t = 0; t < T; ++t)
#pragma unroll
                for (int h = 0; h < NQH; ++h) acc[t][h] = mfma_f16(av[t][u], bv[h][u], acc[t][h]);
        };
        if (n_pairs > 0) {
            load_a(0, a);
            load_b(0, b);
        }
        for (int s = 0; s < n_pairs; ++s) {
            i32x4 an[T][2], bn[NQH][2];
            const bool more = s + 1 < n_pairs;
            if (more) {
                load_a(s + 1, an);
                load_b(s + 1, bn);
            }
            mfma_half(a, b, 0);
            mfma_half(a, b, 1);
            if (more) {
#pragma unroll
                for (int t = 0; t < T; ++t) {
                    a[t][0] = an[t][0];
                    a[t][1] = an[t][1];
                }
#pragma unroll
                for (int h = 0; h < NQH; ++h) {
                    b[h][0] = bn[h][0];
                    b[h][1] = bn[h][1];
                }
            }
        }
        if (S & 1) {  // the last 64 bytes of a row whose dim_b is an odd number of steps
#pragma unroll
            for (int t = 0; t < T; ++t) a[t][0] = *reinterpret_cast<const i32x4*>(sb + (t * tile_bytes + 128u * n_pairs) + voff);
#pragma unroll
            for (int h = 0; h < NQH; ++h) b[h][0] = qf[((2 * n_pairs) * 2 + h) * 64 + lane];
            mfma_half(a, b, 0);
        }
#pragma unroll
        for (int h = 0; h < NQH; ++h) {
            const int qi = 16 * h + c;
            if (qi >= B) continue;
#pragma unroll
            for (int t = 0; t < T; ++t) {
                const int64_t r = row0 + 16 * g + 4 * t;  // accumulator i of tile t: row r + i
                if (r >= n_rows) continue;
                Out* dst = out + (size_t)qi * ld + groups.column(grp, r);
                typedef Out Out4 __attribute__((ext_vector_type(4)));
                Out4 word;  // exact: see above
                if constexpr (KEYS) word = -acc[t][h];
                else word = (Out4){(int)acc[t][h][0], (int)acc[t][h][1], (int)acc[t][h][2], (int)acc[t][h][3]};
                if (aligned && r + 4 <= n_rows) {
                    *reinterpret_cast<Out4*>(dst) = word;
                } else {
#pragma unroll
                    for (int i = 0; i < 4; ++i)
                        if (r + i < n_rows) dst[i] = word[i];
                }
            }
        }
    }
}

template <int NQH>
constexpr auto i16_scores_kernel = i16_walk_kernel<NQH, int32_t, AllGroups>;
template <int NQH>
constexpr auto i16_keys_kernel = i16_walk_kernel<NQH, float, SomeGroups>;

struct TopkParams {
    const char* rows;      // [n_rows + 64][dim_b] bytes
    const i32x4* qfrag;    // [n_batches][dim_b / 64][2][64]
    int dim_b;
    int64_t n_rows;
    int n_batches;
    float* slots;          // [n_batches][32][kSlotStride] (pre-set to +inf) or nullptr = no exchange
    int k1;
    int32_t id_offset;
    float* part_d;         // [n_batches][32][kSlotStride][KCAP]
    int32_t* part_i;
};

// the organisation of scan_nd_i8_kernel (vs_scan_nd_i8.hip); key of a row = -(q'.b'), smallest first
template <int NQH, int KCAP>
__global__ __launch_bounds__(vs::kScanThreads, 1) void i16_topk_kernel(const TopkParams p) {
    using namespace vs;
    constexpr int T = 4;
    constexpr int kBlockRows = T * kTileRows;  // 64
    // the fragments of a step are loaded one step ahead like its rows, except in the largest instantiation (two query
    // blocks, 16-entry lists), which has no registers left for the second set
    constexpr bool BAHEAD = NQH * KCAP < 32;
    __shared__ NdTailLds tail;
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r = lane & 15, g = lane >> 4;
    const int dim_b = p.dim_b;
    const unsigned voff = (unsigned)(r * dim_b + 16 * g);  // this lane's 16 bytes inside a 16-row tile's 64-byte step
    const int S = dim_b / 64;
    const int n_pairs = S >> 1;
    const int64_t last_row = p.n_rows - 1;
    const int blocks_total = (int)((p.n_rows + kBlockRows - 1) / kBlockRows);
    const int wb0 = blockIdx.x * kScanWaves + wave;
    const int wb_step = gridDim.x * kScanWaves;

#pragma clang loop unroll(disable)
    for (int batch = 0; batch < p.n_batches; ++batch) {
        const i32x4* qf_b = p.qfrag + (int64_t)batch * S * 128;
        float* slots = p.slots ? p.slots + (int64_t)batch * 32 * kSlotStride : nullptr;
        float tau[NQH], tq[NQH], wmin[NQH];
        float ld[NQH][KCAP];
        int li[NQH][KCAP];
#pragma unroll
        for (int h = 0; h < NQH; ++h) {
            tau[h] = tq[h] = VS_INF;
            wmin[h] = VS_INF;
#pragma unroll
            for (int j = 0; j < KCAP; ++j) {
                ld[h][j] = VS_INF;
                li[h][j] = -1;
            }
        }

        auto do_block = [&](int wb) __attribute__((always_inline)) {
            const int64_t row0 = (int64_t)wb * kBlockRows;
            const char* sb = p.rows + row0 * (int64_t)dim_b;
            const unsigned tile_bytes = 16u * (unsigned)dim_b;
            f32x4 acc[T][NQH];
#pragma unroll
            for (int t = 0; t < T; ++t)
#pragma unroll
                for (int h = 0; h < NQH; ++h) acc[t][h] = (f32x4){0.f, 0.f, 0.f, 0.f};
            i32x4 a[T][2], b[NQH][2];
            auto load_a = [&](int s, i32x4 (&av)[T][2]) __attribute__((always_inline)) {
#pragma unroll
                for (int t = 0; t < T; ++t) {
                    av[t][0] = __builtin_nontemporal_load(reinterpret_cast<const i32x4*>(sb + (t * tile_bytes + 128u * s) + voff));
                    av[t][1] = __builtin_nontemporal_load(reinterpret_cast<const i32x4*>(sb + (t * tile_bytes + 128u * s + 64u) + voff));
                }
            };
            auto load_b = [&](int s, i32x4 (&bv)[NQH][2]) __attribute__((always_inline)) {
#pragma unroll
                for (int h = 0; h < NQH; ++h) {
                    bv[h][0] = qf_b[((2 * s) * 2 + h) * 64 + lane];
                    bv[h][1] = qf_b[((2 * s + 1) * 2 + h) * 64 + lane];
                }
            };
            auto mfma_half = [&](const i32x4 (&av)[T][2], const i32x4 (&bv)[NQH][2], int u) __attribute__((always_inline)) {
#pragma unroll
                for (int t = 0; t < T; ++t)
#pragma unroll
                    for (int h = 0; h < NQH; ++h) acc[t][h] = mfma_f16(av[t][u], bv[h][u], acc[t][h]);
            };
            if (n_pairs > 0) {
                load_a(0, a);
                if (BAHEAD) load_b(0, b);
            }
            for (int s = 0; s < n_pairs; ++s) {
                i32x4 an[T][2], bn2[NQH][2];
                const bool more = s + 1 < n_pairs;
                if (!BAHEAD) load_b(s, b);  // (issued before the rows of the next step: its wait leaves those in flight)
                if (more) {
                    load_a(s + 1, an);
                    if (BAHEAD) load_b(s + 1, bn2);
                }
                mfma_half(a, b, 0);
                mfma_half(a, b, 1);
                if (more) {
#pragma unroll
                    for (int t = 0; t < T; ++t) {
                        a[t][0] = an[t][0];
                        a[t][1] = an[t][1];
                    }
                    if (BAHEAD) {
#pragma unroll
                        for (int h = 0; h < NQH; ++h) {
                            b[h][0] = bn2[h][0];
                            b[h][1] = bn2[h][1];
                        }
                    }
                }
            }
            if (S & 1) {
#pragma unroll
                for (int t = 0; t < T; ++t)
                    a[t][0] = __builtin_nontemporal_load(reinterpret_cast<const i32x4*>(sb + (t * tile_bytes + 128u * n_pairs) + voff));
#pragma unroll
                for (int h = 0; h < NQH; ++h) b[h][0] = qf_b[((2 * n_pairs) * 2 + h) * 64 + lane];
                mfma_half(a, b, 0);
            }
            const bool ragged = row0 + kBlockRows - 1 > last_row;  // wave-uniform
#pragma unroll
            for (int t = 0; t < T; ++t) {
                const int64_t rbase = row0 + 16 * t + 4 * g;
#pragma unroll
                for (int h = 0; h < NQH; ++h) {
                    float d[4];
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        d[j] = -acc[t][h][j];  // exact (a zero product gives -0.0, which compares equal to 0.0)
                        if (ragged && rbase + j > last_row) d[j] = VS_INF;
                    }
                    nd_topk_step<KCAP>(d, rbase, p.id_offset, wmin[h], tau[h], ld[h], li[h]);
                }
            }
        };

        bool xchg = slots != nullptr;  // (workgroup-uniform)
        for (int wb = wb0; wb < blocks_total || xchg; wb += wb_step) {
            if (wb < blocks_total) do_block(wb);
            if (xchg) {
                xchg = false;
                xchg_bound<NQH>(tail, slots, p.k1, tid, wave, wmin, tq, tau);  // (after the first block: vs_scan_tail.h)
            }
        }
        // partial lists are query-major, [batch][query][workgroup][KCAP]: one merge launch ranks all batches
        wg_merge_lists_to<NQH, KCAP>(tail, p.k1, tid, wave, ld, li, tq, [&](int qq, float*& od, int32_t*& oi) {
            const int64_t o = (((int64_t)batch * kMaxBatch + qq) * kSlotStride + blockIdx.x) * KCAP;
            od = p.part_d + o;
            oi = p.part_i + o;
            return true;
        });  // (ends with a barrier)
    }
}

// the merge's keys -> scores, in place: -(q'.b') as float becomes the int32 product, an empty slot INT32_MIN
__global__ __launch_bounds__(256) void i16_finish_kernel(int32_t* __restrict__ scores, int n) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float d = __builtin_bit_cast(float, scores[i]);
    scores[i] = d < VS_INF ? (int)(-d) : (int)0x80000000;
}

// ---- wide k (17 <= k <= 128): the filter scan of wide_enqueue below
struct FilterParams {
    const char* rows;      // [n_rows + 64][dim_b] bytes
    const i32x4* qfrag;    // [n_batches][dim_b / 64][2][64]
    int dim_b;
    int64_t n_rows;
    int n_batches;
    const float* tau;      // [n_batches][32]: a row is a candidate of the query when its key is below this bound
    int32_t* cnt;          // [n_batches][32] candidates counted (zero on entry; keeps counting past cap)
    float* cand_d;         // [n_batches][32][cap] keys
    int32_t* cand_i;       //                      rows
    int cap;
};

// i16_topk_kernel's scan (512 threads, 64-row blocks dealt round-robin, non-temporal row loads and the query fragments one
// step ahead, the batch loop inside) without its lists: a block's epilogue compares the 16 x NQH keys of a lane with the
// bound of the lane's query, leaves when no lane of the wave has a key under its bound, and otherwise reserves the
// lane's places in the query's candidate list with one atomicAdd per query block.  No LDS, no exchange, no merge.
template <int NQH>
__global__ __launch_bounds__(vs::kScanThreads, 1) void i16_filter_kernel(const FilterParams p) {
    using namespace vs;
    constexpr int T = 4;
    constexpr int kBlockRows = T * kTileRows;  // 64
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r = lane & 15, g = lane >> 4;
    const int dim_b = p.dim_b;
    const unsigned voff = (unsigned)(r * dim_b + 16 * g);  // this lane's 16 bytes inside a 16-row tile's 64-byte step
    const int S = dim_b / 64;
    const int n_pairs = S >> 1;
    const int64_t last_row = p.n_rows - 1;
    const int blocks_total = (int)((p.n_rows + kBlockRows - 1) / kBlockRows);
    const int wb0 = blockIdx.x * kScanWaves + wave;
    const int wb_step = gridDim.x * kScanWaves;

#pragma clang loop unroll(disable)
    for (int batch = 0; batch < p.n_batches; ++batch) {
        const i32x4* qf_b = p.qfrag + (int64_t)batch * S * 128;
        // Keys are integers: key < tau <=> key < ceil(tau).  tau is next_up of an integer-valued key (+0 for a zero
        // product, whose next_up is the smallest denormal: named by its bits, so that no denormal is ever compared) or
        // an infinity (-inf: a padding query, nothing passes).
        float thr[NQH];
#pragma unroll
        for (int h = 0; h < NQH; ++h) {
            const float t = p.tau[batch * kMaxBatch + 16 * h + r];
            thr[h] = __builtin_bit_cast(int, t) == 1 ? 1.0f : ceilf(t);
        }
        for (int wb = wb0; wb < blocks_total; wb += wb_step) {
            const int64_t row0 = (int64_t)wb * kBlockRows;
            const char* sb = p.rows + row0 * (int64_t)dim_b;
            const unsigned tile_bytes = 16u * (unsigned)dim_b;
            f32x4 acc[T][NQH];
#pragma unroll
            for (int t = 0; t < T; ++t)
#pragma unroll
                for (int h = 0; h < NQH; ++h) acc[t][h] = (f32x4){0.f, 0.f, 0.f, 0.f};
            i32x4 a[T][2], b[NQH][2];
            auto load_a = [&](int s, i32x4 (&av)[T][2]) __attribute__((always_inline)) {
#pragma unroll
                for (int t = 0; t < T; ++t) {
                    av[t][0] = __builtin_nontemporal_load(reinterpret_cast<const i32x4*>(sb + (t * tile_bytes + 128u * s) + voff));
                    av[t][1] = __builtin_nontemporal_load(reinterpret_cast<const i32x4*>(sb + (t * tile_bytes + 128u * s + 64u) + voff));
                }
            };
            auto load_b = [&](int s, i32x4 (&bv)[NQH][2]) __attribute__((always_inline)) {
#pragma unroll
                for (int h = 0; h < NQH; ++h) {
                    bv[h][0] = qf_b[((2 * s) * 2 + h) * 64 + lane];
                    bv[h][1] = qf_b[((2 * s + 1) * 2 + h) * 64 + lane];
                }
            };
            auto mfma_half = [&](const i32x4 (&av)[T][2], const i32x4 (&bv)[NQH][2], int u) __attribute__((always_inline)) {
#pragma unroll
                for (int t = 0; t < T; ++t)
#pragma unroll
                    for (int h = 0; h < NQH; ++h) acc[t][h] = mfma_f16(av[t][u], bv[h][u], acc[t][h]);
            };
            if (n_pairs > 0) {
                load_a(0, a);
                load_b(0, b);
            }
            for (int s = 0; s < n_pairs; ++s) {
                i32x4 an[T][2], bn2[NQH][2];
                const bool more = s + 1 < n_pairs;
                if (more) {
                    load_a(s + 1, an);
                    load_b(s + 1, bn2);
                }
                mfma_half(a, b, 0);
                mfma_half(a, b, 1);
                if (more) {
#pragma unroll
                    for (int t = 0; t < T; ++t) {
                        a[t][0] = an[t][0];
                        a[t][1] = an[t][1];
                    }
#pragma unroll
                    for (int h = 0; h < NQH; ++h) {
                        b[h][0] = bn2[h][0];
                        b[h][1] = bn2[h][1];
                    }
                }
            }
            if (S & 1) {
#pragma unroll
                for (int t = 0; t < T; ++t)
                    a[t][0] = __builtin_nontemporal_load(reinterpret_cast<const i32x4*>(sb + (t * tile_bytes + 128u * n_pairs) + voff));
#pragma unroll
                for (int h = 0; h < NQH; ++h) b[h][0] = qf_b[((2 * n_pairs) * 2 + h) * 64 + lane];
                mfma_half(a, b, 0);
            }
            // accumulator j of tile t: row row0 + 16 t + 4 g + j, query 16 h + r; bit 4 t + j of mask[h] = a candidate
            const bool ragged = row0 + kBlockRows - 1 > last_row;  // wave-uniform
            unsigned mask[NQH], hit = 0;
#pragma unroll
            for (int h = 0; h < NQH; ++h) {
                mask[h] = 0;
#pragma unroll
                for (int t = 0; t < T; ++t)
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        bool ok = -acc[t][h][j] < thr[h];  // exact (a zero product gives -0.0, which compares equal to 0.0)
                        if (ragged && row0 + 16 * t + 4 * g + j > last_row) ok = false;
                        mask[h] |= (unsigned)ok << (4 * t + j);
                    }
                hit |= mask[h];
            }
            if (__builtin_amdgcn_ballot_w64(hit != 0) == 0) continue;  // wave-uniform: the common case
#pragma unroll
            for (int h = 0; h < NQH; ++h) {
                if (!mask[h]) continue;
                const int q = batch * kMaxBatch + 16 * h + r;
                int pos = atomicAdd(p.cnt + q, __builtin_popcount(mask[h]));
                float* cd = p.cand_d + (int64_t)q * p.cap;
                int32_t* ci = p.cand_i + (int64_t)q * p.cap;
#pragma unroll
                for (int t = 0; t < T; ++t)
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        if ((mask[h] >> (4 * t + j)) & 1) {
                            if (pos < p.cap) {
                                cd[pos] = -acc[t][h][j];
                                ci[pos] = (int32_t)(row0 + 16 * t + 4 * g + j);
                            }
                            ++pos;
                        }
            }
        }
    }
}

// One workgroup after a group's ranking launch.  st[0] += queries ranked from their lists, st[1] = max(st[1], candidates
// of any query), st[2] += queries of the batches whose overflow word is set (the dense fallback answers those).
__global__ __launch_bounds__(512) void i16_wide_stats_kernel(const int32_t* __restrict__ cnt, const int32_t* __restrict__ ovf, int nb, int B,
                                                             unsigned long long* __restrict__ st) {
    __shared__ int s_max, s_list, s_dense;
    const int tid = threadIdx.x, batch = tid >> 5, qi = tid & 31;
    if (tid == 0) s_max = s_list = s_dense = 0;
    __syncthreads();
    if (batch < nb && qi < B) {
        atomicMax(&s_max, cnt[tid]);
        atomicAdd(ovf[batch] ? &s_dense : &s_list, 1);
    }
    __syncthreads();
    if (tid == 0) {
        st[0] += (unsigned long long)s_list;
        st[1] = st[1] > (unsigned long long)s_max ? st[1] : (unsigned long long)s_max;
        st[2] += (unsigned long long)s_dense;
    }
}

}  // namespace

struct vs_i16 {
    int device = 0;
    int dim = 0, dim_b = 0;  // vector length; row bytes (2 dim rounded up to 64)
    int64_t n_rows = 0, n_pad = 0;
    int32_t id_offset = 0;
    float scale = 0;
    int num_cus = 256;
    vs::DevBuf<char> d_rows;        // [n_rows + 64][dim_b]
    vs::DevBuf<i32x4> d_qfrag;      // [kGroup][dim_b / 64][2][64] quantised queries as fragments
    vs::DevBuf<float> d_q;          // [kGroup * 32][dim] staging of host queries
    vs::DevBuf<int32_t> d_scores;   // [32][n_pad] the blocking call's score matrix (allocated by its first use)
    vs::DevBuf<float> d_slots;      // [kGroup][32][kSlotStride]
    vs::DevBuf<float> d_part_d;     // [kGroup][32][kSlotStride][16]
    vs::DevBuf<int32_t> d_part_i;
    vs::DevBuf<int32_t> d_ids;      // [kGroup * 32][16]
    vs::DevBuf<int32_t> d_top;      // [kGroup * 32][16]
    // wide k (17..128, wide_enqueue), allocated by the first such call
    struct Wide {
        bool ready = false;
        int64_t ld = 0;                  // columns of keys: the largest sample (k = 128) or a fallback chunk, whichever is longer
        int64_t chunk = 0;               // rows per fallback chunk (a multiple of 64)
        int n_chunks = 0;
        int64_t whole = 0;               // queries whose sample was the whole base (counted on the host)
        vs::DevBuf<float> keys;          // [32][ld] keys of one batch's sample, later of a fallback chunk
        vs::DevBuf<float> tau;           // [kGroup][32]
        vs::DevBuf<float> pre_d;         // [32][128] the sample's best (only its bound is used)
        vs::DevBuf<int32_t> pre_i;
        vs::DevBuf<int32_t> cz;          // [kGroup * 32] candidate counts, [kGroup] overflow words: cleared by the bound launch
        vs::DevBuf<float> cand_d;        // [kGroup][32][kWideCap]
        vs::DevBuf<int32_t> cand_i;
        vs::DevBuf<float> ch_d;          // [32][n_chunks][128] the fallback's chunk lists
        vs::DevBuf<int32_t> ch_i;
        vs::DevBuf<unsigned long long> stats;  // [3] (i16_wide_stats_kernel)
        vs::DevBuf<int32_t> ids, top;    // [kGroup * 32][128] the host call's outputs
    } wide;
    vs::Stream stream;
};

namespace {

template <class F>
int guarded(F&& f) {
    try {
        return f();
    } catch (const std::bad_alloc&) {
        set_error("out of host memory");
        return VS_ERR_NOMEM;
    } catch (const std::exception& e) {
        set_error(std::string("internal error: ") + e.what());
        return VS_ERR_INVALID;
    }
}

int quantize_enqueue(const float* src, int64_t blocks, int B, int dim, int dim_b, float scale, i32x4* dst, hipStream_t s) {
    hipLaunchKernelGGL(i16_quantize_kernel, dim3((unsigned)blocks), dim3(256), 0, s, src, B, dim, dim_b, scale, dst);
    HIPCHK(hipGetLastError());
    return VS_OK;
}

int create_impl(const float* base_host, int64_t n_rows, int dim, float scale, int device, int64_t id_offset, vs_i16** out) {
    if (!out || !base_host || n_rows <= 0) {
        set_error("vs_i16_create: bad arguments");
        return VS_ERR_INVALID;
    }
    if (dim < 1) {
        set_error("vs_i16_create: dim must be at least 1");
        return VS_ERR_INVALID;
    }
    if (dim > vs::kI16MaxDim) {
        set_error("vs_i16_create: dim > 2048 is not supported");
        return VS_ERR_UNSUPPORTED;
    }
    if (n_rows + id_offset > 0x7fffffffLL || id_offset < 0) {
        set_error("ids must fit int32");
        return VS_ERR_UNSUPPORTED;
    }
    if (!(scale >= 1.0f && scale <= 2047.0f)) {  // (a NaN fails both comparisons)
        set_error("vs_i16_create: scale must be finite and in [1, 2047]");
        return VS_ERR_INVALID;
    }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
        set_error("no HIP device available (this library has no CPU fallback)");
        return VS_ERR_DEVICE;
    }
    if (device < 0 || device >= ndev) {
        set_error("device index out of range");
        return VS_ERR_INVALID;
    }
    HIPCHK(hipSetDevice(device));
    std::unique_ptr<vs_i16> h(new (std::nothrow) vs_i16());  // (released, with what it holds, on every early return)
    if (!h) {
        set_error("out of host memory");
        return VS_ERR_NOMEM;
    }
    h->device = device;
    h->dim = dim;
    h->dim_b = i16_dim_b(dim);
    h->n_rows = n_rows;
    h->n_pad = (n_rows + kGroupRows - 1) / kGroupRows * kGroupRows;
    h->id_offset = (int32_t)id_offset;
    h->scale = scale;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) == hipSuccess && prop.multiProcessorCount > 0) h->num_cus = prop.multiProcessorCount;
    const int dim_b = h->dim_b;
    int rc;
    if ((rc = h->d_rows.alloc((size_t)(n_rows + kPadRows) * dim_b))) return rc;
    if ((rc = h->d_qfrag.alloc((size_t)kGroup * (dim_b / 64) * 128))) return rc;
    if ((rc = h->d_q.alloc((size_t)kGroup * kBatch * dim))) return rc;
    if ((rc = h->d_slots.alloc((size_t)kGroup * kBatch * vs::kSlotStride))) return rc;
    if ((rc = h->d_part_d.alloc((size_t)kGroup * kBatch * vs::kSlotStride * kMaxK))) return rc;
    if ((rc = h->d_part_i.alloc((size_t)kGroup * kBatch * vs::kSlotStride * kMaxK))) return rc;
    if ((rc = h->d_ids.alloc((size_t)kGroup * kBatch * kMaxK))) return rc;
    if ((rc = h->d_top.alloc((size_t)kGroup * kBatch * kMaxK))) return rc;
    if ((rc = h->stream.create())) return rc;
    // float rows in chunks of 64 MB through one staging buffer, quantised by the kernel that quantises the queries
    const int64_t chunk = std::max<int64_t>(1, std::min<int64_t>(n_rows, ((int64_t)64 << 20) / ((int64_t)dim * 4)));
    vs::DevBuf<float> stage;
    if ((rc = stage.alloc((size_t)chunk * dim))) return rc;
    HIPCHK(hipMemsetAsync(h->d_rows + (size_t)n_rows * dim_b, 0, (size_t)kPadRows * dim_b, h->stream));
    for (int64_t r0 = 0; r0 < n_rows; r0 += chunk) {
        const int64_t rows = std::min(chunk, n_rows - r0);
        // (stream order: the copy waits for the kernel that still reads the staging buffer)
        HIPCHK(hipMemcpyAsync(stage, base_host + (size_t)r0 * dim, (size_t)rows * dim * 4, hipMemcpyHostToDevice, h->stream));
        if ((rc = quantize_enqueue(stage, rows, 0, dim, dim_b, scale, reinterpret_cast<i32x4*>(h->d_rows + (size_t)r0 * dim_b), h->stream)))
            return rc;
    }
    HIPCHK(hipStreamSynchronize(h->stream));
    *out = h.release();
    return VS_OK;
}

int execute_enqueue(vs_i16* h, const float* q_dev, int B, int32_t* scores_dev, int64_t ld, hipStream_t s) {
    int rc = quantize_enqueue(q_dev, kBatch, B, h->dim, h->dim_b, h->scale, h->d_qfrag, s);
    if (rc) return rc;
    const int64_t n_groups = h->n_pad / kGroupRows;
    // 3 workgroups = 12 waves per CU, as q8_scores_nd_kernel; a wave strides over the groups
    const int grid = (int)std::max<int64_t>(1, std::min<int64_t>((n_groups + 3) / 4, (int64_t)h->num_cus * 3));
    const int aligned = (ld % 4 == 0) && (reinterpret_cast<uintptr_t>(scores_dev) % 16 == 0);
    if (B <= 16)
        hipLaunchKernelGGL(i16_scores_kernel<1>, dim3(grid), dim3(256), 0, s, h->d_rows.get(), h->d_qfrag.get(), h->dim_b, h->n_rows, n_groups, B,
                           scores_dev, ld, aligned, AllGroups{});
    else
        hipLaunchKernelGGL(i16_scores_kernel<2>, dim3(grid), dim3(256), 0, s, h->d_rows.get(), h->d_qfrag.get(), h->dim_b, h->n_rows, n_groups, B,
                           scores_dev, ld, aligned, AllGroups{});
    HIPCHK(hipGetLastError());
    return VS_OK;
}

template <int NQH, int KCAP>
void topk_launch(const TopkParams& p, int grid, hipStream_t s) {
    hipLaunchKernelGGL((i16_topk_kernel<NQH, KCAP>), dim3(grid), dim3(vs::kScanThreads), 0, s, p);
}

// nb <= kGroup batches of B queries: quantiser, fused scan, merge, finish -- four launches and at most one fill
int search_enqueue(vs_i16* h, const float* q_dev, int nb, int B, int k, int32_t* ids_dev, int32_t* scores_dev, hipStream_t s) {
    int rc = quantize_enqueue(q_dev, (int64_t)nb * kBatch, B, h->dim, h->dim_b, h->scale, h->d_qfrag, s);
    if (rc) return rc;
    const int kcap = k <= 8 ? 8 : 16;
    const int64_t blocks = h->n_pad / kGroupRows;
    const int grid = (int)std::max<int64_t>(1, std::min<int64_t>((blocks + vs::kScanWaves - 1) / vs::kScanWaves, std::min(h->num_cus, vs::kSlotStride)));
    // the exchange pays once every wave has a few blocks left after its first one; without it every lane list goes
    // through the workgroup merge (small indexes)
    const bool exchange = grid >= 16 && blocks >= (int64_t)grid * vs::kScanWaves * 4;
    TopkParams p{};
    p.rows = h->d_rows;
    p.qfrag = h->d_qfrag;
    p.dim_b = h->dim_b;
    p.n_rows = h->n_rows;
    p.n_batches = nb;
    p.k1 = k;
    p.id_offset = h->id_offset;
    p.part_d = h->d_part_d;
    p.part_i = h->d_part_i;
    if (exchange) {
        // 0x7f800000 = +inf
        HIPCHK(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(h->d_slots.get()), 0x7f800000, (size_t)nb * kBatch * vs::kSlotStride, s));
        p.slots = h->d_slots;
    }
    if (kcap == 8) B <= 16 ? topk_launch<1, 8>(p, grid, s) : topk_launch<2, 8>(p, grid, s);
    else B <= 16 ? topk_launch<1, 16>(p, grid, s) : topk_launch<2, 16>(p, grid, s);
    HIPCHK(hipGetLastError());
    vs::MergeParams m{};
    m.nq = nb * B;
    m.kout = k;
    m.out_d = reinterpret_cast<float*>(scores_dev);  // keys first; i16_finish_kernel turns them into scores in place
    m.out_i = ids_dev;
    m.q_group_out = B;
    m.q_group_in = vs::kMaxBatch;
    m.part_d = h->d_part_d;
    m.part_i = h->d_part_i;
    m.G = grid;
    m.kin = kcap;
    HIPCHK(vs::launch_merge_layout(m, kcap, (int64_t)vs::kSlotStride * kcap, s));
    const int n = nb * B * k;
    hipLaunchKernelGGL(i16_finish_kernel, dim3((n + 255) / 256), dim3(256), 0, s, scores_dev, n);
    HIPCHK(hipGetLastError());
    return VS_OK;
}

int check_k(int k) {
    if (k > kMaxK) {
        set_error("k too large for the compiled top-k kernels (k <= 16)");
        return VS_ERR_UNSUPPORTED;
    }
    return VS_OK;
}

// ---- wide k (17 <= k <= 128), per launch group of nb <= kGroup batches, every step stream-ordered:
//   quantiser; per batch the keys of the strided sample (i16_keys_kernel) and its k best (topk_wide_kernel, dense form):
//   bound tau = next_up(k-th smallest sample key); one filter scan over ALL rows for the whole group (i16_filter_kernel:
//   every key under its query's bound goes to the query's candidate list, counted past the cap); one ranking launch over
//   the lists (topk_wide_kernel, list form, grp_out = B); i16_finish_kernel.  Exact: a row that is not listed has a key
//   >= tau, and the k sample rows under tau are listed and are ahead of it.  A list that overflows raises its batch's
//   overflow word, and the dense fallback enqueued behind the ranking under that word (keys of row chunks, a selection
//   per chunk, a selection over the chunk lists) rewrites the batch.  When the sample is the whole base the bound launch
//   writes the final lists (column = row) and nothing else runs.
// The sampling rule is the header's (vs_i16_wide_plan).
void wide_plan(int64_t n_rows, int k, int64_t& sample_groups, int64_t& stride) {
    const int64_t n_groups = (n_rows + kGroupRows - 1) / kGroupRows;
    const int64_t share = (n_rows / 2048) * k + ((n_rows % 2048) * k + 2047) / 2048;  // ceil(n_rows k / 2048)
    const int64_t l0 = std::max<int64_t>((int64_t)kGroupRows * k, share);
    sample_groups = std::min(n_groups, (l0 + kGroupRows - 1) / kGroupRows);
    stride = n_groups / sample_groups;
}

int ensure_wide(vs_i16* h, hipStream_t s) {
    if (h->wide.ready) return VS_OK;
    vs_i16::Wide w;
    int64_t sg, stride;
    wide_plan(h->n_rows, kWideMaxK, sg, stride);
    w.chunk = std::min(h->n_pad, kWideChunk);
    w.n_chunks = (int)((h->n_pad + w.chunk - 1) / w.chunk);
    w.ld = std::max(sg * kGroupRows, w.chunk);
    const size_t q = (size_t)kGroup * kBatch;
    int rc;
    if ((rc = w.keys.alloc((size_t)kBatch * w.ld)) || (rc = w.tau.alloc(q)) || (rc = w.pre_d.alloc((size_t)kBatch * kWideMaxK)) ||
        (rc = w.pre_i.alloc((size_t)kBatch * kWideMaxK)) || (rc = w.cz.alloc(q + kGroup)) || (rc = w.cand_d.alloc(q * kWideCap)) ||
        (rc = w.cand_i.alloc(q * kWideCap)) || (rc = w.ch_d.alloc((size_t)kBatch * w.n_chunks * kWideMaxK)) ||
        (rc = w.ch_i.alloc((size_t)kBatch * w.n_chunks * kWideMaxK)) || (rc = w.stats.alloc(3)) || (rc = w.ids.alloc(q * kWideMaxK)) ||
        (rc = w.top.alloc(q * kWideMaxK)))
        return rc;
    HIPCHK(hipMemsetAsync(w.stats, 0, 3 * sizeof(unsigned long long), s));
    w.ready = true;
    h->wide = std::move(w);
    return VS_OK;
}

// keys of the groups first + j stride, j < count, of one batch (fragments qf) -> W.keys
int keys_enqueue(vs_i16* h, const i32x4* qf, int64_t first, int64_t stride, int64_t count, int B, const int32_t* run_if, hipStream_t s) {
    const int grid = (int)std::max<int64_t>(1, std::min<int64_t>((count + 3) / 4, (int64_t)h->num_cus * 3));
    const SomeGroups groups{first, stride, run_if};
    if (B <= 16)
        hipLaunchKernelGGL(i16_keys_kernel<1>, dim3(grid), dim3(256), 0, s, h->d_rows.get(), qf, h->dim_b, h->n_rows, count, B, h->wide.keys.get(),
                           h->wide.ld, 1, groups);
    else
        hipLaunchKernelGGL(i16_keys_kernel<2>, dim3(grid), dim3(256), 0, s, h->d_rows.get(), qf, h->dim_b, h->n_rows, count, B, h->wide.keys.get(),
                           h->wide.ld, 1, groups);
    HIPCHK(hipGetLastError());
    return VS_OK;
}

int wide_enqueue(vs_i16* h, const float* q_dev, int nb, int B, int k, int32_t* ids_dev, int32_t* scores_dev, hipStream_t s) {
    vs_i16::Wide& W = h->wide;
    int rc = quantize_enqueue(q_dev, (int64_t)nb * kBatch, B, h->dim, h->dim_b, h->scale, h->d_qfrag, s);
    if (rc) return rc;
    int64_t sg, stride;
    wide_plan(h->n_rows, k, sg, stride);
    const int64_t n = h->n_rows, n_groups = h->n_pad / kGroupRows;
    const bool whole = sg == n_groups;
    const size_t frag_b = (size_t)(h->dim_b / 64) * 128;  // fragments of a batch
    float* const keys_out = reinterpret_cast<float*>(scores_dev);  // keys first; i16_finish_kernel turns them into scores in place
    int32_t* const cnt = W.cz;
    int32_t* const ovf = W.cz + kGroup * kBatch;
    for (int b = 0; b < nb; ++b) {
        if ((rc = keys_enqueue(h, h->d_qfrag + b * frag_b, 0, stride, sg, B, nullptr, s))) return rc;
        vs::TopkWideParams t{};
        t.dense = W.keys;
        t.dense_ld = W.ld;
        t.nq = B;
        t.k1 = k;
        if (whole) {  // column = row: the final lists
            t.n_dense = n;
            t.dense_id0 = h->id_offset;
            t.out_d = keys_out + (size_t)b * B * k;
            t.out_i = ids_dev + (size_t)b * B * k;
            t.out_ld = k;
            HIPCHK(vs::launch_topk_wide(t, B, s));
            continue;
        }
        t.n_dense = sg * kGroupRows;  // full groups (vsearch.h); the ids of this selection are sample columns and unused
        t.out_d = W.pre_d;
        t.out_i = W.pre_i;
        t.out_ld = kWideMaxK;
        t.tau_out = W.tau + b * kBatch;  // padding queries: -inf
        if (b == 0) {  // counts and overflow words of the group, cleared in stream order behind the previous call's use
            t.zero = W.cz;
            t.zero_words = kGroup * kBatch + kGroup;
        }
        HIPCHK(vs::launch_topk_wide(t, kBatch, s));
    }
    if (whole) {
        W.whole += (int64_t)nb * B;
    } else {
        FilterParams f{};
        f.rows = h->d_rows;
        f.qfrag = h->d_qfrag;
        f.dim_b = h->dim_b;
        f.n_rows = n;
        f.n_batches = nb;
        f.tau = W.tau;
        f.cnt = cnt;
        f.cand_d = W.cand_d;
        f.cand_i = W.cand_i;
        f.cap = kWideCap;
        const int grid = (int)std::max<int64_t>(1, std::min<int64_t>((n_groups + vs::kScanWaves - 1) / vs::kScanWaves, h->num_cus));
        if (B <= 16) hipLaunchKernelGGL(i16_filter_kernel<1>, dim3(grid), dim3(vs::kScanThreads), 0, s, f);
        else hipLaunchKernelGGL(i16_filter_kernel<2>, dim3(grid), dim3(vs::kScanThreads), 0, s, f);
        HIPCHK(hipGetLastError());
        vs::TopkWideParams r{};
        r.list[0] = {W.cand_d, W.cand_i, kWideCap, cnt, kWideCap, h->id_offset};
        r.n_list = 1;
        r.nq = nb * B;
        r.k1 = k;
        r.out_d = keys_out;
        r.out_i = ids_dev;
        r.out_ld = k;
        r.overflow = ovf;
        r.grp_out = B;
        r.grp_in = kBatch;
        HIPCHK(vs::launch_topk_wide(r, nb * B, s));
        hipLaunchKernelGGL(i16_wide_stats_kernel, dim3(1), dim3(512), 0, s, cnt, ovf, nb, B, W.stats.get());
        HIPCHK(hipGetLastError());
        // dense fallback of a batch, idle unless one of its lists overflowed
        for (int b = 0; b < nb; ++b) {
            float* const od = keys_out + (size_t)b * B * k;
            int32_t* const oi = ids_dev + (size_t)b * B * k;
            const int nc = W.n_chunks;
            for (int c = 0; c < nc; ++c) {
                const int64_t r0 = (int64_t)c * W.chunk, rows = std::min(W.chunk, n - r0);
                if ((rc = keys_enqueue(h, h->d_qfrag + b * frag_b, r0 / kGroupRows, 1, (rows + kGroupRows - 1) / kGroupRows, B, ovf + b, s)))
                    return rc;
                vs::TopkWideParams d{};
                d.dense = W.keys;
                d.dense_ld = W.ld;
                d.n_dense = rows;
                d.dense_id0 = (int32_t)(h->id_offset + r0);
                d.nq = B;
                d.k1 = k;
                d.run_if = ovf + b;
                if (nc == 1) {
                    d.out_d = od;
                    d.out_i = oi;
                    d.out_ld = k;
                } else {
                    d.out_d = W.ch_d + (size_t)c * k;
                    d.out_i = W.ch_i + (size_t)c * k;
                    d.out_ld = (int64_t)nc * k;
                }
                HIPCHK(vs::launch_topk_wide(d, B, s));
            }
            if (nc > 1) {
                vs::TopkWideParams m{};
                m.list[0] = {W.ch_d, W.ch_i, (int64_t)nc * k, nullptr, nc * k, 0};
                m.n_list = 1;
                m.nq = B;
                m.k1 = k;
                m.out_d = od;
                m.out_i = oi;
                m.out_ld = k;
                m.run_if = ovf + b;
                HIPCHK(vs::launch_topk_wide(m, B, s));
            }
        }
    }
    const int n_out = nb * B * k;
    hipLaunchKernelGGL(i16_finish_kernel, dim3((n_out + 255) / 256), dim3(256), 0, s, scores_dev, n_out);
    HIPCHK(hipGetLastError());
    return VS_OK;
}

int check_wide_k(int k) {
    if (k > kWideMaxK) {
        set_error("k too large for the wide top-k pipeline (k <= 128)");
        return VS_ERR_UNSUPPORTED;
    }
    return VS_OK;
}

}  // namespace

extern "C" {

int vs_i16_create(const float* base_host, int64_t n_rows, int dim, float scale, int device, int64_t id_offset, vs_i16** out) {
    return guarded([&]() -> int { return create_impl(base_host, n_rows, dim, scale, device, id_offset, out); });
}

void vs_i16_destroy(vs_i16* h) {
    if (!h) return;
    (void)hipSetDevice(h->device);
    (void)hipDeviceSynchronize();  // (the handles release without waiting for queued work)
    delete h;
}

int64_t vs_i16_num_docs(const vs_i16* h) { return h ? h->n_rows : 0; }
int vs_i16_dim(const vs_i16* h) { return h ? h->dim : 0; }
int vs_i16_batch(const vs_i16* h) { return h ? kBatch : 0; }
float vs_i16_scale(const vs_i16* h) { return h ? h->scale : 0.0f; }

int vs_i16_rows_read(vs_i16* h, int64_t row0, int64_t n, int16_t* dst) {
    if (!h || !dst || row0 < 0 || n < 0 || row0 > h->n_rows || n > h->n_rows - row0) {
        set_error("vs_i16_rows_read: bad arguments (the range must lie inside the index)");
        return VS_ERR_INVALID;
    }
    return guarded([&]() -> int {
        HIPCHK(hipSetDevice(h->device));
        const int64_t chunk = std::max<int64_t>(1, ((int64_t)16 << 20) / h->dim_b);
        std::vector<uint16_t> buf((size_t)std::min(chunk, std::max<int64_t>(n, 1)) * (h->dim_b / 2));
        for (int64_t r0 = 0; r0 < n; r0 += chunk) {
            const int64_t rows = std::min(chunk, n - r0);
            HIPCHK(hipMemcpy(buf.data(), h->d_rows + (size_t)(row0 + r0) * h->dim_b, (size_t)rows * h->dim_b, hipMemcpyDeviceToHost));
            for (int64_t i = 0; i < rows; ++i)
                for (int t = 0; t < h->dim; ++t)
                    dst[(size_t)(r0 + i) * h->dim + t] = (int16_t)vs::i16_from_f16_bits(buf[(size_t)i * (h->dim_b / 2) + t]);
        }
        return VS_OK;
    });
}

int vs_i16_execute_dev(vs_i16* h, const float* queries_dev, int B, int32_t* scores_dev, int64_t ld, void* stream) {
    if (!h || !queries_dev || !scores_dev || B < 1 || B > kBatch || ld < h->n_rows) {
        set_error("vs_i16_execute_dev: bad arguments (1 <= B <= 32, ld >= rows)");
        return VS_ERR_INVALID;
    }
    HIPCHK(hipSetDevice(h->device));
    return execute_enqueue(h, queries_dev, B, scores_dev, ld, static_cast<hipStream_t>(stream));
}

int vs_i16_execute(vs_i16* h, const float* queries_host, int B, int32_t* scores_host) {
    if (!h || !queries_host || !scores_host || B < 1 || B > kBatch) {
        set_error("vs_i16_execute: bad arguments (1 <= B <= 32)");
        return VS_ERR_INVALID;
    }
    HIPCHK(hipSetDevice(h->device));
    int rc = h->d_scores.reserve((size_t)kBatch * h->n_pad);
    if (rc) return rc;
    HIPCHK(hipMemcpyAsync(h->d_q, queries_host, (size_t)B * h->dim * 4, hipMemcpyHostToDevice, h->stream));
    if ((rc = execute_enqueue(h, h->d_q, B, h->d_scores, h->n_pad, h->stream))) return rc;
    HIPCHK(hipMemcpy2DAsync(scores_host, (size_t)h->n_rows * 4, h->d_scores, (size_t)h->n_pad * 4, (size_t)h->n_rows * 4, (size_t)B,
                            hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return VS_OK;
}

int vs_i16_search_dev(vs_i16* h, const float* queries_dev, int n_batches, int B, int k, int32_t* ids_dev, int32_t* scores_dev, void* stream) {
    if (!h || !queries_dev || !ids_dev || !scores_dev || n_batches < 1 || B < 1 || B > kBatch || k < 1) {
        set_error("vs_i16_search_dev: bad arguments");
        return VS_ERR_INVALID;
    }
    int rc = check_k(k);
    if (rc) return rc;
    HIPCHK(hipSetDevice(h->device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    for (int g0 = 0; g0 < n_batches; g0 += kGroup) {
        const int gs = std::min(kGroup, n_batches - g0);
        const size_t o = (size_t)g0 * B * k;
        if ((rc = search_enqueue(h, queries_dev + (size_t)g0 * B * h->dim, gs, B, k, ids_dev + o, scores_dev + o, s))) return rc;
    }
    return VS_OK;
}

int vs_i16_search(vs_i16* h, const float* queries_host, int64_t nq, int k, int32_t* ids, int32_t* scores) {
    if (!h || !queries_host || !ids || !scores || nq < 0 || k < 1) {
        set_error("vs_i16_search: bad arguments");
        return VS_ERR_INVALID;
    }
    int rc = check_k(k);
    if (rc) return rc;
    HIPCHK(hipSetDevice(h->device));
    for (int64_t q0 = 0; q0 < nq;) {  // groups of full batches of 32, then the short last batch
        const int64_t left = nq - q0;
        const int nb = left >= kBatch ? (int)std::min<int64_t>(kGroup, left / kBatch) : 1;
        const int B = left >= kBatch ? kBatch : (int)left;
        const size_t n = (size_t)nb * B;
        HIPCHK(hipMemcpyAsync(h->d_q, queries_host + (size_t)q0 * h->dim, n * h->dim * 4, hipMemcpyHostToDevice, h->stream));
        if ((rc = search_enqueue(h, h->d_q, nb, B, k, h->d_ids, h->d_top, h->stream))) return rc;
        HIPCHK(hipMemcpyAsync(ids + (size_t)q0 * k, h->d_ids, n * k * 4, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(hipMemcpyAsync(scores + (size_t)q0 * k, h->d_top, n * k * 4, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(hipStreamSynchronize(h->stream));
        q0 += (int64_t)n;
    }
    return VS_OK;
}

int vs_i16_search_topk_dev(vs_i16* h, const float* queries_dev, int n_batches, int B, int k, int32_t* ids_dev, int32_t* scores_dev,
                           void* stream) {
    if (!h || !queries_dev || !ids_dev || !scores_dev || n_batches < 1 || B < 1 || B > kBatch || k < 1) {
        set_error("vs_i16_search_topk_dev: bad arguments");
        return VS_ERR_INVALID;
    }
    int rc = check_wide_k(k);
    if (rc) return rc;
    if (k <= kMaxK) return vs_i16_search_dev(h, queries_dev, n_batches, B, k, ids_dev, scores_dev, stream);
    HIPCHK(hipSetDevice(h->device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    if ((rc = ensure_wide(h, s))) return rc;
    for (int g0 = 0; g0 < n_batches; g0 += kGroup) {
        const int gs = std::min(kGroup, n_batches - g0);
        const size_t o = (size_t)g0 * B * k;
        if ((rc = wide_enqueue(h, queries_dev + (size_t)g0 * B * h->dim, gs, B, k, ids_dev + o, scores_dev + o, s))) return rc;
    }
    return VS_OK;
}

int vs_i16_search_topk(vs_i16* h, const float* queries_host, int64_t nq, int k, int32_t* ids, int32_t* scores) {
    if (!h || !queries_host || !ids || !scores || nq < 0 || k < 1) {
        set_error("vs_i16_search_topk: bad arguments");
        return VS_ERR_INVALID;
    }
    int rc = check_wide_k(k);
    if (rc) return rc;
    if (k <= kMaxK) return vs_i16_search(h, queries_host, nq, k, ids, scores);
    HIPCHK(hipSetDevice(h->device));
    if ((rc = ensure_wide(h, h->stream))) return rc;
    for (int64_t q0 = 0; q0 < nq;) {  // groups of full batches of 32, then the short last batch
        const int64_t left = nq - q0;
        const int nb = left >= kBatch ? (int)std::min<int64_t>(kGroup, left / kBatch) : 1;
        const int B = left >= kBatch ? kBatch : (int)left;
        const size_t n = (size_t)nb * B;
        HIPCHK(hipMemcpyAsync(h->d_q, queries_host + (size_t)q0 * h->dim, n * h->dim * 4, hipMemcpyHostToDevice, h->stream));
        if ((rc = wide_enqueue(h, h->d_q, nb, B, k, h->wide.ids, h->wide.top, h->stream))) return rc;
        HIPCHK(hipMemcpyAsync(ids + (size_t)q0 * k, h->wide.ids, n * k * 4, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(hipMemcpyAsync(scores + (size_t)q0 * k, h->wide.top, n * k * 4, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(hipStreamSynchronize(h->stream));
        q0 += (int64_t)n;
    }
    return VS_OK;
}

int vs_i16_wide_plan(int64_t n_rows, int k, int64_t* out) {
    if (!out || n_rows < 1 || k <= kMaxK || k > kWideMaxK) {
        set_error("vs_i16_wide_plan: bad arguments (n_rows >= 1, 17 <= k <= 128)");
        return VS_ERR_INVALID;
    }
    wide_plan(n_rows, k, out[0], out[1]);
    out[2] = kWideCap;
    return VS_OK;
}

int vs_i16_wide_stats(vs_i16* h, int64_t* out, int reset) {
    if (!h || !out) {
        set_error("vs_i16_wide_stats: bad arguments");
        return VS_ERR_INVALID;
    }
    out[0] = out[1] = out[2] = out[3] = 0;
    if (!h->wide.ready) return VS_OK;  // no wide call yet
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipDeviceSynchronize());
    unsigned long long st[3];
    HIPCHK(hipMemcpy(st, h->wide.stats, sizeof(st), hipMemcpyDeviceToHost));
    for (int i = 0; i < 3; ++i) out[i] = (int64_t)st[i];
    out[3] = h->wide.whole;
    if (reset) {
        HIPCHK(hipMemset(h->wide.stats, 0, sizeof(st)));
        HIPCHK(hipDeviceSynchronize());
        h->wide.whole = 0;
    }
    return VS_OK;
}

}  // extern "C"
