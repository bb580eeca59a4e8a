// vs_ivf_nd_i8.hip -- the list-major IVF scan of a general index on the byte copy of its rows (vs_ivf_create_nd_u8;
// gfx950).
//
//   ivf_nd_prep_i8  : the launch group's queries as int8 (x - 128), zero padded, row-major [group_q][dim_b]; per query
//                     qterm = sum (q - 128)^2 and valid = 1 when the query runs on bytes; clears the byte plan's counters.
//   ivf_scan_nd_i8_kernel<KCAP> : ivf_scan_nd_kernel's organisation (vs_ivf_nd.hip: a fixed grid of 512-thread workgroups
//                     loops over the item table, the 8 waves take the list's 64-row blocks round-robin, 4 x 1
//                     accumulators per wave) on rows stored as int8, with v_mfma_i32_16x16x64_i8: a wave walks the rows
//                     in 128-byte steps, two MFMAs per tile and step, with a 64-byte tail step when dim_b / 64 is odd.
//                     The rows are the A operand, loaded as scan_nd_i8_kernel loads them (one step ahead, unclamped: the
//                     64 spare rows cover a list's last block); the B operand is gathered -- lane (r, g) reads the 16
//                     bytes at 64 s + 16 g of the byte row of the query in slot r.
//
// Exactness rule (vs_scan_nd_i8.hip), per query: a slot of the list-major scan is one query, so the rule
// that decides per batch in the brute-force byte scan decides per query here.  A query is valid when every value of it
// is an integer in [0, 255] and ||q||^2 + bmax <= 2^24; the fp32 scan's fma(-2, dot, qn + bn) is then the exact integer
// ||q - b||^2 for every row, and so is qterm + rterm - 2 q'.b' in int32 (terms as in vs_scan_nd_i8.hip: every intermediate
// fits).  The plan (vs_ivf_nd.hip) gives the pairs of valid queries slots in the byte plan and every other pair a slot
// in the fp32 plan: a pair has exactly one writer, whichever it is it writes the same bits, and nothing is rerun.
//
// Inner product (IvfNdParams::metric == 1, the IP instantiation): under the same rule every partial sum of q.b is at most
// (||q||^2 + ||b||^2) / 2 <= 2^23, so the fp32 chain is exact in any order and equals the int32 product.  The epilogue
// rebuilds it from the stored bytes, q.b = q'.b' + 128 (sum q' + sum b') + 128^2 dim, with sum q' from ivf_nd_prep_i8
// and sum b' from ivf_nd_i8_rowsum_kernel (built at the index's first inner-product call), and writes -(float)(q.b):
// the fp32 scan's bits, -0.0 for a zero product included.
//
// All loads are ordinary global loads whose waits the compiler places.  The row loads carry no nontemporal hint, as in
// ivf_scan_nd_kernel: a list is read again by every item that probes it.  Measured once with the hint on the byte rows
// (1 M rows, profiles/ivf_nd_u8_bench.txt): the list scan was 3 % slower at 96-d and 9 % slower at 384-d.
#include "vs_kernels.h"
#include "vs_dev.h"
#include "vs_scan_tail.h"

namespace vs {

constexpr int kIvfNd8Tiles = 4;                            // 16-row tiles per wave block
constexpr int kIvfNd8BlockRows = kIvfNd8Tiles * kTileRows;  // 64 <= kScanPadRows: a block never reads past the spare rows
static_assert(kIvfNd8BlockRows <= kScanPadRows, "row blocks are loaded unclamped");
static_assert(kIvfNdSlotBlock == kTileRows, "an item is one MFMA column block");

// grid = ceil(group_q / 32), 256 threads
__global__ __launch_bounds__(256) void ivf_nd_prep_i8(const IvfNdI8Params pb) {
    const IvfNdParams& p = pb.s;
    const int q0 = blockIdx.x * kMaxBatch;
    const int nq = min(kMaxBatch, p.group_q - q0);
    const int dim = p.dim, words = pb.dim_b / 4;
    // a value that is no byte becomes 0 (its query is not valid and its row is never read)
    unsigned* out = reinterpret_cast<unsigned*>(pb.q8rows) + (int64_t)q0 * words;
    for (int e = threadIdx.x; e < nq * words; e += 256) {
        const int qq = e / words, c0 = 4 * (e - qq * words);
        const float* src = p.q + (int64_t)(q0 + qq) * dim;
        unsigned word = 0;
#pragma unroll
        for (int i = 0; i < 4; ++i)
            if (c0 + i < dim) {
                int xi;
                byte_value(src[c0 + i], xi);
                word |= ((unsigned)((xi - 128) & 0xff)) << (8 * i);
            }
        out[e] = word;
    }
    // per query (8 lanes each): qterm = sum (q - 128)^2 and ||q||^2, in integers, and the verdict
    const int row = threadIdx.x >> 3, j = threadIdx.x & 7;
    const bool live = row < nq;
    const float* src = p.q + (int64_t)(q0 + (live ? row : 0)) * dim;
    int t = 0, n2 = 0, bad = 0, s1 = 0;
    if (live) {
        for (int i = j; i < dim; i += 8) {
            int xi;
            if (byte_value(src[i], xi)) {
                t += (xi - 128) * (xi - 128);
                s1 += xi - 128;
                n2 += xi * xi;
            } else {
                bad = 1;
            }
        }
    }
#pragma unroll
    for (int m = 1; m < 8; m <<= 1) {
        t += __shfl_xor(t, m);
        n2 += __shfl_xor(n2, m);
        s1 += __shfl_xor(s1, m);
        bad |= __shfl_xor(bad, m);
    }
    if (j == 0 && live) {
        pb.qterm[q0 + row] = t;
        if (pb.qsum) pb.qsum[q0 + row] = s1;  // (inner product only)
        // (n2 <= 2048 * 255^2, 0 <= bmax < 2^24: no overflow)
        pb.valid[q0 + row] = (!pb.all_f32 && !bad && n2 <= kNd8NormLimit - pb.bmax) ? 1 : 0;
    }
    for (int i = blockIdx.x * 256 + threadIdx.x; i < 2 * p.nlist; i += gridDim.x * 256) p.list_cnt[i] = 0;
}

// IP: the inner-product instantiation -- the same loads and MFMAs; the epilogue rebuilds q.b from the shifted bytes
template <int KCAP, bool IP>
__global__ __launch_bounds__(kScanThreads, 1) void ivf_scan_nd_i8_kernel(const IvfNdI8Params pb) {
    const IvfNdParams& p = pb.s;
    constexpr int T = kIvfNd8Tiles;
    __shared__ NdTailLds tail;

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r = lane & 15, g = lane >> 4;
    const int dim_b = pb.dim_b;
    const unsigned voff = (unsigned)(r * dim_b + 16 * g);  // this lane's 16 bytes inside a 16-row tile's 64-byte step
    const unsigned tile_bytes = 16u * (unsigned)dim_b;     // 16 rows
    const int S = dim_b / 64;    // 64-byte steps per row
    const int n_pairs = S >> 1;  // full 128-byte steps
    const int n_items = p.n_items[0];

#pragma clang loop unroll(disable)
    for (int item = blockIdx.x; item < n_items; item += gridDim.x) {
        const int list = p.items[2 * item], slot0 = p.items[2 * item + 1];
        const int n_slots = min(kIvfNdSlotBlock, p.list_start[list + 1] - slot0);
        const int64_t row_lo = p.offsets[list], row_end = p.offsets[list + 1];
        const int64_t last_row = row_end - 1;
        const int blocks_total = (int)((row_end - row_lo + kIvfNd8BlockRows - 1) / kIvfNd8BlockRows);
        const int sv = p.slots[slot0 + (r < n_slots ? r : 0)];  // (a slot past the run's end repeats the first: discarded below)
        const int qi = sv >> 8;
        int qt;
        if constexpr (IP)
            qt = 128 * pb.qsum[qi] + 16384 * p.dim;  // q.b = q'.b' + 128 (sum q' + sum b') + 128^2 dim
        else
            qt = pb.qterm[qi];
        // this lane's 16 bytes of a 64-byte step of its slot's byte query row
        const char* qb = reinterpret_cast<const char*>(pb.q8rows) + (int64_t)qi * dim_b + 16 * g;
        float wmin = VS_INF, tau = VS_INF;
        float ld[1][KCAP];
        int li[1][KCAP];
#pragma unroll
        for (int j = 0; j < KCAP; ++j) {
            ld[0][j] = VS_INF;
            li[0][j] = -1;
        }

#pragma clang loop unroll(disable)
        for (int wb = wave; wb < blocks_total; wb += kScanWaves) {
            const int64_t row0 = row_lo + (int64_t)wb * kIvfNd8BlockRows;
            const char* sb = reinterpret_cast<const char*>(pb.vecs_u8) + row0 * (int64_t)dim_b;
            i32x4 acc[T];
#pragma unroll
            for (int t = 0; t < T; ++t) acc[t] = (i32x4){0, 0, 0, 0};
            i32x4 a[T][2], b[2];
            auto load_pair = [&](int s, i32x4 (&av)[T][2], i32x4 (&bv)[2]) __attribute__((always_inline)) {
#pragma unroll
                for (int t = 0; t < T; ++t) {
                    av[t][0] = *(reinterpret_cast<const i32x4*>(sb + (t * tile_bytes + 128u * s) + voff));
                    av[t][1] = *(reinterpret_cast<const i32x4*>(sb + (t * tile_bytes + 128u * s + 64u) + voff));
                }
                bv[0] = *reinterpret_cast<const i32x4*>(qb + 128u * s);
                bv[1] = *reinterpret_cast<const i32x4*>(qb + 128u * s + 64u);
            };
            auto mfma_half = [&](const i32x4 (&av)[T][2], const i32x4 (&bv)[2], int u) __attribute__((always_inline)) {
#pragma unroll
                for (int t = 0; t < T; ++t) acc[t] = __builtin_amdgcn_mfma_i32_16x16x64_i8(av[t][u], bv[u], acc[t], 0, 0, 0);
            };
            if (n_pairs > 0) load_pair(0, a, b);
            for (int s = 0; s < n_pairs; ++s) {
                i32x4 an[T][2], bn2[2];
                const bool more = s + 1 < n_pairs;
                if (more) load_pair(s + 1, an, bn2);
                mfma_half(a, b, 0);
                mfma_half(a, b, 1);
                if (more) {
#pragma unroll
                    for (int t = 0; t < T; ++t) {
                        a[t][0] = an[t][0];
                        a[t][1] = an[t][1];
                    }
                    b[0] = bn2[0];
                    b[1] = bn2[1];
                }
            }
            if (S & 1) {  // the last 64 bytes of a row whose dim_b is an odd number of steps
#pragma unroll
                for (int t = 0; t < T; ++t) a[t][0] = *(reinterpret_cast<const i32x4*>(sb + (t * tile_bytes + 128u * n_pairs) + voff));
                b[0] = *reinterpret_cast<const i32x4*>(qb + 128u * n_pairs);
                mfma_half(a, b, 0);
            }
            const bool ragged = row0 + kIvfNd8BlockRows - 1 > last_row;  // wave-uniform
#pragma unroll
            for (int t = 0; t < T; ++t) {
                const int64_t rbase = row0 + 16 * t + 4 * g;
                float d[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    // the integer the fp32 scan computes exactly: ||q||^2 + ||b||^2 - 2 q.b  (the terms have 64 spare entries)
                    if constexpr (IP)  // (|q'.b'| <= 2^25, |128 (sum q' + sum b')| <= 2^26, 128^2 dim <= 2^25; zero gives -0.0)
                        d[j] = -(float)(qt + 128 * pb.rsum[rbase + j] + acc[t][j]);
                    else
                        d[j] = (float)(qt + pb.rterm[rbase + j] - 2 * acc[t][j]);
                    if (ragged && rbase + j > last_row) d[j] = VS_INF;
                }
                nd_topk_step<KCAP>(d, rbase, 0, wmin, tau, ld[0], li[0]);
            }
        }
        const float tq[1] = {VS_INF};
        wg_merge_lists_to<1, KCAP>(tail, p.k, tid, wave, ld, li, tq, [&](int qq, float*& od, int32_t*& oi) {
            if (qq >= n_slots) return false;
            const int s = p.slots[slot0 + qq];
            const int64_t o = ((int64_t)(s >> 8) * p.nprobe + (s & 255)) * KCAP;
            od = p.part_d + o;
            oi = p.part_i + o;
            return true;
        });  // (ends with a barrier)
    }
}

// grid = ceil((rows + 64) / 256), 256 threads: one thread per entry
__global__ __launch_bounds__(256) void ivf_nd_i8_rowsum_kernel(const int8_t* __restrict__ vecs_u8, const int dim_b, const int64_t rows,
                                                               int32_t* __restrict__ rsum) {
    const int64_t row = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (row >= rows + 64) return;
    int t = 0;
    if (row < rows) {
        const i32x4* src = reinterpret_cast<const i32x4*>(vecs_u8 + row * dim_b);  // (dim_b is a multiple of 64)
        for (int c = 0; c < dim_b / 16; ++c) {
            const i32x4 v = src[c];
#pragma unroll
            for (int w = 0; w < 4; ++w)
#pragma unroll
                for (int b = 0; b < 4; ++b) t += (int)(int8_t)((unsigned)v[w] >> (8 * b));
        }
    }
    rsum[row] = t;
}

static bool ivf_nd_i8_params_ok(const IvfNdI8Params& pb) {
    const IvfNdParams& p = pb.s;
    if (p.metric != 0 && p.metric != 1) return false;
    if (p.metric == 1 && (!pb.rsum || !pb.qsum)) return false;
    return p.dim >= 1 && p.dim <= kNdMaxDim && pb.dim_b == nd_dim_b(p.dim) && p.group_q >= 1 && p.group_q <= kIvfNdGroupQ &&
           p.nprobe >= 1 && p.nprobe <= kIvfMaxProbe && p.nlist >= 1 && (p.kcap == 8 || p.kcap == 16) && pb.vecs_u8 && pb.rterm &&
           pb.q8rows && pb.qterm && pb.valid && pb.bmax >= 0 && pb.bmax < kNd8NormLimit;
}

hipError_t launch_ivf_nd_i8_prep(const IvfNdI8Params& pb, hipStream_t s) {
    if (!ivf_nd_i8_params_ok(pb)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(ivf_nd_prep_i8, dim3((pb.s.group_q + kMaxBatch - 1) / kMaxBatch), dim3(256), 0, s, pb);
    return hipGetLastError();
}

hipError_t launch_ivf_nd_i8_scan(const IvfNdI8Params& pb, int grid, hipStream_t s) {
    if (!ivf_nd_i8_params_ok(pb) || grid < 1 || pb.s.k < 1 || pb.s.k > pb.s.kcap) return hipErrorInvalidValue;
    if (pb.s.kcap == 8 && !pb.s.metric)
        hipLaunchKernelGGL((ivf_scan_nd_i8_kernel<8, false>), dim3(grid), dim3(kScanThreads), 0, s, pb);
    else if (!pb.s.metric)
        hipLaunchKernelGGL((ivf_scan_nd_i8_kernel<16, false>), dim3(grid), dim3(kScanThreads), 0, s, pb);
    else if (pb.s.kcap == 8)
        hipLaunchKernelGGL((ivf_scan_nd_i8_kernel<8, true>), dim3(grid), dim3(kScanThreads), 0, s, pb);
    else
        hipLaunchKernelGGL((ivf_scan_nd_i8_kernel<16, true>), dim3(grid), dim3(kScanThreads), 0, s, pb);
    return hipGetLastError();
}

hipError_t launch_ivf_nd_i8_rowsum(const int8_t* vecs_u8, int dim_b, int64_t rows, int32_t* rsum, hipStream_t s) {
    if (!vecs_u8 || !rsum || dim_b < 64 || dim_b % 64 || rows < 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL(ivf_nd_i8_rowsum_kernel, dim3((unsigned)((rows + 64 + 255) / 256)), dim3(256), 0, s, vecs_u8, dim_b, rows, rsum);
    return hipGetLastError();
}

}  // namespace vs
