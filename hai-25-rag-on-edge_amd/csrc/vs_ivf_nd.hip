// vs_ivf_nd.hip -- the list-major IVF scan of a general index, 1 <= dim <= 2048, fp32 rows, squared L2 or inner product
// (gfx950).
//
//   ivf_nd_prep     : the launch group's queries zero-padded row-major [group_q][dim_p] and their squared norms in
//                     nd_prep_kernel's summation order; clears the plan's counters.
//   ivf_nd_count    : one thread per (query, probe rank) pair: pairs per list, rows per pair (total_candidates), and the
//                     pair's partial list preset to (+inf, -1).  An index with a byte copy of its rows
//                     (vs_ivf_create_nd_u8) keeps two plans per group and routes every query to one of them
//                     (IvfNdParams::route); its second plan's count leaves the preset and the candidates alone.
//   ivf_nd_prefix   : one workgroup: prefix of the pair counts over the lists -> the first slot of every list's run, and
//                     the item table -- (list, first slot) for every 16 slots of a probed list that holds rows.
//   ivf_nd_fill     : one thread per pair: the pair's slot (query << 8 | rank) into its list's run.  The order inside a
//                     run comes from an atomic; nothing depends on it (see the kernel contract below).
//   ivf_scan_nd_kernel<KCAP> : a fixed grid of 512-thread workgroups loops over the item table.  Per item the 8 waves
//                     take the list's 64-row blocks round-robin; a wave keeps 4 x 1 accumulators (four 16-row tiles
//                     against the item's 16 slots) and walks K as scan_nd_kernel does.  The rows are the A operand,
//                     loaded as scan_nd_kernel loads them (one step ahead, unclamped: a list may start at any row, the
//                     spare rows cover its last block); the B operand is gathered -- lane (r, g) reads 16 bytes of the
//                     padded row of the query in slot r.  A lane keeps a sorted list per slot; the workgroup merge of
//                     vs_scan_tail.h takes the 32 lane lists of a slot to the item's top-KCAP by (distance, row).
//
// Kernel contract: the accumulation chain of a (row, query) distance is scan_nd_kernel's -- the same order of s, u and
// i and the same lane-to-k mapping, then fma(-2, dot, qn + bn) -- so a distance is bit-identical to what the brute-force
// general scan returns for the pair, whichever item, slot or wave computed it.  Under inner product (IvfNdParams::metric,
// the IP instantiation) the score is the same chain negated, -(q.v), as the brute-force general scan returns it under
// VS_METRIC_IP.  Slots past the run's end in a list's last item repeat the item's first slot; their results are discarded.
//
// All loads are ordinary global loads whose waits the compiler places.  The row loads carry no nontemporal
// hint, unlike scan_nd_kernel's: a list is read again by every item that probes it, and with the hint the pipeline was
// 9 to 11 % slower (384-d, 1 M rows, profiles/ivf_nd_bench.txt).
#include "vs_kernels.h"
#include "vs_dev.h"
#include "vs_scan_tail.h"

namespace vs {

constexpr int kIvfNdTiles = 4;                           // 16-row tiles per wave block
constexpr int kIvfNdBlockRows = kIvfNdTiles * kTileRows;  // 64 <= kScanPadRows: a block never reads past the spare rows
static_assert(kIvfNdBlockRows <= kScanPadRows, "row blocks are loaded unclamped");
static_assert(kIvfNdSlotBlock == kTileRows, "an item is one MFMA column block");
static_assert(kIvfMaxProbe <= 256, "a slot keeps the probe rank in 8 bits");

// grid = ceil(group_q / 32), 256 threads
__global__ __launch_bounds__(256) void ivf_nd_prep(const IvfNdParams p) {
    const int q0 = blockIdx.x * kMaxBatch;
    const int nq = min(kMaxBatch, p.group_q - q0);
    const int dim = p.dim, dim_p = p.dim_p;
    for (int e = threadIdx.x; e < nq * dim_p; e += 256) {
        const int qq = e / dim_p, c = e - qq * dim_p;
        p.qrows[(int64_t)(q0 + qq) * dim_p + c] = c < dim ? p.q[(int64_t)(q0 + qq) * dim + c] : 0.f;
    }
    // squared norms: 8 FMA lanes, r0 + ... + r7, then the tail (nd_prep_kernel's order)
    const int row = threadIdx.x >> 3, j = threadIdx.x & 7;
    const bool live = row < nq;
    const float* src = p.q + (int64_t)(q0 + (live ? row : 0)) * dim;
    float acc = 0.f;
    const int d8 = dim & ~7;
    for (int i = 0; i < d8; i += 8) {
        const float x = src[i + j];
        acc = fmaf(x, x, acc);
    }
    const int b8 = (threadIdx.x & 63) & ~7;
    float sum = __shfl(acc, b8);
#pragma unroll
    for (int u = 1; u < 8; ++u) sum = sum + __shfl(acc, b8 + u);
    for (int i = d8; i < dim; ++i) sum = fmaf(src[i], src[i], sum);
    if (j == 0 && live) p.qnorm[q0 + row] = sum;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < 2 * p.nlist; i += gridDim.x * 256) p.list_cnt[i] = 0;
}

// the list a pair probes, or -1 when it yields no slot in this plan (no probe, a list without rows, a query routed to
// the group's other plan, or a pair the rescan's mask leaves out); rows = the probed list's length either way
__device__ __forceinline__ int ivf_nd_pair_list(const IvfNdParams& p, int pair, int& rows) {
    const int c = p.probes[pair];
    rows = (c >= 0 && c < p.nlist) ? p.offsets[c + 1] - p.offsets[c] : 0;
    if (rows <= 0) return -1;
    if (p.route && p.route[pair / p.nprobe] != p.route_want) return -1;
    if (p.pair_mask && !p.pair_mask[pair]) return -1;
    return c;
}

// grid = ceil(group_q * nprobe / 256), 256 threads.  first: the group's first (or only) plan, which also presets the
// partial lists and counts the candidates
__global__ __launch_bounds__(256) void ivf_nd_count(const IvfNdParams p, const int first) {
    const int pair = blockIdx.x * 256 + threadIdx.x;
    int rows = 0, got = 0;
    if (pair < p.group_q * p.nprobe) {
        const int c = ivf_nd_pair_list(p, pair, rows);
        if (c >= 0) {
            atomicAdd(p.list_cnt + c, 1);
            got = 1;
        }
        if (first)
            for (int j = 0; j < p.kcap; ++j) {
                p.part_d[(int64_t)pair * p.kcap + j] = VS_INF;
                p.part_i[(int64_t)pair * p.kcap + j] = -1;
            }
    }
    if (first && p.cand_count) {
        unsigned long long t = (unsigned long long)rows;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) t += __shfl_xor(t, o);
        if ((threadIdx.x & 63) == 0 && t) atomicAdd(p.cand_count, t);
    }
    if (p.pair_count) {
        int t = got;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) t += __shfl_xor(t, o);
        if ((threadIdx.x & 63) == 0 && t) atomicAdd(p.pair_count, (unsigned long long)t);
    }
}

// one workgroup of 1024 threads: thread t owns lists [t * per, (t + 1) * per)
__global__ __launch_bounds__(1024) void ivf_nd_prefix(const IvfNdParams p) {
    __shared__ int s_slots[1024], s_items[1024];
    const int tid = threadIdx.x;
    const int per = (p.nlist + 1023) / 1024;
    const int lo = min(tid * per, p.nlist), hi = min(lo + per, p.nlist);
    int ns = 0, ni = 0;
    for (int c = lo; c < hi; ++c) {
        const int n = p.list_cnt[c];
        ns += n;
        ni += (n + kIvfNdSlotBlock - 1) / kIvfNdSlotBlock;
    }
    s_slots[tid] = ns;
    s_items[tid] = ni;
    __syncthreads();
    for (int o = 1; o < 1024; o <<= 1) {  // inclusive scan
        const int as = tid >= o ? s_slots[tid - o] : 0, ai = tid >= o ? s_items[tid - o] : 0;
        __syncthreads();
        s_slots[tid] += as;
        s_items[tid] += ai;
        __syncthreads();
    }
    int slot = s_slots[tid] - ns, item = s_items[tid] - ni;
    for (int c = lo; c < hi; ++c) {
        const int n = p.list_cnt[c];
        p.list_start[c] = slot;
        for (int b = 0; b < n; b += kIvfNdSlotBlock, ++item) {
            p.items[2 * item] = c;
            p.items[2 * item + 1] = slot + b;
        }
        slot += n;
    }
    if (tid == 1023) {
        p.list_start[p.nlist] = s_slots[1023];
        p.n_items[0] = s_items[1023];
    }
}

// grid = ceil(group_q * nprobe / 256), 256 threads
__global__ __launch_bounds__(256) void ivf_nd_fill(const IvfNdParams p) {
    const int pair = blockIdx.x * 256 + threadIdx.x;
    if (pair >= p.group_q * p.nprobe) return;
    int rows;
    const int c = ivf_nd_pair_list(p, pair, rows);
    if (c < 0) return;
    const int q = pair / p.nprobe, rank = pair - q * p.nprobe;
    const int pos = p.list_start[c] + atomicAdd(p.list_cnt + p.nlist + c, 1);
    p.slots[pos] = q << 8 | rank;
}

// IP: the inner-product instantiation -- the same loads and chain, the epilogue is d = -acc and no norm is loaded
template <int KCAP, bool IP>
__global__ __launch_bounds__(kScanThreads, 1) void ivf_scan_nd_kernel(const IvfNdParams p) {
    constexpr int T = kIvfNdTiles;
    __shared__ NdTailLds tail;

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r = lane & 15, g = lane >> 4;
    const int dim_p = p.dim_p;
    const unsigned voff = (unsigned)(r * dim_p + 4 * g) * 4u;  // this lane's 16 bytes inside a 16-row tile's segment
    const unsigned tile_bytes = 64u * (unsigned)dim_p;         // 16 rows
    const int C = dim_p / 16;    // 64-byte segments per row
    const int n_pairs = C >> 1;  // full 32-float steps
    const int n_items = p.n_items[0];

#pragma clang loop unroll(disable)
    for (int item = blockIdx.x; item < n_items; item += gridDim.x) {
        const int list = p.items[2 * item], slot0 = p.items[2 * item + 1];
        const int n_slots = min(kIvfNdSlotBlock, p.list_start[list + 1] - slot0);
        const int64_t row_lo = p.offsets[list], row_end = p.offsets[list + 1];
        const int64_t last_row = row_end - 1;
        const int blocks_total = (int)((row_end - row_lo + kIvfNdBlockRows - 1) / kIvfNdBlockRows);
        const int sv = p.slots[slot0 + (r < n_slots ? r : 0)];  // (a slot past the run's end repeats the first: discarded below)
        const int qi = sv >> 8;
        float qn = 0.f;
        if constexpr (!IP) qn = p.qnorm[qi];
        // this lane's 16 bytes of a 64-byte segment of its slot's padded query row
        const char* qb = reinterpret_cast<const char*>(p.qrows + (int64_t)qi * dim_p + 4 * g);
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
            const int64_t row0 = row_lo + (int64_t)wb * kIvfNdBlockRows;
            const char* sb = reinterpret_cast<const char*>(p.vecs + row0 * (int64_t)dim_p);
            f32x4 acc[T];
#pragma unroll
            for (int t = 0; t < T; ++t) acc[t] = (f32x4){0.f, 0.f, 0.f, 0.f};
            f32x4 a[T][2], b[2];
            auto load_pair = [&](int s, f32x4 (&av)[T][2], f32x4 (&bv)[2]) __attribute__((always_inline)) {
#pragma unroll
                for (int t = 0; t < T; ++t) {
                    av[t][0] = *(reinterpret_cast<const f32x4*>(sb + (t * tile_bytes + 128u * s) + voff));
                    av[t][1] = *(reinterpret_cast<const f32x4*>(sb + (t * tile_bytes + 128u * s + 64u) + voff));
                }
                bv[0] = *reinterpret_cast<const f32x4*>(qb + 128u * s);
                bv[1] = *reinterpret_cast<const f32x4*>(qb + 128u * s + 64u);
            };
            auto mfma_half = [&](const f32x4 (&av)[T][2], const f32x4 (&bv)[2], int u) __attribute__((always_inline)) {
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int t = 0; t < T; ++t) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[t][u][i], bv[u][i], acc[t], 0, 0, 0);
            };
            if (n_pairs > 0) load_pair(0, a, b);
            for (int s = 0; s < n_pairs; ++s) {
                f32x4 an[T][2], bn2[2];
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
            if (C & 1) {  // the last 16 floats of a row whose dim_p is an odd number of segments
#pragma unroll
                for (int t = 0; t < T; ++t) a[t][0] = *(reinterpret_cast<const f32x4*>(sb + (t * tile_bytes + 128u * n_pairs) + voff));
                b[0] = *reinterpret_cast<const f32x4*>(qb + 128u * n_pairs);
                mfma_half(a, b, 0);
            }
            const bool ragged = row0 + kIvfNdBlockRows - 1 > last_row;  // wave-uniform
#pragma unroll
            for (int t = 0; t < T; ++t) {
                const int64_t rbase = row0 + 16 * t + 4 * g;
                float d[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    if constexpr (IP)
                        d[j] = -acc[t][j];  // (an exactly zero product is +0 out of the chain: -0.0)
                    else
                        d[j] = fmaf(-2.0f, acc[t][j], qn + p.vnorm[rbase + j]);  // (the norms have 64 spare entries)
                    if (ragged && rbase + j > last_row) d[j] = VS_INF;  // (under IP a spare row's -0.0 must never compete)
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

hipError_t launch_ivf_nd_plan(const IvfNdParams& p, hipStream_t s) {
    if (p.dim < 1 || p.dim > kNdMaxDim || p.dim_p != nd_dim_p(p.dim) || p.group_q < 1 || p.group_q > kIvfNdGroupQ || p.nprobe < 1 ||
        p.nprobe > kIvfMaxProbe || p.nlist < 1 || (p.kcap != 8 && p.kcap != 16))
        return hipErrorInvalidValue;
    const int pairs = p.group_q * p.nprobe;
    hipLaunchKernelGGL(ivf_nd_prep, dim3((p.group_q + kMaxBatch - 1) / kMaxBatch), dim3(256), 0, s, p);
    hipLaunchKernelGGL(ivf_nd_count, dim3((pairs + 255) / 256), dim3(256), 0, s, p, 1);
    hipLaunchKernelGGL(ivf_nd_prefix, dim3(1), dim3(1024), 0, s, p);
    hipLaunchKernelGGL(ivf_nd_fill, dim3((pairs + 255) / 256), dim3(256), 0, s, p);
    return hipGetLastError();
}

hipError_t launch_ivf_nd_plan_second(const IvfNdParams& p, hipStream_t s) {
    if (p.group_q < 1 || p.group_q > kIvfNdGroupQ || p.nprobe < 1 || p.nprobe > kIvfMaxProbe || p.nlist < 1 || (!p.route && !p.pair_mask))
        return hipErrorInvalidValue;
    const int pairs = p.group_q * p.nprobe;
    hipLaunchKernelGGL(ivf_nd_count, dim3((pairs + 255) / 256), dim3(256), 0, s, p, 0);
    hipLaunchKernelGGL(ivf_nd_prefix, dim3(1), dim3(1024), 0, s, p);
    hipLaunchKernelGGL(ivf_nd_fill, dim3((pairs + 255) / 256), dim3(256), 0, s, p);
    return hipGetLastError();
}

hipError_t launch_ivf_nd_scan(const IvfNdParams& p, int grid, hipStream_t s) {
    if (grid < 1 || p.k < 1 || p.k > p.kcap) return hipErrorInvalidValue;
    if (p.metric != 0 && p.metric != 1) return hipErrorInvalidValue;
    if (p.kcap == 8 && !p.metric)
        hipLaunchKernelGGL((ivf_scan_nd_kernel<8, false>), dim3(grid), dim3(kScanThreads), 0, s, p);
    else if (p.kcap == 16 && !p.metric)
        hipLaunchKernelGGL((ivf_scan_nd_kernel<16, false>), dim3(grid), dim3(kScanThreads), 0, s, p);
    else if (p.kcap == 8)
        hipLaunchKernelGGL((ivf_scan_nd_kernel<8, true>), dim3(grid), dim3(kScanThreads), 0, s, p);
    else if (p.kcap == 16)
        hipLaunchKernelGGL((ivf_scan_nd_kernel<16, true>), dim3(grid), dim3(kScanThreads), 0, s, p);
    else
        return hipErrorInvalidValue;
    return hipGetLastError();
}

}  // namespace vs
