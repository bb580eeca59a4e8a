// vs_ndf_sweep.h -- the prefilter sweep of a general index, written once for its two sources of rows: the bf16 image of
// fp32 rows (vs_scan_nd_f32f.hip) and the stored half rows (vs_scan_nd_f16f.hip).
//
// ONE sweep over the rows for up to 8 * CBW 16-query column blocks: a tiled 16-bit MFMA product with a threshold epilogue.
// What passes is recomputed exactly by the source's recheck functor when the wave bins its buffer, so every id, distance
// bit and flag is decided as the per-batch scan decides it.
//
// Organisation.  A unit is 64 rows (four 16-row tiles), K walks in slabs of 32 elements, S slabs per row.  Workgroup x
// of gridDim.x sweeps units x + n G; gridDim.y = passes, pass y serves column blocks [64 y CBW / 8 ...): wave w owns
// column blocks cb0 + w + 8 h, h < CBW, and keeps their accumulators for the unit's four row tiles (4 CBW f32x4) resident
// while K walks in slabs.  A step is one (unit, slab): every wave issues 1 + CBW LDS-DMA pieces for step j + D - 1 --
// waves 0..3 one of the slab's four 1 KB row pieces (tile `wave`: where it lies is the source's business, it lands
// lane-linear and is read back with one ds_read_b128 at 16 lane, no bank conflict, no swizzle), waves 4..7 the unit's 64
// stored norms (256 bytes, the same piece four times), and every wave the CBW 1 KB B pieces of its own column blocks,
// which only it reads -- waits for its own pieces of step j by a constant vmcnt, passes one raw s_barrier (which publishes
// the row pieces of step j and frees the slot of step j - 1), and feeds 4 CBW MFMAs from LDS.  The loop contains no other
// vector-memory instruction than these pieces and the (rare) candidate stores, which only make the counted wait stricter.
// Each unit of the rows leaves HBM once per pass: ceil(n_cb / (8 CBW)) times per launch group, i.e. once up to 16
// batches and twice from 17 to 32 (CBW <= 4: the accumulators, not LDS, set that limit).
// The prepared queries are 16-bit B fragments in the k order of the rows' pieces: qb16[(cb * S + s) * 64 + lane][j], j < 8.
//
// A source is a policy struct `Src`, defined beside the code it describes, built once per thread from (p, lane):
//   Src::Params                      its parameter struct (NdfSweepParams and its own fields)
//   row_piece(unit, s, wave), voff   wave-uniform address and per-lane byte offset of row tile `wave` of step (unit, s)
//   Src::mfma(a, b, c)               the 16x16x32 MFMA of its number format on i32x4 fragments
//   Src::threshold(p, ip, qg, herald) the hot test's threshold of query qg; `herald` is true in lane group 0 of the pass's
//                                    first workgroup, for a source that has something to announce about a query
//   Src::recheck(p, ip)              the exact recheck functor for sink_bin_wave
//   Src::kernel<CBW, IP>()           (host) its __global__ wrapper around ndf_sweep<Src, CBW, IP>
// The body does not know which source it serves.
#pragma once
#include "vs_kernels.h"
#include "vs_dev.h"
#include "vs_sink.h"
#include "vs_ring.h"
#include <algorithm>

namespace vs {

constexpr int kNdfWaves = 8;
constexpr int kNdfSlabBytes = kNdfUnitRows * 64;             // 4 KB: 64 rows x 32 16-bit elements
constexpr int kNdfNormOff = kNdfSlabBytes;                   // the unit's 64 stored norms behind the rows
constexpr int kNdfBOff = kNdfSlabBytes + kNdfUnitRows * 4;   // the waves' B pieces behind those
constexpr int ndf_slot_bytes(int cbw) { return kNdfBOff + kNdfWaves * cbw * 1024; }
constexpr int ndf_depth(int cbw) { return std::min(8, (160 * 1024) / ndf_slot_bytes(cbw)); }  // slots of the ring

template <class Src, int CBW, bool IP>
__device__ __forceinline__ void ndf_sweep(const typename Src::Params& p) {
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

    // per (h, lane): the hot test's threshold of query 16 cb + r; +inf for a dead block or a padding query
    float th[CBW];
#pragma unroll
    for (int h = 0; h < CBW; ++h) {
        const int cb = cb0 + wave + NW * h;
        const int qrow = 16 * (cb & 1) + r;
        th[h] = VS_INF;
        if (cb < n_cb && qrow < p.nq_valid) th[h] = Src::threshold(p, IP ? 1 : 0, (cb >> 1) * kMaxBatch + qrow, bx == 0 && g == 0);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // (the accesses above are the compiler's; the counted queue starts empty)

    const unsigned ring_lds = __builtin_amdgcn_readfirstlane((unsigned)(size_t)(__attribute__((address_space(3))) char*)smem);
    const unsigned voff16 = (unsigned)lane * 16u, voff4 = (unsigned)lane * 4u;
    const Src src(p, lane);
    const char* qsrc[CBW];  // this wave's column blocks in the prepared queries (a block past the launch's: the last one)
#pragma unroll
    for (int h = 0; h < CBW; ++h) qsrc[h] = reinterpret_cast<const char*>(p.qb16) + (int64_t)min(cb0 + wave + NW * h, n_cb - 1) * S * 1024;
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
            const char* from = uni(src.row_piece(unit, s, wave));
            const unsigned dst = sbase + (unsigned)wave * 1024u;
            asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2 nt\n\ts_mov_b32 m0, %0"
                         : "=&s"(keep) : "v"(src.voff), "s"(from), "s"(dst) : "memory");
        } else {
            const char* from = uni(reinterpret_cast<const char*>(p.bnorm + unit * kNdfUnitRows));
            const unsigned dst = sbase + (unsigned)kNdfNormOff;
            asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\tglobal_load_lds_dword %1, %2\n\ts_mov_b32 m0, %0"
                         : "=&s"(keep) : "v"(voff4), "s"(from), "s"(dst) : "memory");
        }
#pragma unroll
        for (int h = 0; h < CBW; ++h) {
            const char* from = uni(qsrc[h] + s * 1024);
            const unsigned dst = sbase + (unsigned)(kNdfBOff + (wave * CBW + h) * 1024);
            asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2\n\ts_mov_b32 m0, %0"
                         : "=&s"(keep) : "v"(voff16), "s"(from), "s"(dst) : "memory");
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
            for (int t = 0; t < 4; ++t) acc[t][h] = Src::mfma(a[t], b[h], acc[t][h]);
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
                                // (query, value, id): the value is replaced by the recheck's
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
    const auto fix = Src::recheck(p, IP ? 1 : 0);
    int kept = sink_bin_wave<decltype(fix), true>(p.sink, ((int)blockIdx.y * G + bx) * NW + wave, wbase, lane, fix);
    if (p.sink.stats && wbase > 0) {  // (wave-uniform) one atomic instruction: lane 0 adds the sweep's count, lane 1 the survivors
#pragma unroll
        for (int u = 32; u >= 1; u >>= 1) kept += __shfl_xor(kept, u);
        if (lane < 2) atomicAdd(p.sink.stats + 2 + lane, (unsigned long long)(lane == 0 ? wbase : kept));
    }
}

// what the two launchers ask of the common parameters and of the plan (each adds its own checks)
inline bool ndf_sweep_args_ok(const NdfSweepParams& p, const NdFilterPlan& g) {
    const int64_t units = (p.n_rows + kNdfUnitRows - 1) / kNdfUnitRows;
    return p.n_batches >= 1 && p.n_batches <= 32 && p.dim >= 1 && p.dim <= kNdMaxDim && g.grid >= 1 && g.grid <= units && g.passes >= 1 &&
           g.cbw >= 1 && g.cbw <= 4 && g.passes * kNdfWaves * g.cbw >= 2 * p.n_batches && (g.passes - 1) * kNdfWaves * g.cbw < 2 * p.n_batches &&
           (int64_t)g.grid * g.passes <= kSlotStride && p.n_rows <= 0x7fffffff - 2 * kNdfUnitRows && p.qb16 && p.qfrag && p.zero;
}

template <class Src, int CBW, bool IP>
static hipError_t launch_ndf_t(const typename Src::Params& p, int grid, int passes, hipStream_t s) {
    constexpr int kLds = ndf_depth(CBW) * ndf_slot_bytes(CBW);
    auto kfn = Src::template kernel<CBW, IP>();
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

// the sweep of a validated plan: column blocks per wave x metric
template <class Src>
static hipError_t launch_ndf_sweep(const typename Src::Params& p, const NdFilterPlan& g, hipStream_t s) {
    const bool ip = p.metric != 0;
    switch (g.cbw) {
    case 1: return ip ? launch_ndf_t<Src, 1, true>(p, g.grid, g.passes, s) : launch_ndf_t<Src, 1, false>(p, g.grid, g.passes, s);
    case 2: return ip ? launch_ndf_t<Src, 2, true>(p, g.grid, g.passes, s) : launch_ndf_t<Src, 2, false>(p, g.grid, g.passes, s);
    case 3: return ip ? launch_ndf_t<Src, 3, true>(p, g.grid, g.passes, s) : launch_ndf_t<Src, 3, false>(p, g.grid, g.passes, s);
    default: return ip ? launch_ndf_t<Src, 4, true>(p, g.grid, g.passes, s) : launch_ndf_t<Src, 4, false>(p, g.grid, g.passes, s);
    }
}

}  // namespace vs
