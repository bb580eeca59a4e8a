// vs_scan_one.hip -- the single-call brute-force scan: ONE launch per query batch (cpu_baseline.cpp:222-254 runs one
// query per iteration; BASELINE configs[1] is batch = 1).
//
//   scan_one_kernel<NQH, KCAP>: Q[<= 16 NQH x 128] x base^T on v_mfma_f32_16x16x4_f32 with the L2 epilogue of
//   cpu_baseline.cpp:239-242 and select_topk's k smallest (:127-153) fused in, for calls too short to amortise the seed
//   launches of the streaming scans.  What it does without:
//     * no seed launches, no threshold exchange: a lane keeps its own sorted list of KCAP entries per query column and
//       looks at a distance only if it is below the list's last entry -- with 8192 lane streams per query the lists
//       settle after a few tiles (a lane inserts about k ln(n / k) of its n = N / 8192 rows);
//     * no second launch: every workgroup ranks its lanes' lists into one sorted partial list per query, and the
//       workgroup that arrives last (one atomic per workgroup) merges the partial lists into the result
//       (vs_one_tail.h, shared with scan_one_nd_kernel, like the bound from the lane minima that the loop takes).
//   Data path = the streaming scans': the per-wave ring of two 16-row tile slots of vs_ring.h (`nt`); tiles dealt statically (wave w of workgroup b takes tiles
//   b + (w + 8 n) G: at step n the 2048 waves of the grid read 2048 consecutive tiles) and no tile is fetched that is
//   not used -- with one pass over the rows per launch two discarded tail prefetches per wave would be 6 % of the bytes.
//   Bound: HBM (516 MB per call at SIFT-1M whatever the batch size).
#include "vs_kernels.h"
#include "vs_dev.h"
#include "vs_ring.h"
#include "vs_one_tail.h"

namespace vs {

namespace {

constexpr int kOneRing = kScanWaves * kRingWaveBytes;          // 135168
constexpr int kOneScratch = 8192;                                 // per-wave query norms [8][32] | counters [32] | bounds [32] | flag | lane minima [32][32]
constexpr int kOneLds = kOneRing + kOneScratch;

}  // namespace

template <int NQH, int KCAP>
__global__ __launch_bounds__(kScanThreads, 2) void scan_one_kernel(const OneParams p) {
    constexpr int TR = kTileRows;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* qn_w = reinterpret_cast<float*>(smem + kOneRing);       // [8 waves][32]
    int* lds_cnt = reinterpret_cast<int*>(qn_w + kScanWaves * 32);  // [32]
    unsigned* lds_bound = reinterpret_cast<unsigned*>(lds_cnt + 32);  // [32] ordered-float bits
    int* lds_flag = reinterpret_cast<int*>(lds_bound + 32);        // [1]
    int* lds_ticket = lds_flag + 1;                                 // [1] next tile ticket of the workgroup
    float* lds_lmin = reinterpret_cast<float*>(lds_flag + 32);      // [32 queries][32 lanes of the workgroup holding that column]
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r = lane & 15, g = lane >> 4;
    const int G = (int)gridDim.x;
    const int tiles_total = (int)((p.n_rows + TR - 1) / TR);
    // Run n of the base = tiles [n G, n G + G): the grid reads one run at about the same time, every workgroup one tile of
    // it.  A workgroup's ticket n (its tile of run n) goes to whichever of its waves asks next (an LDS counter: a wave
    // that is served late by HBM takes fewer tiles); the first two tickets of every wave are fixed: wave and wave + 8.
    // (a workgroup stays on one residue b of the runs.  Moving through the residues -- tile n G + (b + 17 n) mod G -- was
    // measured: the slowest workgroup then finished 60 % later than the fastest instead of 25 %)
    // (p.reverse: the runs are walked from the last to the first.  Calls alternate, so a call starts on the rows the previous
    // one read last -- what of them the 256 MB Infinity Cache still holds is not fetched from HBM again: 85.4 against 87.2 us
    // per call at 1 M rows; with the rows loaded without `nt` the effect is larger, 88.6 against 93.9, but the level worse)
    // (only the FULL runs change places; an incomplete last run stays the last ticket: a workgroup's tickets are valid up
    // to some n and invalid from there on, which is what the loop below relies on)
    const int n_full = tiles_total / G;
    auto tile_of = [&](int n) { return ((p.reverse && n < n_full) ? n_full - 1 - n : n) * G + (int)blockIdx.x; };
    const int t_first = tile_of(wave), t_second = tile_of(wave + kScanWaves);

    // ---- data path (vs_ring.h): LDS-DMA pieces as instructions, scalar tile base + the lane's 32-bit offset
    char* ring = smem + wave * kRingWaveBytes;
    unsigned voff[8];
    ring_src_offsets_f32(lane, voff);
    const unsigned voff_n = (unsigned)lane * 4u;
    const unsigned ring_lds = __builtin_amdgcn_readfirstlane((unsigned)(size_t)(__attribute__((address_space(3))) char*)ring);
    auto issue_tile = [&](int tile, int slot) __attribute__((always_inline)) {
        const int64_t row0 = (int64_t)tile * TR;
        ring_issue_tile<true>(ring_lds + (unsigned)(slot * kRingSlotBytes), reinterpret_cast<const char*>(p.base) + row0 * (kDim * 4),
                              reinterpret_cast<const char*>(p.bnorm + row0), voff, voff_n);  // (the norm array is padded by 64)
    };
    // ---- the queries as MFMA B operands: qf[h][c][i] = Q[16 h + r][16 c + 4 g + i]; padding queries (main.cpp:206-211)
    // are zero columns that nothing looks at.  Every wave for itself.  The loads go out FIRST and as instructions the
    // compiler does not see as memory operations (it would wait for them with vmcnt(0), i.e. for the two tiles requested
    // right behind them as well: the tile loop then started 3 us later).  One wait covers them -- always exactly two
    // tiles' younger pieces: a wave without a first or second tile fetches tile 0 into the slot -- and every loaded
    // register is tied behind it: nothing that reads them can be placed above it (copies of a loaded register that
    // the compiler made ahead of an untied wait statement were seen to break a test at random).
    f32x4 qf[NQH][8];
#pragma unroll
    for (int h = 0; h < NQH; ++h) {
        const int qsafe = min(16 * h + r, p.nq_valid - 1);
#pragma unroll
        for (int c = 0; c < 8; ++c) asm_load_b128(qf[h][c], p.q + (int64_t)qsafe * kDim + 16 * c + 4 * g);
    }
    ONE_STAMP(0);
    const bool have0 = t_first < tiles_total, have1 = t_second < tiles_total;  // (wave-uniform)
    issue_tile(have0 ? t_first : 0, 0);
    issue_tile(have1 ? t_second : 0, 1);
    wait_vm<2 * kRingPieces>();
#pragma unroll
    for (int h = 0; h < NQH; ++h) tie_loaded(qf[h]);
#pragma unroll
    for (int h = 0; h < NQH; ++h)
#pragma unroll
        for (int c = 0; c < 8; ++c)
            if (16 * h + r >= p.nq_valid) qf[h][c] = (f32x4){0.f, 0.f, 0.f, 0.f};
    // ||q||^2 in the reference's order (cpu_baseline.cpp:95-114): FMA lane j = e mod 8 accumulates Q[e]^2 over e = j,
    // j + 8, ..., then r0 + r1 + ... + r7 left to right.  Element e = 16 c + 4 g + i sits in lane group g: lane j's chain
    // alternates between groups g = j / 4 (steps 2 c) and g + 2 (steps 2 c + 1), so group g fetches group g + 2's
    // fragments (the lane 32 further on), runs the four chains j = 4 g + i, and group 0 then adds its four sums and the
    // four of group 1 (the lane 16 further on) in order.  No second set of loads, no LDS.
    float qn[NQH], tau[NQH];
    bool live[NQH];
#pragma unroll
    for (int h = 0; h < NQH; ++h) {
        float chain[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            f32x4 other;
#pragma unroll
            for (int i = 0; i < 4; ++i) other[i] = __shfl(qf[h][c][i], (lane + 32) & 63);
#pragma unroll
            for (int i = 0; i < 4; ++i) chain[i] = fmaf(qf[h][c][i], qf[h][c][i], chain[i]);  // step 2 c
#pragma unroll
            for (int i = 0; i < 4; ++i) chain[i] = fmaf(other[i], other[i], chain[i]);          // step 2 c + 1
        }
        float s = ((chain[0] + chain[1]) + chain[2]) + chain[3];  // r0 .. r3 in group 0 (r4 .. r7 in group 1)
#pragma unroll
        for (int i = 0; i < 4; ++i) s = s + __shfl(chain[i], (lane + 16) & 63);  // group 0: + r4, + r5, + r6, + r7
        qn[h] = __shfl(s, r);  // group 0's lane of this column
    }
#pragma unroll
    for (int h = 0; h < NQH; ++h) {
        live[h] = 16 * h + r < p.nq_valid;
        tau[h] = live[h] ? VS_INF : -VS_INF;  // a padding column never takes a candidate
    }
    // the lanes' current minima, shared by the workgroup (see the tile loop)
    for (int i = tid; i < 32 * 33; i += kScanThreads) lds_lmin[i] = VS_INF;  // (rows 33 apart: bank spread)
    if (tid == 0) lds_ticket[0] = 2 * kScanWaves;
    __syncthreads();
    ONE_STAMP(1);
    float ld[NQH][KCAP];
    int li[NQH][KCAP];
#pragma unroll
    for (int h = 0; h < NQH; ++h)
#pragma unroll
        for (int j = 0; j < KCAP; ++j) {
            ld[h][j] = VS_INF;
            li[h][j] = -1;
        }

    unsigned fa[8], fa_n;
    ring_frag_offsets_f32(wave * kRingWaveBytes, r, g, fa, fa_n);
    const int last_row = (int)p.n_rows - 1;

    // t_cur sits in slot `sl` (landed or landing), t_nxt in the other slot: nine DMA pieces behind it if it is a tile at all
    int t_cur = t_first, t_nxt = t_second;
    auto step = [&](const int sl) __attribute__((always_inline)) {
        const int tile = t_cur;
        int tk = 0;
        if (lane == 0) tk = atomicAdd(lds_ticket, 1);
        const int t_new = tile_of(__builtin_amdgcn_readfirstlane(tk));
        if (t_nxt < tiles_total) wait_vm<kRingPieces>();
        else wait_vm<0>();
        const char* src = smem + sl * kRingSlotBytes;
        f32x4 a[8];
#pragma unroll
        for (int c = 0; c < 8; ++c) a[c] = *reinterpret_cast<const f32x4*>(src + fa[c]);
        const f32x4 bn = *reinterpret_cast<const f32x4*>(src + fa_n);
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        if (t_new < tiles_total) issue_tile(t_new, sl);  // the slot is refilled as soon as its fragments sit in registers
        f32x4 acc[NQH];
#pragma unroll
        for (int h = 0; h < NQH; ++h) acc[h] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int c = 0; c < 8; ++c)
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int h = 0; h < NQH; ++h) acc[h] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[c][i], qf[h][c][i], acc[h], 0, 0, 0);
        const int rbase = tile * TR + 4 * g;
#pragma unroll
        for (int h = 0; h < NQH; ++h) {
            float d[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                // cpu_baseline.cpp:241  dist = qn + bn - 2*dot  (gcc contracts to fnmadd(2, dot, qn+bn))
                const float l2 = fmaf(-2.0f, acc[h][j], qn[h] + bn[j]);
                d[j] = p.metric ? -acc[h][j] : l2;
            }
            if (tile * TR + TR - 1 > last_row) {  // wave-uniform: only the last tile holds rows past the end
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (rbase + j > last_row) d[j] = VS_INF;
            }
            const float dmin = fminf(fminf(d[0], d[1]), fminf(d[2], d[3]));
            if (dmin < tau[h]) {
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (d[j] < tau[h]) {
                        list_insert<KCAP>(ld[h], li[h], d[j], rbase + j + p.id_offset);
                        tau[h] = fminf(tau[h], ld[h][KCAP - 1]);
                    }
                lds_lmin[(16 * h + r) * 33 + 4 * wave + g] = ld[h][0];  // this lane's best so far, for the shared bound
            }
        }
        t_cur = t_nxt;
        t_nxt = t_new;
    };
    int n = 0;
    while (t_cur < tiles_total) {  // (step() advances t_cur)
        step(0);
        if (t_cur < tiles_total) step(1);
        if (n == 0 || n == 2 || n == 6 || n == 14) {  // wave-uniform
#pragma unroll
            for (int h = 0; h < NQH; ++h) {
                const float sb = one_shared_bound(lds_lmin, 16 * h + r, g, p.k1);
                if (live[h] && sb < VS_INF) tau[h] = fminf(tau[h], next_up(sb));
            }
        }
        n += 2;
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    ONE_STAMP(2);
    one_tail<NQH, KCAP, kOneRing>(p, OneTailLds{smem, lds_cnt, lds_flag, lds_lmin}, ld, li);
}

int scan_one_grid(int64_t n_rows, int num_cus) {
    const int64_t tiles = (n_rows + kTileRows - 1) / kTileRows;
    return (int)std::max<int64_t>(1, std::min<int64_t>(std::min(num_cus, kSlotStride), (tiles + kScanWaves - 1) / kScanWaves));
}

template <int NQH, int KCAP>
static hipError_t launch_one_t(const OneParams& p, int grid, hipStream_t s) {
    return launch_big_lds<scan_one_kernel<NQH, KCAP>, kOneLds>(p, grid, kOneLds, s);
}

hipError_t launch_scan_one(const OneParams& p, int grid, hipStream_t s) {
    if (p.nq_valid < 1 || p.nq_valid > kMaxBatch || p.k1 < 1 || p.k1 > 16 || grid < 1 || grid > kSlotStride || p.n_rows < 1) return hipErrorInvalidValue;
    const int kcap = p.k1 <= 8 ? 8 : 16;
    if (p.nq_valid <= 16) return kcap == 8 ? launch_one_t<1, 8>(p, grid, s) : launch_one_t<1, 16>(p, grid, s);
    return kcap == 8 ? launch_one_t<2, 8>(p, grid, s) : launch_one_t<2, 16>(p, grid, s);
}

}  // namespace vs
