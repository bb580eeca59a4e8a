// vs_scan_f32f_i8.hip -- int8 prefilter sweep of the fp32 streaming scan on a byte-valued shard.
//
// scan_f32f_i8_kernel<CBW, D, NW> is scan_f32f_kernel (vs_scan.hip) with the bulk test on v_mfma_i32_16x16x64_i8: the rows
// come from the shard's exact byte copy (vs_index::d_vecs_u8, bytes x - 128, and the row terms d_rterm), the queries from
// the byte forms that the seed's query preparation writes (SeedParams::q8frag / qterm) -- two MFMAs per 16-row tile and
// column block instead of four, and ring units of 8 KB + 256 B instead of 16 KB + 256 B.  The test is exact in integers
// (filter_i8_thr, vs_kernels.h): there is no error bound, the candidates are the rows under tau0 (plus, for an odd bound,
// nothing: the rare path tests exactly).  L2 only.
//
// The sweep's entry is final: (query, (float)d, row + id_offset) is binned as it stands, and the kernel reads neither the
// fp32 rows nor their norms nor the raw queries.  The kernel runs only on a group whose batches are all byte valued
// (f32f_some_batch_not_bytes) against a byte-valued shard, and for such a pair scan_f32s_kernel's arithmetic gives the
// sweep's integer (filter_i8_dist, vs_kernels.h): dot = sum q b <= 128 * 255^2 < 2^24 with every product and partial
// sum an integer, so its fmaf chain is exact in any order; qn and bn are sums of integer squares <= 8 323 200 and
// qn + bn <= 16 646 400 < 2^24 is exact; d = fmaf(-2, dot, qn + bn) is one rounding of an exact integer below 2^24 --
// the integer d of the sweep, which it stores as (float)d (+0.0 for a zero distance on both sides).  scan_f32s_kernel
// keeps a row iff fmaf(-2, dot, bn) < stream_l2_thr(tau, qn) && d < tau, and stream_l2_thr is built so that d < tau
// implies the first test (vs_f32f.h): keep <=> d < tau0, which filter_i8_exact decided before the entry was written
// (NaN and infinite bounds alike: filter_i8_thr's clamp).  So every id, distance bit and flag is what scan_f32s_kernel
// decides.  Comparison toggle VSEARCH_F32_FILTER_I8_RECHECK=1 (StreamParams::i8_recheck): the wave recomputes every
// entry from the fp32 rows by RecheckF32 when it bins its buffer, as the bf16 sweep must -- the same bytes, later.
//
// Kept from scan_f32f_kernel: the grid and both organisations (NW = 8: one workgroup per CU; NW = 4: two halves, waves vw =
// w + 4 z), one sweep of the workgroup's 64-row units (bx + n G) for all batches, column blocks vw + 8 h, one shared ring
// of D unit slots filled by LDS-DMA, one raw s_barrier per unit with the constant-vmcnt handshake, two alternating
// fragment sets, the test of block h beside the MFMAs of h + 1, the wave buffers, list hashes and candidate entry.
//
// Layout of a slot.  A byte row is 128 bytes = 8 chunks of 16; chunk 4 s + g is what lane (r, g) feeds k-step s (bytes
// 64 s + 16 g ..: the row-major row already is in fragment order).  A unit is eight 1 KB pieces of 8 rows; wave w moves
// pieces kPieces w .. kPieces (w + 1) - 1 (kPieces = 8 / NW).  The LDS side of a DMA is lane-linear -- lane l of piece c
// lands at row b = 8 c + (l >> 3), stored chunk l & 7 -- and the swizzle is applied to the source address:
//     stored chunk j of row b  <-  source chunk j ^ ((b >> 1) & 7).
// Rows are 128 bytes apart, two per 256-byte bank row, so the sixteen rows r = 0..15 that one ds_read_b128 lane group
// reads (fixed s, g) lie in eight bank rows; the 16-byte slot a lane hits is 8 (r & 1) + ((4 s + g) ^ (r >> 1)): r & 1
// picks the half of the bank row and the XOR with r >> 1 = 0..7 runs through all eight chunks of that half -- sixteen
// different slots, no conflict.  (The bf16 image's swizzle, chunk ^ (b & 15) over 256-byte rows, would put rows 2 i and
// 2 i + 1 of a 128-byte layout on chunks that collide in pairs.)  This is the byte tile layout of vs_ring.h.
// The unit's 64 row terms ride behind the rows in place of the norms (every wave moves them: one constant vmcnt).
#include "vs_f32f.h"
#include "vs_sink.h"
#include "vs_ring.h"
#include <algorithm>

namespace vs {

typedef int i32x4 __attribute__((ext_vector_type(4)));

#ifndef VS_F32F_I8_DEPTH
#define VS_F32F_I8_DEPTH 4
#endif
constexpr int kI8FilterDepth = VS_F32F_I8_DEPTH;
constexpr int kI8UnitRowBytes = kUnitRows * kDim;              // 8 KB of byte rows
constexpr int kI8UnitBytes = kI8UnitRowBytes + kUnitRows * 4;  // + the unit's 64 row terms

// CBW = column blocks per (virtual) wave (1, 2, 4 or 8), D = unit slots of the shared ring, NW = waves per workgroup.
template <int CBW, int D, int NW>
__global__ __launch_bounds__(NW * 64, NW == 8 ? 1 : 2) void scan_f32f_i8_kernel(const StreamParams p) {
    constexpr int TR = kTileRows;
    static_assert(NW == 8 || NW == 4, "one 8-wave workgroup per CU, or two 4-wave halves");
    constexpr int kPieces = kScanWaves / NW;  // 1 KB row pieces per wave and unit
    constexpr int kUnitVmem = kPieces + 1;    // vector-memory instructions per wave and unit: the row pieces + the term piece
    static_assert(kI8UnitRowBytes == kPieces * NW * 1024, "a unit is kPieces 1 KB row pieces per wave");
    static_assert(D >= 3 && D <= 8 && (kScanWaves / NW) * D * kI8UnitBytes <= 160 * 1024, "the ring: one slot being read, one being filled, >= 1 in flight");
    static_assert((D - 2) * kUnitVmem <= 63, "vmcnt is a 6-bit count");
    extern __shared__ __attribute__((aligned(16))) char smem[];
#ifdef VS_F32F_ENDS
    // Diagnostic builds (-DVS_F32F_ENDS, scripts/diag/f32fstamps.py --ends): scan_f32f_kernel's three clock reads per wave,
    // none inside the loop, and two words from inside the tail (sink_bin_wave)
    const unsigned long long en_start = __builtin_amdgcn_s_memrealtime();
#endif
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int r = lane & 15, g = lane >> 4;
    const int units_total = (int)((p.n_rows + kUnitRows - 1) / kUnitRows);
    // NW = 4: workgroup x + G z is half z of workgroup x of the 8-wave grid (scan_f32f_kernel)
    const int G = (int)gridDim.x / (kScanWaves / NW);
    const int z = NW == 8 ? 0 : ((int)blockIdx.x >= G ? 1 : 0);
    const int bx = (int)blockIdx.x - z * G;
    const int vw = wave + NW * z;
    const int T = (units_total - bx + G - 1) / G;  // units of this workgroup (G <= units_total: T >= 1)
    const int n_cb = 2 * p.n_batches;
    if (NW * z >= n_cb) return;  // (workgroup-uniform, NW = 4 only) a half none of whose waves has a column block
    // a batch that is not byte valued: the bf16 sweep enqueued behind answers the whole group (kernel-uniform)
    if (f32f_some_batch_not_bytes(p.invalid, p.n_batches, lane)) {
        if (p.i8_stats && blockIdx.x == 0 && threadIdx.x == 0) atomicAdd(p.i8_stats + 1, 1ull);
        return;
    }

    // LDS-DMA as in scan_f32f_kernel: "scalar unit base + this lane's 32-bit offset", M0 saved and restored in the statement
    unsigned voff[kPieces];
#pragma unroll
    for (int j = 0; j < kPieces; ++j) {
        const int row_in = 8 * (kPieces * wave + j) + (lane >> 3);
        voff[j] = (unsigned)(row_in * kDim + 16 * ((lane & 7) ^ ((row_in >> 1) & 7)));
    }
    const unsigned voff_n = (unsigned)lane * 4u;
    const unsigned ring_lds = __builtin_amdgcn_readfirstlane((unsigned)(size_t)(__attribute__((address_space(3))) char*)smem);
    auto issue_unit = [&](int n, int slot) __attribute__((always_inline)) {  // unit n of the workgroup, kUnitVmem instructions
        // past the end (the last D - 1 prefetches): the workgroup's last unit once more, into a slot nobody reads
        const int64_t row0 = ((int64_t)bx + (int64_t)min(n, T - 1) * G) * kUnitRows;
        const char* ub = reinterpret_cast<const char*>(p.base_u8) + row0 * kDim;
        const char* nb = reinterpret_cast<const char*>(p.rterm + row0);
        const unsigned dst_n = ring_lds + (unsigned)(slot * kI8UnitBytes + kI8UnitRowBytes);
        unsigned keep;
#pragma unroll
        for (int j = 0; j < kPieces; ++j) {
            const unsigned dst = ring_lds + (unsigned)(slot * kI8UnitBytes) + (unsigned)(kPieces * wave + j) * 1024u;
            asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2 nt\n\ts_mov_b32 m0, %0"
                         : "=&s"(keep) : "v"(voff[j]), "s"(ub), "s"(dst) : "memory");
        }
        asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\tglobal_load_lds_dword %1, %2\n\ts_mov_b32 m0, %0"
                     : "=&s"(keep) : "v"(voff_n), "s"(nb), "s"(dst_n) : "memory");
    };
    // this lane's fragment of k-step s of tile 0 of a slot (tile i: + 2048 i): row r, chunk (4 s + g) ^ (r >> 1)
    unsigned fa[2];
#pragma unroll
    for (int s = 0; s < 2; ++s) fa[s] = (unsigned)(r * kDim + (((4 * s + g) ^ (r >> 1)) << 4));
    const unsigned fa_n = (unsigned)(kI8UnitRowBytes + 16 * g);  // terms of rows 4 g .. 4 g + 3 of tile 0 (tile i: + 64 i)

    // The wave's column blocks as int8 B operands, loaded once for the launch, with the queries' terms and bounds: loads
    // written as instructions and tied behind the prologue's wait (vs_ring.h).  A column block past the launch's loads
    // the last one and gets the bound that nothing passes.
    i32x4 qb[CBW][2];
    int qt[CBW];
    float tau[CBW];
#pragma unroll
    for (int h = 0; h < CBW; ++h) {
        const int cb = min(vw + kScanWaves * h, n_cb - 1);  // = 2 batch + half
        const int qrow = 16 * (cb & 1) + r;
        const int qglob = (cb >> 1) * kMaxBatch + (qrow < p.nq_valid ? qrow : 0);
        const int8_t* src = p.q8frag + ((int64_t)cb * 2 * 64 + lane) * 16;  // 1 KB per instruction
        asm_load_b128(qb[h][0], src);
        asm_load_b128(qb[h][1], src + 64 * 16);
        asm_load_b32(qt[h], p.qterm + qglob);
        asm_load_b32(tau[h], p.tau0 + qglob);
    }
#pragma unroll
    for (int s = 0; s < D - 1; ++s) issue_unit(s, s);
    wait_vm<(D - 2) * kUnitVmem>();  // the operands (older than every DMA) and unit 0 are here
    int thr[CBW], thr2[CBW];  // filter_i8_thr and its floored half (the hot test's side)
#pragma unroll
    for (int h = 0; h < CBW; ++h) {
        tie_loaded(qb[h]), tie_loaded(qt[h]), tie_loaded(tau[h]);
        const int cb = vw + kScanWaves * h;
        const bool live = cb < n_cb && 16 * (cb & 1) + r < p.nq_valid;
        thr[h] = live ? filter_i8_thr(tau[h], qt[h]) : kFilterI8Dead;
        thr2[h] = thr[h] >> 1;
    }

    int4* wbuf = p.sink.wbuf + ((int64_t)bx * kScanWaves + vw) * p.sink.wcap;
    int wbase = 0;  // wave-uniform fill of the private candidate buffer

    // The step is scan_f32f_kernel's (the handshake is described there): wait for this wave's pieces of unit t + 1, barrier,
    // issue unit t + D - 1 into the slot just freed, four tiles alternating between two fragment sets read two tiles ahead.
    i32x4 a[2][2], rt[2];
    auto read_frags = [&](const int set, const int sl, const int i) __attribute__((always_inline)) {
        const char* src = smem + sl * kI8UnitBytes + i * (TR * kDim);
#pragma unroll
        for (int s = 0; s < 2; ++s) a[set][s] = *reinterpret_cast<const i32x4*>(src + fa[s]);
        rt[set] = *reinterpret_cast<const i32x4*>(smem + sl * kI8UnitBytes + fa_n + 64 * i);
    };
    __builtin_amdgcn_s_barrier();  // unit 0 landed with the operands: publish it, read its first two tiles
    asm volatile("" ::: "memory");
    read_frags(0, 0, 0);
    read_frags(1, 0, 1);
    auto score_tile = [&](const int set, const int row_t) __attribute__((always_inline)) {  // row_t: this lane's first row, 16 tile + 4 g
        // -rh through the C operand of the first MFMA: the accumulators come out as A = acc - rh (filter_i8_thr)
        i32x4 c0;
#pragma unroll
        for (int j = 0; j < 4; ++j) c0[j] = filter_i8_c0(rt[set][j]);
        auto mfma_cb = [&](const int h) __attribute__((always_inline)) -> i32x4 {
            i32x4 acc = __builtin_amdgcn_mfma_i32_16x16x64_i8(a[set][0], qb[h][0], c0, 0, 0, 0);
            return __builtin_amdgcn_mfma_i32_16x16x64_i8(a[set][1], qb[h][1], acc, 0, 0, 0);
        };
        auto test_cb = [&](const int h, const i32x4 acc) __attribute__((always_inline)) {
            const int emax = max(max(max(acc[0], acc[1]), acc[2]), acc[3]);
            if (__builtin_expect(__ballot(emax > thr2[h]) != 0, 0)) {  // rare: a few hundred rows per query per million
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int row = row_t + j;
                    const bool pass = filter_i8_exact(acc[j], rt[set][j], thr[h]) && row < (int)p.n_rows;
                    const unsigned long long mask = __ballot(pass);
                    if (mask) {  // wave-uniform
                        const int pos = wbase + (int)__builtin_amdgcn_mbcnt_hi((unsigned)(mask >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)mask, 0));
                        // (query, value, id): the value is the distance, final (the kernel's head); query = 16 cb + r
                        const int qglob = 16 * (vw + kScanWaves * h) + r;
                        const float d = filter_i8_dist(qt[h], rt[set][j], acc[j] + (rt[set][j] >> 1));  // acc = dot - (rt >> 1)
                        if (pass && pos < p.sink.wcap)
                            wbuf[pos] = make_int4(qglob, __builtin_bit_cast(int, d), row + p.id_offset, 0);
                        wbase += __popcll(mask);
                    }
                }
            }
        };
        i32x4 acc = mfma_cb(0);
#pragma unroll
        for (int h = 1; h < CBW; ++h) {
            const i32x4 nxt = mfma_cb(h);
            test_cb(h - 1, acc);
            acc = nxt;
        }
        test_cb(CBW - 1, acc);
        // the tile's last chain has issued, so every fragment of this set has arrived: the barrier behind which the
        // set's slot is refilled follows the set's LDS reads
        asm volatile("" ::"v"(acc));
    };
    // Diagnostic builds (-DVS_STAMPS, scripts/diag/f32fstamps.py): the step split of scan_f32f_kernel -- [0] between
    // steps, [1] the vmcnt wait, [2] the barrier, [3] the unit's DMA issue, [4 + i] tile i, summed over the wave's steps in
    // shader clocks and written by lane 0 at the wave's end to dbg[workgroup][wave][16] ([8] = steps, [9] = candidates).
#ifdef VS_STAMPS
    int st_sum[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    unsigned st_prev = (unsigned)__builtin_amdgcn_s_memtime();
#define VS_F32F_STAMP(i)                                                \
    do {                                                                \
        const unsigned now_ = (unsigned)__builtin_amdgcn_s_memtime();   \
        st_sum[i] += (int)(now_ - st_prev);                             \
        st_prev = now_;                                                 \
    } while (0)
#else
#define VS_F32F_STAMP(i)
#endif
    auto step = [&](const int t, const int sl) __attribute__((always_inline)) {
        VS_F32F_STAMP(0);
        wait_vm<(D - 3) * kUnitVmem>();
        VS_F32F_STAMP(1);
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
        VS_F32F_STAMP(2);
        if constexpr (NW == 4) {  // half 1 wins the SIMD on f32f_prio steps of every eight (scan_f32f_kernel)
            if (z == 1 && p.f32f_prio) {
                if ((t & 7) < p.f32f_prio) __builtin_amdgcn_s_setprio(1);
                else __builtin_amdgcn_s_setprio(0);
            }
        }
        issue_unit(t + D - 1, (sl + D - 1) % D);
        VS_F32F_STAMP(3);
        const int row_u = (bx + t * G) * kUnitRows + 4 * g;
#pragma unroll
        for (int i = 0; i < kUnitTiles; ++i) {
            score_tile(i & 1, row_u + TR * i);
            if (i + 2 < kUnitTiles) read_frags(i & 1, sl, i + 2);
            else read_frags(i & 1, (sl + 1) % D, i + 2 - kUnitTiles);
            VS_F32F_STAMP(4 + i);
        }
    };
    // one turn of the ring per iteration, every slot a constant; T is workgroup-uniform: every wave passes the same barriers
    for (int t0 = 0; t0 < T; t0 += D) {
        step(t0, 0);
        if (t0 + 1 >= T) break;
        step(t0 + 1, 1);
        if (t0 + 2 >= T) break;
        step(t0 + 2, 2);
        if constexpr (D > 3) { if (t0 + 3 >= T) break; step(t0 + 3, 3); }
        if constexpr (D > 4) { if (t0 + 4 >= T) break; step(t0 + 4, 4); }
        if constexpr (D > 5) { if (t0 + 5 >= T) break; step(t0 + 5, 5); }
        if constexpr (D > 6) { if (t0 + 6 >= T) break; step(t0 + 6, 6); }
        if constexpr (D > 7) { if (t0 + 7 >= T) break; step(t0 + 7, 7); }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // retire the tail prefetches before the wave ends
#ifdef VS_STAMPS
    if (p.dbg && lane == 0) {
        int32_t* o = p.dbg + ((int64_t)bx * kScanWaves + vw) * 16;
#pragma unroll
        for (int i = 0; i < 8; ++i) o[i] = st_sum[i];
        o[8] = T;
        o[9] = wbase;
    }
#endif
#undef VS_F32F_STAMP
    if constexpr (NW == 4) {
        if (z == 1 && p.f32f_prio) __builtin_amdgcn_s_setprio(0);
    }
#ifdef VS_F32F_ENDS
    const unsigned long long en_loop = __builtin_amdgcn_s_memrealtime();
    unsigned long long en_tail[2] = {0ull, 0ull};
#define VS_F32F_TAIL , 0, en_tail
#else
#define VS_F32F_TAIL
#endif
    // the entries are final and binned as they are; the toggle (kernel-uniform) recomputes them from the fp32 rows first
    int kept;
    if (__builtin_expect(p.i8_recheck, 0)) {
        const RecheckF32 fix{p.base, p.bnorm, p.q, p.q_batch_stride, p.qnorm, p.tau0, 0, p.id_offset};
        kept = sink_bin_wave<RecheckF32, true>(p.sink, bx * kScanWaves + vw, wbase, lane, fix VS_F32F_TAIL);
    } else {
        kept = sink_bin_wave(p.sink, bx * kScanWaves + vw, wbase, lane, SinkEntryAsIs() VS_F32F_TAIL);
    }
#undef VS_F32F_TAIL
    if (p.i8_stats && wbase > 0) {  // (wave-uniform) one atomic instruction: lane 0 adds the sweep's count, lane 1 the entries binned
#pragma unroll
        for (int u = 32; u >= 1; u >>= 1) kept += __shfl_xor(kept, u);
        if (lane < 2) atomicAdd(p.i8_stats + 2 + lane, (unsigned long long)(lane == 0 ? wbase : kept));
    }
#ifdef VS_F32F_ENDS
    // scan_f32f_kernel's dbg[workgroup][wave][16]: [0..1] start, [2..3] loop end, [4..5] end (100 MHz ticks, low word first),
    // [6] units swept, [7] XCC_ID, [8] candidates; and of the tail: [9..10] the first round read back (and rechecked, under
    // the toggle), just before the first binning atomic, [11] ticks of read-back (and recheck) summed over the rounds
    const unsigned long long en_end = __builtin_amdgcn_s_memrealtime();
    if (p.dbg && lane == 0) {
        int32_t* o = p.dbg + ((int64_t)bx * kScanWaves + vw) * 16;
        o[0] = (int)en_start, o[1] = (int)(en_start >> 32);
        o[2] = (int)en_loop, o[3] = (int)(en_loop >> 32);
        o[4] = (int)en_end, o[5] = (int)(en_end >> 32);
        o[6] = T;
        o[7] = (int)(__builtin_amdgcn_s_getreg((3 << 11) | 20) & 7);
        o[8] = wbase;
        o[9] = (int)en_tail[0], o[10] = (int)(en_tail[0] >> 32);
        o[11] = (int)en_tail[1];
    }
#endif
}

template <int CBW, int NW>
static hipError_t launch_i8(const StreamParams& p0, int grid, hipStream_t s) {
    constexpr int kLds = kI8FilterDepth * kI8UnitBytes;  // per workgroup: at NW = 4 a CU holds two rings
    auto kfn = scan_f32f_i8_kernel<CBW, kI8FilterDepth, NW>;
    const int64_t units = (p0.n_rows + kUnitRows - 1) / kUnitRows;
    grid = (int)std::max<int64_t>(1, std::min<int64_t>(grid, units));  // every workgroup owns a unit
    StreamParams p = p0;
    if (p.f32f_prio < 0) p.f32f_prio = f32f_prio_default(units / grid);
    static bool attr_set[64] = {};
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) dev = 0;
    if (!attr_set[dev]) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kfn), hipFuncAttributeMaxDynamicSharedMemorySize, kLds);
        if (e != hipSuccess) return e;
        attr_set[dev] = true;
    }
    hipLaunchKernelGGL(kfn, dim3(grid * (kScanWaves / NW)), dim3(NW * 64), kLds, s, p);
    return hipGetLastError();
}

template <int CBW>
static hipError_t launch_i8(const StreamParams& p, int grid, hipStream_t s) {
    const int nw = p.f32f_waves ? p.f32f_waves : f32f_waves_default(CBW);
    return nw == 4 ? launch_i8<CBW, 4>(p, grid, s) : launch_i8<CBW, 8>(p, grid, s);
}

hipError_t launch_scan_f32f_i8(const StreamParams& p, int cbw, int grid, hipStream_t s) {
    return cbw == 1 ? launch_i8<1>(p, grid, s) : cbw == 2 ? launch_i8<2>(p, grid, s) : cbw == 4 ? launch_i8<4>(p, grid, s) : launch_i8<8>(p, grid, s);
}

}  // namespace vs
