// vs_ivf_one_nd_i8.hip -- the scan launch of the single-call IVF search of a general index that keeps a byte copy of its
// rows (vs_ivf_create_nd_u8; gfx950): the second of TWO launches per batch of at most 16 queries, k <= 16.
//
//   ivf_one_scan_u8_kernel<KCAP, IP>: ivf_one_scan_kernel's organisation (vs_ivf_one_nd.hip: a fixed grid loops over the
//                     unit table the coarse launch wrote, the 8 waves take a unit's 64-row blocks round-robin, lane (r, g)
//                     keeps ONE sorted list for query column r, vs_one_tail.h after the loop) in two phases over one
//                     unit table.  Units [0, n_units8) are BYTE units: their column masks hold the queries that qualify
//                     under the exactness rule (ivf_nd_prep_i8's, per query; the coarse launch's last workgroup decided),
//                     and their rows are read from the byte copy with v_mfma_i32_16x16x64_i8 -- ivf_scan_nd_i8_kernel's
//                     walk (128-byte steps one step ahead, a 64-byte tail step when dim_b / 64 is odd, unclamped onto the
//                     64 spare rows, no nontemporal hint) with the B fragments from LDS.  Units [n_units8, n_units) are
//                     FP32 units: the other queries of the batch, ivf_one_scan_kernel's own loop (vs_ivf_one_scan.h).
//                     A workgroup stages the queries once per phase it has units in -- bytes and integer terms
//                     (one_nd_stage_queries_i8; its batch verdict is ignored, the unit masks carry the per-query
//                     decision), then floats and norms over the same LDS region -- so a batch of one kind pays for
//                     one staging.  The lane lists, the bounds, the lane minima and the checkpoint count run through
//                     both phases: a column takes candidates in one phase only, and which one does not change a bit
//                     of its distances (below).
//
// Every branch on a phase is workgroup-uniform.  Nothing waits for another workgroup: the only hand-over is the ticket of
// the last arriver (vs_one_tail.h), left at zero.
//
// Kernel contract: for a query in a byte unit's mask the distance is (float)(qterm + rterm - 2 q'.b'), the integer
// ||q - b||^2 that the fp32 chain computes exactly under the rule (vs_ivf_nd_i8.hip), or -(float)(q.b) with q.b = q'.b' +
// 128 (sum q' + sum b') + 128^2 dim under inner product, -0.0 for a zero product: ivf_scan_nd_i8_kernel's numbers, which
// are ivf_scan_nd_kernel's.  Ids, distance bits, empty slots and the candidate count of a call are the group route's.
#include "vs_ivf_one_scan.h"

namespace vs {

template <int KCAP, bool IP>
__global__ __launch_bounds__(kScanThreads, 1) void ivf_one_scan_u8_kernel(const IvfOneU8Params p) {
    constexpr int T = kIvfOneTiles;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int dim_p = p.dim_p, dim_b = p.dim_b, B = p.o.nq_valid;
    const auto L = one_nd_lds<float>(smem, 4 * dim_p, KCAP);  // (the fp32 layout in both phases: 16 dim_b <= 64 dim_p)
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r = lane & 15, g = lane >> 4;
    const int n_units8 = p.n_units8[0], n_units = p.n_units[0];  // (the coarse launch's, stream ordered)
    const bool has8 = (int)blockIdx.x < n_units8;                 // workgroup-uniform, both
    const bool has32 = n_units8 + (int)blockIdx.x < n_units;

    // (no barrier of its own behind the reset: the staging of either phase ends with one, and a workgroup without units
    // reads the lane minima first in one_tail, behind one_tail's own opening barrier)
    one_nd_reset_lmin(L.tail.lmin);
    const bool live = r < B;
    float tau = VS_INF;  // the column's bound
    float ld[1][KCAP];
    int li[1][KCAP];
#pragma unroll
    for (int j = 0; j < KCAP; ++j) {
        ld[0][j] = VS_INF;
        li[0][j] = -1;
    }
    int c_n = 0;  // blocks this wave has done (wave-uniform): the checkpoints of the shared bound

    // ---- phase 1: the byte units
    if (has8) {
        const i32x4* q8frag = reinterpret_cast<const i32x4*>(L.tail.region);  // [dim_b / 64][64]
        int* lds_qt = reinterpret_cast<int*>(L.term);                          // [16]
        // (ends with a barrier, which also publishes the lane minima's reset)
        one_nd_stage_queries_i8<IP>(p.o.q, B, p.dim, dim_b, p.bmax, reinterpret_cast<i32x4*>(L.tail.region), lds_qt);
        const int qt = lds_qt[r];
        const unsigned voff = (unsigned)(r * dim_b + 16 * g);  // this lane's 16 bytes inside a 16-row tile's 64-byte step
        const unsigned tile_bytes = 16u * (unsigned)dim_b;     // 16 rows
        const int S = dim_b / 64;    // 64-byte steps per row
        const int n_pairs = S >> 1;  // full 128-byte steps
        const int32_t* const row_term = IP ? p.rsum : p.rterm;
#pragma clang loop unroll(disable)
        for (int unit = blockIdx.x; unit < n_units8; unit += gridDim.x) {
            const i32x4 u = reinterpret_cast<const i32x4*>(p.units)[unit];
            const int row_lo = u[0], row_end = u[1];  // (a unit that is not its list's last ends on a block boundary)
            const int last_row = row_end - 1;
            const bool mine = live && ((u[2] >> r) & 1);
            const int blocks_total = (row_end - row_lo + kIvfOneBlockRows - 1) / kIvfOneBlockRows;
#pragma clang loop unroll(disable)
            for (int wb = wave; wb < blocks_total; wb += kScanWaves) {
                const int row0 = row_lo + wb * kIvfOneBlockRows;
                const char* sb = reinterpret_cast<const char*>(p.vecs_u8) + (int64_t)row0 * dim_b;
                const int rt = row_term[row0 + lane];  // the block's row terms, one per lane (the terms have 64 spare entries)
                i32x4 acc[T];
#pragma unroll
                for (int t = 0; t < T; ++t) acc[t] = (i32x4){0, 0, 0, 0};
                i32x4 a[T][2];
                auto load_pair = [&](int s, i32x4 (&av)[T][2]) __attribute__((always_inline)) {
#pragma unroll
                    for (int t = 0; t < T; ++t) {
                        av[t][0] = *(reinterpret_cast<const i32x4*>(sb + (t * tile_bytes + 128u * s) + voff));
                        av[t][1] = *(reinterpret_cast<const i32x4*>(sb + (t * tile_bytes + 128u * s + 64u) + voff));
                    }
                };
                auto mfma_half = [&](const i32x4 (&av)[T][2], const i32x4 bv, int h) __attribute__((always_inline)) {
#pragma unroll
                    for (int t = 0; t < T; ++t) acc[t] = __builtin_amdgcn_mfma_i32_16x16x64_i8(av[t][h], bv, acc[t], 0, 0, 0);
                };
                if (n_pairs > 0) load_pair(0, a);
                for (int s = 0; s < n_pairs; ++s) {
                    i32x4 an[T][2];
                    const bool more = s + 1 < n_pairs;
                    if (more) load_pair(s + 1, an);
                    const i32x4 b0 = q8frag[(2 * s) * 64 + lane], b1 = q8frag[(2 * s + 1) * 64 + lane];
                    mfma_half(a, b0, 0);
                    mfma_half(a, b1, 1);
                    if (more) {
#pragma unroll
                        for (int t = 0; t < T; ++t) {
                            a[t][0] = an[t][0];
                            a[t][1] = an[t][1];
                        }
                    }
                }
                if (S & 1) {  // the last 64 bytes of a row whose dim_b is an odd number of steps
#pragma unroll
                    for (int t = 0; t < T; ++t) a[t][0] = *(reinterpret_cast<const i32x4*>(sb + (t * tile_bytes + 128u * n_pairs) + voff));
                    mfma_half(a, q8frag[(2 * n_pairs) * 64 + lane], 0);
                }
                const bool ragged = row0 + kIvfOneBlockRows - 1 > last_row;  // wave-uniform
                bool touched = false;
#pragma unroll
                for (int t = 0; t < T; ++t) {
                    const int rbase = row0 + 16 * t + 4 * g;
                    float d[4];
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const int rtj = __shfl(rt, 16 * t + 4 * g + j);
                        // ivf_scan_nd_i8_kernel's: the integer the fp32 scan computes exactly, ||q||^2 + ||b||^2 - 2 q.b, or
                        // -(q.b) (|q'.b'| <= 2^25, |128 (sum q' + sum b')| <= 2^26, 128^2 dim <= 2^25; zero gives -0.0)
                        if constexpr (IP)
                            d[j] = -(float)(qt + 128 * rtj + acc[t][j]);
                        else
                            d[j] = (float)(qt + rtj - 2 * acc[t][j]);
                        if (ragged && rbase + j > last_row) d[j] = VS_INF;  // (under IP a spare row's -0.0 must never compete)
                    }
                    if (ivf_one_take<KCAP>(d, rbase, mine, tau, ld[0], li[0])) touched = true;
                }
                ivf_one_checkpoint(L.tail, touched, ld[0][0], wave, r, g, live, p.o.k1, c_n, tau);
            }
        }
    }

    // ---- phase 2: the fp32 units, ivf_one_scan_kernel's loop
    if (has32) {
        f32x4* qfrag = reinterpret_cast<f32x4*>(L.tail.region);  // [dim_p / 16][64]
        float* lds_qn = L.term;                                  // [16]
        __syncthreads();  // (every wave is done with the byte fragments and terms; without phase 1: nothing to wait for)
        one_nd_stage_queries(p.o.q, B, p.dim, dim_p, qfrag, lds_qn);
        __syncthreads();
        float qn = 0.f;
        if constexpr (!IP) qn = lds_qn[r];
        const int C = dim_p / 16;
        const unsigned voff = (unsigned)(r * dim_p + 4 * g) * 4u;  // this lane's 16 bytes inside a 16-row tile's segment
        const unsigned tile_bytes = 64u * (unsigned)dim_p;         // 16 rows
        VS_IVF_ONE_UNITS_F32(n_units8 + (int)blockIdx.x)
    }

    // (the query fragments are done with: the merges overlay them)
    one_tail<1, KCAP, one_nd_region(64, KCAP)>(p.o, L.tail, ld, li, IvfOneIdMap{p.id_map});  // (64: the shortest row, dim_p = 16)
}

hipError_t launch_ivf_one_scan_u8(const IvfOneU8Params& p, int grid, hipStream_t s) {
    if (!ivf_one_params_ok(p) || grid < 1 || grid > kSlotStride || p.dim_b != nd_dim_b(p.dim) || p.dim_b > 4 * p.dim_p || !p.vecs_u8 ||
        !(p.metric ? p.rsum : p.rterm) || p.bmax < 0 || p.bmax >= kNd8NormLimit || !p.n_units8)
        return hipErrorInvalidValue;
    const int kcap = p.o.k1 <= 8 ? 8 : 16;
    const int lds = one_nd_lds_bytes(4 * p.dim_p, kcap);
    if (kcap == 8)
        return p.metric ? launch_big_lds<ivf_one_scan_u8_kernel<8, true>, kIvfOneMaxLds>(p, grid, lds, s)
                          : launch_big_lds<ivf_one_scan_u8_kernel<8, false>, kIvfOneMaxLds>(p, grid, lds, s);
    return p.metric ? launch_big_lds<ivf_one_scan_u8_kernel<16, true>, kIvfOneMaxLds>(p, grid, lds, s)
                      : launch_big_lds<ivf_one_scan_u8_kernel<16, false>, kIvfOneMaxLds>(p, grid, lds, s);
}

}  // namespace vs
