// vs_ivf_nd_f16.hip -- the list-major IVF scan of a general index whose rows are IEEE binary16 (vs_ivf_create_nd_f16,
// gfx950), 1 <= dim <= 2048, squared L2 or inner product, k <= 16.
//
//   ivf_scan_nd_f16_kernel<KCAP, IP> : ivf_scan_nd_kernel's contract and organisation -- a fixed grid of 512-thread
//                     workgroups loops over the item table of launch_ivf_nd_plan; an item is one list and up to 16 slots;
//                     the 8 waves take the list's 64-row blocks round-robin; a wave keeps 4 x 1 accumulators of
//                     v_mfma_f32_16x16x4_f32 (rows = A operand, the slot's padded query row gathered as B); a lane keeps
//                     one sorted list per slot and vs_scan_tail.h's workgroup merge takes them to the item's top-KCAP by
//                     (distance, row) -- on the half rows, which are the index's only row storage.
//
// Kernel contract: a half widens to fp32 exactly (v_cvt_f32_f16; fp16 denormals are on, the target's default, so a
// subnormal half becomes the normal float it names), and every (row, query) chain runs scan_nd_kernel's order of segment,
// lane group and element on the widened operands, then fma(-2, dot, qn + bn) or -dot.  A distance is therefore the number
// ivf_scan_nd_kernel returns on the rows widened to float, to the bit: the steps the wider padding adds (dim_h = dim
// rounded up to 32, against 16) multiply zeros by zeros and leave a chain as it was.
//
// Row side.  Rows are stored [n_rows + kScanPadRows][dim_h] in the permuted 32-half blocks of DESIGN 4.4g
// (nd_f16_layout_kernel): one 16-byte load per lane, tile and K step of 32 elements delivers both 4-float pieces.  Loads
// are unclamped (a list may start at any row; the spare rows cover its last block), row stride 2 dim_h bytes.
//
// Ring.  This kernel carries one query block where scan_nd_f16_kernel carries up to two, and spends the registers on
// depth: a ring of kIvfNdhRing sets, each the rows of one K step (4 tiles x 4 VGPRs) AND that step's two query pieces
// (8 VGPRs), filled kIvfNdhRing - 1 steps ahead of the MFMAs that read them and unrolled by the ring's length, so no set
// is ever copied.  The query pieces ride in the ring rather than one step ahead as in scan_nd_f16_kernel: vmcnt retires
// loads in issue order, so a wait for a query piece issued at step s would also wait for every row load issued before
// it -- with the pieces one step ahead no row load could stay in flight for more than two steps, whatever the ring's
// depth.  Inside a step the query pieces are issued before the rows, the set's oldest loads.  The group's query rows come
// from ivf_nd_prep with dim_p = dim_h, so the gathered loads walk 32-float steps without a tail step.
// The depth comes from the compiler's resource report (profiles/ivf_nd_f16_resources.txt): see kIvfNdhRing.
//
// No nontemporal hint on the row loads: a list is read again by every item that probes it, and with the hint the list
// scan measured 1.7 to 11 % slower (384 and 768-d, 1 M rows, profiles/ivf_nd_f16_bench.txt).  -DVS_IVF_ND_F16_NT builds
// that other form.
//
// Left for later, deliberately: wide k (17 <= k <= 128) and a short-call (two-launch) scan on half rows -- the index
// refuses the first and sends short calls through the group route.
#include "vs_kernels.h"
#include "vs_dev.h"
#include "vs_scan_tail.h"

namespace vs {

constexpr int kIvfNdhTiles = 4;                             // 16-row tiles per wave block
constexpr int kIvfNdhBlockRows = kIvfNdhTiles * kTileRows;  // 64 <= kScanPadRows: a block never reads past the spare rows
static_assert(kIvfNdhBlockRows <= kScanPadRows, "row blocks are loaded unclamped");
static_assert(kIvfNdSlotBlock == kTileRows, "an item is one MFMA column block");
// Sets in the ring (a set is 24 VGPRs).  Four: 3 K steps of rows and query pieces in flight per wave, 168 to 192 VGPRs of
// the 256 an 8-wave workgroup may use, no scratch.  A fifth set still fits (199 to 216 VGPRs, no scratch;
// profiles/ivf_nd_f16_resources.txt has both reports) and measured 0.1 to 1.6 % slower on the list scan at 384
// and 768-d (profiles/ivf_nd_f16_bench.txt), with a longer conditional tail for short rows: four it is.
#ifndef VS_IVF_ND_F16_RING
#define VS_IVF_ND_F16_RING 4  // (-DVS_IVF_ND_F16_RING=5 builds the deeper ring for the measurement)
#endif
constexpr int kIvfNdhRing = VS_IVF_ND_F16_RING;

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));

template <int KCAP, bool IP>
__global__ __launch_bounds__(kScanThreads, 1) void ivf_scan_nd_f16_kernel(const IvfNdF16Params pn) {
    const IvfNdParams& p = pn.s;
    constexpr int T = kIvfNdhTiles, R = kIvfNdhRing, D = R - 1;
    __shared__ NdTailLds tail;

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r = lane & 15, g = lane >> 4;
    const int dim_h = pn.dim_h;
    const unsigned voff = (unsigned)(r * dim_h + 8 * g) * 2u;  // this lane's 16 bytes inside a 16-row tile's 64-byte segment
    const unsigned tile_bytes = 32u * (unsigned)dim_h;         // 16 rows
    const int n_steps = dim_h >> 5;                            // K steps of 32 elements (>= 1)
    const int n_items = p.n_items[0];

#pragma clang loop unroll(disable)
    for (int item = blockIdx.x; item < n_items; item += gridDim.x) {
        const int list = p.items[2 * item], slot0 = p.items[2 * item + 1];
        const int n_slots = min(kIvfNdSlotBlock, p.list_start[list + 1] - slot0);
        const int64_t row_lo = p.offsets[list], row_end = p.offsets[list + 1];
        const int64_t last_row = row_end - 1;
        const int blocks_total = (int)((row_end - row_lo + kIvfNdhBlockRows - 1) / kIvfNdhBlockRows);
        const int sv = p.slots[slot0 + (r < n_slots ? r : 0)];  // (a slot past the run's end repeats the first: discarded below)
        const int qi = sv >> 8;
        float qn = 0.f;
        if constexpr (!IP) qn = p.qnorm[qi];
        // this lane's 16 bytes of a 64-byte segment of its slot's padded query row (dim_p == dim_h floats)
        const char* qb = reinterpret_cast<const char*>(p.qrows + (int64_t)qi * dim_h + 4 * g);
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
            const int64_t row0 = row_lo + (int64_t)wb * kIvfNdhBlockRows;
            // "uniform base + 32-bit lane offset" addressing: one address register serves every row load of the block
            const char* sb = reinterpret_cast<const char*>(pn.vecs_f16 + row0 * (int64_t)dim_h);
            f32x4 acc[T];
#pragma unroll
            for (int t = 0; t < T; ++t) acc[t] = (f32x4){0.f, 0.f, 0.f, 0.f};
            // the ring: set (s % R) holds K step s -- per tile the lane's 8 halves (both segments), and the two query pieces
            f16x8 a[R][T];
            f32x4 b[R][2];
            auto load_set = [&](int s, f16x8 (&av)[T], f32x4 (&bv)[2]) __attribute__((always_inline)) {
                bv[0] = *reinterpret_cast<const f32x4*>(qb + 128u * s);
                bv[1] = *reinterpret_cast<const f32x4*>(qb + 128u * s + 64u);
#pragma unroll
                for (int t = 0; t < T; ++t) {
                    const f16x8* src = reinterpret_cast<const f16x8*>(sb + (t * tile_bytes + 64u * s) + voff);
#ifdef VS_IVF_ND_F16_NT
                    av[t] = __builtin_nontemporal_load(src);
#else
                    av[t] = *src;
#endif
                }
            };
            // K step s on set CUR; the set of step s + D is filled first.  AHEAD: step s + D exists, so its loads are issued
            // without a test (a conditional load makes the compiler wait for everything in flight where the paths join).
            // Segment 2 s, then 2 s + 1; inside a segment scan_nd_kernel's order (i, tile): four independent chains between
            // two MFMAs of one chain
            auto k_step = [&](int s, auto cur, auto ahead) __attribute__((always_inline)) {
                constexpr int CUR = decltype(cur)::value, FILL = (CUR + D) % R;
                if (decltype(ahead)::value || s + D < n_steps) load_set(s + D, a[FILL], b[FILL]);
                __builtin_amdgcn_sched_barrier(0);  // the loads stay in front of this step's MFMAs
#pragma unroll
                for (int u = 0; u < 2; ++u) {
                    float w[T][4];
#pragma unroll
                    for (int t = 0; t < T; ++t)
#pragma unroll
                        for (int i = 0; i < 4; ++i) w[t][i] = (float)a[CUR][t][4 * u + i];  // exact
#pragma unroll
                    for (int i = 0; i < 4; ++i)
#pragma unroll
                        for (int t = 0; t < T; ++t) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(w[t][i], b[CUR][u][i], acc[t], 0, 0, 0);
                }
            };
            // R consecutive steps from s (a multiple of R) on sets 0 .. R - 1; the tail form stops at the row's last step
            auto k_round = [&](int s, auto ahead) __attribute__((always_inline)) {
                k_step(s, std::integral_constant<int, 0>{}, ahead);
                if (decltype(ahead)::value || s + 1 < n_steps) {
                    k_step(s + 1, std::integral_constant<int, 1 % R>{}, ahead);
                    if (decltype(ahead)::value || s + 2 < n_steps) {
                        k_step(s + 2, std::integral_constant<int, 2 % R>{}, ahead);
                        if (decltype(ahead)::value || s + 3 < n_steps) {
                            k_step(s + 3, std::integral_constant<int, 3 % R>{}, ahead);
                            if constexpr (R == 5)
                                if (decltype(ahead)::value || s + 4 < n_steps) k_step(s + 4, std::integral_constant<int, 4 % R>{}, ahead);
                        }
                    }
                }
            };
            static_assert(R == 4 || R == 5, "k_round is written out for these ring lengths");
            load_set(0, a[0], b[0]);
#pragma unroll
            for (int j = 1; j < D; ++j)
                if (j < n_steps) load_set(j, a[j], b[j]);
            int s = 0;
#pragma clang loop unroll(disable)
            for (; s + R - 1 + D < n_steps; s += R) k_round(s, std::true_type{});
            // the last 1 .. 2 R - 2 steps
            k_round(s, std::false_type{});
            if (s + R < n_steps) k_round(s + R, std::false_type{});

            const bool ragged = row0 + kIvfNdhBlockRows - 1 > last_row;  // wave-uniform
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

hipError_t launch_ivf_nd_f16_scan(const IvfNdF16Params& pn, int grid, hipStream_t s) {
    const IvfNdParams& p = pn.s;
    if (grid < 1 || p.k < 1 || p.k > p.kcap || !pn.vecs_f16 || p.dim < 1 || p.dim > kNdMaxDim || pn.dim_h != nd_dim_h(p.dim) ||
        p.dim_p != pn.dim_h)
        return hipErrorInvalidValue;
    if (p.metric != 0 && p.metric != 1) return hipErrorInvalidValue;
    if (p.kcap == 8 && !p.metric)
        hipLaunchKernelGGL((ivf_scan_nd_f16_kernel<8, false>), dim3(grid), dim3(kScanThreads), 0, s, pn);
    else if (p.kcap == 16 && !p.metric)
        hipLaunchKernelGGL((ivf_scan_nd_f16_kernel<16, false>), dim3(grid), dim3(kScanThreads), 0, s, pn);
    else if (p.kcap == 8)
        hipLaunchKernelGGL((ivf_scan_nd_f16_kernel<8, true>), dim3(grid), dim3(kScanThreads), 0, s, pn);
    else if (p.kcap == 16)
        hipLaunchKernelGGL((ivf_scan_nd_f16_kernel<16, true>), dim3(grid), dim3(kScanThreads), 0, s, pn);
    else
        return hipErrorInvalidValue;
    return hipGetLastError();
}

}  // namespace vs
