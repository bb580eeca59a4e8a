// vs_kernels.h -- host-callable launchers of the gfx950 kernels (internal to libvsearch_hip.so).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace vs {

constexpr int kDim = 128;          // SIFT descriptor length; the scan kernels are specialised for it
constexpr int kTileRows = 16;      // base rows per MFMA tile (v_mfma_f32_16x16x4_f32, base = A operand)
constexpr int kScanThreads = 512;  // 8 waves: 2 per SIMD
constexpr int kScanWaves = 8;
constexpr int kMaxBatch = 32;      // queries per scan pass (two 16-query MFMA column blocks)
constexpr int kScanPadRows = 64;  // every row array handed to the scan is allocated with this many spare rows (tile DMAs are not clamped)
constexpr int kSlotStride = 256;   // threshold-exchange slots: [32 queries][256 workgroups]

// Launch of a kernel of kScanThreads threads that takes its parameter block P by value and `lds` <= MAX_LDS bytes of
// dynamic LDS, more than the default limit allows: the kernel's limit is raised once per device (the attribute belongs
// to the device's copy of the code object).
template <auto kfn, int MAX_LDS, class P>
hipError_t launch_big_lds(const P& p, int grid, int lds, hipStream_t s) {
    static bool attr_set[64] = {};
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) dev = 0;
    if (!attr_set[dev]) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kfn), hipFuncAttributeMaxDynamicSharedMemorySize, MAX_LDS);
        if (e != hipSuccess) return e;
        attr_set[dev] = true;
    }
    hipLaunchKernelGGL(kfn, dim3(grid), dim3(kScanThreads), lds, s, p);
    return hipGetLastError();
}

enum ScanMode { kModeTopK = 0, kModeStore = 1, kModeAssign = 2, kModeFilter = 3 };

struct ScanParams {
    const float* base;       // [n_rows][128] row-major (the flat fvecs payload, cpu_baseline.cpp:48-49)
    const float* bnorm;      // [n_rows (+64 pad)] squared norms (cpu_baseline.cpp:116-125)
    const int8_t* base_u8;   // int8 path: [n_rows][128] bytes (x - 128), or nullptr = fp32 path
    const int32_t* rterm;    // int8 path: [n_rows (+64 pad)] ||b||^2 - 256 * sum(b - 128)
    int32_t* invalid;        // int8 path: [n_batches], set to 1 for a batch whose queries are not integers in [0, 255]
    const float* q;          // [n_batches][nq_valid][128] raw queries; rows up to 32 are zero-padded in-kernel (main.cpp:206-211)
    int n_batches;           // query batches served by this one persistent launch (1 for kModeStore)
    int64_t q_batch_stride;  // floats between consecutive batches in q
    float* slots_cur;        // [n_batches][32][kSlotStride] per-workgroup minima (pre-set to +inf) or nullptr = no exchange
    const float* tau0;       // [n_batches][32] bounds computed beforehand by launch_seed (then no exchange, no warm-up), or nullptr
    int k1;                  // the exchange bounds the k1-th best distance; also entries kept per partial list
    int* dbg;                // optional debug counters [grid][16]
    const int32_t* run_if;   // optional [1]: the launch does nothing unless *run_if != 0 (fallback behind a streaming scan)
    int64_t row_begin;       // multiple of 16
    int64_t row_end;         // exclusive
    int tiles_per_wg;
    int metric;              // 0 = L2, 1 = IP (scores negated so that smallest wins)
    int32_t id_offset;       // added to the row number
    int nq_valid;            // queries beyond this are padding
    // kModeTopK outputs: per-workgroup sorted partial lists, query-major (ranked by merge_compact_kernel)
    float* part_d;           // [n_batches][32][kSlotStride][KCAP]
    int32_t* part_i;
    // kModeStore output
    float* store;            // [nq_valid][store_ld], column = row - row_begin
    int64_t store_ld;
    // kModeAssign (k-means): running nearest "query" (centroid) per base row, id = assign_base + batch*32 + column
    float* best_d;           // [n_rows] (pre-set to +inf)
    int32_t* best_i;         // [n_rows] (pre-set to -1)
    int assign_base;
    // kModeFilter (tie resolver): every (row, dist) with dist < tau0[query] is appended to the query's candidate list --
    // the rows select_topk (cpu_baseline.cpp:139-150) can still act on once its buffer maximum is below tau0
    int32_t* f_cnt;          // [32] entries appended per query (pre-set to 0; may exceed f_cap: overflow)
    int32_t* f_row;          // [32][f_cap] row numbers (relative to the index, unordered)
    float* f_d;              // [32][f_cap]
    int f_cap;
};

// Brute-force / coarse scan.  kcap in {8, 16}; nqh = 1 (<=16 queries) or 2.
hipError_t launch_scan(const ScanParams& p, int grid, int kcap, int nqh, int mode, hipStream_t s);

// General-dimension scan (vs_scan_nd.hip): ScanParams as above for kModeTopK / kModeStore / kModeFilter, and
// for kModeAssign with nqh = 2 (any n_batches; the index builder at general dimensions), with rows of dim_p = nd_dim_p(dim) floats ([n_rows + kScanPadRows][dim_p], zero padded) and queries of dim floats
// ([n_batches][nq_valid][dim], unpadded; q_batch_stride in floats).  A preparation launch writes the queries in MFMA
// B-fragment order and their squared norms into the caller's scratch; the fp32 fields of ScanParams are the only ones read.
constexpr int kNdMaxDim = 2048;
constexpr int nd_dim_p(int dim) { return (dim + 15) & ~15; }  // whole 64-byte segments
struct ScanNdParams {
    ScanParams s;
    int dim, dim_p;
    float* qfrag;            // scratch [n_batches][dim_p / 16][2][64][4]: fragment (c, h, lane) = Q[16 h + (lane & 15)][16 c + 4 (lane >> 4) ..]
    float* qnorm;            // scratch [n_batches][32]
};
hipError_t launch_scan_nd(const ScanNdParams& p, int grid, int kcap, int nqh, int mode, hipStream_t s);

// Byte scan of a general index made from uint8 rows (vs_scan_nd_i8.hip): launch_scan_nd's kModeTopK contract
// on s.base_u8 = [n_rows + kScanPadRows][dim_b] bytes (x - 128), dim_b = nd_dim_b(dim), zero padded, with
// s.rterm[n_rows + 64] = sum (b - 128)^2 per row.  The preparation launch writes the byte queries in MFMA B-fragment
// order, qterm = sum (q - 128)^2 per query and s.invalid[batch] (0 or 1): 1 unless every query value of the batch is an
// integer in [0, 255] and max ||q||^2 + bmax <= 2^24; the scan skips such a batch.  Inner product (s.metric == 1, -(q.b)
// ascending like launch_scan_nd): rsum instead of s.rterm, and the per-query term is 128 sum (q - 128) + 128^2 dim, so
// that q.b = q'.b' + 128 (sum q' + sum b') + 128^2 dim in int32; the rule and the verdict are the same.
constexpr int nd_dim_b(int dim) { return (dim + 63) & ~63; }  // whole 64-byte MFMA steps
struct ScanNdI8Params {
    ScanParams s;
    int dim, dim_b;
    int32_t bmax;            // max over the base of ||b||^2, < 2^24
    int8_t* q8frag;          // scratch [n_batches][dim_b / 64][2][64][16]: fragment (s, h, lane) = bytes Q'[16 h + (lane & 15)][64 s + 16 (lane >> 4) ..]
    int32_t* qterm;          // scratch [n_batches][32]
    // inner product (s.metric == 1) only, null otherwise: [n_rows + 64] sum (b - 128) per row (launch_ivf_nd_i8_rowsum)
    const int32_t* rsum;
    // launch_scan_nd_i8_wide only (zero otherwise).  wide_batch: the batch of the prepared scratch (fragments, terms,
    // verdict) that the launch scans.  wide_prepared != 0: an earlier launch on the stream prepared that scratch for
    // these queries, so the preparation launch is left out.  wide_cnt, kModeStore, optional: [2] batches scanned on the
    // byte rows | batches the verdict sent away, counted once per launch.
    int wide_batch, wide_prepared;
    unsigned long long* wide_cnt;
};
constexpr int kNd8Tiles = 4;                          // 16-row tiles per wave block of the byte scans
constexpr int kNd8BlockRows = kNd8Tiles * kTileRows;  // 64 <= kScanPadRows: a block never reads past the spare rows
static_assert(kNd8BlockRows <= kScanPadRows, "row blocks are loaded unclamped");
hipError_t launch_scan_nd_i8(const ScanNdI8Params& p, int grid, int kcap, int nqh, hipStream_t s);
// What launch_scan_nd_i8 refuses; and that check (hipErrorInvalidValue), then its preparation launch for all s.n_batches batches.
bool scan_nd_i8_params_ok(const ScanNdI8Params& p, int grid);
hipError_t launch_nd_prep_i8(const ScanNdI8Params& p, int grid, hipStream_t s);

// Wide-k passes on the byte rows (vs_scan_nd_i8_wide.hip): launch_scan_nd's kModeStore and kModeFilter
// contracts (store / store_ld, or tau0 / f_cnt / f_row / f_d / f_cap; s.run_if is not read) on the byte copy, for one
// batch: batch wide_batch of the prepared scratch.  The launch does nothing when s.invalid[wide_batch] is set -- the
// caller enqueues the fp32 launch behind it with run_if on that word.  Under the exactness rule the distances are
// launch_scan_nd's bits.  kModeStore: store_ld a multiple of 16.  Unless wide_prepared, the preparation launch comes
// first (launch_nd_prep_i8: s.q, s.n_batches, s.q_batch_stride).
hipError_t launch_scan_nd_i8_wide(const ScanNdI8Params& p, int grid, int nqh, int mode, hipStream_t s);

// bf16 prefilter of the fp32 streaming scan (scan_f32f_kernel).  With S = q.b exact, S_fl the fp32 chain of
// scan_f32s_kernel and S' the v_mfma_f32_16x16x32_bf16 sum of q' = bf16(q), b' = bf16(b):
//   |S_fl - S'| <= |S_fl - S| + |S - q'.b'| + |q'.b' - S'|
//               <= g32 ||q|| ||b||  +  (e_q ||b|| + ||q'|| e_b)  +  g16 ||q'|| ||b'||
// with e_x = ||x - x'||.  S - q'.b' = (q - q').b + q'.(b - b') and Cauchy-Schwarz give the middle term.  g32 = 128 u / (1 -
// 128 u), u = 2^-24, is the classic bound of a 128-step fmaf chain (each step rounds once).  bf16 x bf16 products are exact in
// fp32; how the bf16 MFMA accumulates them is not documented, so g16 assumes the worst that is plausible: a unit roundoff
// of 2^-22 (truncation allowed, twice over) per each of the 128 additions.  Shard constants replace ||b||, e_b, ||b'||
// by their maxima.  Holds on well-scaled data only: every value finite and every non-zero magnitude in [2^-60, 2^60],
// so that no product leaves the normal range and flushing subnormals cannot matter (a 2^-100 absolute term covers
// partial sums that cancel into the subnormal range).  The result is rounded up to float.
constexpr double kFiltG32 = 128.0 / 16777216.0 / (1.0 - 128.0 / 16777216.0);
constexpr double kFiltG16 = 128.0 / 4194304.0 / (1.0 - 128.0 / 4194304.0);
constexpr double kFiltLo = 8.673617379884035e-19;  // 2^-60
constexpr double kFiltHi = 1152921504606846976.0;  // 2^60
struct FilterStats {     // per shard, from launch_row_filter_image (index creation)
    double bmax;         // max ||b||
    double emax;         // max ||b - bf16(b)||
    double bpmax;        // max ||bf16(b)||
};
__host__ __device__ inline float filter_bound(double eq, double nq, double nqp, const FilterStats& f) {
    const double nb = f.bmax > f.bpmax ? f.bmax : f.bpmax, nqm = nq > nqp ? nq : nqp;
    const double e = eq * f.bmax + nqp * f.emax + (kFiltG32 + kFiltG16) * nqm * nb + 7.888609052210118e-31;  // + 2^-100
    return (float)(e * (1.0 + 1.0 / 1048576.0));  // (the 2^-20 covers the rounding of the norms and of this cast)
}
// The L2 hot test of scan_f32f_kernel carries the row norm through the C operand of the chain's first MFMA:
// with c0 = -bn / 2 (bn the STORED fp32 norm, the one scan_f32s_kernel tests with; halving is exact on well-scaled rows)
// the accumulator comes out as S'' ~ q'.b' - bn / 2, and the test is S'' > th2.  Claim: every (row, query) that
// scan_f32s_kernel's hot test RN(bn - 2 S_fl) < thr admits is admitted.  Proof: thr is a float and RN is monotone, so the
// old test gives bn - 2 S_fl < thr in the reals, i.e. A := S_fl - bn / 2 > -thr / 2.  The MFMA now sums 129 terms, c0 and the
// 128 exact products, with sum of magnitudes <= ||q'|| ||b'|| + bn / 2 (Cauchy-Schwarz), so under the accumulation
// assumption above, |S'' - (q'.b' - bn / 2)| <= g16c (||q'|| ||b'|| + bn / 2), g16c = 129 u / (1 - 129 u), u = 2^-22.  Hence
//   A - S'' <= |S_fl - q'.b'| + g16c ||q'|| ||b'|| + g16c bn / 2
//           <= E + (g16c - g16) ||q'|| ||b'|| + g16c bnmax / 2      (E = filter_bound: its g16 term is the 128-term one)
//           <= E (1 + 2^-7) + C                                     =: Et
// because E 2^-7 >= 2^-7 (g32 + g16) nqm nb >= 1.25 * 2^-22 nqm nb > (g16c - g16) nqm nb, and C = filter_cnorm(bnmax), a
// constant of the shard: bnmax is its largest stored norm.  So S'' >= A - Et > -thr / 2 - Et >= th2, where filter_th2 forms
// the right-hand side rounded DOWN: in double, -thr / 2 and e (1 + 2^-7) are exact and the two subtractions round by at
// most 2^-53 of a partial sum <= |thr| / 2 + Et each, which the 2^-50 term covers; the cast rounds to nearest (at most
// half an ulp up) and the step to the next float below takes at least that back.  e = +inf (a query outside the
// well-scaled range) or thr = +inf gives -inf: every row passes.
constexpr double kFiltG16C = 129.0 / 4194304.0 / (1.0 - 129.0 / 4194304.0);
__host__ __device__ inline float filter_cnorm(double bnmax) {  // (+ 2^-100 and 2^-20 as in filter_bound: flushed subnormals, this cast)
    return (float)((kFiltG16C * 0.5 * bnmax + 7.888609052210118e-31) * (1.0 + 1.0 / 1048576.0));
}
__host__ __device__ inline float filter_th2(float thr, float e, float cn) {  // thr = stream_l2_thr(tau, ||q||^2)
    const float inf = __builtin_inff();
    if (!(e < inf) || !(cn < inf) || thr == inf) return -inf;
    if (!(thr > -inf)) return inf;  // (nothing is under such a bound; NaN: nothing passes the exact test either)
    const double et = (double)e * (1.0 + 1.0 / 128.0) + (double)cn;
    const double x = -0.5 * (double)thr - et;
    const double y = x - 8.881784197001252e-16 * (0.5 * __builtin_fabs((double)thr) + et);  // 2^-50
    const float f = (float)y;  // finite or -inf: |y| can exceed the float range only downwards (a huge e)
    if (f == -inf) return f;
    const unsigned b = __builtin_bit_cast(unsigned, f);
    return (b << 1) == 0 ? -1.401298464324817e-45f : __builtin_bit_cast(float, f > 0.f ? b - 1 : b + 1);
}

// Bounds for a multi-batch scan, computed up front on a sample of the rows: kSeedWaves 16-row tiles spread evenly
// over the shard, scored against every batch; tau0[batch][q] = next_up of the k1-th smallest of 64 group minima
// (groups of 32 tiles) -- an upper bound of the k1-th best distance, because k1 distinct rows are at least that
// close.  Three small launches per call.
constexpr int kSeedWaves = 2048;  // sample tiles
struct SeedParams {
    const float* base;       // [n_rows (+pad)][128]
    const float* bnorm;
    // optional (launch_seed_sample): the kSeedWaves sample tiles once more, compact and in MFMA A-fragment order -- the seed
    // reads 1 KB per load instruction out of 4 MB (bytes) / 16 MB (fp32) that stay in L2, instead of 64 pieces per
    // instruction scattered over the whole shard (which made the address unit, not the arithmetic, set its 24 us)
    const float* sample_f32;     // [kSeedWaves][8][64][4]   fp32 tile: chunk c, lane (r, g) -> row r, floats 16 c + 4 g ..
    const float* sample_bnorm;   // [kSeedWaves][16]
    const int8_t* sample_u8;     // [kSeedWaves][2][64][16]  byte tile: half, lane (r, g) -> row r, bytes 64 half + 16 g ..
    const int32_t* sample_rterm; // [kSeedWaves][16]
    const int8_t* base_u8;   // optional exact int8 copy (x - 128) + row terms: the seed then runs on v_mfma_i32_16x16x64_i8
    const int32_t* rterm;    //   (16x fewer MFMA cycles) for batches whose queries are byte valued too (q8 / qterm / invalid below are then required)
    int64_t n_rows;
    const float* q;          // [n_batches][nq_valid][128]
    int n_batches;
    int64_t q_batch_stride;
    int nq_valid;
    int metric;
    int k1;
    float* qnorm;            // scratch [n_batches][32]
    float* wmin;             // scratch [n_batches][64 groups][32]
    float* tau0;             // out [n_batches][32]
    int32_t* zero;           // optional: zero_words words cleared by the query-preparation launch (except [16, 48) when `invalid` is set)
    int zero_words;
    // optional outputs of the query-preparation launch for the wide int8 scan (launch_scan_i8_wide): the queries as
    // bytes (x - 128), qterm = ||q||^2 - 256 sum(q - 128) - 2 * 128^3 per query, invalid[batch] = 1 when a query of the
    // batch is not an integer in [0, 255] (pre-set to 0)
    int8_t* q8;              // [n_batches][32][128]
    int32_t* qterm;          // [n_batches][32]
    int32_t* invalid;        // [n_batches]
    // optional: the queries in MFMA B-fragment order for the fp32 streaming scan, qfrag[batch][h][c][lane] = the four floats
    // Q[16 h + (lane & 15)][16 c + 4 (lane >> 4) ..] (zeros for padding queries): a wave's operand load is then 1 KB in one
    // piece (as fragments straight from the row-major queries it is 64 pieces 512 bytes apart per instruction, and eight
    // waves entering a pass kept a CU's address unit busy for 8 us)
    float* qfrag;            // [n_batches][2][8][64][4]
    // optional, with qfrag: the queries rounded to bf16 (RNE) in the B-fragment order of the bf16 prefilter
    // (scan_f32f_kernel): qbf[batch][h][s][lane][j] = Q'[16 h + (lane & 15)][32 s + 16 (j >> 2) + 4 (lane >> 4) + (j & 3)],
    // and per query the bound E of the prefilter (filter_bound with the shard constants below; +inf for a query outside
    // the well-scaled range, 0 for padding)
    uint16_t* qbf;           // [n_batches][2][4][64][8]
    float* qbound;           // [n_batches][32]
    FilterStats fstats;
    int8_t* q8frag;          // [n_batches][2][2][64][16] the byte queries likewise: (h, half, lane) -> bytes [64 half + 16 (lane >> 4) ..] of query 16 h + (lane & 15)
};
hipError_t launch_seed(const SeedParams& p, hipStream_t s);
// gathers the sample tiles of a shard into the compact arrays above (once, at index creation); u8 outputs optional
hipError_t launch_seed_sample(const float* base, const float* bnorm, const int8_t* base_u8, const int32_t* rterm, int64_t n_rows,
                              float* sample_f32, float* sample_bnorm, int8_t* sample_u8, int32_t* sample_rterm, hipStream_t s);

// Wide exact-int8 brute-force scan: ONE pass over the byte rows serves NQH 16-query column blocks = NQH / bpb query
// batches (bpb = 1 for batches of <= 16 queries, else 2), with the bounds of launch_seed in force from the first tile.
// No lane lists, no workgroup merge: a distance under its query's bound is appended to that query's candidate list in
// global memory (a few hundred per query per million rows); launch_merge_flat ranks the lists.  Waves are independent:
// tiles of ALL passes are handed out through one monotonic ticket counter per workgroup, so nothing synchronises
// between batches.
// Where the streaming scans put what they find: wave-private buffers filled with plain stores (positions from a wave
// ballot -- a returning atomic in the tile loop would have to be waited for with vmcnt(0), i.e. drain the tile queue on
// every hit), binned into per-query lists by a small launch after the scan.
struct CandSink {
    int4* wbuf;              // [grid * 8][wcap] x (query = batch * 32 + q, dist bits, id, 0)
    int wcap;
    int32_t* overflow;       // [1] (pre-set to 0): a wave buffer or a query list overflowed -> the launch's fallback kernels
                             //     (brute force: the per-batch scan enqueued behind with run_if = overflow, whose lists the merge
                             //     launch then ranks, MergeParams::run_mode 3) produce the result
    // per-query lists, split into nsub sub-lists (wave buffer w appends to sub-list w % nsub) so that the appending
    // atomics of one query spread over nsub counters
    int32_t* cnt;            // [n_batches][32][nsub] entries per sub-list (pre-set to 0)
    float* cand_d;           // [n_batches][32][nsub][cap]
    int32_t* cand_i;
    int cap;                 // per sub-list
    int nsub;
    int32_t* slow;           // optional [queries]: a query whose lists overflow is marked here instead of raising `overflow`
    // optional (the bf16 prefilter, vs_bf_filter_stats): [1] += 1 by whoever raises `overflow` first in a launch,
    // [2] += candidates the sweep wrote, [3] += candidates the recheck kept -- one atomic instruction per wave, at its end
    unsigned long long* stats;
    // XCD-local sub-lists (0 = off): sub-list = xcd * xcd_subs + hash % xcd_subs (nsub = 8 * xcd_subs) and the counters
    // are sub-list major, cnt[sub * cnt_sub_stride + query]: every counter line and every list is then written by the
    // workgroups of ONE XCD and stays in that XCD's L2 (lines appended to from several XCDs travel between the L2s
    // on every atomic and every store)
    int xcd_subs;
    int cnt_sub_stride;
};

struct WideParams {
    const int8_t* base_u8;   // [n_rows (+64)][128] bytes (x - 128)
    const int32_t* rterm;    // [n_rows + 64]
    int64_t n_rows;
    const int8_t* q8;        // [n_batches][32][128] from launch_seed
    const int8_t* q8frag;    // [n_batches][2][2][64][16] the same in B-fragment order (SeedParams::q8frag)
    const int32_t* qterm;    // [n_batches][32]
    const float* tau0;       // [n_batches][32]
    const int32_t* invalid;  // [n_batches]
    int n_batches, nq_valid, bpb;
    int32_t id_offset;
    CandSink sink;
};
hipError_t launch_scan_i8_wide(const WideParams& p, int grid, int nqh, hipStream_t s);  // nqh in {4, 8}

// Streaming fp32 scan: the arithmetic of scan_kernel (v_mfma_f32_16x16x4_f32 chain in k order, fma(-2, dot, qn + bn)
// epilogue: bit-identical distances), one batch per pass, but organised like the wide int8 scan: bounds from
// launch_seed, queries and their norms straight from global memory, survivors to the CandSink, tiles of all batches
// handed out through one monotonic ticket per workgroup -- no barrier, no workgroup merge, no per-batch prologue.
struct StreamParams {
    const float* base;       // [n_rows (+64)][128]
    const float* bnorm;      // [n_rows + 64]
    int64_t n_rows;
    const float* q;          // [n_batches][nq_valid][128] raw queries
    int64_t q_batch_stride;
    const float* qfrag;      // [n_batches][2][8][64][4] the same queries in B-fragment order (launch_seed)
    const float* qnorm;      // [n_batches][32] from launch_seed
    const float* tau0;       // [n_batches][32]
    int n_batches, nq_valid, metric;
    int32_t id_offset;
    CandSink sink;
    int batches_per_pass;    // scan_f32s_kernel: 1 (HBM bound) or 2 (two batches share a pass over the rows: MFMA bound)
    // the bf16 prefilter (scan_f32f_kernel: one sweep over the rows for all n_batches <= 32) instead, when set:
    // SeedParams::qbf / qbound, and the rows' bf16 image (launch_row_filter_image)
    const uint16_t* qbf;
    const float* qbound;
    const uint16_t* img;     // [n_rows + 64][128] bf16
    int32_t* dbg;            // diagnostic builds only: scan_f32f_kernel's [sweeper][8 waves][16], under either organisation (rows 12288.. of the debug buffer) -- the step split (-DVS_STAMPS) or the waves' start, loop end and end (-DVS_F32F_ENDS)
    float cnorm;             // filter_cnorm of the shard's largest stored norm (the L2 test, filter_th2)
    int f32f_waves;          // scan_f32f_kernel's waves per workgroup: 8, 4 (two workgroups per CU), 0 = the measured choice per launch size
    int f32f_prio;           // 4-wave organisation: steps of every eight (0..8) on which half 1 raises its wave priority, so that the two workgroups of a CU end together; < 0 = the measured choice per shard size
};
hipError_t launch_scan_f32_stream(const StreamParams& p, int grid, hipStream_t s);

// Single-call scan (vs_scan_one.hip): one launch per batch of <= 32 queries, no seed launches, no merge launch -- a lane
// keeps its own sorted lists, a workgroup ranks them into one partial list per query, the workgroup that arrives last
// merges the partial lists.  fp32 rows; k1 <= 16.
struct OneParams {
    const float* base;       // [n_rows (+64)][128]
    const float* bnorm;      // [n_rows + 64]
    int64_t n_rows;
    const float* q;          // [nq_valid][128] raw queries
    int nq_valid, k1, metric;
    int reverse;             // walk the base from its end (calls alternate: see scan_one_kernel)
    int32_t id_offset;
    float* part_d;           // scratch [32][grid][k1]
    int32_t* part_i;
    int32_t* done;           // [1] arrival counter: 0 at launch, left 0 by the last workgroup
    float* out_d;            // [nq_valid][k1] ascending (dist, id), padded with (+inf, -1)
    int32_t* out_i;
    int32_t* flags;          // optional [nq_valid]: 1 = two equal distances among the k1
    int* dbg;                // diagnostic builds (-DVS_STAMPS) only: time stamps [grid][16]
};
int scan_one_grid(int64_t n_rows, int num_cus);
hipError_t launch_scan_one(const OneParams& p, int grid, hipStream_t s);

// The same at any vector length (vs_scan_one_nd.hip): one launch per batch of <= 16 queries on the fp32 rows
// of a general index -- OneParams with base = [n_rows + kScanPadRows][dim_p] (zero padded), q = [nq_valid][dim] unpadded
// (the kernel pads them and works out their norms itself: no preparation launch), nq_valid <= 16, k1 <= 16.  Distances
// are launch_scan_nd's to the bit.  A wave's unit of work is kOneNdUnit rows; scan_one_nd_geometry gives the launch's
// workgroups and the most units any one wave gets (units are dealt statically).
constexpr int kOneNdUnit = 64;
struct OneNdParams {
    OneParams o;
    int dim, dim_p;
};
void scan_one_nd_geometry(int64_t n_rows, int num_cus, int64_t* grid, int64_t* units_per_wave);
hipError_t launch_scan_one_nd(const OneNdParams& p, int grid, hipStream_t s);

// ... and on the byte rows of a general index made from uint8 rows (vs_scan_one_nd_i8.hip): one launch per
// batch of <= 16 queries, k1 <= 16, under either metric.  o.base / o.bnorm are not read; o.q = [nq_valid][dim] unpadded
// floats: every workgroup turns them into bytes, works out the per-query term and reaches nd_prep_i8_kernel's verdict
// itself.  Distances, ids and flags are launch_scan_nd_i8's to the bit; a batch the verdict refuses comes back with ids
// -1, distances +inf and flags = 2 for all nq_valid queries.  Units and geometry: scan_one_nd_geometry.
struct OneNdI8Params {
    OneParams o;
    int dim, dim_b;
    int32_t bmax;            // max over the base of ||b||^2, < 2^24
    const int8_t* base_u8;   // [n_rows + kScanPadRows][dim_b] bytes (x - 128), zero padded
    const int32_t* rterm;    // [n_rows + 64] sum (b - 128)^2 per row (o.metric == 0)
    const int32_t* rsum;     // [n_rows + 64] sum (b - 128) per row (o.metric == 1)
};
hipError_t launch_scan_one_nd_i8(const OneNdI8Params& p, int grid, hipStream_t s);

// Cross-workgroup merge of sorted partial lists -> [nq][kout] + tie flags (+ seed thresholds).
struct MergeParams {
    const float* part_d;     // [G][nq_stride][kin]
    const int32_t* part_i;
    int G;
    int nq_stride;           // queries per partial block (32 for scan partials)
    int kin;
    int nq;                  // queries to produce
    int kout;                // entries to write per query (<= kin)
    float* out_d;            // [nq][kout] or nullptr
    int32_t* out_i;
    int32_t* flags;          // [nq] or nullptr: adjacent equal distances among the first kout
    float* tau_out;          // [32] or nullptr: nextafter(kout-th best) used as scan seed
    const int32_t* id_map;   // optional: out id = id_map[id] (IVF reorder_to_original)
    int q_group_out, q_group_in;  // output query q reads input query (q / out) * in + q % out (0 = identity)
    const int32_t* invalid;  // optional [nq / q_group_out]: batches skipped by the int8 scan -> flags = 2
    int flag_empty;          // flags = 2 for a query with no finite entry at all (cross-GPU merge: every shard skipped its batch)
    const int32_t* shard_flags;  // optional (cross-GPU merge): shard g's own flag of output query q at g * shard_flags_stride + q;
    int64_t shard_flags_stride;  //   a shard that skipped the query's batch (flag 2) makes the merged flag 2: its rows are missing
    const int32_t* run_if;   // optional [1] with run_mode: 1 = run only if *run_if != 0, 2 = only if *run_if == 0 (the other
    int run_mode;            //   launch of the pair writes the outputs); 3 (launch_merge_layout, compacting merge only) = one launch
                             //   for both: *run_if == 0 ranks the lists above, *run_if != 0 the alternative lists below
    const float* alt_part_d;     // run_mode 3: sorted lists, entry (g, q, j) at g * alt_stride_g + q * alt_stride_q + j, g < alt_G,
    const int32_t* alt_part_i;   //   j < alt_kin (no flat_len); everything else -- outputs, grouping, invalid, flags -- is shared
    int alt_G, alt_kin;
    int64_t alt_stride_g, alt_stride_q;
    const int32_t* flat_len; // optional [queries][G]: list (q, g) holds flat_len[q * G + g] <= kin UNSORTED candidates
    int flat_len_sub_stride; // != 0: the lengths are list major instead, flat_len[g * flat_len_sub_stride + q]
    int32_t* dbg;            // diagnostic builds (-DVS_STAMPS) only
};
hipError_t launch_merge(const MergeParams& p, hipStream_t s);  // scan-partial layout [G][nq_stride][kin]
// general layout: entry (g, q, j) at g*stride_g + q*stride_q + j
hipError_t launch_merge_layout(const MergeParams& p, int64_t stride_g, int64_t stride_q, hipStream_t s);
// Which kernel launch_merge_layout runs for G lists of kin entries (host only; the launch itself goes through this):
// 0 = the compacting merge (G*kin <= cap), else the LPT of the merge_kernel instantiation (1, 2, 4 .. 64: lists per
// thread), -1 = no kernel (G*kin > cap and G > kMergeMaxLists).  cap / track: kCompactCap / kMergeTrack (vs_merge.h).
constexpr int kMergeMaxLists = 16384;
int merge_plan(int G, int kin, int* cap, int* track);

// Wide top-k (vs_topk_wide.hip): per query, the k1 <= kTopkWideMax smallest 64-bit keys (order-preserving bits of the
// distance) << 32 | id out of a dense score block and / or up to two candidate lists -- i.e. the k1 best by (dist, id).
// Radix select over the keys with LDS histograms (8-bit digits, most significant first) until the entries at or below the
// selected prefix fit in LDS, then one compaction and a bitonic sort of those.  Non-finite distances are treated like
// merge_compact_kernel does: +inf and NaN never enter an output (slots past the finite entries are (+inf, -1)).
constexpr int kTopkWideMax = 129;   // k1 = k + 1 for k <= 128
struct TopkList {
    const float* d;          // entry e of query q at d[q * stride_q + e]
    const int32_t* i;        // ids (negative: padding, skipped)
    int64_t stride_q;
    const int32_t* cnt;      // optional [nq]: entries of query q (more than cap: the launch's overflow word is raised)
    int cap;                 // entries per query (cnt == nullptr: all of them)
    int32_t id_add;          // added to every id read from i
};
struct TopkWideParams {
    const float* dense;      // optional form (b): [nq][dense_ld] scores, column c has id dense_id0 + c
    int64_t dense_ld;        // a multiple of 4
    int64_t n_dense;         // columns per query
    int32_t dense_id0;
    TopkList list[2];        // form (a): list[0..n_list) (unsorted)
    int n_list;
    int nq;                  // queries with outputs; blocks [nq, gridDim.x) only write tau_out = -inf
    int k1;
    float* out_d;            // [nq][out_ld] ascending (dist, id), padded with (+inf, -1)
    int32_t* out_i;
    int64_t out_ld;
    int32_t* flags;          // optional [nq]: 1 = two equal finite distances among the k1 outputs
    float* tau_out;          // optional [gridDim.x]: next_up(k1-th best), +inf when there are fewer, -inf for blocks >= nq
    int32_t* zero;           // optional: zero_words words cleared by block 0 (before anything reads them: not an input)
    int zero_words;
    int32_t* overflow;       // optional [1]: set to 1 when a list count exceeds its cap
    const int32_t* run_if;   // optional [1]: the launch does nothing unless *run_if != 0
    int grp_out, grp_in;     // grp_out > 0: several batches in one launch.  Block q writes output q as before and reads
                             //   the dense row, the lists and cnt of query (q / grp_out) * grp_in + q % grp_out; overflow
                             //   is then [ceil(nq / grp_out)], one word per batch.  0: every index is q, one overflow word
};
hipError_t launch_topk_wide(const TopkWideParams& p, int grid, hipStream_t s);

// One Lloyd update: deterministic fixed-point cluster sums -> new centroids; shift[c] = ||new - old||^2.
hipError_t launch_kmeans_update(const float* x, const int32_t* assign, int64_t rows, int nlist, float* cents,
                                unsigned long long* acc, int32_t* counts, double* shift, hipStream_t s);

// k-means++ seeding (Arthur & Vassilvitskii D^2 sampling; sklearn's KMeans default init, create_ivf_model_reordered.py:
// 97-103).  Step c: d2[i] = min(d2[i], ||x_i - cents[c-1]||^2) with per-block sums, then the row where the running sum
// of d2 passes u * total becomes cents[c].  Two launches per centre, no host round trip.
hipError_t launch_kpp_step(const float* x, const float* xnorm, int64_t rows, float* cents, int c, float* d2, double* block_sums,
                           int n_blocks, double u, hipStream_t s);
constexpr int kKppBlockRows = 1024;
// The builder's update and seeding step at any dimension 1 <= dim <= kNdMaxDim (vs_ivf_build_nd): rows [rows][ld], ld =
// nd_dim_p(dim), zero padded; cents / acc [nlist][dim].  Same fixed-point sums, same D^2 rule and block sums.
hipError_t launch_kmeans_update_nd(const float* x, int64_t ld, int dim, const int32_t* assign, int64_t rows, int nlist, float* cents,
                                   unsigned long long* acc, int32_t* counts, double* shift, hipStream_t s);
hipError_t launch_kpp_step_nd(const float* x, int64_t ld, const float* xnorm, int64_t rows, int dim, float* cents, int c, float* d2,
                              double* block_sums, int n_blocks, double u, hipStream_t s);

// ||v||^2 per row in the reference's AVX2 summation order (cpu_baseline.cpp:95-114).
hipError_t launch_row_sqnorm(const float* v, int64_t rows, int dim, float* out, hipStream_t s);
hipError_t launch_row_sqnorm_ld(const float* v, int64_t rows, int dim, int64_t ld, float* out, hipStream_t s);  // rows ld floats apart
// shard constants of the bf16 prefilter: out[0..2] = max of ||b||^2, ||b - bf16(b)||^2, ||bf16(b)||^2 as double bits,
// out[3] = 1 when a row is not well scaled (FilterStats), out[4] = max of bnorm[row] (the stored fp32 norms, optional) as
// double bits; the five words of out must be zeroed before.  The same pass writes the rows'
// bf16 image for scan_f32f_kernel when img is given: img[row][8 (4 s + g) + 4 u + i] = bf16(v[row][32 s + 16 u + 4 g + i])
// (round to nearest even, the rounding the statistics are taken from), s, g < 4, u < 2, i < 4: 16-byte chunk 4 s + g of
// a row is lane (row & 15, g)'s A fragment of k-step s.  Rows [rows, rows + kScanPadRows) of img are the caller's to zero.
hipError_t launch_row_filter_image(const float* v, const float* bnorm, int64_t rows, unsigned long long* out, uint16_t* img, hipStream_t s);

// ---- IVF ----
// Per query: the nprobe nearest centroids (ascending (dist, id)) out of a [B][ld] score matrix.
hipError_t launch_pick_probes(const float* scores, int64_t ld, int B, int nlist, int nprobe,
                              int32_t* probes /*[B][nprobe]*/, hipStream_t s);

constexpr int kIvfMaxProbe = 256;

// Multi-batch IVF launches: blockIdx.y = batch.  Per-batch pointers point at batch 0's copy; batch y's coarse scores lie
// y * slab bytes, its probes y * probes bytes, its queries y * q bytes further on.
struct IvfMulti {
    long long slab, probes, q;
};

// What the coarse / pick kernels of the wide pipeline do beside scores and probes (every pointer optional)
struct IvfGroup {
    IvfMulti mb;                     // batch y's slab (coarse scores, probes) lies mb.slab bytes, its queries mb.q bytes further on
    int sb_batches;                  // batches per super-batch (<= kIvfWideBatches)
    // the coarse kernel also prepares the queries for the int8 paths (block x = 0 of every batch)
    float* w_qnorm;                  // [n_batches][32] ||q||^2
    int8_t* w_q8;                    // [n_batches][32][128] queries as bytes (x - 128)
    int32_t* w_qterm;                // [n_batches][32]
    int32_t* w_invalid;              // [n_batches]: a query of the batch is not byte valued (written as 0 or 1)
    int32_t* w_overflow;             // [1]: cleared (the wide pipeline's candidate-buffer overflow word)
    int32_t* w_glist;                // [1]: cleared (count of the ranking's left-over list, see launch_ivf_wide_rank)
    // the pick kernel also enters every (query, probe) pair in its list's slot table
    int32_t* w_cnt;                  // [n_sb][ivf_wide_plan_words] pair counters (pre-set to 0), list c's at word c * kIvfWideCntStride
    int32_t* w_lq;                   // [n_sb][nlist][w_q] slots: 128 * (slot of the query in its super-batch)
    int w_q;
    // ... and enters the query in the bound tables of its two nearest lists that hold rows (ivf_bounds_list_body)
    int32_t* w_tq;                   // [nlist][w_tq_cap] entries: query of the launch group | segment << 16
    int w_tq_cap;
    int32_t* w_tcnt;                 // list c's entry counter at word c * kIvfWideCntStride + 1 (pre-set to 0)
    int32_t* w_nseg;                 // [n_batches][32] segments the query has (0..kBoundSegs)
    const int32_t* t_offsets;        // [nlist + 1] extents of the rows the bounds are taken from
    int32_t* dbg;                    // diagnostic builds (-DVS_STAMPS) only: time stamps of the pick kernel
};

// Coarse stage: Q x C^T + L2 epilogue on MFMA into scores [n_batches][32][ld] (ld >= nlist rounded up to 64; batch y's
// copy lies grp.mb.slab bytes further on), then the nprobe nearest lists per query (nlist <= kIvfFastNlist).
constexpr int kIvfFastNlist = 4096;
hipError_t launch_ivf_coarse_pick(const float* q, int B, const float* cents, const float* cnorm, int nlist, int nprobe,
                                  int metric, float* scores, int ld, int32_t* probes, const IvfGroup& grp, hipStream_t s,
                                  int n_batches = 1);
hipError_t launch_ivf_prep_queries(const float* q, int B, const float* cents, const float* cnorm, int nlist, const IvfGroup& grp,
                                   hipStream_t s, int n_batches);
hipError_t launch_ivf_fill(const int32_t* gathered, long long blk_words, int B, int nprobe, int nlist, const int32_t* offsets,
                           int32_t* probes_out, float* tau_out, int32_t* slow_out, const IvfGroup& grp, hipStream_t s, int n_batches);

// ---- wide IVF pipeline: launch groups are cut into super-batches of kIvfWideBatches batches (<= 1024 queries) that
// share ONE list-major pass: a list probed by any of them is read once and scored against all its queries (MFMA
// column blocks of 16).  Bounds first (ivf_bounds_plan_kernel, list-major too: the k-th best among the first rows of the
// query's two nearest lists), survivors to a CandSink, ranking by a wave per query -- no candidate-score arrays, no
// selection kernel.
constexpr int kIvfWideBatches = 32;  // batches per super-batch at most: every resident list is read once per 1024 queries
constexpr int kIvfWideQ = kIvfWideBatches * kMaxBatch;  // query slots per super-batch
#ifndef VS_BOUND_SEGS
#define VS_BOUND_SEGS 2
#endif
constexpr int kBoundSegs = VS_BOUND_SEGS;               // lists a query takes its bound from (list-major bounds; <= 4)
#ifndef VS_TAU_ROWS
#define VS_TAU_ROWS 256
#endif
constexpr int kIvfTauRows = VS_TAU_ROWS;                 // rows of a list that seed its queries' bounds (a multiple of 64)
#ifndef VS_WIDE_UNIT
#define VS_WIDE_UNIT 32
#endif
constexpr int kIvfWideUnit = VS_WIDE_UNIT;  // rows per unit of the wide scan's plan (lists are padded to multiples of it)
constexpr int kIvfWideCntStride = 32;
constexpr long long ivf_wide_plan_words(int nlist) { return (long long)nlist * kIvfWideCntStride + 16; }
struct IvfWideParams {
    const float* vecs;        // [n_rows (+64)][128] cluster-reordered
    const float* vnorm;       // [n_rows + 64]
    const int8_t* vecs_u8;    // optional exact int8 copy (x - 128) + row terms
    const int32_t* rterm;
    // the scan's own copy: lists padded to multiples of 32 rows ("padded rows"), 16-row tiles [half][chunk][row][16 B]
    const int8_t* vecs_t8;
    const int32_t* nrh_t;     // [padded rows + 64] -(rterm >> 1): the MFMA C operand
    const int32_t* rterm_t;
    const int32_t* tdelta;    // [nlist] padded row - row (null: 0)
    const int32_t* chunk_trow0;  // [n_chunks] first padded row of a chunk: the plan's records and the candidates are padded rows
    const int32_t* offsets;   // [nlist+1] local list offsets (lists not resident here are empty)
    const int32_t* chunk_list;
    const int32_t* chunk_row0;
    const int32_t* chunk_rows;
    int n_chunks, nlist, nprobe, k, metric;
    const float* q;           // batch b's [B][128] at (char*)q + b * q_batch_bytes
    long long q_batch_bytes;
    int n_batches, B;
    int sb_batches;           // batches per super-batch (<= kIvfWideBatches): super-batch sb = batches [sb * sb_batches, ...)
    const float* qnorm;       // [n_batches][32]   | from ivf_coarse_mfma_kernel
    const int8_t* q8;         // [n_batches][32][128]
    const int32_t* qterm;     // [n_batches][32]
    const int32_t* invalid;   // [n_batches] (pre-set to 0) a query of the batch is not byte valued
    const int32_t* probes;    // batch b's [B][nprobe] at (char*)probes + b * probes_batch_bytes
    long long probes_batch_bytes;
    int32_t* lq;              // [n_sb][nlist][kIvfWideQ] slot tables: 128 * ((batch % 32) * 32 + q) of the queries probing each list
                              //   (= where the scan's LDS keeps the query), padded to a multiple of 16 entries with the dummy slot
    int32_t* zero;            // [n_sb][ivf_wide_plan_words(nlist)] (pre-set to 0): list c's pair counter at word c * kIvfWideCntStride
                              //   (a 128-byte line each: the pick kernel's atomics come from all XCDs), the super-batch's record
                              //   count at word nlist * kIvfWideCntStride
    unsigned long long* cand_count;  // optional: += rows the probed lists hold per (query, probe) pair
    int32_t* units;           // [n_sb][units_cap][4] records (first row, chunk end, list, first slot | end slot << 16)
    long long units_sb_stride;  // in int32 (= 4 units_cap)
    int units_cap;            // records per super-batch the plan may hold (>= the index's units: the unsplit plan fits)
    // bounds, list-major: entries of the pick kernel (see IvfGroup), entry counter of list c at zero[c * kIvfWideCntStride + 1]
    const int32_t* tq;        // [nlist][tq_cap]
    int tq_cap;
    float* tk;                // [n_batches][32][kBoundSegs][16] the k smallest distances per (query, segment), ascending
    const int32_t* nseg;      // [n_batches][32]
    int tau_inline;           // the scan works a query's bound out of tk / nseg itself (no ivf_tau_combine_kernel launch, tau unused)
    float* tau;               // [n_batches][32] bounds
    int32_t* slow;            // [n_batches][32] (pre-set to 0): no bound could be had -> exact slow path
    CandSink sink;
    float* out_d;             // [n_batches][B][k]   (slow path writes here directly)
    int32_t* out_i;
    const int32_t* id_map;    // reorder_to_original (local), by row: the slow path's
    int32_t* dbg;             // diagnostic builds (-DVS_STAMPS) only: per-workgroup time stamps, dbg[0..] see ivf_scan_wide_kernel
    int diag;                 // diagnostic builds only: bit 0 no column blocks, bit 1 every unit = the wave's first, bit 2 no binning
};
hipError_t launch_ivf_wide_bounds_plan(const IvfWideParams& p, hipStream_t s, int what = 3);  // bounds (what & 1) and the plan (what & 2), one launch
hipError_t launch_ivf_wide_scan(const IvfWideParams& p, int num_cus, hipStream_t s);  // the list-major scan
int ivf_wide_grid_x(int num_cus, int n_sb);  // grid.x of the scan
int ivf_wide_waves(int num_cus, int n_sb);   // its waves = candidate buffers
// merge of the candidate lists (flat layout, see launch_merge_layout) or the exact slow path, per query
// glist (optional): 1 + queries int32 words; with it launches of more than 2048 queries rank one query per wave and leave the
// few that need a workgroup to a second launch (the list's count, word 0, is cleared by the next group's coarse / prep kernel)
hipError_t launch_ivf_wide_rank(const MergeParams& m, int64_t stride_g, int64_t stride_q, const IvfWideParams& p, hipStream_t s,
                                int32_t* glist = nullptr);
// wide k (17 <= k <= kIvfWideKMax, p.tau_inline = 0): the pipeline above with another bound and another ranking.
// Bounds + plan: the bounds launch stores every (query, segment) distance to p.tk ([queries][kBoundSegs][kIvfTauRows], left
// at +inf by the ranking), topk_wide_kernel selects the k smallest per query into kth_d / kth_i ([queries][k]), and the
// k-th becomes p.tau (or p.slow).  The ranking: the k smallest (dist, row) per query over its candidate sub-lists, or over
// every row of its probed lists for a slow query or an overflowed group; ids through id_map; the counters left zeroed.
constexpr int kIvfWideKMax = 128;
hipError_t launch_ivf_widek_bounds_plan(const IvfWideParams& p, float* kth_d, int32_t* kth_i, hipStream_t s);
hipError_t launch_ivf_widek_rank(const IvfWideParams& p, const int32_t* id_map, unsigned long long* stats, hipStream_t s);

struct IvfScanParams {
    const float* vecs;        // [n_rows][128] cluster-reordered (vectors_reordered.npy)
    const float* vnorm;       // [n_rows]
    const int32_t* offsets;   // [nlist+1] (cluster_offsets.npy)
    const uint8_t* owned;     // [nlist] 1 = this shard scans the list, or nullptr = all
    const float* q;           // [B][128] raw queries (norms are computed in-kernel)
    const int32_t* probes;    // [B][nprobe]
    int B, nprobe, kcap;
    int metric;
    float* part_d;            // [B][nprobe][kcap]
    int32_t* part_i;          // reordered row positions
    unsigned long long* cand_count;  // total rows scanned (IVFIndex::searchBatch return value)
};
hipError_t launch_ivf_scan(const IvfScanParams& p, hipStream_t s);

// ---- list-major IVF scan of a general index (vs_ivf_nd.hip): a launch group of group_q <= kIvfNdGroupQ
// queries (batches back to back, [group_q][dim]) whose probes are known.  launch_ivf_nd_plan prepares the queries
// (zero-padded rows + squared norms in nd_prep_kernel's order), inverts probes[group_q][nprobe] into per-list runs of
// slots (query << 8 | probe rank) and cuts the runs of the non-empty lists into items of up to 16 slots;
// launch_ivf_nd_scan scores every item's list against its slots' queries (scan_nd_kernel's accumulation chain: a distance
// is the number the brute-force general scan returns for that row and query) and writes the item's sorted top-kcap by
// (distance, row) per slot to part[(query * nprobe + rank) * kcap] -- the layout ivf_fallback_batch_dev ranks.
// IvfNdParams::metric == 1 (inner product): the "distance" everywhere below is the score -(q.v), the same chain negated.
constexpr int kIvfNdGroupQ = 1024;     // 32 batches of 32 queries
constexpr int kIvfNdSlotBlock = 16;    // slots per item: one MFMA column block
constexpr long long ivf_nd_items_cap(int nlist, int nprobe) {  // every probed list ends in one ragged item at most
    return (long long)kIvfNdGroupQ * nprobe / kIvfNdSlotBlock + ((long long)kIvfNdGroupQ * nprobe < nlist ? (long long)kIvfNdGroupQ * nprobe : nlist);
}
struct IvfNdParams {
    const float* vecs;        // [n_rows + kScanPadRows][dim_p] cluster-reordered, zero padded
    const float* vnorm;       // [n_rows + 64]
    const int32_t* offsets;   // [nlist + 1]
    int nlist, dim, dim_p;
    const float* q;           // [group_q][dim] raw queries
    int group_q, nprobe, k, kcap;
    const int32_t* probes;    // [group_q][nprobe] (-1: none)
    float* qrows;             // scratch [kIvfNdGroupQ][dim_p]
    float* qnorm;             // scratch [kIvfNdGroupQ]
    int32_t* list_cnt;        // scratch [2][nlist]: pairs per list, fill cursors (cleared by the plan's first launch)
    int32_t* list_start;      // scratch [nlist + 1] first slot of every list's run
    int32_t* slots;           // scratch [group_q * nprobe]
    int32_t* items;           // scratch [ivf_nd_items_cap][2] (list, first slot)
    int32_t* n_items;         // scratch [1]
    float* part_d;            // [group_q][nprobe][kcap] (pairs without an item: (+inf, -1))
    int32_t* part_i;          // reordered row positions
    unsigned long long* cand_count;  // += rows of every probed list, per (query, probe) pair
    // the per-query route of an index that keeps two plans per group (vs_ivf_create_nd_u8): a pair gets a slot in this
    // plan only when route[query] == route_want.  Null: every pair, as on a vs_ivf_create index.
    const int32_t* route;     // [group_q]
    int route_want;
    unsigned long long* pair_count;  // += pairs that got a slot in this plan (null: not counted)
    // the rescan plan of the wide-k pipeline (vs_ivf_nd_wide.hip): a pair gets a slot only when pair_mask[pair] != 0.
    // Null: every pair, as everywhere else.
    const int32_t* pair_mask; // [group_q * nprobe]
    // 0: squared L2.  1: inner product -- a row's score is -(q.v), the accumulation chain negated, smallest first; vnorm
    // and qnorm are not read, and a row past its list's end is left out by its row number in every epilogue (a spare
    // row scores -0.0 and would beat every row with a negative product).
    int metric;
};
hipError_t launch_ivf_nd_plan(const IvfNdParams& p, hipStream_t s);
// a group's second plan (p.route or p.pair_mask set): the pair counts, prefix and fill of launch_ivf_nd_plan on p's own
// plan tables -- no query preparation, no preset of the partial lists, no candidate count (the first plan's launches did
// those), and p's list_cnt cleared by the caller's earlier launch (launch_ivf_nd_i8_prep, launch_ivf_nd_wide_bound)
hipError_t launch_ivf_nd_plan_second(const IvfNdParams& p, hipStream_t s);
hipError_t launch_ivf_nd_scan(const IvfNdParams& p, int grid, hipStream_t s);

// ---- the single-call IVF search of a general index (vs_ivf_one_nd.hip): one batch of o.nq_valid <= 16
// queries, o.k1 = k <= 16 results each (k entries, not k + 1), nlist <= kIvfOneMaxNlist, in TWO launches on one stream.
// launch_ivf_one_coarse scores the centroid table (launch_scan_nd's kModeStore numbers, to the bit) and its last
// workgroup writes the probes (launch_pick_probes' table), the unit table -- every probed list that holds rows cut into
// units of unit_rows rows with the 16-bit mask of the query columns that probe it -- and the counts;
// launch_ivf_one_scan scores the units (ivf_scan_nd_kernel's distances, to the bit) and its last workgroup writes
// out_d / out_i [nq_valid][k] by (distance, position), ids through id_map, (+inf, -1) in empty slots.  No memset, no
// preparation launch, no merge launch; both tickets are zero between launches.
constexpr int kIvfOneMaxNlist = 1024;  // lists the coarse launch's selection is built for: a wave keeps a query's scores in registers, 16 per lane
constexpr int kIvfOneUnitRows = 512;   // rows per unit of the scan: one 64-row block for each of a workgroup's 8 waves
struct IvfOneParams {
    OneParams o;              // q = [nq_valid][dim] raw queries, nq_valid, k1 = k, part_d / part_i = [16][grid][k] scratch of the
                              // scan launch, done = the scan launch's ticket, out_d / out_i; base, bnorm, n_rows, reverse, id_offset, flags unused
    const float* vecs;        // [n_rows + kScanPadRows][dim_p] cluster-reordered, zero padded
    const float* vnorm;       // [n_rows + 64]
    const int32_t* offsets;   // [nlist + 1]
    const float* cents;       // [nlist + kScanPadRows][dim_p]
    const float* cnorm;       // [nlist + 64]
    const int32_t* id_map;    // [n_rows] position -> output id (null: the position)
    int nlist, dim, dim_p, nprobe, metric;
    int unit_rows;            // a multiple of 64
    float* scores;            // scratch [16][ld]
    int64_t ld;
    int32_t* probes;          // [nq_valid][nprobe] (-1: fewer valid scores than nprobe)
    int32_t* units;           // scratch [units_cap][4]: first row, end row, column mask, list
    int units_cap;
    int32_t* n_units;         // scratch [1]
    int32_t* ticket;          // [1] the coarse launch's arrival counter: 0 at launch, left 0
    unsigned long long* counters;    // [2] batches answered | the most units of any one of them
    unsigned long long* cand_count;  // += rows of every probed list, per (query, probe) pair
    unsigned long long* pair_count;  // optional: += pairs whose list holds rows (what ivf_nd_count adds for an fp32 plan)
};
int ivf_one_coarse_grid(int nlist, int num_cus);
int ivf_one_scan_grid(int num_cus);
hipError_t launch_ivf_one_coarse(const IvfOneParams& p, int grid, hipStream_t s);
hipError_t launch_ivf_one_scan(const IvfOneParams& p, int grid, hipStream_t s);

// ---- the same two launches on a general IVF index that keeps a byte copy of its rows (vs_ivf_create_nd_u8).
// The coarse launch (vs_ivf_one_nd.hip, its byte-index mode) scores and selects as above; its last workgroup also reaches
// launch_ivf_nd_i8_prep's verdict for every query of the batch (every value an integer in [0, 255] and ||q||^2 + bmax <=
// 2^24, in integers) and cuts every probed list that holds rows into BYTE units (unit_rows8 rows, column mask = the
// probing queries that qualify) and FP32 units (s.unit_rows rows, column mask = the others), each kind only when its
// mask is non-zero: units [0, n_units8) are byte units, [n_units8, n_units) fp32 units.  The scan launch
// (vs_ivf_one_nd_i8.hip) scores the byte units with v_mfma_i32_16x16x64_i8 -- (float)(qterm + rterm - 2 q'.b'), or
// -(float)(q.b) under inner product: the fp32 scan's bits for such a query -- and then the fp32 units as
// launch_ivf_one_scan does, into the same lane lists; one tail.
#ifndef VS_IVF_ONE_U8_UNIT_ROWS  // (a build with EXTRA=-DVS_IVF_ONE_U8_UNIT_ROWS=2048 is the other side of the unit-size measurement)
#define VS_IVF_ONE_U8_UNIT_ROWS 512
#endif
constexpr int kIvfOneU8UnitRows = VS_IVF_ONE_U8_UNIT_ROWS;  // rows per byte unit (measured against 2048: DESIGN 4.6e)
struct IvfOneU8Params : IvfOneParams {  // counters = [3] batches answered | of those with both kinds of unit | the most units of
                                        // any one; pair_count = the pairs of the queries that do not qualify (fp32 rows)
    const int8_t* vecs_u8;    // [n_rows + kScanPadRows][dim_b] bytes (x - 128), zero padded
    const int32_t* rterm;     // [n_rows + 64] sum (b - 128)^2 (squared L2)
    const int32_t* rsum;      // [n_rows + 64] sum (b - 128) (inner product; launch_ivf_nd_i8_rowsum)
    int dim_b;                // nd_dim_b(dim)
    int32_t bmax;             // max over the rows of ||b||^2, < 2^24
    int unit_rows8;           // a multiple of 64
    int32_t* n_units8;        // scratch [1]
    unsigned long long* pair_count8;  // optional: += pairs of the qualifying queries whose list holds rows
};
hipError_t launch_ivf_one_coarse_u8(const IvfOneU8Params& p, int grid, hipStream_t s);
hipError_t launch_ivf_one_scan_u8(const IvfOneU8Params& p, int grid, hipStream_t s);
bool ivf_one_params_ok(const IvfOneParams& p);

// ---- the same on the byte copy of a general IVF index made from uint8 rows (vs_ivf_nd_i8.hip).
// launch_ivf_nd_i8_prep writes the group's queries as int8 (x - 128), zero padded, row-major [group_q][dim_b], qterm =
// sum (q - 128)^2 and valid[query]: 1 when the query runs on bytes -- every value an integer in [0, 255] and ||q||^2 +
// bmax <= 2^24, checked in integers (nd_prep_i8_kernel's rules, per query) -- and 0 otherwise or when all_f32 is set; it
// also clears s.list_cnt.  s is the byte plan (route = valid, route_want = 1); the caller's fp32 plan takes route_want =
// 0 on the same words.  launch_ivf_nd_i8_scan scores the byte plan's items with v_mfma_i32_16x16x64_i8 and writes
// (float)(qterm + rterm - 2 q'.b') -- the integer the fp32 scan computes exactly for such a query -- into the shared
// partial lists; a pair has one writer.
struct IvfNdI8Params {
    IvfNdParams s;            // vecs / vnorm / qrows / qnorm are not read
    const int8_t* vecs_u8;    // [n_rows + kScanPadRows][dim_b] bytes (x - 128), zero padded
    const int32_t* rterm;     // [n_rows + 64] sum (b - 128)^2
    int dim_b;                // nd_dim_b(dim)
    int32_t bmax;             // max over the rows of ||b||^2, < 2^24
    int all_f32;              // vs_set_precision(1): no query runs on bytes
    int8_t* q8rows;           // scratch [kIvfNdGroupQ][dim_b]
    int32_t* qterm;           // scratch [kIvfNdGroupQ]
    int32_t* valid;           // scratch [kIvfNdGroupQ]
    // inner product (s.metric == 1) only, null otherwise: q.b = q'.b' + 128 (qsum + rsum) + 128^2 dim in int32, exact
    // and equal to the fp32 chain for a valid query (every partial sum of q.b is at most (||q||^2 + ||b||^2) / 2 <=
    // 2^23); the scan writes -(float)(q.b)
    const int32_t* rsum;      // [n_rows + 64] sum (b - 128) (launch_ivf_nd_i8_rowsum)
    int32_t* qsum;            // scratch [kIvfNdGroupQ] sum (q - 128), written by launch_ivf_nd_i8_prep
};
hipError_t launch_ivf_nd_i8_prep(const IvfNdI8Params& p, hipStream_t s);
hipError_t launch_ivf_nd_i8_scan(const IvfNdI8Params& p, int grid, hipStream_t s);
// rsum[row] = the sum of the row's dim_b stored bytes (the padding is zero) for row < rows, 0 for the 64 spare entries
// (also ScanNdI8Params::rsum: the inner-product brute-force byte index builds it with this launch at creation)
hipError_t launch_ivf_nd_i8_rowsum(const int8_t* vecs_u8, int dim_b, int64_t rows, int32_t* rsum, hipStream_t s);

// ---- wide k (17 <= k <= kIvfNdWideKMax) on a general IVF index (vs_ivf_nd_wide.hip).  The group's first
// plan and scan run as above at kcap 16 on the fp32 rows with every pair; part[(query * nprobe + rank) * 16] then holds
// each probed list's 16 best by (distance, row).
//   launch_ivf_nd_wide_bound : tau[query] = the k-th smallest finite distance among the query's partial lists (+inf when
//       there are fewer than k).  A pair whose 16th entry is finite and <= tau is saturated: its list may hold more rows
//       at or under tau, pair_mask = 1.  Every other pair has all its rows at or under tau in its partial list already;
//       those entries go to the query's candidate list as keys (tw_key of vs_wide_select.h) and pair_mask = 0.  Also
//       clears r.list_cnt, the rescan plan's counters.
//   launch_ivf_nd_plan_second(r) with r.pair_mask : the rescan plan, over the saturated pairs only.
//   launch_ivf_nd_wide_scan  : ivf_scan_nd_kernel's item loop and accumulation chain on the rescan plan; no lane lists,
//       no merge: every real row of a real slot with d <= tau[query] and d < +inf is appended to the query's list (no
//       slack: the same chain computed tau).  Entries past kIvfNdWideCand are dropped, cnt keeps counting.
//   launch_ivf_nd_wide_rank  : per query, the k smallest keys of its list, ids through id_map; a query whose list
//       overflowed is ranked over every row of its probed lists instead, each distance recomputed by one thread in the
//       MFMA's order (segments of 16 floats ascending, i = 0..3, g = 0..3, element 16 c + 4 g + i, one fma each: bit-
//       identical).  Leaves cnt[query] = 0 and adds to stats: candidates ranked from lists, the most of one query (max),
//       queries ranked by the fallback.
constexpr int kIvfNdWideKMax = 128;
constexpr int kIvfNdWideCand = 8192;   // keys per query
struct IvfNdWideParams {
    IvfNdParams r;            // the rescan plan: the first plan's fields with tables of its own and pair_mask set
    float* tau;               // [kIvfNdGroupQ]
    int32_t* pair_mask;       // [group_q * nprobe] (= r.pair_mask)
    int32_t* cnt;             // [kIvfNdGroupQ] (zero between groups)
    unsigned long long* cand; // [kIvfNdGroupQ][kIvfNdWideCand]
    const int32_t* id_map;    // reorder_to_original
    float* out_d;             // [group_q][k]
    int32_t* out_i;
    unsigned long long* stats;  // [3]
};
hipError_t launch_ivf_nd_wide_bound(const IvfNdWideParams& p, hipStream_t s);
hipError_t launch_ivf_nd_wide_scan(const IvfNdWideParams& p, int grid, hipStream_t s);
hipError_t launch_ivf_nd_wide_rank(const IvfNdWideParams& p, hipStream_t s);

}  // namespace vs
