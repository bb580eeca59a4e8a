// vs_api.hip -- C ABI of libvsearch_hip.so: index objects, device memory, launch orchestration.
//
// One vs_index owns: the base (or cluster-reordered) vectors and their squared norms in HBM,
// a small scratch arena (padded queries, thresholds, per-workgroup partial lists, result
// staging) and a HIP stream.  Nothing here computes distances on the host: without a HIP device
// every create/search call fails (VS_ERR_DEVICE).
#include <hip/hip_runtime.h>
#include <dlfcn.h>
#include <rccl/rccl.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <numeric>
#include <atomic>
#include <string>
#include <thread>
#include <vector>

#include "../../include/vsearch.h"
#include "vs_host.h"
#include "vs_kernels.h"
#include "vs_res.h"

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

constexpr int kMaxEvents = 8192;
constexpr int kKcapMax = 16;       // largest per-lane list the scan kernels are compiled for
constexpr int kMaxNprobe = 256;
constexpr int kMaxLanes = 4;
constexpr int kMaxMulti = 32;  // batches per persistent scan launch
constexpr int kOneMaxBatches = 4;  // calls of fewer batches take one single-call scan launch per batch (fp32 rows)
constexpr int kOneMaxQueries = 16;  // ... when a batch holds at most this many queries
constexpr int kPairMinTiles = 96;
constexpr int kIvfGroupDefault = 256; // batches per launch group of an unsharded IVF index (VSEARCH_IVF_GROUP): 46 us per 1024 queries against 79 with groups of 32
constexpr int kIvfGroupMax = 256;     // ... at most (8 super-batches of 32): also the group of an index sharded 8 ways
constexpr int kIvfShardMaxWorld = 16; // ranks the cluster-sharded pipeline is compiled for (one super-batch per rank)
constexpr int64_t kIvfHostChunk = 4 * 32 * 32;  // queries per chunk of the host-buffer IVF call (one upload, one download)
constexpr int kWideLanesMax = 4;  // streams (and scratch sets) the launch groups of one wide IVF call may be dealt to
constexpr int kWideWaveCap = 1024;  // entries per wave buffer of the wide int8 scan (expected fill: about 100 per launch)
constexpr int kWideSub = 16;      // sub-lists per query of the streaming scans' candidate lists
constexpr int kWideCap = 128;     // entries per sub-list (2048 per query; more: the per-batch scan behind takes over)
constexpr int kIvfWideWaveCap = 512;  // entries per wave buffer of the wide IVF scan (expected fill: a few dozen per group)
constexpr int kIvfWideSubCap = 256;   // entries per candidate sub-list (16 per query: 4096 candidates)
// wide k (17 <= k <= 128): candidates per query grow about in proportion to k (DESIGN.md 4.6b has the measured fill)
constexpr int kIvfWideKWaveCap = 32768;  // entries per wave buffer (more in one wave: the group is ranked exactly)
constexpr int kIvfWideKSubCap = 1024;   // entries per candidate sub-list (more: the query is ranked exactly)
constexpr int kTieDense = 4096;   // rows whose distances the tie resolver takes densely
constexpr int kTieCap = 8192;     // candidate slots per flagged query (more: full-row fallback)
constexpr int kTopwFilterCap = 8192;  // filter candidates per query of the wide-k launcher (more: the dense fallback)
constexpr int64_t kTopwChunkBytes = (int64_t)256 << 20;  // score scratch of the wide-k dense fallback ([32][chunk] floats)

struct ProfSlot {
    std::vector<vs::Event> ev;  // pairs
    int used = 0;
};

double now_ms() {
    using namespace std::chrono;
    return duration<double, std::milli>(steady_clock::now().time_since_epoch()).count();
}

}  // namespace

struct vs_index {
    int kind = 0;  // 0 = brute force, 1 = IVF
    int device = 0;
    int dim = 0;
    // general index (vs_bf_create_nd with dim != 128, or VSEARCH_ND_FORCE): rows of dim_p = nd_dim_p(dim) floats, zero padded,
    // scanned by scan_nd_kernel; no int8 copy, no seed sample, no bf16 filter statistics.  Otherwise dim_p == dim == 128.
    // General IVF index (kind 1; vs_ivf_create / vs_ivf_load with dim != 128, or VSEARCH_IVF_ND_FORCE): rows and centroids
    // laid out the same way, searched by the list-major general scan (ivf_group_nd_dev); no tiled copy, no head rows, no
    // chunk table, and no int8 copy unless the rows came as uint8 (vs_ivf_create_nd_u8: the byte fields below, scanned by
    // ivf_scan_nd_i8_kernel for the queries that qualify).
    bool general = false;
    int dim_p = 0;
    bool nd_one = true;  // general brute-force index: short calls on the fp32 rows take scan_one_nd_kernel (VSEARCH_ND_ONE=0 at creation: off)
    bool nd_one_u8 = true;  // ... and short calls on its byte rows scan_one_nd_i8_kernel (VSEARCH_ND_ONE_U8=0 at creation: off)
    int64_t one_stat[2] = {0, 0};  // single-call launches enqueued on the fp32 rows | on the byte rows (vs_bf_one_stats; host side)
    bool nd_wide_u8 = true;  // ... and wide k (k >= 16) runs its bulk passes on the byte rows (VSEARCH_ND_WIDE_U8=0 at creation: off)
    int64_t wide_batches = 0;  // wide batches enqueued on this index, on any route (vs_bf_wide_stats; host side)
    vs::DevBuf<float> d_nd_qfrag;  // [kMaxMulti][dim_p / 16][2][64][4] scratch of launch_scan_nd
    vs::DevBuf<float> d_nd_qnorm;  // [kMaxMulti][32]
    // general index made from uint8 rows (vs_bf_create_nd_u8, vs_bf_create_nd_u8_metric): the rows once more as int8
    // (x - 128), scanned by scan_nd_i8_kernel for k <= 15 under the index's metric.  Absent when max ||b||^2 >= 2^24: no batch could ever run on it.
    bool nd_from_u8 = false;
    int dim_b = 0;                   // dim rounded up to 64 bytes
    int32_t nd_bmax = 0;             // max ||b||^2 over the base (< 2^24)
    vs::DevBuf<int8_t> d_nd_u8;      // [n_rows + 64][dim_b], zero padded
    vs::DevBuf<int32_t> d_nd_rterm;  // [n_rows + 64] sum (b - 128)^2 (squared L2 indexes)
    vs::DevBuf<int32_t> d_nd_rsum;   // [n_rows + 64] sum (b - 128) (inner-product indexes, vs_bf_create_nd_u8_metric)
    vs::DevBuf<int8_t> d_nd_q8frag;  // [kMaxMulti][dim_b / 64][2][64][16] scratch of launch_scan_nd_i8
    vs::DevBuf<int32_t> d_nd_qterm;  // [kMaxMulti][32]
    vs::DevBuf<unsigned long long> d_wide_cnt;  // brute force: [2] wide batches scanned on the byte rows | sent to the fp32 rows by their verdict
    vs::DevBuf<unsigned long long> d_nd_stats;  // general IVF index from uint8 rows: (query, probe) pairs planned on bytes | on fp32
    int metric = VS_METRIC_L2;
    int64_t n_rows = 0;   // rows resident on this GPU
    int64_t n_total = 0;  // rows of the whole (unsharded) index
    int64_t id_offset = 0;
    int batch = vs::kMaxBatch;
    int num_cus = 256;

    vs::DevBuf<float> d_vecs;   // [n_rows + 64][128] (general index: [n_rows + 64][dim_p])
    vs::DevBuf<float> d_norm;   // [n_rows + 64]
    // the bf16 prefilter of the fp32 streaming scan (scan_f32f_kernel): shard constants, whether every row is well
    // scaled (otherwise the index keeps scan_f32s_kernel), and the rows once more as bf16 in A-fragment order, which is
    // what that kernel sweeps (launch_row_filter_image; present exactly when filter_ok: +256 bytes per row)
    vs::FilterStats fstats{};
    float filter_cnorm = 0.f;  // vs::filter_cnorm of the largest stored norm: the L2 test's shard constant (vs::filter_th2)
    bool filter_ok = false;
    // vs_bf_filter_stats: [1] launches that overflowed, [2] candidates of the sweeps, [3] survivors of the recheck (device
    // counters, allocated with the image), and the prefilter launches made (counted where they are enqueued)
    vs::DevBuf<unsigned long long> filter_stats;
    int64_t filter_launches = 0;
    vs::DevBuf<uint16_t> d_img;  // [n_rows + 64][128], spare rows zero
    // int8 data path: only when every base value is an integer in [0, 255]
    vs::DevBuf<int8_t> d_vecs_u8;   // [n_rows][128] bytes (x - 128)
    vs::DevBuf<int32_t> d_rterm;    // [n_rows + 64] ||b||^2 - 256 * sum(b - 128)
    // the seed's sample tiles, compact and in MFMA fragment order (SeedParams::sample_*; brute-force indexes)
    vs::DevBuf<float> d_seed_f32;
    vs::DevBuf<float> d_seed_bnorm;
    vs::DevBuf<int8_t> d_seed_u8;
    vs::DevBuf<int32_t> d_seed_rterm;
    // wide IVF scan: the byte rows once more, every list padded to a multiple of 32 rows ("padded rows") and stored as
    // 16-row MFMA tiles of 2 KB, [half of the row][16-byte chunk][row][16 bytes] -- a wave's A-operand load is then 1 KB
    // of consecutive bytes (from the row-major copy the same load touches 16 B in each of 64 places)
    vs::DevBuf<int8_t> d_vecs_t8;   // [n_padded + 64 rows]
    vs::DevBuf<int32_t> d_nrh_t;    // [n_padded + 64] -(rterm >> 1) by padded row: the MFMA C operand
    vs::DevBuf<int32_t> d_rterm_t;  // [n_padded + 64]
    vs::DevBuf<int32_t> d_r2o_t;    // [n_padded + 64] padded row -> original id (-1: padding)
    vs::DevBuf<int32_t> d_tdelta;   // [nlist] padded row - row, per list
    vs::DevBuf<int32_t> d_chunk_trow0;  // [n_chunks] first padded row of a chunk
    vs::DevBuf<int32_t> d_invalid;  // [kMaxMulti] batches the int8 scan had to skip
    int precision = 0;             // 0 = auto (int8 when possible), 1 = fp32, 2 = int8

    // IVF
    int nlist = 0;
    int rank = 0, world = 1;
    vs::DevBuf<float> d_centroids;  // [nlist][128]
    vs::DevBuf<float> d_cnorm;      // [nlist + 16]
    vs::DevBuf<int32_t> d_offsets;  // [nlist + 1] offsets into the LOCAL d_vecs (non-owned lists are empty)
    vs::DevBuf<int32_t> d_r2o;      // [n_rows] local position -> original id
    std::vector<int32_t> h_offsets_global;  // as loaded (for save / stats)
    double avg_cluster_size = 0;

    // scratch
    vs::DevBuf<float> d_q;        // staging for host queries [kMaxMulti * 32][dim]
    // Pipeline lanes: consecutive batches of a multi-batch call run on different internal streams
    // so that the start-up / tail of one scan overlaps the streaming phase of its neighbours
    // (inside one launch all workgroups go through those phases in lock-step and HBM idles).
    struct Lane {
        vs::Stream s;
        vs::Event done_ev;
        vs::DevBuf<float> slots;     // [kMaxMulti][32][kSlotStride] threshold-exchange slots, reset per launch
        vs::DevBuf<int> done;        // [kMaxMulti] arrival counters, reset per launch
        vs::DevBuf<float> part_d;    // [kMaxMulti][32][kSlotStride][16]
        vs::DevBuf<int32_t> part_i;
        vs::DevBuf<float> seed_qnorm; // [kMaxMulti][32]   scratch of launch_seed
        vs::DevBuf<float> qfrag;      // [kMaxMulti][2][8][64][4] queries in MFMA B-fragment order (fp32 streaming scan)
        vs::DevBuf<int8_t> q8frag;    // [kMaxMulti][2][2][64][16] byte queries in B-fragment order (wide int8 scan)
        vs::DevBuf<uint16_t> qbf;     // [kMaxMulti][2][4][64][8] bf16 queries in B-fragment order (bf16 prefilter)
        vs::DevBuf<float> qbound;     // [kMaxMulti][32] the prefilter's error bound per query
        vs::DevBuf<float> seed_wmin;  // [kMaxMulti][kSeedWaves][32]
        vs::DevBuf<float> tau0;       // [kMaxMulti][32]   bounds of the current multi-batch launch
        // wide int8 scan (several batches per pass over the rows): prepared queries + per-query candidate lists (ensure_wide)
        struct Wide8 {
            vs::DevBuf<int8_t> q8;        // [kMaxMulti][32][128]
            vs::DevBuf<int32_t> qterm;    // [kMaxMulti][32]
            vs::DevBuf<int32_t> wcnt;     // [16] (word 0: overflow) + [kMaxMulti][32][kWideSub]
            vs::DevBuf<float> wcand_d;    // [kMaxMulti][32][kWideCap]
            vs::DevBuf<int32_t> wcand_i;
            vs::DevBuf<int4> wbuf;        // [256 * 8][kWideWaveCap] wave-private candidate buffers of the scan
            bool ready = false;           // every buffer above allocated
        } wide8;
    };
    Lane lane[kMaxLanes];
    int n_lanes = 1;
    vs::Event fork;
    vs::DevBuf<float> d_out_d;    // [kMaxMulti * 32][kTopkWideMax]
    vs::DevBuf<int32_t> d_out_i;
    vs::DevBuf<int32_t> d_flags;  // [kMaxMulti * 32]
    vs::DevBuf<float> d_scores;   // IVF query-major fallback: coarse scores [32][nlist_pad]
    vs::DevBuf<int32_t> d_probes; // [32][kMaxNprobe]
    vs::DevBuf<float> d_ipart_d;  // [32][kMaxNprobe][16]
    vs::DevBuf<int32_t> d_ipart_i;
    vs::DevBuf<unsigned long long> d_cand;
    // list-major IVF scan (grouped path)
    vs::DevBuf<int32_t> d_chunk_list;   // [n_chunks] (list, 1024-row chunk) work items over the resident lists
    vs::DevBuf<int32_t> d_chunk_row0;
    vs::DevBuf<int32_t> d_chunk_rows;
    int ivf_gb = 32;                   // batches per launch group (multiple of 32) the wide pipeline's scratch is sized for
    int ivf_nsb = 1;                   // ... in at most this many super-batches (sharded: one per rank)
    int ivf_lanes = 2;                 // streams the launch groups of one device call are dealt to
    int64_t ivf_host_cap = 0;          // queries per chunk the host-buffer call's staging slots hold
    // sharded index: the first kIvfTauRows rows of EVERY list (resident or not), replicated on every rank: a query's bound
    // then comes from its two nearest lists wherever they live -- the bounds of the unsharded index (a bound from the
    // nearest RESIDENT lists of an eighth of the lists let ten times the candidates through)
    vs::DevBuf<float> d_head_vecs;      // [head rows + 64][128], lists packed
    vs::DevBuf<float> d_head_norm;      // [head rows + 64]
    vs::DevBuf<int32_t> d_head_off;     // [nlist + 1]
    vs::DevBuf<int8_t> d_head_t8;       // byte-valued heads: 16-row tiles, every list padded to a multiple of 16 rows
    vs::DevBuf<int32_t> d_head_rterm_t;
    vs::DevBuf<int32_t> d_head_tdelta;  // [nlist] padded row - row
    vs::DevBuf<int32_t> d_sh;           // host-buffer brute force (bf_search_shards): the owner's gathered scratch (see ShBuf)
    vs::PinBuf<char> pin_sh;            // ... and the tie resolver's pinned downloads
    vs::DevBuf<int32_t> sl_blk[2];      // sliced IVF pipeline (ivf_sliced_groups): the owner's gathered blocks / top-k lists, per lane
    vs::DevBuf<int32_t> sl_lists[2];
    // wide IVF pipeline (a launch group of up to 32 batches shares one list-major pass): slot tables, zeroed counters,
    // plans, bounds, prepared queries, candidate sink
    struct IvfWide {
        vs::DevBuf<int32_t> lq;      // [ivf_nsb][nlist][kIvfWideQ]
        vs::DevBuf<int32_t> zero;    // one zeroed block per launch group (see wide_zero)
        size_t zero_words = 0;
        vs::DevBuf<int32_t> units;   // [n_sb_max][units_cap][4]
        int units_cap = 0;
        vs::DevBuf<float> tau;       // [1024]
        vs::DevBuf<int32_t> tq;      // [nlist][group queries] bound tables (ivf_bounds_list_body)
        vs::DevBuf<float> tk;        // [group queries][kBoundSegs][16]
        vs::DevBuf<int32_t> nseg;    // [group queries]
        vs::DevBuf<float> qnorm;     // [1024]
        vs::DevBuf<int8_t> q8;       // [1024][128]
        vs::DevBuf<int32_t> qterm;   // [1024]
        vs::DevBuf<int4> wbuf;       // [waves][kIvfWideWaveCap]
        int n_waves = 0;
        vs::DevBuf<float> cand_d;    // [1024][16][kIvfWideSubCap]
        vs::DevBuf<int32_t> rank_list;   // groups of more than 2048 queries: [0] count, [1..] the queries the wave-per-query ranking left over
        vs::DevBuf<int32_t> cand_i;
        bool dirty = false;         // the zeroed block may hold a failed call's counts: memset before the next group
        vs::DevBuf<char> slab;       // per batch: probes [32][kMaxNprobe] | coarse scores [32][nlist padded]
        long long slab_stride = 0, off_scores = 0;
        bool ready = false;         // every buffer above allocated (ensure_ivf_wide)
    } wide[kWideLanesMax];          // scratch sets: consecutive launch groups of one call run on different streams
    // wide k (17 <= k <= 128), per lane beside `wide`, allocated on the first such call: the segments' distances, their k
    // smallest, a larger candidate sink
    struct IvfWideK {
        vs::DevBuf<float> tk;        // [group queries][kBoundSegs][kIvfTauRows] (+inf between groups)
        vs::DevBuf<float> kth_d;     // [group queries][128]
        vs::DevBuf<int32_t> kth_i;
        vs::DevBuf<int4> wbuf;       // [waves][kIvfWideKWaveCap]
        vs::DevBuf<float> cand_d;    // [group queries][16][kIvfWideKSubCap]
        vs::DevBuf<int32_t> cand_i;
        bool ready = false;          // every buffer above allocated (ensure_ivf_widek)
    } widek[kWideLanesMax];
    vs::DevBuf<unsigned long long> widek_stats;  // [4] (VSEARCH_IVF_WIDEK_STATS=1 only): see vs_ivf_widek_stats
    // general IVF index: scratch of one launch group of up to kIvfNdGroupQ queries (vs::IvfNdParams; ensure_ivf_nd)
    struct IvfNd {
        int np_max = 0;              // probes per query the buffers hold: min(kMaxNprobe, nlist)
        vs::DevBuf<int32_t> probes;  // [kIvfNdGroupQ][np_max]
        vs::DevBuf<float> qrows;     // [kIvfNdGroupQ][dim_p]
        vs::DevBuf<float> qnorm;     // [kIvfNdGroupQ]
        vs::DevBuf<int32_t> plan;    // list_cnt [2][nlist] | list_start [nlist + 1] | n_items [1]
        vs::DevBuf<int32_t> slots;   // [kIvfNdGroupQ * np_max]
        vs::DevBuf<int32_t> items;   // [ivf_nd_items_cap(nlist, np_max)][2]
        vs::DevBuf<float> part_d;    // [kIvfNdGroupQ][np_max][kKcapMax]
        vs::DevBuf<int32_t> part_i;
        // an index with a byte copy (vs_ivf_create_nd_u8): the byte plan's tables and the byte queries
        vs::DevBuf<int32_t> plan8, slots8, items8;  // as plan / slots / items
        vs::DevBuf<int8_t> q8rows;   // [kIvfNdGroupQ][dim_b]
        vs::DevBuf<int32_t> qterm;   // [kIvfNdGroupQ]
        vs::DevBuf<int32_t> valid;   // [kIvfNdGroupQ] 1: the query runs on bytes
        bool ready = false;          // every buffer above allocated
    } ivfnd;
    // ... and what a short call (ivf_one_route) needs instead of the plan tables, allocated by the index's
    // first such call (ensure_ivf_one)
    struct IvfOne {
        vs::DevBuf<float> scores;    // [16][nlist padded to 64] the coarse launch's scores
        vs::DevBuf<int32_t> probes;  // [16][min(kMaxNprobe, nlist)] the batch's probes (pick_probes' table)
        vs::DevBuf<int32_t> units;   // [units_cap][4] first row, end row, column mask, list
        int units_cap = 0;
        vs::DevBuf<float> part_d;    // [16][kSlotStride][kKcapMax] one partial list per workgroup and query
        vs::DevBuf<int32_t> part_i;
        vs::DevBuf<int32_t> words;   // [0] the coarse launch's ticket | [1] the scan launch's | [2] units of the batch in flight |
                                     // [3] of those, byte units (the byte route)
        vs::DevBuf<unsigned long long> counters;  // [2]: see vs_ivf_one_stats | [3]: see vs_ivf_one_u8_stats
        bool ready = false;          // every buffer above allocated
    } ivfone;
    bool ivf_one = true;  // general IVF index: short calls take the two-launch route (VSEARCH_IVF_ONE=0 at creation: off)
    // ... and on an index with a byte copy the byte route.  VSEARCH_IVF_ONE_U8 at creation: 0 = off, 2 = the
    // byte route at every shape of ivf_one_route, the shapes ivf_one_route_u8 takes out included (the measurement's leg)
    int ivf_one_u8 = 1;
    // ... and what a wide-k group (17 <= k <= 128, ivf_group_nd_wide_dev) needs beside it, allocated on the first such call
    struct IvfNdWide {
        vs::DevBuf<int32_t> plan, slots, items;  // the rescan plan's tables, as IvfNd's
        vs::DevBuf<float> tau;       // [kIvfNdGroupQ]
        vs::DevBuf<int32_t> mask;    // [kIvfNdGroupQ * np_max] saturated pairs
        vs::DevBuf<int32_t> cnt;     // [kIvfNdGroupQ] candidates per query (zero between groups)
        vs::DevBuf<unsigned long long> cand;   // [kIvfNdGroupQ][kIvfNdWideCand] keys
        vs::DevBuf<unsigned long long> stats;  // [3]: see vs_ivf_nd_widek_stats
        bool ready = false;          // every buffer above allocated (ensure_ivf_nd_wide)
    } ivfndw;
    // ... and what an inner-product group on the byte rows needs, built at the index's first such call (ensure_ivf_nd_ip)
    struct IvfNdIp {
        vs::DevBuf<int32_t> rsum;    // [n_rows + 64] sum (b - 128) per row of d_nd_u8
        vs::DevBuf<int32_t> qsum;    // [kIvfNdGroupQ] sum (q - 128) per query of the group
        bool ready = false;
    } ivfndip;
    vs::Stream wide_stream[kWideLanesMax];
    vs::Event wide_fork, wide_join[kWideLanesMax];
    bool wide_streams_ready = false;
    int64_t n_units_max = 0;
    int n_chunks = 0;
    int32_t max_list = 0;              // longest resident list
    int max_grid = 0;
    unsigned one_calls = 0;            // single-call scans issued so far (they alternate the direction of their pass)

    // host-buffer API (bf_search_shards / vs_ivf_search): two slots of pinned staging + device I/O buffers, so that chunk
    // c + 1's query upload and chunk c - 1's result download run beside chunk c's kernels (copy streams + events)
    struct PipeSlot {
        vs::PinBuf<float> pin_q;   // [kMaxMulti * 32][dim]
        vs::PinBuf<char> pin_out;  // dists | ids | flags of one chunk (k1 <= kTopkWideMax)
        // device I/O: views of the index's d_q / d_out_* / d_flags (slot 0) or of the own_* buffers (slot 1)
        float* d_q = nullptr;
        float* d_out_d = nullptr;  // [kMaxMulti * 32][kTopkWideMax]
        int32_t* d_out_i = nullptr;
        int32_t* d_flags = nullptr;
        vs::DevBuf<float> own_q, own_out_d;
        vs::DevBuf<int32_t> own_out_i, own_flags;
        vs::Event ev_h2d, ev_comp, ev_d2h;
        int64_t q0 = -1, n = 0;    // the chunk in flight in this slot (q0 < 0: free)
    } pipe[2];
    vs::Stream s_h2d, s_d2h;
    bool pipe_ready = false;       // both slots and the copy streams set up (ensure_pipe)
    // vs_ivf_search through the wide pipeline: larger chunks (up to kIvfHostGroups launch groups each, dealt to the two
    // lanes), ONE upload and ONE download per chunk -- every hipMemcpyAsync costs the host tens of microseconds
    struct IvfHostSlot {
        vs::PinBuf<float> pin_q;   // [ivf_host_cap][dim]
        vs::PinBuf<float> pin_out; // dists [n][k] | ids [n][k] of one chunk
        vs::DevBuf<float> d_q;
        vs::DevBuf<float> d_out;   // same layout on the device
        vs::Event ev_h2d, ev_comp[2], ev_d2h;
        int64_t q0 = -1, n = 0;
        int out_k = 0;             // results per query the output buffers hold
        bool ready = false;        // every buffer and event above created (ensure_ivf_host)
    } ihs[2];
    // wide-k brute force (k + 1 > 16, topw_launch), allocated on the first such call: distances to the prefix rows, the
    // prefix's k1 best and bound, the filter's candidates, the dense fallback's chunk scores and per-chunk lists
    struct TopW {
        int64_t l0p = 0;              // prefix rows (padded) the buffers hold: topw_prefix(n_rows, kTopkWideMax)
        int64_t chunk = 0;            // rows per chunk of the dense fallback
        int n_chunks = 0;
        vs::DevBuf<float> pre;        // [32][l0p]
        vs::DevBuf<float> tau;        // [32]
        vs::DevBuf<float> pre_d;      // [32][kTopkWideMax]
        vs::DevBuf<int32_t> pre_i;
        vs::DevBuf<int32_t> fz;       // filter counts [32] | overflow word (cleared by the prefix selection)
        vs::DevBuf<int32_t> f_row;    // [32][kTopwFilterCap]
        vs::DevBuf<float> f_d;
        vs::DevBuf<float> full;       // [32][chunk]
        vs::DevBuf<float> ch_d;       // [32][n_chunks][kTopkWideMax]
        vs::DevBuf<int32_t> ch_i;
        bool ready = false;           // every buffer above allocated (ensure_topw)
    } topw;

    // SearchTiming split of vs_ivf_search (IVFIndex.h:31-36): HIP events between the stages of every launch group
    std::vector<vs::Event> stage_ev;  // quadruples: start, after coarse + pick, after grouping, after scan + select
    int stage_used = 0;
    bool stage_on = false;
    double stage_ms[3] = {0, 0, 0};

    vs::Stream stream;
    vs::Event ev_busy;  // a call on another stream than the previous call's waits for that stream through this event
    hipStream_t last_stream = nullptr;
    bool have_last = false;
    bool prof = false;
    ProfSlot prof_slot[2];
};

namespace {

int set_device(const vs_index* h) {
    HIPCHK(hipSetDevice(h->device));
    return VS_OK;
}

int check_device(int device) {
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0) {
        set_error("no HIP device available (this library has no CPU fallback)");
        return VS_ERR_DEVICE;
    }
    if (device < 0 || device >= n) {
        set_error("device index out of range");
        return VS_ERR_INVALID;
    }
    return VS_OK;
}

// scan geometry for n rows: persistent-style grid of at most one workgroup per CU
// min_tp > 0: a smaller shard uses fewer workgroups so that each still has min_tp (16-row) tiles, the amount from
// which the threshold exchange pays -- as long as that keeps at least half of the CUs busy
void scan_geometry(int64_t rows, int num_cus, int& grid, int& tiles_per_wg, int min_tp = 0) {
    const int64_t tiles = (rows + vs::kTileRows - 1) / vs::kTileRows;
    int64_t g = std::min<int64_t>(num_cus, (tiles + vs::kScanWaves - 1) / vs::kScanWaves);
    if (min_tp > 0 && tiles / g < min_tp && tiles / min_tp >= num_cus / 2) g = tiles / min_tp;
    g = std::max<int64_t>(std::min<int64_t>(g, vs::kSlotStride), 1);
    tiles_per_wg = (int)((tiles + g - 1) / g);
    grid = (int)((tiles + tiles_per_wg - 1) / tiles_per_wg);
    grid = std::max(grid, 1);
}

// scratch of the query-major IVF fallback (one batch at a time)
int alloc_ivf_scratch(vs_index* h) {
    int rc;
    if ((rc = h->d_scores.alloc((size_t)32 * ((h->nlist + 63) & ~63)))) return rc;
    if ((rc = h->d_probes.alloc(32 * kMaxNprobe))) return rc;
    if ((rc = h->d_ipart_d.alloc((size_t)32 * kMaxNprobe * kKcapMax))) return rc;
    if ((rc = h->d_ipart_i.alloc((size_t)32 * kMaxNprobe * kKcapMax))) return rc;
    return VS_OK;
}

int alloc_scratch(vs_index* h) {
    int rc;
    hipDeviceProp_t prop;
    HIPCHK(hipGetDeviceProperties(&prop, h->device));
    h->num_cus = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    if (const char* e = getenv("VSEARCH_GRID_CUS")) h->num_cus = std::max(1, std::min(h->num_cus, atoi(e)));  // tuning knob
    int tp;
    scan_geometry(std::max<int64_t>(h->n_rows, 1), h->num_cus, h->max_grid, tp);
    h->max_grid = std::max(h->max_grid, h->num_cus);
    if ((rc = h->d_q.alloc((size_t)kMaxMulti * 32 * h->dim))) return rc;
    if (h->general && ((rc = h->d_nd_qfrag.alloc((size_t)kMaxMulti * 32 * h->dim_p)) || (rc = h->d_nd_qnorm.alloc((size_t)kMaxMulti * 32))))
        return rc;
    {
        const char* e = getenv("VSEARCH_LANES");
        h->n_lanes = e ? std::max(1, std::min(kMaxLanes, atoi(e))) : 1;
        const size_t nslot = (size_t)kMaxMulti * 32 * vs::kSlotStride;
        const size_t part = (size_t)kMaxMulti * 32 * vs::kSlotStride * kKcapMax;
        for (int i = 0; i < h->n_lanes; ++i) {
            vs_index::Lane& L = h->lane[i];
            if ((rc = L.slots.alloc(nslot))) return rc;
            if ((rc = L.seed_qnorm.alloc((size_t)kMaxMulti * 32))) return rc;
            if ((rc = L.qfrag.alloc((size_t)kMaxMulti * 4096))) return rc;
            if ((rc = L.q8frag.alloc((size_t)kMaxMulti * 4096))) return rc;
            if ((rc = L.qbf.alloc((size_t)kMaxMulti * 4096))) return rc;
            if ((rc = L.qbound.alloc((size_t)kMaxMulti * 32))) return rc;
            if ((rc = L.seed_wmin.alloc((size_t)kMaxMulti * vs::kSeedWaves * 32))) return rc;
            if ((rc = L.tau0.alloc((size_t)kMaxMulti * 32))) return rc;
            if ((rc = L.done.alloc(kMaxMulti))) return rc;
            HIPCHK(hipMemset(L.done, 0, kMaxMulti * sizeof(int)));  // arrival counter of the single-call scan: 0 between launches
            if (h->kind == 0) {
                if ((rc = L.part_d.alloc(part))) return rc;
                if ((rc = L.part_i.alloc(part))) return rc;
            }
            if ((rc = L.s.create()) || (rc = L.done_ev.create())) return rc;
        }
        if ((rc = h->fork.create())) return rc;
    }
    if ((rc = h->d_out_d.alloc((size_t)kMaxMulti * 32 * vs::kTopkWideMax))) return rc;
    if ((rc = h->d_out_i.alloc((size_t)kMaxMulti * 32 * vs::kTopkWideMax))) return rc;
    if ((rc = h->d_flags.alloc((size_t)kMaxMulti * 32))) return rc;
    if (h->kind == 1) {
        if ((rc = h->d_cand.alloc(1))) return rc;
        if ((rc = alloc_ivf_scratch(h))) return rc;
    }
    return h->stream.create();
}

bool f32_filter_enabled();  // VSEARCH_F32_FILTER != 0 (below)

// upload `rows x dim` floats in chunks through the default pageable path and compute norms
int upload_vectors(vs_index* h, const float* host, int64_t rows) {
    int rc;
    if (h->general) {  // [rows + 64][dim_p], zero filled: the padding of a row and the spare rows add exact zeros
        const size_t ld = (size_t)h->dim_p, total = ((size_t)std::max<int64_t>(rows, 1) + vs::kScanPadRows) * ld;
        if ((rc = h->d_vecs.alloc(total))) return rc;
        HIPCHK(hipMemset(h->d_vecs, 0, total * sizeof(float)));
        if ((rc = h->d_norm.alloc((size_t)rows + 64))) return rc;
        HIPCHK(hipMemset(h->d_norm, 0, ((size_t)rows + 64) * sizeof(float)));
        HIPCHK(hipMemcpy2D(h->d_vecs, ld * sizeof(float), host, (size_t)h->dim * sizeof(float), (size_t)h->dim * sizeof(float), (size_t)rows,
                           hipMemcpyHostToDevice));
        HIPCHK(vs::launch_row_sqnorm_ld(h->d_vecs, rows, h->dim, (int64_t)ld, h->d_norm, nullptr));
        HIPCHK(hipDeviceSynchronize());
        return VS_OK;
    }
    if ((rc = h->d_vecs.alloc(((size_t)std::max<int64_t>(rows, 1) + vs::kScanPadRows) * vs::kDim))) return rc;
    HIPCHK(hipMemset(h->d_vecs + (size_t)std::max<int64_t>(rows, 1) * vs::kDim, 0, (size_t)vs::kScanPadRows * vs::kDim * sizeof(float)));
    if ((rc = h->d_norm.alloc((size_t)rows + 64))) return rc;
    HIPCHK(hipMemset(h->d_norm, 0, ((size_t)rows + 64) * sizeof(float)));
    if (rows > 0) {
        HIPCHK(hipMemcpy(h->d_vecs, host, (size_t)rows * vs::kDim * sizeof(float), hipMemcpyHostToDevice));
        HIPCHK(vs::launch_row_sqnorm(h->d_vecs, rows, vs::kDim, h->d_norm, nullptr));
        if (h->kind == 0) {  // brute force: the bf16 prefilter's shard constants and row image, in one pass
            vs::DevBuf<unsigned long long> st;
            if ((rc = st.alloc(5))) return rc;
            HIPCHK(hipMemset(st, 0, 5 * sizeof(unsigned long long)));
            // the image is an accelerator, not a requirement: without the memory for it the index keeps scan_f32s_kernel
            // (and only a shard that the seeded streaming launches take can use it: bf_launch's tiles_total test)
            const bool want_img = f32_filter_enabled() && (rows + vs::kTileRows - 1) / vs::kTileRows >= 2 * vs::kSeedWaves;
            bool have_img = want_img && h->d_img.alloc(((size_t)rows + vs::kScanPadRows) * vs::kDim) == VS_OK;
            if (want_img && !have_img) {
                (void)hipGetLastError();
                vs::set_error("");
            }
            if (have_img) HIPCHK(hipMemset(h->d_img + (size_t)rows * vs::kDim, 0, (size_t)vs::kScanPadRows * vs::kDim * sizeof(uint16_t)));
            HIPCHK(vs::launch_row_filter_image(h->d_vecs, h->d_norm, rows, st, have_img ? h->d_img.get() : nullptr, nullptr));
            unsigned long long v[5];
            HIPCHK(hipMemcpy(v, st, sizeof(v), hipMemcpyDeviceToHost));
            double m[3];
            for (int i = 0; i < 3; ++i) memcpy(&m[i], &v[i], sizeof(double));
            h->fstats.bmax = sqrt(m[0]);
            h->fstats.emax = sqrt(m[1]);
            h->fstats.bpmax = sqrt(m[2]);
            double bnmax;
            memcpy(&bnmax, &v[4], sizeof(double));
            h->filter_cnorm = vs::filter_cnorm(bnmax);
            h->filter_ok = have_img && v[3] == 0 && std::isfinite(m[0]) && std::isfinite(m[2]) && std::isfinite(h->filter_cnorm);
            if (h->filter_ok && h->filter_stats.alloc(4) != VS_OK) {  // (as the image: an accelerator, not a requirement)
                (void)hipGetLastError();
                vs::set_error("");
                h->filter_ok = false;
            }
            if (h->filter_ok) HIPCHK(hipMemset(h->filter_stats, 0, 4 * sizeof(unsigned long long)));
            if (!h->filter_ok) h->d_img.reset();  // (the copy above has waited for the kernel)
        }
        HIPCHK(hipDeviceSynchronize());
    }
    return VS_OK;
}

// int8 copy of the base when it is exactly representable: bytes (x - 128) and the per-row term
// ||b||^2 - 256 * sum(b - 128); dist = [||q||^2 - 256 sum(q-128) - 2*128^3] + rterm - 2 * sum((q-128)(b-128)).
int build_u8_copy(vs_index* h, const float* host, int64_t rows, std::vector<int8_t>* bytes_out = nullptr, std::vector<int32_t>* rterm_out = nullptr) {
    std::vector<int8_t> bytes(((size_t)rows + vs::kScanPadRows) * vs::kDim, 0);  // spare rows: tile DMAs are not clamped
    std::vector<int32_t> rterm((size_t)rows + 64, 0);
    for (int64_t i = 0; i < rows; ++i) {
        int32_t n2 = 0, sb = 0;
        for (int t = 0; t < vs::kDim; ++t) {
            const float x = host[i * vs::kDim + t];
            const int xi = (int)x;
            if (!((float)xi == x) || xi < 0 || xi > 255) return VS_OK;  // not representable: fp32 path only
            bytes[(size_t)i * vs::kDim + t] = (int8_t)(xi - 128);
            n2 += xi * xi;
            sb += xi - 128;
        }
        rterm[(size_t)i] = n2 - 256 * sb;
    }
    int rc;
    if ((rc = h->d_vecs_u8.alloc(bytes.size()))) return rc;
    if ((rc = h->d_rterm.alloc(rterm.size()))) return rc;
    if ((rc = h->d_invalid.alloc((size_t)kMaxMulti))) return rc;
    HIPCHK(hipMemcpy(h->d_vecs_u8, bytes.data(), bytes.size(), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(h->d_rterm, rterm.data(), rterm.size() * sizeof(int32_t), hipMemcpyHostToDevice));
    if (bytes_out) bytes_out->swap(bytes);
    if (rterm_out) rterm_out->swap(rterm);
    return VS_OK;
}

// byte copy of a general index made from uint8 rows: int8 (x - 128) rows padded to dim_b bytes, rterm = sum (b - 128)^2
// over the real dim (dist = qterm + rterm - 2 q'.b', see vs_scan_nd_i8.hip), and max ||b||^2 for the exactness rule.
// An inner-product brute-force index keeps rsum = sum (b - 128) per row instead of rterm (launch_ivf_nd_i8_rowsum).
int build_nd_u8_copy(vs_index* h, const uint8_t* rows_u8, int64_t rows) {
    const size_t ld = (size_t)h->dim_b;
    std::vector<int8_t> bytes(((size_t)rows + vs::kScanPadRows) * ld, 0);  // spare rows: block loads are not clamped
    std::vector<int32_t> rterm((size_t)rows + 64, 0);
    int64_t bmax = 0;
    for (int64_t i = 0; i < rows; ++i) {
        const uint8_t* src = rows_u8 + (size_t)i * h->dim;
        int8_t* dst = bytes.data() + (size_t)i * ld;
        int64_t n2 = 0;
        int32_t t = 0;
        for (int c = 0; c < h->dim; ++c) {
            const int x = src[c], sb = x - 128;
            dst[c] = (int8_t)sb;
            n2 += x * x;
            t += sb * sb;
        }
        rterm[(size_t)i] = t;
        bmax = std::max(bmax, n2);
    }
    if (bmax >= (int64_t)1 << 24) return VS_OK;  // ||q||^2 + ||b||^2 <= 2^24 fails for every batch: fp32 rows only
    h->nd_bmax = (int32_t)bmax;
    int rc;
    if ((rc = h->d_nd_u8.alloc(bytes.size())) || (rc = h->d_invalid.alloc((size_t)kMaxMulti)) ||
        (rc = h->d_nd_q8frag.alloc((size_t)kMaxMulti * 32 * ld)) || (rc = h->d_nd_qterm.alloc((size_t)kMaxMulti * 32)))
        return rc;
    HIPCHK(hipMemcpy(h->d_nd_u8, bytes.data(), bytes.size(), hipMemcpyHostToDevice));
    if (h->kind == 0) {
        if ((rc = h->d_wide_cnt.alloc(2))) return rc;
        HIPCHK(hipMemset(h->d_wide_cnt, 0, 2 * sizeof(unsigned long long)));
    }
    if (h->kind == 0 && h->metric == VS_METRIC_IP) {
        // a brute-force index keeps its metric: the inner-product epilogue needs sum (b - 128) per row, not the L2 term
        if ((rc = h->d_nd_rsum.alloc(rterm.size()))) return rc;
        HIPCHK(vs::launch_ivf_nd_i8_rowsum(h->d_nd_u8, h->dim_b, rows, h->d_nd_rsum, nullptr));
        HIPCHK(hipDeviceSynchronize());
        return VS_OK;
    }
    if ((rc = h->d_nd_rterm.alloc(rterm.size()))) return rc;
    HIPCHK(hipMemcpy(h->d_nd_rterm, rterm.data(), rterm.size() * sizeof(int32_t), hipMemcpyHostToDevice));
    return VS_OK;
}

void prof_begin(vs_index* h, int which, hipStream_t s) {
    if (!h->prof) return;
    ProfSlot& ps = h->prof_slot[which];
    if (ps.used + 2 > kMaxEvents) return;
    while ((int)ps.ev.size() < ps.used + 2) {
        vs::Event e;
        if (e.create(true)) return;
        ps.ev.push_back(std::move(e));
    }
    (void)hipEventRecord(ps.ev[ps.used], s);
}
void prof_end(vs_index* h, int which, hipStream_t s) {
    if (!h->prof) return;
    ProfSlot& ps = h->prof_slot[which];
    if ((int)ps.ev.size() < ps.used + 2) return;
    (void)hipEventRecord(ps.ev[ps.used + 1], s);
    ps.used += 2;
}

// stage mark i (0..3) of the current launch group (vs_ivf_search only)
void stage_mark(vs_index* h, int i, hipStream_t s) {
    if (!h->stage_on) return;
    if (i == 0 && h->stage_used + 4 > kMaxEvents) {
        h->stage_on = false;
        return;
    }
    while ((int)h->stage_ev.size() < h->stage_used + 4) {
        vs::Event e;
        if (e.create(true)) {
            h->stage_on = false;
            return;
        }
        h->stage_ev.push_back(std::move(e));
    }
    (void)hipEventRecord(h->stage_ev[h->stage_used + i], s);
    if (i == 3) h->stage_used += 4;
}

// tuning knob (VSEARCH_XCHG_IT): loop iteration of the first threshold-exchange attempt
int g_xchg_first_it = [] {
    const char* e = getenv("VSEARCH_XCHG_IT");
    return e ? atoi(e) : 1;
}();

int* g_dbg = nullptr;
// tuning knob (VSEARCH_SEED_MIN): multi-batch launches of at least this many batches take their bounds from
// launch_seed instead of the in-kernel exchange (0 = never)
int g_seed_min_batches = [] {
    const char* e = getenv("VSEARCH_SEED_MIN");
    const int v = e ? atoi(e) : 4;
    return v > 0 ? v : 1 << 30;
}();

int g_seed_i8 = [] {
    const char* e = getenv("VSEARCH_SEED_I8");
    return e ? atoi(e) : 1;
}();

// tuning knob (VSEARCH_I8_WIDE): query column blocks per pass of the wide int8 scan (8 = four 32-query batches share one
// pass over the rows, 4 = two, 0 = off: the per-batch int8 scan)
int g_i8_wide = [] {
    const char* e = getenv("VSEARCH_I8_WIDE");
    const int v = e ? atoi(e) : 8;
    return v >= 12 ? 12 : (v >= 8 ? 8 : (v >= 4 ? 4 : 0));
}();

// tuning knob (VSEARCH_F32_PAIR=0): the fp32 streaming scan makes one pass over the rows per batch (HBM bound) instead of
// one per two batches (MFMA bound); 2 = pair on shards of any size (default 1: from kPairMinTiles tiles per workgroup on)
int g_f32_pair = [] {
    const char* e = getenv("VSEARCH_F32_PAIR");
    return e ? atoi(e) : 1;
}();

// tuning knob (VSEARCH_F32_FILTER=0): seeded streaming launches on fp32 rows run scan_f32s_kernel (every dot product on fp32
// MFMA) instead of the bf16 prefilter with the exact fp32 recheck (scan_f32f_kernel; default 1, on shards whose rows are well
// scaled).  VSEARCH_F32_PAIR applies to scan_f32s_kernel only.
int g_f32_filter = [] {
    const char* e = getenv("VSEARCH_F32_FILTER");
    return e ? atoi(e) : 1;
}();
bool f32_filter_enabled() { return g_f32_filter != 0; }

// comparison toggle (VSEARCH_F32F_WAVES=8 or 4): scan_f32f_kernel runs as one 8-wave workgroup per CU, or as two 4-wave
// workgroups per CU, at every launch size (default unset: the measured choice per launch size, launch_scan_f32_stream)
int g_f32f_waves = [] {
    const char* e = getenv("VSEARCH_F32F_WAVES");
    const int v = e ? atoi(e) : 0;
    return v == 4 || v == 8 ? v : 0;
}();

// comparison toggle (VSEARCH_F32F_PRIO=0..8): the second 4-wave workgroup of a CU raises its wave priority in
// scan_f32f_kernel on that many steps of every eight, at every shard size; 0 = never (default unset: the measured choice
// per shard size, launch_scan_f32_stream)
int g_f32f_prio = [] {
    const char* e = getenv("VSEARCH_F32F_PRIO");
    const int v = e ? atoi(e) : -1;
    return v >= 0 && v <= 8 ? v : -1;
}();

// tuning knob (VSEARCH_STREAM=0): seeded launches use the per-batch scan kernels (lane lists + workgroup merge) instead of
// the streaming scans
int g_stream = [] {
    const char* e = getenv("VSEARCH_STREAM");
    return e ? atoi(e) : 1;
}();

// comparison toggle (VSEARCH_ND_FORCE=1): vs_bf_create builds a general index at dim 128 as well, so that scan_nd_kernel
// can be set against the specialised 128-d paths on the same data (default 0: nothing changes)
int g_nd_force = [] {
    const char* e = getenv("VSEARCH_ND_FORCE");
    return e ? atoi(e) : 0;
}();

// floats between consecutive device rows of a brute-force index
inline int64_t row_ld(const vs_index* h) { return h->general ? h->dim_p : vs::kDim; }

// whether a top-k launch on this index takes the byte scan of a general index (scan_nd_i8_kernel, under either metric:
// the byte copy comes with the row term of the index's metric)
inline bool nd_u8_path(const vs_index* h, bool force_f32) {
    return h->general && h->d_nd_u8 && h->precision != 1 && !force_f32 && (h->metric == VS_METRIC_IP ? (bool)h->d_nd_rsum : (bool)h->d_nd_rterm);
}

// the per-batch scan of an index: scan_kernel on 128-d rows, scan_nd_kernel on a general index -- or, for a top-k launch
// whose caller set the byte fields of p (bf_launch, under nd_u8_path), scan_nd_i8_kernel on its byte copy
hipError_t scan_any(vs_index* h, const vs::ScanParams& p, int grid, int kcap, int nqh, int mode, hipStream_t s) {
    if (!h->general) return vs::launch_scan(p, grid, kcap, nqh, mode, s);
    if (p.base_u8 && mode == vs::kModeTopK) {
        vs::ScanNdI8Params bp{};
        bp.s = p;
        bp.dim = h->dim;
        bp.dim_b = h->dim_b;
        bp.bmax = h->nd_bmax;
        bp.q8frag = h->d_nd_q8frag;
        bp.qterm = h->d_nd_qterm;
        bp.rsum = h->d_nd_rsum;  // (inner product; null on an L2 index)
        return vs::launch_scan_nd_i8(bp, grid, kcap, nqh, s);
    }
    vs::ScanNdParams np{};
    np.s = p;
    np.dim = h->dim;
    np.dim_p = h->dim_p;
    np.qfrag = h->d_nd_qfrag;
    np.qnorm = h->d_nd_qnorm;
    return vs::launch_scan_nd(np, grid, kcap, nqh, mode, s);
}

// calls that are compiled for 128-d rows only
int refuse_general(const vs_index* h, const char* what) {
    if (!h || !h->general) return VS_OK;
    char msg[160];
    snprintf(msg, sizeof(msg), "%s: not available on a general-dimension index (dim = %d); only dim == 128 is compiled in", what, h->dim);
    set_error(msg);
    return VS_ERR_UNSUPPORTED;
}

// vs_ivf_* calls on an index made by vs_bf_create_nd*
int refuse_general_bf(const vs_index* h, const char* what) { return h && h->kind == 0 ? refuse_general(h, what) : VS_OK; }
// what a general IVF index leaves out
int refuse_general_ivf(const vs_index* h, const char* what) {
    if (!h || !h->general || h->kind != 1) return VS_OK;
    char msg[280];
    snprintf(msg, sizeof(msg),
             "%s: not available on a general-dimension IVF index (dim = %d): %ssquared L2, k <= 16, one GPU (inner product and k <= 128: "
             "vs_ivf_search_metric)",
             what, h->dim, h->nd_from_u8 ? "" : "fp32 rows, ");
    set_error(msg);
    return VS_ERR_UNSUPPORTED;
}

int ensure_wide(vs_index::Lane& L) {
    if (L.wide8.ready) return VS_OK;
    vs_index::Lane::Wide8 w;
    int rc;
    if ((rc = w.q8.alloc((size_t)kMaxMulti * 32 * vs::kDim))) return rc;
    if ((rc = w.qterm.alloc((size_t)kMaxMulti * 32))) return rc;
    if ((rc = w.wcnt.alloc((size_t)kMaxMulti * 32 * kWideSub + 64))) return rc;  // overflow word | skipped batches | list counters
    if ((rc = w.wcand_d.alloc((size_t)kMaxMulti * 32 * kWideSub * kWideCap))) return rc;
    if ((rc = w.wcand_i.alloc((size_t)kMaxMulti * 32 * kWideSub * kWideCap))) return rc;
    if ((rc = w.wbuf.alloc((size_t)vs::kSlotStride * vs::kScanWaves * kWideWaveCap))) return rc;
    w.ready = true;
    L.wide8 = std::move(w);
    return VS_OK;
}

int pick_kcap(int need) { return need <= 8 ? 8 : (need <= 16 ? 16 : 0); }

// whether a call of nb batches on the specialised 128-d index takes its bounds from the seed launches (bf_launch)
bool bf_seeded(int64_t n_rows, int nb, int k1) {
    const int64_t tiles_total = (n_rows + vs::kTileRows - 1) / vs::kTileRows;
    // The streaming scans' candidate buffers are sized for what survives the seeded bounds: about n_rows * k1 / 32768 rows per
    // query (the sample is 32 768 rows), in kWideSub sub-lists of kWideCap entries.  A shard on which that expectation passes
    // half the capacity (5.6 M rows at k = 5) would overflow on nearly every launch and run the fallback scan as well:
    // it takes the per-batch scan directly.
    const bool cap_ok = (double)n_rows * k1 <= 0.5 * 32768.0 * kWideSub * kWideCap;
    return nb >= g_seed_min_batches && tiles_total >= 2 * vs::kSeedWaves && g_xchg_first_it >= 0 && cap_ok;
}

// What every single-call route refuses, and the plan of routes 2 and 3, which share their body and its geometry.
bool one_call_is_short(int nb, int B, int k1) { return nb < kOneMaxBatches && B <= kOneMaxQueries && k1 <= 16; }
int one_route_nd(int route, int64_t n_rows, int num_cus, int64_t* out) {
    if (n_rows > 0x7fffffff - 2 * vs::kOneNdUnit) return 0;  // (the kernel counts rows in 32 bits)
    out[0] = route;
    out[2] = vs::kOneNdUnit;
    vs::scan_one_nd_geometry(n_rows, num_cus, &out[1], &out[3]);
    return route;
}

// The single-call route of a call that reads the fp32 rows (vs_bf_one_plan's rule; bf_launch goes through it): 0 = none,
// 1 = scan_one_kernel (the specialised 128-d index), 2 = scan_one_nd_kernel (a general index), with the
// launch's workgroups, the rows of a wave's unit of work and the most units any one wave gets in out[1..3] (route 1
// hands its units out through a ticket: the even share).
int one_route(int64_t n_rows, bool general, int num_cus, int nb, int B, int k1, int64_t* out) {
    out[0] = out[1] = out[2] = out[3] = 0;
    if (!one_call_is_short(nb, B, k1)) return 0;
    if (general) return one_route_nd(2, n_rows, num_cus, out);
    if (bf_seeded(n_rows, nb, k1)) return 0;
    const int64_t tiles = (n_rows + vs::kTileRows - 1) / vs::kTileRows;
    out[0] = 1;
    out[1] = vs::scan_one_grid(n_rows, num_cus);
    out[2] = vs::kTileRows;
    out[3] = (tiles + out[1] * vs::kScanWaves - 1) / (out[1] * vs::kScanWaves);
    return 1;
}

// The single-call route of a short call that reads the byte rows of a general index (vs_bf_one_plan_u8's rule; bf_launch
// goes through it): 0 = none, 3 = scan_one_nd_i8_kernel, with the geometry of route 2 in out[1..3].
// The measured exception: rows of at most 128 bytes (dim <= 128: a unit is a single K step and the distance epilogue runs
// every step) with more than 12 queries in the batch keep the per-batch route -- at 64-d and 96-d under squared L2 the
// single-call kernel took 63.7 and 69.2 us against 62.8 and 67.6 us at B = 16 (1 M rows; the same 2 - 3 % at 400 K and
// 700 K rows), and was 2 - 4 % faster at B = 12.
constexpr int kOneU8ShortRowBytes = 128;
constexpr int kOneU8ShortRowQueries = 12;
int one_route_u8(int64_t n_rows, int dim, int num_cus, int nb, int B, int k1, int64_t* out) {
    out[0] = out[1] = out[2] = out[3] = 0;
    if (!one_call_is_short(nb, B, k1)) return 0;
    if (vs::nd_dim_b(dim) <= kOneU8ShortRowBytes && B > kOneU8ShortRowQueries) return 0;
    return one_route_nd(3, n_rows, num_cus, out);
}

// nb <= kMaxMulti batches of B queries in ONE persistent launch on stream s (preceded by the seed launches or the
// slot reset, followed by one merge launch), outputs [nb][B][k1].  Consecutive calls on one lane must be stream-ordered.
int bf_launch(vs_index* h, vs_index::Lane& L, const float* q_dev, int nb, int B, int k1, float* out_d, int32_t* out_i,
              int32_t* flags, hipStream_t s, bool force_f32 = false) {
    const int kcap = pick_kcap(k1);
    if (!kcap) {
        set_error("k too large for the compiled scan kernels (k <= 15)");
        return VS_ERR_UNSUPPORTED;
    }
    const int nqh = B <= 16 ? 1 : 2;
    vs::ScanParams p{};
    p.base = h->d_vecs;
    p.bnorm = h->d_norm;
    p.q = q_dev;
    p.n_batches = nb;
    p.q_batch_stride = (int64_t)B * h->dim;
    p.metric = h->metric;
    p.id_offset = (int32_t)h->id_offset;
    p.nq_valid = B;
    p.k1 = k1;
    p.dbg = g_dbg;
    // the exchange pays once every wave has a few tiles left after its warm-up tiles (int8 tiles hold 64 rows)
    const bool u8_path = h->d_vecs_u8 && h->precision != 1 && !force_f32;
    // a multi-batch launch gets its bounds up front from a sample of the rows (three small launches for all
    // batches): every batch then streams from its first tile on, whatever the shard size (as long as the 2048
    // sample tiles are a minority of it); a short call keeps the in-kernel exchange, which needs a few tiles per
    // wave after its warm-up tiles (int8 tiles hold 64 rows)
    const int64_t tiles_total = (h->n_rows + vs::kTileRows - 1) / vs::kTileRows;
    // (a general index has no seed sample and no streaming scan: per-batch scan_nd_kernel + merge, with the threshold exchange)
    const bool seeded = !h->general && bf_seeded(h->n_rows, nb, k1);
    int grid, tp;
    scan_geometry(h->n_rows, h->num_cus, grid, tp, seeded ? 0 : (u8_path ? 16 : 6) * vs::kScanWaves);
    const bool exchange = !seeded && grid >= 16 && tp >= (u8_path ? 16 : 6) * vs::kScanWaves && g_xchg_first_it >= 0;
    const bool use_u8 = u8_path;
    // With the bounds known up front the batches need nothing from each other: the streaming scans (fp32: one batch per
    // pass; exact int8 rows: several batches per pass over the rows) hand out the tiles of ALL batches through one
    // ticket per workgroup and write survivors to candidate lists -- no barrier, no workgroup merge, no per-batch prologue.
    const bool i8_seed = h->d_vecs_u8 && h->metric == VS_METRIC_L2 && g_seed_i8;
    const bool stream = seeded && g_stream && (use_u8 ? (g_i8_wide > 0 && i8_seed) : true);
    const bool f32_filter = stream && !use_u8 && g_f32_filter && h->filter_ok;
    // a short call on the fp32 rows: one launch per batch (lane lists, workgroup ranking, the last workgroup merges).
    // Batches of more than 16 queries stay with the per-batch scan below: with two column blocks per tile the
    // single-call kernel's lane lists cost more than that kernel's threshold exchange (measured at 1 M rows, B = 32:
    // 154 us against 102 us; B <= 16: 88 - 97 us against 102 - 114 us).  On a general index the same rule sends the
    // call to scan_one_nd_kernel, unless the index was created under VSEARCH_ND_ONE=0.
    int64_t one_plan[4] = {0, 0, 0, 0};
    const bool reads_f32 = h->general ? !nd_u8_path(h, force_f32) : !use_u8;
    if (reads_f32 && (!h->general || h->nd_one)) one_route(h->n_rows, h->general, h->num_cus, nb, B, k1, one_plan);
    // ... and a short call on the byte rows of a general index goes to scan_one_nd_i8_kernel, unless the
    // index was created under VSEARCH_ND_ONE_U8=0
    if (!reads_f32 && h->general && h->nd_one_u8) one_route_u8(h->n_rows, h->dim, h->num_cus, nb, B, k1, one_plan);
    if (one_plan[0]) {
        for (int b = 0; b < nb; ++b) {
            vs::OneParams op{};
            op.base = h->d_vecs;
            op.bnorm = h->d_norm;
            op.n_rows = h->n_rows;
            op.q = q_dev + (size_t)b * B * h->dim;
            op.nq_valid = B;
            op.k1 = k1;
            op.metric = h->metric;
            op.reverse = (int)(h->one_calls++ & 1u);
            op.id_offset = (int32_t)h->id_offset;
            op.part_d = L.part_d;
            op.part_i = L.part_i;
            op.done = L.done;
            op.out_d = out_d + (size_t)b * B * k1;
            op.out_i = out_i + (size_t)b * B * k1;
            op.flags = flags ? flags + (size_t)b * B : nullptr;
            op.dbg = g_dbg;
            if (b == 0) prof_begin(h, 0, s);
            ++h->one_stat[one_plan[0] == 3 ? 1 : 0];
            if (one_plan[0] == 3) {
                vs::OneNdI8Params bp{};
                bp.o = op;
                bp.dim = h->dim;
                bp.dim_b = h->dim_b;
                bp.bmax = h->nd_bmax;
                bp.base_u8 = h->d_nd_u8;
                bp.rterm = h->d_nd_rterm;  // (squared L2; null on an inner-product index)
                bp.rsum = h->d_nd_rsum;    // (inner product; null on an L2 index)
                HIPCHK(vs::launch_scan_one_nd_i8(bp, (int)one_plan[1], s));
            } else if (one_plan[0] == 2) {
                vs::OneNdParams np{};
                np.o = op;
                np.dim = h->dim;
                np.dim_p = h->dim_p;
                HIPCHK(vs::launch_scan_one_nd(np, (int)one_plan[1], s));
            } else {
                HIPCHK(vs::launch_scan_one(op, (int)one_plan[1], s));
            }
            if (b == nb - 1) prof_end(h, 0, s);
        }
        return VS_OK;
    }
    if (seeded || use_u8) {
        int rc = ensure_wide(L);
        if (rc) return rc;
    }
    // one zeroed block per launch: [0] overflow word | [16, 48) batches the int8 path has to skip | [64, ...) list counters
    int32_t* const overflow = L.wide8.wcnt;
    int32_t* const invalid = L.wide8.wcnt ? L.wide8.wcnt + 16 : nullptr;
    // (cleared by the seed's query-preparation launch where there is one and nobody else writes the batches' verdict words)
    const size_t zero_words = 64 + (stream ? (size_t)nb * 32 * kWideSub : 0);
    const bool zero_in_seed = seeded && (!use_u8 || i8_seed);
    if (L.wide8.wcnt && !zero_in_seed) HIPCHK(hipMemsetAsync(L.wide8.wcnt, 0, zero_words * sizeof(int32_t), s));
    if (seeded) {
        vs::SeedParams sp{};
        sp.base = h->d_vecs;
        sp.bnorm = h->d_norm;
        sp.sample_f32 = h->d_seed_f32;
        sp.sample_bnorm = h->d_seed_bnorm;
        if (i8_seed) {  // exact int8 copy of the rows: 16x cheaper seed
            sp.base_u8 = h->d_vecs_u8;
            sp.rterm = h->d_rterm;
            sp.sample_u8 = h->d_seed_u8;
            sp.sample_rterm = h->d_seed_rterm;
        }
        sp.n_rows = h->n_rows;
        sp.q = q_dev;
        sp.n_batches = nb;
        sp.q_batch_stride = (int64_t)B * vs::kDim;
        sp.nq_valid = B;
        sp.metric = h->metric;
        sp.k1 = k1;
        sp.qnorm = L.seed_qnorm;
        sp.wmin = L.seed_wmin;
        sp.tau0 = L.tau0;
        if (zero_in_seed) {
            sp.zero = L.wide8.wcnt;
            sp.zero_words = (int)zero_words;
        }
        sp.qfrag = L.qfrag;
        if (f32_filter) {
            sp.qbf = L.qbf;
            sp.qbound = L.qbound;
            sp.fstats = h->fstats;
        }
        if (i8_seed) {  // queries as bytes + constant terms + the "not byte valued" verdict: int8 seed and wide int8 scan
            sp.q8 = L.wide8.q8;
            sp.q8frag = L.q8frag;
            sp.qterm = L.wide8.qterm;
            sp.invalid = invalid;
        }
        HIPCHK(vs::launch_seed(sp, s));
        p.tau0 = L.tau0;
    } else if (exchange) {
        // 0x7f800000 = +inf
        HIPCHK(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(L.slots.get()), 0x7f800000, (size_t)nb * 32 * vs::kSlotStride, s));
        p.slots_cur = L.slots;
    }
    vs::MergeParams m{};
    m.nq = nb * B;
    m.kout = k1;
    m.out_d = out_d;
    m.out_i = out_i;
    m.flags = flags;
    m.q_group_out = B;
    m.q_group_in = vs::kMaxBatch;
    m.invalid = use_u8 ? invalid : nullptr;
    if (stream) {
        vs::CandSink sink{};
        sink.wbuf = L.wide8.wbuf;
        sink.wcap = kWideWaveCap;
        sink.overflow = overflow;
        sink.cnt = L.wide8.wcnt + 64;
        sink.cand_d = L.wide8.wcand_d;
        sink.cand_i = L.wide8.wcand_i;
        sink.cap = kWideCap;
        sink.nsub = kWideSub;
        prof_begin(h, 0, s);
        if (use_u8) {
            vs::WideParams wp{};
            wp.base_u8 = h->d_vecs_u8;
            wp.rterm = h->d_rterm;
            wp.n_rows = h->n_rows;
            wp.q8 = L.wide8.q8;
            wp.q8frag = L.q8frag;
            wp.qterm = L.wide8.qterm;
            wp.tau0 = L.tau0;
            wp.invalid = invalid;
            wp.n_batches = nb;
            wp.nq_valid = B;
            wp.bpb = nqh;
            wp.id_offset = (int32_t)h->id_offset;
            wp.sink = sink;
            const int64_t tiles64 = (h->n_rows + 63) / 64;
            const int wgrid = (int)std::max<int64_t>(1, std::min<int64_t>(std::min(h->num_cus, vs::kSlotStride), tiles64));
            HIPCHK(vs::launch_scan_i8_wide(wp, wgrid, g_i8_wide, s));
            prof_end(h, 0, s);
        } else {
            vs::StreamParams sp{};
            sp.base = h->d_vecs;
            sp.bnorm = h->d_norm;
            sp.n_rows = h->n_rows;
            sp.q = q_dev;
            sp.q_batch_stride = (int64_t)B * vs::kDim;
            sp.qfrag = L.qfrag;
            sp.qnorm = L.seed_qnorm;
            sp.tau0 = L.tau0;
            sp.n_batches = nb;
            sp.nq_valid = B;
            sp.metric = h->metric;
            sp.id_offset = (int32_t)h->id_offset;
            sp.sink = sink;
            const int sgrid = (int)std::max<int64_t>(1, std::min<int64_t>(std::min(h->num_cus, vs::kSlotStride), tiles_total));
            // two batches per pass pay where a workgroup has many tiles per pass (1 M rows: 244, + 14 %); on a small shard
            // (125 K rows: 30 tiles) the per-pass operand fetch and drain weigh more than the halved traffic saves (- 15 %)
            sp.batches_per_pass = (nb >= 2 && (g_f32_pair > 1 || (g_f32_pair == 1 && tiles_total / sgrid >= kPairMinTiles))) ? 2 : 1;
            if (f32_filter) {  // one sweep over the rows serves all nb batches (batches_per_pass does not apply)
                sp.qbf = L.qbf;
                sp.qbound = L.qbound;
                sp.img = h->d_img;
#if defined(VS_STAMPS) || defined(VS_F32F_ENDS)
                sp.dbg = g_dbg ? g_dbg + 12288 * 16 : nullptr;  // (rows of its own: the kernels around it stamp rows [0, 256))
#endif
                sp.cnorm = h->filter_cnorm;
                sp.f32f_waves = g_f32f_waves;
                sp.f32f_prio = g_f32f_prio;
                sp.sink.stats = h->filter_stats;
                ++h->filter_launches;
            }
            HIPCHK(vs::launch_scan_f32_stream(sp, sgrid, s));
            prof_end(h, 0, s);
        }
        // every query's candidate list (unsorted, a few hundred entries) -> k1 best by (dist, id), tie flags: the merge
        // launch at the end, which ranks the lane lists of the fallback instead where the overflow word is raised
        m.G = kWideSub;
        m.kin = kWideCap;
        m.flat_len = L.wide8.wcnt + 64;
        m.run_if = overflow;
        m.run_mode = 3;
        // Fallback, enqueued behind and idle unless a candidate buffer overflowed (thousands of rows under one query's
        // bound: masses of duplicates): the per-batch scan with lane lists, which copes with any data.
        p.run_if = overflow;
    }
    p.row_begin = 0;
    p.row_end = h->n_rows;
    p.tiles_per_wg = tp;
    p.part_d = L.part_d;
    p.part_i = L.part_i;
    if (use_u8) {
        p.base_u8 = h->d_vecs_u8;
        p.rterm = h->d_rterm;
        p.invalid = invalid;
    }
    if (nd_u8_path(h, force_f32)) {  // the verdict words are written (0 or 1) by the byte scan's preparation launch
        p.base_u8 = h->d_nd_u8;
        p.rterm = h->d_nd_rterm;
        p.invalid = h->d_invalid;
        m.invalid = h->d_invalid;
    }
    if (!stream) prof_begin(h, 0, s);
    HIPCHK(scan_any(h, p, grid, kcap, nqh, vs::kModeTopK, s));
    if (!stream) prof_end(h, 0, s);
    // one merge launch ranks every (batch, query): lists are [batch*32 + q][workgroup][kcap]
    if (stream) {  // ... or, unless the streaming scan overflowed, its candidate lists [batch*32 + q][kWideSub][kWideCap]
        m.part_d = L.wide8.wcand_d;
        m.part_i = L.wide8.wcand_i;
        m.alt_part_d = L.part_d;
        m.alt_part_i = L.part_i;
        m.alt_G = grid;
        m.alt_kin = kcap;
        m.alt_stride_g = kcap;
        m.alt_stride_q = (int64_t)vs::kSlotStride * kcap;
        HIPCHK(vs::launch_merge_layout(m, kWideCap, (int64_t)kWideSub * kWideCap, s));
        return VS_OK;
    }
    m.part_d = L.part_d;
    m.part_i = L.part_i;
    m.G = grid;
    m.kin = kcap;
    HIPCHK(vs::launch_merge_layout(m, kcap, (int64_t)vs::kSlotStride * kcap, s));
    return VS_OK;
}

int bf_batch_dev(vs_index* h, vs_index::Lane& L, const float* q_dev, int B, int k1, float* out_d, int32_t* out_i,
                 int32_t* flags, hipStream_t s) {
    return bf_launch(h, L, q_dev, 1, B, k1, out_d, out_i, flags, s);
}

// nb batches of B queries: chunks of kMaxMulti batches per persistent launch, on the caller's stream.
int bf_multi_dev(vs_index* h, const float* q_dev, int nb, int B, int k1, float* out_d, int32_t* out_i, int32_t* flags,
                 hipStream_t user) {
    for (int b0 = 0; b0 < nb; b0 += kMaxMulti) {
        const int n = std::min(kMaxMulti, nb - b0);
        int rc = bf_launch(h, h->lane[0], q_dev + (size_t)b0 * B * h->dim, n, B, k1, out_d + (size_t)b0 * B * k1,
                           out_i + (size_t)b0 * B * k1, flags ? flags + (size_t)b0 * B : nullptr, user);
        if (rc) return rc;
    }
    return VS_OK;
}

int scores_dev(vs_index* h, const float* vecs, const float* norms, int64_t rows, const float* q_dev, int B,
               float* scores, int64_t ld, hipStream_t s, const int32_t* run_if = nullptr) {
    vs::ScanParams p{};
    p.run_if = run_if;
    p.base = vecs;
    p.bnorm = norms;
    p.q = q_dev;
    p.metric = h->metric;
    p.nq_valid = B;
    p.n_batches = 1;
    p.row_begin = 0;
    p.row_end = rows;
    int grid, tp;
    scan_geometry(rows, h->num_cus, grid, tp);
    p.tiles_per_wg = tp;
    p.store = scores;
    p.store_ld = ld;
    HIPCHK(scan_any(h, p, grid, 8, B <= 16 ? 1 : 2, vs::kModeStore, s));
    return VS_OK;
}

// ---- wide k (k1 = k + 1 in 17..129).  Per batch: the distances to a prefix of the rows (scores_dev), its k1 best and
// bound tau = next_up(k1-th best) (topk_wide_kernel, dense form), one filtered pass over the other rows that keeps every
// distance under tau (kModeFilter, about n_rows * k1 / prefix rows per query), and the k1 best of the prefix's list and the
// candidates (topk_wide_kernel, list form).  Exact: a row after the prefix at or above tau has k1 prefix rows before it.
// A candidate list that overflows (masses of equal rows) raises the batch's overflow word, and the dense fallback enqueued
// behind it (scores of row chunks, a selection per chunk, a selection over the chunk lists) rewrites the outputs.
int64_t topw_prefix(int64_t n_rows, int k1) {
    // about n_rows / 512 candidates per query at most 2048 (larger bases take a longer prefix), a multiple of 4096 rows
    int64_t l = std::max<int64_t>(512 * (int64_t)k1, n_rows * k1 / 2048);
    l = (l + 4095) & ~int64_t(4095);
    return std::min(l, n_rows);
}

// Whether a wide call (k1 = k + 1 > 16) on the byte copy of a general index of this shape runs its two bulk passes on the
// byte rows (vs_bf_wide_plan's rule; topw_launch goes through it).  Every shape does: none measured slower -- 1.07 x at
// 96-d to 3.8 x at 2048-d on 1 M rows; a shape that does would leave here, with its numbers.
bool wide_route_u8(int64_t n_rows, int dim, int k1) {
    (void)n_rows;
    (void)dim;
    return k1 > kKcapMax;
}

int ensure_topw(vs_index* h) {
    if (h->topw.ready) return VS_OK;
    vs_index::TopW w;
    w.l0p = (topw_prefix(h->n_rows, vs::kTopkWideMax) + 15) & ~int64_t(15);
    w.chunk = std::min<int64_t>((h->n_rows + 15) & ~int64_t(15), kTopwChunkBytes / (32 * sizeof(float)));
    w.n_chunks = (int)((h->n_rows + w.chunk - 1) / w.chunk);
    const size_t kw = vs::kTopkWideMax;
    int rc;
    if ((rc = w.pre.alloc((size_t)32 * w.l0p)) || (rc = w.tau.alloc(32)) || (rc = w.pre_d.alloc(32 * kw)) || (rc = w.pre_i.alloc(32 * kw)) ||
        (rc = w.fz.alloc(64)) || (rc = w.f_row.alloc((size_t)32 * kTopwFilterCap)) || (rc = w.f_d.alloc((size_t)32 * kTopwFilterCap)) ||
        (rc = w.full.alloc((size_t)32 * w.chunk)) || (rc = w.ch_d.alloc((size_t)32 * w.n_chunks * kw)) ||
        (rc = w.ch_i.alloc((size_t)32 * w.n_chunks * kw)))
        return rc;
    HIPCHK(hipMemset(w.fz, 0, 64 * sizeof(int32_t)));
    w.ready = true;
    h->topw = std::move(w);
    return VS_OK;
}

// diagnostic knob (VSEARCH_TOPW_STATS=1): topw_launch waits for every batch and counts the batches whose candidate lists
// overflowed and the candidates per query; vs_bf_search_topk prints the counts to stderr
int g_topw_stats = [] {
    const char* e = getenv("VSEARCH_TOPW_STATS");
    return e ? atoi(e) : 0;
}();
struct TopwStats {
    int64_t batches = 0, overflowed = 0, queries = 0, cand_sum = 0, cand_max = 0;
} g_topw_st;

// nb batches of B queries -> [nb][B][k1] by (dist, id) + flags (1 = two equal distances among the k1), on stream s
int topw_launch(vs_index* h, const float* q_dev, int nb, int B, int k1, float* out_d, int32_t* out_i, int32_t* flags,
                hipStream_t s) {
    vs_index::TopW& W = h->topw;
    const int64_t n = h->n_rows;
    const int64_t l0 = topw_prefix(n, k1), l0p = (l0 + 15) & ~int64_t(15);
    int32_t* const overflow = W.fz + 32;
    int rc;
    // On an index with byte rows the two bulk passes (prefix scores, filter) run on them: one preparation
    // launch per kMaxMulti batches (what the scratch holds) gives each its byte fragments and its verdict word; per batch the byte launch of a pass
    // returns at once where the word is set, and the fp32 launch behind it runs only there (run_if).  Either writes the
    // same scratch with the same bits, so the selections between the passes and the fallback stay as they are.
    const bool u8 = nd_u8_path(h, false) && h->nd_wide_u8 && wide_route_u8(n, h->dim, k1);
    vs::ScanNdI8Params bp{};
    if (u8) {
        bp.dim = h->dim;
        bp.dim_b = h->dim_b;
        bp.bmax = h->nd_bmax;
        bp.q8frag = h->d_nd_q8frag;
        bp.qterm = h->d_nd_qterm;
        bp.rsum = h->d_nd_rsum;  // (inner product; null on an L2 index)
        bp.wide_cnt = h->d_wide_cnt;
        bp.s.base_u8 = h->d_nd_u8;
        bp.s.rterm = h->d_nd_rterm;
        bp.s.invalid = h->d_invalid;
        bp.s.q_batch_stride = (int64_t)B * h->dim;
        bp.s.metric = h->metric;
        bp.s.nq_valid = B;
        bp.s.k1 = k1;
    }
    const int nqh8 = B <= 16 ? 1 : 2;
    h->wide_batches += nb;
    prof_begin(h, 0, s);
    for (int b = 0; b < nb; ++b) {
        const float* qb = q_dev + (size_t)b * B * h->dim;
        float* const od = out_d + (size_t)b * B * k1;
        int32_t* const oi = out_i + (size_t)b * B * k1;
        int32_t* const fl = flags ? flags + (size_t)b * B : nullptr;
        const int slot = b % kMaxMulti;  // this batch's place in the byte scratch
        const int32_t* const not_bytes = u8 ? h->d_invalid + slot : nullptr;  // the fp32 passes' run_if
        if (u8) {
            bp.wide_batch = slot;
            if (slot == 0) {
                bp.s.q = qb;
                bp.s.n_batches = std::min(kMaxMulti, nb - b);
            }
            vs::ScanNdI8Params sp = bp;
            sp.wide_prepared = slot > 0;
            sp.s.row_begin = 0;
            sp.s.row_end = l0;
            sp.s.store = W.pre;
            sp.s.store_ld = l0p;
            int sgrid, stp;
            scan_geometry(l0, h->num_cus, sgrid, stp);
            HIPCHK(vs::launch_scan_nd_i8_wide(sp, sgrid, nqh8, vs::kModeStore, s));
        }
        if ((rc = scores_dev(h, h->d_vecs, h->d_norm, l0, qb, B, W.pre, l0p, s, not_bytes))) return rc;
        vs::TopkWideParams t{};
        t.dense = W.pre;
        t.dense_ld = l0p;
        t.n_dense = l0;
        t.dense_id0 = (int32_t)h->id_offset;
        t.nq = B;
        t.k1 = k1;
        if (l0 == n) {  // the prefix is the whole shard
            t.out_d = od;
            t.out_i = oi;
            t.out_ld = k1;
            t.flags = fl;
            HIPCHK(vs::launch_topk_wide(t, B, s));
            continue;
        }
        t.out_d = W.pre_d;
        t.out_i = W.pre_i;
        t.out_ld = vs::kTopkWideMax;
        t.tau_out = W.tau;
        t.zero = W.fz;
        t.zero_words = 33;
        HIPCHK(vs::launch_topk_wide(t, 32, s));
        vs::ScanParams p{};
        p.base = h->d_vecs;
        p.bnorm = h->d_norm;
        p.q = qb;
        p.n_batches = 1;
        p.metric = h->metric;
        p.nq_valid = B;
        p.k1 = k1;
        p.tau0 = W.tau;
        p.row_begin = l0;  // a multiple of 4096
        p.row_end = n;
        p.f_cnt = W.fz;
        p.f_row = W.f_row;
        p.f_d = W.f_d;
        p.f_cap = kTopwFilterCap;
        int grid, tp;
        scan_geometry(n - l0, h->num_cus, grid, tp);
        p.tiles_per_wg = tp;
        if (u8) {
            vs::ScanNdI8Params fp = bp;
            fp.wide_prepared = 1;
            fp.s.row_begin = l0;
            fp.s.row_end = n;
            fp.s.tau0 = W.tau;
            fp.s.f_cnt = W.fz;
            fp.s.f_row = W.f_row;
            fp.s.f_d = W.f_d;
            fp.s.f_cap = kTopwFilterCap;
            HIPCHK(vs::launch_scan_nd_i8_wide(fp, grid, nqh8, vs::kModeFilter, s));
            p.run_if = not_bytes;
        }
        HIPCHK(scan_any(h, p, grid, 8, 2, vs::kModeFilter, s));
        vs::TopkWideParams f{};
        f.list[0] = {W.pre_d, W.pre_i, vs::kTopkWideMax, nullptr, k1, 0};
        f.list[1] = {W.f_d, W.f_row, kTopwFilterCap, W.fz, kTopwFilterCap, (int32_t)h->id_offset};
        f.n_list = 2;
        f.nq = B;
        f.k1 = k1;
        f.out_d = od;
        f.out_i = oi;
        f.out_ld = k1;
        f.flags = fl;
        f.overflow = overflow;
        HIPCHK(vs::launch_topk_wide(f, B, s));
        if (g_topw_stats) {
            int32_t c[33];
            HIPCHK(hipMemcpyAsync(c, W.fz, sizeof(c), hipMemcpyDeviceToHost, s));
            HIPCHK(hipStreamSynchronize(s));
            ++g_topw_st.batches;
            g_topw_st.overflowed += c[32] != 0;
            for (int i = 0; i < B; ++i) {
                ++g_topw_st.queries;
                g_topw_st.cand_sum += c[i];
                g_topw_st.cand_max = std::max<int64_t>(g_topw_st.cand_max, c[i]);
            }
        }
        // dense fallback, idle unless a candidate list overflowed
        const int nc = W.n_chunks;
        for (int c = 0; c < nc; ++c) {
            const int64_t r0 = (int64_t)c * W.chunk, rows = std::min(W.chunk, n - r0);
            if ((rc = scores_dev(h, h->d_vecs + (size_t)r0 * row_ld(h), h->d_norm + r0, rows, qb, B, W.full, W.chunk, s, overflow)))
                return rc;
            vs::TopkWideParams d{};
            d.dense = W.full;
            d.dense_ld = W.chunk;
            d.n_dense = rows;
            d.dense_id0 = (int32_t)(h->id_offset + r0);
            d.nq = B;
            d.k1 = k1;
            d.run_if = overflow;
            if (nc == 1) {
                d.out_d = od;
                d.out_i = oi;
                d.out_ld = k1;
                d.flags = fl;
            } else {
                d.out_d = W.ch_d + (size_t)c * k1;
                d.out_i = W.ch_i + (size_t)c * k1;
                d.out_ld = (int64_t)nc * k1;
            }
            HIPCHK(vs::launch_topk_wide(d, B, s));
        }
        if (nc > 1) {
            vs::TopkWideParams m{};
            m.list[0] = {W.ch_d, W.ch_i, (int64_t)nc * k1, nullptr, nc * k1, 0};
            m.n_list = 1;
            m.nq = B;
            m.k1 = k1;
            m.out_d = od;
            m.out_i = oi;
            m.out_ld = k1;
            m.flags = fl;
            m.run_if = overflow;
            HIPCHK(vs::launch_topk_wide(m, B, s));
        }
    }
    prof_end(h, 0, s);
    return VS_OK;
}

// tuning knob (VSEARCH_IVF_WIDE_LANES=1, read when an index is created): vs_ivf_search_dev_multi keeps all launch groups of
// a call on the caller's stream instead of alternating them between two streams
int ivf_wide_lanes() {
    const char* e = getenv("VSEARCH_IVF_WIDE_LANES");
    return e ? std::max(1, std::min(kWideLanesMax, atoi(e))) : 2;
}
// tuning knob (VSEARCH_IVF_GROUP, read when an index is created): batches per launch group of an unsharded index
// (multiple of 32, <= 256): every kernel of the pipeline is launched once per group
int ivf_group_batches() {
    const char* e = getenv("VSEARCH_IVF_GROUP");
    const int v = e ? atoi(e) : kIvfGroupDefault;
    return std::max(32, std::min(kIvfGroupMax, (v + 31) / 32 * 32));
}

// Is the wide list-major pipeline available for this index?  (nlist <= 4096, rows resident, k <= 16; otherwise the
// query-major fallback: coarse scores on the MFMA scan kernel, pick_probes, one workgroup per (query, probe).)
bool ivf_wide_ok(const vs_index* h, int k) {
    return h->nlist <= vs::kIvfFastNlist && h->n_chunks > 0 && k >= 1 && k <= vs::kIvfWideKMax;
}

// Query-major fallback for one batch (nlist > 4096, or a shard without resident rows).
int ivf_fallback_batch_dev(vs_index* h, const float* q_dev, int B, int k, int nprobe, float* out_d, int32_t* out_i, hipStream_t s) {
    const int kcap = pick_kcap(k);
    if (!kcap) {
        set_error("k too large for the compiled IVF kernels (k <= 16)");
        return VS_ERR_UNSUPPORTED;
    }
    const int64_t ld = (h->nlist + 63) & ~63;
    stage_mark(h, 0, s);
    int rc = scores_dev(h, h->d_centroids, h->d_cnorm, h->nlist, q_dev, B, h->d_scores, ld, s);
    if (rc) return rc;
    HIPCHK(vs::launch_pick_probes(h->d_scores, ld, B, h->nlist, nprobe, h->d_probes, s));
    stage_mark(h, 1, s);
    stage_mark(h, 2, s);
    vs::IvfScanParams ip{};
    ip.vecs = h->d_vecs;
    ip.vnorm = h->d_norm;
    ip.offsets = h->d_offsets;
    ip.owned = nullptr;
    ip.q = q_dev;
    ip.probes = h->d_probes;
    ip.B = B;
    ip.nprobe = nprobe;
    ip.kcap = kcap;
    ip.metric = h->metric;
    ip.part_d = h->d_ipart_d;
    ip.part_i = h->d_ipart_i;
    ip.cand_count = h->d_cand;
    prof_begin(h, 1, s);
    HIPCHK(vs::launch_ivf_scan(ip, s));
    prof_end(h, 1, s);
    vs::MergeParams m{};
    m.part_d = h->d_ipart_d;
    m.part_i = h->d_ipart_i;
    m.G = nprobe;
    m.kin = kcap;
    m.nq = B;
    m.kout = k;
    m.out_d = out_d;
    m.out_i = out_i;
    m.id_map = h->d_r2o;
    HIPCHK(vs::launch_merge_layout(m, kcap, (int64_t)nprobe * kcap, s));
    stage_mark(h, 3, s);
    return VS_OK;
}

// Scratch of the general IVF index's launch groups.  Built aside and moved in whole: a failure part-way frees what it
// allocated and leaves the index as it was.
int ensure_ivf_nd(vs_index* h) {
    if (h->ivfnd.ready) return VS_OK;
    vs_index::IvfNd W;
    int rc;
    W.np_max = std::min(kMaxNprobe, h->nlist);
    const size_t gq = vs::kIvfNdGroupQ, pairs = gq * W.np_max;
    if ((rc = W.probes.alloc(pairs)) || (rc = W.qrows.alloc(gq * h->dim_p)) || (rc = W.qnorm.alloc(gq)) ||
        (rc = W.plan.alloc((size_t)3 * h->nlist + 2)) || (rc = W.slots.alloc(pairs)) ||
        (rc = W.items.alloc((size_t)2 * vs::ivf_nd_items_cap(h->nlist, W.np_max))) || (rc = W.part_d.alloc(pairs * kKcapMax)) ||
        (rc = W.part_i.alloc(pairs * kKcapMax)))
        return rc;
    if (h->d_nd_u8 && ((rc = W.plan8.alloc((size_t)3 * h->nlist + 2)) || (rc = W.slots8.alloc(pairs)) ||
                       (rc = W.items8.alloc((size_t)2 * vs::ivf_nd_items_cap(h->nlist, W.np_max))) ||
                       (rc = W.q8rows.alloc(gq * h->dim_b)) || (rc = W.qterm.alloc(gq)) || (rc = W.valid.alloc(gq))))
        return rc;
    W.ready = true;
    h->ivfnd = std::move(W);
    return VS_OK;
}

// The two-launch route of a short call on a general IVF index (vs_ivf_one_plan's rule; ivf_group_nd_dev goes through it):
// 0 = the group route, 1 = ivf_one_coarse_kernel + ivf_one_scan_kernel per batch, with the coarse launch's
// workgroups, the rows of one unit of the scan and the scan launch's workgroups in out[1..3].  nprobe is the call's,
// clamped to nlist here.
//   Measured over the whole rule (profiles/ivf_one_bench.txt: 1 M synth_sift rows, trained index, nlist 1024, k = 10,
//   us per call back to back, two launches against the group route, spread between repeats under 0.3 %):
//     B = 1 : 96-d 86 / 92 / 139 / 191 against 170 / 187 / 221 / 257 at nprobe 8 / 32 / 128 / 256; 768-d 162 / 322 / 539 / 635
//             against 1873 / 1964 / 2015 / 2072
//     B = 16: 96-d 173 / 247 / 371 / 477 against 202 / 304 / 380 / 523; 128-d 195 / 268 / 383 / 490 against 267 / 327 / 498 /
//             558; 768-d 449 / 556 / 699 / 859 against 2258 / 2397 / 2433 / 2641
//   The closest point is 96-d, B = 16, nprobe 128 (2.4 % faster): the coarse launch's selection costs about 0.4 us per round
//   and query, two queries per wave at B = 16.  Nothing measured is slower, so no shape is taken out; B > 16 is not built.
int ivf_one_route(int64_t n_rows, int nlist, int num_cus, int nb, int B, int k, int nprobe, int64_t* out) {
    out[0] = out[1] = out[2] = out[3] = 0;
    if (nb >= kOneMaxBatches || B > kOneMaxQueries || k > 16 || std::min(nprobe, nlist) > kMaxNprobe) return 0;
    if (n_rows >= (1ll << 31) - 128) return 0;  // (the kernels count rows in 32 bits)
    if (nlist > vs::kIvfOneMaxNlist) return 0;   // (the coarse launch's last workgroup selects from [16][1024] scores in LDS)
    out[0] = 1;
    out[1] = vs::ivf_one_coarse_grid(nlist, num_cus);
    out[2] = vs::kIvfOneUnitRows;
    out[3] = vs::ivf_one_scan_grid(num_cus);
    return 1;
}

// The same for a short call on a general IVF index that keeps a byte copy of its rows, at precision 0 or 2
// (vs_ivf_one_plan_u8's rule; ivf_group_nd_dev goes through it): 0 = the group route, 2 = ivf_one_coarse_kernel in its
// byte-index mode + ivf_one_scan_u8_kernel per batch; out[2] = the rows of one BYTE unit (an fp32 unit of
// the same batch has kIvfOneUnitRows).  The default rule is ivf_one_route's own; a shape leaves it only because it
// measured slower than the route it would replace (include/vsearch.h, vs_ivf_one_plan_u8, lists them with their numbers).
//   Measured (profiles/ivf_one_u8_bench.txt: 1 M synth_sift rows as uint8, trained index, nlist 1024, k = 10, B = 1 / 8 / 16,
//   nprobe 8 / 32 / 128 / 256, 96, 128, 384 and 768-d, us per call back to back; the byte route | the group route on the byte
//   rows | the fp32 two launches on the same index (precision 1)).  Two of the 48 shapes were slower than the group route
//   they would replace, and keep it: B = 16 at nprobe 128 on 96-d rows, 345 | 330 | 369, and B = 16 at nprobe 256 on 128-d
//   rows, 446 | 441 | 488.  Their measured neighbours were faster than both alternatives (96-d B = 16: nprobe 32 234 | 267 |
//   247, nprobe 256 456 | 456 | 474; 128-d B = 16 nprobe 128: 340 | 392 | 380; B = 8 at every nprobe by 2.0 - 16 %), so the
//   exception is those two shapes and nothing around them: what was not measured stays on the rule.
//   One shape is 1.6 % behind the fp32 two launches and stays IN, because the rule could only send it to the group route
//   instead: 96-d, B = 1, nprobe 8: 87.7 | 157.0 | 86.2.
static bool ivf_one_u8_measured_slower(int dim, int B, int probes) {
    return B == 16 && ((dim == 96 && probes == 128) || (dim == 128 && probes == 256));
}
int ivf_one_route_u8(int64_t n_rows, int dim, int nlist, int num_cus, int nb, int B, int k, int nprobe, int64_t* out) {
    if (!ivf_one_route(n_rows, nlist, num_cus, nb, B, k, nprobe, out)) return 0;
    if (ivf_one_u8_measured_slower(dim, B, std::min(nprobe, nlist))) {
        out[0] = out[1] = out[2] = out[3] = 0;
        return 0;
    }
    out[0] = 2;
    out[2] = vs::kIvfOneU8UnitRows;
    return 2;
}

// scratch of the two-launch route, all or nothing (vs_res.h handles); the tickets and counters start at zero
int ensure_ivf_one(vs_index* h) {
    if (h->ivfone.ready) return VS_OK;
    vs_index::IvfOne W;
    int rc;
    const size_t ld = ((size_t)h->nlist + 63) & ~(size_t)63;
    const int np_max = std::min(kMaxNprobe, h->nlist);
    W.units_cap = (int)(std::min<int64_t>((int64_t)kOneMaxQueries * np_max, h->nlist) + h->n_rows / vs::kIvfOneUnitRows);
    // (an index with a byte copy: a list probed by both kinds of query of a batch appears once as byte units and once as
    // fp32 units)
    if (h->d_nd_u8) W.units_cap += (int)(std::min<int64_t>((int64_t)kOneMaxQueries * np_max, h->nlist) + h->n_rows / vs::kIvfOneU8UnitRows);
    const size_t part = (size_t)kOneMaxQueries * vs::kSlotStride * kKcapMax;
    if ((rc = W.scores.alloc(kOneMaxQueries * ld)) || (rc = W.probes.alloc((size_t)kOneMaxQueries * np_max)) || (rc = W.units.alloc((size_t)4 * W.units_cap)) || (rc = W.part_d.alloc(part)) ||
        (rc = W.part_i.alloc(part)) || (rc = W.words.alloc(4)) || (rc = W.counters.alloc(5)))
        return rc;
    HIPCHK(hipMemset(W.words, 0, 4 * sizeof(int32_t)));
    HIPCHK(hipMemset(W.counters, 0, 5 * sizeof(unsigned long long)));
    HIPCHK(hipDeviceSynchronize());  // (the first launches go to the caller's stream, which nothing orders behind the memsets)
    W.ready = true;
    h->ivfone = std::move(W);
    return VS_OK;
}

int ensure_ivf_nd_ip(vs_index* h, hipStream_t s);

// nb < kOneMaxBatches batches of B <= 16 queries, two launches each, everything on s.  plan[0] == 2: the byte route of an
// index with a byte copy of its rows -- the coarse launch in its byte-index mode and ivf_one_scan_u8_kernel, the same
// scratch, tickets and stage marks, counters of its own (vs_ivf_one_u8_stats); under inner product the rows' byte sums
// first (ensure_ivf_nd_ip: one build launch on s at the index's first inner-product call, as on the group route).
int ivf_one_nd_dev(vs_index* h, const int64_t* plan, const float* q_dev, int nb, int B, int k, int nprobe, float* out_d, int32_t* out_i,
                   hipStream_t s) {
    int rc = ensure_ivf_one(h);
    if (rc) return rc;
    const bool bytes = plan[0] == 2;
    if (bytes && h->metric == VS_METRIC_IP && (rc = ensure_ivf_nd_ip(h, s))) return rc;
    vs_index::IvfOne& W = h->ivfone;
    vs::IvfOneU8Params p{};  // (the fp32 route launches its base)
    p.vecs = h->d_vecs;
    p.vnorm = h->d_norm;
    p.offsets = h->d_offsets;
    p.cents = h->d_centroids;
    p.cnorm = h->d_cnorm;
    p.id_map = h->d_r2o;
    p.nlist = h->nlist;
    p.dim = h->dim;
    p.dim_p = h->dim_p;
    p.nprobe = nprobe;
    p.metric = h->metric;
    p.unit_rows = (int)plan[2];
    p.scores = W.scores;
    p.ld = (h->nlist + 63) & ~63;
    p.units = W.units;
    p.units_cap = W.units_cap;
    p.ticket = W.words;
    p.n_units = W.words + 2;
    p.counters = W.counters;
    p.cand_count = h->d_cand;
    if (h->d_nd_stats) p.pair_count = h->d_nd_stats + 1;  // (an index with a byte copy, under vs_set_precision(h, 1): fp32 pairs)
    p.o.nq_valid = B;
    p.o.k1 = k;
    p.o.metric = h->metric;
    p.o.part_d = W.part_d;
    p.o.part_i = W.part_i;
    p.o.done = W.words + 1;
    if (bytes) {
        p.unit_rows = vs::kIvfOneUnitRows;  // (plan[2] is the byte unit's)
        p.unit_rows8 = vs::kIvfOneU8UnitRows;
        p.counters = W.counters + 2;
        p.pair_count8 = h->d_nd_stats;
        p.vecs_u8 = h->d_nd_u8;
        p.rterm = h->d_nd_rterm;
        if (h->metric == VS_METRIC_IP) p.rsum = h->ivfndip.rsum;
        p.dim_b = h->dim_b;
        p.bmax = h->nd_bmax;
        p.n_units8 = W.words + 3;
    }
    const vs::IvfOneParams& pf = p;
    for (int b = 0; b < nb; ++b) {
        p.o.q = q_dev + (size_t)b * B * h->dim;
        p.o.out_d = out_d + (size_t)b * B * k;
        p.o.out_i = out_i + (size_t)b * B * k;
        p.probes = W.probes;
        stage_mark(h, 0, s);  // (a set of marks per batch: centroid_search_ms = the coarse launches, fine_search_ms = the scan launches)
        HIPCHK(bytes ? vs::launch_ivf_one_coarse_u8(p, (int)plan[1], s) : vs::launch_ivf_one_coarse(pf, (int)plan[1], s));
        stage_mark(h, 1, s);
        stage_mark(h, 2, s);
        prof_begin(h, 1, s);
        HIPCHK(bytes ? vs::launch_ivf_one_scan_u8(p, (int)plan[3], s) : vs::launch_ivf_one_scan(pf, (int)plan[3], s));
        prof_end(h, 1, s);
        stage_mark(h, 3, s);
    }
    return VS_OK;
}

// ... of its wide-k groups, the same way
int ensure_ivf_nd_wide(vs_index* h) {
    if (h->ivfndw.ready) return VS_OK;
    int rc = ensure_ivf_nd(h);
    if (rc) return rc;
    vs_index::IvfNdWide W;
    const size_t gq = vs::kIvfNdGroupQ, pairs = gq * h->ivfnd.np_max;
    if ((rc = W.plan.alloc((size_t)3 * h->nlist + 2)) || (rc = W.slots.alloc(pairs)) ||
        (rc = W.items.alloc((size_t)2 * vs::ivf_nd_items_cap(h->nlist, h->ivfnd.np_max))) || (rc = W.tau.alloc(gq)) ||
        (rc = W.mask.alloc(pairs)) || (rc = W.cnt.alloc(gq)) || (rc = W.cand.alloc(gq * vs::kIvfNdWideCand)) || (rc = W.stats.alloc(3)))
        return rc;
    HIPCHK(hipMemset(W.cnt, 0, gq * sizeof(int32_t)));
    HIPCHK(hipMemset(W.stats, 0, 3 * sizeof(unsigned long long)));
    W.ready = true;
    h->ivfndw = std::move(W);
    return VS_OK;
}

// ... and the row term of the inner-product byte scan, the same way: allocated and filled (one launch on s, ahead of
// the scan that reads it) at the first inner-product group of an index with a byte copy
int ensure_ivf_nd_ip(vs_index* h, hipStream_t s) {
    if (h->ivfndip.ready) return VS_OK;
    vs_index::IvfNdIp W;
    int rc;
    if ((rc = W.rsum.alloc((size_t)h->n_rows + 64)) || (rc = W.qsum.alloc((size_t)vs::kIvfNdGroupQ))) return rc;
    HIPCHK(vs::launch_ivf_nd_i8_rowsum(h->d_nd_u8, h->dim_b, h->n_rows, W.rsum, s));
    W.ready = true;
    h->ivfndip = std::move(W);
    return VS_OK;
}

// the fp32 plan of a launch group of a general IVF index on the index's own tables, every pair
vs::IvfNdParams ivf_nd_params(vs_index* h, const float* q_dev, int group_q, int k, int kcap, int nprobe) {
    vs_index::IvfNd& W = h->ivfnd;
    vs::IvfNdParams ip{};
    ip.vecs = h->d_vecs;
    ip.vnorm = h->d_norm;
    ip.offsets = h->d_offsets;
    ip.nlist = h->nlist;
    ip.dim = h->dim;
    ip.dim_p = h->dim_p;
    ip.q = q_dev;
    ip.group_q = group_q;
    ip.nprobe = nprobe;
    ip.k = k;
    ip.kcap = kcap;
    ip.probes = W.probes;
    ip.qrows = W.qrows;
    ip.qnorm = W.qnorm;
    ip.list_cnt = W.plan;
    ip.list_start = W.plan + (size_t)2 * h->nlist;
    ip.n_items = W.plan + (size_t)3 * h->nlist + 1;
    ip.slots = W.slots;
    ip.items = W.items;
    ip.part_d = W.part_d;
    ip.part_i = W.part_i;
    ip.cand_count = h->d_cand;
    if (h->d_nd_stats) ip.pair_count = h->d_nd_stats + 1;
    ip.metric = h->metric;
    return ip;
}

// One launch group of a general IVF index: nb <= 32 batches of B queries ([nb][B][dim], back to back), everything on s.
// Coarse scores per batch are the brute-force general scan's on the centroid table (equal scores: the lower list id,
// launch_pick_probes); then the plan, the list-major scan and the ranking of the group's partial lists.  An index with a
// byte copy of its rows plans twice: the pairs of the queries that qualify for the byte rows (IvfNdI8Params::valid) go to
// ivf_scan_nd_i8_kernel, the others to ivf_scan_nd_kernel, both into the same partial lists.  The metric is the handle's at the
// time of the call (vs_ivf_search_metric* set it for the call's duration): under inner product the coarse scores are
// -(q.c), the scans run their IP instantiations, and the byte scan needs the rows' byte sums (ensure_ivf_nd_ip).
int ivf_group_nd_dev(vs_index* h, const float* q_dev, int nb, int B, int k, int nprobe, float* out_d, int32_t* out_i, hipStream_t s) {
    const int kcap = pick_kcap(k);
    if (!kcap) return refuse_general_ivf(h, "k > 16");
    // a short call: two launches per batch, unless the index was created under VSEARCH_IVF_ONE=0.  An index
    // with a byte copy of its rows takes the fp32 route when no query can run on bytes (vs_set_precision(h, 1)) and the
    // byte route otherwise, unless it was created under VSEARCH_IVF_ONE_U8=0.  The routes share scratch of
    // their own: an index that only ever serves short calls allocates none of the group route's.
    int64_t one_plan[4] = {0, 0, 0, 0};
    if (h->ivf_one && nb >= 1 && B >= 1 && nprobe >= 1 && nprobe <= std::min(kMaxNprobe, h->nlist)) {
        if (!h->d_nd_u8 || h->precision == 1)
            ivf_one_route(h->n_rows, h->nlist, h->num_cus, nb, B, k, nprobe, one_plan);
        else if (h->ivf_one_u8 == 2 && ivf_one_route(h->n_rows, h->nlist, h->num_cus, nb, B, k, nprobe, one_plan))
            one_plan[0] = 2, one_plan[2] = vs::kIvfOneU8UnitRows;
        else if (h->ivf_one_u8 == 1)
            ivf_one_route_u8(h->n_rows, h->dim, h->nlist, h->num_cus, nb, B, k, nprobe, one_plan);
    }
    if (one_plan[0]) return ivf_one_nd_dev(h, one_plan, q_dev, nb, B, k, nprobe, out_d, out_i, s);
    int rc = ensure_ivf_nd(h);
    if (rc) return rc;
    vs_index::IvfNd& W = h->ivfnd;
    if (nb < 1 || nb * B > vs::kIvfNdGroupQ || nprobe > W.np_max) {
        set_error("ivf_group_nd_dev: launch group out of range");
        return VS_ERR_INVALID;
    }
    const int64_t ld = (h->nlist + 63) & ~63;
    stage_mark(h, 0, s);
    for (int b = 0; b < nb; ++b) {
        if ((rc = scores_dev(h, h->d_centroids, h->d_cnorm, h->nlist, q_dev + (size_t)b * B * h->dim, B, h->d_scores, ld, s))) return rc;
        HIPCHK(vs::launch_pick_probes(h->d_scores, ld, B, h->nlist, nprobe, W.probes + (size_t)b * B * nprobe, s));
    }
    stage_mark(h, 1, s);
    vs::IvfNdParams ip = ivf_nd_params(h, q_dev, nb * B, k, kcap, nprobe);
    vs::IvfNdI8Params bp{};
    const bool two_plans = (bool)h->d_nd_u8;
    if (two_plans && h->metric == VS_METRIC_IP && (rc = ensure_ivf_nd_ip(h, s))) return rc;
    if (two_plans) {
        bp.s = ip;
        bp.s.list_cnt = W.plan8;
        bp.s.list_start = W.plan8 + (size_t)2 * h->nlist;
        bp.s.n_items = W.plan8 + (size_t)3 * h->nlist + 1;
        bp.s.slots = W.slots8;
        bp.s.items = W.items8;
        bp.s.route = W.valid;
        bp.s.route_want = 1;
        bp.s.pair_count = h->d_nd_stats;
        bp.vecs_u8 = h->d_nd_u8;
        bp.rterm = h->d_nd_rterm;
        bp.dim_b = h->dim_b;
        bp.bmax = h->nd_bmax;
        bp.all_f32 = h->precision == 1;
        bp.q8rows = W.q8rows;
        bp.qterm = W.qterm;
        bp.valid = W.valid;
        if (h->metric == VS_METRIC_IP) {
            bp.rsum = h->ivfndip.rsum;
            bp.qsum = h->ivfndip.qsum;
        }
        ip.route = W.valid;
        ip.route_want = 0;
        HIPCHK(vs::launch_ivf_nd_i8_prep(bp, s));
    }
    HIPCHK(vs::launch_ivf_nd_plan(ip, s));
    if (two_plans) HIPCHK(vs::launch_ivf_nd_plan_second(bp.s, s));
    stage_mark(h, 2, s);
    prof_begin(h, 1, s);
    HIPCHK(vs::launch_ivf_nd_scan(ip, h->num_cus, s));
    if (two_plans) HIPCHK(vs::launch_ivf_nd_i8_scan(bp, h->num_cus, s));
    prof_end(h, 1, s);
    vs::MergeParams m{};
    m.part_d = W.part_d;
    m.part_i = W.part_i;
    m.G = nprobe;
    m.kin = kcap;
    m.nq = nb * B;
    m.kout = k;
    m.out_d = out_d;
    m.out_i = out_i;
    m.id_map = h->d_r2o;
    HIPCHK(vs::launch_merge_layout(m, kcap, (int64_t)nprobe * kcap, s));
    stage_mark(h, 3, s);
    return VS_OK;
}

// The same launch group at 17 <= k <= 128: coarse, query rows, plan and scan exactly as above at KCAP 16 on
// the fp32 rows with every pair (an index with a byte copy plans once: wide k scans the fp32 rows whatever
// vs_set_precision says); then the bound, the rescan of the saturated pairs into per-query candidate lists, and the ranking.
// Everything on s, no host synchronisation.
int ivf_group_nd_wide_dev(vs_index* h, const float* q_dev, int nb, int B, int k, int nprobe, float* out_d, int32_t* out_i, hipStream_t s) {
    if (k <= 16 || k > vs::kIvfNdWideKMax) {
        set_error("ivf_group_nd_wide_dev: 17 <= k <= 128");
        return VS_ERR_INVALID;
    }
    int rc = ensure_ivf_nd_wide(h);
    if (rc) return rc;
    vs_index::IvfNdWide& X = h->ivfndw;
    if (nb < 1 || nb * B > vs::kIvfNdGroupQ || nprobe > h->ivfnd.np_max) {
        set_error("ivf_group_nd_wide_dev: launch group out of range");
        return VS_ERR_INVALID;
    }
    const int64_t ld = (h->nlist + 63) & ~63;
    stage_mark(h, 0, s);
    for (int b = 0; b < nb; ++b) {
        if ((rc = scores_dev(h, h->d_centroids, h->d_cnorm, h->nlist, q_dev + (size_t)b * B * h->dim, B, h->d_scores, ld, s))) return rc;
        HIPCHK(vs::launch_pick_probes(h->d_scores, ld, B, h->nlist, nprobe, h->ivfnd.probes + (size_t)b * B * nprobe, s));
    }
    stage_mark(h, 1, s);
    vs::IvfNdParams ip = ivf_nd_params(h, q_dev, nb * B, kKcapMax, kKcapMax, nprobe);
    HIPCHK(vs::launch_ivf_nd_plan(ip, s));
    stage_mark(h, 2, s);
    prof_begin(h, 1, s);
    HIPCHK(vs::launch_ivf_nd_scan(ip, h->num_cus, s));
    vs::IvfNdWideParams wp{};
    wp.r = ip;
    wp.r.k = k;
    wp.r.list_cnt = X.plan;
    wp.r.list_start = X.plan + (size_t)2 * h->nlist;
    wp.r.n_items = X.plan + (size_t)3 * h->nlist + 1;
    wp.r.slots = X.slots;
    wp.r.items = X.items;
    wp.r.cand_count = nullptr;  // (counted once, by the first plan)
    wp.r.pair_count = nullptr;
    wp.r.pair_mask = X.mask;
    wp.tau = X.tau;
    wp.pair_mask = X.mask;
    wp.cnt = X.cnt;
    wp.cand = X.cand;
    wp.id_map = h->d_r2o;
    wp.out_d = out_d;
    wp.out_i = out_i;
    wp.stats = X.stats;
    HIPCHK(vs::launch_ivf_nd_wide_bound(wp, s));
    HIPCHK(vs::launch_ivf_nd_plan_second(wp.r, s));
    HIPCHK(vs::launch_ivf_nd_wide_scan(wp, h->num_cus, s));
    prof_end(h, 1, s);
    HIPCHK(vs::launch_ivf_nd_wide_rank(wp, s));
    stage_mark(h, 3, s);
    return VS_OK;
}

// Scratch of one lane of the wide pipeline, sized for launch groups of h->ivf_gb batches in up to h->ivf_nsb super-batches.
int ensure_ivf_wide(vs_index* h, int lane) {
    if (h->wide[lane].ready) return VS_OK;
    vs_index::IvfWide W;
    int rc;
    const size_t nq = (size_t)h->ivf_gb * 32;
    const int n_sb_max = h->ivf_nsb;
    W.n_waves = 0;
    for (int n = 1; n <= n_sb_max; ++n) W.n_waves = std::max(W.n_waves, vs::ivf_wide_waves(h->num_cus, n));
    W.zero_words = (size_t)n_sb_max * vs::ivf_wide_plan_words(h->nlist) + nq + 16 + h->ivf_gb + nq * kWideSub;
    if ((rc = W.lq.alloc((size_t)n_sb_max * h->nlist * vs::kIvfWideQ))) return rc;
    if ((rc = W.zero.alloc(W.zero_words))) return rc;
    HIPCHK(hipMemset(W.zero, 0, W.zero_words * sizeof(int32_t)));
    W.units_cap = (int)std::min<int64_t>(2 * h->n_units_max + 4096, 0x7fffffff / 16);
    if ((rc = W.units.alloc((size_t)n_sb_max * W.units_cap * 4))) return rc;
    if ((rc = W.tau.alloc(nq))) return rc;
    if ((rc = W.tq.alloc((size_t)h->nlist * nq))) return rc;
    if ((rc = W.tk.alloc(nq * vs::kBoundSegs * 16))) return rc;
    if ((rc = W.nseg.alloc(nq))) return rc;
    if ((rc = W.qnorm.alloc(nq))) return rc;
    if ((rc = W.q8.alloc(nq * vs::kDim))) return rc;
    if ((rc = W.qterm.alloc(nq))) return rc;
    if ((rc = W.wbuf.alloc((size_t)W.n_waves * kIvfWideWaveCap))) return rc;
    if ((rc = W.cand_d.alloc(nq * kWideSub * kIvfWideSubCap))) return rc;
    if ((rc = W.cand_i.alloc(nq * kWideSub * kIvfWideSubCap))) return rc;
    if (nq > 2048) {
        if ((rc = W.rank_list.alloc(nq + 1))) return rc;
        HIPCHK(hipMemset(W.rank_list, 0, sizeof(int32_t)));
    }
    W.off_scores = (32ll * kMaxNprobe * 4 + 255) & ~255ll;
    W.slab_stride = (W.off_scores + 32ll * ((h->nlist + 63) & ~63) * 4 + 255) & ~255ll;
    if ((rc = W.slab.alloc((size_t)W.slab_stride * h->ivf_gb))) return rc;
    W.ready = true;
    h->wide[lane] = std::move(W);
    return VS_OK;
}

// Wide-k scratch of one lane (beside ensure_ivf_wide's): built in a local set, so that a failure part way frees what it
// allocated, and moved in when complete.
int ensure_ivf_widek(vs_index* h, int lane) {
    if (h->widek[lane].ready) return VS_OK;
    vs_index::IvfWideK K;
    const size_t nq = (size_t)h->ivf_gb * 32;
    const size_t tk_words = nq * vs::kBoundSegs * vs::kIvfTauRows;
    int rc;
    if ((rc = K.tk.alloc(tk_words)) || (rc = K.kth_d.alloc(nq * vs::kIvfWideKMax)) || (rc = K.kth_i.alloc(nq * vs::kIvfWideKMax)) ||
        (rc = K.wbuf.alloc((size_t)h->wide[lane].n_waves * kIvfWideKWaveCap)) || (rc = K.cand_d.alloc(nq * kWideSub * kIvfWideKSubCap)) ||
        (rc = K.cand_i.alloc(nq * kWideSub * kIvfWideKSubCap)))
        return rc;
    HIPCHK(hipMemsetD32(reinterpret_cast<hipDeviceptr_t>(K.tk.get()), 0x7f800000, tk_words));  // +inf
    static const bool stats = getenv("VSEARCH_IVF_WIDEK_STATS") && atoi(getenv("VSEARCH_IVF_WIDEK_STATS"));  // (diagnostic knob)
    if (stats && !h->widek_stats) {
        if ((rc = h->widek_stats.alloc(4))) return rc;
        HIPCHK(hipMemset(h->widek_stats, 0, 4 * sizeof(unsigned long long)));
    }
    K.ready = true;
    h->widek[lane] = std::move(K);
    return VS_OK;
}

// The zeroed block of a lane: plan words per super-batch | slow [nq] | overflow (16) | invalid [batches] | list counters [16][nq]
struct WideZero {
    int32_t *plan, *slow, *ovf, *invalid, *cnt;
};
WideZero wide_zero(const vs_index* h, const vs_index::IvfWide& W) {
    const size_t nq = (size_t)h->ivf_gb * 32;
    WideZero z;
    z.plan = W.zero;
    z.slow = z.plan + (size_t)h->ivf_nsb * vs::ivf_wide_plan_words(h->nlist);
    z.ovf = z.slow + nq;
    z.invalid = z.ovf + 16;
    z.cnt = z.invalid + h->ivf_gb;
    return z;
}

// Parameters of the wide pipeline's kernels for a launch group of nb batches in super-batches of sbb.
vs::IvfWideParams wide_params(vs_index* h, vs_index::IvfWide& W, const float* q_dev, int nb, int sbb, int B, int k, int nprobe,
                              float* out_d, int32_t* out_i) {
    const WideZero z = wide_zero(h, W);
    const size_t nq = (size_t)h->ivf_gb * 32;
    vs::IvfWideParams wp{};
#ifdef VS_STAMPS
    wp.dbg = g_dbg;
    wp.diag = getenv("VSEARCH_DIAG") ? atoi(getenv("VSEARCH_DIAG")) : 0;
#endif
    wp.vecs = h->d_vecs;
    wp.vnorm = h->d_norm;
    if (h->d_vecs_u8 && h->precision != 1 && h->metric == VS_METRIC_L2) {
        wp.vecs_u8 = h->d_vecs_u8;
        wp.rterm = h->d_rterm;
        wp.vecs_t8 = h->d_vecs_t8;
        wp.nrh_t = h->d_nrh_t;
        wp.rterm_t = h->d_rterm_t;
    }
    // (without the byte path the records and candidates are plain rows: no padded-row offsets)
    wp.tdelta = wp.vecs_t8 ? h->d_tdelta : nullptr;
    wp.chunk_trow0 = wp.vecs_t8 ? h->d_chunk_trow0 : h->d_chunk_row0;
    wp.offsets = h->d_offsets;
    wp.chunk_list = h->d_chunk_list;
    wp.chunk_row0 = h->d_chunk_row0;
    wp.chunk_rows = h->d_chunk_rows;
    wp.n_chunks = h->n_chunks;
    wp.nlist = h->nlist;
    wp.nprobe = nprobe;
    wp.k = k;
    wp.metric = h->metric;
    wp.q = q_dev;
    wp.q_batch_bytes = (long long)B * vs::kDim * sizeof(float);
    wp.n_batches = nb;
    wp.B = B;
    wp.sb_batches = sbb;
    wp.qnorm = W.qnorm;
    wp.q8 = W.q8;
    wp.qterm = W.qterm;
    wp.invalid = z.invalid;
    wp.probes = reinterpret_cast<int32_t*>(W.slab.get());
    wp.probes_batch_bytes = W.slab_stride;
    wp.lq = W.lq;
    wp.zero = z.plan;
    wp.cand_count = h->d_cand;
    wp.units = W.units;
    wp.units_sb_stride = (long long)W.units_cap * 4;
    wp.units_cap = W.units_cap;
    wp.tq = W.tq;
    wp.tq_cap = (int)nq;
    wp.tk = W.tk;
    wp.nseg = W.nseg;
    wp.tau = W.tau;
    wp.slow = z.slow;
    wp.sink.wbuf = W.wbuf;
    wp.sink.wcap = kIvfWideWaveCap;
    wp.sink.overflow = z.ovf;
    wp.sink.cnt = z.cnt;
    wp.sink.cand_d = W.cand_d;
    wp.sink.cand_i = W.cand_i;
    wp.sink.cap = kIvfWideSubCap;
    wp.sink.nsub = kWideSub;
    wp.sink.slow = z.slow;
    wp.sink.xcd_subs = kWideSub / 8;
    wp.sink.cnt_sub_stride = (int)nq;
    wp.out_d = out_d;
    wp.out_i = out_i;
    wp.id_map = h->d_r2o;
    return wp;
}

vs::IvfGroup wide_group(vs_index* h, vs_index::IvfWide& W, int sbb, int B) {
    const WideZero z = wide_zero(h, W);
    vs::IvfGroup grp{};
    grp.mb.slab = W.slab_stride;
    grp.mb.probes = W.slab_stride;  // (the probes sit at the head of a batch's slab)
    grp.mb.q = (long long)B * vs::kDim * sizeof(float);
    grp.sb_batches = sbb;
    grp.w_qnorm = W.qnorm;
    grp.w_q8 = W.q8;
    grp.w_qterm = W.qterm;
    grp.w_invalid = z.invalid;
    grp.w_overflow = z.ovf;
    grp.w_glist = W.rank_list;
    grp.w_cnt = z.plan;
    grp.w_lq = W.lq;
    grp.w_q = vs::kIvfWideQ;
    grp.w_tq = W.tq;
    grp.w_tq_cap = h->ivf_gb * 32;
    grp.w_tcnt = z.plan;
    grp.w_nseg = W.nseg;
    grp.t_offsets = h->d_offsets;
#ifdef VS_STAMPS
    grp.dbg = g_dbg ? g_dbg + 4096 * 16 : nullptr;
#endif
    return grp;
}

// scan + rank of a launch group whose slot tables, bounds and plan are in place
int wide_scan_rank(vs_index* h, vs_index::IvfWide& W, const vs::IvfWideParams& wp, hipStream_t s) {
    const WideZero z = wide_zero(h, W);
    const size_t nq = (size_t)h->ivf_gb * 32;
    prof_begin(h, 1, s);  // (the profiling window holds the scan kernel alone)
    HIPCHK(vs::launch_ivf_wide_scan(wp, h->num_cus, s));
    prof_end(h, 1, s);
    vs::MergeParams m{};
    m.part_d = W.cand_d;
    m.part_i = W.cand_i;
    m.G = kWideSub;
    m.kin = kIvfWideSubCap;
    m.nq = wp.n_batches * wp.B;
    m.kout = wp.k;
    m.out_d = wp.out_d;
    m.out_i = wp.out_i;
    m.q_group_out = wp.B;
    m.q_group_in = vs::kMaxBatch;
    m.flat_len = z.cnt;
    m.flat_len_sub_stride = (int)nq;
    m.id_map = (wp.vecs_t8 && h->d_r2o_t) ? h->d_r2o_t : h->d_r2o;  // the byte scan's candidates are padded rows
#ifdef VS_STAMPS
    m.dbg = g_dbg ? g_dbg + 8192 * 16 : nullptr;
#endif
    HIPCHK(vs::launch_ivf_wide_rank(m, kIvfWideSubCap, (int64_t)kWideSub * kIvfWideSubCap, wp, s, W.rank_list));
    return VS_OK;
}

// nb <= h->ivf_gb independent batches (one launch group) through the wide pipeline on scratch lane `lane`: coarse (MFMA,
// also prepares the byte queries) + pick (also fills the lists' slot tables), bounds and plan in one launch, ONE list-major
// pass per super-batch of 32 batches with candidates to the sink (binned by the scan's own waves), and the ranking launch
// (merge, or the exact slow path for queries without a bound / for everybody if a candidate buffer overflowed).
// The same for 17 <= k <= 128: coarse + pick as above; bounds + plan with the segments' distances stored, their k-th
// (topk_wide_kernel) as the bound; the scan reading those bounds into the wide-k sink; the wide-k ranking.
int ivf_group_widek_dev(vs_index* h, int lane, const float* q_dev, int nb, int B, int k, int nprobe, float* out_d, int32_t* out_i,
                        hipStream_t s) {
    int rc;
    if ((rc = ensure_ivf_wide(h, lane)) || (rc = ensure_ivf_widek(h, lane))) return rc;
    vs_index::IvfWide& W = h->wide[lane];
    vs_index::IvfWideK& K = h->widek[lane];
    if (W.dirty) {  // (a failed call may also have left segment distances behind)
        HIPCHK(hipMemsetAsync(W.zero, 0, W.zero_words * sizeof(int32_t), s));
        HIPCHK(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(K.tk.get()), 0x7f800000, (size_t)h->ivf_gb * 32 * vs::kBoundSegs * vs::kIvfTauRows, s));
    }
    W.dirty = true;
    const int sbb = vs::kIvfWideBatches;
    const vs::IvfGroup grp = wide_group(h, W, sbb, B);
    vs::IvfWideParams wp = wide_params(h, W, q_dev, nb, sbb, B, k, nprobe, out_d, out_i);
    wp.tau_inline = 0;  // (the scan reads tau / slow)
    wp.tk = K.tk;
    wp.sink.wbuf = K.wbuf;
    wp.sink.wcap = kIvfWideKWaveCap;
    wp.sink.cand_d = K.cand_d;
    wp.sink.cand_i = K.cand_i;
    wp.sink.cap = kIvfWideKSubCap;
    stage_mark(h, 0, s);
    HIPCHK(vs::launch_ivf_coarse_pick(q_dev, B, h->d_centroids, h->d_cnorm, h->nlist, nprobe, h->metric,
                                      reinterpret_cast<float*>(W.slab + W.off_scores), (h->nlist + 63) & ~63,
                                      reinterpret_cast<int32_t*>(W.slab.get()), grp, s, nb));
    stage_mark(h, 1, s);
    HIPCHK(vs::launch_ivf_widek_bounds_plan(wp, K.kth_d, K.kth_i, s));
    stage_mark(h, 2, s);
    prof_begin(h, 1, s);
    HIPCHK(vs::launch_ivf_wide_scan(wp, h->num_cus, s));
    prof_end(h, 1, s);
    const int32_t* id_map = (wp.vecs_t8 && h->d_r2o_t) ? h->d_r2o_t : h->d_r2o;  // (as wide_scan_rank: padded rows on the byte path)
    HIPCHK(vs::launch_ivf_widek_rank(wp, id_map, h->widek_stats.get(), s));
    W.dirty = false;
    stage_mark(h, 3, s);
    return VS_OK;
}

int ivf_group_wide_dev(vs_index* h, int lane, const float* q_dev, int nb, int B, int k, int nprobe, float* out_d, int32_t* out_i, hipStream_t s) {
    if (k > 16) return ivf_group_widek_dev(h, lane, q_dev, nb, B, k, nprobe, out_d, out_i, s);
    int rc = ensure_ivf_wide(h, lane);
    if (rc) return rc;
    vs_index::IvfWide& W = h->wide[lane];
    // The zeroed block is left zeroed by the group's last kernel (ivf_wide_rank_kernel): a memset only after a call that
    // did not get as far as that launch.
    if (W.dirty) HIPCHK(hipMemsetAsync(W.zero, 0, W.zero_words * sizeof(int32_t), s));
    W.dirty = true;
    const int sbb = vs::kIvfWideBatches;
    const vs::IvfGroup grp = wide_group(h, W, sbb, B);
    vs::IvfWideParams wp = wide_params(h, W, q_dev, nb, sbb, B, k, nprobe, out_d, out_i);
    wp.tau_inline = 1;  // (bounds launch and scan are in this one pipeline: the scan merges a query's segment lists itself)
    stage_mark(h, 0, s);
    HIPCHK(vs::launch_ivf_coarse_pick(q_dev, B, h->d_centroids, h->d_cnorm, h->nlist, nprobe, h->metric,
                                      reinterpret_cast<float*>(W.slab + W.off_scores), (h->nlist + 63) & ~63,
                                      reinterpret_cast<int32_t*>(W.slab.get()), grp, s, nb));
    stage_mark(h, 1, s);
    HIPCHK(vs::launch_ivf_wide_bounds_plan(wp, s));
    stage_mark(h, 2, s);  // "gather" (IVFIndex.cpp's second stage) = bounds + plan here; the fine search is the scan + ranking
    if ((rc = wide_scan_rank(h, W, wp, s))) return rc;
#ifdef VS_STAMPS
    W.dirty = (wp.diag & 128) != 0;
#else
    W.dirty = false;
#endif
    stage_mark(h, 3, s);
    return VS_OK;
}

// ---- cluster-sharded pipeline (SURVEY 8e / BASELINE configs[4]).  A launch group is cut into `world` slices of sbb batches;
// slice r's per-query stages (coarse scores, probe selection, bound) run on rank r ONLY, their output -- a block of
// int32 words: probes [sbb * 32][nprobe] | tau [sbb * 32] | slow [sbb * 32] -- is exchanged (one all-gather), and every
// rank then scans its resident lists for ALL slices (slice = super-batch of the list-major pass).  What a rank does
// per launch group is therefore what an unsharded index does for ONE slice, except the ranking (all queries, an eighth of
// the candidates each).
long long ivf_block_words(int sbb, int nprobe) { return (long long)sbb * 32 * (nprobe + 2); }
// slice of `rank` in a launch group of nb batches on `world` ranks: sbb batches per slice, its own [b0, b0 + nbs)
void ivf_slice(int nb, int world, int rank, int& sbb, int& b0, int& nbs) {
    sbb = (nb + world - 1) / world;
    b0 = rank * sbb;
    nbs = std::max(0, std::min(sbb, nb - b0));
}

// front half on rank h->rank: prepares ALL queries of the group (bytes, terms, norms: the scan needs them for every
// slice), scores its own slice [b0, b0 + nbs) and writes the slice's block to `blk`
int ivf_shard_front(vs_index* h, int lane, const float* q_dev, int nb, int sbb, int b0, int nbs, int B, int k, int nprobe, int32_t* blk,
                    hipStream_t s) {
    int rc = ensure_ivf_wide(h, lane);
    if (rc) return rc;
    vs_index::IvfWide& W = h->wide[lane];
    if (W.dirty) HIPCHK(hipMemsetAsync(W.zero, 0, W.zero_words * sizeof(int32_t), s));
    W.dirty = true;
    vs::IvfGroup grp = wide_group(h, W, sbb, B);
    HIPCHK(vs::launch_ivf_prep_queries(q_dev, B, h->d_centroids, h->d_cnorm, h->nlist, grp, s, nb));
    const long long sb_q = (long long)sbb * 32;
    HIPCHK(hipMemsetAsync(blk + sb_q * nprobe + sb_q, 0, (size_t)sb_q * sizeof(int32_t), s));  // the slice's `slow` marks
    if (nbs <= 0) return VS_OK;
    // the slice's launches see their own batches only: every per-batch / per-query array is advanced to batch b0
    const size_t q0 = (size_t)b0 * 32;
    vs::IvfGroup fg = grp;
    fg.w_qnorm = nullptr;
    fg.w_q8 = nullptr;
    fg.w_qterm = nullptr;
    fg.w_invalid = nullptr;
    fg.w_overflow = nullptr;
    fg.w_glist = nullptr;
    fg.w_cnt = nullptr;  // (slot tables are filled after the exchange, for all slices)
    fg.w_lq = nullptr;
    fg.mb.probes = (long long)32 * nprobe * sizeof(int32_t);
    fg.t_offsets = h->d_head_vecs ? h->d_head_off : h->d_offsets;  // (the rows the bounds come from, see below)
    const float* qs = q_dev + (size_t)b0 * B * vs::kDim;
    HIPCHK(vs::launch_ivf_coarse_pick(qs, B, h->d_centroids, h->d_cnorm, h->nlist, nprobe, h->metric,
                                      reinterpret_cast<float*>(W.slab + W.off_scores), (h->nlist + 63) & ~63, blk, fg, s, nbs));
    vs::IvfWideParams wp = wide_params(h, W, qs, nbs, sbb, B, k, nprobe, nullptr, nullptr);
    wp.qnorm = W.qnorm + q0;
    wp.q8 = W.q8 + q0 * vs::kDim;
    wp.qterm = W.qterm + q0;
    wp.invalid = wp.invalid + b0;
    wp.probes = blk;
    wp.probes_batch_bytes = fg.mb.probes;
    wp.tau = reinterpret_cast<float*>(blk + sb_q * nprobe);
    wp.slow = blk + sb_q * nprobe + sb_q;
    if (h->d_head_vecs) {  // the bound's rows: the replicated heads of the query's two nearest lists, wherever those live
        wp.vecs = h->d_head_vecs;
        wp.vnorm = h->d_head_norm;
        wp.offsets = h->d_head_off;
        const bool bytes = h->d_head_t8 && h->precision != 1 && h->metric == VS_METRIC_L2;
        wp.vecs_u8 = bytes ? h->d_head_t8 : nullptr;  // (non-null = "byte rows exist"; the tiled copy is what is read)
        wp.rterm = nullptr;
        wp.vecs_t8 = bytes ? h->d_head_t8 : nullptr;
        wp.rterm_t = bytes ? h->d_head_rterm_t : nullptr;
        wp.nrh_t = nullptr;
        wp.tdelta = bytes ? h->d_head_tdelta : nullptr;
    }
    HIPCHK(vs::launch_ivf_wide_bounds_plan(wp, s, 1));  // bounds only
    return VS_OK;
}

// back half: slot tables for all slices from the exchanged blocks, plan, scan, rank -> this rank's top-k of every query
int ivf_shard_back(vs_index* h, int lane, const float* q_dev, int nb, int sbb, int B, int k, int nprobe, const int32_t* gathered,
                   float* out_d, int32_t* out_i, hipStream_t s) {
    vs_index::IvfWide& W = h->wide[lane];
    const WideZero z = wide_zero(h, W);
    const vs::IvfGroup grp = wide_group(h, W, sbb, B);
    const vs::IvfWideParams wp = wide_params(h, W, q_dev, nb, sbb, B, k, nprobe, out_d, out_i);
    HIPCHK(vs::launch_ivf_fill(gathered, ivf_block_words(sbb, nprobe), B, nprobe, h->nlist, h->d_offsets, reinterpret_cast<int32_t*>(W.slab.get()),
                               W.tau, z.slow, grp, s, nb));
    HIPCHK(vs::launch_ivf_wide_bounds_plan(wp, s, 2));  // plan only
    int rc = wide_scan_rank(h, W, wp, s);
    if (rc) return rc;
    W.dirty = false;
    return VS_OK;
}

int ensure_wide_streams(vs_index* h) {
    if (h->wide_streams_ready) return VS_OK;
    vs::Stream st[kWideLanesMax];
    vs::Event join[kWideLanesMax], fork;
    int rc;
    for (int i = 0; i < kWideLanesMax; ++i)
        if ((rc = st[i].create()) || (rc = join[i].create())) return rc;
    if ((rc = fork.create())) return rc;
    for (int i = 0; i < kWideLanesMax; ++i) {
        h->wide_stream[i] = std::move(st[i]);
        h->wide_join[i] = std::move(join[i]);
    }
    h->wide_fork = std::move(fork);
    h->wide_streams_ready = true;
    return VS_OK;
}

// k: the call's (the output buffers hold 64 results per query, 128 from the first call with k > 64 on)
int ensure_ivf_host(vs_index* h, int k = 0) {
    int rc;
    h->ivf_host_cap = std::max<int64_t>(kIvfHostChunk, (int64_t)h->ivf_gb * 32);
    const size_t cap = (size_t)h->ivf_host_cap;
    for (auto& slot : h->ihs) {
        if (slot.ready && k <= slot.out_k) continue;
        if (slot.ready) HIPCHK(hipDeviceSynchronize());  // (growing: a failed call's copies may still use the old buffers)
        vs_index::IvfHostSlot S;
        S.out_k = std::max(k > 64 ? vs::kIvfWideKMax : 64, slot.ready ? slot.out_k : 0);
        const size_t out = cap * S.out_k * 2;
        if ((rc = S.pin_q.alloc(cap * h->dim)) || (rc = S.pin_out.alloc(out)) || (rc = S.d_q.alloc(cap * h->dim)) ||
            (rc = S.d_out.alloc(out)) || (rc = S.ev_h2d.create()) || (rc = S.ev_comp[0].create()) || (rc = S.ev_comp[1].create()) ||
            (rc = S.ev_d2h.create()))
            return rc;
        S.ready = true;
        slot = std::move(S);
    }
    return VS_OK;
}

// nb batches on the device, any number: launch groups of h->ivf_gb batches, alternating between the lanes' streams when
// there is more than one group (a group is a chain of dependent kernels, several of them small: the next group's small
// kernels fill the device beside the current group's scan and ranking)
int ivf_multi_dev(vs_index* h, const float* q_dev, int nb, int B, int k, int nprobe, float* out_d, int32_t* out_i, hipStream_t user) {
    int rc = VS_OK;
    if (k > vs::kIvfWideKMax || (k > 16 && !h->general && !ivf_wide_ok(h, k))) {
        set_error(k > vs::kIvfWideKMax ? "k > 128 not supported"
                                       : "k > 16 needs the list-major IVF pipeline (nlist <= 4096, rows resident)");
        return VS_ERR_UNSUPPORTED;
    }
    if (h->general) {  // launch groups of up to 32 batches, all on the caller's stream
        for (int b0 = 0; b0 < nb && !rc; b0 += vs::kIvfWideBatches)
            rc = (k > 16 ? ivf_group_nd_wide_dev : ivf_group_nd_dev)(h, q_dev + (size_t)b0 * B * h->dim, std::min(vs::kIvfWideBatches, nb - b0), B, k,
                                                                     nprobe, out_d + (size_t)b0 * B * k, out_i + (size_t)b0 * B * k, user);
        return rc;
    }
    if (!ivf_wide_ok(h, k)) {
        for (int b = 0; b < nb && !rc; ++b)
            rc = ivf_fallback_batch_dev(h, q_dev + (size_t)b * B * h->dim, B, k, nprobe, out_d + (size_t)b * B * k, out_i + (size_t)b * B * k, user);
        return rc;
    }
    const int gb = h->ivf_gb;
    const int groups = (nb + gb - 1) / gb;
    const int lanes = std::min({h->ivf_lanes, kWideLanesMax, groups});
    if (lanes <= 1) {
        for (int b0 = 0; b0 < nb && !rc; b0 += gb)
            rc = ivf_group_wide_dev(h, 0, q_dev + (size_t)b0 * B * h->dim, std::min(gb, nb - b0), B, k, nprobe, out_d + (size_t)b0 * B * k,
                                    out_i + (size_t)b0 * B * k, user);
        return rc;
    }
    if ((rc = ensure_wide_streams(h))) return rc;
    HIPCHK(hipEventRecord(h->wide_fork, user));
    for (int i = 0; i < lanes; ++i) HIPCHK(hipStreamWaitEvent(h->wide_stream[i], h->wide_fork, 0));
    int g = 0;
    for (int b0 = 0; b0 < nb && !rc; b0 += gb, ++g)
        rc = ivf_group_wide_dev(h, g % lanes, q_dev + (size_t)b0 * B * h->dim, std::min(gb, nb - b0), B, k, nprobe, out_d + (size_t)b0 * B * k,
                                out_i + (size_t)b0 * B * k, h->wide_stream[g % lanes]);
    for (int i = 0; i < lanes; ++i) {  // (also after an error: the user's stream must not run ahead of what was enqueued)
        HIPCHK(hipEventRecord(h->wide_join[i], h->wide_stream[i]));
        HIPCHK(hipStreamWaitEvent(user, h->wide_join[i], 0));
    }
    return rc;
}

// no C++ exception leaves the C ABI (vs_status instead)
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

// Calls on one index may arrive on different caller streams, but its scratch is one set: every enqueue waits for the
// previous call's work (an event), so that two calls never overlap on the device.
int order_begin(vs_index* h, hipStream_t s) {
    // Calls that stay on one stream are ordered by the stream itself: no event traffic (two runtime calls and two
    // barrier packets per search call are what a single-query call's latency is made of).  A call on ANOTHER stream than
    // the previous one waits for everything enqueued on that one so far.
    int rc;
    if (!h->ev_busy && (rc = h->ev_busy.create())) return rc;
    if (h->have_last && h->last_stream != s) {
        HIPCHK(hipEventRecord(h->ev_busy, h->last_stream));
        HIPCHK(hipStreamWaitEvent(s, h->ev_busy, 0));
    }
    h->last_stream = s;  // (set here, not at the end: a call that fails half way has still enqueued work on s)
    h->have_last = true;
    return VS_OK;
}
int order_end(vs_index*, hipStream_t) { return VS_OK; }

// A call that failed half way leaves chunks marked in flight in the host-buffer slots: wait for the streams their work
// went to, then free the slots (nothing of that call may land in, or be retired into, THIS call's buffers).
template <class Slot>
void settle_slots(Slot (&slots)[2], std::initializer_list<hipStream_t> streams) {
    if (slots[0].q0 < 0 && slots[1].q0 < 0) return;
    for (hipStream_t s : streams) (void)hipStreamSynchronize(s);
    slots[0].q0 = slots[1].q0 = -1;
}

int ensure_pipe(vs_index* h) {
    if (h->pipe_ready) return VS_OK;
    const size_t nqc = (size_t)kMaxMulti * 32;
    vs_index::PipeSlot P[2];
    vs::Stream h2d, d2h;
    int rc;
    for (int i = 0; i < 2; ++i) {
        vs_index::PipeSlot& S = P[i];
        if ((rc = S.pin_q.alloc(nqc * h->dim)) || (rc = S.pin_out.alloc(nqc * (2 * vs::kTopkWideMax + 1) * sizeof(float)))) return rc;
        if (i == 1 && ((rc = S.own_q.alloc(nqc * h->dim)) || (rc = S.own_out_d.alloc(nqc * vs::kTopkWideMax)) ||
                       (rc = S.own_out_i.alloc(nqc * vs::kTopkWideMax)) ||
                       (rc = S.own_flags.alloc(nqc))))
            return rc;
        if ((rc = S.ev_h2d.create()) || (rc = S.ev_comp.create()) || (rc = S.ev_d2h.create())) return rc;
    }
    if ((rc = h2d.create()) || (rc = d2h.create())) return rc;
    P[0].d_q = h->d_q;
    P[0].d_out_d = h->d_out_d;
    P[0].d_out_i = h->d_out_i;
    P[0].d_flags = h->d_flags;
    P[1].d_q = P[1].own_q;
    P[1].d_out_d = P[1].own_out_d;
    P[1].d_out_i = P[1].own_out_i;
    P[1].d_flags = P[1].own_flags;
    for (int i = 0; i < 2; ++i) h->pipe[i] = std::move(P[i]);
    h->s_h2d = std::move(h2d);
    h->s_d2h = std::move(d2h);
    h->pipe_ready = true;
    return VS_OK;
}

}  // namespace

// =============================================================================================== C ABI
extern "C" {

const char* vs_version(void) { return "vsearch-hip 0.1 (gfx950)"; }

int vs_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

int64_t vs_index_rows(const vs_index* h) { return h ? h->n_total : 0; }
int vs_index_dim(const vs_index* h) { return h ? h->dim : 0; }
float vs_f32_filter_bound(double eq, double nq, double nqp, double bmax, double emax, double bpmax) {
    return vs::filter_bound(eq, nq, nqp, vs::FilterStats{bmax, emax, bpmax});
}
int vs_bf_filter_image_read(const vs_index* h, int64_t row0, int64_t n, uint16_t* dst) {
    if (!h || !dst || !h->filter_ok || !h->d_img || row0 < 0 || n < 0 || row0 + n > h->n_rows + vs::kScanPadRows) {
        set_error("vs_bf_filter_image_read: no image or rows out of range");
        return VS_ERR_INVALID;
    }
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(dst, h->d_img + (size_t)row0 * vs::kDim, (size_t)n * vs::kDim * sizeof(uint16_t), hipMemcpyDeviceToHost));
    return VS_OK;
}
float vs_f32_filter_cnorm(double bnmax) { return vs::filter_cnorm(bnmax); }
float vs_f32_filter_th2(float thr, float e, float cnorm) { return vs::filter_th2(thr, e, cnorm); }
int vs_bf_filter_stats(vs_index* h, int64_t* out, int reset) {
    if (!h || !out || !h->filter_ok || !h->filter_stats) {
        set_error("vs_bf_filter_stats: an index with the bf16 prefilter and an output of four words");
        return VS_ERR_INVALID;
    }
    HIPCHK(hipSetDevice(h->device));
    unsigned long long v[4];
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(v, h->filter_stats, sizeof(v), hipMemcpyDeviceToHost));
    out[0] = h->filter_launches;
    for (int i = 1; i < 4; ++i) out[i] = (int64_t)v[i];
    if (reset) {
        HIPCHK(hipMemset(h->filter_stats, 0, sizeof(v)));
        h->filter_launches = 0;
    }
    return VS_OK;
}
int vs_index_nlist(const vs_index* h) { return h ? h->nlist : 0; }
void vs_destroy(vs_index* h) {
    if (!h) return;
    (void)hipSetDevice(h->device);
    (void)hipDeviceSynchronize();  // (the handles release without waiting for queued work)
    delete h;
}

int vs_set_batch(vs_index* h, int batch) {
    if (!h || batch < 1 || batch > vs::kMaxBatch) {
        set_error("batch must be in 1..32");
        return VS_ERR_INVALID;
    }
    h->batch = batch;
    return VS_OK;
}

int vs_prof_enable(vs_index* h, int on) {
    if (!h) return VS_ERR_INVALID;
    h->prof = on != 0;
    for (auto& ps : h->prof_slot) ps.used = 0;
    return VS_OK;
}

int vs_ivf_widek_stats(vs_index* h, int64_t* out, int reset) {
    if (refuse_general_bf(h, "vs_ivf_widek_stats") || refuse_general_ivf(h, "vs_ivf_widek_stats")) return VS_ERR_UNSUPPORTED;
    if (!h || h->kind != 1 || !out) {
        set_error("vs_ivf_widek_stats: bad arguments");
        return VS_ERR_INVALID;
    }
    if (!h->widek_stats) {
        set_error("vs_ivf_widek_stats: no wide-k call since VSEARCH_IVF_WIDEK_STATS=1 was set");
        return VS_ERR_UNSUPPORTED;
    }
    int rc = set_device(h);
    if (rc) return rc;
    unsigned long long v[4];
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(v, h->widek_stats, sizeof(v), hipMemcpyDeviceToHost));
    for (int i = 0; i < 4; ++i) out[i] = (int64_t)v[i];
    if (reset) HIPCHK(hipMemset(h->widek_stats, 0, sizeof(v)));
    return VS_OK;
}

int vs_ivf_nd_widek_stats(vs_index* h, int64_t* out, int reset) {
    if (!h || h->kind != 1 || !h->general || !out) {
        set_error("vs_ivf_nd_widek_stats: a general IVF index and an output of three words");
        return VS_ERR_INVALID;
    }
    int rc = set_device(h);
    if (rc) return rc;
    HIPCHK(hipDeviceSynchronize());
    unsigned long long v[3] = {0, 0, 0};  // (no wide-k call yet: nothing counted)
    if (h->ivfndw.ready) {
        HIPCHK(hipMemcpy(v, h->ivfndw.stats, sizeof(v), hipMemcpyDeviceToHost));
        if (reset) HIPCHK(hipMemset(h->ivfndw.stats, 0, sizeof(v)));
    }
    for (int i = 0; i < 3; ++i) out[i] = (int64_t)v[i];
    return VS_OK;
}

int vs_ivf_nd_u8_stats(vs_index* h, int64_t* out, int reset) {
    if (!h || h->kind != 1 || !h->d_nd_stats || !out) {
        set_error("vs_ivf_nd_u8_stats: a general IVF index made by vs_ivf_create_nd_u8 and an output of two words");
        return VS_ERR_INVALID;
    }
    int rc = set_device(h);
    if (rc) return rc;
    unsigned long long v[2];
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(v, h->d_nd_stats, sizeof(v), hipMemcpyDeviceToHost));
    out[0] = (int64_t)v[0];
    out[1] = (int64_t)v[1];
    if (reset) HIPCHK(hipMemset(h->d_nd_stats, 0, sizeof(v)));
    return VS_OK;
}

int vs_ivf_one_stats(vs_index* h, int64_t* out, int reset) {
    if (!h || h->kind != 1 || !h->general || !out) {
        set_error("vs_ivf_one_stats: a general IVF index and an output of two words");
        return VS_ERR_INVALID;
    }
    int rc = set_device(h);
    if (rc) return rc;
    unsigned long long v[2] = {0, 0};
    HIPCHK(hipDeviceSynchronize());
    if (h->ivfone.ready) {  // (zero before the index's first short call)
        HIPCHK(hipMemcpy(v, h->ivfone.counters, sizeof(v), hipMemcpyDeviceToHost));
        if (reset) HIPCHK(hipMemset(h->ivfone.counters, 0, sizeof(v)));
    }
    out[0] = (int64_t)v[0];
    out[1] = (int64_t)v[1];
    return VS_OK;
}

int vs_ivf_one_u8_stats(vs_index* h, int64_t* out, int reset) {
    if (!h || h->kind != 1 || !h->general || !h->d_nd_u8 || !out) {
        set_error("vs_ivf_one_u8_stats: a general IVF index that keeps a byte copy of its rows and an output of three words");
        return VS_ERR_INVALID;
    }
    int rc = set_device(h);
    if (rc) return rc;
    unsigned long long v[3] = {0, 0, 0};
    HIPCHK(hipDeviceSynchronize());
    if (h->ivfone.ready) {  // (zero before the index's first short call)
        HIPCHK(hipMemcpy(v, h->ivfone.counters + 2, sizeof(v), hipMemcpyDeviceToHost));
        if (reset) HIPCHK(hipMemset(h->ivfone.counters + 2, 0, sizeof(v)));
    }
    for (int i = 0; i < 3; ++i) out[i] = (int64_t)v[i];
    return VS_OK;
}

int vs_prof_read(vs_index* h, int which, double* total_ms, int64_t* launches) {
    if (!h || which < 0 || which > 1) return VS_ERR_INVALID;
    int rc = set_device(h);
    if (rc) return rc;
    ProfSlot& ps = h->prof_slot[which];
    double tot = 0;
    for (int i = 0; i + 1 < ps.used; i += 2) {
        HIPCHK(hipEventSynchronize(ps.ev[i + 1]));
        float ms = 0;
        HIPCHK(hipEventElapsedTime(&ms, ps.ev[i], ps.ev[i + 1]));
        tot += ms;
    }
    if (total_ms) *total_ms = tot;
    if (launches) *launches = ps.used / 2;
    return VS_OK;
}

int vs_prof_read_launches(vs_index* h, int which, double* ms_out, int64_t cap, int64_t* launches) {
    if (!h || which < 0 || which > 1 || (cap > 0 && !ms_out)) return VS_ERR_INVALID;
    int rc = set_device(h);
    if (rc) return rc;
    ProfSlot& ps = h->prof_slot[which];
    int64_t n = 0;
    for (int i = 0; i + 1 < ps.used; i += 2, ++n) {
        if (n >= cap) continue;
        HIPCHK(hipEventSynchronize(ps.ev[i + 1]));
        float ms = 0;
        HIPCHK(hipEventElapsedTime(&ms, ps.ev[i], ps.ev[i + 1]));
        ms_out[n] = ms;
    }
    if (launches) *launches = n;
    return VS_OK;
}

// ------------------------------------------------------------------------------------- brute force
static int bf_create_impl(const float* base_host, int64_t n_rows, int dim, int metric, int device, int64_t id_offset, vs_index** out,
                          bool any_dim, const uint8_t* rows_u8 = nullptr, bool force_general = false);
int vs_bf_create(const float* base_host, int64_t n_rows, int dim, int metric, int device, int64_t id_offset,
                 vs_index** out) {
    return guarded([&]() -> int { return bf_create_impl(base_host, n_rows, dim, metric, device, id_offset, out, false); });
}
int vs_bf_create_nd(const float* base_host, int64_t n_rows, int dim, int metric, int device, int64_t id_offset, vs_index** out) {
    return guarded([&]() -> int { return bf_create_impl(base_host, n_rows, dim, metric, device, id_offset, out, true); });
}
// uint8 rows: the checks of vs_bf_create_nd, then the rows as floats through the same path, plus the byte copy
int vs_bf_create_nd_u8(const uint8_t* base_host, int64_t n_rows, int dim, int device, int64_t id_offset, vs_index** out) {
    return guarded([&]() -> int {
        if (!out || !base_host || n_rows <= 0) {
            set_error("vs_bf_create_nd_u8: bad arguments");
            return VS_ERR_INVALID;
        }
        if (dim < 1) {
            set_error("vs_bf_create_nd_u8: dim must be at least 1");
            return VS_ERR_INVALID;
        }
        if (dim > vs::kNdMaxDim) {
            set_error("vs_bf_create_nd_u8: dim > 2048 is not compiled in");
            return VS_ERR_UNSUPPORTED;
        }
        std::vector<float> f((size_t)n_rows * dim);
        for (size_t i = 0; i < f.size(); ++i) f[i] = (float)base_host[i];
        return bf_create_impl(f.data(), n_rows, dim, VS_METRIC_L2, device, id_offset, out, true, base_host);
    });
}
// ... under a metric.  Squared L2 is vs_bf_create_nd_u8 itself; inner product builds the general index at every dimension,
// 128 included (the specialised 128-d index has no inner-product byte kernel), with the byte copy and its row sums
int vs_bf_create_nd_u8_metric(const uint8_t* base_host, int64_t n_rows, int dim, int metric, int device, int64_t id_offset,
                              vs_index** out) {
    if (out && base_host && n_rows > 0 && dim >= 1 && dim <= vs::kNdMaxDim && metric == VS_METRIC_L2)
        return vs_bf_create_nd_u8(base_host, n_rows, dim, device, id_offset, out);
    return guarded([&]() -> int {
        if (!out || !base_host || n_rows <= 0) {
            set_error("vs_bf_create_nd_u8_metric: bad arguments");
            return VS_ERR_INVALID;
        }
        if (dim < 1) {
            set_error("vs_bf_create_nd_u8_metric: dim must be at least 1");
            return VS_ERR_INVALID;
        }
        if (dim > vs::kNdMaxDim) {
            set_error("vs_bf_create_nd_u8_metric: dim > 2048 is not compiled in");
            return VS_ERR_UNSUPPORTED;
        }
        if (metric != VS_METRIC_IP) {  // (VS_METRIC_L2 went above)
            set_error("vs_bf_create_nd_u8_metric: metric must be VS_METRIC_L2 or VS_METRIC_IP");
            return VS_ERR_INVALID;
        }
        if (n_rows + id_offset > std::numeric_limits<int32_t>::max()) {  // (before the float copy of the rows is made)
            set_error("ids must fit int32");
            return VS_ERR_UNSUPPORTED;
        }
        int rc = check_device(device);
        if (rc) return rc;
        std::vector<float> f((size_t)n_rows * dim);
        for (size_t i = 0; i < f.size(); ++i) f[i] = (float)base_host[i];
        return bf_create_impl(f.data(), n_rows, dim, VS_METRIC_IP, device, id_offset, out, true, base_host, true);
    });
}
static int bf_create_impl(const float* base_host, int64_t n_rows, int dim, int metric, int device, int64_t id_offset,
                          vs_index** out, bool any_dim, const uint8_t* rows_u8, bool force_general) {
    if (!out || !base_host || n_rows <= 0) {
        set_error(any_dim ? "vs_bf_create_nd: bad arguments" : "vs_bf_create: bad arguments");
        return VS_ERR_INVALID;
    }
    if (any_dim && dim < 1) {
        set_error("vs_bf_create_nd: dim must be at least 1");
        return VS_ERR_INVALID;
    }
    if (any_dim && dim > vs::kNdMaxDim) {
        set_error("vs_bf_create_nd: dim > 2048 is not compiled in");
        return VS_ERR_UNSUPPORTED;
    }
    if (!any_dim && dim != vs::kDim) {
        set_error("only dim == 128 is compiled in");
        return VS_ERR_UNSUPPORTED;
    }
    if (metric != VS_METRIC_L2 && metric != VS_METRIC_IP) {
        set_error("unknown metric");
        return VS_ERR_INVALID;
    }
    if (n_rows + id_offset > std::numeric_limits<int32_t>::max()) {
        set_error("ids must fit int32");
        return VS_ERR_UNSUPPORTED;
    }
    int rc = check_device(device);
    if (rc) return rc;
    HIPCHK(hipSetDevice(device));
    vs_index* h = new (std::nothrow) vs_index();
    if (!h) {
        set_error("out of host memory");
        return VS_ERR_NOMEM;
    }
    h->kind = 0;
    h->device = device;
    h->dim = dim;
    h->general = dim != vs::kDim || g_nd_force != 0 || force_general;
    h->dim_p = h->general ? vs::nd_dim_p(dim) : dim;
    // comparison toggle (VSEARCH_ND_ONE=0, read here): short calls on this general index keep the per-batch scan_nd_kernel
    // route instead of scan_one_nd_kernel
    if (const char* e = getenv("VSEARCH_ND_ONE")) h->nd_one = atoi(e) != 0;
    // ... and VSEARCH_ND_ONE_U8=0 the per-batch scan_nd_i8_kernel route for short calls on its byte rows
    if (const char* e = getenv("VSEARCH_ND_ONE_U8")) h->nd_one_u8 = atoi(e) != 0;
    // ... and VSEARCH_ND_WIDE_U8=0 the fp32 launches for wide k on an index with byte rows (topw_launch)
    if (const char* e = getenv("VSEARCH_ND_WIDE_U8")) h->nd_wide_u8 = atoi(e) != 0;
    h->metric = metric;
    h->n_rows = h->n_total = n_rows;
    h->id_offset = id_offset;
    if ((rc = upload_vectors(h, base_host, n_rows)) || (rc = alloc_scratch(h))) {
        vs_destroy(h);
        return rc;
    }
    if (h->general) {  // no seed sample; fp32 rows only, unless the rows came as uint8 (vs_bf_create_nd_u8)
        if (rows_u8) {
            h->nd_from_u8 = true;
            h->dim_b = vs::nd_dim_b(dim);
            if ((rc = build_nd_u8_copy(h, rows_u8, n_rows))) {
                vs_destroy(h);
                return rc;
            }
        }
        *out = h;
        return VS_OK;
    }
    if (metric == VS_METRIC_L2 && (rc = build_u8_copy(h, base_host, n_rows))) {
        vs_destroy(h);
        return rc;
    }
    if ((n_rows + vs::kTileRows - 1) / vs::kTileRows >= 2 * vs::kSeedWaves) {  // shards on which launches are seeded (bf_launch)
        auto sample = [&]() -> int {
            int r2;
            if ((r2 = h->d_seed_f32.alloc((size_t)vs::kSeedWaves * 2048)) || (r2 = h->d_seed_bnorm.alloc((size_t)vs::kSeedWaves * 16))) return r2;
            if (h->d_vecs_u8 && ((r2 = h->d_seed_u8.alloc((size_t)vs::kSeedWaves * 2048)) || (r2 = h->d_seed_rterm.alloc((size_t)vs::kSeedWaves * 16))))
                return r2;
            HIPCHK(vs::launch_seed_sample(h->d_vecs, h->d_norm, h->d_vecs_u8, h->d_rterm, n_rows, h->d_seed_f32, h->d_seed_bnorm,
                                          h->d_seed_u8, h->d_seed_rterm, nullptr));
            HIPCHK(hipDeviceSynchronize());
            return VS_OK;
        };
        if ((rc = sample())) {
            vs_destroy(h);
            return rc;
        }
    }
    *out = h;
    return VS_OK;
}

int vs_ivf_set_metric(vs_index* h, int metric) {
    if (refuse_general_bf(h, "vs_ivf_set_metric")) return VS_ERR_UNSUPPORTED;
    if (!h || h->kind != 1 || (metric != VS_METRIC_L2 && metric != VS_METRIC_IP)) {
        set_error("vs_ivf_set_metric: an IVF index and VS_METRIC_L2 or VS_METRIC_IP");
        return VS_ERR_INVALID;
    }
    if (metric == VS_METRIC_IP && refuse_general_ivf(h, "vs_ivf_set_metric(VS_METRIC_IP)")) return VS_ERR_UNSUPPORTED;
    h->metric = metric;  // (inner product: centroid scores, bounds, list scan and ranking on -q.v over the fp32 rows)
    return VS_OK;
}

int vs_set_precision(vs_index* h, int precision) {
    if (!h || precision < 0 || precision > 2) {
        set_error("vs_set_precision: 0 = auto, 1 = fp32, 2 = int8");
        return VS_ERR_INVALID;
    }
    if (precision == 2 && h->general && !h->nd_from_u8) return refuse_general(h, "vs_set_precision(2)");
    if (precision == 2 && h->general && !h->d_nd_u8) {
        set_error("vs_set_precision(2): max ||b||^2 >= 2^24 on this index: no batch could run on the byte rows");
        return VS_ERR_UNSUPPORTED;
    }
    if (precision == 2 && !h->general && !h->d_vecs_u8) {
        set_error("int8 path unavailable: the base is not integer valued in [0, 255] (or the index is not brute-force L2)");
        return VS_ERR_UNSUPPORTED;
    }
    h->precision = precision;
    return VS_OK;
}

int vs_bf_search_dev(vs_index* h, const float* queries_dev, int B, int k, int32_t* ids_dev, float* dists_dev,
                     int32_t* flags_dev, void* stream) {
    if (!h || h->kind != 0 || !queries_dev || !ids_dev || !dists_dev || B < 1 || B > vs::kMaxBatch || k < 1) {
        set_error("vs_bf_search_dev: bad arguments");
        return VS_ERR_INVALID;
    }
    int rc = set_device(h);
    if (rc) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    if ((rc = order_begin(h, st))) return rc;
    rc = bf_batch_dev(h, h->lane[0], queries_dev, B, k + 1, dists_dev, ids_dev, flags_dev ? flags_dev : h->d_flags, st);
    return rc ? rc : order_end(h, st);
}

int vs_bf_search_dev_multi(vs_index* h, const float* queries_dev, int n_batches, int B, int k, int32_t* ids_dev,
                           float* dists_dev, int32_t* flags_dev, void* stream) {
    if (!h || h->kind != 0 || !queries_dev || !ids_dev || !dists_dev || n_batches < 1 || B < 1 || B > vs::kMaxBatch || k < 1) {
        set_error("vs_bf_search_dev_multi: bad arguments");
        return VS_ERR_INVALID;
    }
    int rc = set_device(h);
    if (rc) return rc;
    if (!pick_kcap(k + 1)) {
        set_error("k too large for the compiled scan kernels (k <= 15)");
        return VS_ERR_UNSUPPORTED;
    }
    hipStream_t st = static_cast<hipStream_t>(stream);
    if ((rc = order_begin(h, st))) return rc;
    rc = bf_multi_dev(h, queries_dev, n_batches, B, k + 1, dists_dev, ids_dev, flags_dev, st);
    return rc ? rc : order_end(h, st);
}

int vs_bf_scores_dev(vs_index* h, const float* queries_dev, int B, float* scores_dev_, int64_t ld, void* stream) {
    if (!h || h->kind != 0 || !queries_dev || !scores_dev_ || B < 1 || B > vs::kMaxBatch || ld < h->n_rows) {
        set_error("vs_bf_scores_dev: bad arguments");
        return VS_ERR_INVALID;
    }
    int rc = set_device(h);
    if (rc) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    if ((rc = order_begin(h, st))) return rc;
    rc = scores_dev(h, h->d_vecs, h->d_norm, h->n_rows, queries_dev, B, scores_dev_, ld, st);
    return rc ? rc : order_end(h, st);
}

int vs_bf_search_topk_dev_multi(vs_index* h, const float* queries_dev, int n_batches, int B, int k, int32_t* ids_dev,
                                float* dists_dev, int32_t* flags_dev, void* stream) {
    if (!h || h->kind != 0 || !queries_dev || !ids_dev || !dists_dev || n_batches < 1 || B < 1 || B > vs::kMaxBatch || k < 1) {
        set_error("vs_bf_search_topk_dev_multi: bad arguments");
        return VS_ERR_INVALID;
    }
    if (k > vs::kTopkWideMax - 1) {
        set_error("vs_bf_search_topk_dev_multi: k > 128");
        return VS_ERR_UNSUPPORTED;
    }
    if (k + 1 <= kKcapMax) return vs_bf_search_dev_multi(h, queries_dev, n_batches, B, k, ids_dev, dists_dev, flags_dev, stream);
    int rc = set_device(h);
    if (rc) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    if ((rc = ensure_topw(h)) || (rc = order_begin(h, st))) return rc;
    const int k1 = k + 1;
    for (int b0 = 0; b0 < n_batches; b0 += kMaxMulti) {
        const int n = std::min(kMaxMulti, n_batches - b0);
        if ((rc = topw_launch(h, queries_dev + (size_t)b0 * B * h->dim, n, B, k1, dists_dev + (size_t)b0 * B * k1,
                              ids_dev + (size_t)b0 * B * k1, flags_dev ? flags_dev + (size_t)b0 * B : nullptr, st)))
            return rc;
    }
    return order_end(h, st);
}

// --------------------------------------------------------------------------------------------- IVF
int vs_ivf_list_owners(const int32_t* cluster_offsets, int nlist, int world, int32_t* owner_out) {
    if (!cluster_offsets || !owner_out || nlist <= 0 || world < 1) {
        set_error("vs_ivf_list_owners: bad arguments");
        return VS_ERR_INVALID;
    }
    std::vector<int> order(nlist);
    std::iota(order.begin(), order.end(), 0);
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) {
        return (cluster_offsets[a + 1] - cluster_offsets[a]) > (cluster_offsets[b + 1] - cluster_offsets[b]);
    });
    for (int i = 0; i < nlist; ++i) owner_out[order[i]] = i % world;
    return VS_OK;
}

int vs_ivf_shard_group(int world) {
    if (world < 1) return 0;
    return world > 1 ? std::min(kIvfGroupMax, 32 * std::min(world, kIvfShardMaxWorld)) : kIvfGroupDefault;
}

int vs_ivf_shard_slice(int n_batches, int world, int rank, int32_t* slice_batches, int32_t* first_batch, int32_t* own_batches) {
    if (n_batches < 1 || world < 1 || rank < 0 || rank >= world || !slice_batches || !first_batch || !own_batches) {
        set_error("vs_ivf_shard_slice: bad arguments");
        return VS_ERR_INVALID;
    }
    int sbb, b0, nbs;
    ivf_slice(n_batches, world, rank, sbb, b0, nbs);
    if (sbb > vs::kIvfWideBatches) {
        set_error("vs_ivf_shard_slice: more than 32 batches per slice (a launch group holds at most vs_ivf_shard_group(world) batches)");
        return VS_ERR_INVALID;
    }
    *slice_batches = sbb;
    *first_batch = b0;
    *own_batches = nbs;
    return VS_OK;
}

int64_t vs_ivf_shard_block_words(int slice_batches, int nprobe) { return ivf_block_words(slice_batches, nprobe); }

// the replicated heads of a sharded index (see vs_index::d_head_vecs): rows [offsets[c], offsets[c] + min(len, kIvfTauRows))
// of every list of the WHOLE index, fp32 packed + (when every head row is byte valued) the tiled byte copy
static int build_tau_heads(vs_index* h, const float* vectors, const int32_t* offsets, int nlist) {
    std::vector<int32_t> hoff((size_t)nlist + 1, 0), tdelta((size_t)nlist, 0);
    int64_t t = 0;
    for (int c = 0; c < nlist; ++c) {
        const int32_t len = std::min<int32_t>(offsets[c + 1] - offsets[c], vs::kIvfTauRows);
        hoff[c + 1] = hoff[c] + len;
        tdelta[c] = (int32_t)t - hoff[c];
        t += (len + 15) / 16 * 16;
    }
    const size_t nh = (size_t)hoff[nlist], nt = (size_t)t + 64;
    std::vector<float> hv((nh + vs::kScanPadRows) * vs::kDim, 0.f);
    for (int c = 0; c < nlist; ++c)
        if (hoff[c + 1] > hoff[c])
            std::memcpy(&hv[(size_t)hoff[c] * vs::kDim], vectors + (size_t)offsets[c] * vs::kDim, (size_t)(hoff[c + 1] - hoff[c]) * vs::kDim * sizeof(float));
    int rc;
    if ((rc = h->d_head_vecs.alloc(hv.size())) || (rc = h->d_head_norm.alloc(nh + 64)) || (rc = h->d_head_off.alloc(hoff.size())) ||
        (rc = h->d_head_tdelta.alloc(tdelta.size())))
        return rc;
    HIPCHK(hipMemcpy(h->d_head_vecs, hv.data(), hv.size() * sizeof(float), hipMemcpyHostToDevice));
    HIPCHK(hipMemset(h->d_head_norm, 0, (nh + 64) * sizeof(float)));
    HIPCHK(hipMemcpy(h->d_head_off, hoff.data(), hoff.size() * 4, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(h->d_head_tdelta, tdelta.data(), tdelta.size() * 4, hipMemcpyHostToDevice));
    if (nh > 0) HIPCHK(vs::launch_row_sqnorm(h->d_head_vecs, (int64_t)nh, vs::kDim, h->d_head_norm, nullptr));
    HIPCHK(hipDeviceSynchronize());
    if (h->metric != VS_METRIC_L2) return VS_OK;
    std::vector<int8_t> tb(nt * vs::kDim, 0);
    std::vector<int32_t> rterm_t(nt, 0);
    for (int c = 0; c < nlist; ++c)
        for (int32_t j = 0; j < hoff[c + 1] - hoff[c]; ++j) {
            const float* src = &hv[((size_t)hoff[c] + j) * vs::kDim];
            const size_t R = (size_t)hoff[c] + tdelta[c] + j;
            int8_t* tile = &tb[(R >> 4) * 16 * vs::kDim + (R & 15) * 16];
            int32_t n2 = 0, sb = 0;
            for (int e = 0; e < vs::kDim; ++e) {
                const float x = src[e];
                const int xi = (int)x;
                if (!((float)xi == x) || xi < 0 || xi > 255) return VS_OK;  // not byte valued: bounds on the fp32 heads
                tile[(e >> 6) * 1024 + ((e >> 4) & 3) * 256 + (e & 15)] = (int8_t)(xi - 128);
                n2 += xi * xi;
                sb += xi - 128;
            }
            rterm_t[R] = n2 - 256 * sb;
        }
    if ((rc = h->d_head_t8.alloc(tb.size())) || (rc = h->d_head_rterm_t.alloc(nt))) return rc;
    HIPCHK(hipMemcpy(h->d_head_t8, tb.data(), tb.size(), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(h->d_head_rterm_t, rterm_t.data(), nt * 4, hipMemcpyHostToDevice));
    return VS_OK;
}

// rows_u8: the rows as uint8 instead of `vectors` (vs_ivf_create_nd_u8; unsharded): converted to float once the
// arguments are checked, and kept as bytes beside the fp32 rows when the index is a general one
static int ivf_create_impl(const float* vectors, int64_t n_rows, int dim, const float* centroids, int nlist,
                           const int32_t* offsets, const int32_t* r2o, int device, int rank, int world,
                           vs_index** out, const uint8_t* rows_u8 = nullptr) {
    const std::string who = rows_u8 ? "vs_ivf_create_nd_u8" : "vs_ivf_create";
    if (!out || (!vectors && !rows_u8) || !centroids || !offsets || n_rows <= 0 || nlist <= 0 || world < 1 || rank < 0 || rank >= world) {
        set_error(who + ": bad arguments");
        return VS_ERR_INVALID;
    }
    if (dim < 1) {
        set_error(who + ": dim must be at least 1");
        return VS_ERR_INVALID;
    }
    if (dim > vs::kNdMaxDim) {
        set_error(who + ": dim > 2048 is not compiled in");
        return VS_ERR_UNSUPPORTED;
    }
    if (dim != vs::kDim && world > 1) {
        char msg[160];
        snprintf(msg, sizeof(msg), "vs_ivf_create: a general-dimension IVF index (dim = %d) cannot be sharded; only dim == 128 can", dim);
        set_error(msg);
        return VS_ERR_UNSUPPORTED;
    }
    if (offsets[0] != 0 || offsets[nlist] != n_rows) {
        set_error("cluster_offsets do not cover the vectors");
        return VS_ERR_INVALID;
    }
    for (int c = 0; c < nlist; ++c)
        if (offsets[c + 1] < offsets[c]) {
            set_error("cluster_offsets not monotone");
            return VS_ERR_INVALID;
        }
    int rc = check_device(device);
    if (rc) return rc;
    HIPCHK(hipSetDevice(device));
    std::vector<float> rows_f32;
    if (rows_u8) {  // (exact: every byte is a float)
        rows_f32.resize((size_t)n_rows * dim);
        for (size_t i = 0; i < rows_f32.size(); ++i) rows_f32[i] = (float)rows_u8[i];
        vectors = rows_f32.data();
    }
    vs_index* h = new (std::nothrow) vs_index();
    if (!h) {
        set_error("out of host memory");
        return VS_ERR_NOMEM;
    }
    h->kind = 1;
    h->device = device;
    h->dim = dim;
    // comparison toggle (VSEARCH_IVF_ND_FORCE=1, read here): an unsharded 128-d index is built as a general IVF index as
    // well, so that the list-major general scan can be set against the specialised pipeline on the same data
    const char* nd_force = getenv("VSEARCH_IVF_ND_FORCE");
    h->general = dim != vs::kDim || (world == 1 && nd_force && atoi(nd_force) != 0);
    h->dim_p = h->general ? vs::nd_dim_p(dim) : dim;
    // comparison toggle (VSEARCH_IVF_ONE=0, read here): short calls on this general index keep the group route
    if (const char* e = getenv("VSEARCH_IVF_ONE")) h->ivf_one = atoi(e) != 0;
    if (const char* e = getenv("VSEARCH_IVF_ONE_U8")) h->ivf_one_u8 = atoi(e) == 2 ? 2 : atoi(e) != 0;
    h->metric = VS_METRIC_L2;
    h->n_total = n_rows;
    h->nlist = nlist;
    h->rank = rank;
    h->world = world;
    h->h_offsets_global.assign(offsets, offsets + nlist + 1);
    h->avg_cluster_size = (double)n_rows / nlist;

    // Ownership: lists sorted by length (desc), dealt round-robin -> balanced bytes and probe hits
    // (SURVEY.md 8e).  Only owned lists are made resident; the others become empty ranges.
    std::vector<int32_t> owner(nlist);
    vs_ivf_list_owners(offsets, nlist, world, owner.data());
    std::vector<uint8_t> owned(nlist, 0);
    for (int c = 0; c < nlist; ++c) owned[c] = owner[c] == rank;
    std::vector<int32_t> loc_off(nlist + 1, 0);
    for (int c = 0; c < nlist; ++c) loc_off[c + 1] = loc_off[c] + (owned[c] ? offsets[c + 1] - offsets[c] : 0);
    const int64_t n_local = loc_off[nlist];
    h->n_rows = n_local;
    std::vector<int32_t> loc_r2o((size_t)std::max<int64_t>(n_local, 1));
    const float* up = vectors;
    std::vector<float> packed;
    if (world > 1) {
        packed.resize((size_t)std::max<int64_t>(n_local, 1) * dim);
        for (int c = 0; c < nlist; ++c)
            if (owned[c] && offsets[c + 1] > offsets[c])
                std::memcpy(&packed[(size_t)loc_off[c] * dim], vectors + (size_t)offsets[c] * dim,
                            (size_t)(offsets[c + 1] - offsets[c]) * dim * sizeof(float));
        up = packed.data();
    }
    for (int c = 0; c < nlist; ++c)
        if (owned[c])
            for (int32_t r = offsets[c]; r < offsets[c + 1]; ++r)
                loc_r2o[(size_t)loc_off[c] + (r - offsets[c])] = r2o ? r2o[r] : r;

    auto fail = [&](int code) {
        vs_destroy(h);
        return code;
    };
    if ((rc = upload_vectors(h, up, n_local))) return fail(rc);
    // exact int8 copy of the (reordered, local) rows when they are byte valued: the list scan then moves 4x fewer bytes
    std::vector<int8_t> host_bytes;
    std::vector<int32_t> host_rterm;
    if (!h->general && h->metric == VS_METRIC_L2 && n_local > 0 && (rc = build_u8_copy(h, up, n_local, &host_bytes, &host_rterm)))
        return fail(rc);
    // centroids [nlist + 64][dim_p]: zero padded like the rows on a general index (the coarse scores are a brute-force scan
    // of this table)
    const size_t cld = (size_t)h->dim_p, cents_total = ((size_t)nlist + vs::kScanPadRows) * cld;
    if ((rc = h->d_centroids.alloc(cents_total))) return fail(rc);
    if (hipMemset(h->d_centroids, 0, cents_total * sizeof(float)) != hipSuccess) return fail(VS_ERR_DEVICE);
    if ((rc = h->d_cnorm.alloc((size_t)nlist + 64))) return fail(rc);
    if ((rc = h->d_offsets.alloc((size_t)nlist + 1))) return fail(rc);
    if ((rc = h->d_r2o.alloc((size_t)std::max<int64_t>(n_local, 1)))) return fail(rc);
    hipError_t e;
    if ((e = hipMemset(h->d_cnorm, 0, ((size_t)nlist + 64) * sizeof(float))) != hipSuccess ||
        (e = hipMemcpy2D(h->d_centroids, cld * sizeof(float), centroids, (size_t)dim * sizeof(float), (size_t)dim * sizeof(float), (size_t)nlist,
                         hipMemcpyHostToDevice)) != hipSuccess ||
        (e = hipMemcpy(h->d_offsets, loc_off.data(), ((size_t)nlist + 1) * sizeof(int32_t), hipMemcpyHostToDevice)) != hipSuccess ||
        (e = hipMemcpy(h->d_r2o, loc_r2o.data(), (size_t)std::max<int64_t>(n_local, 1) * sizeof(int32_t), hipMemcpyHostToDevice)) != hipSuccess ||
        (e = vs::launch_row_sqnorm_ld(h->d_centroids, nlist, dim, (int64_t)cld, h->d_cnorm, nullptr)) != hipSuccess ||
        (e = hipDeviceSynchronize()) != hipSuccess) {
        set_error(std::string("ivf upload: ") + hipGetErrorString(e));
        return fail(VS_ERR_DEVICE);
    }
    if (h->general) {
        // no chunk table, no tiled copy, no heads: launch groups of 32 batches on the caller's stream (ivf_group_nd_dev),
        // their scratch and the host staging now rather than inside the first search
        h->ivf_gb = vs::kIvfWideBatches;
        h->ivf_lanes = 1;
        h->ivf_nsb = 1;
        for (int c = 0; c < nlist; ++c) h->max_list = std::max(h->max_list, loc_off[c + 1] - loc_off[c]);
        if (rows_u8) {  // (unsharded: the local rows are the caller's) the byte copy, unless max ||b||^2 >= 2^24, and the pair counters
            h->nd_from_u8 = true;
            h->dim_b = vs::nd_dim_b(dim);
            if ((rc = build_nd_u8_copy(h, rows_u8, n_local)) || (rc = h->d_nd_stats.alloc(2))) return fail(rc);
            if (hipMemset(h->d_nd_stats, 0, 2 * sizeof(unsigned long long)) != hipSuccess) return fail(VS_ERR_DEVICE);
        }
        if ((rc = alloc_scratch(h)) || (rc = ensure_ivf_nd(h)) || (rc = ensure_wide_streams(h)) || (rc = ensure_ivf_host(h))) return fail(rc);
        *out = h;
        return VS_OK;
    }
    {
        // (list, 1024-row chunk) work items of the list-major scan, resident lists only
        std::vector<int32_t> cl, cr0, crn;
        int32_t mx = 0;
        for (int c = 0; c < nlist; ++c) {
            const int32_t n = loc_off[c + 1] - loc_off[c];
            mx = std::max(mx, n);
            for (int32_t r = 0; r < n; r += 1024) {
                cl.push_back(c);
                cr0.push_back(loc_off[c] + r);
                crn.push_back(std::min<int32_t>(1024, n - r));
            }
        }
        h->n_chunks = (int)cl.size();
        h->max_list = mx;
        if (h->n_chunks > 0 && h->d_vecs_u8) {
            // the tiled, padded copy for the wide scan (see vs_index::d_vecs_t8)
            std::vector<int32_t> toff((size_t)nlist + 1), tdelta((size_t)nlist), ctr0;
            int64_t t = 0;
            for (int c = 0; c < nlist; ++c) {
                toff[c] = (int32_t)t;
                tdelta[c] = (int32_t)t - loc_off[c];
                t += ((int64_t)(loc_off[c + 1] - loc_off[c]) + vs::kIvfWideUnit - 1) / vs::kIvfWideUnit * vs::kIvfWideUnit;
            }
            toff[nlist] = (int32_t)t;
            if (t + 64 >= (1ll << 31)) {  // (padded rows are int32 like rows)
                set_error("ivf: too many rows for one shard");
                return fail(VS_ERR_UNSUPPORTED);
            }
            const size_t n_t = (size_t)t + 64;
            std::vector<int8_t> tb(n_t * vs::kDim, 0);
            std::vector<int32_t> nrh_t(n_t, 0), rterm_t(n_t, 0), r2o_t(n_t, -1);
            for (int c = 0; c < nlist; ++c)
                for (int32_t j = 0; j < loc_off[c + 1] - loc_off[c]; ++j) {
                    const size_t R = (size_t)toff[c] + j, row = (size_t)loc_off[c] + j;
                    const int8_t* src = &host_bytes[row * vs::kDim];
                    int8_t* tile = &tb[(R >> 4) * 16 * vs::kDim + (R & 15) * 16];
                    for (int ch = 0; ch < 8; ++ch) std::memcpy(tile + (ch >> 2) * 1024 + (ch & 3) * 256, src + 16 * ch, 16);
                    rterm_t[R] = host_rterm[row];
                    nrh_t[R] = -(host_rterm[row] >> 1);
                    r2o_t[R] = loc_r2o[row];
                }
            for (size_t i = 0; i < cl.size(); ++i) ctr0.push_back(cr0[i] + tdelta[cl[i]]);
            if ((rc = h->d_vecs_t8.alloc(tb.size())) || (rc = h->d_nrh_t.alloc(n_t)) || (rc = h->d_rterm_t.alloc(n_t)) ||
                (rc = h->d_r2o_t.alloc(n_t)) || (rc = h->d_tdelta.alloc(tdelta.size())) || (rc = h->d_chunk_trow0.alloc(ctr0.size())))
                return fail(rc);
            if ((e = hipMemcpy(h->d_vecs_t8, tb.data(), tb.size(), hipMemcpyHostToDevice)) != hipSuccess ||
                (e = hipMemcpy(h->d_nrh_t, nrh_t.data(), n_t * 4, hipMemcpyHostToDevice)) != hipSuccess ||
                (e = hipMemcpy(h->d_rterm_t, rterm_t.data(), n_t * 4, hipMemcpyHostToDevice)) != hipSuccess ||
                (e = hipMemcpy(h->d_r2o_t, r2o_t.data(), n_t * 4, hipMemcpyHostToDevice)) != hipSuccess ||
                (e = hipMemcpy(h->d_tdelta, tdelta.data(), tdelta.size() * 4, hipMemcpyHostToDevice)) != hipSuccess ||
                (e = hipMemcpy(h->d_chunk_trow0, ctr0.data(), ctr0.size() * 4, hipMemcpyHostToDevice)) != hipSuccess) {
                set_error(std::string("ivf tiled copy: ") + hipGetErrorString(e));
                return fail(VS_ERR_DEVICE);
            }
        }
        if (h->n_chunks > 0) {
            if ((rc = h->d_chunk_list.alloc(cl.size()))) return fail(rc);
            if ((rc = h->d_chunk_row0.alloc(cl.size()))) return fail(rc);
            if ((rc = h->d_chunk_rows.alloc(cl.size()))) return fail(rc);
            h->n_units_max = 0;
            for (int32_t r : crn) h->n_units_max += (r + 31) >> 5;
            if ((e = hipMemcpy(h->d_chunk_list, cl.data(), cl.size() * 4, hipMemcpyHostToDevice)) != hipSuccess ||
                (e = hipMemcpy(h->d_chunk_row0, cr0.data(), cl.size() * 4, hipMemcpyHostToDevice)) != hipSuccess ||
                (e = hipMemcpy(h->d_chunk_rows, crn.data(), cl.size() * 4, hipMemcpyHostToDevice)) != hipSuccess) {
                set_error(std::string("ivf chunk table: ") + hipGetErrorString(e));
                return fail(VS_ERR_DEVICE);
            }
        }
    }
    if (world > 1 && (rc = build_tau_heads(h, vectors, offsets, nlist))) return fail(rc);
    if ((rc = alloc_scratch(h))) return fail(rc);
    // launch groups: an unsharded index takes VSEARCH_IVF_GROUP batches per group (super-batches of 32); a sharded one a
    // slice of up to 32 batches per rank (ivf_shard_front / ivf_shard_back)
    h->ivf_gb = world > 1 ? std::min(kIvfGroupMax, 32 * std::min(world, kIvfShardMaxWorld)) : ivf_group_batches();
    h->ivf_lanes = ivf_wide_lanes();
    h->ivf_nsb = world > 1 ? std::max(h->ivf_gb / 32, std::min(world, kIvfShardMaxWorld)) : h->ivf_gb / 32;
    if (h->nlist <= vs::kIvfFastNlist && h->n_chunks > 0) {
        // the wide pipeline's scratch (two lanes), streams and host staging now rather than inside the first search:
        // index load is outside every timed region, a first call that allocates 200 MB is not (the reference's harness
        // times every searchBatch call, main_ivf.cpp:157-163)
        if ((rc = ensure_ivf_wide(h, 0)) || (rc = ensure_ivf_wide(h, 1)) || (rc = ensure_wide_streams(h)) || (rc = ensure_ivf_host(h)))
            return fail(rc);
    }
    *out = h;
    return VS_OK;
}

// GPU index builder: Lloyd k-means on the scan kernel (assignment = the brute-force MFMA scan with the
// centroids as "queries", 32 per pass) + deterministic fixed-point update.
//
// The argument checks and the one host pass of both builders, before any device work: every value finite, max |x| inside
// the range of the fixed-point cluster sums (kmeans_accum_kernel: 64-bit sums of rint(x * 2^20) wrap once a sum leaves
// +-2^63), and the per-feature variance of sklearn's stopping rule: sum of squared centre shifts <= tol * mean
// per-feature variance.  dim_lo .. dim_hi: what the entry point compiles (below dim_lo, for the general builder: invalid).
static int ivf_build_checks(const char* who, const float* base_host, int64_t n_rows, int dim, int dim_lo, int dim_hi, int nlist,
                            int max_iter, double tol, const float* centroids_out, const int32_t* assign_out, double& tol_abs) {
    if (!base_host || !centroids_out || !assign_out || n_rows <= 0 || nlist <= 0 || nlist > n_rows || max_iter < 0) {
        set_error(std::string(who) + ": bad arguments");
        return VS_ERR_INVALID;
    }
    if (dim_lo != dim_hi && dim < dim_lo) {
        set_error(std::string(who) + ": dim must be at least 1");
        return VS_ERR_INVALID;
    }
    if (dim < dim_lo || dim > dim_hi) {
        set_error(dim_lo == dim_hi ? std::string("only dim == 128 is compiled in")
                                   : std::string(who) + ": dim " + std::to_string(dim) + " is above the largest supported, 2048");
        return VS_ERR_UNSUPPORTED;
    }
    tol_abs = 0.0;
    std::vector<double> sum(dim, 0.0), sq(dim, 0.0);
    double amax = 0.0;
    bool finite = true;
    for (int64_t i = 0; i < n_rows; ++i)
        for (int t = 0; t < dim; ++t) {
            const double v = base_host[i * dim + t];
            const double a = std::fabs(v);
            if (!(a <= 3.4028234663852886e38)) finite = false;  // inf or NaN
            else if (a > amax) amax = a;
            sum[t] += v;
            sq[t] += v * v;
        }
    if (!finite) {
        set_error(std::string(who) + ": the base holds a NaN or an infinity");
        return VS_ERR_INVALID;
    }
    // |sum of n quantised values| <= n * (max|x| * 2^20 + 1/2) must stay below 2^63
    if ((double)n_rows * (amax + 0x1p-21) >= 0x1p43) {
        set_error(std::string(who) + ": n_rows * max|x| = " + std::to_string((double)n_rows * amax) +
                  " is outside the fixed-point range of the k-means update (must be < 2^43)");
        return VS_ERR_INVALID;
    }
    if (tol > 0) {
        double mv = 0;
        for (int t = 0; t < dim; ++t) {
            const double m = sum[t] / n_rows;
            mv += sq[t] / n_rows - m * m;
        }
        tol_abs = tol * mv / dim;
    }
    return VS_OK;
}

// What both builders do once the rows [n_rows][ld], their norms and the zeroed centroids [nlist_pad][dim] are on the device:
// the seeding stream and the initial centres, the Lloyd loop with its stopping rule, the final assignment, the outputs.
// The launches are the caller's: kpp_step(c, u, n_blocks, d_bsum) = one D^2 step, assign_pass() = best_d / best_i of every
// row against the current centroids, update() = one fixed-point update with the shifts in d_shift.
static thread_local double g_build_assign_ms = 0.0;  // device time of the calling thread's last assignment pass
double vs_ivf_build_last_assign_ms(void) { return g_build_assign_ms; }

extern "C++" {
template <class KppStep, class AssignPass, class Update>
static int ivf_build_run(const float* base_host, int64_t n_rows, int dim, int64_t ld, int nlist, int nlist_pad, int max_iter,
                         double tol_abs, uint64_t seed, const float* d_x, float* d_cents, float* d_best_d, const int32_t* d_best_i,
                         const double* d_shift, KppStep kpp_step, AssignPass assign_pass, Update update, float* centroids_out,
                         int32_t* assign_out, int* iters_done) {
    int rc;
    // initial centroids: k-means++ (D^2 sampling), sklearn's default for the reference's KMeans(random_state=42, n_init=1),
    // create_ivf_model_reordered.py:97-103.  sklearn's RNG stream and its greedy multi-trial variant are not
    // reproduced (VSEARCH_KMEANS_INIT=random: nlist distinct random rows instead).
    {
        uint64_t st = seed * 0x9E3779B97F4A7C15ull + 0x1234567ull;
        auto next = [&]() {
            uint64_t z = (st += 0x9E3779B97F4A7C15ull);
            z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
            z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
            return z ^ (z >> 31);
        };
        const char* init_env = getenv("VSEARCH_KMEANS_INIT");
        const bool random_init = init_env && std::string(init_env) == "random";
        HIPCHK(hipMemset(d_cents, 0, (size_t)nlist_pad * dim * sizeof(float)));
        if (random_init) {
            std::vector<float> init((size_t)nlist_pad * dim, 0.f);
            std::vector<bool> used((size_t)n_rows, false);
            for (int c = 0; c < nlist; ++c) {
                int64_t r;
                do r = (int64_t)(next() % (uint64_t)n_rows); while (used[(size_t)r]);
                used[(size_t)r] = true;
                std::memcpy(&init[(size_t)c * dim], base_host + r * dim, (size_t)dim * sizeof(float));
            }
            HIPCHK(hipMemcpy(d_cents, init.data(), init.size() * sizeof(float), hipMemcpyHostToDevice));
        } else {
            const int n_blocks = (int)((n_rows + vs::kKppBlockRows - 1) / vs::kKppBlockRows);
            vs::DevBuf<double> d_bsum;
            if ((rc = d_bsum.alloc((size_t)n_blocks))) return rc;
            const int64_t first = (int64_t)(next() % (uint64_t)n_rows);
            hipError_t e = hipMemcpy(d_cents, d_x + first * ld, (size_t)dim * sizeof(float), hipMemcpyDeviceToDevice);
            // d_best_d doubles as the running min squared distance (+inf to start with)
            if (e == hipSuccess) e = hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(d_best_d), 0x7f800000, (size_t)n_rows, nullptr);
            for (int c = 1; c < nlist && e == hipSuccess; ++c) {
                const double u = (double)(next() >> 11) * (1.0 / 9007199254740992.0);  // [0, 1)
                e = kpp_step(c, u, n_blocks, d_bsum.get());
            }
            if (e == hipSuccess) e = hipDeviceSynchronize();
            HIPCHK(e);
        }
    }
    int it = 0;
    std::vector<double> shift((size_t)nlist);
    for (; it < max_iter; ++it) {
        HIPCHK(assign_pass());
        HIPCHK(update());
        HIPCHK(hipMemcpy(shift.data(), d_shift, (size_t)nlist * sizeof(double), hipMemcpyDeviceToHost));
        double total = 0;
        for (double v : shift) total += v;
        if (total <= tol_abs) {
            ++it;
            break;
        }
    }
    vs::Event ev0, ev1;  // the last pass is timed for vs_ivf_build_last_assign_ms
    if ((rc = ev0.create(true)) || (rc = ev1.create(true))) return rc;
    HIPCHK(hipEventRecord(ev0, nullptr));
    HIPCHK(assign_pass());  // labels consistent with the final centroids
    HIPCHK(hipEventRecord(ev1, nullptr));
    HIPCHK(hipMemcpy(assign_out, d_best_i, (size_t)n_rows * sizeof(int32_t), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(centroids_out, d_cents, (size_t)nlist * dim * sizeof(float), hipMemcpyDeviceToHost));
    float ms = 0.f;
    HIPCHK(hipEventElapsedTime(&ms, ev0, ev1));
    g_build_assign_ms = (double)ms;
    if (iters_done) *iters_done = it;
    return VS_OK;
}

// best_d / best_i of one assignment pass: +inf / -1, then the launch for the nlist / 32 full batches of centroids and the
// launch for the remainder (scan(p, grid) = the kModeAssign launch of the builder's scan kernel)
template <class Scan>
static hipError_t ivf_assign_launches(vs::ScanParams p, const float* d_cents, int dim, int nlist, int64_t n_rows, int grid, Scan scan) {
    hipError_t e = hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(p.best_d), 0x7f800000, (size_t)n_rows, nullptr);
    if (e != hipSuccess) return e;
    e = hipMemsetAsync(p.best_i, 0xff, (size_t)n_rows * sizeof(int32_t), nullptr);
    if (e != hipSuccess) return e;
    p.metric = 0;
    p.row_begin = 0;
    p.row_end = n_rows;
    p.q_batch_stride = (int64_t)32 * dim;
    const int full = nlist / 32, rem = nlist % 32;
    if (full) {
        p.q = d_cents;
        p.n_batches = full;
        p.nq_valid = 32;
        p.assign_base = 0;
        e = scan(p, grid, 0);
        if (e != hipSuccess) return e;
    }
    if (rem) {
        p.q = d_cents + (size_t)full * 32 * dim;
        p.n_batches = 1;
        p.nq_valid = rem;
        p.assign_base = full * 32;
        e = scan(p, grid, full);
    }
    return e;
}
}  // extern "C++"

static int ivf_build_impl(const float* base_host, int64_t n_rows, int dim, int nlist, int max_iter, double tol, uint64_t seed,
                          int device, float* centroids_out, int32_t* assign_out, int* iters_done);
int vs_ivf_build(const float* base_host, int64_t n_rows, int dim, int nlist, int max_iter, double tol, uint64_t seed,
                 int device, float* centroids_out, int32_t* assign_out, int* iters_done) {
    return guarded([&]() -> int {
        return ivf_build_impl(base_host, n_rows, dim, nlist, max_iter, tol, seed, device, centroids_out, assign_out, iters_done);
    });
}
static int ivf_build_impl(const float* base_host, int64_t n_rows, int dim, int nlist, int max_iter, double tol, uint64_t seed,
                          int device, float* centroids_out, int32_t* assign_out, int* iters_done) {
    double tol_abs = 0.0;
    int rc = ivf_build_checks("vs_ivf_build", base_host, n_rows, dim, vs::kDim, vs::kDim, nlist, max_iter, tol, centroids_out, assign_out,
                              tol_abs);
    if (rc) return rc;
    if ((rc = check_device(device))) return rc;
    HIPCHK(hipSetDevice(device));
    hipDeviceProp_t prop;
    HIPCHK(hipGetDeviceProperties(&prop, device));
    const int num_cus = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    vs::DevBuf<float> d_x, d_norm, d_cents, d_best_d;
    vs::DevBuf<int32_t> d_best_i, d_counts;
    vs::DevBuf<unsigned long long> d_acc;
    vs::DevBuf<double> d_shift;
    const int nlist_pad = (nlist + 31) & ~31;
    if ((rc = d_x.alloc(((size_t)n_rows + vs::kScanPadRows) * dim))) return rc;
    HIPCHK(hipMemset(d_x + (size_t)n_rows * dim, 0, (size_t)vs::kScanPadRows * dim * sizeof(float)));
    if ((rc = d_norm.alloc((size_t)n_rows + 64)) || (rc = d_cents.alloc((size_t)nlist_pad * dim)) || (rc = d_best_d.alloc((size_t)n_rows)) ||
        (rc = d_best_i.alloc((size_t)n_rows)) || (rc = d_counts.alloc((size_t)nlist)) || (rc = d_acc.alloc((size_t)nlist * dim)) ||
        (rc = d_shift.alloc((size_t)nlist)))
        return rc;
    HIPCHK(hipMemcpy(d_x, base_host, (size_t)n_rows * dim * sizeof(float), hipMemcpyHostToDevice));
    HIPCHK(hipMemset(d_norm, 0, ((size_t)n_rows + 64) * sizeof(float)));
    HIPCHK(vs::launch_row_sqnorm(d_x, n_rows, dim, d_norm, nullptr));
    int grid, tp;
    scan_geometry(n_rows, num_cus, grid, tp);
    vs::ScanParams p{};
    p.base = d_x;
    p.bnorm = d_norm;
    p.tiles_per_wg = tp;
    p.best_d = d_best_d;
    p.best_i = d_best_i;
    return ivf_build_run(
        base_host, n_rows, dim, dim, nlist, nlist_pad, max_iter, tol_abs, seed, d_x, d_cents, d_best_d, d_best_i, d_shift,
        [&](int c, double u, int n_blocks, double* d_bsum) {
            return vs::launch_kpp_step(d_x, d_norm, n_rows, d_cents, c, d_best_d, d_bsum, n_blocks, u, nullptr);
        },
        [&]() {
            return ivf_assign_launches(p, d_cents, dim, nlist, n_rows, grid, [](const vs::ScanParams& sp, int g, int) {
                return vs::launch_scan(sp, g, 8, 2, vs::kModeAssign, nullptr);
            });
        },
        [&]() { return vs::launch_kmeans_update(d_x, d_best_i, n_rows, nlist, d_cents, d_acc, d_counts, d_shift, nullptr); },
        centroids_out, assign_out, iters_done);
}

// comparison toggle (VSEARCH_BUILD_ND_FORCE=1, read at every call of the _nd builders): the general builder at dim 128 too
static bool build_nd_forced() {
    const char* e = getenv("VSEARCH_BUILD_ND_FORCE");
    return e && atoi(e) != 0;
}

// The builder at any dimension 1 <= dim <= 2048 (vsearch.h at vs_ivf_build_nd): the same contract on the layout of a general
// index -- rows [n_rows + kScanPadRows][dim_p] zero padded, centroids [nlist_pad][dim] unpadded (what nd_prep_kernel reads),
// assignment on scan_nd_kernel's kModeAssign, so that a distance is the brute-force general scan's to the bit.
static int ivf_build_nd_impl(const float* base_host, int64_t n_rows, int dim, int nlist, int max_iter, double tol, uint64_t seed,
                             int device, float* centroids_out, int32_t* assign_out, int* iters_done) {
    // dim 128 is vs_ivf_build's, checks included (the same ones in the same order)
    if (dim == vs::kDim && !build_nd_forced())
        return ivf_build_impl(base_host, n_rows, dim, nlist, max_iter, tol, seed, device, centroids_out, assign_out, iters_done);
    double tol_abs = 0.0;
    int rc = ivf_build_checks("vs_ivf_build_nd", base_host, n_rows, dim, 1, vs::kNdMaxDim, nlist, max_iter, tol, centroids_out,
                              assign_out, tol_abs);
    if (rc) return rc;
    if ((rc = check_device(device))) return rc;
    HIPCHK(hipSetDevice(device));
    hipDeviceProp_t prop;
    HIPCHK(hipGetDeviceProperties(&prop, device));
    const int num_cus = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    vs::DevBuf<float> d_x, d_norm, d_cents, d_best_d, d_qfrag, d_qnorm;
    vs::DevBuf<int32_t> d_best_i, d_counts;
    vs::DevBuf<unsigned long long> d_acc;
    vs::DevBuf<double> d_shift;
    const int nlist_pad = (nlist + 31) & ~31, n_batches = nlist_pad / 32;
    const int dim_p = vs::nd_dim_p(dim);
    const int64_t ld = dim_p;
    const size_t x_floats = ((size_t)n_rows + vs::kScanPadRows) * (size_t)ld;
    if ((rc = d_x.alloc(x_floats)) || (rc = d_norm.alloc((size_t)n_rows + 64)) || (rc = d_cents.alloc((size_t)nlist_pad * dim)) ||
        (rc = d_best_d.alloc((size_t)n_rows)) || (rc = d_best_i.alloc((size_t)n_rows)) || (rc = d_counts.alloc((size_t)nlist)) ||
        (rc = d_acc.alloc((size_t)nlist * dim)) || (rc = d_shift.alloc((size_t)nlist)) ||
        (rc = d_qfrag.alloc((size_t)n_batches * dim_p * 32)) || (rc = d_qnorm.alloc((size_t)n_batches * vs::kMaxBatch)))
        return rc;
    // zero filled: the padding of a row and the spare rows add exact zeros to every chain (scan blocks are read unclamped)
    HIPCHK(hipMemset(d_x, 0, x_floats * sizeof(float)));
    HIPCHK(hipMemcpy2D(d_x, (size_t)ld * sizeof(float), base_host, (size_t)dim * sizeof(float), (size_t)dim * sizeof(float), (size_t)n_rows,
                       hipMemcpyHostToDevice));
    HIPCHK(hipMemset(d_norm, 0, ((size_t)n_rows + 64) * sizeof(float)));
    HIPCHK(vs::launch_row_sqnorm_ld(d_x, n_rows, dim, ld, d_norm, nullptr));
    int grid, tp;
    scan_geometry(n_rows, num_cus, grid, tp);
    vs::ScanParams p{};
    p.base = d_x;
    p.bnorm = d_norm;
    p.tiles_per_wg = tp;
    p.best_d = d_best_d;
    p.best_i = d_best_i;
    return ivf_build_run(
        base_host, n_rows, dim, ld, nlist, nlist_pad, max_iter, tol_abs, seed, d_x, d_cents, d_best_d, d_best_i, d_shift,
        [&](int c, double u, int n_blocks, double* d_bsum) {
            return vs::launch_kpp_step_nd(d_x, ld, d_norm, n_rows, dim, d_cents, c, d_best_d, d_bsum, n_blocks, u, nullptr);
        },
        [&]() {
            return ivf_assign_launches(p, d_cents, dim, nlist, n_rows, grid, [&](const vs::ScanParams& sp, int g, int batch0) {
                vs::ScanNdParams np{};
                np.s = sp;
                np.dim = dim;
                np.dim_p = dim_p;
                np.qfrag = d_qfrag + (size_t)batch0 * dim_p * 32;  // the remainder's batch has its own fragments and norms
                np.qnorm = d_qnorm + (size_t)batch0 * vs::kMaxBatch;
                return vs::launch_scan_nd(np, g, 8, 2, vs::kModeAssign, nullptr);
            });
        },
        [&]() {
            return vs::launch_kmeans_update_nd(d_x, ld, dim, d_best_i, n_rows, nlist, d_cents, d_acc, d_counts, d_shift, nullptr);
        },
        centroids_out, assign_out, iters_done);
}
int vs_ivf_build_nd(const float* base_host, int64_t n_rows, int dim, int nlist, int max_iter, double tol, uint64_t seed, int device,
                    float* centroids_out, int32_t* assign_out, int* iters_done) {
    return guarded([&]() -> int {
        return ivf_build_nd_impl(base_host, n_rows, dim, nlist, max_iter, tol, seed, device, centroids_out, assign_out, iters_done);
    });
}

// build_ivf_index_reordered (create_ivf_model_reordered.py:82-177) end to end: k-means, reordered layout, resident index.
// build = vs_ivf_build or vs_ivf_build_nd.
extern "C++" template <class Build>
static int ivf_build_index_with(Build build, const float* base_host, int64_t n_rows, int dim, int nl, int max_iter, double tol,
                                uint64_t seed, int device, vs_index** out, int* iters_done) {
    std::vector<float> cents((size_t)nl * dim);
    std::vector<int32_t> assign((size_t)n_rows), off((size_t)nl + 1), r2o((size_t)n_rows);
    int rc = build(base_host, n_rows, dim, nl, max_iter, tol, seed, device, cents.data(), assign.data(), iters_done);
    if (rc) return rc;
    if ((rc = vs_ivf_layout(assign.data(), n_rows, nl, off.data(), r2o.data()))) return rc;
    std::vector<float> vr((size_t)n_rows * dim);
    for (int64_t i = 0; i < n_rows; ++i)
        std::memcpy(&vr[(size_t)i * dim], base_host + (size_t)r2o[(size_t)i] * dim, (size_t)dim * sizeof(float));
    return ivf_create_impl(vr.data(), n_rows, dim, cents.data(), nl, off.data(), r2o.data(), device, 0, 1, out);
}

int vs_ivf_build_index(const float* base_host, int64_t n_rows, int dim, int nlist, int max_iter, double tol, uint64_t seed,
                       int device, vs_index** out, int* iters_done) {
    if (!out || !base_host || n_rows <= 0 || nlist <= 0) {
        set_error("vs_ivf_build_index: bad arguments");
        return VS_ERR_INVALID;
    }
    return guarded([&]() -> int {
        return ivf_build_index_with(vs_ivf_build, base_host, n_rows, dim, vs_ivf_clamp_nlist(n_rows, nlist), max_iter, tol, seed, device,
                                    out, iters_done);
    });
}

int vs_ivf_build_index_nd(const float* base_host, int64_t n_rows, int dim, int nlist, int max_iter, double tol, uint64_t seed,
                          int device, vs_index** out, int* iters_done) {
    if (!out || !base_host || n_rows <= 0 || nlist <= 0) {
        set_error("vs_ivf_build_index_nd: bad arguments");
        return VS_ERR_INVALID;
    }
    return guarded([&]() -> int {
        const int nl = vs_ivf_clamp_nlist(n_rows, nlist);
        // vs_ivf_build_nd's argument checks that decide the size of the arrays below, in its order
        if (nl > n_rows || max_iter < 0 || dim < 1) {
            set_error("vs_ivf_build_index_nd: bad arguments");
            return VS_ERR_INVALID;
        }
        if (dim > vs::kNdMaxDim) {
            set_error("vs_ivf_build_index_nd: dim " + std::to_string(dim) + " is above the largest supported, 2048");
            return VS_ERR_UNSUPPORTED;
        }
        return ivf_build_index_with(vs_ivf_build_nd, base_host, n_rows, dim, nl, max_iter, tol, seed, device, out, iters_done);
    });
}

int vs_ivf_create(const float* vectors_reordered, int64_t n_rows, int dim, const float* centroids, int nlist,
                  const int32_t* cluster_offsets, const int32_t* reorder_to_original, int device, int rank, int world,
                  vs_index** out) {
    return guarded([&]() -> int {
        return ivf_create_impl(vectors_reordered, n_rows, dim, centroids, nlist, cluster_offsets, reorder_to_original, device, rank,
                               world, out);
    });
}

// uint8 rows: vs_ivf_create's checks and index, unsharded, plus the byte copy on a general index
int vs_ivf_create_nd_u8(const uint8_t* vectors_reordered, int64_t n_rows, int dim, const float* centroids, int nlist,
                        const int32_t* cluster_offsets, const int32_t* reorder_to_original, int device, vs_index** out) {
    return guarded([&]() -> int {
        if (!vectors_reordered) {
            set_error("vs_ivf_create_nd_u8: bad arguments");
            return VS_ERR_INVALID;
        }
        return ivf_create_impl(nullptr, n_rows, dim, centroids, nlist, cluster_offsets, reorder_to_original, device, 0, 1, out,
                               vectors_reordered);
    });
}

int vs_ivf_load(const char* index_dir, int device, int rank, int world, vs_index** out) {
    if (!index_dir || !out) {
        set_error("vs_ivf_load: bad arguments");
        return VS_ERR_INVALID;
    }
    return guarded([&]() -> int {
    const std::string dir(index_dir);
    vs::IvfConfig cfg;
    if (!vs::ivf_config_read(dir + "/ivf_config.json", cfg)) return VS_ERR_IO;
    std::vector<int32_t> offsets, r2o;
    std::vector<float> vecs, cents;
    std::vector<int64_t> shp;
    if (!vs::npy_read_i32(dir + "/cluster_offsets.npy", offsets, shp)) return VS_ERR_IO;  // IVFIndex.cpp:210-213
    if (!vs::npy_read_f32(dir + "/centroids.npy", cents, shp)) return VS_ERR_IO;
    if (shp.size() != 2 || shp[0] != cfg.n_clusters || shp[1] != cfg.dim) {
        set_error("centroids.npy shape does not match ivf_config.json");
        return VS_ERR_IO;
    }
    if ((int64_t)offsets.size() != cfg.n_clusters + 1) {
        set_error("cluster_offsets.npy length != n_clusters + 1");
        return VS_ERR_IO;
    }
    if (cfg.reordered) {
        if (!vs::npy_read_i32(dir + "/reorder_to_original.npy", r2o, shp)) return VS_ERR_IO;  // IVFIndex.cpp:225-228
        if (!vs::npy_read_f32(dir + "/vectors_reordered.npy", vecs, shp)) return VS_ERR_IO;   // IVFIndex.cpp:239-244
    } else {
        // plain mode (IVFIndex.cpp:216-222,247-252): gather into the contiguous layout at load time
        std::vector<int32_t> cidx;
        std::vector<float> plain;
        if (!vs::npy_read_i32(dir + "/cluster_indices.npy", cidx, shp)) return VS_ERR_IO;
        if (!vs::npy_read_f32(dir + "/vectors.npy", plain, shp)) return VS_ERR_IO;
        if (shp.size() != 2 || shp[1] != cfg.dim) {
            set_error("vectors.npy shape mismatch");
            return VS_ERR_IO;
        }
        const int64_t n = (int64_t)cidx.size();
        vecs.resize((size_t)n * cfg.dim);
        r2o = cidx;
        for (int64_t i = 0; i < n; ++i) {
            if (cidx[i] < 0 || cidx[i] >= shp[0]) {
                set_error("cluster_indices.npy out of range");
                return VS_ERR_IO;
            }
            std::memcpy(&vecs[(size_t)i * cfg.dim], &plain[(size_t)cidx[i] * cfg.dim], (size_t)cfg.dim * sizeof(float));
        }
    }
    const int64_t n = (int64_t)vecs.size() / std::max<int64_t>(cfg.dim, 1);
    if (n != cfg.n_vectors || (int64_t)r2o.size() != n) {
        set_error("vector count does not match ivf_config.json");
        return VS_ERR_IO;
    }
    for (int32_t v : r2o)
        if (v < 0 || v >= n) {
            set_error("reorder_to_original.npy holds an id outside [0, n_vectors)");
            return VS_ERR_IO;
        }
    int rc = ivf_create_impl(vecs.data(), n, (int)cfg.dim, cents.data(), (int)cfg.n_clusters, offsets.data(), r2o.data(),
                             device, rank, world, out);
    if (rc == VS_OK && cfg.avg_cluster_size > 0) (*out)->avg_cluster_size = cfg.avg_cluster_size;
    return rc;
    });
}

int vs_ivf_save(vs_index* h, const char* index_dir) {
    if (refuse_general_bf(h, "vs_ivf_save")) return VS_ERR_UNSUPPORTED;
    if (!h || h->kind != 1 || !index_dir) {
        set_error("vs_ivf_save: bad arguments");
        return VS_ERR_INVALID;
    }
    if (h->world != 1) {
        set_error("vs_ivf_save needs an unsharded index");
        return VS_ERR_UNSUPPORTED;
    }
    int rc = set_device(h);
    if (rc) return rc;
    const std::string dir(index_dir);
    std::vector<float> vecs((size_t)h->n_rows * h->dim), cents((size_t)h->nlist * h->dim);
    std::vector<int32_t> r2o((size_t)h->n_rows);
    // unpadded [n_rows][dim] arrays (a general index keeps rows of dim_p floats on the device)
    const size_t row_b = (size_t)h->dim * sizeof(float), ld_b = (size_t)h->dim_p * sizeof(float);
    HIPCHK(hipMemcpy2D(vecs.data(), row_b, h->d_vecs, ld_b, row_b, (size_t)h->n_rows, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy2D(cents.data(), row_b, h->d_centroids, ld_b, row_b, (size_t)h->nlist, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(r2o.data(), h->d_r2o, r2o.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
    std::vector<int32_t> sizes(h->nlist);
    int32_t mn = std::numeric_limits<int32_t>::max(), mx = 0;
    for (int c = 0; c < h->nlist; ++c) {
        sizes[c] = h->h_offsets_global[c + 1] - h->h_offsets_global[c];
        mn = std::min(mn, sizes[c]);
        mx = std::max(mx, sizes[c]);
    }
    vs::IvfConfig cfg;
    cfg.n_vectors = h->n_rows;
    cfg.n_clusters = h->nlist;
    cfg.dim = h->dim;
    cfg.batch_size = h->batch;
    cfg.avg_cluster_size = (double)h->n_rows / h->nlist;
    cfg.min_cluster_size = mn;
    cfg.max_cluster_size = mx;
    cfg.reordered = true;
    if (!vs::ivf_config_write(dir + "/ivf_config.json", cfg)) return VS_ERR_IO;
    if (!vs::npy_write(dir + "/vectors_reordered.npy", vecs.data(), "<f4", {h->n_rows, h->dim}, 4)) return VS_ERR_IO;
    if (!vs::npy_write(dir + "/reorder_to_original.npy", r2o.data(), "<i4", {h->n_rows}, 4)) return VS_ERR_IO;
    if (!vs::npy_write(dir + "/cluster_offsets.npy", h->h_offsets_global.data(), "<i4", {h->nlist + 1}, 4)) return VS_ERR_IO;
    if (!vs::npy_write(dir + "/cluster_sizes.npy", sizes.data(), "<i4", {h->nlist}, 4)) return VS_ERR_IO;
    if (!vs::npy_write(dir + "/centroids.npy", cents.data(), "<f4", {h->nlist, h->dim}, 4)) return VS_ERR_IO;
    return VS_OK;
}

int vs_ivf_search_dev(vs_index* h, const float* queries_dev, int B, int k, int nprobe, int32_t* ids_dev,
                      float* dists_dev, void* stream) {
    if (refuse_general_bf(h, "vs_ivf_search_dev")) return VS_ERR_UNSUPPORTED;
    if (!h || h->kind != 1 || !queries_dev || !ids_dev || !dists_dev || B < 1 || B > vs::kMaxBatch || k < 1 || nprobe < 1) {
        set_error("vs_ivf_search_dev: bad arguments");
        return VS_ERR_INVALID;
    }
    if (k > 16 && refuse_general_ivf(h, "vs_ivf_search_dev with k > 16")) return VS_ERR_UNSUPPORTED;
    nprobe = std::min(nprobe, h->nlist);  // IVFIndex.cpp:647
    if (nprobe > kMaxNprobe) {
        set_error("nprobe > 256 not supported");
        return VS_ERR_UNSUPPORTED;
    }
    int rc = set_device(h);
    if (rc) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    if ((rc = order_begin(h, st))) return rc;
    rc = ivf_multi_dev(h, queries_dev, 1, B, k, nprobe, dists_dev, ids_dev, st);
    return rc ? rc : order_end(h, st);
}

int vs_ivf_search_dev_multi(vs_index* h, const float* queries_dev, int n_batches, int B, int k, int nprobe, int32_t* ids_dev,
                            float* dists_dev, void* stream) {
    if (refuse_general_bf(h, "vs_ivf_search_dev_multi")) return VS_ERR_UNSUPPORTED;
    if (!h || h->kind != 1 || !queries_dev || !ids_dev || !dists_dev || n_batches < 1 || B < 1 || B > vs::kMaxBatch || k < 1 ||
        nprobe < 1) {
        set_error("vs_ivf_search_dev_multi: bad arguments");
        return VS_ERR_INVALID;
    }
    if (k > 16 && refuse_general_ivf(h, "vs_ivf_search_dev_multi with k > 16")) return VS_ERR_UNSUPPORTED;
    nprobe = std::min(nprobe, h->nlist);  // IVFIndex.cpp:647
    if (nprobe > kMaxNprobe) {
        set_error("nprobe > 256 not supported");
        return VS_ERR_UNSUPPORTED;
    }
    int rc = set_device(h);
    if (rc) return rc;
    hipStream_t user = static_cast<hipStream_t>(stream);
    if ((rc = order_begin(h, user))) return rc;
    rc = ivf_multi_dev(h, queries_dev, n_batches, B, k, nprobe, dists_dev, ids_dev, user);
    return rc ? rc : order_end(h, user);
}

int vs_ivf_search_topk_dev_multi(vs_index* h, const float* queries_dev, int n_batches, int B, int k, int nprobe, int32_t* ids_dev,
                                 float* dists_dev, void* stream) {
    if (h && h->kind == 0) {
        set_error("vs_ivf_search_topk_dev_multi: not an IVF index");
        return VS_ERR_UNSUPPORTED;
    }
    if (!h || !queries_dev || !ids_dev || !dists_dev || n_batches < 1 || B < 1 || B > vs::kMaxBatch || k < 1 || nprobe < 1) {
        set_error("vs_ivf_search_topk_dev_multi: bad arguments");
        return VS_ERR_INVALID;
    }
    if (k > vs::kIvfNdWideKMax) {
        set_error("vs_ivf_search_topk_dev_multi: k > 128");
        return VS_ERR_UNSUPPORTED;
    }
    if (k <= 16 || !h->general) return vs_ivf_search_dev_multi(h, queries_dev, n_batches, B, k, nprobe, ids_dev, dists_dev, stream);
    nprobe = std::min(nprobe, h->nlist);
    if (nprobe > kMaxNprobe) {
        set_error("nprobe > 256 not supported");
        return VS_ERR_UNSUPPORTED;
    }
    int rc = set_device(h);
    if (rc) return rc;
    hipStream_t user = static_cast<hipStream_t>(stream);
    if ((rc = order_begin(h, user))) return rc;
    rc = ivf_multi_dev(h, queries_dev, n_batches, B, k, nprobe, dists_dev, ids_dev, user);
    return rc ? rc : order_end(h, user);
}

// The metric of one call: the kernels, the coarse scores and the host pipeline's sign all read h->metric, so the call runs
// with it set to its own metric and puts the index's setting back on every way out.  (Calls on one index are not
// concurrent: its scratch is one set.)
struct CallMetric {
    vs_index* h;
    int saved;
    CallMetric(vs_index* h_, int metric) : h(h_), saved(h_->metric) { h->metric = metric; }
    ~CallMetric() { h->metric = saved; }
    CallMetric(const CallMetric&) = delete;
    CallMetric& operator=(const CallMetric&) = delete;
};

// the checks the two vs_ivf_search_metric* calls share, in the order vsearch.h states them
static int search_metric_checks(const char* who, const vs_index* h, bool ptrs_ok, int k, int metric) {
    char msg[160];
    if (!h || !ptrs_ok) {
        snprintf(msg, sizeof(msg), "%s: null argument", who);
        set_error(msg);
        return VS_ERR_INVALID;
    }
    if (h->kind == 0) {
        snprintf(msg, sizeof(msg), "%s: not an IVF index", who);
        set_error(msg);
        return VS_ERR_UNSUPPORTED;
    }
    if (metric != VS_METRIC_L2 && metric != VS_METRIC_IP) {
        snprintf(msg, sizeof(msg), "%s: metric must be VS_METRIC_L2 or VS_METRIC_IP", who);
        set_error(msg);
        return VS_ERR_INVALID;
    }
    if (k < 1) {
        snprintf(msg, sizeof(msg), "%s: k < 1", who);
        set_error(msg);
        return VS_ERR_INVALID;
    }
    if (k > vs::kIvfNdWideKMax) {
        snprintf(msg, sizeof(msg), "%s: k > 128", who);
        set_error(msg);
        return VS_ERR_UNSUPPORTED;
    }
    return VS_OK;
}

int vs_ivf_search_metric_dev_multi(vs_index* h, const float* queries_dev, int n_batches, int B, int k, int nprobe, int metric,
                                   int32_t* ids_dev, float* dists_dev, void* stream) {
    const int rc = search_metric_checks("vs_ivf_search_metric_dev_multi", h, queries_dev && ids_dev && dists_dev, k, metric);
    if (rc) return rc;
    CallMetric cm(h, metric);
    return vs_ivf_search_topk_dev_multi(h, queries_dev, n_batches, B, k, nprobe, ids_dev, dists_dev, stream);
}

#ifdef VS_STAMPS
// diagnostic builds only (make EXTRA=-DVS_STAMPS; not part of the ABI): state of the wide IVF pipeline after the last launch group
__attribute__((visibility("default"))) int vs_debug_ivf_wide_stats(vs_index* h, int64_t* out /*[8]*/) {
    if (!h || !h->wide[0].lq) return VS_ERR_INVALID;
    (void)hipSetDevice(h->device);
    (void)hipDeviceSynchronize();
    const size_t nq = (size_t)h->ivf_gb * 32;
    const int n_sb_max = h->ivf_nsb;
    std::vector<int32_t> z(h->wide[0].zero_words);
    std::vector<float> tau(nq);
    HIPCHK(hipMemcpy(z.data(), h->wide[0].zero, z.size() * 4, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(tau.data(), h->wide[0].tau, nq * 4, hipMemcpyDeviceToHost));
    const int32_t* slow = z.data() + (size_t)n_sb_max * vs::ivf_wide_plan_words(h->nlist);
    const int32_t* ovf = slow + nq;
    const int32_t* cnt = ovf + 16 + h->ivf_gb;
    int64_t nslow = 0, total = 0, maxw = 0, maxsub = 0, ninf = 0;
    for (size_t i = 0; i < nq; ++i) nslow += slow[i] != 0;
    for (size_t i = 0; i < nq; ++i) ninf += !(tau[i] < 3e38f);
    for (size_t i = 0; i < nq * kWideSub; ++i) maxsub = std::max<int64_t>(maxsub, cnt[i]);
    out[0] = ovf[0];
    out[1] = nslow;
    out[3] = maxw;
    out[4] = maxsub;
    out[5] = ninf;
    out[6] = z[(size_t)h->nlist * vs::kIvfWideCntStride];  // records of super-batch 0
    int64_t big = 0, maxq = 0;
    for (size_t i = 0; i < nq; ++i) {
        int64_t t = 0;
        for (int g = 0; g < kWideSub; ++g) t += cnt[(size_t)g * nq + i];
        big += t > 256;
        maxq = std::max(maxq, t);
        total += t;
    }
    out[2] = total;
    out[7] = big * 100000 + maxq;
    return VS_OK;
}
#endif

#if defined(VS_STAMPS) || defined(VS_F32F_ENDS)
// diagnostic builds only: where the stamping kernels write
__attribute__((visibility("default"))) int vs_debug_buffer(int* dev_ptr) {
    g_dbg = dev_ptr;
    return VS_OK;
}
#endif

// --------------------------------------------------------------------------------------- multi-GPU
// vs::merge_plan for the ABI: the kernel of (G, kin) and the two constants into out[3] (may be null), or VS_ERR_UNSUPPORTED where there is none
static int merge_plan_checked(const char* who, int G, int kin, int64_t* out) {
    int cap = 0, track = 0;
    const int lpt = vs::merge_plan(G, kin, &cap, &track);
    if (lpt < 0) {
        set_error(std::string(who) + ": G*kin = " + std::to_string((int64_t)G * kin) + " is above " + std::to_string(cap) +
                  " and G = " + std::to_string(G) + " is above the largest supported there, " + std::to_string(vs::kMergeMaxLists));
        return VS_ERR_UNSUPPORTED;
    }
    if (out) {
        out[0] = lpt;
        out[1] = cap;
        out[2] = track;
    }
    return VS_OK;
}

int vs_topk_merge_plan(int G, int kin, int kout, int64_t* out) {
    if (!out || G < 1 || kin < 1 || kout < 1) {
        set_error("vs_topk_merge_plan: bad arguments (out != NULL, G, kin, kout >= 1)");
        return VS_ERR_INVALID;
    }
    return merge_plan_checked("vs_topk_merge_plan", G, kin, out);
}

// one_route for the ABI (host only): the index shape comes as arguments; dim == 128 stands for the specialised index
// unless VSEARCH_ND_FORCE makes vs_bf_create build the general one there too
int vs_bf_one_plan(int64_t n_rows, int dim, int num_cus, int n_batches, int B, int k, int64_t* out) {
    if (!out || n_rows < 1 || num_cus < 1 || n_batches < 1 || B < 1 || B > vs::kMaxBatch || k < 1) {
        set_error("vs_bf_one_plan: bad arguments (out != NULL, n_rows, num_cus, n_batches, k >= 1, 1 <= B <= 32)");
        return VS_ERR_INVALID;
    }
    if (dim < 1) {
        set_error("vs_bf_one_plan: dim must be at least 1");
        return VS_ERR_INVALID;
    }
    if (dim > vs::kNdMaxDim) {
        set_error("vs_bf_one_plan: dim > 2048 is not compiled in");
        return VS_ERR_UNSUPPORTED;
    }
    if (k > vs::kTopkWideMax - 1) {
        set_error("vs_bf_one_plan: k > 128 is not compiled in");
        return VS_ERR_UNSUPPORTED;
    }
    one_route(n_rows, dim != vs::kDim || g_nd_force != 0, num_cus, n_batches, B, k + 1, out);
    return VS_OK;
}

// one_route_u8 for the ABI (host only): vs_bf_one_plan's checks in its order; whether an index keeps a byte copy, its
// precision setting and VSEARCH_ND_ONE_U8 are not its business
int vs_bf_one_plan_u8(int64_t n_rows, int dim, int num_cus, int n_batches, int B, int k, int64_t* out) {
    if (!out || n_rows < 1 || num_cus < 1 || n_batches < 1 || B < 1 || B > vs::kMaxBatch || k < 1) {
        set_error("vs_bf_one_plan_u8: bad arguments (out != NULL, n_rows, num_cus, n_batches, k >= 1, 1 <= B <= 32)");
        return VS_ERR_INVALID;
    }
    if (dim < 1) {
        set_error("vs_bf_one_plan_u8: dim must be at least 1");
        return VS_ERR_INVALID;
    }
    if (dim > vs::kNdMaxDim) {
        set_error("vs_bf_one_plan_u8: dim > 2048 is not compiled in");
        return VS_ERR_UNSUPPORTED;
    }
    if (k > vs::kTopkWideMax - 1) {
        set_error("vs_bf_one_plan_u8: k > 128 is not compiled in");
        return VS_ERR_UNSUPPORTED;
    }
    one_route_u8(n_rows, dim, num_cus, n_batches, B, k + 1, out);
    return VS_OK;
}

// wide_route_u8 and topw_prefix for the ABI (host only); whether an index keeps a byte copy, its precision setting and
// VSEARCH_ND_WIDE_U8 are not its business
int vs_bf_wide_plan(int64_t n_rows, int dim, int k, int64_t* out) {
    if (!out || n_rows < 1 || k < 1) {
        set_error("vs_bf_wide_plan: bad arguments (out != NULL, n_rows, k >= 1)");
        return VS_ERR_INVALID;
    }
    if (dim < 1) {
        set_error("vs_bf_wide_plan: dim must be at least 1");
        return VS_ERR_INVALID;
    }
    if (dim > vs::kNdMaxDim) {
        set_error("vs_bf_wide_plan: dim > 2048 is not compiled in");
        return VS_ERR_UNSUPPORTED;
    }
    if (k > vs::kTopkWideMax - 1) {
        set_error("vs_bf_wide_plan: k > 128 is not compiled in");
        return VS_ERR_UNSUPPORTED;
    }
    out[0] = out[1] = out[2] = 0;
    if (k + 1 <= kKcapMax) return VS_OK;  // not a wide call
    out[0] = wide_route_u8(n_rows, dim, k + 1) ? 1 : 0;
    out[1] = topw_prefix(n_rows, k + 1);
    out[2] = kTopwFilterCap;
    return VS_OK;
}

int vs_bf_wide_stats(vs_index* h, int64_t* out, int reset) {
    if (!h || h->kind != 0 || !out) {
        set_error("vs_bf_wide_stats: a brute-force index and an output of three words");
        return VS_ERR_INVALID;
    }
    int rc = set_device(h);
    if (rc) return rc;
    HIPCHK(hipDeviceSynchronize());
    unsigned long long c[2] = {0, 0};
    if (h->d_wide_cnt) HIPCHK(hipMemcpy(c, h->d_wide_cnt, sizeof(c), hipMemcpyDeviceToHost));
    out[0] = (int64_t)c[0];
    out[1] = (int64_t)c[1];
    out[2] = h->wide_batches;
    if (reset) {
        if (h->d_wide_cnt) HIPCHK(hipMemset(h->d_wide_cnt, 0, sizeof(c)));
        h->wide_batches = 0;
    }
    return VS_OK;
}

int vs_bf_one_stats(vs_index* h, int64_t* out, int reset) {
    if (!h || h->kind != 0 || !out) {
        set_error("vs_bf_one_stats: a brute-force index and an output of two words");
        return VS_ERR_INVALID;
    }
    out[0] = h->one_stat[0];
    out[1] = h->one_stat[1];
    if (reset) h->one_stat[0] = h->one_stat[1] = 0;
    return VS_OK;
}

// ivf_one_route for the ABI (host only): the index shape comes as arguments.  VSEARCH_IVF_ONE and the byte copy of a
// vs_ivf_create_nd_u8 index are not its business.
int vs_ivf_one_plan(int64_t n_rows, int dim, int nlist, int num_cus, int n_batches, int B, int k, int nprobe, int64_t* out) {
    if (!out || n_rows < 1 || nlist < 1 || num_cus < 1 || n_batches < 1 || B < 1 || B > vs::kMaxBatch || k < 1 || nprobe < 1) {
        set_error("vs_ivf_one_plan: bad arguments (out != NULL, n_rows, nlist, num_cus, n_batches, k, nprobe >= 1, 1 <= B <= 32)");
        return VS_ERR_INVALID;
    }
    if (dim < 1) {
        set_error("vs_ivf_one_plan: dim must be at least 1");
        return VS_ERR_INVALID;
    }
    if (dim > vs::kNdMaxDim) {
        set_error("vs_ivf_one_plan: dim > 2048 is not compiled in");
        return VS_ERR_UNSUPPORTED;
    }
    if (k > vs::kIvfWideKMax) {
        set_error("vs_ivf_one_plan: k > 128 is not compiled in");
        return VS_ERR_UNSUPPORTED;
    }
    ivf_one_route(n_rows, nlist, num_cus, n_batches, B, k, nprobe, out);
    return VS_OK;
}

// ivf_one_route_u8 for the ABI (host only), vs_ivf_one_plan's checks in its order.  The toggles, the precision and
// whether the byte copy was kept are not its business.
int vs_ivf_one_plan_u8(int64_t n_rows, int dim, int nlist, int num_cus, int n_batches, int B, int k, int nprobe, int64_t* out) {
    if (!out || n_rows < 1 || nlist < 1 || num_cus < 1 || n_batches < 1 || B < 1 || B > vs::kMaxBatch || k < 1 || nprobe < 1) {
        set_error("vs_ivf_one_plan_u8: bad arguments (out != NULL, n_rows, nlist, num_cus, n_batches, k, nprobe >= 1, 1 <= B <= 32)");
        return VS_ERR_INVALID;
    }
    if (dim < 1) {
        set_error("vs_ivf_one_plan_u8: dim must be at least 1");
        return VS_ERR_INVALID;
    }
    if (dim > vs::kNdMaxDim) {
        set_error("vs_ivf_one_plan_u8: dim > 2048 is not compiled in");
        return VS_ERR_UNSUPPORTED;
    }
    if (k > vs::kIvfWideKMax) {
        set_error("vs_ivf_one_plan_u8: k > 128 is not compiled in");
        return VS_ERR_UNSUPPORTED;
    }
    ivf_one_route_u8(n_rows, dim, nlist, num_cus, n_batches, B, k, nprobe, out);
    return VS_OK;
}

int vs_topk_merge_dev(const float* dists_dev, const int32_t* ids_dev, int G, int B, int kin, int64_t stride_g,
                      int kout, float* out_dists_dev, int32_t* out_ids_dev, int32_t* flags_dev, void* stream) {
    if (!dists_dev || !ids_dev || !out_dists_dev || !out_ids_dev || G < 1 || B < 1 || kin < 1 || kout < 1) {
        set_error("vs_topk_merge_dev: bad arguments");
        return VS_ERR_INVALID;
    }
    if (stride_g < 0 || (stride_g > 0 && stride_g < (int64_t)B * kin)) {
        set_error("vs_topk_merge_dev: stride_g must be 0 (dense) or at least B*kin = " + std::to_string((int64_t)B * kin) +
                  " (got " + std::to_string(stride_g) + ")");
        return VS_ERR_INVALID;
    }
    if (int rc = merge_plan_checked("vs_topk_merge_dev", G, kin, nullptr)) return rc;
    vs::MergeParams m{};
    m.part_d = dists_dev;
    m.part_i = ids_dev;
    m.G = G;
    m.kin = kin;
    m.nq = B;
    m.kout = kout;
    m.out_d = out_dists_dev;
    m.out_i = out_ids_dev;
    m.flags = flags_dev;
    HIPCHK(vs::launch_merge_layout(m, stride_g > 0 ? stride_g : (int64_t)B * kin, kin, static_cast<hipStream_t>(stream)));
    return VS_OK;
}

}  // extern "C"

// --------------------------------------------------------------------------------------- multi-GPU
// One process per GPU.  The only data-path collective of the hot path is the all-gather of per-shard top-k lists
// (SURVEY.md 8e); it lives here, behind the ABI: a vs_comm owns an RCCL communicator, a stream for the collective
// and two sets of exchange buffers, so that all-gather + merge of launch group g run beside the scan of group g + 1.
// RCCL is bound at run time (dlopen of librccl.so.1: inside a PyTorch process that is the copy torch already loaded,
// otherwise ROCm's), so single-GPU users of the library do not need it at all.
namespace {

struct RcclApi {
    void* lib = nullptr;
    ncclResult_t (*GetUniqueId)(ncclUniqueId*) = nullptr;
    ncclResult_t (*CommInitRank)(ncclComm_t*, int, ncclUniqueId, int) = nullptr;
    ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
    ncclResult_t (*AllGather)(const void*, void*, size_t, ncclDataType_t, ncclComm_t, hipStream_t) = nullptr;
    const char* (*GetErrorString)(ncclResult_t) = nullptr;
    std::string err;
};

RcclApi& rccl() {
    static RcclApi api = [] {
        RcclApi a;
        std::vector<std::string> names = {"librccl.so.1", "librccl.so"};
        if (const char* rp = getenv("ROCM_PATH")) names.push_back(std::string(rp) + "/lib/librccl.so.1");
        names.push_back("/opt/rocm/lib/librccl.so.1");
        for (const std::string& n : names) {
            a.lib = dlopen(n.c_str(), RTLD_NOW | RTLD_LOCAL);
            if (a.lib) break;
            if (const char* e = dlerror()) a.err = e;
        }
        if (!a.lib) return a;
        a.GetUniqueId = reinterpret_cast<decltype(a.GetUniqueId)>(dlsym(a.lib, "ncclGetUniqueId"));
        a.CommInitRank = reinterpret_cast<decltype(a.CommInitRank)>(dlsym(a.lib, "ncclCommInitRank"));
        a.CommDestroy = reinterpret_cast<decltype(a.CommDestroy)>(dlsym(a.lib, "ncclCommDestroy"));
        a.AllGather = reinterpret_cast<decltype(a.AllGather)>(dlsym(a.lib, "ncclAllGather"));
        a.GetErrorString = reinterpret_cast<decltype(a.GetErrorString)>(dlsym(a.lib, "ncclGetErrorString"));
        if (!a.GetUniqueId || !a.CommInitRank || !a.CommDestroy || !a.AllGather || !a.GetErrorString) {
            a.err = "librccl is missing a required symbol";
            a.lib = nullptr;
        }
        return a;
    }();
    return api;
}

int rccl_ready() {
    if (rccl().lib) return VS_OK;
    set_error("RCCL not available: " + rccl().err);
    return VS_ERR_DEVICE;
}

#define NCCLCHK(expr)                                                                                  \
    do {                                                                                               \
        ncclResult_t _r = (expr);                                                                      \
        if (_r != ncclSuccess) {                                                                       \
            set_error(std::string(#expr) + ": " + rccl().GetErrorString(_r));                          \
            return VS_ERR_DEVICE;                                                                      \
        }                                                                                              \
    } while (0)

}  // namespace

struct vs_comm {
    ncclComm_t comm = nullptr;
    int rank = 0, world = 1, device = 0;
    vs::Stream s_coll;
    vs::Event ev_scan[2], ev_coll[2];
    bool coll_used[2] = {false, false};
    vs::DevBuf<int32_t> d_loc[2];   // this rank's lists of one launch group: [dists n*kin][ids n*kin] as 32-bit words
    vs::DevBuf<int32_t> d_gath[2];  // [world] x the same
    vs::Event ev_front[2], ev_probe[2];  // cluster-sharded IVF: a lane's blocks are written / exchanged (ivf_sliced_groups)
};

namespace {

// two pairs of grow-only buffers of a communicator: `words` each in own[], `words` per rank in gath[] (the device is
// synchronised before any of them is replaced)
int reserve_pairs(vs::DevBuf<int32_t> (&own)[2], vs::DevBuf<int32_t> (&gath)[2], size_t words, int world) {
    bool grow = false;
    for (int i = 0; i < 2; ++i) grow |= own[i].size() < words || gath[i].size() < words * (size_t)world;
    if (grow) HIPCHK(hipDeviceSynchronize());
    int rc = VS_OK;
    for (int i = 0; i < 2 && !rc; ++i)
        if (!(rc = own[i].reserve(words))) rc = gath[i].reserve(words * (size_t)world);
    return rc;
}


// groups of <= kMaxMulti batches: local top-kin of group g on `user` -> event -> (collective stream) all-gather + merge
// into the caller's outputs; the local search of group g + 1 is enqueued on `user` right away and runs meanwhile.
template <class LocalSearch>
int sharded_groups(vs_index* h, vs_comm* c, int n_batches, int B, int kin, int kout, int32_t* ids_dev, float* dists_dev,
                   int32_t* flags_dev, const int32_t* id_map_unused, hipStream_t user, LocalSearch local) {
    (void)id_map_unused;
    if (h->device != c->device) {
        set_error("index and communicator live on different devices");
        return VS_ERR_INVALID;
    }
    int rc = reserve_pairs(c->d_loc, c->d_gath, (size_t)(2 * kin + 1) * kMaxMulti * 32, c->world);
    if (rc) return rc;
    int g = 0;
    for (int b0 = 0; b0 < n_batches; b0 += kMaxMulti, ++g) {
        const int nb = std::min(kMaxMulti, n_batches - b0);
        const int buf = g & 1;
        const size_t n = (size_t)nb * B;         // queries of the group
        const size_t words = 2 * n * kin + (flags_dev ? n : 0);  // per rank: dists | ids | (brute force) the shard's own flags
        if (c->coll_used[buf]) HIPCHK(hipStreamWaitEvent(user, c->ev_coll[buf], 0));  // group g - 2 is done with the buffers
        float* loc_d = reinterpret_cast<float*>(c->d_loc[buf].get());
        int32_t* loc_i = c->d_loc[buf] + n * kin;
        if ((rc = local(b0, nb, loc_d, loc_i, c->d_loc[buf] + 2 * n * kin, user))) return rc;
        HIPCHK(hipEventRecord(c->ev_scan[buf], user));
        HIPCHK(hipStreamWaitEvent(c->s_coll, c->ev_scan[buf], 0));
        const int32_t* src = c->d_loc[buf];
        if (c->world > 1) {
            NCCLCHK(rccl().AllGather(c->d_loc[buf], c->d_gath[buf], words, ncclInt32, c->comm, c->s_coll));
            src = c->d_gath[buf];
        }
        vs::MergeParams m{};
        m.part_d = reinterpret_cast<const float*>(src);
        m.part_i = src + n * kin;
        m.G = c->world;
        m.kin = kin;
        m.nq = (int)n;
        m.kout = kout;
        m.out_d = dists_dev + (size_t)b0 * B * kout;
        m.out_i = ids_dev + (size_t)b0 * B * kout;
        m.flags = flags_dev ? flags_dev + (size_t)b0 * B : nullptr;
        m.flag_empty = 1;
        if (flags_dev) {  // a shard that skipped a batch (int8 rows, non-byte query) must not go unnoticed: its rows are missing
            m.shard_flags = src + 2 * n * kin;
            m.shard_flags_stride = (int64_t)words;
        }
        HIPCHK(vs::launch_merge_layout(m, (int64_t)words, kin, c->s_coll));
        HIPCHK(hipEventRecord(c->ev_coll[buf], c->s_coll));
        c->coll_used[buf] = true;
    }
    // the caller's stream continues after the last two groups' merges
    for (int buf = 0; buf < 2; ++buf)
        if (c->coll_used[buf]) HIPCHK(hipStreamWaitEvent(user, c->ev_coll[buf], 0));
    return VS_OK;
}

// ---- The shards one process drives: either ONE shard of a collective job (c: the other ranks run the same code, the
// exchanges are RCCL all-gathers) or ALL G shards on one device (virtual ranks: an exchange is a no-op, every shard has
// written its part of the gathered buffer in place).  Everything else -- per-shard device steps, merge, host steps -- is
// the same code.  Brute force: shards are contiguous row ranges in rank order (vs_bf_create(rows of the shard, id_offset =
// first row)), and vs_bf_search / vs_bf_search_topk are one index (G = 1, no communicator) without the merge.  IVF: shard r
// is the index created with (rank r, world G).
struct Shards {
    std::vector<vs_index*> hs;  // the shards driven here; hs[i] is global shard first + i
    int G = 1, first = 0;
    vs_comm* c = nullptr;
    bool merge = true;          // brute force: the shards' lists go through the exchange and the merge (every sharded call, G = 1 included)
    vs_index* owner() const { return hs[0]; }
    hipStream_t s() const { return hs[0]->stream; }
    int exchange(int32_t* buf, size_t words, hipStream_t st) const {  // buf = [G][words], this process's parts in place
        if (!c || c->world == 1) return VS_OK;
        NCCLCHK(rccl().AllGather(buf + (size_t)c->rank * words, buf, words, ncclInt32, c->comm, st));
        return VS_OK;
    }
};

// ---- sliced pipeline of the shards driven here, per launch group of the owner's ivf_gb batches: every shard's front half
// (its own slice) into its part of the gathered blocks [G][block words], the exchange of the blocks, every shard's back half
// (all slices, its own lists) into its part of the gathered lists [G][2 * n * k], the exchange of the lists, one merge into
// the caller's outputs.  With a communicator the groups are software pipelined over two lanes: the caller's stream runs
// F(g), then B(g - 1); the collective stream the exchange of g's blocks, then g - 1's lists and their merge -- the same
// order on every rank -- so that an exchange is in flight while the neighbouring group computes.  Group g uses lane g & 1.
// Virtual ranks run F(g), then B(g), on lane 0 and the caller's stream alone; rank_ms[r] (optional) then adds the device
// time of shard r's two halves.
int ivf_sliced_groups(const Shards& S, const float* q_dev, int n_batches, int B, int k, int nprobe, int32_t* ids, float* dists,
                      double* rank_ms, hipStream_t st) {
    vs_index* o = S.owner();
    vs_comm* c = S.c;
    const int G = S.G, gb = o->ivf_gb, lanes = c ? 2 : 1;
    const hipStream_t sc = c ? static_cast<hipStream_t>(c->s_coll) : st;  // exchanges and merge
    // the owner's gathered buffers of each lane: grown only after a synchronise (an earlier call's groups may still use them)
    const size_t blk_words = (size_t)G * ivf_block_words(vs::kIvfWideBatches, kMaxNprobe), list_words = (size_t)G * 2 * gb * 32 * k;
    bool grow = false;
    for (int l = 0; l < lanes; ++l) grow |= o->sl_blk[l].size() < blk_words || o->sl_lists[l].size() < list_words;
    if (grow) HIPCHK(hipDeviceSynchronize());
    int rc;
    for (int l = 0; l < lanes; ++l)
        if ((rc = o->sl_blk[l].reserve(blk_words)) || (rc = o->sl_lists[l].reserve(list_words))) return rc;
    std::vector<vs::Event> ev;  // rank_ms: start and end of each shard's front and back half
    if (rank_ms) {
        ev.resize((size_t)4 * S.hs.size());
        for (auto& e : ev)
            if ((rc = e.create(true))) return rc;
        for (size_t i = 0; i < S.hs.size(); ++i) rank_ms[S.first + i] = 0;
    }
    auto front = [&](int g) -> int {
        const int lane = g % lanes, b0 = g * gb, nb = std::min(gb, n_batches - b0);
        const float* q = q_dev + (size_t)b0 * B * vs::kDim;
        int sbb = (nb + G - 1) / G, sb0, nbs;
        for (size_t i = 0; i < S.hs.size(); ++i) {
            ivf_slice(nb, G, S.first + (int)i, sbb, sb0, nbs);
            // (the lane's scratch and blocks: group g - 2's back half is behind on this stream, and it waited for that group's exchange)
            int32_t* blk = o->sl_blk[lane] + (size_t)(S.first + i) * ivf_block_words(sbb, nprobe);
            if (rank_ms) HIPCHK(hipEventRecord(ev[4 * i], st));
            if (int r2 = ivf_shard_front(S.hs[i], lane, q, nb, sbb, sb0, nbs, B, k, nprobe, blk, st)) return r2;
            if (rank_ms) HIPCHK(hipEventRecord(ev[4 * i + 1], st));
        }
        if (c) {
            HIPCHK(hipEventRecord(c->ev_front[lane], st));
            HIPCHK(hipStreamWaitEvent(sc, c->ev_front[lane], 0));
        }
        if (int r2 = S.exchange(o->sl_blk[lane], (size_t)ivf_block_words(sbb, nprobe), sc)) return r2;
        if (c) HIPCHK(hipEventRecord(c->ev_probe[lane], sc));
        return VS_OK;
    };
    auto back = [&](int g) -> int {
        const int lane = g % lanes, b0 = g * gb, nb = std::min(gb, n_batches - b0), sbb = (nb + G - 1) / G;  // (= ivf_slice's)
        const float* q = q_dev + (size_t)b0 * B * vs::kDim;
        const size_t n = (size_t)nb * B, words = 2 * n * k;
        int32_t* lists = o->sl_lists[lane];
        if (c) {
            HIPCHK(hipStreamWaitEvent(st, c->ev_probe[lane], 0));
            if (c->coll_used[lane]) HIPCHK(hipStreamWaitEvent(st, c->ev_coll[lane], 0));  // group g - 2's merge has read the lists
        }
        for (size_t i = 0; i < S.hs.size(); ++i) {
            int32_t* loc = lists + (S.first + i) * words;
            if (rank_ms) HIPCHK(hipEventRecord(ev[4 * i + 2], st));
            if (int r2 = ivf_shard_back(S.hs[i], lane, q, nb, sbb, B, k, nprobe, o->sl_blk[lane], reinterpret_cast<float*>(loc), loc + n * k, st))
                return r2;
            if (rank_ms) HIPCHK(hipEventRecord(ev[4 * i + 3], st));
        }
        if (c) {
            HIPCHK(hipEventRecord(c->ev_scan[lane], st));
            HIPCHK(hipStreamWaitEvent(sc, c->ev_scan[lane], 0));
        }
        if (int r2 = S.exchange(lists, words, sc)) return r2;
        vs::MergeParams m{};
        m.part_d = reinterpret_cast<const float*>(lists);
        m.part_i = lists + n * k;
        m.G = G;
        m.kin = k;
        m.nq = (int)n;
        m.kout = k;
        m.out_d = dists + (size_t)b0 * B * k;
        m.out_i = ids + (size_t)b0 * B * k;
        HIPCHK(vs::launch_merge_layout(m, (int64_t)words, k, sc));
        if (c) {
            HIPCHK(hipEventRecord(c->ev_coll[lane], sc));
            c->coll_used[lane] = true;
        }
        if (rank_ms) {
            HIPCHK(hipStreamSynchronize(st));
            for (size_t i = 0; i < S.hs.size(); ++i) {
                float a = 0, b = 0;
                HIPCHK(hipEventElapsedTime(&a, ev[4 * i], ev[4 * i + 1]));
                HIPCHK(hipEventElapsedTime(&b, ev[4 * i + 2], ev[4 * i + 3]));
                rank_ms[S.first + i] += a + b;
            }
        }
        return VS_OK;
    };
    const int n_groups = (n_batches + gb - 1) / gb, lag = c ? 1 : 0;
    for (int g = 0; g < n_groups + lag; ++g) {
        if (g < n_groups && (rc = front(g))) return rc;
        if (g >= lag && (rc = back(g - lag))) return rc;
    }
    // the caller's stream continues after the last two groups' merges
    if (c)
        for (int lane = 0; lane < 2; ++lane)
            if (c->coll_used[lane]) HIPCHK(hipStreamWaitEvent(st, c->ev_coll[lane], 0));
    return VS_OK;
}

}  // namespace

extern "C" {

int vs_comm_unique_id(void* id_out) {
    if (!id_out) {
        set_error("vs_comm_unique_id: id_out is NULL");
        return VS_ERR_INVALID;
    }
    int rc = rccl_ready();
    if (rc) return rc;
    ncclUniqueId id;
    NCCLCHK(rccl().GetUniqueId(&id));
    static_assert(sizeof(id) == VS_COMM_ID_BYTES, "ncclUniqueId size");
    std::memcpy(id_out, &id, sizeof(id));
    return VS_OK;
}

int vs_comm_create(const void* unique_id, int rank, int world, int device, vs_comm** out) {
    if (!out || !unique_id || world < 1 || rank < 0 || rank >= world) {
        set_error("vs_comm_create: bad arguments");
        return VS_ERR_INVALID;
    }
    int rc = check_device(device);
    if (rc) return rc;
    if ((rc = rccl_ready())) return rc;
    HIPCHK(hipSetDevice(device));
    vs_comm* c = new (std::nothrow) vs_comm();
    if (!c) {
        set_error("out of host memory");
        return VS_ERR_NOMEM;
    }
    c->rank = rank;
    c->world = world;
    c->device = device;
    ncclUniqueId id;
    std::memcpy(&id, unique_id, sizeof(id));
    ncclResult_t r = rccl().CommInitRank(&c->comm, world, id, rank);
    if (r != ncclSuccess) {
        set_error(std::string("ncclCommInitRank: ") + rccl().GetErrorString(r));
        delete c;
        return VS_ERR_DEVICE;
    }
    rc = c->s_coll.create();
    for (int i = 0; i < 2 && !rc; ++i)
        if (!(rc = c->ev_scan[i].create()) && !(rc = c->ev_coll[i].create()) && !(rc = c->ev_front[i].create())) rc = c->ev_probe[i].create();
    if (rc) {
        vs_comm_destroy(c);
        return rc;
    }
    *out = c;
    return VS_OK;
}

int vs_comm_rank(const vs_comm* c) { return c ? c->rank : -1; }
int vs_comm_world(const vs_comm* c) { return c ? c->world : 0; }

void vs_comm_destroy(vs_comm* c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    if (c->s_coll) (void)hipStreamSynchronize(c->s_coll);
    if (c->comm && rccl().lib) (void)rccl().CommDestroy(c->comm);
    delete c;
}

int vs_bf_search_dev_sharded(vs_index* h, vs_comm* c, const float* queries_dev, int n_batches, int B, int k, int32_t* ids_dev,
                             float* dists_dev, int32_t* flags_dev, void* stream) {
    if (!h || !c || h->kind != 0 || !queries_dev || !ids_dev || !dists_dev || n_batches < 1 || B < 1 || B > vs::kMaxBatch || k < 1) {
        set_error("vs_bf_search_dev_sharded: bad arguments");
        return VS_ERR_INVALID;
    }
    if (refuse_general(h, "vs_bf_search_dev_sharded")) return VS_ERR_UNSUPPORTED;
    int rc = set_device(h);
    if (rc) return rc;
    const int k1 = k + 1;
    if (!pick_kcap(k1)) {
        set_error("k too large for the compiled scan kernels (k <= 15)");
        return VS_ERR_UNSUPPORTED;
    }
    hipStream_t user = static_cast<hipStream_t>(stream);
    if ((rc = order_begin(h, user))) return rc;
    if (!flags_dev && n_batches <= kMaxMulti) flags_dev = h->d_flags;  // (the shards' flags travel whenever there is room to merge them)
    rc = sharded_groups(h, c, n_batches, B, k1, k1, ids_dev, dists_dev, flags_dev, nullptr, user,
                        [&](int b0, int nb, float* loc_d, int32_t* loc_i, int32_t* loc_f, hipStream_t s) {
                            return bf_launch(h, h->lane[0], queries_dev + (size_t)b0 * B * vs::kDim, nb, B, k1, loc_d, loc_i, loc_f, s);
                        });
    return rc ? rc : order_end(h, user);
}

int vs_ivf_search_dev_sharded(vs_index* h, vs_comm* c, const float* queries_dev, int n_batches, int B, int k, int nprobe,
                              int32_t* ids_dev, float* dists_dev, void* stream) {
    if (refuse_general_bf(h, "vs_ivf_search_dev_sharded") || refuse_general_ivf(h, "vs_ivf_search_dev_sharded")) return VS_ERR_UNSUPPORTED;
    if (!h || !c || h->kind != 1 || !queries_dev || !ids_dev || !dists_dev || n_batches < 1 || B < 1 || B > vs::kMaxBatch || k < 1 ||
        nprobe < 1) {
        set_error("vs_ivf_search_dev_sharded: bad arguments");
        return VS_ERR_INVALID;
    }
    nprobe = std::min(nprobe, h->nlist);  // IVFIndex.cpp:647
    if (nprobe > kMaxNprobe || !pick_kcap(k)) {
        set_error("nprobe > 256 or k > 16 not supported");
        return VS_ERR_UNSUPPORTED;
    }
    if (h->world != c->world || h->rank != c->rank) {
        set_error("the index was sharded for a different (rank, world) than the communicator's");
        return VS_ERR_INVALID;
    }
    if (h->device != c->device) {
        set_error("index and communicator live on different devices");
        return VS_ERR_INVALID;
    }
    int rc = set_device(h);
    if (rc) return rc;
    hipStream_t user = static_cast<hipStream_t>(stream);
    if ((rc = order_begin(h, user))) return rc;
    // The per-query stages can be cut by slice only where EVERY rank runs the wide pipeline (a rank without resident
    // rows, or nlist > 4096, takes the query-major fallback): that is a property of the index, the same on all ranks,
    // except for empty shards -- which only occur with fewer lists than ranks.
    const bool sliced = c->world > 1 && c->world <= kIvfShardMaxWorld && h->nlist <= vs::kIvfFastNlist && h->nlist >= c->world;
    if (!sliced) {
        // every rank runs the whole pipeline on its own lists, one all-gather of top-k lists per launch group
        rc = sharded_groups(h, c, n_batches, B, k, k, ids_dev, dists_dev, nullptr, nullptr, user,
                            [&](int b0, int nb, float* loc_d, int32_t* loc_i, int32_t*, hipStream_t s) -> int {
                                return ivf_multi_dev(h, queries_dev + (size_t)b0 * B * vs::kDim, nb, B, k, nprobe, loc_d, loc_i, s);
                            });
        return rc ? rc : order_end(h, user);
    }
    Shards S;
    S.hs = {h};
    S.G = c->world;
    S.first = c->rank;
    S.c = c;
    rc = ivf_sliced_groups(S, queries_dev, n_batches, B, k, nprobe, ids_dev, dists_dev, nullptr, user);
    return rc ? rc : order_end(h, user);
}

// Virtual ranks: the cluster-sharded pipeline of vs_ivf_search_dev_sharded for G shards that live on ONE device, driven by
// one thread, the two collectives replaced by writing every rank's block / top-k lists straight into the gathered
// layout.  For tests (the sliced pipeline must reproduce the unsharded result) and for measuring what a rank of a G-way
// job does per launch group on a single GPU: rank_ms[r] (optional) = device time of rank r's front + back halves.
int vs_ivf_search_dev_vshards(vs_index* const* shards, int G, const float* queries_dev, int n_batches, int B, int k, int nprobe,
                              int32_t* ids_dev, float* dists_dev, double* rank_ms, void* stream) {
    if (!shards || G < 2 || G > kIvfShardMaxWorld || !queries_dev || !ids_dev || !dists_dev || n_batches < 1 || B < 1 || B > vs::kMaxBatch || k < 1 ||
        nprobe < 1) {
        set_error("vs_ivf_search_dev_vshards: bad arguments");
        return VS_ERR_INVALID;
    }
    for (int r = 0; r < G; ++r)
        if (shards[r] && (refuse_general_bf(shards[r], "vs_ivf_search_dev_vshards") || refuse_general_ivf(shards[r], "vs_ivf_search_dev_vshards")))
            return VS_ERR_UNSUPPORTED;
    for (int r = 0; r < G; ++r)
        if (!shards[r] || shards[r]->kind != 1 || shards[r]->world != G || shards[r]->rank != r || shards[r]->device != shards[0]->device ||
            shards[r]->nlist != shards[0]->nlist || !ivf_wide_ok(shards[r], k)) {
            set_error("vs_ivf_search_dev_vshards: shard r must be an IVF index created with (rank r, world G) on one device, rows resident, nlist <= 4096");
            return VS_ERR_INVALID;
        }
    vs_index* h0 = shards[0];
    nprobe = std::min(nprobe, h0->nlist);
    if (nprobe > kMaxNprobe || !pick_kcap(k)) {
        set_error("nprobe > 256 or k > 16 not supported");
        return VS_ERR_UNSUPPORTED;
    }
    return guarded([&]() -> int {
        int rc = set_device(h0);
        if (rc) return rc;
        hipStream_t s = static_cast<hipStream_t>(stream);
        for (int r = 0; r < G; ++r)
            if ((rc = order_begin(shards[r], s))) return rc;
        Shards S;
        S.hs.assign(shards, shards + G);
        S.G = G;
        return ivf_sliced_groups(S, queries_dev, n_batches, B, k, nprobe, ids_dev, dists_dev, rank_ms, s);
    });
}

}  // extern "C"

namespace {

// ---- brute force on host buffers, the reference's answer out (cpu_baseline.cpp:127-153 tie order included), over the row
// shards of a Shards.

constexpr size_t kShPackWords = 32 + (size_t)2 * 32 * kTieCap;  // filter output of one shard: cnt [32] | rows [32][kTieCap] | dists [32][kTieCap]

// gathered scratch of the owner, [G] parts per region: meta [G][2] (rows, id_offset) | lists [G][lists_words] (sharded calls:
// each shard's dists | ids | flags of one launch step) | the tie resolver's tau [G][32] | dense [G][32 * L0p] |
// pack [G][kShPackWords] | row [G][ldm] (one query's full distance row).  The search reserves meta and lists, the resolver
// meta and its own regions (L0p > 0); nothing in the buffer outlives either.
struct ShBuf {
    int32_t *meta, *lists, *tau, *dense, *pack, *row;
};
int sh_reserve(vs_index* o, int G, size_t lists_words, int64_t L0p, int64_t ldm, ShBuf& B) {
    const size_t tie = L0p ? 32 + (size_t)32 * L0p + kShPackWords + (size_t)ldm : 0;
    const size_t total = (size_t)G * (2 + lists_words + tie);
    if (o->d_sh.size() < total) HIPCHK(hipDeviceSynchronize());
    if (int rc = o->d_sh.reserve(total)) return rc;
    B.meta = o->d_sh;
    B.lists = B.meta + (size_t)G * 2;
    B.tau = B.lists + (size_t)G * lists_words;
    B.dense = B.tau + (size_t)G * 32;
    B.pack = B.dense + (size_t)G * 32 * L0p;
    B.row = B.pack + (size_t)G * kShPackWords;
    return VS_OK;
}

// Exact select_topk (cpu_baseline.cpp:127-153) for the queries whose k+1 best distances contain a tie.  The slot replay
// only depends on rows that change the k-slot buffer, i.e. rows whose distance is below the buffer maximum when they
// arrive -- and that maximum never rises.  So: the first L0 rows of shard 0 are taken densely (their distance rows), the
// k-th smallest of them bounds the buffer maximum for every later row of every shard, each shard emits its rows under that
// bound in ONE filtered pass (about N * k / L0 of them), and the host replays "dense rows, then the shards' candidates in row
// order".  Exact whenever the distances are: the replay compares the scan kernels' own fp32 numbers, whatever their sign, so
// it is as exact on real-valued rows as on integer-valued SIFT.  Both are tested: integer ties throughout the suite,
// bit-equal noise distances (negative ones and +0 included) of duplicate real-valued rows by tests/test_gpu_cancel.py.
int resolve_ties_shards(const Shards& S, const std::vector<int32_t>& meta /*[G][2] rows, id_offset*/, const float* queries_host,
                        const std::vector<int64_t>& flagged, int k, int32_t* ids, float* dists) {
    vs_index* o = S.owner();
    hipStream_t st = S.s();
    const int G = S.G;
    for (int g = 1; g < G; ++g)
        if ((int64_t)meta[2 * g + 1] != (int64_t)meta[2 * (g - 1) + 1] + meta[2 * (g - 1)]) {
            set_error("sharded tie order needs shards that are contiguous row ranges in rank order");
            return VS_ERR_UNSUPPORTED;
        }
    // k >= 16 (one index: the sharded calls take k <= 15): a prefix that grows with k (512 k rows, a multiple of 4096), so
    // that about n_rows / 512 rows pass the bound whatever k is (the k <= 15 prefix of kTieDense rows would let
    // n_rows * k / 4096 through, past kTieCap at 1 M rows)
    const int64_t L0 = std::min<int64_t>(meta[0], k <= 15 ? kTieDense : ((int64_t)512 * k + 4095) & ~int64_t(4095));
    const int64_t L0p = (L0 + 15) & ~int64_t(15);
    int64_t ldm = 0, total = 0;
    for (int g = 0; g < G; ++g) {
        ldm = std::max<int64_t>(ldm, ((int64_t)meta[2 * g] + 15) & ~int64_t(15));
        total += meta[2 * g];
    }
    ShBuf Bf{};
    int rc;
    if ((rc = sh_reserve(o, G, 0, L0p, ldm, Bf))) return rc;
    // downloads land in pinned memory (pageable destinations are staged by the runtime: several times slower):
    // dense [32][L0p] f32 | cnt [G][32] | rows [G][32][mx] | dists [G][32][mx], mx <= kTieCap
    if ((rc = o->pin_sh.reserve(((size_t)32 * L0p + (size_t)G * 32 * (1 + 2 * (size_t)kTieCap)) * sizeof(float)))) return rc;
    float* const dense = reinterpret_cast<float*>(o->pin_sh.get());
    int32_t* const cnt = reinterpret_cast<int32_t*>(dense + (size_t)32 * L0p);
    int32_t* const cr = cnt + (size_t)G * 32;
    float* const cd = reinterpret_cast<float*>(cr + (size_t)G * 32 * kTieCap);
    float* const tau0 = reinterpret_cast<float*>(Bf.tau);      // shard 0's part: the bound every shard filters with
    float* const dense0 = reinterpret_cast<float*>(Bf.dense);  // shard 0's part: [B][L0p]
    const size_t qd = (size_t)o->dim;  // floats per query in the caller's buffer and in d_q
    std::vector<float> qbuf((size_t)32 * qd), row;
    for (size_t f0 = 0; f0 < flagged.size(); f0 += 32) {
        const int B = (int)std::min<size_t>(32, flagged.size() - f0);
        for (int b = 0; b < B; ++b)
            std::memcpy(&qbuf[(size_t)b * qd], queries_host + flagged[f0 + b] * qd, qd * sizeof(float));
        HIPCHK(hipMemcpyAsync(o->d_q, qbuf.data(), (size_t)B * qd * sizeof(float), hipMemcpyHostToDevice, st));
        if (S.first == 0) {
            vs_index* h0 = S.hs[0];
            if ((rc = scores_dev(h0, h0->d_vecs, h0->d_norm, L0, o->d_q, B, dense0, L0p, st))) return rc;
            if (total > L0) {  // rows follow the prefix: bound = next_up(k-th smallest of the dense rows)
                HIPCHK(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(tau0), 0xff800000u, 32, st));  // -inf: padding queries emit nothing
                if (k <= 15) {  // merge kernel over G = L0 one-entry lists
                    vs::MergeParams m{};
                    m.part_d = dense0;
                    m.G = (int)L0;
                    m.kin = 1;
                    m.nq = B;
                    m.kout = k;
                    m.tau_out = tau0;
                    HIPCHK(vs::launch_merge_layout(m, 1, L0p, st));
                } else {  // (vs_bf_search_topk: the wide-k scratch exists)
                    vs::TopkWideParams t{};
                    t.dense = dense0;
                    t.dense_ld = L0p;
                    t.n_dense = L0;
                    t.nq = B;
                    t.k1 = k;
                    t.out_d = h0->topw.pre_d;
                    t.out_i = h0->topw.pre_i;
                    t.out_ld = vs::kTopkWideMax;
                    t.tau_out = tau0;
                    HIPCHK(vs::launch_topk_wide(t, 32, st));
                }
            }
        }
        if ((rc = S.exchange(Bf.tau, 32, st)) || (rc = S.exchange(Bf.dense, (size_t)32 * L0p, st))) return rc;
        for (size_t i = 0; i < S.hs.size(); ++i) {
            vs_index* h = S.hs[i];
            const int g = S.first + (int)i;
            int32_t* pk = Bf.pack + (size_t)g * kShPackWords;
            HIPCHK(hipMemsetAsync(pk, 0, 32 * sizeof(int32_t), st));
            const int64_t rb = g == 0 ? L0 : 0;
            if (h->n_rows <= rb) continue;
            vs::ScanParams p{};
            p.base = h->d_vecs;
            p.bnorm = h->d_norm;
            p.q = o->d_q;
            p.n_batches = 1;
            p.metric = h->metric;
            p.nq_valid = B;
            p.k1 = k + 1;
            p.tau0 = tau0;
            p.row_begin = rb;  // a multiple of 16 (kTieDense, 4096) where rows follow
            p.row_end = h->n_rows;
            p.f_cnt = pk;
            p.f_row = pk + 32;
            p.f_d = reinterpret_cast<float*>(pk + 32 + (size_t)32 * kTieCap);
            p.f_cap = kTieCap;
            int grid, tp;
            scan_geometry(h->n_rows - rb, h->num_cus, grid, tp);
            p.tiles_per_wg = tp;
            HIPCHK(scan_any(h, p, grid, 8, 2, vs::kModeFilter, st));
        }
        if ((rc = S.exchange(Bf.pack, kShPackWords, st))) return rc;
        HIPCHK(hipMemcpyAsync(dense, dense0, (size_t)B * L0p * sizeof(float), hipMemcpyDeviceToHost, st));
        HIPCHK(hipMemcpy2DAsync(cnt, 32 * 4, Bf.pack, kShPackWords * 4, 32 * 4, G, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        int mx = 0;
        std::vector<int> overflow;  // more than kTieCap candidates on a shard: the full-row fallback below
        for (int b = 0; b < B; ++b) {
            bool ov = false;
            for (int g = 0; g < G; ++g) {
                const int cg = cnt[(size_t)g * 32 + b];
                if (cg > kTieCap) ov = true;
                else mx = std::max(mx, cg);
            }
            if (ov) overflow.push_back(b);
        }
        if (mx > 0) {
            for (int g = 0; g < G; ++g) {
                const int32_t* pk = Bf.pack + (size_t)g * kShPackWords;
                HIPCHK(hipMemcpy2DAsync(cr + (size_t)g * 32 * mx, (size_t)mx * 4, pk + 32, (size_t)kTieCap * 4, (size_t)mx * 4, B,
                                        hipMemcpyDeviceToHost, st));
                HIPCHK(hipMemcpy2DAsync(cd + (size_t)g * 32 * mx, (size_t)mx * 4, pk + 32 + (size_t)32 * kTieCap, (size_t)kTieCap * 4,
                                        (size_t)mx * 4, B, hipMemcpyDeviceToHost, st));
            }
            HIPCHK(hipStreamSynchronize(st));
        }
        // the flagged queries are independent: their replays run on a few host threads (a replay walks ~5000 entries)
        auto replay = [&](int b_begin, int b_end) {
            std::vector<int32_t> srow, order;
            std::vector<float> sdist;
            for (int b = b_begin; b < b_end; ++b) {
                if (std::find(overflow.begin(), overflow.end(), b) != overflow.end()) continue;
                int64_t n = L0;
                for (int g = 0; g < G; ++g) n += cnt[(size_t)g * 32 + b];
                srow.resize((size_t)n);
                sdist.resize((size_t)n);
                for (int64_t j = 0; j < L0; ++j) {
                    srow[(size_t)j] = (int32_t)(j + meta[1]);
                    sdist[(size_t)j] = dense[(size_t)b * L0p + j];
                }
                int64_t at = L0;
                for (int g = 0; g < G; ++g) {
                    const int m = cnt[(size_t)g * 32 + b];
                    const int32_t* rr = cr + ((size_t)g * 32 + b) * mx;
                    const float* dd = cd + ((size_t)g * 32 + b) * mx;
                    order.resize((size_t)m);
                    std::iota(order.begin(), order.end(), 0);
                    std::sort(order.begin(), order.end(), [&](int32_t x, int32_t y) { return rr[x] < rr[y]; });
                    for (int j = 0; j < m; ++j, ++at) {
                        srow[(size_t)at] = rr[order[(size_t)j]] + meta[2 * g + 1];
                        sdist[(size_t)at] = dd[order[(size_t)j]];
                    }
                }
                const int64_t qi = flagged[f0 + b];
                vs::select_topk_slots_sparse(srow.data(), sdist.data(), n, k, ids + qi * k, dists + qi * k);
            }
        };
        const int n_thr = std::min(4, B / 4);
        if (n_thr <= 1) {
            replay(0, B);
        } else {
            std::vector<std::thread> pool;
            std::atomic<bool> failed{false};
            for (int t = 0; t < n_thr; ++t)
                pool.emplace_back([&, t]() {
                    try {
                        replay(B * t / n_thr, B * (t + 1) / n_thr);
                    } catch (...) {
                        failed = true;
                    }
                });
            for (auto& th : pool) th.join();
            if (failed) {
                set_error("out of host memory");
                return VS_ERR_NOMEM;
            }
        }
        // masses of rows under the bound (duplicates): the query's full distance row, shard after shard, replayed densely
        for (int b : overflow) {
            for (size_t i = 0; i < S.hs.size(); ++i) {
                vs_index* h = S.hs[i];
                const int g = S.first + (int)i;
                if ((rc = scores_dev(h, h->d_vecs, h->d_norm, h->n_rows, o->d_q + (size_t)b * qd, 1,
                                     reinterpret_cast<float*>(Bf.row + (size_t)g * ldm), ldm, st)))
                    return rc;
            }
            if ((rc = S.exchange(Bf.row, (size_t)ldm, st))) return rc;
            row.resize((size_t)total);
            int64_t at = 0;
            for (int g = 0; g < G; ++g) {
                HIPCHK(hipMemcpyAsync(row.data() + at, Bf.row + (size_t)g * ldm, (size_t)meta[2 * g] * sizeof(float), hipMemcpyDeviceToHost, st));
                at += meta[2 * g];
            }
            HIPCHK(hipStreamSynchronize(st));
            const int64_t qi = flagged[f0 + b];
            vs::select_topk_slots_dense(row.data(), total, k, meta[1], ids + qi * k, dists + qi * k);
        }
    }
    return VS_OK;
}

int bf_search_shards(const Shards& S, const float* queries_host, int64_t nq, int k, int32_t* ids, float* dists, vs_timing* timing) {
    vs_index* o = S.owner();
    hipStream_t st = S.s();
    const int G = S.G;
    const double t_start = now_ms();
    vs_timing tm{};
    const int k1 = k + 1;
    if (S.merge && !pick_kcap(k1)) {
        set_error("k too large for the compiled scan kernels (k <= 15)");
        return VS_ERR_UNSUPPORTED;
    }
    int rc;
    if ((rc = ensure_pipe(o))) return rc;
    settle_slots(o->pipe, {st, o->s_h2d, o->s_d2h});
    ShBuf Bf{};
    if ((rc = sh_reserve(o, G, S.merge ? (size_t)(2 * k1 + 1) * kMaxMulti * 32 : 0, 0, 0, Bf))) return rc;
    if (k1 > kKcapMax && (rc = ensure_topw(o))) return rc;
    // every process needs every shard's (rows, id_offset)
    std::vector<int32_t> meta((size_t)2 * G, 0);
    for (size_t i = 0; i < S.hs.size(); ++i) {
        meta[2 * (S.first + i)] = (int32_t)S.hs[i]->n_rows;
        meta[2 * (S.first + i) + 1] = (int32_t)S.hs[i]->id_offset;
    }
    if (S.c && S.c->world > 1) {
        HIPCHK(hipMemcpyAsync(Bf.meta + 2 * S.first, &meta[2 * S.first], 2 * sizeof(int32_t), hipMemcpyHostToDevice, st));
        if ((rc = S.exchange(Bf.meta, 2, st))) return rc;
        HIPCHK(hipMemcpyAsync(meta.data(), Bf.meta, meta.size() * sizeof(int32_t), hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
    }
    // the launch step: nb batches of B queries at q -> [nb * B][k1] lists by (dist, id) + flags, on st
    auto step = [&](const float* q, int nb, int B, float* out_d, int32_t* out_i, int32_t* flags, bool force_f32) -> int {
        if (k1 > kKcapMax) return topw_launch(o, q, nb, B, k1, out_d, out_i, flags, st);
        if (!S.merge) return bf_launch(o, o->lane[0], q, nb, B, k1, out_d, out_i, flags, st, force_f32);
        // the lists of every shard driven here, the exchange, the merge
        const size_t np = (size_t)nb * B, words = 2 * np * k1 + np;
        for (size_t i = 0; i < S.hs.size(); ++i) {
            int32_t* loc = Bf.lists + (S.first + i) * words;
            int r2 = bf_launch(S.hs[i], S.hs[i]->lane[0], q, nb, B, k1, reinterpret_cast<float*>(loc), loc + np * k1, loc + 2 * np * k1,
                               st, force_f32);
            if (r2) return r2;
        }
        if (int r2 = S.exchange(Bf.lists, words, st)) return r2;
        vs::MergeParams m{};
        m.part_d = reinterpret_cast<const float*>(Bf.lists);
        m.part_i = Bf.lists + np * k1;
        m.G = G;
        m.kin = k1;
        m.nq = (int)np;
        m.kout = k1;
        m.out_d = out_d;
        m.out_i = out_i;
        m.flags = flags;
        m.flag_empty = 1;
        m.shard_flags = Bf.lists + 2 * np * k1;
        m.shard_flags_stride = (int64_t)words;
        HIPCHK(vs::launch_merge_layout(m, (int64_t)words, k1, st));
        return VS_OK;
    };
    // Queries go through in chunks of kMaxMulti batches: the full batches in one launch step, a ragged tail batch in another
    // (the harness loop of main.cpp:201-251 collapsed into a call).  Two chunks are in flight: uploads and downloads run on
    // copy streams beside the other chunk's kernels.
    const int batch = o->batch;
    const int64_t chunk = (int64_t)kMaxMulti * batch;
    const float inf = std::numeric_limits<float>::infinity();
    std::vector<int64_t> flagged;
    auto launch_chunk = [&](vs_index::PipeSlot& P, bool force_f32) -> int {
        const int full = (int)(P.n / batch), rem = (int)(P.n % batch);
        int r2 = VS_OK;
        if (full) r2 = step(P.d_q, full, batch, P.d_out_d, P.d_out_i, P.d_flags, force_f32);
        if (!r2 && rem) {
            const size_t o0 = (size_t)full * batch;
            r2 = step(P.d_q + o0 * (size_t)o->dim, 1, rem, P.d_out_d + o0 * k1, P.d_out_i + o0 * k1, P.d_flags + o0, force_f32);
        }
        return r2;
    };
    auto download = [&](vs_index::PipeSlot& P, hipStream_t s) -> int {
        float* hd = reinterpret_cast<float*>(P.pin_out.get());
        int32_t* hi = reinterpret_cast<int32_t*>(P.pin_out.get()) + (size_t)chunk * k1;
        int32_t* hf = hi + (size_t)chunk * k1;
        HIPCHK(hipMemcpyAsync(hd, P.d_out_d, (size_t)P.n * k1 * sizeof(float), hipMemcpyDeviceToHost, s));
        HIPCHK(hipMemcpyAsync(hi, P.d_out_i, (size_t)P.n * k1 * sizeof(int32_t), hipMemcpyDeviceToHost, s));
        HIPCHK(hipMemcpyAsync(hf, P.d_flags, (size_t)P.n * sizeof(int32_t), hipMemcpyDeviceToHost, s));
        return VS_OK;
    };
    auto enqueue = [&](vs_index::PipeSlot& P, int64_t q0, int64_t n) -> int {
        const double t0 = now_ms();
        P.q0 = q0;
        P.n = n;
        std::memcpy(P.pin_q, queries_host + q0 * o->dim, (size_t)n * o->dim * sizeof(float));
        HIPCHK(hipMemcpyAsync(P.d_q, P.pin_q, (size_t)n * o->dim * sizeof(float), hipMemcpyHostToDevice, o->s_h2d));
        HIPCHK(hipEventRecord(P.ev_h2d, o->s_h2d));
        tm.h2d_ms += now_ms() - t0;
        HIPCHK(hipStreamWaitEvent(st, P.ev_h2d, 0));
        int r2 = launch_chunk(P, false);
        if (r2) return r2;
        HIPCHK(hipEventRecord(P.ev_comp, st));
        HIPCHK(hipStreamWaitEvent(o->s_d2h, P.ev_comp, 0));
        if ((r2 = download(P, o->s_d2h))) return r2;
        HIPCHK(hipEventRecord(P.ev_d2h, o->s_d2h));
        return VS_OK;
    };
    auto retire = [&](vs_index::PipeSlot& P) -> int {
        if (P.q0 < 0) return VS_OK;
        const double t0 = now_ms();
        HIPCHK(hipEventSynchronize(P.ev_d2h));
        const float* hd = reinterpret_cast<const float*>(P.pin_out.get());
        const int32_t* hi = reinterpret_cast<const int32_t*>(P.pin_out.get()) + (size_t)chunk * k1;
        const int32_t* hf = hi + (size_t)chunk * k1;
        bool rerun = false;
        for (int64_t b = 0; b < P.n; ++b) rerun = rerun || hf[(size_t)b] == 2;
        // Flag 2: an int8 scan skipped a batch of this chunk (a query that is not an integer in [0, 255]) -> the chunk again
        // on the fp32 rows.  Sharded calls issue every collective in the same order on every rank: the chunks' exchanges,
        // a rerun's (decided here from the merged flags, which every rank holds alike; enqueued behind the next chunk), then
        // the tie resolver's.
        if (rerun) {
            int r2 = launch_chunk(P, true);
            if (r2) return r2;
            if ((r2 = download(P, st))) return r2;
            HIPCHK(hipStreamSynchronize(st));
        }
        tm.d2h_ms += now_ms() - t0;
        // k of the k1 entries (+inf: no row; inner product: the score q.v); flag 1: equal distances among the k1
        for (int64_t b = 0; b < P.n; ++b) {
            for (int t = 0; t < k; ++t) {
                const int32_t id = hi[(size_t)b * k1 + t];
                ids[(P.q0 + b) * k + t] = id;
                float d = id >= 0 ? hd[(size_t)b * k1 + t] : inf;
                if (o->metric == VS_METRIC_IP && id >= 0) d = -d;
                dists[(P.q0 + b) * k + t] = d;
            }
            if (hf[(size_t)b] == 1) flagged.push_back(P.q0 + b);
        }
        P.q0 = -1;
        return VS_OK;
    };
    int c = 0;
    for (int64_t q0 = 0; q0 < nq; q0 += chunk, ++c) {
        vs_index::PipeSlot& P = o->pipe[c & 1];
        if ((rc = retire(P))) return rc;
        if ((rc = enqueue(P, q0, std::min<int64_t>(chunk, nq - q0)))) return rc;
    }
    if ((rc = retire(o->pipe[c & 1]))) return rc;  // the older chunk first
    if ((rc = retire(o->pipe[(c + 1) & 1]))) return rc;
    tm.fine_search_ms = now_ms() - t_start;
    // ties inside the k+1 best: the reference's order is history dependent -> replay select_topk over the rows that can
    // change its buffer
    if (!flagged.empty() && o->metric == VS_METRIC_L2) {
        const double t0 = now_ms();
        if ((rc = resolve_ties_shards(S, meta, queries_host, flagged, k, ids, dists))) return rc;
        tm.tie_resolve_ms = now_ms() - t0;
        tm.tie_queries = (int64_t)flagged.size();
    }
    tm.total_ms = now_ms() - t_start;
    if (timing) *timing = tm;
    return VS_OK;
}

// ---- IVF on host buffers (vs_ivf_search; vs_ivf_search_sharded: c = the communicator).  Queries go through in chunks (the
// harness loop of main_ivf.cpp:150-214 collapsed into a call): a chunk is ONE upload, its launch step, ONE download -- the
// host, not the device, is the limit of this call (a hipMemcpyAsync costs about as much host time as a launch group's five
// launches).  Two chunks in flight; at least two chunks per call where there is enough work, so that the second upload runs
// beside the first chunk's kernels.  The launch step deals the chunk's launch groups to the two lanes' streams, a ragged
// tail batch in a group of its own; sharded, it is the device-sharded search on the index's stream, for the chunk's full
// batches and then for its ragged tail.  The chunks depend on nq, batch, ivf_gb and ivf_host_cap only: every rank issues
// the same collectives in the same order.
int ivf_search_host(vs_index* h, vs_comm* c, const float* queries_host, int64_t nq, int k, int nprobe, int32_t* ids, float* dists,
                    int64_t* total_candidates, vs_timing* timing) {
    int rc = set_device(h);
    if (rc) return rc;
    const double t_start = now_ms();
    vs_timing tm{};
    if ((rc = ensure_pipe(h)) || (rc = ensure_wide_streams(h)) || (rc = ensure_ivf_host(h, k)) || (rc = order_begin(h, h->stream))) return rc;
    settle_slots(h->ihs, {h->stream, h->wide_stream[0], h->wide_stream[1], h->s_h2d, h->s_d2h, c ? c->s_coll : h->stream});
    h->stage_on = !c;  // (the sharded call has no stage split)
    h->stage_used = 0;
    HIPCHK(hipMemsetAsync(h->d_cand, 0, sizeof(unsigned long long), h->stream));
    const float inf = std::numeric_limits<float>::infinity();
    const bool wide = !h->general && ivf_wide_ok(h, k);
    HIPCHK(hipEventRecord(h->wide_fork, h->stream));  // (behind the memset above)
    for (int i = 0; i < 2; ++i) HIPCHK(hipStreamWaitEvent(h->wide_stream[i], h->wide_fork, 0));
    const int64_t unit_q = (int64_t)vs::kIvfWideBatches * h->batch;  // a super-batch of queries: chunks are cut at these
    const int64_t cap_q = h->ivf_host_cap / unit_q * unit_q;
    const int64_t wchunk = std::min<int64_t>(cap_q, std::max<int64_t>(unit_q, (nq / 2 + unit_q - 1) / unit_q * unit_q));
    const int64_t group_q = c ? wchunk : (int64_t)h->ivf_gb * h->batch;  // queries per launch step
    auto lane_stream = [&](int lane) -> hipStream_t { return c ? static_cast<hipStream_t>(h->stream) : static_cast<hipStream_t>(h->wide_stream[lane]); };
    int next_lane = 0;
    auto enqueue = [&](vs_index::IvfHostSlot& S, int64_t q0, int64_t n) -> int {
        const double t0 = now_ms();
        S.q0 = q0;
        S.n = n;
        std::memcpy(S.pin_q, queries_host + q0 * h->dim, (size_t)n * h->dim * sizeof(float));
        HIPCHK(hipMemcpyAsync(S.d_q, S.pin_q, (size_t)n * h->dim * sizeof(float), hipMemcpyHostToDevice, h->s_h2d));
        HIPCHK(hipEventRecord(S.ev_h2d, h->s_h2d));
        tm.h2d_ms += now_ms() - t0;
        float* od = S.d_out;
        int32_t* oi = reinterpret_cast<int32_t*>(S.d_out + (size_t)n * k);
        bool used[2] = {false, false};
        for (int64_t g0 = 0; g0 < n; g0 += group_q) {
            const int64_t gn = std::min<int64_t>(group_q, n - g0);
            const int full = (int)(gn / h->batch), rem = (int)(gn % h->batch);
            const int lane = wide && !c ? next_lane : 0;
            next_lane ^= 1;
            const hipStream_t cs = lane_stream(lane);
            if (!used[lane]) HIPCHK(hipStreamWaitEvent(cs, S.ev_h2d, 0));
            used[lane] = true;
            int r2 = VS_OK;
            auto run = [&](size_t o, int nb, int B) -> int {
                const float* q = S.d_q + o * h->dim;
                if (c) return vs_ivf_search_dev_sharded(h, c, q, nb, B, k, nprobe, oi + o * k, od + o * k, cs);
                if (wide) return ivf_group_wide_dev(h, lane, q, nb, B, k, nprobe, od + o * k, oi + o * k, cs);
                if (h->general) return (k > 16 ? ivf_group_nd_wide_dev : ivf_group_nd_dev)(h, q, nb, B, k, nprobe, od + o * k, oi + o * k, cs);
                int r3 = VS_OK;
                for (int b = 0; b < nb && !r3; ++b)
                    r3 = ivf_fallback_batch_dev(h, q + (size_t)b * B * h->dim, B, k, nprobe, od + (o + (size_t)b * B) * k,
                                                oi + (o + (size_t)b * B) * k, cs);
                return r3;
            };
            if (full) r2 = run((size_t)g0, full, h->batch);
            if (!r2 && rem) r2 = run((size_t)g0 + (size_t)full * h->batch, 1, rem);  // the call's ragged tail
            if (r2) return r2;
        }
        for (int lane = 0; lane < 2; ++lane)
            if (used[lane]) {
                HIPCHK(hipEventRecord(S.ev_comp[lane], lane_stream(lane)));
                HIPCHK(hipStreamWaitEvent(h->s_d2h, S.ev_comp[lane], 0));
            }
        HIPCHK(hipMemcpyAsync(S.pin_out, S.d_out, (size_t)n * k * 2 * sizeof(float), hipMemcpyDeviceToHost, h->s_d2h));
        HIPCHK(hipEventRecord(S.ev_d2h, h->s_d2h));
        return VS_OK;
    };
    auto retire = [&](vs_index::IvfHostSlot& S) -> int {
        if (S.q0 < 0) return VS_OK;
        const double t0 = now_ms();
        HIPCHK(hipEventSynchronize(S.ev_d2h));
        tm.d2h_ms += now_ms() - t0;
        const float* hd = S.pin_out;
        const int32_t* hi = reinterpret_cast<const int32_t*>(S.pin_out + (size_t)S.n * k);
        for (int64_t i = 0; i < S.n * k; ++i) {
            const int32_t id = hi[i];
            ids[S.q0 * k + i] = id;
            dists[S.q0 * k + i] = id >= 0 ? (h->metric == VS_METRIC_IP ? -hd[i] : hd[i]) : inf;  // (IP: the score q.v, as IVFIndex returns it)
        }
        S.q0 = -1;
        return VS_OK;
    };
    int ci = 0;
    for (int64_t q0 = 0; q0 < nq; q0 += wchunk, ++ci) {
        vs_index::IvfHostSlot& S = h->ihs[ci & 1];
        if ((rc = retire(S))) return rc;
        if ((rc = enqueue(S, q0, std::min<int64_t>(wchunk, nq - q0)))) return rc;
    }
    if ((rc = retire(h->ihs[ci & 1]))) return rc;
    if ((rc = retire(h->ihs[(ci + 1) & 1]))) return rc;
    for (int i = 0; i < 2; ++i) {  // the index's stream continues behind the lanes
        HIPCHK(hipEventRecord(h->wide_join[i], h->wide_stream[i]));
        HIPCHK(hipStreamWaitEvent(h->stream, h->wide_join[i], 0));
    }
    unsigned long long cand = 0;  // (sharded: the rows THIS rank scanned, IVFIndex::searchBatch's return value per shard)
    HIPCHK(hipMemcpyAsync(&cand, h->d_cand, sizeof(cand), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    if (total_candidates) *total_candidates = (int64_t)cand;
    tm.total_ms = now_ms() - t_start;
    // SearchTiming split (IVFIndex.h:31-36): device time of the three stages from the events between their launches,
    // summed over the call's launch groups (uploads and downloads overlap them)
    for (int i = 0; i + 3 < h->stage_used; i += 4) {
        float ms[3] = {0, 0, 0};
        for (int j = 0; j < 3; ++j) (void)hipEventElapsedTime(&ms[j], h->stage_ev[i + j], h->stage_ev[i + j + 1]);
        tm.centroid_search_ms += ms[0];
        tm.gather_ms += ms[1];
        tm.fine_search_ms += ms[2];
    }
    if (c) tm.fine_search_ms = tm.total_ms;
    h->stage_on = false;
    h->stage_used = 0;
    if (timing) *timing = tm;
    return order_end(h, h->stream);
}

}  // namespace

extern "C" {

int vs_bf_search(vs_index* h, const float* queries_host, int64_t nq, int k, int32_t* ids, float* dists,
                 vs_timing* timing) {
    if (!h || h->kind != 0 || !queries_host || !ids || !dists || nq < 0 || k < 1) {
        set_error("vs_bf_search: bad arguments");
        return VS_ERR_INVALID;
    }
    return guarded([&]() -> int {
        int rc = set_device(h);
        if (rc) return rc;
        if (!pick_kcap(k + 1)) {
            set_error("k too large for the compiled scan kernels (k <= 15)");
            return VS_ERR_UNSUPPORTED;
        }
        if ((rc = order_begin(h, h->stream))) return rc;
        Shards S;
        S.hs = {h};
        S.merge = false;
        return bf_search_shards(S, queries_host, nq, k, ids, dists, timing);
    });
}

int vs_bf_search_topk(vs_index* h, const float* queries_host, int64_t nq, int k, int32_t* ids, float* dists, vs_timing* timing) {
    if (!h || h->kind != 0 || !queries_host || !ids || !dists || nq < 0 || k < 1) {
        set_error("vs_bf_search_topk: bad arguments");
        return VS_ERR_INVALID;
    }
    if (k > vs::kTopkWideMax - 1) {
        set_error("vs_bf_search_topk: k > 128");
        return VS_ERR_UNSUPPORTED;
    }
    if (k + 1 <= kKcapMax) return vs_bf_search(h, queries_host, nq, k, ids, dists, timing);
    return guarded([&]() -> int {
        int rc = set_device(h);
        if (rc) return rc;
        if (g_topw_stats) g_topw_st = TopwStats{};
        if ((rc = order_begin(h, h->stream))) return rc;
        Shards S;
        S.hs = {h};
        S.merge = false;
        vs_timing tm{};
        if ((rc = bf_search_shards(S, queries_host, nq, k, ids, dists, &tm))) return rc;
        if (timing) *timing = tm;
        if (g_topw_stats)
            fprintf(stderr, "topw_stats k=%d batches=%lld overflowed=%lld queries=%lld cand_mean=%.1f cand_max=%lld flagged=%lld\n", k,
                    (long long)g_topw_st.batches, (long long)g_topw_st.overflowed, (long long)g_topw_st.queries,
                    g_topw_st.queries ? (double)g_topw_st.cand_sum / g_topw_st.queries : 0.0, (long long)g_topw_st.cand_max,
                    (long long)tm.tie_queries);
        return VS_OK;
    });
}

// Host-buffer forms of the sharded searches (what the CLIs call with --gpus N): every rank passes the same queries and
// receives the same result -- for brute force the reference's own (select_topk's tie order, fp32 rerun of batches the
// int8 scan cannot take), like vs_bf_search on one GPU.
int vs_bf_search_sharded(vs_index* h, vs_comm* c, const float* queries_host, int64_t nq, int k, int32_t* ids, float* dists,
                         vs_timing* timing) {
    if (!h || !c || h->kind != 0 || !queries_host || !ids || !dists || nq < 0 || k < 1) {
        set_error("vs_bf_search_sharded: bad arguments");
        return VS_ERR_INVALID;
    }
    if (refuse_general(h, "vs_bf_search_sharded")) return VS_ERR_UNSUPPORTED;
    if (h->device != c->device) {
        set_error("index and communicator live on different devices");
        return VS_ERR_INVALID;
    }
    return guarded([&]() -> int {
        int rc = set_device(h);
        if (rc) return rc;
        if ((rc = order_begin(h, h->stream))) return rc;
        Shards S;
        S.hs = {h};
        S.G = c->world;
        S.first = c->rank;
        S.c = c;
        return bf_search_shards(S, queries_host, nq, k, ids, dists, timing);
    });
}

// Virtual ranks: the same call for G row shards that live on ONE device (shards[g] = vs_bf_create(rows of shard g,
// id_offset = its first row)), driven by the calling thread; the exchanges are no-ops.  For tests of the sharded tie
// order / fp32 rerun without a multi-GPU node.
int vs_bf_search_vshards(vs_index* const* shards, int G, const float* queries_host, int64_t nq, int k, int32_t* ids, float* dists,
                         vs_timing* timing) {
    if (!shards || G < 1 || G > 64 || !queries_host || !ids || !dists || nq < 0 || k < 1) {
        set_error("vs_bf_search_vshards: bad arguments");
        return VS_ERR_INVALID;
    }
    for (int g = 0; g < G; ++g)
        if (shards[g] && refuse_general(shards[g], "vs_bf_search_vshards")) return VS_ERR_UNSUPPORTED;
    for (int g = 0; g < G; ++g)
        if (!shards[g] || shards[g]->kind != 0 || shards[g]->device != shards[0]->device || shards[g]->metric != shards[0]->metric ||
            shards[g]->batch != shards[0]->batch) {
            set_error("vs_bf_search_vshards: shards must be brute-force indexes on one device with one metric and batch size");
            return VS_ERR_INVALID;
        }
    return guarded([&]() -> int {
        int rc = set_device(shards[0]);
        if (rc) return rc;
        Shards S;
        S.hs.assign(shards, shards + G);
        S.G = G;
        for (int g = 0; g < G; ++g)
            if ((rc = order_begin(shards[g], shards[0]->stream))) return rc;
        return bf_search_shards(S, queries_host, nq, k, ids, dists, timing);
    });
}

int vs_ivf_search(vs_index* h, const float* queries_host, int64_t nq, int k, int nprobe, int32_t* ids, float* dists,
                  int64_t* total_candidates, vs_timing* timing) {
    if (refuse_general_bf(h, "vs_ivf_search")) return VS_ERR_UNSUPPORTED;
    if (!h || h->kind != 1 || !queries_host || !ids || !dists || nq < 0 || k < 1 || nprobe < 1) {
        set_error("vs_ivf_search: bad arguments");
        return VS_ERR_INVALID;
    }
    if (k > 16 && refuse_general_ivf(h, "vs_ivf_search with k > 16")) return VS_ERR_UNSUPPORTED;
    nprobe = std::min(nprobe, h->nlist);
    if (nprobe > kMaxNprobe) {
        set_error("nprobe > 256 not supported");
        return VS_ERR_UNSUPPORTED;
    }
    if (k > vs::kIvfWideKMax) {
        set_error("k > 128 not supported");
        return VS_ERR_UNSUPPORTED;
    }
    return guarded([&] { return ivf_search_host(h, nullptr, queries_host, nq, k, nprobe, ids, dists, total_candidates, timing); });
}

int vs_ivf_search_topk(vs_index* h, const float* queries_host, int64_t nq, int k, int nprobe, int32_t* ids, float* dists,
                       int64_t* total_candidates, vs_timing* timing) {
    if (h && h->kind == 0) {
        set_error("vs_ivf_search_topk: not an IVF index");
        return VS_ERR_UNSUPPORTED;
    }
    if (!h || !queries_host || !ids || !dists || nq < 0 || k < 1 || nprobe < 1) {
        set_error("vs_ivf_search_topk: bad arguments");
        return VS_ERR_INVALID;
    }
    if (k > vs::kIvfNdWideKMax) {
        set_error("vs_ivf_search_topk: k > 128");
        return VS_ERR_UNSUPPORTED;
    }
    if (k <= 16 || !h->general) return vs_ivf_search(h, queries_host, nq, k, nprobe, ids, dists, total_candidates, timing);
    nprobe = std::min(nprobe, h->nlist);
    if (nprobe > kMaxNprobe) {
        set_error("nprobe > 256 not supported");
        return VS_ERR_UNSUPPORTED;
    }
    return guarded([&] { return ivf_search_host(h, nullptr, queries_host, nq, k, nprobe, ids, dists, total_candidates, timing); });
}

int vs_ivf_search_metric(vs_index* h, const float* queries_host, int64_t nq, int k, int nprobe, int metric, int32_t* ids, float* dists,
                         int64_t* total_candidates, vs_timing* timing) {
    const int rc = search_metric_checks("vs_ivf_search_metric", h, queries_host && ids && dists, k, metric);
    if (rc) return rc;
    CallMetric cm(h, metric);
    return vs_ivf_search_topk(h, queries_host, nq, k, nprobe, ids, dists, total_candidates, timing);
}

int vs_ivf_search_sharded(vs_index* h, vs_comm* c, const float* queries_host, int64_t nq, int k, int nprobe, int32_t* ids,
                          float* dists, int64_t* total_candidates, vs_timing* timing) {
    if (refuse_general_bf(h, "vs_ivf_search_sharded") || refuse_general_ivf(h, "vs_ivf_search_sharded")) return VS_ERR_UNSUPPORTED;
    if (!h || !c || h->kind != 1 || !queries_host || !ids || !dists || nq < 0 || k < 1 || nprobe < 1) {
        set_error("vs_ivf_search_sharded: bad arguments");
        return VS_ERR_INVALID;
    }
    if (k > 16) {
        set_error("k > 16 not supported by the sharded IVF calls");
        return VS_ERR_UNSUPPORTED;
    }
    return guarded([&] { return ivf_search_host(h, c, queries_host, nq, k, nprobe, ids, dists, total_candidates, timing); });
}

}  // extern "C"
