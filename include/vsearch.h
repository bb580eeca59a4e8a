/*
 * vsearch.h -- C ABI of libvsearch_hip.so, the MI355X (gfx950) vector-search backend.
 *
 * This is the drop-in boundary for the distance + top-k hot path of
 * zyx7k/HAI-25-RAG-on-Edge.  The reference has no FFI; its device seam is the
 * C++ class pair QnnRunner ("queries[B x d] in -> scores[B x N] out") and
 * IVFIndex ("queries in -> (ids, scores) out").  Every entry point below cites
 * the reference interface it replaces (paths relative to the reference root).
 *
 * Conventions
 *   - plain C, no exceptions: every call returns VS_OK (0) or a negative
 *     vs_status; vs_last_error() gives the message for the calling thread.
 *     (Reference: bool + std::cerr in cpu/cpu_baseline.cpp:194-207; throw
 *     std::runtime_error caught in main in main_ivf.cpp:287-290.)
 *   - "host" pointers are ordinary memory owned by the caller; "_dev" entry
 *     points take device (HBM) pointers and a hipStream_t passed as void*.
 *   - one vs_index = one GPU = one caller thread at a time (QnnRunner is not
 *     re-entrant either: shared I/O buffers, QnnRunner.cpp:322-323).  An index has ONE
 *     set of scratch buffers: calls may come on different streams, but each call's work
 *     is ordered behind the previous call's (an event the library records), so calls on
 *     one index never overlap on the device.  Use one index per concurrent stream.
 *   - ids are 0-based row numbers of the base file (cpu_baseline.cpp:130,142),
 *     or reorder_to_original[] values for IVF (IVFIndex.cpp:774-779).
 *   - the product path never falls back to a CPU implementation: without a
 *     usable HIP device every create/search call fails with VS_ERR_DEVICE.
 */
#ifndef VSEARCH_H
#define VSEARCH_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VS_API __attribute__((visibility("default")))

typedef enum vs_status {
    VS_OK = 0,
    VS_ERR_INVALID = -1,     /* bad argument / shape mismatch (main.cpp:121-126, main_ivf.cpp:106-109) */
    VS_ERR_IO = -2,          /* cannot open / truncated / inconsistent file (cpu_baseline.cpp:33-56)     */
    VS_ERR_DEVICE = -3,      /* HIP error or no gfx950 device                                              */
    VS_ERR_NOMEM = -4,
    VS_ERR_UNSUPPORTED = -5  /* e.g. dim != 128, k too large for the compiled kernels                      */
} vs_status;

typedef enum vs_metric {
    VS_METRIC_L2 = 0,        /* squared L2, smallest wins (cpu_baseline.cpp:239-242) -- every graded config */
    VS_METRIC_IP = 1         /* raw inner product, largest wins (qidk main.cpp:30-57, IVFIndex.cpp:449-496) */
} vs_metric;

typedef struct vs_index vs_index; /* opaque: owns device memory, scratch, streams */

/* Mirrors IVFIndex::SearchTiming (IVFIndex.h:31-36) plus the distance / top-k
 * split cpu_baseline prints (cpu_baseline.cpp:281-299).  All in milliseconds,
 * accumulated over the call. */
typedef struct vs_timing {
    double centroid_search_ms; /* IVF coarse stage (IVFIndex.cpp:654-666)                  */
    double gather_ms;          /* probe selection (IVFIndex.cpp:694-726)                   */
    double fine_search_ms;     /* scan + top-k; for brute force: the whole device pipeline */
    double total_ms;           /* wall time of the call                                    */
    double h2d_ms;             /* query upload                                             */
    double d2h_ms;             /* result download                                          */
    double tie_resolve_ms;     /* exact select_topk slot emulation for flagged queries     */
    int64_t tie_queries;       /* how many queries needed it                               */
} vs_timing;

/* ------------------------------------------------------------------ library */
VS_API const char* vs_version(void);
VS_API const char* vs_last_error(void);           /* thread-local, never NULL */
VS_API int vs_device_count(void);                 /* 0 when no HIP device is visible */

/* -------------------------------------------------------------- file formats */
/* .fvecs / .ivecs: repeated [int32 d][d x 4 bytes], little endian
 * (cpu_baseline.cpp:31-58 read_fvecs; main_ivf.cpp:18-50 load_fvecs/load_ivecs).
 * *_shape fills rows/dim only; *_read needs cap_elems >= rows*dim. */
VS_API int vs_fvecs_shape(const char* path, int64_t* rows, int* dim);
VS_API int vs_fvecs_read(const char* path, float* dst, int64_t cap_elems, int64_t* rows, int* dim);
VS_API int vs_ivecs_read(const char* path, int32_t* dst, int64_t cap_elems, int64_t* rows, int* dim);
VS_API int vs_fvecs_write(const char* path, const float* src, int64_t rows, int dim);
VS_API int vs_ivecs_write(const char* path, const int32_t* src, int64_t rows, int dim);
/* .bvecs (TEXMEX byte vectors): repeated [int32 d][d x uint8], little endian; the same rules
 * and errors as the .fvecs functions (cannot open, truncated, inconsistent d: VS_ERR_IO;
 * cap_elems < rows*dim: VS_ERR_INVALID). */
VS_API int vs_bvecs_shape(const char* path, int64_t* rows, int* dim);
VS_API int vs_bvecs_read(const char* path, uint8_t* dst, int64_t cap_elems, int64_t* rows, int* dim);
VS_API int vs_bvecs_write(const char* path, const uint8_t* src, int64_t rows, int dim);

/* results.txt: "Query <i>: (<id>, <dist>) ...\n".
 * style 0 = cpu_baseline.cpp:155-175 (default ostream float formatting),
 * style 1 = main_ivf.cpp:179-183 (std::fixed, 4 decimals).  ids < 0 are skipped. */
VS_API int vs_results_write(const char* path, const int32_t* ids, const float* dists,
                            int64_t nq, int k, int style);

/* Deterministic SIFT-shaped synthetic data: integer-valued
 * f32 in [0, 218], clustered.  Row i depends only on (seed, i), so any slice
 * can be generated independently.  row_begin lets ranks generate shards. */
VS_API int vs_synth_sift(float* dst, int64_t row_begin, int64_t rows, int dim, uint64_t seed);
/* The same generator with the mixture as parameters: x = clip(rint(c_u + N(0, row_sigma^2)), 0, 218), u uniform over
 * n_centers centres c = |N(0, center_sigma^2)| (vs_synth_sift = 4096 centres, 40, 18: strongly clustered, an IVF index
 * reaches recall ~ 1 with a handful of probes).  Many centres and a wide row_sigma give weakly clustered data on which
 * recall falls well below 1: the second distribution of the IVF tests and bench. */
VS_API int vs_synth_mixture(float* dst, int64_t row_begin, int64_t rows, int dim, uint64_t seed, int n_centers,
                            double center_sigma, double row_sigma);

/* The reference's select_topk (cpu_baseline.cpp:127-153) applied to a sparse,
 * row-ordered candidate list; exposed so the tie resolver can be unit-tested. */
VS_API int vs_select_topk_slots(const int32_t* rows, const float* dists, int64_t m, int k,
                                int32_t* out_ids, float* out_dists);

/* -------------------------------------------------------- exact brute force */
/* Replaces the body of run_benchmark's query loop (cpu_baseline.cpp:209-254):
 * norms + cblas_sgemm(1 x N x d) + L2 epilogue + select_topk, and the QNN
 * "database baked into the model" runner (QnnRunner ctor, QnnRunner.h:20).
 * The base is copied to HBM once; id_offset is added to every returned id
 * (row-sharded multi-GPU: each rank passes its shard and its first row). */
VS_API int vs_bf_create(const float* base_host, int64_t n_rows, int dim, int metric,
                        int device, int64_t id_offset, vs_index** out);

/* The same for any vector length, as cpu_baseline.cpp reads whatever dimension the .fvecs
 * header states: 1 <= dim <= 2048 (dim < 1: VS_ERR_INVALID, dim > 2048: VS_ERR_UNSUPPORTED).
 * dim == 128 gives exactly vs_bf_create's index.  Any other dim gives a "general" index: fp32
 * rows padded to a multiple of 16 floats, scanned by the general-dimension kernels (short
 * calls by one launch per batch: vs_bf_one_plan below; same results either way).  It is
 * accepted by vs_bf_search, vs_bf_search_topk, vs_bf_search_dev, vs_bf_search_dev_multi,
 * vs_bf_search_topk_dev_multi, vs_bf_scores_dev, vs_set_batch, vs_index_rows, vs_index_dim,
 * vs_prof_* and vs_destroy, with the same signatures and output layouts (queries are
 * [nq][dim], unpadded).  vs_set_precision: 0 and 1 both mean the fp32 rows, 2 returns
 * VS_ERR_UNSUPPORTED (an index with a byte copy of the rows at other dimensions comes from
 * vs_bf_create_nd_u8 below, not from this creator).  The
 * sharded calls (vs_bf_search_dev_sharded, vs_bf_search_sharded, vs_bf_search_vshards) and
 * every vs_ivf_* call return VS_ERR_UNSUPPORTED on a general index made by this creator (an IVF
 * index at other dimensions comes from vs_ivf_create / vs_ivf_load; a q8 runner from vs_q8_create_nd). */
VS_API int vs_bf_create_nd(const float* base_host, int64_t n_rows, int dim, int metric,
                           int device, int64_t id_offset, vs_index** out);

/* The single-call scan (host only, no GPU needed).  A short call that reads the fp32 rows --
 * fewer than 4 batches of at most 16 queries, k <= 15 -- is answered by ONE launch per batch,
 * without preparation, threshold exchange or merge launches: on the specialised 128-d index
 * by the 128-d single-call kernel, on a general index (vs_bf_create_nd with dim != 128, the
 * fp32 rows of a vs_bf_create_nd_u8* index under vs_set_precision(1) or in a rerun, and the
 * VSEARCH_ND_FORCE=1 form at dim 128) by its sibling for any 1 <= dim <= 2048 (DESIGN.md
 * 4.4d).  The result of a call does not depend on the route: ids, distance bits and flags are
 * those of the per-batch scan.  VSEARCH_ND_ONE=0, read when a general index is created, keeps
 * the per-batch scan for short calls on that index: the comparison toggle.
 *
 * vs_bf_one_plan states the rule for a call of n_batches batches of B queries for k neighbours
 * on the fp32 rows of an index of n_rows rows of dim floats on a device of num_cus compute
 * units; the launch code takes its decision and geometry through the same function.
 *   out[0] = 0: no single-call launch; 1: the 128-d kernel (dim == 128, unless VSEARCH_ND_FORCE
 *            makes vs_bf_create build general indexes there); 2: the general-dimension kernel
 *   out[1] = workgroups of the launch
 *   out[2] = rows in one unit of work handed to a wave (16 / 64)
 *   out[3] = the largest number of such units any one wave gets (route 2 deals them
 *            statically; route 1 hands them out on demand and reports the even share)
 * out[1..3] are 0 with out[0] = 0.  It describes the default rule: the toggle above and a byte
 * scan in force on the index are not its business (a short call that reads the BYTE rows of a
 * general index has a single-call route of its own: vs_bf_one_plan_u8 below).
 * Checks, in this order: null out, n_rows < 1, num_cus < 1, n_batches < 1, B outside [1, 32],
 * k < 1 -> VS_ERR_INVALID; dim < 1 -> VS_ERR_INVALID; dim > 2048 -> VS_ERR_UNSUPPORTED;
 * k > 128 -> VS_ERR_UNSUPPORTED. */
VS_API int vs_bf_one_plan(int64_t n_rows, int dim, int num_cus, int n_batches, int B, int k,
                          int64_t* out /* [4] */);

/* The same for a call that reads the byte rows of a general index made from uint8 rows
 * (vs_bf_create_nd_u8, vs_bf_create_nd_u8_metric; precision 0 / 2, k <= 15): fewer than 4
 * batches of at most 16 queries on at most 2^31 - 1 - 128 rows are ONE launch per batch of the
 * single-call byte kernel, under either metric, instead of a reset, a
 * preparation launch, the per-batch byte scan and a merge launch.  One measured exception: at
 * dim <= 128 (rows of at most 128 bytes) a batch of more than 12 queries keeps the per-batch
 * route, which was 2 - 3 % faster there.  Results do not depend on the
 * route: ids, distance bits and flags (flags == 2 for a batch the exactness rule refuses
 * included) are those of the per-batch byte scan.  VSEARCH_ND_ONE_U8=0, read when the index is
 * created, keeps the per-batch route for short byte calls on that index (VSEARCH_ND_ONE is the
 * toggle of the fp32 rows only).
 *   out[0] = 0: no single-call launch; 3: the single-call byte kernel
 *   out[1..3] as for vs_bf_one_plan's route 2 (workgroups, 64 rows per unit, the most units of
 *            any one wave); 0 with out[0] = 0
 * Host only; the launch code takes its decision and geometry through the same function.  Whether
 * a given index keeps a byte copy, its precision setting and the toggle are not its business.
 * Checks and codes: vs_bf_one_plan's, in the same order. */
VS_API int vs_bf_one_plan_u8(int64_t n_rows, int dim, int num_cus, int n_batches, int B, int k,
                             int64_t* out /* [4] */);

/* Single-call launches enqueued on a brute-force index since the last reset: out[0] = on the
 * fp32 rows (routes 1 and 2 of vs_bf_one_plan), out[1] = on the byte rows (route 3 of
 * vs_bf_one_plan_u8).  Counted on the host when a launch is enqueued, always; no device
 * synchronisation.  reset != 0 clears both after reading.  Null pointers or an IVF index:
 * VS_ERR_INVALID. */
VS_API int vs_bf_one_stats(vs_index* h, int64_t* out /* [2] */, int reset);

/* Wide k on the byte rows (host only, no GPU needed).  A wide call (16 <= k <= 128) spends most
 * of its time in two bulk passes per batch: the distances to a prefix of the rows, and a
 * filtered pass over the rest that keeps what falls under the prefix's bound.  On a general
 * index that keeps a byte copy of its rows (vs_bf_create_nd_u8, vs_bf_create_nd_u8_metric) both
 * passes read the byte rows with int8 MFMA for every batch the exactness rule
 * admits -- decided per batch on the device, without a host synchronisation; any other batch is
 * answered on the fp32 rows inside the same call.  Results do not depend on the route: ids,
 * distance bits and flags are those of the same index under vs_set_precision(h, 1).
 * VSEARCH_ND_WIDE_U8=0, read when the index is created, keeps the fp32 launches for wide k on
 * that index: the comparison toggle.
 *
 * vs_bf_wide_plan states the rule for a call for k neighbours on an index of n_rows rows of dim
 * values; the launch code takes its decision and geometry through the same function.
 *   out[0] = 1: a wide call on the byte copy of a general index of this shape reads the byte
 *            rows; 0: it reads the fp32 rows
 *   out[1] = rows of the prefix: min(n_rows, max(512 (k + 1), n_rows (k + 1) / 2048) rounded up
 *            to a multiple of 4096)
 *   out[2] = 8192, the candidates stored per query behind the prefix (more: the dense fallback)
 * For k <= 15 (not a wide call) all three are 0.  out[0] = 1 for every 16 <= k <= 128 and every
 * dim: no shape left the rule, because none measured slower on the byte rows than under the
 * toggle (1 M rows, batches of 32, k = 16 / 100 / 128, us per batch): 96-d 339 / 457 / 461
 * against 374 / 491 / 498, the smallest gain; 128-d inner product 253 / 338 / 350 against 304 /
 * 390 / 402; 384-d 366 / 464 / 471 against 612 / 680 / 693; 768-d 366 / 485 / 495 against 1049 /
 * 1110 / 1128; 2048-d 578 / 664 / 680 against 2199 / 2265 / 2281 -- every margin many times the
 * spread of either leg (DESIGN.md 4.5c has the table).  Whether a given index keeps a byte copy, its precision setting
 * and the toggle are not its business.
 * Checks, in this order: null out, n_rows < 1, k < 1 -> VS_ERR_INVALID; dim < 1 ->
 * VS_ERR_INVALID; dim > 2048 -> VS_ERR_UNSUPPORTED; k > 128 -> VS_ERR_UNSUPPORTED. */
VS_API int vs_bf_wide_plan(int64_t n_rows, int dim, int k, int64_t* out /* [3] */);

/* Wide batches (k >= 16) on a brute-force index since the last reset: out[0] = batches whose
 * bulk passes ran on the byte rows, out[1] = batches enqueued on the byte route whose verdict
 * sent them to the fp32 rows (both counted on the device, by the first launch of the batch),
 * out[2] = every wide batch enqueued on the index, on any route (counted on the host).  The call
 * synchronises the device; reset != 0 clears all three after reading.  All zeros before the
 * first wide call.  Null pointers or an IVF index: VS_ERR_INVALID (a null handle is refused
 * before any device is touched). */
VS_API int vs_bf_wide_stats(vs_index* h, int64_t* out /* [3] */, int reset);

/* Byte-valued rows at any vector length: base_host is uint8 [n_rows][dim], 1 <= dim <= 2048
 * (dim < 1: VS_ERR_INVALID, dim > 2048: VS_ERR_UNSUPPORTED), squared L2 only.  dim == 128 gives
 * the index vs_bf_create gives for the same rows converted to float: same results, same
 * launches.  Any other dim gives a general index exactly as vs_bf_create_nd builds it (fp32
 * rows padded to 16 floats, norms) PLUS the rows once more as int8 (x - 128), padded to 64
 * bytes, with an int32 term per row, scanned with int8 MFMA at a quarter of the row traffic:
 * for k <= 15 by the byte scan, for 16 <= k <= 128 by the two bulk passes of the wide call
 * (vs_bf_wide_plan above).  The fp32 rows stay -- they serve vs_bf_scores_dev, the tie replay,
 * the dense fallback of a wide call, reruns and every batch the rule below refuses -- so the index takes 1.25 x the device memory of a vs_bf_create_nd index (more below
 * 64-d, where the byte rows are padded to 64).
 *
 * Exactness rule.  The byte scan returns the fp32 scan's distances to the bit when every fp32
 * quantity of the epilogue is an exactly representable integer: with integer values and
 * ||q||^2 + ||b||^2 <= 2^24 both norms, every partial sum of q.b (each <= (||q||^2 + ||b||^2) / 2)
 * and fma(-2, dot, qn + bn) are exact in any summation order.  A batch therefore runs on the
 * byte rows only when (1) every query value of the batch is an integer in [0, 255] and (2) max
 * over the batch of ||q||^2 + max over the base of ||b||^2 <= 2^24; both are checked on the
 * device, in integers.  Any other batch is skipped at k <= 15: the *_dev calls report flags == 2
 * for its queries, vs_bf_search / vs_bf_search_topk rerun it on the fp32 rows themselves.  At
 * k >= 16 such a batch is answered on the fp32 rows inside the same call (flags == 2 does not
 * occur).  Nothing ever returns a distance that differs from the fp32 path's.
 *
 * vs_set_precision on such an index: 0 (default) and 2 use the byte rows for every k, 1 forces
 * the fp32 rows; 2 returns VS_ERR_UNSUPPORTED when max ||b||^2 >= 2^24 (the byte rows are then
 * not kept: no batch could run on them).  Calls accepted and refused: as vs_bf_create_nd.
 *
 * A short call on the byte rows -- fewer than 4 batches of at most 16 queries, k <= 15 -- is one
 * launch per batch (vs_bf_one_plan_u8 above; VSEARCH_ND_ONE_U8=0 at creation keeps the
 * per-batch byte scan); same results and flags either way. */
VS_API int vs_bf_create_nd_u8(const uint8_t* base_host, int64_t n_rows, int dim,
                              int device, int64_t id_offset, vs_index** out);

/* The same under a metric.  Checks, in this order (all but the last need no device; *out is
 * written on success only): null pointers or n_rows <= 0: VS_ERR_INVALID; dim < 1:
 * VS_ERR_INVALID; dim > 2048: VS_ERR_UNSUPPORTED; a metric other than VS_METRIC_L2 /
 * VS_METRIC_IP: VS_ERR_INVALID; ids that do not fit int32: VS_ERR_UNSUPPORTED; no device:
 * VS_ERR_DEVICE.
 *
 * VS_METRIC_L2: the call is vs_bf_create_nd_u8 -- same index, same launches, at dim 128 too.
 *
 * VS_METRIC_IP, dim != 128: the general index of vs_bf_create_nd(rows as float, VS_METRIC_IP)
 * PLUS the byte rows vs_bf_create_nd_u8 stores (int8 (x - 128), padded to 64 bytes) and one
 * int32 per row, the sum of its stored bytes; not kept when max ||b||^2 >= 2^24, as under L2.
 * VS_METRIC_IP, dim == 128: the specialised 128-d index has no inner-product byte kernel, so the
 * creator builds the GENERAL form here as well, with the byte copy, and the same kernels serve
 * SIFT.  The sharded and virtual-shard calls and every vs_ivf_* call refuse this index like any
 * general index; data that needs those calls under inner product goes through vs_bf_create on
 * float rows.
 *
 * For k <= 15 under precision 0 or 2, vs_bf_search, vs_bf_search_dev, vs_bf_search_dev_multi,
 * vs_bf_search_topk and vs_bf_search_topk_dev_multi run on the byte rows under inner product.
 * The exactness rule above applies unchanged, per batch: every query value an integer in
 * [0, 255] and max over the batch of ||q||^2 + max over the base of ||b||^2 <= 2^24, checked on
 * the device in integers.  Every partial sum of q.b is then at most (||q||^2 + ||b||^2) / 2 <=
 * 2^23, so the fp32 chain is exact in any order and equals the int32 product the byte scan
 * rebuilds, q.b = q'.b' + 128 (sum q' + sum b') + 128^2 dim with x' = x - 128.  Any other batch
 * is skipped: the *_dev calls report flags == 2, the host calls rerun it on the fp32 rows.
 * Precision 1 forces the fp32 rows; precision 2 returns VS_ERR_UNSUPPORTED when the byte copy
 * was not kept.  k >= 16 runs its bulk passes on the byte rows as under L2 (vs_bf_wide_plan; a
 * batch the rule refuses: on the fp32 rows, in the same call); vs_bf_scores_dev reads the fp32
 * rows.  Short calls on
 * the byte rows take the single-call byte kernel as under L2 (vs_bf_one_plan_u8).
 *
 * Outputs are the inner-product ones of vs_bf_create_nd: the *_dev calls return s = -(q.v)
 * ascending by (s, id), an exactly zero product as -0.0; the host calls return q.v descending,
 * equal scores in ascending id, no tie replay.  Nothing ever returns a number that differs from
 * what vs_bf_create_nd(rows as float, VS_METRIC_IP) returns for the same call. */
VS_API int vs_bf_create_nd_u8_metric(const uint8_t* base_host, int64_t n_rows, int dim, int metric,
                                     int device, int64_t id_offset, vs_index** out);

/* Fixed model batch, like QnnRunner::getBatchSize (QnnRunner.h:37); 1..32, default 32.
 * Larger query sets are processed in batches of this size, the last one
 * zero-padded (main.cpp:206-211). */
VS_API int vs_set_batch(vs_index* h, int batch);

/* Data path of the scan.  0 = auto (default): when every base value is an integer in [0, 255] -- true for
 * SIFT -- the index also keeps the rows as bytes and scans them with int8 MFMA; distances are then
 * computed in int32 and are the same integers the fp32 path produces exactly, at a quarter of the memory
 * traffic.  A batch containing a non-integer query is detected on the device, skipped and rerun in fp32
 * (vs_bf_search does that itself; the *_dev calls report it as flags == 2).  1 = force fp32 (the reference
 * arithmetic, cblas_sgemm + epilogue); 2 = require int8 (VS_ERR_UNSUPPORTED when the base does not allow it).
 * IVF indexes alike: 1 = the list scan reads the fp32 rows (IVFIndex.cpp:270-358's arithmetic).
 * Wide k (k >= 16): the specialised 128-d index and vs_bf_create_nd indexes read the fp32 rows whatever the setting; a
 * general index with a byte copy (vs_bf_create_nd_u8*) reads the byte rows at 0 and 2 and the fp32 rows at 1. */
VS_API int vs_set_precision(vs_index* h, int precision);
/* IVF indexes are created with the north-star's squared L2; VS_METRIC_IP selects the reference's own ranking (IVFIndex.cpp:
 * 449-496, :697-723): nprobe lists of LARGEST q.c, k candidates of largest q.v (fp32 rows; the int8 copies are an L2 device).
 * The host call returns the scores q.v (descending); the *_dev calls return -q.v (ascending), like brute force. */
VS_API int vs_ivf_set_metric(vs_index* h, int metric);

/* Host-buffer search with the reference's exact semantics: ids/dists are
 * [nq x k], ascending distance, ties ordered exactly as select_topk leaves
 * them (flagged queries are re-resolved, see DESIGN.md "Ties").  k clamps to
 * n_rows; unused slots are id -1 / dist +inf.
 * VS_METRIC_IP: dists holds the scores q.v, descending (the *_dev calls below return
 * -q.v, ascending); equal scores are returned in ascending id, with no tie replay
 * (timing->tie_queries stays 0). */
VS_API int vs_bf_search(vs_index* h, const float* queries_host, int64_t nq, int k,
                        int32_t* ids, float* dists, vs_timing* timing);

/* Device-level, asynchronous on `stream`: one batch (B <= batch) of queries
 * already in HBM -> the k+1 best (dist, id) per query by (dist, id) ascending,
 * [B x (k+1)], plus flags[B]: 1 where two of those distances are equal (the
 * caller must then use vs_bf_search for reference tie order), 2 where the int8
 * path had to skip the batch (rerun with vs_set_precision(h, 1)).  A query with
 * flags == 2 has all its k+1 ids -1 and all its k+1 distances +inf.  This is the
 * analogue of QnnRunner::executeBatchRaw + getRawOutputBuffer (QnnRunner.h:28-30)
 * with the top-k fused in, so the B x N score matrix never exists. */
VS_API int vs_bf_search_dev(vs_index* h, const float* queries_dev, int B, int k,
                            int32_t* ids_dev, float* dists_dev, int32_t* flags_dev, void* stream);

/* The same for n_batches consecutive batches of exactly B queries each
 * (queries_dev [n_batches*B x d], outputs [n_batches*B x (k+1)], flags [n_batches*B]):
 * the harness loop of main.cpp:201-251 in one call.  Every batch still streams the
 * base once; groups of up to 32 batches share ONE persistent scan launch (preceded by
 * three small bound-seeding launches, followed by one merge launch), all on `stream`,
 * so no launch gap, grid fill or drain separates consecutive batches.
 * flags == 2 is a verdict per batch: all B queries of a skipped batch carry it (ids -1,
 * distances +inf), and every other batch of the same call is unaffected -- its lists and
 * flags are what a call without the skipped batches returns, so only the flagged batches
 * need the rerun under vs_set_precision(h, 1). */
VS_API int vs_bf_search_dev_multi(vs_index* h, const float* queries_dev, int n_batches, int B, int k,
                                  int32_t* ids_dev, float* dists_dev, int32_t* flags_dev, void* stream);

/* Wide k: 1 <= k <= 128.  For k <= 15 the result is exactly vs_bf_search's (same code path).  For k >= 16: the k best by
 * select_topk's slot semantics; order among equal distances = slot order, stably sorted.  k > 128 returns
 * VS_ERR_UNSUPPORTED.  The k >= 16 path scans the fp32 rows whatever vs_set_precision says -- except on a general index
 * with a byte copy (vs_bf_create_nd_u8*), where its two bulk passes read the byte rows at precision 0 or 2 (vs_bf_wide_plan);
 * the tie replay reads the fp32 rows; the distances are the same either way.
 * VS_METRIC_IP, for every k: the scores q.v, descending (vs_bf_search_topk_dev_multi returns -q.v, ascending); equal scores
 * in ascending id, with no tie replay. */
VS_API int vs_bf_search_topk(vs_index* h, const float* queries_host, int64_t nq, int k,
                             int32_t* ids, float* dists, vs_timing* timing);
/* Device form of vs_bf_search_dev_multi for 1 <= k <= 128: outputs [n_batches*B x (k+1)] by (dist, id) ascending,
 * flags[n_batches*B] as vs_bf_search_dev_multi (1 = equal distances among the k+1, 2 = int8 batch skipped; for k >= 16
 * 2 does not occur: the fp32 rows are scanned, or, on a general index with a byte copy, the byte rows for the batches the
 * exactness rule admits and the fp32 rows for the others, in the same call -- vs_bf_wide_plan). */
VS_API int vs_bf_search_topk_dev_multi(vs_index* h, const float* queries_dev, int n_batches, int B, int k,
                                       int32_t* ids_dev, float* dists_dev, int32_t* flags_dev, void* stream);

/* QnnRunner::executeBatchRaw proper (QnnRunner.cpp:683-724): the raw
 * [B x ld] score matrix, scores_dev[b*ld + j] = dist(query b, row j), ld >= n_rows. */
VS_API int vs_bf_scores_dev(vs_index* h, const float* queries_dev, int B,
                            float* scores_dev, int64_t ld, void* stream);

/* ------------------------------------------- quantised score path (UFIXED_POINT_8) */
/* The reference's device runner with its uint8 I/O (qidk_bruteforce/android/app/main/jni):
 * QnnRunner ctor (QnnRunner.h:20) bakes the database into the graph as uint8 weights;
 * executeBatchRaw (QnnRunner.cpp:608-645) quantises a [B x d] batch with
 * quantize_buffer_neon (QnnRunner.cpp:13-55: q8 = sat_u8(trunc(x * (1 / input_scale) + 0.5)): a multiplication by the
 * reciprocal and an addition, rounded separately, as QnnRunner.cpp:544 computes it --
 * offset 0), runs the graph and leaves the raw uint8 [B x N] inner-product scores in
 * its output buffer (getRawOutputBuffer, QnnRunner.h:37); the harness takes the k
 * largest per query (find_top_k_int8, main.cpp:30-57) and prints score * output_scale
 * (main.cpp:244-246).  Here: real = scale * (q + offset) for all three tensors (QNN's
 * scale-offset encoding, QnnRunner.cpp:490-508; input and output offsets are 0 there),
 *   ip      = sum_t q8[t] * (w8[t] + weight_offset)                      (int32, exact)
 *   score8  = sat_u8(trunc(ip * ((input_scale * weight_scale) / output_scale) + 0.5))
 * with every product and sum rounded separately in fp32 (no fused multiply-add), the
 * rounding rule of the reference's own quantiser.  What the closed QNN converter / HTP
 * runtime do inside the graph (weight encoding, accumulator requantisation) is not in the
 * reference: results are checked against oracle/ (vo_q8_*), parity unpinned.
 * Equal scores are returned in ascending id order (the reference: whatever its C++
 * library's heap leaves). */
typedef struct vs_q8 vs_q8; /* opaque: quantised database, I/O buffers, stream */
typedef struct vs_q8_encodings {
    float input_scale;     /* QnnRunner.cpp:490  0.6627451181411743  */
    float weight_scale;    /* database tensor (inside the reference's model blob) */
    int32_t weight_offset; /* <= 0, real = scale * (q + offset) */
    float output_scale;    /* QnnRunner.cpp:507  1013.43121337890625 */
} vs_q8_encodings;

/* enc == NULL: the runner's hard-coded input / output scales and weight_scale =
 * max(database) / 255, offset 0.  id_offset as in vs_bf_create.  dim must be 128
 * (VS_ERR_UNSUPPORTED otherwise); any other vector length: vs_q8_create_nd. */
VS_API int vs_q8_create(const float* base_host, int64_t n_rows, int dim, const vs_q8_encodings* enc,
                        int device, int64_t id_offset, vs_q8** out);

/* The same for any vector length, as create_model.py builds the [batch, dim] x [dim, N] graph for
 * whatever dim the .fvecs header states and QnnRunner::getDim() reports it: 1 <= dim <= 2048.
 * Checked in this order, the first five without a device: null pointers or n_rows <= 0:
 * VS_ERR_INVALID; dim < 1: VS_ERR_INVALID; dim > 2048: VS_ERR_UNSUPPORTED; ids that do not fit
 * int32 (n_rows + id_offset > 2^31 - 1, id_offset < 0): VS_ERR_UNSUPPORTED; enc given with a scale
 * that is not > 0 or a weight_offset outside [-255, 0]: VS_ERR_INVALID; no device: VS_ERR_DEVICE.
 * dim == 128 gives exactly vs_q8_create's runner: the same kernels, launches and bytes
 * (VSEARCH_Q8_ND_FORCE=1 in the environment, read at creation by this function only, builds the
 * general runner at 128 as well: the comparison toggle).  Any other dim gives a "general"
 * runner: rows as int8 (w8 - 128) padded with zeros to a multiple of 64 bytes, scored by a kernel
 * that walks the row in 128-byte steps.  Every vs_q8_* call below accepts it with the same
 * signatures and output layouts; queries are [B][dim] floats, unpadded; k <= 16 stays (k <= 128: the _topk calls);
 * vs_q8_dim returns dim.  enc == NULL: as above, weight_scale over all n_rows * dim values.
 * The arithmetic is the one stated above, with t < dim; ip is exact in int32 (|ip| <= 255 * 255 *
 * 2048 < 2^27) and (float)ip is its one round-to-nearest conversion, inexact above 2^24 exactly
 * as in oracle/. */
VS_API int vs_q8_create_nd(const float* base_host, int64_t n_rows, int dim, const vs_q8_encodings* enc,
                           int device, int64_t id_offset, vs_q8** out);
VS_API void vs_q8_destroy(vs_q8* h);
VS_API int64_t vs_q8_num_docs(const vs_q8* h);     /* QnnRunner::getNumDocs   (QnnRunner.h:52) */
VS_API int vs_q8_dim(const vs_q8* h);              /* QnnRunner::getDim       (QnnRunner.h:50) */
VS_API int vs_q8_batch(const vs_q8* h);            /* QnnRunner::getBatchSize (QnnRunner.h:48): 32 = the largest B */
VS_API float vs_q8_output_scale(const vs_q8* h);   /* QnnRunner::getOutputScale (QnnRunner.h:41) */
VS_API int vs_q8_get_encodings(const vs_q8* h, vs_q8_encodings* out);

/* executeBatchRaw + getRawOutputBuffer: scores_dev[b*ld + j] = score8(query b, row j),
 * 1 <= B <= 32, ld >= rows (16-byte stores when ld and scores_dev are multiples of 16). */
VS_API int vs_q8_execute_dev(vs_q8* h, const float* queries_dev, int B, uint8_t* scores_dev,
                             int64_t ld, void* stream);
/* The same through host buffers: scores_host is [B x rows], dense. Blocking. */
VS_API int vs_q8_execute(vs_q8* h, const float* queries_host, int B, uint8_t* scores_host);

/* executeBatchRaw + find_top_k_batch_parallel (main.cpp:59-71) for n_batches batches of B
 * queries: ids_dev [n_batches*B x k] (-1 where the database has fewer than k rows),
 * scores_dev [n_batches*B x k] uint8, largest first.  k <= 16. */
VS_API int vs_q8_search_dev(vs_q8* h, const float* queries_dev, int n_batches, int B, int k,
                            int32_t* ids_dev, uint8_t* scores_dev, void* stream);
/* Host-buffer form: the harness loop of main.cpp:201-251 (batches of 32, the last one
 * short). Blocking. */
VS_API int vs_q8_search(vs_q8* h, const float* queries_host, int64_t nq, int k, int32_t* ids,
                        uint8_t* scores);

/* The same for k up to 128 (find_top_k_int8 takes any top_k, main.cpp:36-57, 85).  Layouts and
 * meaning are those of vs_q8_search_dev / vs_q8_search: [n_batches*B x k] ([nq x k] for the host
 * form), largest score first, equal scores in ascending id, ids include id_offset, slots past the
 * rows are (-1, 0), 1 <= B <= 32.  Checked in this order: null pointers (a NULL handle is refused
 * without touching a device), n_batches < 1, B out of range or nq < 0: VS_ERR_INVALID; k < 1:
 * VS_ERR_INVALID; k > 128: VS_ERR_UNSUPPORTED.
 *  - k <= 16: the call IS vs_q8_search_dev / vs_q8_search (same launches, same results).
 *  - 17 <= k <= 128: per batch the quantiser and score kernel as above (one quantiser launch per
 *    group of 32 batches), then a counting select over the score matrix in three launches: the
 *    256-bin histogram of every 16384-row chunk; per query the cut value t = the largest score
 *    with at least min(k, rows) rows at or above it, from a suffix sum, and for every value at or
 *    above t the output position of each chunk's first row of that value; then every chunk that
 *    holds a row to be returned writes its rows straight into their sorted places (of the rows
 *    equal to t, the lowest-numbered ones).  No sort, no candidate cap, no fallback, no atomics on
 *    global memory: exact by construction, the same bits on every run, at a cost that does not
 *    depend on the score distribution.  Bytes of the matrix past the last row are never counted.
 * The device call is asynchronous on the caller's stream: no host synchronisation, nothing is
 * rerun from the host.  Scratch is allocated by the first call with k >= 17, all or nothing
 * (callers with k <= 16 pay nothing), and does not depend on n_batches: vs_q8_wide_plan. */
VS_API int vs_q8_search_topk_dev(vs_q8* h, const float* queries_dev, int n_batches, int B, int k,
                                 int32_t* ids_dev, uint8_t* scores_dev, void* stream);
/* Host-buffer form: batches of 32, the last one short.  Blocking. */
VS_API int vs_q8_search_topk(vs_q8* h, const float* queries_host, int64_t nq, int k,
                             int32_t* ids, uint8_t* scores);
/* find_top_k_batch_parallel (main.cpp:59-71) on a raw score buffer the caller owns, as the harness
 * ranks the buffer of getRawOutputBuffer: B rows of ld bytes, of which the first
 * vs_q8_num_docs(h) are the scores of the runner's rows (ids include id_offset); the bytes from
 * there to ld may hold anything and are ignored.  ids_dev / top_dev are [B x k] as above.
 * ld >= rows, ld % 64 == 0 and a 16-byte aligned scores_dev, otherwise VS_ERR_INVALID before any
 * device work; then k < 1: VS_ERR_INVALID, k > 128: VS_ERR_UNSUPPORTED.  k <= 16 runs the chunk
 * and final kernels of vs_q8_search_dev on that buffer, 17 <= k <= 128 the counting select.
 * Asynchronous on the caller's stream. */
VS_API int vs_q8_topk_scores_dev(vs_q8* h, const uint8_t* scores_dev, int64_t ld, int B, int k,
                                 int32_t* ids_dev, uint8_t* top_dev, void* stream);
/* Host only, no GPU: the counting select for a runner of n_rows rows at 17 <= k <= 128
 * (VS_ERR_INVALID for a null out, n_rows < 1 or any other k).  out[0] = chunks per query =
 * ceil(n_rows / 16384), out[1] = 16384, out[2] = the device scratch bytes the first wide call
 * allocates (the launch code sizes its allocation through the same function): with C = out[0],
 * 32 C 1024 of histograms / positions, 32 * 4 of cut values, 32 C 4 of chunk flags and
 * 32 * 128 * (4 + 1) of host-form results. */
VS_API int vs_q8_wide_plan(int64_t n_rows, int k, int64_t* out /* [3] */);

/* ------------------------------------------- int16 cosine score path */
/* The reference's third score path (AMD_npu/): Codes/preprocess.py:24-42 L2-normalises every
 * base row and every query, multiplies by 1000 and truncates to int16; Codes/test.cpp:32-43,
 * 285-311 produces the int16 x int16 -> int32 matrix C = A B^T in row-major order.  A score is a
 * cosine similarity in fixed point, scale^2 cos(theta).  XRT, the xclbin and the AIE tile-major
 * output layout are not restated; the quantiser and the integer score matrix are, exactly.
 *
 * The quantiser.  For a row x[0..n) and a scale:
 *  1. Squares: s_i = RN(x_i * x_i).  Every product and sum is rounded separately in fp32, with no
 *     FMA.
 *  2. Sum of squares: S = P(s, n), which is numpy's pairwise order.
 *     - For n < 8: a running sum from 0, in order.
 *     - For 8 <= n <= 128: start eight partial sums as r_j = s_j; for i = 8, 16, ... while
 *       i + 8 <= n: r_j = RN(r_j + s_{i+j}); res = ((r0+r1)+(r2+r3))+((r4+r5)+(r6+r7)); add the
 *       last n mod 8 elements to res in order.
 *     - For n > 128: n2 = floor(n / 2) rounded down to a multiple of 8;
 *       S = RN(P(s[0..n2)) + P(s[n2..n))).
 *  3. Quantise: den = RN(sqrt_rn(S) + (float)1e-8); v_i = RN(RN(x_i / den) * scale);
 *     q_i = (int16) trunc(v_i).  A NaN gives 0.  Division and square root are correctly rounded.
 * This equals ((x / (np.linalg.norm(x, axis=1, keepdims=True) + 1e-8)) * scale).astype(np.int16)
 * on finite float32 rows.  Every finite |q_i| <= scale; a row with an infinity, or whose squares
 * overflow, quantises to all zeros; a zero row stays zero.  scale must be finite and in
 * [1, 2047]; the reference's value is 1000. */
typedef struct vs_i16 vs_i16; /* opaque: quantised database, scratch, stream */

/* Host only, no GPU: dst[rows x dim] = the quantised rows.  VS_ERR_INVALID for null pointers,
 * rows < 0, dim outside [1, 2048] or a bad scale. */
VS_API int vs_i16_quantize(const float* src, int64_t rows, int dim, float scale, int16_t* dst);
/* Host only: the quantised rows as raw little-endian int16, the row count padded with zero rows
 * to a multiple of row_multiple >= 1 (preprocess.py: 32 for A.bin, 256 for B.bin). */
VS_API int vs_i16_write_bin(const char* path, const float* src, int64_t rows, int dim, float scale,
                            int64_t row_multiple);

/* The runner.  Checked in this order, all but the last without a device, *out written on success
 * only: null pointers or n_rows <= 0: VS_ERR_INVALID; dim < 1: VS_ERR_INVALID; dim > 2048:
 * VS_ERR_UNSUPPORTED; ids that do not fit int32 (n_rows + id_offset > 2^31 - 1, id_offset < 0):
 * VS_ERR_UNSUPPORTED; a scale that is not finite or is outside [1, 2047]: VS_ERR_INVALID; no
 * device: VS_ERR_DEVICE.  The float rows are uploaded in bounded chunks and quantised on the
 * device by the kernel that quantises the queries of every call.  The device image holds 2 bytes
 * per element (each int16 value as the float16 of the same integer), rows padded with zeros to 64
 * bytes, 64 spare zero rows behind the last one. */
VS_API int vs_i16_create(const float* base_host, int64_t n_rows, int dim, float scale, int device,
                         int64_t id_offset, vs_i16** out);
VS_API void vs_i16_destroy(vs_i16* h);
VS_API int64_t vs_i16_num_docs(const vs_i16* h);
VS_API int vs_i16_dim(const vs_i16* h);
VS_API int vs_i16_batch(const vs_i16* h); /* 32 = the largest B */
VS_API float vs_i16_scale(const vs_i16* h);
/* Diagnostic: stored rows [row0, row0 + n) back as int16 [n x dim] in host memory.  Blocking.
 * VS_ERR_INVALID when the range leaves the index. */
VS_API int vs_i16_rows_read(vs_i16* h, int64_t row0, int64_t n, int16_t* dst);

/* scores_dev[b*ld + j] = sum_t q'[b][t] * b'[j][t] with q', b' the quantised query b and row j:
 * the row-major matrix test.cpp reconstructs, exact in int32.  queries_dev is [B x dim] floats,
 * 1 <= B <= 32, ld >= rows.  Asynchronous on the caller's stream. */
VS_API int vs_i16_execute_dev(vs_i16* h, const float* queries_dev, int B, int32_t* scores_dev,
                              int64_t ld, void* stream);
/* The same through host buffers: scores_host is [B x rows], dense.  Blocking. */
VS_API int vs_i16_execute(vs_i16* h, const float* queries_host, int B, int32_t* scores_host);

/* The k largest scores per query for n_batches batches of B queries ([n_batches*B x dim] floats):
 * ids_dev and scores_dev are [n_batches*B x k], largest score first, equal scores in ascending
 * id; slots past the rows are (-1, INT32_MIN).  1 <= B <= 32; k < 1: VS_ERR_INVALID; k > 16:
 * VS_ERR_UNSUPPORTED.  The top-k is fused into the scan: the score matrix is never written.
 * Asynchronous on the caller's stream, no host synchronisation. */
VS_API int vs_i16_search_dev(vs_i16* h, const float* queries_dev, int n_batches, int B, int k,
                             int32_t* ids_dev, int32_t* scores_dev, void* stream);
/* Host-buffer form: batches of 32, the last one short.  Blocking. */
VS_API int vs_i16_search(vs_i16* h, const float* queries_host, int64_t nq, int k, int32_t* ids,
                         int32_t* scores);

/* The same for k up to 128.  Layouts and meaning are those of vs_i16_search_dev / vs_i16_search:
 * [n_batches*B x k], largest score first, equal scores in ascending id, ids include id_offset,
 * slots past the rows are (-1, INT32_MIN), scores are the exact int32 products of the quantised
 * vectors, 1 <= B <= 32.  Checked in this order: null pointers, n_batches < 1, B out of range or
 * nq < 0: VS_ERR_INVALID; k < 1: VS_ERR_INVALID; k > 128: VS_ERR_UNSUPPORTED.
 *  - k <= 16: the call IS vs_i16_search_dev / vs_i16_search (same launches, same results).
 *  - 17 <= k <= 128: the wide pipeline.  Per launch group of up to 16 batches, all stream-ordered:
 *    the keys -(q'.b') of a strided sample of the rows and their k-th smallest give a bound per
 *    query; one filter scan over all rows lists every row whose key is at or under the bound
 *    (at most 8192 stored per query, all counted); the k best of each list are the answer.  A
 *    query with more than 8192 candidates (masses of equal scores) has its batch answered by a
 *    dense fallback enqueued behind under a device-side flag: keys of row chunks, a selection per
 *    chunk, a selection over the chunk lists.  When the sample is the whole base its selection is
 *    the answer.  Exact on every path.
 * The device call is asynchronous on the caller's stream: no host synchronisation, nothing is
 * rerun from the host.  Scratch is allocated by the first call with k >= 17 (callers with k <= 16
 * pay nothing) and does not depend on n_batches: with P = rows rounded up to 64,
 * 128 max(min(P, 2^20), 64 sample_groups(rows, 128)) bytes of keys, 2 x 16 MiB of candidate
 * lists, 32 KiB ceil(P / 2^20) of chunk lists and under 1 MiB of outputs, bounds and counters. */
VS_API int vs_i16_search_topk_dev(vs_i16* h, const float* queries_dev, int n_batches, int B, int k,
                                  int32_t* ids_dev, int32_t* scores_dev, void* stream);
/* Host-buffer form: batches of 32, the last one short.  Blocking. */
VS_API int vs_i16_search_topk(vs_i16* h, const float* queries_host, int64_t nq, int k,
                              int32_t* ids, int32_t* scores);
/* Host only, no GPU: the sample of the wide pipeline for a base of n_rows rows at 17 <= k <= 128
 * (VS_ERR_INVALID for a null out, n_rows < 1 or any other k).  out[0] = sample groups,
 * out[1] = stride, out[2] = candidates stored per query (8192).  The rule:
 *  - rows come in groups of 64: n_groups = ceil(n_rows / 64);
 *  - L0 = max(64 k, ceil(n_rows k / 2048));
 *  - sample_groups = min(n_groups, ceil(L0 / 64)); stride = n_groups / sample_groups (integer
 *    division); the sample is the groups j stride for j < sample_groups.
 * When sample_groups < n_groups every sample group is a full group (the last one sampled is at
 * most n_groups - 2), so the sample holds at least 64 k rows; when sample_groups == n_groups the
 * sample is the whole base.  The stride is deliberate: a prefix gives a useless bound on a base
 * whose similar rows sit together, as the chunks of one document do.  A query's candidates are
 * the rows whose score is at least the k-th best score of the sample. */
VS_API int vs_i16_wide_plan(int64_t n_rows, int k, int64_t* out /* [3] */);
/* Counters of the wide pipeline since the last reset, always kept; synchronises the device;
 * reset != 0 clears them afterwards.  out[0] = queries ranked from their candidate lists,
 * out[1] = the most candidates any one query had (the count, not the number stored: it may exceed
 * 8192), out[2] = queries answered by the dense fallback (every query of a batch in which a list
 * overflowed), out[3] = queries whose sample was the whole base.  All zeros before the first call
 * with k >= 17.  VS_ERR_INVALID for null pointers. */
VS_API int vs_i16_wide_stats(vs_i16* h, int64_t* out /* [4] */, int reset);

/* ---------------------------------------------------------------------- IVF */
/* IVFIndex ctor (IVFIndex.cpp:154-177): reads ivf_config.json, cluster_offsets.npy,
 * vectors_reordered.npy, reorder_to_original.npy (reordered mode) and
 * centroids.npy (the reference bakes centroids into centroids.bin for the NPU,
 * IVFIndex.cpp:167-169).  rank/world select the lists this GPU owns
 * (cluster-sharded search); 0/1 = everything. */
VS_API int vs_ivf_load(const char* index_dir, int device, int rank, int world, vs_index** out);

/* Same, from arrays in host memory (layout of create_ivf_model_reordered.py:141-169).
 *
 * Both creators take the dimension the arrays / ivf_config.json state (IVFIndex.cpp:181-204):
 * 1 <= dim <= 2048.  dim == 128 builds the specialised index described elsewhere in this header.
 * Any other dim builds a GENERAL IVF INDEX: the reordered rows and the centroids as fp32 rows
 * padded to a multiple of 16 floats with their norms, offsets and reorder_to_original -- no byte
 * copy, no sharding.  VSEARCH_IVF_ND_FORCE=1 (read at creation) builds the general index at
 * dim 128 as well (unsharded only): the comparison toggle, as VSEARCH_ND_FORCE is for brute force.
 *
 * Checks, in this order (the first four need no device): null pointers, n_rows / nlist <= 0 or a
 * bad (rank, world) -> VS_ERR_INVALID; dim < 1 -> VS_ERR_INVALID; dim > 2048 ->
 * VS_ERR_UNSUPPORTED; dim != 128 with world > 1 -> VS_ERR_UNSUPPORTED; offsets that do not cover
 * the rows or are not monotone -> VS_ERR_INVALID; then the device.
 *
 * A general IVF index is searched list-major on its fp32 rows under squared L2.
 * A centroid score is the number the brute-force general scan returns for the centroid as a row;
 * equal scores go to the lower list id.  A distance is bit-identical to what vs_bf_create_nd's
 * index returns for that row and query; equal distances rank by position in vectors_reordered.
 *   accepted: vs_ivf_search, vs_ivf_search_dev, vs_ivf_search_dev_multi for 1 <= k <= 16 (same
 *     signatures and output layouts; queries are [nq][dim], unpadded; every launch group of up to
 *     32 batches stays on the caller's stream), vs_ivf_save, vs_index_rows, vs_index_dim,
 *     vs_index_nlist, vs_prof_*, vs_set_batch, vs_destroy, vs_set_precision 0 or 1 (both mean the
 *     fp32 rows), vs_ivf_set_metric(VS_METRIC_L2);
 *   VS_ERR_UNSUPPORTED, with the dimension in the message: 17 <= k <= 128, vs_set_precision 2,
 *     vs_ivf_set_metric(VS_METRIC_IP), vs_ivf_widek_stats, every sharded and virtual-shard call.
 *   17 <= k <= 128 comes through vs_ivf_search_topk / vs_ivf_search_topk_dev_multi below.
 *   Inner product comes through vs_ivf_search_metric / vs_ivf_search_metric_dev_multi below, which
 *     take the metric per call; the index's own setting stays squared L2.
 * Short calls.  A launch group of fewer than 4 batches of at most 16 queries with k <= 16 on a
 * general IVF index (any creator, VSEARCH_IVF_ND_FORCE=1 at 128-d included, either metric) is
 * answered by TWO launches per batch on the caller's stream -- centroid scores, probe selection
 * and the work table; then the probed lists in row chunks over the whole grid, top-k, ranking and
 * id mapping (vs_ivf_one_plan below states the rule).  The result of a call does
 * not depend on the route: ids, distance bits, empty slots and *total_candidates are those of the
 * launch group's ordinary route.  VSEARCH_IVF_ONE=0, read when the index is created, keeps that
 * route for short calls on that index: the comparison toggle.  An index with a byte copy of its
 * rows (vs_ivf_create_nd_u8) takes two launches too: under vs_set_precision(h, 1) the ones above,
 * on the fp32 rows; at precision 0 or 2 the byte route (vs_ivf_one_plan_u8 below
 * states the rule) -- the same coarse launch, which also decides per query whether it runs on
 * bytes, and ONE scan launch that reads the byte rows with int8 MFMA for the queries that qualify
 * and the fp32 rows for every other query of the same batch.  VSEARCH_IVF_ONE_U8=0, read when
 * the index is created, keeps the group route for such calls on that index.
 * The route's scratch (scores, unit table, tickets, counters) exists once per index, like the
 * group route's: calls on ONE index must be ordered by their streams.  Short calls on one index
 * from two streams at once corrupt each other silently; concurrent front ends need an index each
 * or a stream in common.
 * vs_ivf_build and vs_ivf_build_index stay 128-d only; vs_ivf_build_nd and vs_ivf_build_index_nd
 * build at every dimension this creator takes.  A general IVF index that also keeps its rows as
 * bytes and scans them with int8 MFMA comes from vs_ivf_create_nd_u8 below, not from this creator. */
VS_API int vs_ivf_create(const float* vectors_reordered, int64_t n_rows, int dim,
                         const float* centroids, int nlist, const int32_t* cluster_offsets,
                         const int32_t* reorder_to_original, int device, int rank, int world,
                         vs_index** out);

/* Byte-valued rows at any vector length: vectors_reordered is uint8 [n_rows][dim], 1 <= dim <=
 * 2048; the centroids stay float [nlist][dim]; the index is unsharded.  Checks in vs_ivf_create's
 * order (the first four need no device): null pointers, n_rows / nlist <= 0 -> VS_ERR_INVALID;
 * dim < 1 -> VS_ERR_INVALID; dim > 2048 -> VS_ERR_UNSUPPORTED; offsets that do not cover the rows
 * or are not monotone -> VS_ERR_INVALID; then the device.
 *
 * dim == 128 gives the index vs_ivf_create gives for the same rows converted to float (same
 * launches, same results; VSEARCH_IVF_ND_FORCE=1 builds the general form here too).  Any other
 * dim gives the general IVF index of vs_ivf_create PLUS the reordered rows once more as int8
 * (x - 128), padded to 64 bytes, with an int32 term per row: about 1.25 x the device memory (more
 * below 64-d).  As for vs_bf_create_nd_u8 the byte copy is not kept when max ||b||^2 >= 2^24.
 *
 * Results: ids, distances and *total_candidates are what vs_ivf_create's index returns for the
 * same rows converted to float, for every query and every call.  Coarse scores and probes are
 * computed as there, on the fp32 centroids; the byte copy only changes which kernel scans a
 * (query, list) pair.  The exactness rule of vs_bf_create_nd_u8 is applied PER QUERY: a query is
 * scanned on the byte rows only when every value of it is an integer in [0, 255] and ||q||^2 +
 * max ||b||^2 <= 2^24, both checked on the device in integers; every other query of the same
 * launch group is scanned on the fp32 rows.  No host synchronisation, nothing is rerun,
 * everything stays on the caller's stream.
 *
 * Short calls (fewer than 4 batches of at most 16 queries, k <= 16; vs_ivf_one_plan_u8) at
 * precision 0 or 2 take TWO launches per batch on the caller's stream, under either metric: the
 * coarse launch of vs_ivf_create's short calls, whose last workgroup also applies the rule above
 * to every query of the batch, and one scan launch that reads the byte rows for the queries that
 * qualify and the fp32 rows for the others.  Results, *total_candidates, the timing fields and
 * vs_ivf_nd_u8_stats are those of the group route; vs_ivf_one_u8_stats counts the route's
 * batches, vs_ivf_one_stats keeps counting the fp32 route only (precision 1).  The first
 * inner-product call of an index builds the rows' byte sums with one more launch, as on the
 * group route.  An index whose byte copy was not kept behaves as vs_ivf_create's.
 * VSEARCH_IVF_ONE_U8=0 at creation keeps the group route for short calls (the comparison
 * toggle); VSEARCH_IVF_ONE=0 turns both short routes off.  (One more value exists for the
 * benchmark only: VSEARCH_IVF_ONE_U8=2 sends every shape of vs_ivf_one_plan's rule to the byte
 * route, the shapes vs_ivf_one_plan_u8 takes out included, so that they can be timed on it; an
 * index created under it does not decide through vs_ivf_one_plan_u8.)  The scratch is the short
 * calls' own, once per index: calls on ONE index must be ordered by their streams.
 *
 * Accepted and refused calls: as vs_ivf_create's general index, except vs_set_precision: 0
 * (default) and 2 use the byte rows for the queries that qualify, 1 scans every pair on the fp32
 * rows, 2 returns VS_ERR_UNSUPPORTED when the byte copy was not kept.  vs_ivf_save writes float
 * arrays: vs_ivf_load of them gives an fp32 general index. */
VS_API int vs_ivf_create_nd_u8(const uint8_t* vectors_reordered, int64_t n_rows, int dim,
                               const float* centroids, int nlist, const int32_t* cluster_offsets,
                               const int32_t* reorder_to_original, int device, vs_index** out);

/* GPU index builder, the device side of build_ivf_index_reordered (create_ivf_model_reordered.py:82-177):
 * Lloyd k-means under L2 with sklearn's stopping rule (sum of squared centre shifts <= tol * mean feature
 * variance, default tol 1e-4, max_iter 100 in the reference, :97-103).  Assignment runs on the MFMA scan
 * kernel, the update uses fixed-point integer atomics (deterministic).  Initial centres: k-means++ (D^2 sampling
 * on the GPU, sklearn's default init; its RNG stream and greedy multi-trial variant are not reproduced, so the
 * centres are statistically, not bitwise, sklearn's; VSEARCH_KMEANS_INIT=random = nlist distinct random rows).
 * Outputs: centroids_out [nlist x dim], assign_out [n_rows] (cluster of every row); vs_ivf_layout turns the
 * assignment into the reordered layout of :108-128, vs_ivf_build_index does all of it.
 *
 * What a build computes, exactly (tests/test_gpu_ivf_build.py replays it on the CPU):
 *   - seeding stream: splitmix64 with state s0 = seed * 0x9E3779B97F4A7C15 + 0x1234567 (mod 2^64); next() is
 *     s += 0x9E3779B97F4A7C15; z = s; z = (z ^ z >> 30) * 0xBF58476D1CE4E5B9; z = (z ^ z >> 27) * 0x94D049BB133111EB;
 *     return z ^ z >> 31.
 *   - k-means++: centre 0 is row next() % n_rows.  Every further centre c draws one u = (next() >> 11) * 2^-53 and is the
 *     first row (in row order) at which the running sum of D^2 (squared distance to the nearest earlier centre, summed in
 *     double) exceeds u * total; when every D^2 is zero it is the last row.  A row with D^2 = 0 is never drawn while
 *     another row has D^2 > 0.  (D^2 is summed per block of 1024 rows; on data whose sums round, the running sum inside
 *     the chosen block may stay under the target, and the centre is then that block's last row with D^2 > 0.  With
 *     exact sums, e.g. integer-valued rows with distances below 2^24, this cannot happen.)
 *   - VSEARCH_KMEANS_INIT=random (read at every call): centre c is row next() % n_rows, drawn again while that row
 *     number was already taken.
 *   - assignment: the nearest centroid under fp32 ||x||^2 + ||c||^2 - 2 x.c; equal distances go to the lower centroid id.
 *   - update: with A = the cluster's sum of rint(x * 2^20), accumulated exactly in 64-bit integers (order independent),
 *     centroid = (float)((double)A / 2^20 / count): the conversion of A (exact while |A| < 2^53, e.g. integer-valued
 *     rows, whose A has 20 zero low bits), one double division and one cast to float.  For rows on the 2^-20 grid with
 *     |A| < 2^53 that is float(double(sum) / count); in general each component is within 2^-21 + 2^-24 |mean| of the
 *     mean.  A cluster without rows keeps its centroid.
 *   - max_iter = 0 returns the seeds and the assignment to them, *iters_done = 0.
 *   - *iters_done = the number of updates performed: update t (t = 1, 2, ...) moves the centroids by s_t = the sum of
 *     squared shifts; the build stops after the first update with s_t <= tol * mean per-feature variance (population
 *     variance of every column, averaged over the columns) and reports that t, or max_iter when none qualifies.  With
 *     tol = 0 it stops after the first update that moves nothing.  assign_out is the assignment to the returned
 *     centroids.
 *   - limits, checked on the host before any device work (VS_ERR_INVALID, nothing written to the outputs): every value
 *     finite, and n_rows * (max|x| + 2^-21) < 2^43, the range in which the 64-bit fixed-point sums cannot wrap.
 *   - nlist > n_rows or max_iter < 0: VS_ERR_INVALID; dim != 128: VS_ERR_UNSUPPORTED. */
VS_API int vs_ivf_build(const float* base_host, int64_t n_rows, int dim, int nlist, int max_iter, double tol,
                        uint64_t seed, int device, float* centroids_out, int32_t* assign_out, int* iters_done);

/* The host side of the same builder (no GPU needed).  vs_ivf_clamp_nlist: the nlist rule of :92-94
 * (nlist > N/10 -> max(16, N/100)).  vs_ivf_layout: :108-128 -- rows sorted by cluster id (stable), cluster_offsets
 * [nlist+1] = running sum of the cluster sizes, reorder_to_original [n_rows] = the sort permutation
 * (vectors_reordered[i] = base[reorder_to_original[i]]). */
VS_API int vs_ivf_clamp_nlist(int64_t n_vectors, int nlist);
VS_API int vs_ivf_layout(const int32_t* assign, int64_t n_rows, int nlist, int32_t* cluster_offsets,
                         int32_t* reorder_to_original);

/* build_ivf_index_reordered end to end (:82-177): nlist clamp, k-means (vs_ivf_build), reordered layout, and the
 * resulting index resident on `device`; vs_ivf_save then writes the reference's directory.  No Python involved. */
VS_API int vs_ivf_build_index(const float* base_host, int64_t n_rows, int dim, int nlist, int max_iter, double tol,
                              uint64_t seed, int device, vs_index** out, int* iters_done);

/* The builder at any dimension 1 <= dim <= 2048: vs_ivf_build's contract, word for word (seeding stream, k-means++ pick
 * rule over blocks of 1024 rows with its all-zero fallback, VSEARCH_KMEANS_INIT=random, ties to the lower centroid id,
 * 2^20 fixed-point update with (float)((double)A / 2^20 / count), empty clusters keep their centroid, max_iter = 0, the
 * meaning of *iters_done, the stopping rule), with these additions.
 *   - dim == 128 runs vs_ivf_build itself: the same launches, the same outputs.  VSEARCH_BUILD_ND_FORCE=1 (read at every
 *     call of the two _nd entry points; off by default) runs the general builder at dim 128 too: the comparison toggle,
 *     as VSEARCH_ND_FORCE and VSEARCH_IVF_ND_FORCE are for the searches.
 *   - assignment: the distance of row x to centroid c is bit for bit the number the general brute-force scan
 *     (vs_bf_create_nd's fp32 index) returns for that pair -- one fp32 accumulation chain in k order over the rows zero
 *     padded to a multiple of 16 floats, then fma(-2, dot, ||c||^2 + ||x||^2) with both norms in the reference's order
 *     (8 FMA lanes over v[8 i + j], r0 + ... + r7, then the tail).  It is also the coarse score of c for query x in a
 *     general IVF index (vs_ivf_create).
 *   - k-means++ D^2 = max(fma(-2, x.c, ||x||^2 + ||c||^2'), 0), summed in double per block of 1024 rows.  ||x||^2 is the
 *     norm above.  x.c and ||c||^2' are summed in fp32 as follows, with the vectors zero padded to a multiple of 16
 *     floats and cut into chunks of 4 floats: partial sum p_s, s = 0..7, is one fmaf chain from 0 over chunks s, s + 8,
 *     s + 16, ... (the four elements of a chunk in order); the result is ((p0 + p1) + (p2 + p3)) + ((p7 + p6) + (p5 + p4)).
 *     At dim 128 this is vs_ivf_build's order.  Deterministic from run to run.
 *   - sum of squared shifts of an update, per centroid in fp32: partial sum q_t, t = 0..127, adds the squared shifts of
 *     columns t, t + 128, ... in that order; the 128 partial sums are folded in halves (q_t += q_{t + 64}, then 32, ...,
 *     1).  The per-centroid sums are added in double in centroid order.  At dim 128 this is vs_ivf_build's order.
 * Checks, in this order (the first five need no device; nothing is written to the outputs on any failure): null
 * pointers, n_rows <= 0, nlist <= 0, nlist > n_rows or max_iter < 0 -> VS_ERR_INVALID; dim < 1 -> VS_ERR_INVALID;
 * dim > 2048 -> VS_ERR_UNSUPPORTED; a non-finite value -> VS_ERR_INVALID; n_rows * (max|x| + 2^-21) >= 2^43 ->
 * VS_ERR_INVALID; then the device. */
VS_API int vs_ivf_build_nd(const float* base_host, int64_t n_rows, int dim, int nlist, int max_iter, double tol,
                           uint64_t seed, int device, float* centroids_out, int32_t* assign_out, int* iters_done);

/* vs_ivf_build_index at any dimension: nlist clamp, vs_ivf_build_nd, vs_ivf_layout, and the index resident on `device`:
 * a general IVF index at dim != 128, the specialised one at 128 (see vs_ivf_create).  vs_ivf_save / vs_ivf_load handle
 * both. */
VS_API int vs_ivf_build_index_nd(const float* base_host, int64_t n_rows, int dim, int nlist, int max_iter, double tol,
                                 uint64_t seed, int device, vs_index** out, int* iters_done);

/* Device time in ms of the assignment pass that closed the calling thread's last successful build (any of the four
 * builders): the two scan launches and the resets before them, between two events.  0 before the first build.  For
 * scripts/ivf_nd_bench.py --build. */
VS_API double vs_ivf_build_last_assign_ms(void);

/* Writes the index held by h in the reference's directory format: unpadded [n_rows][dim] and [nlist][dim] arrays at
 * any dimension; vs_ivf_load of that directory gives the same index. */
VS_API int vs_ivf_save(vs_index* h, const char* index_dir);

/* IVFIndex::searchBatch (IVFIndex.h:45-48, IVFIndex.cpp:640-859): ids/dists
 * [nq x k] (L2: ascending distance; ids are original row numbers), returns the
 * total number of candidates scanned through *total_candidates (the
 * function's return value in the reference) and the SearchTiming fields.
 * k: 1..128.  17 <= k <= 128 needs the list-major pipeline (nlist <= 4096, rows resident): VS_ERR_UNSUPPORTED
 * otherwise, and for k > 128.  Slots past the candidates of the probed lists are (-1, +inf) for every k.
 * A general IVF index (dim != 128, see vs_ivf_create) takes 1 <= k <= 16. */
VS_API int vs_ivf_search(vs_index* h, const float* queries_host, int64_t nq, int k, int nprobe,
                         int32_t* ids, float* dists, int64_t* total_candidates, vs_timing* timing);

/* Device-level, asynchronous: one batch, outputs [B x k] on the device.
 * For a sharded index the outputs are this shard's local top-k (global ids).  k: as vs_ivf_search. */
VS_API int vs_ivf_search_dev(vs_index* h, const float* queries_dev, int B, int k, int nprobe,
                             int32_t* ids_dev, float* dists_dev, void* stream);

/* The batch loop of main_ivf.cpp:150-214 with the queries already on the device: n_batches independent
 * batches [n_batches][B][dim] -> [n_batches][B][k].  Every kernel of the pipeline is launched once for a
 * launch group of up to 32 batches (1024 queries share ONE list-major pass over the probed lists), and the
 * groups of a call are dealt to two internal streams that fork from and join `stream`: pass as many batches
 * per call as there are (128 batches per call: 13.6 M QPS at nlist 1024 / nprobe 32; 32 per call: 10.9 M).
 * k: as vs_ivf_search (17 <= k <= 128 takes a pipeline of its own: bound from the k-th of the segments' distances,
 * wide-k ranking; the k <= 16 path is not affected). */
VS_API int vs_ivf_search_dev_multi(vs_index* h, const float* queries_dev, int n_batches, int B, int k, int nprobe,
                                   int32_t* ids_dev, float* dists_dev, void* stream);

/* IVF search for 1 <= k <= 128 on EVERY IVF index.  Signatures, output layouts ([nq][k], [n_batches][B][k]),
 * *total_candidates and the timing fields are those of vs_ivf_search / vs_ivf_search_dev_multi; slots past the
 * candidates of the probed lists are (-1, +inf).  k < 1 -> VS_ERR_INVALID, k > 128 -> VS_ERR_UNSUPPORTED, a brute-force
 * index -> VS_ERR_UNSUPPORTED.
 *   k <= 16 on any IVF index, and every k on the specialised 128-d index: the call IS vs_ivf_search /
 *     vs_ivf_search_dev_multi (same launches, same results, same refusals).
 *   17 <= k <= 128 on a general IVF index (dim != 128; vs_ivf_create, vs_ivf_load, vs_ivf_build_index_nd,
 *     vs_ivf_create_nd_u8): the wide-k pipeline of DESIGN.md 4.6c, in launch groups of up to 32 batches on the caller's
 *     stream, without a host synchronisation.  The result is the k best rows of the probed lists by (distance, position
 *     in vectors_reordered), ids through reorder_to_original; every distance is bit-identical to what vs_bf_create_nd's
 *     fp32 index returns for that row and query.  Wide k scans the fp32 rows whatever vs_set_precision says, also on a
 *     vs_ivf_create_nd_u8 index (as vs_bf_search_topk does for brute force): on data that qualifies for the byte rows
 *     the distances are the same numbers, so the result does not depend on it.  The first such call allocates about
 *     66 MB of device scratch. */
VS_API int vs_ivf_search_topk(vs_index* h, const float* queries_host, int64_t nq, int k, int nprobe,
                              int32_t* ids, float* dists, int64_t* total_candidates, vs_timing* timing);
VS_API int vs_ivf_search_topk_dev_multi(vs_index* h, const float* queries_dev, int n_batches, int B, int k, int nprobe,
                                        int32_t* ids_dev, float* dists_dev, void* stream);

/* IVF search under a metric given per call, for 1 <= k <= 128 on EVERY IVF index.  Signatures, output layouts,
 * *total_candidates (the rows of the probed lists: it does not depend on the metric) and the timing fields are those of
 * vs_ivf_search_topk / vs_ivf_search_topk_dev_multi, with `metric` added.
 * Checks, in this order: null pointers -> VS_ERR_INVALID; a brute-force index -> VS_ERR_UNSUPPORTED; a metric other than
 * VS_METRIC_L2 / VS_METRIC_IP -> VS_ERR_INVALID; k < 1 -> VS_ERR_INVALID; k > 128 -> VS_ERR_UNSUPPORTED; then those of
 * vs_ivf_search_topk*.
 * The call's metric decides.  What vs_ivf_set_metric left on the index does not enter the result and is the same after
 * the call as before it, also when the call fails (the call is not reentrant on one index, like every other call).
 *   VS_METRIC_L2 on any IVF index: the call IS vs_ivf_search_topk / vs_ivf_search_topk_dev_multi on an index whose
 *     metric is L2 (same launches, same results, same refusals).
 *   VS_METRIC_IP on the specialised 128-d index: exactly what vs_ivf_set_metric(h, VS_METRIC_IP) followed by
 *     vs_ivf_search_topk* returns.
 *   VS_METRIC_IP on a general IVF index (dim != 128; vs_ivf_create, vs_ivf_load, vs_ivf_build_index_nd,
 *     vs_ivf_create_nd_u8, and the VSEARCH_IVF_ND_FORCE=1 form): the reference's own IVF ranking (IVFIndex.cpp:449-496,
 *     :697-723, :738-771) at any dimension, in launch groups of up to 32 batches on the caller's stream, without a host
 *     synchronisation.  The score of list c is -(q.c), the number the brute-force general scan returns
 *     under VS_METRIC_IP for the centroid as a row; the nprobe smallest are taken by (score, list id).  A row scores
 *     s = -(q.v), bit-identical to what the device calls of vs_bf_create_nd(..., VS_METRIC_IP, ...) return for that row
 *     and query.  The result is the k best rows of the probed lists by (s, position in vectors_reordered), ids through
 *     reorder_to_original; slots past the candidates are (-1, +inf).  The device call returns s ascending; the host call
 *     returns q.v = -s descending and +inf in empty slots, as the 128-d index does.  A product that is exactly zero
 *     gives s = -0.0 (sign bit set) on the device.
 *     On a vs_ivf_create_nd_u8 index and k <= 16, the pairs of the queries that qualify (the L2 rule, unchanged: every
 *     value an integer in [0, 255] and ||q||^2 + max ||b||^2 <= 2^24) are scanned on the byte rows with int8 MFMA and
 *     every other pair on the fp32 rows, with the same bits either way; vs_set_precision 0 and 2 do so, 1 puts every pair
 *     on the fp32 rows; 17 <= k <= 128 reads the fp32 rows.  The first inner-product call on such an index builds one
 *     int32 per row on the device (the sum of the row's stored bytes).  vs_ivf_nd_u8_stats and vs_ivf_nd_widek_stats
 *     count these calls like the L2 ones. */
VS_API int vs_ivf_search_metric(vs_index* h, const float* queries_host, int64_t nq, int k, int nprobe, int metric,
                                int32_t* ids, float* dists, int64_t* total_candidates, vs_timing* timing);
VS_API int vs_ivf_search_metric_dev_multi(vs_index* h, const float* queries_dev, int n_batches, int B, int k, int nprobe,
                                          int metric, int32_t* ids_dev, float* dists_dev, void* stream);

/* ---------------------------------------------------------------- multi-GPU */
/* Which rank owns which inverted list in a cluster-sharded index (host only, no GPU needed):
 * lists sorted by length, longest first, dealt round-robin -> owner_out[nlist] in [0, world).
 * vs_ivf_create / vs_ivf_load use exactly this assignment. */
VS_API int vs_ivf_list_owners(const int32_t* cluster_offsets, int nlist, int world, int32_t* owner_out);

/* Merge G per-shard sorted lists (e.g. the receive buffer of an RCCL
 * all-gather) into [B x kout] by (dist, id) ascending.  Entry (g, b, j) lives
 * at g*stride_g + b*kin + j in both arrays; stride_g = 0 means the dense
 * layout B*kin.  Runs on the current device, asynchronously on `stream`.
 *   Input.  Each list (g, b) is ascending by (dist, id).  A list ends at its first entry whose distance is not
 *     < +inf (+inf or NaN) or whose id is negative; whatever follows in that list is ignored (it is read, never used).
 *     The ids of one query are distinct across its G lists and lie in [0, 2^31 - 2]; the result is unspecified
 *     otherwise (2^31 - 1 is taken as "none", and the kernels disagree on repeated ids).  The inputs are not written.
 *   Output.  Row b holds the kout smallest of the pooled entries of query b by (dist, id): equal distances
 *     (-0.0 == +0.0) are ordered by ascending id, and each output distance carries the bits of the entry it came from
 *     (zero signs, subnormals and -inf included).  Slots past the pooled entries are (+inf, -1); kout may exceed kin
 *     and G*kin.
 *   flags_dev (may be NULL): flags[b] = 1 iff two adjacent outputs among the first min(kout, 256) have equal
 *     distances below +inf (the +inf tail is no tie; two -inf are one), else 0.  A tie further down a longer output
 *     is not looked for.
 *   Limits.  G, B, kin, kout >= 1.  stride_g is 0 or >= B*kin: VS_ERR_INVALID otherwise (a smaller stride would alias
 *     the groups).  G*kin <= 4096 takes any G; above that G <= 16384, else VS_ERR_UNSUPPORTED.  All of these are
 *     refused before any device work.
 * vs_topk_merge_plan (host only, no GPU needed) tells which kernel a shape runs on, so that a test can assert the
 * precondition of the path it is about: out[0] = 0 for the compacting kernel (G*kin <= out[1]; it pools a query's
 * entries on chip and ranks them by their number), else the lists per thread of the list-head kernel (1, 2, 4, 8, 16,
 * 32 or 64: the smallest power of two with 256*out[0] >= G); out[1] = 4096, the compacting kernel's capacity; out[2] =
 * 256, the outputs among which flags looks for a tie.  It refuses what vs_topk_merge_dev refuses for (G, kin, kout),
 * with the same codes; the launch goes through the same rule. */
VS_API int vs_topk_merge_dev(const float* dists_dev, const int32_t* ids_dev, int G, int B, int kin,
                             int64_t stride_g, int kout, float* out_dists_dev, int32_t* out_ids_dev,
                             int32_t* flags_dev, void* stream);
VS_API int vs_topk_merge_plan(int G, int kin, int kout, int64_t* out /* [3] */);

/* One process per GPU.  A vs_comm owns an RCCL communicator over the ranks of the job, a stream for
 * the collective and the exchange buffers.  Bootstrap like any NCCL program: rank 0 calls vs_comm_unique_id and
 * hands the VS_COMM_ID_BYTES bytes to the other ranks by whatever channel the host program has (MPI, a pipe, a file,
 * torch.distributed's store), then EVERY rank calls vs_comm_create (collective).  RCCL is loaded on first use
 * (dlopen of librccl.so.1): single-GPU users never need it.  The reference is single device; this replaces nothing
 * there -- it is the north-star's "cluster-sharded IVF / row-sharded brute force over the 8 GPUs of a node". */
#define VS_COMM_ID_BYTES 128
typedef struct vs_comm vs_comm;
VS_API int vs_comm_unique_id(void* id_out /* VS_COMM_ID_BYTES */);
VS_API int vs_comm_create(const void* unique_id, int rank, int world, int device, vs_comm** out);
VS_API int vs_comm_rank(const vs_comm* c);
VS_API int vs_comm_world(const vs_comm* c);
VS_API void vs_comm_destroy(vs_comm* c);

/* Sharded search, collective over the communicator: every rank passes the SAME queries (device memory) and its own
 * shard -- vs_bf_create(rows of this rank, id_offset = first row) or vs_ivf_create/load(..., rank, world) -- and every
 * rank receives the merged global result.  Per launch group of up to 32 batches: local scan -> ONE ncclAllGather of
 * the per-shard top-(k+1) [brute force] / top-k [IVF] lists (dists and ids as 32-bit words) -> device merge by
 * (dist, id); all-gather + merge of group g run on the communicator's stream beside the local scan of group g + 1.
 * Outputs and flags as vs_bf_search_dev_multi / vs_ivf_search_dev_multi (flags = 2: no shard produced a result for
 * the query because the int8 path skipped its batch).  Asynchronous on `stream`. */
VS_API int vs_bf_search_dev_sharded(vs_index* h, vs_comm* c, const float* queries_dev, int n_batches, int B, int k,
                                    int32_t* ids_dev, float* dists_dev, int32_t* flags_dev, void* stream);
VS_API int vs_ivf_search_dev_sharded(vs_index* h, vs_comm* c, const float* queries_dev, int n_batches, int B, int k,
                                     int nprobe, int32_t* ids_dev, float* dists_dev, void* stream);
/* The cluster-sharded IVF call (BASELINE configs[4]; IVFIndex::searchBatch, IVFIndex.cpp:640-859, over `world` ranks).
 * A launch group is cut into `world` slices of up to 32 batches.  Rank r alone runs the per-query stages of slice r
 * (centroid scores, top-nprobe, the bound), ONE all-gather exchanges the slices' results (nprobe + 2 words per query),
 * every rank then scans its resident lists for ALL slices and ranks its candidates, and the all-gather of top-k lists
 * + merge finishes the group.  Per launch group a rank so does what an unsharded index does for ONE slice (plus the
 * ranking of every query over an eighth of the candidates).  The exchanges of group g run beside the front half of
 * group g + 1.  Indexes with nlist > 4096 or fewer lists than ranks run the whole pipeline per rank (one all-gather).
 *
 * Virtual ranks: the same pipeline for G shards (vs_ivf_create / vs_ivf_load with rank r, world G) on ONE device, driven
 * by the calling thread, the collectives no-ops (every shard writes its part of the gathered layout).  For tests and
 * for measuring a rank's cost per launch group on one GPU: rank_ms[r] (optional, G doubles) = device time of rank r's
 * two halves.
 * k: 1..16 on all three sharded IVF calls (vs_ivf_search_dev_sharded, vs_ivf_search_dev_vshards, vs_ivf_search_sharded):
 * VS_ERR_UNSUPPORTED for k >= 17 (their exchange and merge are laid out for top-16). */
/* Host-side arithmetic of the sliced pipeline (no device needed).  vs_ivf_shard_group: batches per launch group of an index
 * created with `world`.  vs_ivf_shard_slice: a group of n_batches batches is cut into `world` slices of *slice_batches
 * batches (the last ones may be short or empty); rank's own slice is [*first_batch, *first_batch + *own_batches).
 * vs_ivf_shard_block_words: 32-bit words of the block a rank contributes to the exchange between the two halves:
 * probes [slice_batches * 32][nprobe] (int32, batch padded) | bounds [slice_batches * 32] (f32) | slow marks [.. * 32]. */
VS_API int vs_ivf_shard_group(int world);
VS_API int vs_ivf_shard_slice(int n_batches, int world, int rank, int32_t* slice_batches, int32_t* first_batch, int32_t* own_batches);
VS_API int64_t vs_ivf_shard_block_words(int slice_batches, int nprobe);
VS_API int vs_ivf_search_dev_vshards(vs_index* const* shards, int G, const float* queries_dev, int n_batches, int B, int k,
                                     int nprobe, int32_t* ids_dev, float* dists_dev, double* rank_ms, void* stream);

/* Host-buffer forms (what the CLIs run with --gpus N): same contract, queries and results in host memory on every
 * rank.  Brute force returns what vs_bf_search returns on one GPU -- the reference's answer (cpu_baseline.cpp:127-153):
 * a chunk whose int8 scan was skipped on some shard (merged flag 2) is rerun on the fp32 rows by every rank, and
 * queries with a tie inside the k+1 best are re-resolved exactly: shard 0's first rows are taken densely, their k-th
 * smallest distance bounds select_topk's buffer maximum for every later row, every shard filters its rows under that
 * bound, the candidates are exchanged (all-gathers of fixed-size buffers) and every rank replays the slots over "dense
 * rows, then candidates in row order".  Shards must be contiguous row ranges in rank order.
 * IVF: vs_ivf_search's chunk pipeline (the same chunks, timing fields and inner-product sign) with the device-sharded
 * search as its launch step; *total_candidates = rows scanned by THIS rank's shard.
 * vs_bf_search_vshards: the brute-force call for G shards on ONE device, driven by the calling thread (no collective):
 * tests of the sharded tie order without a multi-GPU node. */
VS_API int vs_bf_search_sharded(vs_index* h, vs_comm* c, const float* queries_host, int64_t nq, int k, int32_t* ids,
                                float* dists, vs_timing* timing);
VS_API int vs_ivf_search_sharded(vs_index* h, vs_comm* c, const float* queries_host, int64_t nq, int k, int nprobe,
                                 int32_t* ids, float* dists, int64_t* total_candidates, vs_timing* timing);
VS_API int vs_bf_search_vshards(vs_index* const* shards, int G, const float* queries_host, int64_t nq, int k, int32_t* ids,
                                float* dists, vs_timing* timing);

/* ------------------------------------------------------------------ profiling */
/* HIP-event timing of the dominant scan kernel on the stream it is launched on
 * (bench.py's roofline leg).  which: 0 = brute-force scan, 1 = IVF list scan. */
VS_API int vs_prof_enable(vs_index* h, int on);
VS_API int vs_prof_read(vs_index* h, int which, double* total_ms, int64_t* launches);
/* Diagnostics of the wide-k IVF pipeline (17 <= k <= 128), collected only when the environment variable
 * VSEARCH_IVF_WIDEK_STATS=1 was set at the index's first wide-k call: out[0] = candidates ranked (queries ranked from
 * their candidate lists), out[1] = the most candidates of one such query, out[2] = queries ranked exactly over every row
 * of their probed lists (no bound, or a candidate list overflowed), out[3] = launch groups whose candidate buffers
 * overflowed (all their queries ranked exactly).  Synchronises the device; reset != 0 clears the counters. */
VS_API int vs_ivf_widek_stats(vs_index* h, int64_t* out /* [4] */, int reset);
/* Which rows the list scan of a vs_ivf_create_nd_u8 general index read: out[0] = (query, probe) pairs that got a slot in
 * the byte plan since the last reset, out[1] = the same for the fp32 plan (pairs that probe an empty list get neither).
 * Always counted.  Synchronises the device; reset != 0 clears the counters.  VS_ERR_INVALID on any other kind of index. */
VS_API int vs_ivf_nd_u8_stats(vs_index* h, int64_t* out /* [2] */, int reset);
/* The two-launch route of short calls on a general IVF index (host only, no GPU needed): the rule for a launch
 * group of n_batches batches of B queries for k neighbours in nprobe lists (clamped to nlist) on an index of n_rows rows
 * of dim floats in nlist lists on a device of num_cus compute units; the launch code takes its decision and geometry
 * through the same function.
 *   out[0] = 0: the group route; 1: the two-launch route -- all of n_batches < 4, B <= 16, k <= 16,
 *            min(nprobe, nlist) <= 256, n_rows < 2^31 - 128 and nlist <= 1024 (the coarse launch's last workgroup selects
 *            the probes from [16][1024] scores in its LDS; above that the call keeps the group route)
 *   out[1] = workgroups of the coarse launch
 *   out[2] = rows in one unit of the scan: a probed list is cut into units of at most this many rows, a multiple of 64
 *            counted from the list's first row
 *   out[3] = workgroups of the scan launch
 * out[1..3] are 0 with out[0] = 0.  It describes the default rule: VSEARCH_IVF_ONE=0 and the byte copy of a
 * vs_ivf_create_nd_u8 index are not its business.
 * Checks, in this order: null out, n_rows < 1, nlist < 1, num_cus < 1, n_batches < 1, B outside [1, 32], k < 1,
 * nprobe < 1 -> VS_ERR_INVALID; dim < 1 -> VS_ERR_INVALID; dim > 2048 -> VS_ERR_UNSUPPORTED; k > 128 -> VS_ERR_UNSUPPORTED. */
VS_API int vs_ivf_one_plan(int64_t n_rows, int dim, int nlist, int num_cus, int n_batches, int B, int k, int nprobe,
                           int64_t* out /* [4] */);
/* What that route did on a general IVF index since the last reset: out[0] = batches answered by the two launches,
 * out[1] = the most units any one of those batches had (written by the coarse launch).  Always counted; zeros before the
 * first short call.  Synchronises the device; reset != 0 clears the counters.  VS_ERR_INVALID on any other kind of index. */
VS_API int vs_ivf_one_stats(vs_index* h, int64_t* out /* [2] */, int reset);
/* The byte route of short calls on a general IVF index that keeps a byte copy of its rows (vs_ivf_create_nd_u8 at
 * precision 0 or 2; host only, no GPU needed): the rule for the same launch group as vs_ivf_one_plan, and the launch
 * code takes its decision and geometry through the same function.
 *   out[0] = 0: the group route; 2: the two-launch byte route.  The default rule is vs_ivf_one_plan's own conditions:
 *            n_batches < 4, B <= 16, k <= 16, min(nprobe, nlist) <= 256, nlist <= 1024, n_rows < 2^31 - 128.  A shape
 *            leaves the rule only because it MEASURED slower than the route it would replace.  Two have, at 1 M rows,
 *            nlist 1024, k = 10 (byte route | group route | fp32 two launches, us per call): dim 96, B = 16, nprobe 128:
 *            345 | 330 | 369; dim 128, B = 16, nprobe 256: 446 | 441 | 488.  Exactly these two shapes (nprobe after the
 *            clamp to nlist) keep the group route; every measured neighbour was faster than both alternatives.  One shape
 *            stays in although the fp32 two launches were 1.6 % faster, because the group route is what it would get
 *            instead: dim 96, B = 1, nprobe 8: 87.7 | 157.0 | 86.2 (profiles/ivf_one_u8_bench.txt)
 *   out[1] = workgroups of the coarse launch
 *   out[2] = rows in one BYTE unit of the scan (a multiple of 64 counted from the list's first row); the fp32 units of
 *            the same batch have vs_ivf_one_plan's out[2] rows
 *   out[3] = workgroups of the scan launch
 * out[1..3] are 0 with out[0] = 0; out[1] and out[3] equal vs_ivf_one_plan's wherever both say "short".  VSEARCH_IVF_ONE=0,
 * VSEARCH_IVF_ONE_U8=0 (and its benchmark-only value 2, see vs_ivf_create_nd_u8), the precision and whether the byte
 * copy was kept are not its business.
 * Checks, codes and their order: vs_ivf_one_plan's. */
VS_API int vs_ivf_one_plan_u8(int64_t n_rows, int dim, int nlist, int num_cus, int n_batches, int B, int k, int nprobe,
                              int64_t* out /* [4] */);
/* What the byte route did on such an index since the last reset: out[0] = batches answered by it, out[1] = of those,
 * batches that held both byte units and fp32 units (queries of both kinds that probe lists with rows), out[2] = the most
 * units, both kinds together, any one of those batches had (all three written by the coarse launch).  Always counted;
 * zeros before the first such call.  Synchronises the device; reset != 0 clears the counters.  VS_ERR_INVALID for null
 * pointers and on any index that is not a general IVF index with a byte copy of its rows. */
VS_API int vs_ivf_one_u8_stats(vs_index* h, int64_t* out /* [3] */, int reset);
/* The wide-k calls (17 <= k <= 128) on a general IVF index since the last reset: out[0] = candidates ranked from
 * candidate lists, out[1] = the most candidates of one query, out[2] = queries ranked by the exact fallback (more than
 * 8192 candidates: every row of their probed lists scored again).  Always counted; zeros before the first wide-k call.
 * Synchronises the device; reset != 0 clears the counters.  VS_ERR_INVALID on any other kind of index. */
VS_API int vs_ivf_nd_widek_stats(vs_index* h, int64_t* out /* [3] */, int reset);
/* per-launch durations (ms) of the same window, oldest first; *launches = how many there were (may exceed cap).
 * One brute-force launch serves up to 32 batches: the CLIs turn these into the per-batch statistics of
 * main.cpp:262-330 (avg / stddev / min / max / P50 / P95 / P99 "graph execute time"). */
VS_API int vs_prof_read_launches(vs_index* h, int which, double* ms_out, int64_t cap, int64_t* launches);

VS_API int64_t vs_index_rows(const vs_index* h);
VS_API int vs_index_dim(const vs_index* h);
VS_API int vs_index_nlist(const vs_index* h);     /* 0 for brute force */
/* The error bound E of the bf16 prefilter of the fp32 brute-force scan: |fp32 dot - bf16 MFMA dot| <= E for a
 * query with ||q|| = nq, ||bf16(q)|| = nqp, ||q - bf16(q)|| = eq against a shard with max ||b|| = bmax, max ||b - bf16(b)||
 * = emax, max ||bf16(b)|| = bpmax, as the library computes it (rounded up to float).  Pure host arithmetic. */
VS_API float vs_f32_filter_bound(double eq, double nq, double nqp, double bmax, double emax, double bpmax);
/* Diagnostic read-back of the bf16 row image of the prefilter: rows [row0, row0 + n) of the image, 128
 * uint16 each, to dst (host memory); the 64 zero spare rows behind the index's last row can be read as well.
 * VS_ERR_INVALID when the index has no image (not a 128-d brute-force index, too small for the prefilter, ill-scaled
 * rows, VSEARCH_F32_FILTER=0) or the range leaves it. */
VS_API int vs_bf_filter_image_read(const vs_index* h, int64_t row0, int64_t n, uint16_t* dst);
/* The L2 test of the prefilter carries the row norm through the MFMA's C operand: a value S'' = bf16 dot -
 * norm / 2 passes when it is above th2.  vs_f32_filter_cnorm: the shard constant C of that test from the shard's largest
 * stored fp32 norm.  vs_f32_filter_th2: the bound th2 from the exact scan's hot-test bound thr (a row passes the exact
 * scan when RN(norm - 2 dot) < thr), the query's E (vs_f32_filter_bound) and C, as the library computes it (rounded
 * down).  Pure host arithmetic. */
VS_API float vs_f32_filter_cnorm(double bnmax);
VS_API float vs_f32_filter_th2(float thr, float e, float cnorm);
/* Counters of the prefilter since the index was created or last reset (waits for the device): out[0] = launches that took
 * the prefilter, out[1] = of those, launches whose candidate buffers overflowed (the exact fallback scan behind produced
 * their results), out[2] = candidates written by the sweeps, out[3] = candidates that survived the exact recheck.
 * VS_ERR_INVALID when the index has no prefilter (see vs_bf_filter_image_read). */
VS_API int vs_bf_filter_stats(vs_index* h, int64_t* out /* [4] */, int reset);
VS_API void vs_destroy(vs_index* h);

#ifdef __cplusplus
}
#endif
#endif /* VSEARCH_H */
