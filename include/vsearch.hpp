// vsearch.hpp -- header-only C++ host layer over the C ABI (vsearch.h).
//
// Mirrors the reference's C++ operator interfaces so that a caller of the reference can switch
// with the same names, argument meaning and error behaviour:
//   vsearch::read_fvecs / load_ivecs   <- cpu/cpu_baseline.cpp:31-58, main_ivf.cpp:35-50
//   vsearch::ExactSearch               <- the query loop of run_benchmark (cpu_baseline.cpp:209-254)
//                                         with QnnRunner-style getters (QnnRunner.h:37-39)
//   vsearch::QuantizedRunner           <- class QnnRunner (qidk_bruteforce QnnRunner.h:18-55), UFIXED_POINT_8 I/O
//   vsearch::IVFIndex                  <- class IVFIndex (IVFIndex.h:14-97): search / searchBatch /
//                                         SearchTiming / getNumVectors / getNumClusters / getDim
// Errors: the IVF side throws std::runtime_error like the reference (IVFIndex.cpp:184-198,
// main_ivf.cpp:287-290); the exact-search side returns bool like cpu_baseline.cpp:194-207.
#pragma once
#include <algorithm>
#include <array>
#include <cstdint>
#include <stdexcept>
#include <chrono>
#include <string>
#include <vector>

#include "vsearch.h"

namespace vsearch {

inline void check(int rc) {
    if (rc != VS_OK) throw std::runtime_error(vs_last_error());
}

// cpu_baseline.cpp:31-58 -- same signature, same bool/std::cerr-free contract (message via vs_last_error)
inline bool read_fvecs(const std::string& filename, std::vector<float>& data, int& rows, int& dim) {
    int64_t r = 0;
    int d = 0;
    if (vs_fvecs_shape(filename.c_str(), &r, &d) != VS_OK) return false;
    data.resize((size_t)r * (size_t)d);
    if (r > 0 && vs_fvecs_read(filename.c_str(), data.data(), (int64_t)data.size(), &r, &d) != VS_OK) return false;
    rows = (int)r;
    dim = d;
    return true;
}

// TEXMEX .bvecs ([int32 d][d x uint8] records): read_fvecs' contract for byte vectors
inline bool read_bvecs(const std::string& filename, std::vector<uint8_t>& data, int& rows, int& dim) {
    int64_t r = 0;
    int d = 0;
    if (vs_bvecs_shape(filename.c_str(), &r, &d) != VS_OK) return false;
    data.resize((size_t)r * (size_t)d);
    if (r > 0 && vs_bvecs_read(filename.c_str(), data.data(), (int64_t)data.size(), &r, &d) != VS_OK) return false;
    rows = (int)r;
    dim = d;
    return true;
}

// main_ivf.cpp:35-50 (throws like the reference)
inline void load_ivecs(const std::string& filename, std::vector<std::vector<int>>& vectors, int& dim) {
    int64_t r = 0;
    int d = 0;
    check(vs_fvecs_shape(filename.c_str(), &r, &d));
    std::vector<int32_t> flat((size_t)r * (size_t)d);
    if (r > 0) check(vs_ivecs_read(filename.c_str(), flat.data(), (int64_t)flat.size(), &r, &d));
    vectors.assign((size_t)r, std::vector<int>((size_t)d));
    for (int64_t i = 0; i < r; ++i)
        for (int j = 0; j < d; ++j) vectors[(size_t)i][(size_t)j] = flat[(size_t)i * d + j];
    dim = d;
}

// main_ivf.cpp:52-59
inline double compute_recall(const std::vector<int>& predicted, const std::vector<int>& ground_truth, int k) {
    int hits = 0;
    const int kg = std::min<int>(k, (int)ground_truth.size());
    for (int i = 0; i < std::min<int>(k, (int)predicted.size()); ++i)
        for (int j = 0; j < kg; ++j)
            if (predicted[(size_t)i] == ground_truth[(size_t)j]) {
                ++hits;
                break;
            }
    return static_cast<double>(hits) / k;
}

struct Result {  // cpu_baseline.cpp:13-19
    float dist;
    int idx;
    bool operator<(const Result& other) const { return dist < other.dist; }
};

// Any vector length 1 <= dim <= 2048: 128-d bases take vs_bf_create, the others vs_bf_create_nd (a general index:
// one GPU, fp32 rows; the sharded calls refuse it with the library's message).  uint8 rows take vs_bf_create_nd_u8:
// at dimensions other than 128 a byte copy beside the fp32 rows, scanned with int8 MFMA for k <= 15; under VS_METRIC_IP
// (vs_bf_create_nd_u8_metric) at 128 too, as a general index.
class ExactSearch {
public:
    ExactSearch(const uint8_t* rows_u8, int64_t rows, int dim, int64_t id_offset = 0, int device = 0, int metric = VS_METRIC_L2) {
        check(vs_bf_create_nd_u8_metric(rows_u8, rows, dim, metric, device, id_offset, &h_));
    }
    ExactSearch(const std::vector<float>& base, int rows, int dim, int device = 0, int metric = VS_METRIC_L2) {
        check((dim == 128 ? vs_bf_create : vs_bf_create_nd)(base.data(), rows, dim, metric, device, 0, &h_));
    }
    // one rank's row shard of a larger base: ids are shard rows + id_offset (multi-GPU, vs_bf_search_sharded)
    ExactSearch(const float* shard, int64_t rows, int dim, int64_t id_offset, int device, int metric = VS_METRIC_L2) {
        check((dim == 128 ? vs_bf_create : vs_bf_create_nd)(shard, rows, dim, metric, device, id_offset, &h_));
    }
    ~ExactSearch() { vs_destroy(h_); }
    ExactSearch(const ExactSearch&) = delete;
    ExactSearch& operator=(const ExactSearch&) = delete;

    size_t getNumDocs() const { return (size_t)vs_index_rows(h_); }
    size_t getDim() const { return (size_t)vs_index_dim(h_); }
    void setBatchSize(int b) { check(vs_set_batch(h_, b)); }

    // all queries -> results[i] = k nearest, ascending, reference tie order
    void search(const std::vector<float>& queries, int nq, int k, std::vector<std::vector<Result>>& results,
                vs_timing* timing = nullptr) {
        std::vector<int32_t> ids((size_t)nq * k);
        std::vector<float> dists((size_t)nq * k);
        check(vs_bf_search(h_, queries.data(), nq, k, ids.data(), dists.data(), timing));
        results.assign((size_t)nq, {});
        for (int i = 0; i < nq; ++i)
            for (int t = 0; t < k; ++t)
                if (ids[(size_t)i * k + t] >= 0) results[(size_t)i].push_back({dists[(size_t)i * k + t], ids[(size_t)i * k + t]});
    }
    // the same for 1 <= k <= 128 (vs_bf_search_topk): for k >= 16 ties leave in select_topk's slot order, stably sorted
    void search_topk(const std::vector<float>& queries, int nq, int k, std::vector<std::vector<Result>>& results,
                     vs_timing* timing = nullptr) {
        std::vector<int32_t> ids((size_t)nq * k);
        std::vector<float> dists((size_t)nq * k);
        check(vs_bf_search_topk(h_, queries.data(), nq, k, ids.data(), dists.data(), timing));
        results.assign((size_t)nq, {});
        for (int i = 0; i < nq; ++i)
            for (int t = 0; t < k; ++t)
                if (ids[(size_t)i * k + t] >= 0) results[(size_t)i].push_back({dists[(size_t)i * k + t], ids[(size_t)i * k + t]});
    }
    // collective over `comm` (every rank: same queries, own shard); ties come out in (dist, id) order
    void searchSharded(vs_comm* comm, const std::vector<float>& queries, int nq, int k, std::vector<std::vector<Result>>& results,
                       vs_timing* timing = nullptr) {
        std::vector<int32_t> ids((size_t)nq * k);
        std::vector<float> dists((size_t)nq * k);
        check(vs_bf_search_sharded(h_, comm, queries.data(), nq, k, ids.data(), dists.data(), timing));
        results.assign((size_t)nq, {});
        for (int i = 0; i < nq; ++i)
            for (int t = 0; t < k; ++t)
                if (ids[(size_t)i * k + t] >= 0) results[(size_t)i].push_back({dists[(size_t)i * k + t], ids[(size_t)i * k + t]});
    }
    vs_index* handle() { return h_; }

private:
    vs_index* h_ = nullptr;
};

// QnnRunner with its UFIXED_POINT_8 I/O (qidk_bruteforce QnnRunner.h:18-55): same method names, the database is handed
// over as floats and quantised at construction (the reference bakes it into the model blob offline).
struct ExecutionTiming {  // QnnRunner.h:12-17
    double quantize_ms = 0.0;       // here: inside graph_execute_ms (the quantiser is a device launch)
    double graph_execute_ms = 0.0;
    double dequantize_ms = 0.0;
    double total_ms = 0.0;
};

class QuantizedRunner {
public:
    // enc == nullptr: the runner's hard-coded input / output scales (QnnRunner.cpp:490-521), weights min-max.
    // Any vector length 1 <= dim <= 2048: 128-d documents take vs_q8_create, the others vs_q8_create_nd.
    QuantizedRunner(const std::vector<float>& docs, int64_t rows, int dim, const vs_q8_encodings* enc = nullptr, int device = 0) {
        check((dim == 128 ? vs_q8_create : vs_q8_create_nd)(docs.data(), rows, dim, enc, device, 0, &h_));
        out_.resize((size_t)vs_q8_batch(h_) * (size_t)rows);
    }
    ~QuantizedRunner() { vs_q8_destroy(h_); }
    QuantizedRunner(const QuantizedRunner&) = delete;
    QuantizedRunner& operator=(const QuantizedRunner&) = delete;

    size_t getBatchSize() const { return (size_t)vs_q8_batch(h_); }
    size_t getDim() const { return (size_t)vs_q8_dim(h_); }
    size_t getNumDocs() const { return (size_t)vs_q8_num_docs(h_); }
    float getOutputScale() const { return vs_q8_output_scale(h_); }
    bool isFloatModel() const { return false; }

    // batch_queries: [B * dim], B <= getBatchSize() (the reference pads to the model batch with zeros, main.cpp:206-211)
    void executeBatchRaw(const std::vector<float>& batch_queries, ExecutionTiming& timing) {
        const auto t0 = std::chrono::high_resolution_clock::now();
        const int B = (int)(batch_queries.size() / getDim());
        check(vs_q8_execute(h_, batch_queries.data(), B, out_.data()));
        timing.graph_execute_ms = timing.total_ms =
            std::chrono::duration<double, std::milli>(std::chrono::high_resolution_clock::now() - t0).count();
        rows_valid_ = B;
    }
    // [B x getNumDocs()] uint8, valid until the next execute (QnnRunner.h:37)
    const uint8_t* getRawOutputBuffer() const { return out_.data(); }
    size_t getOutputSize() const { return (size_t)rows_valid_ * getNumDocs(); }

    // executeBatchRaw + find_top_k_batch_parallel (main.cpp:59-71) on the device: ids / raw scores, [nq x k]
    void search(const std::vector<float>& queries, int64_t nq, int k, std::vector<int32_t>& ids, std::vector<uint8_t>& scores) {
        ids.assign((size_t)nq * k, -1);
        scores.assign((size_t)nq * k, 0);
        check(vs_q8_search(h_, queries.data(), nq, k, ids.data(), scores.data()));
    }
    // the same for k <= 128 (k <= 16 is search itself; vsearch.h at vs_q8_search_topk_dev)
    void searchTopk(const std::vector<float>& queries, int64_t nq, int k, std::vector<int32_t>& ids, std::vector<uint8_t>& scores) {
        ids.assign((size_t)nq * std::max(k, 0), -1);
        scores.assign((size_t)nq * std::max(k, 0), 0);
        check(vs_q8_search_topk(h_, queries.data(), nq, k, ids.data(), scores.data()));
    }
    vs_q8* handle() { return h_; }

private:
    vs_q8* h_ = nullptr;
    std::vector<uint8_t> out_;
    int rows_valid_ = 0;
};

// The reference's int16 cosine score path (AMD_npu/Codes/preprocess.py:24-42, test.cpp:32-43, 285-311): rows and queries
// L2-normalised, scaled and truncated to int16, scores = the exact int32 matrix C = A B^T (scale^2 cos).
class I16Runner {
public:
    // Any vector length 1 <= dim <= 2048; scale finite and in [1, 2047] (the reference: 1000)
    I16Runner(const std::vector<float>& docs, int64_t rows, int dim, float scale = 1000.0f, int device = 0, int64_t id_offset = 0) {
        check(vs_i16_create(docs.data(), rows, dim, scale, device, id_offset, &h_));
    }
    ~I16Runner() { vs_i16_destroy(h_); }
    I16Runner(const I16Runner&) = delete;
    I16Runner& operator=(const I16Runner&) = delete;

    size_t getBatchSize() const { return (size_t)vs_i16_batch(h_); }
    size_t getDim() const { return (size_t)vs_i16_dim(h_); }
    size_t getNumDocs() const { return (size_t)vs_i16_num_docs(h_); }
    float getScale() const { return vs_i16_scale(h_); }

    // the quantiser alone, on the host: [rows * dim] int16
    static std::vector<int16_t> quantize(const std::vector<float>& x, int64_t rows, int dim, float scale = 1000.0f) {
        std::vector<int16_t> q((size_t)rows * dim);
        check(vs_i16_quantize(x.data(), rows, dim, scale, q.data()));
        return q;
    }
    // batch_queries: [B * dim], B <= getBatchSize(); scores: [B x getNumDocs()] int32, row-major
    void execute(const std::vector<float>& batch_queries, std::vector<int32_t>& scores) {
        const int B = (int)(batch_queries.size() / getDim());
        scores.resize((size_t)B * getNumDocs());
        check(vs_i16_execute(h_, batch_queries.data(), B, scores.data()));
    }
    // the k <= 16 largest scores per query, equal scores in ascending id: ids / scores [nq x k], (-1, INT32_MIN) past the rows
    void search(const std::vector<float>& queries, int64_t nq, int k, std::vector<int32_t>& ids, std::vector<int32_t>& scores) {
        ids.assign((size_t)nq * k, -1);
        scores.assign((size_t)nq * k, INT32_MIN);
        check(vs_i16_search(h_, queries.data(), nq, k, ids.data(), scores.data()));
    }
    // the same for k <= 128 (k <= 16 is search itself; vsearch.h at vs_i16_search_topk_dev)
    void searchTopk(const std::vector<float>& queries, int64_t nq, int k, std::vector<int32_t>& ids, std::vector<int32_t>& scores) {
        ids.assign((size_t)nq * std::max(k, 0), -1);
        scores.assign((size_t)nq * std::max(k, 0), INT32_MIN);
        check(vs_i16_search_topk(h_, queries.data(), nq, k, ids.data(), scores.data()));
    }
    // (sample groups, stride, candidate cap) of searchTopk at 17 <= k <= 128, on the host
    static std::array<int64_t, 3> widePlan(int64_t rows, int k) {
        std::array<int64_t, 3> out{};
        check(vs_i16_wide_plan(rows, k, out.data()));
        return out;
    }
    // (queries ranked from lists, most candidates of a query, queries of the dense fallback, queries with a whole-base sample)
    std::array<int64_t, 4> wideStats(bool reset = false) {
        std::array<int64_t, 4> out{};
        check(vs_i16_wide_stats(h_, out.data(), reset ? 1 : 0));
        return out;
    }
    vs_i16* handle() { return h_; }

private:
    vs_i16* h_ = nullptr;
};

class IVFIndex {
public:
    struct SearchTiming {  // IVFIndex.h:31-36
        double centroid_search_ms = 0.0;
        double gather_ms = 0.0;
        double fine_search_ms = 0.0;
        double total_ms = 0.0;
    };

    // backendPath is kept for signature compatibility (the reference passes libQnnHtp.so); the
    // backend here is always the HIP library this header links against.
    // The directory states the dimension (1 <= dim <= 2048, getDim()): 128-d indexes take the specialised pipeline,
    // any other a general IVF index (fp32 rows, squared L2, one GPU; k <= 16 through searchBatch, k <= 128 through
    // searchBatchTopk, inner product through searchBatchMetric; vsearch.h at vs_ivf_create).
    explicit IVFIndex(const std::string& indexDir, const std::string& backendPath = "libvsearch_hip.so",
                      int device = 0, int rank = 0, int world = 1) {
        (void)backendPath;
        check(vs_ivf_load(indexDir.c_str(), device, rank, world, &h_));
    }
    // uint8 rows in the reordered layout (vs_ivf_create_nd_u8): at dimensions other than 128 the general IVF index plus
    // a byte copy of the rows, scanned with int8 MFMA for the queries that are byte valued themselves; same results.
    IVFIndex(const uint8_t* vectorsReordered, int64_t rows, int dim, const float* centroids, int nlist,
             const int32_t* clusterOffsets, const int32_t* reorderToOriginal, int device = 0) {
        check(vs_ivf_create_nd_u8(vectorsReordered, rows, dim, centroids, nlist, clusterOffsets, reorderToOriginal, device, &h_));
    }
    ~IVFIndex() { vs_destroy(h_); }
    IVFIndex(const IVFIndex&) = delete;
    IVFIndex& operator=(const IVFIndex&) = delete;

    // One query, one answer.  On a general index (dim != 128) with k <= 16 and nlist <= 1024 this is the two-launch route
    // of short calls (vsearch.h at vs_ivf_create, vs_ivf_one_plan); same result as through searchBatch.
    size_t search(const std::vector<float>& query, int k, int nprobe, std::vector<int>& indices,
                  std::vector<float>& scores) {
        SearchTiming t;
        return search(query, k, nprobe, indices, scores, t);
    }
    size_t search(const std::vector<float>& query, int k, int nprobe, std::vector<int>& indices,
                  std::vector<float>& scores, SearchTiming& timing) {
        std::vector<std::vector<int>> ai;
        std::vector<std::vector<float>> as;
        size_t n = searchBatch(query, 1, k, nprobe, ai, as, timing);
        indices = ai[0];
        scores = as[0];
        return n;
    }
    // IVFIndex.h:45-48 -- queries holds batchSize x dim floats (zero-padded by the caller or not)
    size_t searchBatch(const std::vector<float>& queries, int batchSize, int k, int nprobe,
                       std::vector<std::vector<int>>& allIndices, std::vector<std::vector<float>>& allScores,
                       SearchTiming& timing) {
        return searchBatchWith(vs_ivf_search, queries, batchSize, k, nprobe, allIndices, allScores, timing);
    }
    // the same for 1 <= k <= 128 at every dimension (vs_ivf_search_topk): k <= 16, and every k on a 128-d index, is
    // searchBatch itself; 17 <= k <= 128 on a general index takes the wide-k pipeline
    size_t searchBatchTopk(const std::vector<float>& queries, int batchSize, int k, int nprobe,
                           std::vector<std::vector<int>>& allIndices, std::vector<std::vector<float>>& allScores,
                           SearchTiming& timing) {
        return searchBatchWith(vs_ivf_search_topk, queries, batchSize, k, nprobe, allIndices, allScores, timing);
    }
    // the same under a metric given per call (vs_ivf_search_metric; VS_METRIC_L2 or VS_METRIC_IP) on every IVF index:
    // inner product returns the scores q.v, descending, as the reference's IVFIndex does.  The index's own metric is
    // neither used nor changed.
    size_t searchBatchMetric(const std::vector<float>& queries, int batchSize, int k, int nprobe, int metric,
                             std::vector<std::vector<int>>& allIndices, std::vector<std::vector<float>>& allScores,
                             SearchTiming& timing) {
        auto call = [metric](vs_index* h, const float* q, int64_t nq, int k_, int np, int32_t* ids, float* dists, int64_t* total,
                             vs_timing* tm) { return vs_ivf_search_metric(h, q, nq, k_, np, metric, ids, dists, total, tm); };
        return searchBatchWith(call, queries, batchSize, k, nprobe, allIndices, allScores, timing);
    }

  private:
    // call: int(vs_index*, const float*, int64_t, int, int, int32_t*, float*, int64_t*, vs_timing*)
    template <class HostSearch>
    size_t searchBatchWith(HostSearch call, const std::vector<float>& queries, int batchSize, int k, int nprobe,
                           std::vector<std::vector<int>>& allIndices, std::vector<std::vector<float>>& allScores,
                           SearchTiming& timing) {
        std::vector<int32_t> ids((size_t)batchSize * k);
        std::vector<float> dists((size_t)batchSize * k);
        int64_t total = 0;
        vs_timing tm{};
        check(call(h_, queries.data(), batchSize, k, nprobe, ids.data(), dists.data(), &total, &tm));
        allIndices.assign((size_t)batchSize, {});
        allScores.assign((size_t)batchSize, {});
        for (int b = 0; b < batchSize; ++b)
            for (int t = 0; t < k; ++t)
                if (ids[(size_t)b * k + t] >= 0) {
                    allIndices[(size_t)b].push_back(ids[(size_t)b * k + t]);
                    allScores[(size_t)b].push_back(dists[(size_t)b * k + t]);
                }
        timing.centroid_search_ms = tm.centroid_search_ms;
        timing.gather_ms = tm.gather_ms;
        timing.fine_search_ms = tm.fine_search_ms;
        timing.total_ms = tm.total_ms;
        return (size_t)total;
    }

  public:
    // collective over `comm`: this index holds rank's lists (constructed with the same rank / world); returns the rows
    // scanned by THIS rank
    size_t searchBatchSharded(vs_comm* comm, const std::vector<float>& queries, int batchSize, int k, int nprobe,
                              std::vector<std::vector<int>>& allIndices, std::vector<std::vector<float>>& allScores,
                              SearchTiming& timing) {
        std::vector<int32_t> ids((size_t)batchSize * k);
        std::vector<float> dists((size_t)batchSize * k);
        int64_t total = 0;
        vs_timing tm{};
        check(vs_ivf_search_sharded(h_, comm, queries.data(), batchSize, k, nprobe, ids.data(), dists.data(), &total, &tm));
        allIndices.assign((size_t)batchSize, {});
        allScores.assign((size_t)batchSize, {});
        for (int b = 0; b < batchSize; ++b)
            for (int t = 0; t < k; ++t)
                if (ids[(size_t)b * k + t] >= 0) {
                    allIndices[(size_t)b].push_back(ids[(size_t)b * k + t]);
                    allScores[(size_t)b].push_back(dists[(size_t)b * k + t]);
                }
        timing.fine_search_ms = tm.fine_search_ms;
        timing.total_ms = tm.total_ms;
        return (size_t)total;
    }

    size_t getNumVectors() const { return (size_t)vs_index_rows(h_); }
    size_t getNumClusters() const { return (size_t)vs_index_nlist(h_); }
    size_t getDim() const { return (size_t)vs_index_dim(h_); }
    void setBatchSize(int b) { check(vs_set_batch(h_, b)); }
    vs_index* handle() { return h_; }

private:
    vs_index* h_ = nullptr;
};

}  // namespace vsearch
