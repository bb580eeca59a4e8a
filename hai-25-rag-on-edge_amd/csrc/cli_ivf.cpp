// vsearch_ivf -- drop-in for the reference's qidk_ivf CLI (main_ivf.cpp:61-293) on the MI355X backend.
//   vsearch_ivf <index_dir> <queries.fvecs> <results_dir> <backend.so> <top_k> [nprobe=16] [groundtruth.ivecs] [batch=1]
// Writes <results_dir>/results.txt and metrics.txt in the reference's layouts.  The <backend.so>
// slot is accepted and ignored (the reference passes libQnnHtp.so there).
//   ... --gpus N : one process per GPU (forked before HIP starts); every rank loads the lists it owns (longest-first
//   round robin), runs the same coarse stage and scans its lists; per-shard top-k lists meet in one RCCL all-gather per
//   32 batches (vs_ivf_search_sharded); rank 0 writes the files ("Avg candidates" is then rank 0's share).
//   ... --metric ip|l2 : the search goes through vs_ivf_search_metric with that metric, at any dimension; under ip
//   results.txt holds the scores q.v, descending, as the reference's own main_ivf prints them.  Without the flag the
//   index's own metric (squared L2) is used, as before.  Not together with --gpus N > 1.
#include <sys/stat.h>

#include <algorithm>
#include <chrono>
#include <fstream>
#include <iomanip>
#include <iostream>
#include <string>
#include <vector>

#include "../../include/vsearch.hpp"
#include "cli_ranks.hpp"

// takes "--metric ip|l2" out of argv like --gpus; -1 when the flag is not given
static int take_metric_flag(int& argc, char** argv) {
    for (int i = 1; i < argc; ++i)
        if (std::string(argv[i]) == "--metric" && i + 1 < argc) {
            const std::string v = argv[i + 1];
            if (v != "ip" && v != "l2") throw std::runtime_error("--metric must be ip or l2");
            for (int j = i; j + 2 < argc; ++j) argv[j] = argv[j + 2];
            argc -= 2;
            return v == "ip" ? VS_METRIC_IP : VS_METRIC_L2;
        }
    return -1;
}

int main(int argc, char* argv[]) {
    vsearch::RankSet ranks;
    int METRIC = -1;
    try {
        METRIC = take_metric_flag(argc, argv);
        const int gpus = vsearch::take_gpus_flag(argc, argv);
        if (METRIC >= 0 && gpus > 1) throw std::runtime_error("--metric is not available together with --gpus N > 1 (the sharded calls are squared L2)");
        ranks = vsearch::fork_ranks(gpus);  // before anything touches HIP
    } catch (const std::exception& e) {
        std::cerr << "FATAL ERROR: " << e.what() << std::endl;
        return 1;
    }
    if (argc < 6) {
        if (ranks.rank == 0)
            std::cerr << "Usage: " << argv[0]
                      << " <index_dir> <queries.fvecs> <results_dir> <backend.so> <top_k> [nprobe] [groundtruth.ivecs] [batch] [--gpus N] [--metric ip|l2]"
                      << std::endl;
        return vsearch::join_ranks(ranks, 1);
    }
    const std::string index_dir = argv[1], query_file = argv[2], results_dir = argv[3], backend_path = argv[4];
    int TOP_K = 0, NPROBE = 16, BATCH_SIZE = 1;  // main_ivf.cpp:76, :78
    const std::string gt_file = (argc > 7) ? argv[7] : "";
    if (!vsearch::arg_int(argv[5], TOP_K) || (argc > 6 && !vsearch::arg_int(argv[6], NPROBE)) || (argc > 8 && !vsearch::arg_int(argv[8], BATCH_SIZE))) {
        if (ranks.rank == 0) std::cerr << "FATAL ERROR: <top_k>, [nprobe] and [batch] must be integers" << std::endl;
        return vsearch::join_ranks(ranks, 1);
    }
    int status = 0;
    try {
        vsearch::connect_ranks(ranks);
        mkdir(results_dir.c_str(), 0755);
        const std::string results_txt = results_dir + "/results.txt", metrics_txt = results_dir + "/metrics.txt";
        std::cout << "Loading queries..." << std::endl;
        std::vector<float> queries;
        int nq = 0, query_dim = 0;
        if (!vsearch::read_fvecs(query_file, queries, nq, query_dim)) throw std::runtime_error(vs_last_error());
        std::cout << "Loaded " << nq << " queries." << std::endl;
        std::vector<std::vector<int>> ground_truth;
        int gt_k = 0;
        if (!gt_file.empty()) {
            vsearch::load_ivecs(gt_file, ground_truth, gt_k);
            std::cout << "Loaded " << ground_truth.size() << " ground truth entries." << std::endl;
        }
        std::cout << "Loading IVF index..." << std::endl;
        vsearch::IVFIndex ivf(index_dir, backend_path, ranks.rank, ranks.rank, ranks.world);
        if (query_dim != static_cast<int>(ivf.getDim()))
            throw std::runtime_error("Query dim (" + std::to_string(query_dim) + ") != index dim (" +
                                     std::to_string(ivf.getDim()) + ")");
        ivf.setBatchSize(std::min(std::max(BATCH_SIZE, 1), 32));
        std::ofstream results_file(ranks.rank == 0 ? results_txt : std::string("/dev/null"));
        if (!results_file) throw std::runtime_error("Cannot open output file: " + results_txt);

        double total_centroid_ms = 0, total_gather_ms = 0, total_fine_ms = 0, total_search_ms = 0, total_recall = 0;
        size_t total_candidates = 0;
        std::vector<double> latencies;
        const size_t num_queries = (size_t)nq;
        {   // one untimed call first (the reference has none): the first launch of every kernel loads its code -- 17 ms
            // against the 3 ms all 10 000 SIFT queries take afterwards.  Results are discarded.
            const size_t wn = std::min<size_t>(num_queries, (size_t)std::min(std::max(BATCH_SIZE, 1), 32) * 32);
            std::vector<float> wq(queries.begin(), queries.begin() + (long)(wn * query_dim));
            std::vector<std::vector<int>> wi;
            std::vector<std::vector<float>> ws;
            vsearch::IVFIndex::SearchTiming wt;
            if (wn > 0) {
                if (ranks.world > 1) ivf.searchBatchSharded(ranks.comm, wq, (int)wn, TOP_K, NPROBE, wi, ws, wt);
                else if (METRIC >= 0) ivf.searchBatchMetric(wq, (int)wn, TOP_K, NPROBE, METRIC, wi, ws, wt);
                else ivf.searchBatchTopk(wq, (int)wn, TOP_K, NPROBE, wi, ws, wt);
            }
        }
        auto total_start = std::chrono::high_resolution_clock::now();
        // The reference calls searchBatch once per model batch (main_ivf.cpp:150-189).  Here up to 128 batches go down in
        // one call (the index still processes them BATCH_SIZE queries at a time: every kernel is launched once per group of
        // 32 batches, the groups of a call run on two streams, and a call is two uploads and two downloads; sharded: one
        // group = one all-gather per call); a query's latency entry is its batch's share of the call.
        const size_t per_call = (size_t)std::min(std::max(BATCH_SIZE, 1), 32) * (ranks.world > 1 ? 32 : 128);
        for (size_t i = 0; i < num_queries; i += per_call) {
            const size_t cur = std::min(per_call, num_queries - i);
            std::vector<float> batch(queries.begin() + (long)(i * query_dim), queries.begin() + (long)((i + cur) * query_dim));
            std::vector<std::vector<int>> bi;
            std::vector<std::vector<float>> bs;
            vsearch::IVFIndex::SearchTiming timing;
            auto b0 = std::chrono::high_resolution_clock::now();
            if (ranks.world > 1) total_candidates += ivf.searchBatchSharded(ranks.comm, batch, (int)cur, TOP_K, NPROBE, bi, bs, timing);
            else if (METRIC >= 0) total_candidates += ivf.searchBatchMetric(batch, (int)cur, TOP_K, NPROBE, METRIC, bi, bs, timing);
            else total_candidates += ivf.searchBatchTopk(batch, (int)cur, TOP_K, NPROBE, bi, bs, timing);  // (k up to 128 at every dimension)
            auto b1 = std::chrono::high_resolution_clock::now();
            const double call_ms = std::chrono::duration<double, std::milli>(b1 - b0).count();
            const size_t n_b = (cur + (size_t)std::max(BATCH_SIZE, 1) - 1) / (size_t)std::max(BATCH_SIZE, 1);
            const double batch_ms = call_ms / (double)n_b;
            total_centroid_ms += timing.centroid_search_ms;
            total_gather_ms += timing.gather_ms;
            total_fine_ms += timing.fine_search_ms;
            total_search_ms += call_ms;
            for (size_t j = 0; j < cur; ++j) {
                latencies.push_back(batch_ms);
                if (!ground_truth.empty() && (i + j) < ground_truth.size())
                    total_recall += vsearch::compute_recall(bi[j], ground_truth[i + j], TOP_K);
                results_file << "Query " << (i + j) << ":";
                for (size_t t = 0; t < bi[j].size(); ++t)
                    results_file << " (" << bi[j][t] << ", " << std::fixed << std::setprecision(4) << bs[j][t] << ")";
                results_file << "\n";
            }
        }
        auto total_end = std::chrono::high_resolution_clock::now();
        const std::chrono::duration<double> total_time = total_end - total_start;
        results_file.close();

        const double avg_latency = total_search_ms / num_queries;
        const double avg_candidates = static_cast<double>(total_candidates) / num_queries;
        const double avg_recall = ground_truth.empty() ? 0.0 : total_recall / num_queries;
        const double throughput = num_queries / total_time.count();
        std::sort(latencies.begin(), latencies.end());
        const double p50 = latencies[latencies.size() / 2];
        const double p95 = latencies[static_cast<size_t>(latencies.size() * 0.95)];
        const double p99 = latencies[static_cast<size_t>(latencies.size() * 0.99)];
        const double speedup_candidates = ivf.getNumVectors() / avg_candidates;

        std::ofstream m(ranks.rank == 0 ? metrics_txt : std::string("/dev/null"));
        if (!m) throw std::runtime_error("Cannot open metrics file: " + metrics_txt);
        m << std::fixed << std::setprecision(6);
        m << "=== IVF Search Performance Metrics ===\n\n";
        m << "(one untimed warm-up call before the timed loop)\n";
        m << "Index Configuration:\n  Total vectors: " << ivf.getNumVectors() << "\n  Number of clusters: " << ivf.getNumClusters()
          << "\n  Dimension: " << ivf.getDim() << "\n  nprobe: " << NPROBE << "\n  top_k: " << TOP_K
          << "\n  batch_size: " << BATCH_SIZE << "\n\n";
        m << "Query Statistics:\n  Number of queries: " << num_queries << "\n  Avg candidates searched: " << avg_candidates
          << "\n  Candidate reduction: " << speedup_candidates << "x\n\n";
        if (!ground_truth.empty()) m << "Accuracy:\n  Recall@" << TOP_K << ": " << (avg_recall * 100.0) << "%\n\n";
        m << "Latency:\n  Avg per query (amortized): " << avg_latency << " ms\n  Avg centroid search (GPU): "
          << (total_centroid_ms / num_queries) << " ms\n  Avg gather: " << (total_gather_ms / num_queries)
          << " ms\n  Avg fine search (GPU): " << (total_fine_ms / num_queries) << " ms\n  Batch P50: " << p50
          << " ms\n  Batch P95: " << p95 << " ms\n  Batch P99: " << p99 << " ms\n\n";
        m << "Throughput:\n  Total time: " << total_time.count() << " s\n  QPS: " << throughput << "\n\n";
        const double cf = 2.0 * ivf.getDim() * ivf.getNumClusters(), ff = 2.0 * ivf.getDim() * avg_candidates;
        m << "Compute:\n  FLOPs per query (centroid): " << std::scientific << cf << "\n  FLOPs per query (fine): " << ff
          << "\n  FLOPs per query (total): " << (cf + ff) << "\n  Avg GFLOPS: " << std::fixed
          << ((cf + ff) / 1e9) / (avg_latency / 1000.0) << "\n  Total GFLOPS: " << (cf + ff) * num_queries / (total_time.count() * 1e9)
          << "\n\n";
        // main_ivf.cpp:266-271: share of the end-to-end time per stage (device time of the stage's launches, from HIP events)
        const double total_ms = total_time.count() * 1000.0;
        m << "Time Breakdown:\n  Centroid search (GPU): " << (total_centroid_ms / total_ms * 100.0) << "%\n  Gather candidates: "
          << (total_gather_ms / total_ms * 100.0) << "%\n  Fine search (GPU): " << (total_fine_ms / total_ms * 100.0) << "%\n";
        m.close();

        std::cout << "\n=== IVF Search Complete ===" << std::endl;
        std::cout << "Throughput: " << throughput << " QPS" << std::endl;
        std::cout << "Avg latency: " << avg_latency << " ms" << std::endl;
        std::cout << "Avg candidates: " << avg_candidates << " (" << speedup_candidates << "x reduction)" << std::endl;
        if (!ground_truth.empty()) std::cout << "Recall@" << TOP_K << ": " << (avg_recall * 100.0) << "%" << std::endl;
        std::cout << "\nResults saved to: " << results_txt << std::endl;
        std::cout << "Metrics saved to: " << metrics_txt << std::endl;
    } catch (const std::exception& e) {
        std::cerr << "FATAL ERROR: " << e.what() << std::endl;  // main_ivf.cpp:287-290
        status = 1;
    }
    return vsearch::join_ranks(ranks, status);
}
