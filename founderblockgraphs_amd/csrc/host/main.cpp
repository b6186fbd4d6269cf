// main.cpp -- founderblockgraph host program on top of libfbg_hip.so.
//
// Mirrors main() of the reference (founderblockgraph.cpp:3298-3521): same flag checks, messages
// and exit codes, same output file.  The three calls into the hot path -- load_cst (3378),
// segment_elastic_minmaxlength (3393) and segment (3437) -- are replaced by calls through the
// C ABI of include/fbg_hip.h; nothing in this program computes a segmentation on the CPU.
// Differences that are not part of the output contract are listed in INTEGRATION.md
// (no <input>.plain / .cst side files, stderr wording of the index-size line).
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <set>
#include <string>
#include <unordered_map>
#include <vector>
#include "../../../include/fbg_hip.h"
#include "fasta.hpp"
#include "options.hpp"
#include "xgfa.hpp"

namespace {

int engine_failure(fbg_ctx *ctx, const char *what, int rc)
{
    std::cerr << "ERROR: " << what << " failed (code " << rc << "): " << fbg_last_error(ctx) << std::endl;
    return EXIT_FAILURE;
}

void write_empty_graphviz(const std::string &path)
{
    // output_graphviz (fbg.cpp:3043-3092) receives empty node/edge vectors in elastic mode
    std::ofstream os(path);
    os << "digraph founder_block_graph {\n" << "rankdir=\"LR\"\n" << "}\n";
}

// The repair loop (fbg.cpp:3471-3497) for inputs fbg_segmentation_repair declines: labels are cut out of the MSA and
// numbered here as output_efg does (per block a map label -> id by first row, a set of edges), the check itself is
// fbg_pindex_build + fbg_pindex_validate, once per round.
int repair_on_host(fbg_ctx *ctx, const Msa &msa, std::vector<uint64_t> &boundaries, const std::string &ignore_chars,
                   uint64_t &rounds, std::vector<uint64_t> &removed)
{
    rounds = 0;
    removed.assign(boundaries.size(), 0);
    for (;;) {
        const uint64_t nb = boundaries.size();
        std::string labels;
        std::vector<uint64_t> label_off{0}, edge_off{0}, edge_dst;
        std::vector<uint32_t> node_block;
        std::vector<std::set<uint64_t>> out;                  // distinct out-neighbours per node
        std::vector<int64_t> prev(msa.m, -1), cur(msa.m, -1);
        for (uint64_t j = 0; j < nb; j++) {
            const uint64_t x0 = j ? boundaries[j - 1] + 1 : 0, x1 = std::min(boundaries[j] + 1, msa.n);
            std::unordered_map<std::string, uint64_t> ids;
            for (uint64_t i = 0; i < msa.m; i++) {
                std::string lab;
                for (uint64_t x = x0; x < x1; x++)
                    if (msa.cells[i * msa.n + x] != '-') lab.push_back((char)msa.cells[i * msa.n + x]);
                cur[i] = -1;
                if (lab.empty()) continue;                    // a row of gaps has no node in this block
                auto it = ids.find(lab);
                if (it == ids.end()) {
                    it = ids.emplace(lab, node_block.size()).first;
                    labels += lab;
                    label_off.push_back(labels.size());
                    node_block.push_back((uint32_t)j);
                    out.emplace_back();
                }
                cur[i] = (int64_t)it->second;
                if (j && prev[i] >= 0) out[(size_t)prev[i]].insert(it->second);
            }
            std::swap(prev, cur);
        }
        const uint64_t n_nodes = node_block.size();
        for (uint64_t u = 0; u < n_nodes; u++) {
            edge_dst.insert(edge_dst.end(), out[u].begin(), out[u].end());
            edge_off.push_back(edge_dst.size());
        }
        edge_dst.push_back(0);
        labels.push_back('\0');
        fbg_pindex *ix = nullptr;
        int rc = fbg_pindex_build(ctx, reinterpret_cast<const uint8_t *>(labels.data()), label_off.data(), n_nodes, edge_off.data(),
                                  edge_dst.data(), &ix);
        if (rc != FBG_OK) return rc;
        std::vector<uint8_t> status(n_nodes + 1);
        rc = fbg_pindex_validate(ix, node_block.data(), reinterpret_cast<const uint8_t *>(ignore_chars.data()), ignore_chars.size(),
                                 status.data(), nullptr, nullptr, nullptr, nullptr);
        fbg_pindex_destroy(ix);
        if (rc != FBG_OK) return rc;
        std::vector<bool> cut(nb, false);
        for (uint64_t u = 0; u < n_nodes; u++)
            if (status[u] == FBG_NODE_INVALID && node_block[u] > 0) cut[node_block[u] - 1] = true;
        const uint64_t flagged = (uint64_t)std::count(cut.begin(), cut.end(), true);
        if (!flagged) return FBG_OK;
        removed[rounds++] = flagged;
        std::vector<uint64_t> kept;
        for (uint64_t k = 0; k < nb; k++)
            if (!cut[k]) kept.push_back(boundaries[k]);
        boundaries.swap(kept);
    }
}

} // namespace

int main(int argc, char **argv)
{
    Options opt;
    if (parse_options(argc, argv, opt) != 0) return EXIT_FAILURE;
    std::ios_base::sync_with_stdio(false);

    if (opt.gap_limit < 0) { std::cerr << "Gap limit needs to be non-negative.\n"; return EXIT_FAILURE; }   // 3309-3313
    if (!opt.elastic && opt.output_paths) {                                                                  // 3319-3323
        std::cerr << "Output of original sequences as paths without option --elastic is not implemented!\n";
        return EXIT_FAILURE;
    }
    if ((!opt.elastic && opt.gfa) || (opt.elastic && !opt.gfa)) {                                            // 3325-3329
        std::cerr << "--elastic and --gfa options are currently only supported when both are used!\n";
        return EXIT_FAILURE;
    }
    if (opt.heuristic_subset < -1 || opt.heuristic_subset == 0) {                                            // 3331-3334
        std::cerr << "wrong value for --heuristic-subset!\n";
        return EXIT_FAILURE;
    }
    const bool heuristic = opt.heuristic_subset != -1;
    if (heuristic && !(opt.elastic && opt.gfa)) {
        // the reference goes on to segment() with an MSA it never read (fbg.cpp:3347-3366, 3437): undefined
        std::cerr << "--heuristic-subset needs --elastic and --gfa: the row-chunk mode is defined for the elastic xGFA output only.\n";
        return EXIT_FAILURE;
    }

    const auto start = std::chrono::high_resolution_clock::now();
    // FBG_TIMING=1: where the wall time goes, on stderr (not part of the reference's output)
    const bool timing = std::getenv("FBG_TIMING") != nullptr;
    auto last = start;
    auto lap = [&](const char *what) {
        if (!timing) return;
        const auto now = std::chrono::high_resolution_clock::now();
        std::cerr << "[timing] " << what << ": " << std::chrono::duration<double>(now - last).count() << " s\n";
        last = now;
    };

    Msa msa;
    const bool have_input = heuristic ? read_msa_strict(opt.input, opt.output_paths, msa)                     // 3363
                                      : read_msa(opt.input, opt.gap_limit, opt.elastic, opt.output_paths, msa);
    if (!have_input || msa.m == 0 || msa.n == 0) {
        std::cerr << "Unable to read sequences from the input\n.";                                          // 3353
        return EXIT_FAILURE;
    }
    std::cerr << "Input MSA[1.." << msa.m << ",1.." << msa.n << "]" << std::endl;                            // 3357
    lap("read FASTA");

    if (opt.elastic && opt.threads != -1 && opt.threads <= 0) {                                              // 3396-3399
        std::cerr << "Invalid number of threads." << std::endl;
        return EXIT_FAILURE;
    }

    if (opt.threads > 0) set_host_threads((unsigned)opt.threads);

    // Which GPUs: FBG_DEVICES="0,1,2,3" names them (an id may repeat: several contexts on one device); otherwise one
    // GPU for texts it indexes in one piece, and for longer ones every visible GPU -- at most --threads of them, the
    // reference's own knob for how wide the scan fans out (fbg.cpp:3392-3399).  The group runs the index and the scan
    // (partitioned over the devices, or in column ranges like compute_f_range); the sweep runs on its first member.
    std::vector<int> devices;
    int ndev = 1;
    if (const char *spec = std::getenv("FBG_DEVICES")) {
        for (const char *p = spec; *p;) {
            char *end = nullptr;
            const long d = std::strtol(p, &end, 10);
            if (end == p) break;
            devices.push_back((int)d);
            p = *end == ',' ? end + 1 : end;
        }
        ndev = (int)devices.size();
    } else if ((double)msa.m * (double)(msa.n + 1) >= 1073741824.0) {
        ndev = opt.threads > 0 ? (int)std::min<long>(opt.threads, 64) : 0;       // 0: all visible devices
    }
    fbg_group *grp = nullptr;
    int rc = fbg_group_create(ndev, devices.empty() ? nullptr : devices.data(), &grp);
    if (rc != FBG_OK) {
        std::cerr << "ERROR: cannot open the GPU engine: " << fbg_group_last_error(nullptr) << std::endl;
        return EXIT_FAILURE;
    }
    fbg_ctx *ctx = fbg_group_member(grp, 0);
    struct GroupGuard { fbg_group *g; ~GroupGuard() { if (g) fbg_group_destroy(g); } } guard{grp};
    auto close_engine = [&]() { fbg_group_destroy(grp); guard.g = nullptr; };
    auto group_failure = [&](const char *what, int code) {
        std::cerr << "ERROR: " << what << " failed (code " << code << "): " << fbg_group_last_error(grp) << std::endl;
        return EXIT_FAILURE;
    };

    lap("open the GPU engine");
    std::vector<uint64_t> boundaries;
    const uint8_t *ignore = reinterpret_cast<const uint8_t *>(opt.ignore_chars.data());
    if (heuristic) {
        // fbg.cpp:3400-3433: f of every chunk of ROWNUM consecutive rows, max-merged (1681); the sweep on the merged f.
        // Chunks are small: they run on member 0.  --threads only spreads the reference's chunks over workers; the
        // merge is a max, so the result does not depend on it.
        std::vector<uint64_t> f(msa.n, 0);                                                                   // 3388
        const uint64_t R = (uint64_t)opt.heuristic_subset;
        for (uint64_t r0 = 0; r0 < msa.m; r0 += R) {
            const uint64_t rows = std::min<uint64_t>(R, msa.m - r0);
            std::cerr << "Reading MSA[" << r0 << ".." << r0 + R - 1 << "]..." << std::endl;                  // 271
            rc = fbg_elastic_f(ctx, msa.cells.data() + r0 * msa.n, rows, msa.n, ignore, opt.ignore_chars.size(),
                               opt.disable_elastic_tricks ? 1 : 0, f.data());
            std::cerr << "MSA index construction complete, index requires "
                      << (double)fbg_device_bytes(ctx) / (1024.0 * 1024.0) << " MiB." << std::endl;          // 3410
            if (rc == FBG_ERR_NO_SEGMENTATION) { std::cerr << "No valid segmentation found!\n"; close_engine(); std::exit(1); }
            if (rc != FBG_OK) return engine_failure(ctx, "fbg_elastic_f", rc);
        }
        std::cerr << "Computing optimal segmentation..." << std::flush;                                     // 1958
        boundaries.resize(msa.n + 1);
        uint64_t count = 0;
        std::vector<uint64_t> mml(msa.n + 1);
        rc = fbg_minmax_dp(ctx, f.data(), msa.n, boundaries.data(), &count, mml.data(), nullptr);
        if (rc != FBG_OK) return engine_failure(ctx, "fbg_minmax_dp", rc);
        boundaries.resize(count);
        std::cerr << "done (optimal segment length = " << mml[msa.n] << ")." << std::endl;                   // 2023
        lap("chunked scan and sweep");
        // fbg.cpp:3467-3498: the graph of this segmentation is in general not semi-repeat-free; repair it
        rc = fbg_msa_load_host(ctx, msa.cells.data(), msa.m, msa.n);
        if (rc != FBG_OK) return engine_failure(ctx, "fbg_msa_load_host", rc);
        uint64_t nb = boundaries.size(), rounds = 0;
        std::vector<uint64_t> removed(nb);
        rc = fbg_segmentation_repair(ctx, boundaries.data(), &nb, ignore, opt.ignore_chars.size(), &rounds, removed.data(), nullptr);
        if (rc == FBG_ERR_HASH_COLLISION || rc == FBG_ERR_TOO_LARGE) {
            // block grouping declined (a hash collision, more rows than it takes): labels cut and numbered here
            rc = repair_on_host(ctx, msa, boundaries, opt.ignore_chars, rounds, removed);
            if (rc != FBG_OK) return engine_failure(ctx, "the repair of the segmentation", rc);
        } else {
            if (rc != FBG_OK) return engine_failure(ctx, "fbg_segmentation_repair", rc);
            boundaries.resize(nb);
        }
        for (uint64_t r = 0; r < rounds; r++) std::cerr << "There are " << removed[r] << " blocks to remove" << std::endl;   // 3476-3480
        std::cerr << "There are 0 blocks to remove" << std::endl;
        std::cerr << "Graph fixed in " << rounds << "iterations\xe2\x80\xa6\n";                             // 3498
    } else if (opt.elastic) {
        std::vector<uint64_t> f(msa.n, 0);                                                                   // 3388
        rc = fbg_group_elastic_f(grp, msa.cells.data(), msa.m, msa.n,
                                 reinterpret_cast<const uint8_t *>(opt.ignore_chars.data()), opt.ignore_chars.size(),
                                 opt.disable_elastic_tricks ? 1 : 0, f.data());
        std::cerr << "MSA index construction complete, index requires "
                  << (double)fbg_device_bytes(ctx) / (1024.0 * 1024.0) << " MiB." << std::endl;              // 3380
        if (rc == FBG_ERR_NO_SEGMENTATION) { std::cerr << "No valid segmentation found!\n"; close_engine(); std::exit(1); }
        if (rc != FBG_OK) return group_failure("fbg_group_elastic_f", rc);
        std::cerr << "Computing optimal segmentation..." << std::flush;                                     // 1958
        boundaries.resize(msa.n + 1);
        uint64_t count = 0;
        std::vector<uint64_t> mml(msa.n + 1);
        rc = fbg_minmax_dp(ctx, f.data(), msa.n, boundaries.data(), &count, mml.data(), nullptr);
        if (rc != FBG_OK) return engine_failure(ctx, "fbg_minmax_dp", rc);
        boundaries.resize(count);
        std::cerr << "done (optimal segment length = " << mml[msa.n] << ")." << std::endl;                   // 2023
    } else if (opt.gap_limit == 1) {
        std::vector<uint64_t> v(msa.n), s(msa.n), prev(msa.n);
        rc = fbg_group_repeatfree_v(grp, msa.cells.data(), msa.m, msa.n, v.data());
        if (rc != FBG_OK) return group_failure("fbg_group_repeatfree_v", rc);
        std::cerr << "MSA index construction complete, index requires "
                  << (double)fbg_device_bytes(ctx) / (1024.0 * 1024.0) << " MiB." << std::endl;
        boundaries.resize(msa.n);
        uint64_t count = 0;
        rc = fbg_repeatfree_dp(ctx, v.data(), msa.n, s.data(), prev.data(), boundaries.data(), &count);
        if (rc != FBG_OK && rc != FBG_ERR_NO_SEGMENTATION) {
            return engine_failure(ctx, "fbg_repeatfree_dp", rc);
        }
        std::cerr << "Optimal score: " << s[msa.n - 1] << std::endl;                                        // 646
        if (rc == FBG_ERR_NO_SEGMENTATION) {                                                                 // 648-652
            std::cerr << "No proper segmentation exists.\n";
            return EXIT_FAILURE;
        }
        boundaries.resize(count);
        std::cerr << "Number of segments: " << boundaries.size() << std::endl;                               // 664
        const GraphStats st = segment_stats(msa, boundaries);
        std::cerr << "#nodes=" << st.nodes << std::endl;                                                     // 694-728
        std::cerr << "total length of node labels=" << st.total_label_length << std::endl;
        std::cerr << "#founders=" << st.founders << std::endl;
        std::cerr << "#edges=" << st.edges << std::endl;
    } else {
        // segment2elasticValid (fbg.cpp:738-935): rows may hold gaps (runs shorter than the limit survived read_msa)
        std::vector<uint64_t> v(msa.n), s(msa.n), prev(msa.n);
        rc = fbg_group_gapped_v(grp, msa.cells.data(), msa.m, msa.n, v.data());
        if (rc != FBG_OK) return group_failure("fbg_group_gapped_v", rc);
        std::cerr << "MSA index construction complete, index requires "
                  << (double)fbg_device_bytes(ctx) / (1024.0 * 1024.0) << " MiB." << std::endl;
        boundaries.resize(msa.n);
        uint64_t count = 0;
        rc = fbg_gapped_dp(ctx, v.data(), msa.n, s.data(), prev.data(), boundaries.data(), &count);
        if (rc != FBG_OK && rc != FBG_ERR_NO_SEGMENTATION) {
            return engine_failure(ctx, "fbg_gapped_dp", rc);
        }
        std::cerr << "Optimal score: " << s[msa.n - 1] << std::endl;                                        // 848
        if (rc == FBG_ERR_NO_SEGMENTATION) {                                                                 // 850-854
            std::cerr << "No valid segmentation found!\n";
            return EXIT_FAILURE;
        }
        boundaries.resize(count);
        std::cerr << "Number of segments: " << boundaries.size() << std::endl;                               // 866
        const GraphStats st = segment_stats(msa, boundaries);
        std::cerr << "#nodes=" << st.nodes << std::endl;                                                     // 896-929
        std::cerr << "total length of node labels=" << st.total_label_length << std::endl;
        std::cerr << "#founders=" << st.founders << std::endl;
        std::cerr << "#edges=" << st.edges << std::endl;
    }
    lap("segmentation (copy in, index, scan, sweep)");
    // nodes and edges of the graph come from the engine too (fbg_block_graph); ask before it goes away
    BlockGraph graph;
    bool have_graph = false;
    if (opt.elastic) {
        const uint64_t cells = msa.m * boundaries.size();
        graph.node_of.resize(cells); graph.rep_row.resize(cells); graph.edges.resize(cells);
        graph.first_node.resize(boundaries.size() + 1); graph.edge_count.resize(boundaries.size());
        rc = fbg_block_graph(ctx, boundaries.data(), boundaries.size(), graph.node_of.data(), graph.first_node.data(),
                             graph.rep_row.data(), graph.edge_count.data(), graph.edges.data());
        have_graph = rc == FBG_OK;          // otherwise (a hash collision, an input beyond its limits): hash on the host
    }
    lap("graph nodes and edges");
    close_engine();

    if (!opt.elastic) {
        // The reference goes on to make_efg() with an EMPTY block_indices vector (fbg.cpp:3385,3449) and reads
        // boundaries[0] of it (fbg.cpp:1012-1017): undefined behaviour, so there is no defined .index output
        // to reproduce at this commit.  The segmentation and statistics above are the observable result.
        std::cerr << "Writing the index to disk\xe2\x80\xa6\n";                                              // 3448
        std::cerr << "The founder block index (.index) writer is not provided by this build; "
                     "the reference's own output on this path is undefined (fbg.cpp:3449, 1012-1017).\n";
        return EXIT_FAILURE;
    }

    std::cerr << "Writing the xGFA to disk\xe2\x80\xa6\n";                                                   // 3502
    std::string error;
    const bool written = have_graph ? write_xgfa_graph(msa, boundaries, graph, opt.output_paths, opt.output, error)
                                    : write_xgfa(msa, boundaries, opt.output_paths, opt.output, error);
    if (!written) {
        // the reference lets std::ios_base::failure escape (fbg.cpp:1197) or trips an assert: it aborts
        std::cerr << "ERROR: " << error << std::endl;
        std::abort();
    }

    lap("write xGFA");
    const auto end = std::chrono::high_resolution_clock::now();
    const auto seconds = std::chrono::duration_cast<std::chrono::seconds>(end - start).count();
    if (opt.graphviz_output_given) {                                                                         // 3511-3515
        std::cerr << "Writing the Graphviz file\xe2\x80\xa6\n";
        write_empty_graphviz(opt.graphviz_output);
    }
    std::cerr << "Time taken: " << seconds << " seconds" << std::endl;                                      // 3517-3518
    return EXIT_SUCCESS;
}
