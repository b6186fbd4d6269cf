// validate_main.cpp -- fbg_validate: the semi-repeat-free check of a founder graph through the pattern index of
// libfbg_hip.so (include/fbg_hip.h, fbg_pindex_validate):
//
//   fbg_validate --graph=efg.xgfa [--ignore-chars=STRING]
//
// Blocks come from the graph's B line (block sizes over the nodes in ascending S id, xGFAspec.md).  stdout: one line
// per INVALID node in S id order,
//   invalid <id> <block> <witness id> <witness offset> <witness block>
// (tab-separated; ids are the file's S ids, blocks count from 1), then
//   nodes <n> valid <a> invalid <b> source_sink <c> ignored <d> empty <e>
// Exit status: 0 when no node is INVALID, 1 when some node is, 2 on a usage error, an unreadable file, a missing or
// inconsistent B line (all found before a GPU context is created) or a library error.  stderr carries the messages.
#include <cstdio>
#include <iostream>
#include <string>
#include <vector>
#include "../../../include/fbg_hip.h"
#include "xgfa_read.hpp"

static int usage(const char *msg)
{
    std::cerr << "fbg_validate: " << msg << "\n"
              << "usage: fbg_validate --graph=efg.xgfa [--ignore-chars=STRING]\n";
    return 2;
}

int main(int argc, char **argv)
{
    std::string graph, ignore;
    bool have_graph = false, have_ignore = false;
    for (int i = 1; i < argc; i++) {
        const std::string a = argv[i];
        auto value = [&](const char *name, std::string &out, bool &have) {
            const std::string pre = std::string(name) + "=";
            if (a.compare(0, pre.size(), pre) == 0) { out = a.substr(pre.size()); have = true; return true; }
            if (a == name && i + 1 < argc) { out = argv[++i]; have = true; return true; }
            return false;
        };
        if (value("--graph", graph, have_graph) || value("--ignore-chars", ignore, have_ignore)) continue;
        if (a == "--help" || a == "-h") { usage("semi-repeat-free check of a founder graph"); return 0; }
        return usage(("unknown argument " + a).c_str());
    }
    if (!have_graph || graph.empty()) return usage("--graph is required");

    XgfaGraph g;
    std::string error;
    std::vector<uint32_t> block;
    if (!read_xgfa_graph(graph, g, error) || !block_of(g, block, error)) {
        std::cerr << "fbg_validate: " << error << "\n";
        return 2;
    }
    const uint64_t nodes = g.ids.size();

    fbg_ctx *ctx = nullptr;
    int rc = fbg_ctx_create(0, &ctx);
    if (rc != FBG_OK) { std::cerr << "fbg_validate: " << fbg_last_error(nullptr) << "\n"; return 2; }
    fbg_pindex *ix = nullptr;
    std::vector<uint8_t> status(nodes + 1);
    std::vector<uint64_t> wnode(nodes + 1), woff(nodes + 1);
    rc = fbg_pindex_build(ctx, (const uint8_t *)g.labels.data(), g.label_off.data(), nodes, g.edge_off.data(), g.edge_dst.data(), &ix);
    if (rc == FBG_OK)
        rc = fbg_pindex_validate(ix, block.data(), (const uint8_t *)ignore.data(), ignore.size(), status.data(), wnode.data(),
                                 woff.data(), nullptr, nullptr);
    if (rc != FBG_OK) {
        std::cerr << "fbg_validate: " << fbg_last_error(ctx) << "\n";
        fbg_pindex_destroy(ix);
        fbg_ctx_destroy(ctx);
        return 2;
    }
    fbg_pindex_destroy(ix);
    fbg_ctx_destroy(ctx);

    uint64_t count[5] = {0, 0, 0, 0, 0};
    std::string out;
    for (uint64_t u = 0; u < nodes; u++) {
        count[status[u] < 5 ? status[u] : 1]++;
        if (status[u] != FBG_NODE_INVALID) continue;
        const uint64_t w = wnode[u];
        out += "invalid\t" + std::to_string(g.ids[u]) + "\t" + std::to_string(block[u] + 1ull) + "\t" + std::to_string(g.ids[w]) +
               "\t" + std::to_string(woff[u]) + "\t" + std::to_string(block[w] + 1ull) + "\n";
    }
    out += "nodes\t" + std::to_string(nodes) + "\tvalid\t" + std::to_string(count[FBG_NODE_VALID]) + "\tinvalid\t" +
           std::to_string(count[FBG_NODE_INVALID]) + "\tsource_sink\t" + std::to_string(count[FBG_NODE_SKIP_SOURCE_SINK]) +
           "\tignored\t" + std::to_string(count[FBG_NODE_SKIP_IGNORED]) + "\tempty\t" + std::to_string(count[FBG_NODE_SKIP_EMPTY]) + "\n";
    std::fwrite(out.data(), 1, out.size(), stdout);
    std::fflush(stdout);
    return count[FBG_NODE_INVALID] ? 1 : 0;
}
