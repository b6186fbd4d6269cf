// xgfa_read.hpp -- the graph of an xGFA (or GFA) file for the pattern index: S and L lines, nothing else.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

struct XgfaGraph {
    std::string labels;                 // all labels, node after node
    std::vector<uint64_t> label_off;    // [nodes + 1]
    std::vector<uint64_t> edge_off;     // [nodes + 1] CSR by source
    std::vector<uint64_t> edge_dst;     // node indices
};

// Nodes are the S lines in ascending id order (0- or 1-based alike; ids need not be contiguous), empty labels
// included; L lines become edges between them.  Returns false with a message on an unreadable file, a malformed
// line, a repeated S id or an L line naming an unknown node.
bool read_xgfa_graph(const std::string &path, XgfaGraph &g, std::string &error);
