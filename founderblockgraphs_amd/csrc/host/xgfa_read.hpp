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
    std::vector<uint64_t> ids;          // [nodes] the S id of every node
    // the B line (block sizes over the nodes in ascending S id, xGFAspec.md), recorded but not checked here
    bool has_blocks = false;            // a B line was seen
    std::string blocks_error;           // non-empty: the B line is malformed or repeated
    std::vector<uint64_t> block_sizes;
};

// Nodes are the S lines in ascending id order (0- or 1-based alike; ids need not be contiguous), empty labels
// included; L lines become edges between them.  Returns false with a message on an unreadable file, a malformed
// line, a repeated S id or an L line naming an unknown node.  A B line never makes the read fail: what is wrong with
// it goes to blocks_error, for the callers that need blocks (block_of).
bool read_xgfa_graph(const std::string &path, XgfaGraph &g, std::string &error);

// node_block[nodes] (blocks from 0) from the B line; false with a message when the B line is missing, malformed,
// repeated, or its sizes do not sum to the node count.
bool block_of(const XgfaGraph &g, std::vector<uint32_t> &node_block, std::string &error);
