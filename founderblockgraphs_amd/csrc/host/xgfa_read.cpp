// xgfa_read.cpp -- S / L lines of an xGFA file into labels + CSR edges (xgfa_read.hpp).
#include "xgfa_read.hpp"
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <unordered_map>

namespace {

bool parse_id(const std::string &s, uint64_t &v)
{
    if (s.empty() || s.size() > 19) return false;
    v = 0;
    for (char c : s) {
        if (c < '0' || c > '9') return false;
        v = v * 10 + (uint64_t)(c - '0');
    }
    return true;
}

void split_tabs(const std::string &line, std::vector<std::string> &f)
{
    f.clear();
    size_t a = 0;
    while (true) {
        const size_t b = line.find('\t', a);
        f.push_back(line.substr(a, b == std::string::npos ? std::string::npos : b - a));
        if (b == std::string::npos) break;
        a = b + 1;
    }
}

} // namespace

bool read_xgfa_graph(const std::string &path, XgfaGraph &g, std::string &error)
{
    std::ifstream is(path, std::ios::binary);
    if (!is) { error = "cannot open " + path; return false; }
    g.has_blocks = false;
    g.blocks_error.clear();
    g.block_sizes.clear();
    struct Node { uint64_t id; std::string label; };
    std::vector<Node> nodes;
    std::vector<std::pair<uint64_t, uint64_t>> links;
    std::string line;
    std::vector<std::string> f;
    uint64_t lineno = 0;
    while (std::getline(is, line)) {
        lineno++;
        if (!line.empty() && line.back() == '\r') line.pop_back();
        if (line.empty() || (line[0] != 'S' && line[0] != 'L' && line[0] != 'B') || (line.size() > 1 && line[1] != '\t')) continue;
        split_tabs(line, f);
        uint64_t a = 0, b = 0;
        if (line[0] == 'B') {
            if (g.has_blocks && g.blocks_error.empty()) g.blocks_error = path + ":" + std::to_string(lineno) + ": a second B line";
            g.has_blocks = true;
            g.block_sizes.clear();
            for (size_t k = 1; k < f.size(); k++) {
                if (k + 1 == f.size() && f[k].empty()) break;         // a trailing tab
                if (!parse_id(f[k], a)) {
                    if (g.blocks_error.empty()) g.blocks_error = path + ":" + std::to_string(lineno) + ": malformed B line";
                    break;
                }
                g.block_sizes.push_back(a);
            }
        } else if (line[0] == 'S') {
            if (f.size() < 2 || !parse_id(f[1], a)) { error = path + ":" + std::to_string(lineno) + ": malformed S line"; return false; }
            nodes.push_back({a, f.size() > 2 ? f[2] : std::string()});
        } else {
            if (f.size() < 4 || !parse_id(f[1], a) || !parse_id(f[3], b)) {
                error = path + ":" + std::to_string(lineno) + ": malformed L line";
                return false;
            }
            links.emplace_back(a, b);
        }
    }
    if (is.bad()) { error = "cannot read " + path; return false; }
    std::stable_sort(nodes.begin(), nodes.end(), [](const Node &x, const Node &y) { return x.id < y.id; });
    std::unordered_map<uint64_t, uint64_t> where;
    where.reserve(nodes.size() * 2);
    g.labels.clear();
    g.label_off.assign(1, 0);
    g.ids.clear();
    for (uint64_t i = 0; i < nodes.size(); i++) {
        if (!where.emplace(nodes[i].id, i).second) { error = path + ": node " + std::to_string(nodes[i].id) + " appears twice"; return false; }
        g.ids.push_back(nodes[i].id);
        g.labels += nodes[i].label;
        g.label_off.push_back(g.labels.size());
    }
    g.edge_off.assign(nodes.size() + 1, 0);
    std::vector<std::pair<uint64_t, uint64_t>> e;
    e.reserve(links.size());
    for (const auto &l : links) {
        const auto u = where.find(l.first), v = where.find(l.second);
        if (u == where.end() || v == where.end()) {
            error = path + ": L line between " + std::to_string(l.first) + " and " + std::to_string(l.second) + " names an unknown node";
            return false;
        }
        e.emplace_back(u->second, v->second);
    }
    std::stable_sort(e.begin(), e.end(), [](const auto &x, const auto &y) { return x.first < y.first; });
    g.edge_dst.clear();
    for (const auto &p : e) { g.edge_off[p.first + 1]++; g.edge_dst.push_back(p.second); }
    for (uint64_t i = 0; i < nodes.size(); i++) g.edge_off[i + 1] += g.edge_off[i];
    return true;
}

bool block_of(const XgfaGraph &g, std::vector<uint32_t> &node_block, std::string &error)
{
    if (!g.has_blocks) { error = "the graph has no B line (block sizes)"; return false; }
    if (!g.blocks_error.empty()) { error = g.blocks_error; return false; }
    const uint64_t nodes = g.ids.size();
    uint64_t sum = 0;
    for (uint64_t s : g.block_sizes) {
        sum += s;
        if (sum > nodes) break;
    }
    if (sum != nodes || g.block_sizes.size() >= 0xffffffffull) {
        error = "the B line's block sizes do not sum to the " + std::to_string(nodes) + " nodes";
        return false;
    }
    node_block.clear();
    node_block.reserve(nodes);
    for (uint64_t b = 0; b < g.block_sizes.size(); b++) node_block.insert(node_block.end(), g.block_sizes[b], (uint32_t)b);
    return true;
}
