// host_selftest.cpp -- the host-side pieces of the program that need no GPU (FASTA input with the reference's row
// filters, xGFA writer, graph statistics) behind a command line, for the CPU tests (tests/test_host_io.py) and for
// sanitizer runs:
//     fbg_host_selftest FASTA GAP_LIMIT ELASTIC(0|1) PATHS(0|1) OUT.gfa [GRAPH=file] [BOUNDARY ...]
// GRAPH=file: the node / edge arrays as fbg_block_graph returns them (u64 nb, u64 m, u32 node_of[nb*m], u32 rep_row[nb*m],
// u64 first_node[nb+1], u64 edge_count[nb], u64 edges[nb*m]); the xGFA is then formatted from them (write_xgfa_graph),
// as the program does with the GPU's arrays, instead of from labels hashed on the host (write_xgfa).
// prints "m n" of the MSA as read, then (with boundaries given: inclusive block ends, the last one == n, fbg.cpp:2027-2039)
// writes the xGFA and prints "nodes total_label_length founders edges".
//     fbg_host_selftest tie-extent
// checks fbg_tie_extent (tie_extent.h, the size of a tie group as rank_scan.hip's k_tie_groups finds it) against the plain count
// it replaces: groups of 1 .. 70 and 8191 .. 8194 slots at the start of a sorted array, in its middle and ending exactly at
// `hi`, each also with `hi` cutting the group short; prints "tie_extent ok CASES" or the first case that differs.
//     fbg_host_selftest twin-hash KEYS.bin BITS
// counts the twins among the 64-bit keys of a file the way suffix_sort.hip's k_sample_twins does (twin_hash.h: a table of 2^BITS
// words and two counters, all filled with all-ones; one insertion per key) and prints "twin_hash TWINS PROBES", PROBES being
// the longest probe sequence of an insertion.
//     fbg_host_selftest twin-slots KEYS.bin BITS
// prints the first slot of every key, one per line.
//     fbg_host_selftest pindex-stages
// prints the table of pindex_stage.h as it acts: "stages NAME ...", then per stage X "begin X" and the stages still done when
// every stage was done and X begins, then per subset of done stages (bit i of MASK: stage i, marked by ps_finish) "need MASK"
// and per stage "-" where ps_missing finds it and its ancestors done, else the stage it names.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>
#include "fasta.hpp"
#include "xgfa.hpp"
#include "../tie_extent.h"
#include "../twin_hash.h"
#include "../pindex_stage.h"

static int tie_extent_selftest()
{
    const uint32_t cap = 8192;                          // rank_scan.hip: RS_BIG_MEMBERS
    std::vector<uint32_t> sizes;
    for (uint32_t s = 1; s <= 70; s++) sizes.push_back(s);
    for (uint32_t s = 8191; s <= 8194; s++) sizes.push_back(s);
    unsigned long long cases = 0;
    for (const uint32_t s : sizes)
        for (int where = 0; where < 3; where++) {       // the group at the array's start, in the middle, ending exactly at hi
            const uint64_t before = where == 0 ? 0 : 37, after = where == 2 ? 0 : 29;
            std::vector<uint64_t> keys;
            for (uint64_t i = 0; i < before; i++) keys.push_back(10 + i / 3);          // (small groups before and after)
            const uint64_t key = 1000;
            for (uint32_t i = 0; i < s; i++) keys.push_back(key);
            for (uint64_t i = 0; i < after; i++) keys.push_back(2000 + i / 2);
            const uint64_t k0 = before;
            uint64_t reads = 0;
            auto key_at = [&](uint64_t k) -> uint64_t {
                reads++;
                if (k >= keys.size()) { std::fprintf(stderr, "tie_extent: read of slot %llu beyond the array\n", (unsigned long long)k); std::exit(1); }
                return keys[k];
            };
            // hi: the array's end, and every place that cuts the group short by 0 .. 3 slots
            std::vector<uint64_t> his = {keys.size()};
            for (uint64_t cut = 0; cut <= 3 && cut < s; cut++) his.push_back(k0 + s - cut);
            for (const uint64_t hi : his) {
                uint32_t want = 1;
                while (k0 + want < hi && want <= cap && keys[k0 + want] == key) want++;
                reads = 0;
                const uint32_t got = fbg_tie_extent(k0, hi, cap, key, key_at);
                // FBG_TIE_PROBE slots one by one, then two reads per doubling: far below one read per member
                const uint64_t most = FBG_TIE_PROBE + 2 * 14;
                if (got != want || reads > most) {
                    std::printf("tie_extent differs: size %u position %d hi %llu: got %u, want %u, %llu reads\n", s, where,
                                (unsigned long long)hi, got, want, (unsigned long long)reads);
                    return 1;
                }
                cases++;
            }
        }
    std::printf("tie_extent ok %llu\n", cases);
    return 0;
}

static int pindex_stages_selftest()
{
    std::printf("stages");
    for (int s = 0; s < PS_COUNT; s++) std::printf(" %s", ps_table[s].name);
    std::printf("\n");
    for (int x = 0; x < PS_COUNT; x++) {
        bool done[PS_COUNT] = {};
        for (int s = 0; s < PS_COUNT; s++) ps_finish(done, (PsStage)s);
        ps_begin(done, (PsStage)x);
        std::printf("begin %s", ps_table[x].name);
        for (int s = 0; s < PS_COUNT; s++)
            if (done[s]) std::printf(" %s", ps_table[s].name);
        std::printf("\n");
    }
    for (unsigned mask = 0; mask < 1u << PS_COUNT; mask++) {
        bool done[PS_COUNT] = {};
        for (int s = 0; s < PS_COUNT; s++)
            if (mask >> s & 1) ps_finish(done, (PsStage)s);
        std::printf("need %u", mask);
        for (int y = 0; y < PS_COUNT; y++) {
            const int miss = ps_missing(done, (PsStage)y);
            std::printf(" %s", miss == PS_COUNT ? "-" : ps_table[miss].name);
        }
        std::printf("\n");
    }
    return 0;
}

static int twin_hash_selftest(const char *path, int bits, bool slots_only)
{
    FILE *fh = std::fopen(path, "rb");
    if (!fh || bits < 1 || bits > 30) { std::fprintf(stderr, "twin-hash: cannot read %s, or BITS not in 1 .. 30\n", path); return 2; }
    std::vector<uint64_t> keys;
    uint64_t k;
    while (std::fread(&k, 8, 1, fh) == 1) keys.push_back(k);
    std::fclose(fh);
    if (slots_only) {
        for (const uint64_t key : keys) std::printf("%llu\n", (unsigned long long)fbg_twin_slot(key, bits));
        return 0;
    }
    std::vector<uint64_t> table((1ull << bits) + 2, FBG_TWIN_EMPTY);
    uint64_t *counters = table.data() + (1ull << bits);
    uint64_t longest = 0;
    for (const uint64_t key : keys) {
        if (key == FBG_TWIN_EMPTY) { counters[1]++; continue; }
        uint64_t probes = 0;
        counters[0] += fbg_twin_insert(key, bits, [&](uint64_t slot, uint64_t kk) -> uint64_t {
            if (slot >= (1ull << bits)) { std::fprintf(stderr, "twin-hash: slot %llu beyond the table\n", (unsigned long long)slot); std::exit(1); }
            probes++;
            const uint64_t seen = table[slot];
            if (seen == FBG_TWIN_EMPTY) table[slot] = kk;
            return seen;
        });
        if (probes > longest) longest = probes;
    }
    std::printf("twin_hash %llu %llu\n", (unsigned long long)fbg_twin_total(counters[0], counters[1]), (unsigned long long)longest);
    return 0;
}

int main(int argc, char **argv)
{
    if (argc == 4 && (std::string(argv[1]) == "twin-hash" || std::string(argv[1]) == "twin-slots"))
        return twin_hash_selftest(argv[2], std::atoi(argv[3]), std::string(argv[1]) == "twin-slots");
    if (argc == 2 && std::string(argv[1]) == "tie-extent") return tie_extent_selftest();
    if (argc == 2 && std::string(argv[1]) == "pindex-stages") return pindex_stages_selftest();
    if (argc < 6) {
        std::fprintf(stderr, "usage: %s FASTA GAP_LIMIT ELASTIC PATHS OUT.gfa [BOUNDARY ...]\n", argv[0]);
        return 2;
    }
    Msa msa;
    if (!read_msa(argv[1], std::atol(argv[2]), std::atoi(argv[3]) != 0, std::atoi(argv[4]) != 0, msa)) {
        std::fprintf(stderr, "cannot read %s\n", argv[1]);
        return 3;
    }
    std::printf("%llu %llu\n", (unsigned long long)msa.m, (unsigned long long)msa.n);
    if (argc == 6 || msa.m == 0) return 0;
    std::vector<uint64_t> boundaries;
    int first_boundary = 6;
    BlockGraph g;
    bool have_graph = false;
    if (std::string(argv[6]).rfind("GRAPH=", 0) == 0) {
        first_boundary = 7;
        have_graph = true;
        FILE *fh = std::fopen(argv[6] + 6, "rb");
        uint64_t hdr[2];
        if (!fh || std::fread(hdr, 8, 2, fh) != 2) { std::fprintf(stderr, "cannot read %s\n", argv[6] + 6); return 5; }
        const uint64_t nb = hdr[0], m = hdr[1];
        g.node_of.resize(nb * m); g.rep_row.resize(nb * m); g.first_node.resize(nb + 1); g.edge_count.resize(nb); g.edges.resize(nb * m);
        const bool ok = std::fread(g.node_of.data(), 4, nb * m, fh) == nb * m && std::fread(g.rep_row.data(), 4, nb * m, fh) == nb * m &&
                        std::fread(g.first_node.data(), 8, nb + 1, fh) == nb + 1 && std::fread(g.edge_count.data(), 8, nb, fh) == nb &&
                        std::fread(g.edges.data(), 8, nb * m, fh) == nb * m;
        std::fclose(fh);
        if (!ok || m != msa.m) { std::fprintf(stderr, "%s does not hold the arrays of this MSA\n", argv[6] + 6); return 5; }
    }
    for (int i = first_boundary; i < argc; i++) boundaries.push_back(std::strtoull(argv[i], nullptr, 10));
    std::string error;
    const bool paths = std::atoi(argv[4]) != 0;
    if (!(have_graph ? write_xgfa_graph(msa, boundaries, g, paths, argv[5], error) : write_xgfa(msa, boundaries, paths, argv[5], error))) {
        std::fprintf(stderr, "%s\n", error.c_str());
        return 4;
    }
    const GraphStats st = segment_stats(msa, boundaries);
    std::printf("%llu %llu %llu %llu\n", (unsigned long long)st.nodes, (unsigned long long)st.total_label_length,
                (unsigned long long)st.founders, (unsigned long long)st.edges);
    return 0;
}
