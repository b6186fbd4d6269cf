// locate_options.hpp -- the command line of fbg_locate (locate_main.cpp states what every option means): the options as a
// struct, their parser with the prerequisite rules, and the usage text.  No HIP or library header: CPU programs link it.
#pragma once
#include <cstdint>
#include <string>

struct LocateOptions {
    std::string graph, patterns, msa_path, complement, gaf_path;
    bool have_graph = false, have_patterns = false, have_msa = false, have_complement = false, have_gaf = false;
    bool error_on_not_found = false, strands = false, rows = false, by_row = false, cigar = false, graph_cigar = false;
    bool occurrences = false, seeds = false, chain = false, align = false, graph_align = false, mapq = false, pair_align = false;
    bool pairs = false;
    bool help = false;                              // --help or -h was met: nothing after it was read
    uint64_t max_places = 64, min_seed = 1, band = UINT64_MAX, pad = 16, graph_pad = 16, margin = 0, max_edits = 0xffffffffu;
    uint64_t min_insert = 0, max_insert = 0;
};

// false: `error` is the message of the first argument that does not parse or, with every argument read, of the first
// prerequisite rule that is broken
bool parse_locate_options(int argc, char **argv, LocateOptions &o, std::string &error);

// what follows the message line on stderr
const char *locate_usage();
