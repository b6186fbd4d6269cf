// locate_main.cpp -- fbg_locate: pattern search in an elastic founder graph through the pattern index of
// libfbg_hip.so (include/fbg_hip.h, fbg_pindex_*).  Stands in for locate_patterns of the reference with a graph in
// place of its .index file:
//
//   fbg_locate --graph=efg.xgfa [--patterns=FILE] [--error-on-not-found] [--occurrences[=M]] [--seeds[=L]] [--msa=msa.fasta]
//              [--chain[=BAND]] [--strands] [--complement=FROMTO] [--rows] [--by-row] [--align[=PAD]] [--cigar]
//              [--graph-align[=PAD]] [--graph-cigar] [--gaf=FILE] [--mapq[=MARGIN]] [--pairs=MIN,MAX]
//              [--pair-align[=MAX_EDITS]]
//
// Patterns are whitespace-separated tokens from FILE or stdin, read as `std::cin >> pattern` reads them (a last
// token without whitespace after it sets EOF and is not answered, as in locate_patterns.cpp:47-53), and answered
// in one fbg_pindex_locate call.  stdout is byte for byte what locate_patterns prints for an index of that graph;
// stderr carries the messages.  --occurrences[=M] (M = 64 when left out) answers through fbg_pindex_occurrences instead
// and adds, after the line of every pattern that is found, one line per reported place:
//   E <tab> src S id <tab> dst S id <tab> offset      where the match ends: an index into label(src) + label(dst)
//   B <tab> src S id <tab> dst S id <tab> offset      where it begins
// at most M of each per pattern, the ends first; a list cut by M is followed by `E <tab> ... <tab> K more` (or B) with
// K the places left out.
// --seeds[=L] (L = 1 when left out) answers through fbg_pindex_seeds instead: every pattern cut greedily into the maximal
// pieces the search accepts, pieces of fewer than L symbols left out.  Per pattern `Pattern? K seeds found.`, then per seed
//   S <tab> q_start <tab> length <tab> count <tab> restarts
// followed, with --occurrences, by that seed's E / B lines as above; the last line is `Pattern? X out of Y patterns
// seeded`, X the patterns with a seed.  --error-on-not-found then fails at the first pattern without one.
// --msa=msa.fasta names the MSA the graph was cut from (read with the elastic rules: no gap filter).  The index is then
// built from that MSA and the segmentation of the graph's M and X lines (fbg_pindex_build_segmentation; block i ends at
// column X[i + 1] - 2, the last one at n), checked against the S lines (node count and label lengths), and every E / B
// line gets `<tab> row <tab> column` appended: the MSA cell, from 0, of that symbol in the representative row of its node
// (fbg_pindex_occurrences_msa / _seeds_msa; `*` in both for an offset outside the edge).  Without --occurrences the
// option only changes how the index is built.  A FASTA that does not fit the graph fails with a message.
// --chain[=BAND] (with --seeds, --msa and --occurrences[=M], M > 0) chains every pattern's seeds by the MSA columns of
// their start places (fbg_pindex_chains; BAND bounds the surplus of columns over pattern symbols between two neighbours of
// a chain, unbounded when left out) and prints, after the S / E / B lines of a pattern,
//   C <tab> score <tab> anchors                       symbols covered by the chain, places in it
//   A <tab> q_start <tab> length <tab> row <tab> column    per place of the chain, in pattern order: its seed and the MSA cell
//                                                     of the seed's first symbol
// --strands (with --seeds) searches every pattern also as its reverse complement (fbg_pindex_seeds_strands; A <-> T,
// C <-> G in either case, or the pairs of --complement=FROMTO, e.g. ATTACGGC: every first character maps to the second,
// every byte not named to itself).  A pattern's block as above is then followed by
//   - <tab> K                                         K the reported seeds of the reverse complement
// and that strand's S / E / B (/ C / A) lines in the same format, q_start counted in the reverse complement; with --chain
// a pattern closes with
//   T <tab> + | - | * <tab> score                     the strand whose chain scores higher (a tie: +; * if that chain is
//                                                     empty) and the higher score (fbg_pindex_chain_strands)
// A pattern counts as seeded with a seed on either strand, and --error-on-not-found fails at the first with none on both.
// --rows (with --seeds and --msa) builds the index with its row table (fbg_pindex_build_segmentation_rows) and appends
// `<tab> rows <tab> first` to every B line of a seed and to every C line: how many MSA rows carry the seed from that place
// on, or every anchor of the chain, and the smallest of them, from 0 (fbg_pindex_seeds_rows / _chains_rows; `*` for first
// when there is none: a place or chain that only a recombinant path of the graph spells).  Without --rows no line changes.
// --by-row (with --chain and --rows) chains every pattern along one MSA row instead (fbg_pindex_chains_by_row): the row
// whose supported start places chain best, the smallest among equals, and that row's chain.  Every C line then ends with
// `<tab> row <tab> n_best_rows`, the chosen row and the number of rows that reach its score (`*` and 0 where no row
// supports a start place); the C / A / T / G lines are those of these chains.  Without --by-row no byte changes.
// --align[=PAD] (with --chain and --rows) aligns every pattern against the smallest row that carries its chain, in a window
// of that row's gap-stripped text PAD symbols (default 16) around the chain's diagonals (fbg_pindex_chains_align), and
// prints after the A lines of a chain
//   G <tab> row <tab> edits <tab> t_start <tab> t_end   the fewest edits, and the stretch [t_start, t_end) of the row's text
// or `G <tab> *` when there is no alignment (no chain, no row that carries it, a pattern longer than the engine aligns).
// Without --align no line changes.
// --cigar (with --align) appends to the G line of every aligned pattern a sixth field, its alignment path against that
// stretch (fbg_pindex_chains_cigar): runs of = (equal symbols), X (a substitution), I (a pattern symbol with no symbol of
// the row) and D (a symbol of the row with no pattern symbol) in pattern order, such as 25=1X24=.  `G <tab> *` stays as it
// is, and without --cigar no line changes.
// --graph-align[=PAD] (with --chain and --rows) aligns every pattern against the graph of the blocks around its chain, PAD
// symbols (default 16) beyond the anchors (fbg_pindex_chains_align_graph), and prints after a chain's lines
//   H <tab> edits <tab> start_node <tab> start_offset <tab> end_node <tab> end_offset <tab> path
// the fewest edits, the S ids and offsets at which the stretch of the graph starts and ends, and the nodes from the start
// to the end as >u>v>w; or `H <tab> *` when there is no alignment.  Without --graph-align no byte changes.
// --graph-cigar (with --graph-align) appends to every H line with numbers an eighth field, the alignment path of the pattern
// against that stretch of the path's labels (fbg_pindex_chains_graph_cigar): runs of = X I D in pattern order and in path
// order, such as 25=1X24=.  `H <tab> *` stays as it is, and without --graph-cigar no byte changes.
// --gaf=FILE (with --graph-cigar) writes one GAF record per H line with numbers, in the order of those lines, to FILE;
// stdout does not change.  Tab-separated: read<k> (k the pattern's index in the input, from 0), L, 0, L (the pattern is
// aligned whole; I runs at either end stay in the CIGAR), + or - (the reverse complement), the path as >id>id, the sum of
// the path's label lengths, start_offset, that sum - |label(end_node)| + end_offset, the number of = symbols, the number of
// alignment columns (= X I D), 255, NM:i:edits and cg:Z:runs.  For - the CIGAR is in path order, PAF's convention.  A FILE
// that cannot be written fails before any search.
// --mapq[=MARGIN] (with --chain) finds every pattern's second-best chain outside the MSA columns of its chain, widened by
// MARGIN columns on either side (default 0), and a mapping quality from the two scores (fbg_pindex_chains_mapq): chains
// through other alleles in the same columns are the same locus and do not compete.  After a chain's C / A lines, before G / H,
//   Q <tab> mapq <tab> second <tab> second_lo <tab> second_hi    60 * (score - min(second, score)) / pattern length, floored;
//                                                     the second chain's score and its columns [second_lo, second_hi)
// with `*` for both columns where there is no second chain, and `Q <tab> 0 <tab> 0 <tab> * <tab> *` for an empty chain.  With
// --strands the other strand's chain competes too (fbg_pindex_mapq_strands): the Q line carries that value, and the T line
// gets a third field, the value of the chosen strand (0 for *).  With --gaf column 12 is the value of that pattern and
// strand instead of 255.  A pattern that matches in one piece has no seed at a shorter copy elsewhere: its second is 0.
// Without --mapq no byte of stdout or of the GAF file changes.
// --pairs=MIN,MAX (with --chain and --strands, an even number of patterns) reads the patterns as pairs of mates, patterns 2p
// and 2p + 1, from opposite strands of one fragment whose extent in MSA columns lies in MIN .. MAX (fbg_pindex_chains_pairs):
// every mate also gets a rescue chain on the start places inside the window that the other mate's chain opens, and the
// pair takes the best valid combination of a chain on one strand and a chain on the other.  The chosen chains replace the
// chains of their patterns and the other strand of either pattern gets the empty chain, before anything is printed: every
// C / A / Q / G / H / T line and the GAF file are those of the adopted chains.  After the T line of a pair's second pattern,
//   Z <tab> which <tab> pair_score <tab> t_lo <tab> t_hi    the candidate 0 .. 3, the sum of the two scores, the pair's columns
// or `Z <tab> *` for a pair without a valid combination, whose chains stay as they were.  The insert is counted in MSA
// columns, forward-reverse orientation only.  Without --pairs no byte of stdout or of the GAF file changes.
// --pair-align[=MAX_EDITS] (with --pairs and --rows) then aligns every strand of a pattern that has no chain, while the
// other mate's opposite strand has one, inside the window of MIN .. MAX symbols that this chain opens on the smallest row
// carrying it (fbg_pindex_pairs_align), and decides every pair again from these alignments.  After the other lines of a
// strand,
//   Y <tab> row <tab> edits <tab> t_start <tab> t_end <tab> insert    the row, the fewest edits of the pattern against the window,
// the stretch of the row's text it lies on, and the pair's extent in symbols of the row (* where there are more than
// MAX_EDITS edits or the extent is below MIN), or `Y <tab> *` where nothing was aligned; after a pair's Z line,
//   W <tab> which <tab> score <tab> lo <tab> hi    the candidate 0 .. 3, the chain's score plus the aligned pattern's length less
// its edits, the pair's extent on the row, or `W <tab> *`.  Without --pair-align no byte of stdout changes.
#include <algorithm>
#include <cerrno>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <string>
#include <vector>
#include "../../../include/fbg_hip.h"
#include "xgfa_read.hpp"
#include "fasta.hpp"

static int usage(const char *msg)
{
    std::cerr << "fbg_locate: " << msg << "\n"
              << "usage: fbg_locate --graph=efg.xgfa [--patterns=FILE] [--error-on-not-found] [--occurrences[=M]] [--seeds[=L]]\n"
              << "                  [--msa=msa.fasta] [--chain[=BAND]] [--strands] [--complement=FROMTO] [--rows]\n"
              << "                  [--by-row] [--align[=PAD]] [--cigar] [--graph-align[=PAD]] [--graph-cigar] [--gaf=FILE]\n"
              << "                  [--mapq[=MARGIN]] [--pairs=MIN,MAX] [--pair-align[=MAX_EDITS]]\n"
              << "  --occurrences[=M]  after every found pattern, the places where its matches end (E lines) and begin\n"
              << "                     (B lines): source S id, destination S id, offset into label(src) + label(dst);\n"
              << "                     at most M of each per pattern (default 64)\n"
              << "  --seeds[=L]        cut every pattern greedily into the maximal pieces the search accepts and print, per\n"
              << "                     piece of L symbols or more (default 1), an S line: q_start, length, count, restarts;\n"
              << "                     with --occurrences the E / B lines of every piece follow its S line\n"
              << "  --msa=msa.fasta    the MSA the graph was cut from: the index is built from it and the graph's M and X\n"
              << "                     lines, and every E / B line ends with the MSA row and column (from 0) of that symbol\n"
              << "                     in the representative row of its node (* for an offset outside the edge)\n"
              << "  --chain[=BAND]     needs --seeds, --msa and --occurrences[=M] with M > 0: after a pattern's S / E / B lines a\n"
              << "                     C line (score, anchors) and per anchor of its best co-linear chain of start places an A\n"
              << "                     line: q_start, length, MSA row, MSA column; BAND bounds the surplus of columns over\n"
              << "                     pattern symbols between neighbours (default: unbounded)\n"
              << "  --strands          needs --seeds: every pattern also as its reverse complement; after a pattern's block a\n"
              << "                     line `- K` and the K seeds of the reverse complement in the same format; with --chain a\n"
              << "                     closing T line: + or - for the strand of the better chain (* if it is empty), its score\n"
              << "  --complement=FROMTO  pairs of characters for --strands, e.g. ATTACGGC (the default, and the same in lower\n"
              << "                     case); every byte not named maps to itself\n"
              << "  --rows             needs --seeds and --msa: every B line of a seed and every C line ends with the number\n"
              << "                     of MSA rows that carry the seed from that place on (the C line: every anchor of the\n"
              << "                     chain) and the smallest such row, from 0 (* if no row does: only a recombinant path\n"
              << "                     of the graph spells it); no other line changes\n"
              << "  --by-row           needs --chain and --rows: chain every pattern along the one MSA row whose supported\n"
              << "                     start places chain best (the smallest among equals); every C line ends with that row\n"
              << "                     and the number of rows that reach its score (* and 0 if no row supports a place)\n"
              << "  --align[=PAD]      needs --chain and --rows: after the A lines of a chain a G line: the smallest row that\n"
              << "                     carries the chain, the fewest edits between the pattern and a stretch of that row's\n"
              << "                     gap-stripped text within PAD symbols (default 16) of the chain, and that stretch's start\n"
              << "                     and end in the row's text, from 0 (G and * if there is no alignment)\n"
              << "  --cigar            needs --align: a G line with numbers ends with the alignment path of the pattern against\n"
              << "                     that stretch, runs of = X I D in pattern order (25=1X24=); no other line changes\n"
              << "  --graph-align[=PAD]  needs --chain and --rows: after a chain's lines an H line: the fewest edits between the\n"
              << "                     pattern and a stretch of a path of the graph through the blocks around the chain, PAD\n"
              << "                     symbols (default 16) beyond its anchors, the node and offset at which that stretch\n"
              << "                     starts and ends, and the path as >u>v>w (H and * if there is no alignment)\n"
              << "  --graph-cigar      needs --graph-align: an H line with numbers ends with the alignment path of the pattern\n"
              << "                     against that stretch, runs of = X I D in pattern and path order; no other line changes\n"
              << "  --gaf=FILE         needs --graph-cigar: one GAF record per H line with numbers goes to FILE (read<k>, the\n"
              << "                     path as >id>id with its coordinates, matches, alignment columns, 255, NM:i: and cg:Z:)\n"
              << "  --mapq[=MARGIN]    needs --chain: after a chain's C / A lines a Q line: mapping quality 0 .. 60, the score of\n"
              << "                     the best chain outside the chain's MSA columns widened by MARGIN (default 0), and that\n"
              << "                     chain's columns (* without one); chains in the same columns are the same locus.  With\n"
              << "                     --strands the other strand competes too and the T line ends with the chosen strand's\n"
              << "                     value; with --gaf column 12 is the value instead of 255.  A pattern matched in one\n"
              << "                     piece has no seed at a shorter copy elsewhere and gets second 0\n"
              << "  --pairs=MIN,MAX    needs --chain and --strands and an even number of patterns: patterns 2p and 2p + 1 are\n"
              << "                     mates on opposite strands, MIN .. MAX MSA columns from the forward mate's first to the\n"
              << "                     reverse mate's last; a mate is chained again inside the window of the other's chain, the\n"
              << "                     best valid combination replaces the pair's chains (every line then describes those), and\n"
              << "                     after the second pattern's T line a Z line: candidate, pair score, first and last column\n"
              << "                     (Z and * without a valid combination)\n"
              << "  --pair-align[=MAX_EDITS]  needs --pairs and --rows: a strand without a chain is aligned inside the window of\n"
              << "                     MIN .. MAX symbols that the other mate's chain opens on the smallest row carrying it; after\n"
              << "                     a strand's lines a Y line: row, edits, start and end in the row's text, the pair's extent\n"
              << "                     in symbols (* with more than MAX_EDITS edits or below MIN; Y and * if nothing was aligned),\n"
              << "                     and after a pair's Z line a W line: candidate, score, first and last position on the row\n"
              << "                     (W and * without one)\n";
    return EXIT_FAILURE;
}

// The M line (rows, columns) and the X line (the first column of every block, from 1) of an xGFA file.
static bool read_segmentation(const std::string &path, uint64_t &m, uint64_t &n, std::vector<uint64_t> &starts, std::string &error)
{
    std::ifstream is(path, std::ios::binary);
    if (!is) { error = "cannot open " + path; return false; }
    bool have_m = false, have_x = false;
    std::string line;
    while (std::getline(is, line)) {
        if (!line.empty() && line.back() == '\r') line.pop_back();
        if (line.size() < 2 || (line[0] != 'M' && line[0] != 'X') || line[1] != '\t') continue;
        std::vector<uint64_t> v;
        size_t a = 2;
        while (a <= line.size()) {
            size_t b = line.find('\t', a);
            if (b == std::string::npos) b = line.size();
            const std::string f = line.substr(a, b - a);
            if (f.empty() && b == line.size()) break;                         // a trailing tab
            if (f.empty() || f.size() > 19 || f.find_first_not_of("0123456789") != std::string::npos) {
                error = path + ": malformed " + line[0] + " line";
                return false;
            }
            v.push_back(std::strtoull(f.c_str(), nullptr, 10));
            a = b + 1;
        }
        if (line[0] == 'M') {
            if (have_m || v.size() != 2) { error = path + ": malformed or repeated M line"; return false; }
            have_m = true; m = v[0]; n = v[1];
        } else {
            if (have_x) { error = path + ": a second X line"; return false; }
            have_x = true; starts = v;
        }
    }
    if (!have_m || !have_x || starts.empty()) { error = path + ": --msa needs the graph's M and X lines"; return false; }
    return true;
}

// the E / B lines of item k of a place state: offsets o[2], totals t[2], places p[6] (end src / dst / offset, start ...);
// rc (NULL without --msa): end row / column, start row / column; rows (NULL without --rows): per start its supporting
// rows and the first of them
static void print_row_set(uint32_t n_rows, uint32_t first)
{
    std::cout << '\t' << n_rows << '\t';
    if (first == 0xffffffffu) std::cout << '*';
    else std::cout << first;
}

static void print_places(const XgfaGraph &g, uint64_t k, const std::vector<uint64_t> *const o[2], const std::vector<uint64_t> *const t[2],
                         const std::vector<uint32_t> *p, const std::vector<uint32_t> *rc = nullptr,
                         const std::vector<uint32_t> *rows = nullptr)
{
    for (int w = 0; w < 2; w++) {
        const std::vector<uint64_t> &off = *o[w];
        const uint64_t total = (*t[w])[k];
        const char *tag = w ? "B\t" : "E\t";
        for (uint64_t i = off[k]; i < off[k + 1]; i++) {
            std::cout << tag << g.ids[p[3 * w][i]] << '\t' << g.ids[p[3 * w + 1][i]] << '\t' << p[3 * w + 2][i];
            if (rc) {
                const uint32_t r = rc[2 * w][i], c = rc[2 * w + 1][i];
                if (r == 0xffffffffu && c == 0xffffffffu) std::cout << "\t*\t*";
                else std::cout << '\t' << r << '\t' << c;
            }
            if (w && rows) print_row_set(rows[0][i], rows[1][i]);
            std::cout << '\n';
        }
        if (total > off[k + 1] - off[k]) std::cout << tag << "...\t" << total - (off[k + 1] - off[k]) << " more\n";
    }
}

// the runs ops[a .. b) as 25=1X24=
static void print_runs(std::ostream &os, const std::vector<uint32_t> &ops, uint64_t a, uint64_t b)
{
    for (uint64_t i = a; i < b; i++) {
        const uint32_t code = ops[i] & 15;
        os << (ops[i] >> 4) << (code == FBG_CIGAR_EQ ? '=' : code == FBG_CIGAR_X ? 'X' : code == FBG_CIGAR_I ? 'I' : 'D');
    }
}

int main(int argc, char **argv)
{
    std::string graph, patterns, msa_path, complement, gaf_path;
    bool graph_cigar = false, have_gaf = false, want_mapq = false, want_pairs = false, pair_align = false;
    uint32_t max_edits = 0xffffffffu;
    uint64_t min_insert = 0, max_insert = 0;
    uint64_t margin = 0;
    bool have_msa = false, have_complement = false, strands = false, rows = false, align = false, cigar = false, by_row = false, graph_align = false;
    uint64_t graph_pad = 16;
    uint64_t pad = 16;
    bool have_graph = false, have_patterns = false, error_on_not_found = false, occurrences = false, seeds = false, chain = false;
    uint64_t max_places = 64, min_seed = 1, band = UINT64_MAX;
    for (int i = 1; i < argc; i++) {
        const std::string a = argv[i];
        auto value = [&](const char *name, std::string &out, bool &have) {
            const std::string pre = std::string(name) + "=";
            if (a.compare(0, pre.size(), pre) == 0) { out = a.substr(pre.size()); have = true; return true; }
            if (a == name && i + 1 < argc) { out = argv[++i]; have = true; return true; }
            return false;
        };
        if (value("--graph", graph, have_graph) || value("--patterns", patterns, have_patterns) ||
            value("--msa", msa_path, have_msa) || value("--complement", complement, have_complement) ||
            value("--gaf", gaf_path, have_gaf)) continue;
        if (a == "--strands") { strands = true; continue; }
        if (a == "--rows") { rows = true; continue; }
        if (a == "--by-row") { by_row = true; continue; }
        if (a == "--error-on-not-found") { error_on_not_found = true; continue; }
        if (a == "--occurrences") { occurrences = true; continue; }
        if (a.compare(0, 14, "--occurrences=") == 0) {
            const std::string v = a.substr(14);
            char *end = nullptr;
            errno = 0;
            const unsigned long long m = std::strtoull(v.c_str(), &end, 10);
            if (v.empty() || v.find_first_not_of("0123456789") != std::string::npos || errno || *end)
                return usage(("--occurrences takes a count, not '" + v + "'").c_str());
            occurrences = true;
            max_places = m;
            continue;
        }
        if (a == "--seeds") { seeds = true; continue; }
        if (a.compare(0, 8, "--seeds=") == 0) {
            const std::string v = a.substr(8);
            char *end = nullptr;
            errno = 0;
            const unsigned long long m = std::strtoull(v.c_str(), &end, 10);
            if (v.empty() || v.find_first_not_of("0123456789") != std::string::npos || errno || *end || m == 0)
                return usage(("--seeds takes a positive count, not '" + v + "'").c_str());
            seeds = true;
            min_seed = m;
            continue;
        }
        if (a == "--chain") { chain = true; continue; }
        if (a.compare(0, 8, "--chain=") == 0) {
            const std::string v = a.substr(8);
            char *end = nullptr;
            errno = 0;
            const unsigned long long m = std::strtoull(v.c_str(), &end, 10);
            if (v.empty() || v.find_first_not_of("0123456789") != std::string::npos || errno || *end)
                return usage(("--chain takes a band, not '" + v + "'").c_str());
            chain = true;
            band = m;
            continue;
        }
        if (a == "--cigar") { cigar = true; continue; }
        if (a == "--align") { align = true; continue; }
        if (a.compare(0, 8, "--align=") == 0) {
            const std::string v = a.substr(8);
            char *end = nullptr;
            errno = 0;
            const unsigned long long m = std::strtoull(v.c_str(), &end, 10);
            if (v.empty() || v.find_first_not_of("0123456789") != std::string::npos || errno || *end)
                return usage(("--align takes a pad, not '" + v + "'").c_str());
            align = true;
            pad = m;
            continue;
        }
        if (a == "--graph-cigar") { graph_cigar = true; continue; }
        if (a == "--graph-align") { graph_align = true; continue; }
        if (a.compare(0, 14, "--graph-align=") == 0) {
            const std::string v = a.substr(14);
            char *end = nullptr;
            errno = 0;
            const unsigned long long m = std::strtoull(v.c_str(), &end, 10);
            if (v.empty() || v.find_first_not_of("0123456789") != std::string::npos || errno || *end)
                return usage(("--graph-align takes a pad, not '" + v + "'").c_str());
            graph_align = true;
            graph_pad = m;
            continue;
        }
        if (a == "--mapq") { want_mapq = true; continue; }
        if (a.compare(0, 7, "--mapq=") == 0) {
            const std::string v = a.substr(7);
            char *end = nullptr;
            errno = 0;
            const unsigned long long m = std::strtoull(v.c_str(), &end, 10);
            if (v.empty() || v.find_first_not_of("0123456789") != std::string::npos || errno || *end)
                return usage(("--mapq takes a margin, not '" + v + "'").c_str());
            want_mapq = true;
            margin = m;
            continue;
        }
        if (a.compare(0, 8, "--pairs=") == 0) {
            const std::string v = a.substr(8);
            const size_t comma = v.find(',');
            const std::string lo = v.substr(0, comma), hi = comma == std::string::npos ? "" : v.substr(comma + 1);
            errno = 0;
            const unsigned long long x = std::strtoull(lo.c_str(), nullptr, 10), y = std::strtoull(hi.c_str(), nullptr, 10);
            if (lo.empty() || hi.empty() || lo.find_first_not_of("0123456789") != std::string::npos ||
                hi.find_first_not_of("0123456789") != std::string::npos || errno || x > y)
                return usage(("--pairs takes MIN,MAX with MIN <= MAX, not '" + v + "'").c_str());
            want_pairs = true;
            min_insert = x;
            max_insert = y;
            continue;
        }
        if (a == "--pair-align") { pair_align = true; continue; }
        if (a.compare(0, 13, "--pair-align=") == 0) {
            const std::string v = a.substr(13);
            char *end = nullptr;
            errno = 0;
            const unsigned long long m = std::strtoull(v.c_str(), &end, 10);
            if (v.empty() || v.find_first_not_of("0123456789") != std::string::npos || errno || *end || m > 0xffffffffull)
                return usage(("--pair-align takes a number of edits, not '" + v + "'").c_str());
            pair_align = true;
            max_edits = (uint32_t)m;
            continue;
        }
        if (a == "--help" || a == "-h") { usage("pattern search in a founder graph"); return EXIT_SUCCESS; }
        return usage(("unknown argument " + a).c_str());
    }
    if (!have_graph || graph.empty()) return usage("--graph is required");
    if (have_msa && msa_path.empty()) return usage("--msa takes a FASTA file");
    if (chain && !(seeds && have_msa && occurrences && max_places > 0))
        return usage("--chain needs --seeds, --msa and --occurrences[=M] with M > 0");
    if (strands && !seeds) return usage("--strands needs --seeds");
    if (rows && !(seeds && have_msa)) return usage("--rows needs --seeds and --msa");
    if (by_row && !(chain && rows)) return usage("--by-row needs --chain and --rows");
    if (cigar && !align) return usage("--cigar needs --align");
    if (align && !(chain && rows)) return usage("--align needs --chain and --rows");
    if (graph_align && !(chain && rows)) return usage("--graph-align needs --chain and --rows");
    if (graph_cigar && !graph_align) return usage("--graph-cigar needs --graph-align");
    if (have_gaf && !graph_cigar) return usage("--gaf needs --graph-cigar");
    if (want_mapq && !chain) return usage("--mapq needs --chain");
    if (want_pairs && !(chain && strands)) return usage("--pairs needs --chain and --strands");
    if (pair_align && !(want_pairs && rows)) return usage("--pair-align needs --pairs and --rows");
    if (have_gaf && gaf_path.empty()) return usage("--gaf takes a file");
    if (have_complement && !strands) return usage("--complement needs --strands");
    if (have_complement && (complement.empty() || complement.size() % 2)) return usage("--complement takes pairs of characters");

    std::ofstream gaf;
    if (have_gaf) {
        gaf.open(gaf_path, std::ios::binary | std::ios::trunc);
        if (!gaf) { std::cerr << "fbg_locate: cannot write " << gaf_path << "\n"; return EXIT_FAILURE; }
    }
    XgfaGraph g;
    std::string error;
    if (!read_xgfa_graph(graph, g, error)) { std::cerr << "fbg_locate: " << error << "\n"; return EXIT_FAILURE; }

    Msa msa;
    std::vector<uint64_t> bounds;                   // inclusive block ends, the last one n (fbg_minmax_dp's convention)
    if (have_msa) {
        uint64_t gm = 0, gn = 0;
        std::vector<uint64_t> xs;
        if (!read_segmentation(graph, gm, gn, xs, error)) { std::cerr << "fbg_locate: " << error << "\n"; return EXIT_FAILURE; }
        if (!read_msa(msa_path, 1, true, false, msa)) { std::cerr << "fbg_locate: cannot open " << msa_path << "\n"; return EXIT_FAILURE; }
        if (msa.m != gm || msa.n != gn) {
            std::cerr << "fbg_locate: " << msa_path << " does not fit " << graph << ": the MSA has " << msa.m << " rows and " << msa.n
                      << " columns, the M line says " << gm << " and " << gn << "\n";
            return EXIT_FAILURE;
        }
        for (size_t i = 1; i < xs.size(); i++) {
            if (xs[i] < 2) { std::cerr << "fbg_locate: " << graph << ": malformed X line\n"; return EXIT_FAILURE; }
            bounds.push_back(xs[i] - 2);
        }
        bounds.push_back(gn);
    }

    std::ifstream pf;
    if (have_patterns) {
        pf.open(patterns, std::ios::binary);
        if (!pf) { std::cerr << "fbg_locate: cannot open " << patterns << "\n"; return EXIT_FAILURE; }
    }
    std::istream &in = have_patterns ? static_cast<std::istream &>(pf) : std::cin;
    std::ios_base::sync_with_stdio(false);
    std::string data;
    std::vector<uint64_t> off(1, 0);
    while (true) {
        std::string p;
        in >> p;
        if (in.eof()) break;           // also drops a last token that ends the input (locate_patterns.cpp:47-53)
        if (!in) { std::cerr << "fbg_locate: cannot read the patterns\n"; return EXIT_FAILURE; }
        data += p;
        off.push_back(data.size());
    }
    const uint64_t np = off.size() - 1;
    const uint64_t nv = strands ? 2 * np : np;      // virtual reads: the patterns, then their reverse complements
    if (want_pairs && np % 2) return usage("--pairs takes an even number of patterns, mates interleaved");

    fbg_ctx *ctx = nullptr;
    int rc = fbg_ctx_create(0, &ctx);
    if (rc != FBG_OK) { std::cerr << "fbg_locate: " << fbg_last_error(nullptr) << "\n"; return EXIT_FAILURE; }
    const uint64_t nodes = g.label_off.size() - 1;
    fbg_pindex *ix = nullptr;
    if (have_msa) {
        // the index of the MSA's segmentation, which must be the graph that was read
        std::string why;
        if (bounds.size() > 1 && !std::is_sorted(bounds.begin(), bounds.end() - 1)) why = "the X line does not increase";
        rc = fbg_msa_load_host(ctx, msa.cells.data(), msa.m, msa.n);
        if (rc == FBG_OK && why.empty())
            rc = rows ? fbg_pindex_build_segmentation_rows(ctx, bounds.data(), bounds.size(), &ix)
                      : fbg_pindex_build_segmentation(ctx, bounds.data(), bounds.size(), &ix);
        if (rc == FBG_OK && why.empty()) {
            std::vector<uint32_t> len(nodes + 1);
            if (fbg_pindex_node_count(ix) != nodes)
                why = "its segmentation has " + std::to_string(fbg_pindex_node_count(ix)) + " nodes, the graph " + std::to_string(nodes);
            else if ((rc = fbg_pindex_node_info(ix, len.data(), nullptr, nullptr)) == FBG_OK)
                for (uint64_t u = 0; u < nodes && why.empty(); u++)
                    if (len[u] != g.label_off[u + 1] - g.label_off[u])
                        why = "node " + std::to_string(g.ids[u]) + " has " + std::to_string(g.label_off[u + 1] - g.label_off[u]) +
                              " symbols in the graph and " + std::to_string(len[u]) + " in the MSA";
        }
        if (!why.empty()) {
            std::cerr << "fbg_locate: " << msa_path << " does not fit " << graph << ": " << why << "\n";
            fbg_pindex_destroy(ix);
            fbg_ctx_destroy(ctx);
            return EXIT_FAILURE;
        }
    } else {
        rc = fbg_pindex_build(ctx, (const uint8_t *)g.labels.data(), g.label_off.data(), nodes, g.edge_off.data(),
                              g.edge_dst.data(), &ix);
    }
    std::vector<uint32_t> coords[4];                // end row / column, start row / column (--msa with --occurrences)
    const bool want_coords = have_msa && occurrences;
    std::vector<uint64_t> count(np + 1), pos(np + 1), end_off, start_off, end_total, start_total;
    std::vector<uint32_t> restarts, places[6];      // end src / dst / offset, start src / dst / offset
    if (occurrences) {
        for (std::vector<uint64_t> *v : {&end_off, &start_off, &end_total, &start_total}) v->assign(np + 1, 0);
        restarts.assign(np + 1, 0);
    }
    std::vector<uint64_t> seed_off(nv + 1, 0), seed_count;
    std::vector<uint32_t> q_start, length;
    std::vector<uint64_t> chain_off(nv + 1, 0);
    std::vector<uint32_t> chain_score(nv + 1, 0), anchor_place, anchor_seed, best_score(np + 1, 0);
    std::vector<uint8_t> strand(np + 1, 0);
    std::vector<uint32_t> place_rows[2], chain_rows[2];     // --rows: supporting rows and the first of them
    std::vector<uint32_t> chosen[2];                        // --by-row: the chosen row and the rows that reach its score
    std::vector<uint32_t> aligned[4];                       // --align: row, edits, t_start, t_end
    std::vector<uint64_t> cigar_off(nv + 1, 0);             // --cigar: the runs of every virtual read
    std::vector<uint32_t> cigar_ops;
    std::vector<uint32_t> on_graph[5];                      // --graph-align: edits, start node and offset, end node and offset
    std::vector<uint64_t> path_off(nv + 1, 0);
    std::vector<uint32_t> path_nodes;
    std::vector<uint64_t> gcigar_off(nv + 1, 0);            // --graph-cigar: the runs of every virtual read
    std::vector<uint32_t> gcigar_ops;
    std::vector<uint64_t> second_off(nv + 1, 0);            // --mapq: the second chains' offsets, scores and spans, the qualities
    std::vector<uint32_t> second[3];
    std::vector<uint8_t> quality(nv + 1, 0);
    std::vector<uint8_t> pair_which(np / 2 + 1, 0);        // --pairs: the candidate, its score and columns per pair
    std::vector<uint32_t> pair_out[3];
    std::vector<uint32_t> mate[5], mate_out[3];             // --pair-align: row, edits, t_start, t_end, insert; score, lo, hi
    std::vector<uint8_t> mate_which(np / 2 + 1, 0);
    if (rc == FBG_OK && seeds) {
        if (strands) {
            uint8_t table[256];
            for (int c = 0; c < 256; c++) table[c] = (uint8_t)c;
            for (size_t i = 0; i + 1 < complement.size(); i += 2) table[(uint8_t)complement[i]] = (uint8_t)complement[i + 1];
            rc = fbg_pindex_seeds_strands(ix, (const uint8_t *)data.data(), off.data(), np, have_complement ? table : nullptr,
                                          min_seed, occurrences ? max_places : 0, seed_off.data(), nullptr);
        } else {
            rc = fbg_pindex_seeds(ix, (const uint8_t *)data.data(), off.data(), np, min_seed, occurrences ? max_places : 0,
                                  seed_off.data(), nullptr);
        }
        const uint64_t ns = rc == FBG_OK ? seed_off[nv] : 0;
        for (std::vector<uint64_t> *v : {&seed_count, &end_off, &start_off, &end_total, &start_total}) v->assign(ns + 1, 0);
        for (std::vector<uint32_t> *v : {&q_start, &length, &restarts}) v->assign(ns + 1, 0);
        if (rc == FBG_OK)
            rc = fbg_pindex_seeds_fetch(ix, q_start.data(), length.data(), seed_count.data(), restarts.data(), end_total.data(),
                                        start_total.data(), end_off.data(), start_off.data(), nullptr);
        if (rc == FBG_OK) {
            for (int k = 0; k < 6; k++) places[k].resize((k < 3 ? end_off[ns] : start_off[ns]) + 1);
            rc = fbg_pindex_seeds_places(ix, places[0].data(), places[1].data(), places[2].data(), places[3].data(),
                                         places[4].data(), places[5].data(), nullptr);
        }
        if (rc == FBG_OK && want_coords) {
            for (int k = 0; k < 4; k++) coords[k].resize((k < 2 ? end_off[ns] : start_off[ns]) + 1);
            rc = fbg_pindex_seeds_msa(ix, coords[0].data(), coords[1].data(), coords[2].data(), coords[3].data(), nullptr);
        }
        if (rc == FBG_OK && chain && by_row) {
            for (int k = 0; k < 2; k++) chosen[k].resize(nv + 1);
            rc = fbg_pindex_chains_by_row(ix, band, 0, chain_off.data(), chain_score.data(), chosen[0].data(), chosen[1].data(), nullptr);
        } else if (rc == FBG_OK && chain) rc = fbg_pindex_chains(ix, band, 0, chain_off.data(), chain_score.data(), nullptr);
        if (rc == FBG_OK && want_pairs) {      // adopt: chain_off and chain_score become those of the pair-consistent chains
            std::vector<uint64_t> rescue_off(nv + 1, 0);
            for (int k = 0; k < 3; k++) pair_out[k].resize(np / 2 + 1);
            rc = fbg_pindex_chains_pairs(ix, min_insert, max_insert, pair_which.data(), pair_out[0].data(), pair_out[1].data(),
                                         pair_out[2].data(), rescue_off.data(), nullptr, nullptr, nullptr, nullptr, nullptr,
                                         chain_off.data(), chain_score.data(), nullptr, nullptr);
        }
        if (rc == FBG_OK && pair_align) {      // on the adopted chains; writes nothing that a later stage reads
            for (int k = 0; k < 5; k++) mate[k].resize(nv + 1);
            for (int k = 0; k < 3; k++) mate_out[k].resize(np / 2 + 1);
            rc = fbg_pindex_pairs_align(ix, min_insert, max_insert, max_edits, 0, nullptr, mate[0].data(), mate[1].data(), mate[2].data(),
                                        mate[3].data(), mate[4].data(), mate_which.data(), mate_out[0].data(), mate_out[1].data(),
                                        mate_out[2].data(), nullptr, nullptr);
        }
        if (rc == FBG_OK && chain) {
            anchor_place.resize(chain_off[nv] + 1);
            anchor_seed.resize(chain_off[nv] + 1);
            rc = fbg_pindex_chains_fetch(ix, anchor_place.data(), anchor_seed.data(), nullptr);
        }
        if (rc == FBG_OK && chain && strands)
            rc = fbg_pindex_chain_strands(ix, strand.data(), best_score.data(), nullptr, nullptr, nullptr, nullptr);
        if (rc == FBG_OK && want_mapq) {
            for (int k = 0; k < 3; k++) second[k].resize(nv + 1);
            rc = fbg_pindex_chains_mapq(ix, margin, second_off.data(), second[0].data(), second[1].data(), second[2].data(),
                                        quality.data(), nullptr);
            if (rc == FBG_OK && strands) rc = fbg_pindex_mapq_strands(ix, quality.data(), nullptr);
        }
        if (rc == FBG_OK && rows && occurrences) {
            for (int k = 0; k < 2; k++) place_rows[k].resize(start_off[ns] + 1);
            rc = fbg_pindex_seeds_rows(ix, place_rows[0].data(), place_rows[1].data(), nullptr);
        }
        if (rc == FBG_OK && rows && chain) {
            for (int k = 0; k < 2; k++) chain_rows[k].resize(nv + 1);
            rc = fbg_pindex_chains_rows(ix, chain_rows[0].data(), chain_rows[1].data(), nullptr, nullptr);
        }
        if (rc == FBG_OK && align) {
            for (int k = 0; k < 4; k++) aligned[k].resize(nv + 1);
            rc = fbg_pindex_chains_align(ix, pad, 0, aligned[0].data(), aligned[1].data(), aligned[2].data(), aligned[3].data(), nullptr);
        }
        if (rc == FBG_OK && cigar) {
            uint64_t total = 0;
            rc = fbg_pindex_chains_cigar(ix, nullptr, &total, nullptr);
            cigar_ops.resize(total + 1);
            if (rc == FBG_OK) rc = fbg_pindex_chains_cigar_fetch(ix, cigar_off.data(), cigar_ops.data());
        }
        if (rc == FBG_OK && graph_align) {
            uint64_t total = 0;
            for (int k = 0; k < 5; k++) on_graph[k].resize(nv + 1);
            rc = fbg_pindex_chains_align_graph(ix, graph_pad, 0, nullptr, on_graph[0].data(), on_graph[1].data(), on_graph[2].data(),
                                               on_graph[3].data(), on_graph[4].data(), nullptr, &total, nullptr);
            path_nodes.resize(total + 1);
            if (rc == FBG_OK) rc = fbg_pindex_chains_align_graph_fetch(ix, path_off.data(), path_nodes.data());
        }
        if (rc == FBG_OK && graph_cigar) {
            uint64_t total = 0;
            rc = fbg_pindex_chains_graph_cigar(ix, nullptr, &total, nullptr);
            gcigar_ops.resize(total + 1);
            if (rc == FBG_OK) rc = fbg_pindex_chains_graph_cigar_fetch(ix, gcigar_off.data(), gcigar_ops.data());
        }
    }
    if (rc == FBG_OK && !occurrences && !seeds)
        rc = fbg_pindex_locate(ix, (const uint8_t *)data.data(), off.data(), np, count.data(), pos.data());
    if (rc == FBG_OK && occurrences && !seeds)
        rc = fbg_pindex_occurrences(ix, (const uint8_t *)data.data(), off.data(), np, max_places, count.data(), pos.data(),
                                    restarts.data(), end_off.data(), start_off.data(), end_total.data(), start_total.data(), nullptr);
    if (rc == FBG_OK && occurrences && !seeds) {
        for (int k = 0; k < 6; k++) places[k].resize((k < 3 ? end_off[np] : start_off[np]) + 1);
        rc = fbg_pindex_occurrences_fetch(ix, places[0].data(), places[1].data(), places[2].data(), places[3].data(),
                                          places[4].data(), places[5].data(), nullptr);
    }
    if (rc == FBG_OK && want_coords && !seeds) {
        for (int k = 0; k < 4; k++) coords[k].resize((k < 2 ? end_off[np] : start_off[np]) + 1);
        rc = fbg_pindex_occurrences_msa(ix, coords[0].data(), coords[1].data(), coords[2].data(), coords[3].data(), nullptr);
    }
    if (rc != FBG_OK) {
        std::cerr << "fbg_locate: " << fbg_last_error(ctx) << "\n";
        fbg_pindex_destroy(ix);
        fbg_ctx_destroy(ctx);
        return EXIT_FAILURE;
    }
    fbg_pindex_destroy(ix);
    fbg_ctx_destroy(ctx);

    const std::vector<uint64_t> *const o[2] = {&end_off, &start_off}, *const t[2] = {&end_total, &start_total};
    uint64_t found = 0;
    if (seeds) {
        // the S / E / B (/ C / A) lines of virtual read v
        auto block = [&](uint64_t v) {
            for (uint64_t j = seed_off[v]; j < seed_off[v + 1]; j++) {
                std::cout << "S\t" << q_start[j] << '\t' << length[j] << '\t' << seed_count[j] << '\t' << restarts[j] << '\n';
                if (occurrences) print_places(g, j, o, t, places, want_coords ? coords : nullptr, rows ? place_rows : nullptr);
            }
            if (chain) {
                std::cout << "C\t" << chain_score[v] << '\t' << chain_off[v + 1] - chain_off[v];
                if (rows) print_row_set(chain_rows[0][v], chain_rows[1][v]);
                if (by_row) {
                    if (chosen[0][v] == 0xffffffffu) std::cout << "\t*";
                    else std::cout << '\t' << chosen[0][v];
                    std::cout << '\t' << chosen[1][v];
                }
                std::cout << '\n';
                for (uint64_t i = chain_off[v]; i < chain_off[v + 1]; i++)
                    std::cout << "A\t" << q_start[anchor_seed[i]] << '\t' << length[anchor_seed[i]] << '\t' << coords[2][anchor_place[i]]
                              << '\t' << coords[3][anchor_place[i]] << '\n';
                if (want_mapq) {
                    std::cout << "Q\t" << (unsigned)quality[v] << '\t' << second[0][v];
                    if (second_off[v + 1] == second_off[v]) std::cout << "\t*\t*\n";
                    else std::cout << '\t' << second[1][v] << '\t' << second[2][v] << '\n';
                }
                if (align && aligned[1][v] == FBG_ALIGN_NONE) std::cout << "G\t*\n";
                else if (align) {
                    std::cout << "G\t" << aligned[0][v] << '\t' << aligned[1][v] << '\t' << aligned[2][v] << '\t' << aligned[3][v];
                    if (cigar) {
                        std::cout << '\t';
                        print_runs(std::cout, cigar_ops, cigar_off[v], cigar_off[v + 1]);
                    }
                    std::cout << '\n';
                }
                if (graph_align && on_graph[0][v] == FBG_ALIGN_NONE) std::cout << "H\t*\n";
                else if (graph_align) {
                    std::cout << "H\t" << on_graph[0][v] << '\t' << g.ids[on_graph[1][v]] << '\t' << on_graph[2][v] << '\t'
                              << g.ids[on_graph[3][v]] << '\t' << on_graph[4][v] << '\t';
                    for (uint64_t i = path_off[v]; i < path_off[v + 1]; i++) std::cout << '>' << g.ids[path_nodes[i]];
                    if (graph_cigar) {
                        std::cout << '\t';
                        print_runs(std::cout, gcigar_ops, gcigar_off[v], gcigar_off[v + 1]);
                    }
                    std::cout << '\n';
                    if (have_gaf) {
                        const uint64_t k = v < np ? v : v - np, L = off[k + 1] - off[k];
                        uint64_t plen = 0, match = 0, cols = 0;
                        gaf << "read" << k << '\t' << L << "\t0\t" << L << '\t' << (v < np ? '+' : '-') << '\t';
                        for (uint64_t i = path_off[v]; i < path_off[v + 1]; i++) {
                            const uint32_t u = path_nodes[i];
                            gaf << '>' << g.ids[u];
                            plen += g.label_off[u + 1] - g.label_off[u];
                        }
                        for (uint64_t i = gcigar_off[v]; i < gcigar_off[v + 1]; i++) {
                            cols += gcigar_ops[i] >> 4;
                            if ((gcigar_ops[i] & 15) == FBG_CIGAR_EQ) match += gcigar_ops[i] >> 4;
                        }
                        const uint32_t ve = on_graph[3][v];
                        gaf << '\t' << plen << '\t' << on_graph[2][v] << '\t'
                            << plen - (g.label_off[ve + 1] - g.label_off[ve]) + on_graph[4][v] << '\t' << match << '\t' << cols
                            << '\t' << (want_mapq ? (unsigned)quality[v] : 255u) << "\tNM:i:" << on_graph[0][v] << "\tcg:Z:";
                        print_runs(gaf, gcigar_ops, gcigar_off[v], gcigar_off[v + 1]);
                        gaf << '\n';
                    }
                }
                if (pair_align && mate[1][v] == FBG_ALIGN_NONE) std::cout << "Y\t*\n";
                else if (pair_align) {
                    std::cout << "Y\t" << mate[0][v] << '\t' << mate[1][v] << '\t' << mate[2][v] << '\t' << mate[3][v] << '\t';
                    if (mate[4][v] == FBG_ALIGN_NONE) std::cout << "*\n";
                    else std::cout << mate[4][v] << '\n';
                }
            }
        };
        for (uint64_t k = 0; k < np; k++) {
            const uint64_t ns = seed_off[k + 1] - seed_off[k];
            const uint64_t nr = strands ? seed_off[np + k + 1] - seed_off[np + k] : 0;
            std::cout << "Pattern? " << ns << " seeds found.\n";
            if (ns + nr == 0 && error_on_not_found) {
                std::cerr << "Pattern has no seed.\n";
                std::cout.flush();
                return EXIT_FAILURE;
            }
            found += ns + nr != 0;
            block(k);
            if (strands) {
                std::cout << "-\t" << nr << '\n';
                block(np + k);
                if (chain) {
                    std::cout << "T\t" << (strand[k] == FBG_STRAND_NONE ? '*' : strand[k] ? '-' : '+') << '\t' << best_score[k];
                    if (want_mapq) std::cout << '\t' << (strand[k] == FBG_STRAND_NONE ? 0u : (unsigned)quality[strand[k] ? np + k : k]);
                    std::cout << '\n';
                    if (want_pairs && k % 2) {
                        const uint64_t p = k / 2;
                        if (pair_which[p] == 0xffu) std::cout << "Z\t*\n";
                        else std::cout << "Z\t" << (unsigned)pair_which[p] << '\t' << pair_out[0][p] << '\t' << pair_out[1][p] << '\t'
                                       << pair_out[2][p] << '\n';
                        if (pair_align && mate_which[p] == 0xffu) std::cout << "W\t*\n";
                        else if (pair_align)
                            std::cout << "W\t" << (unsigned)mate_which[p] << '\t' << mate_out[0][p] << '\t' << mate_out[1][p] << '\t'
                                      << mate_out[2][p] << '\n';
                    }
                }
            }
        }
        std::cout << "Pattern? " << found << " out of " << np << " patterns seeded" << std::endl;
        if (have_gaf) {
            gaf.close();
            if (!gaf) { std::cerr << "fbg_locate: cannot write " << gaf_path << "\n"; return EXIT_FAILURE; }
        }
        return EXIT_SUCCESS;
    }
    for (uint64_t k = 0; k < np; k++) {
        std::cout << "Pattern? " << count[k] << " occurrences found.\n";
        if (count[k] == 0) {
            std::cerr << "Pattern not found, pos = " << pos[k] << ".\n";
            if (error_on_not_found) { std::cout.flush(); return EXIT_FAILURE; }
        } else {
            found++;
            if (occurrences) print_places(g, k, o, t, places, want_coords ? coords : nullptr);
        }
    }
    std::cout << "Pattern? " << found << " out of " << np << " patterns found" << std::endl;
    return EXIT_SUCCESS;
}
