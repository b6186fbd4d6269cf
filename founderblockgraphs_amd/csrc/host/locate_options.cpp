// locate_options.cpp -- see locate_options.hpp.
#include "locate_options.hpp"
#include <cerrno>
#include <cstdlib>

const char *locate_usage()
{
    return "usage: fbg_locate --graph=efg.xgfa [--patterns=FILE] [--error-on-not-found] [--occurrences[=M]] [--seeds[=L]]\n"
           "                  [--msa=msa.fasta] [--chain[=BAND]] [--strands] [--complement=FROMTO] [--rows]\n"
           "                  [--by-row] [--align[=PAD]] [--cigar] [--graph-align[=PAD]] [--graph-cigar] [--gaf=FILE]\n"
           "                  [--mapq[=MARGIN]] [--pairs=MIN,MAX] [--pair-align[=MAX_EDITS]]\n"
           "  --occurrences[=M]  after every found pattern, the places where its matches end (E lines) and begin\n"
           "                     (B lines): source S id, destination S id, offset into label(src) + label(dst);\n"
           "                     at most M of each per pattern (default 64)\n"
           "  --seeds[=L]        cut every pattern greedily into the maximal pieces the search accepts and print, per\n"
           "                     piece of L symbols or more (default 1), an S line: q_start, length, count, restarts;\n"
           "                     with --occurrences the E / B lines of every piece follow its S line\n"
           "  --msa=msa.fasta    the MSA the graph was cut from: the index is built from it and the graph's M and X\n"
           "                     lines, and every E / B line ends with the MSA row and column (from 0) of that symbol\n"
           "                     in the representative row of its node (* for an offset outside the edge)\n"
           "  --chain[=BAND]     needs --seeds, --msa and --occurrences[=M] with M > 0: after a pattern's S / E / B lines a\n"
           "                     C line (score, anchors) and per anchor of its best co-linear chain of start places an A\n"
           "                     line: q_start, length, MSA row, MSA column; BAND bounds the surplus of columns over\n"
           "                     pattern symbols between neighbours (default: unbounded)\n"
           "  --strands          needs --seeds: every pattern also as its reverse complement; after a pattern's block a\n"
           "                     line `- K` and the K seeds of the reverse complement in the same format; with --chain a\n"
           "                     closing T line: + or - for the strand of the better chain (* if it is empty), its score\n"
           "  --complement=FROMTO  pairs of characters for --strands, e.g. ATTACGGC (the default, and the same in lower\n"
           "                     case); every byte not named maps to itself\n"
           "  --rows             needs --seeds and --msa: every B line of a seed and every C line ends with the number\n"
           "                     of MSA rows that carry the seed from that place on (the C line: every anchor of the\n"
           "                     chain) and the smallest such row, from 0 (* if no row does: only a recombinant path\n"
           "                     of the graph spells it); no other line changes\n"
           "  --by-row           needs --chain and --rows: chain every pattern along the one MSA row whose supported\n"
           "                     start places chain best (the smallest among equals); every C line ends with that row\n"
           "                     and the number of rows that reach its score (* and 0 if no row supports a place)\n"
           "  --align[=PAD]      needs --chain and --rows: after the A lines of a chain a G line: the smallest row that\n"
           "                     carries the chain, the fewest edits between the pattern and a stretch of that row's\n"
           "                     gap-stripped text within PAD symbols (default 16) of the chain, and that stretch's start\n"
           "                     and end in the row's text, from 0 (G and * if there is no alignment)\n"
           "  --cigar            needs --align: a G line with numbers ends with the alignment path of the pattern against\n"
           "                     that stretch, runs of = X I D in pattern order (25=1X24=); no other line changes\n"
           "  --graph-align[=PAD]  needs --chain and --rows: after a chain's lines an H line: the fewest edits between the\n"
           "                     pattern and a stretch of a path of the graph through the blocks around the chain, PAD\n"
           "                     symbols (default 16) beyond its anchors, the node and offset at which that stretch\n"
           "                     starts and ends, and the path as >u>v>w (H and * if there is no alignment)\n"
           "  --graph-cigar      needs --graph-align: an H line with numbers ends with the alignment path of the pattern\n"
           "                     against that stretch, runs of = X I D in pattern and path order; no other line changes\n"
           "  --gaf=FILE         needs --graph-cigar: one GAF record per H line with numbers goes to FILE (read<k>, the\n"
           "                     path as >id>id with its coordinates, matches, alignment columns, 255, NM:i: and cg:Z:)\n"
           "  --mapq[=MARGIN]    needs --chain: after a chain's C / A lines a Q line: mapping quality 0 .. 60, the score of\n"
           "                     the best chain outside the chain's MSA columns widened by MARGIN (default 0), and that\n"
           "                     chain's columns (* without one); chains in the same columns are the same locus.  With\n"
           "                     --strands the other strand competes too and the T line ends with the chosen strand's\n"
           "                     value; with --gaf column 12 is the value instead of 255.  A pattern matched in one\n"
           "                     piece has no seed at a shorter copy elsewhere and gets second 0\n"
           "  --pairs=MIN,MAX    needs --chain and --strands and an even number of patterns: patterns 2p and 2p + 1 are\n"
           "                     mates on opposite strands, MIN .. MAX MSA columns from the forward mate's first to the\n"
           "                     reverse mate's last; a mate is chained again inside the window of the other's chain, the\n"
           "                     best valid combination replaces the pair's chains (every line then describes those), and\n"
           "                     after the second pattern's T line a Z line: candidate, pair score, first and last column\n"
           "                     (Z and * without a valid combination)\n"
           "  --pair-align[=MAX_EDITS]  needs --pairs and --rows: a strand without a chain is aligned inside the window of\n"
           "                     MIN .. MAX symbols that the other mate's chain opens on the smallest row carrying it; after\n"
           "                     a strand's lines a Y line: row, edits, start and end in the row's text, the pair's extent\n"
           "                     in symbols (* with more than MAX_EDITS edits or below MIN; Y and * if nothing was aligned),\n"
           "                     and after a pair's Z line a W line: candidate, score, first and last position on the row\n"
           "                     (W and * without one)\n";
}

// v as a decimal number of lo .. hi: digits only, and no more of them than 64 bits hold
static bool number(const std::string &v, uint64_t lo, uint64_t hi, uint64_t &out)
{
    errno = 0;
    const unsigned long long m = std::strtoull(v.c_str(), nullptr, 10);
    if (v.empty() || v.find_first_not_of("0123456789") != std::string::npos || errno || m < lo || m > hi) return false;
    out = m;
    return true;
}

// `a` as --name or --name=N of a numeric flag: `matched` says whether it is one, false that its N is no number of its range
static bool numeric_flag(const std::string &a, LocateOptions &o, bool &matched, std::string &error)
{
    const struct { const char *name, *noun; uint64_t lo, hi; bool LocateOptions::*on; uint64_t LocateOptions::*n; } flags[] = {
        {"--occurrences", "a count", 0, UINT64_MAX, &LocateOptions::occurrences, &LocateOptions::max_places},
        {"--seeds", "a positive count", 1, UINT64_MAX, &LocateOptions::seeds, &LocateOptions::min_seed},
        {"--chain", "a band", 0, UINT64_MAX, &LocateOptions::chain, &LocateOptions::band},
        {"--align", "a pad", 0, UINT64_MAX, &LocateOptions::align, &LocateOptions::pad},
        {"--graph-align", "a pad", 0, UINT64_MAX, &LocateOptions::graph_align, &LocateOptions::graph_pad},
        {"--mapq", "a margin", 0, UINT64_MAX, &LocateOptions::mapq, &LocateOptions::margin},
        {"--pair-align", "a number of edits", 0, 0xffffffffull, &LocateOptions::pair_align, &LocateOptions::max_edits},
    };
    for (const auto &f : flags) {
        const std::string pre = std::string(f.name) + "=";
        matched = a == f.name || a.compare(0, pre.size(), pre) == 0;
        if (!matched) continue;
        o.*f.on = true;
        if (a == f.name || number(a.substr(pre.size()), f.lo, f.hi, o.*f.n)) return true;
        error = std::string(f.name) + " takes " + f.noun + ", not '" + a.substr(pre.size()) + "'";
        return false;
    }
    return true;
}

bool parse_locate_options(int argc, char **argv, LocateOptions &o, std::string &error)
{
    const struct { const char *name; std::string LocateOptions::*value; bool LocateOptions::*have; } texts[] = {
        {"--graph", &LocateOptions::graph, &LocateOptions::have_graph},
        {"--patterns", &LocateOptions::patterns, &LocateOptions::have_patterns},
        {"--msa", &LocateOptions::msa_path, &LocateOptions::have_msa},
        {"--complement", &LocateOptions::complement, &LocateOptions::have_complement},
        {"--gaf", &LocateOptions::gaf_path, &LocateOptions::have_gaf},
    };
    const struct { const char *name; bool LocateOptions::*on; } switches[] = {
        {"--strands", &LocateOptions::strands},         {"--rows", &LocateOptions::rows},
        {"--by-row", &LocateOptions::by_row},           {"--error-on-not-found", &LocateOptions::error_on_not_found},
        {"--cigar", &LocateOptions::cigar},             {"--graph-cigar", &LocateOptions::graph_cigar},
    };
    for (int i = 1; i < argc; i++) {
        const std::string a = argv[i];
        bool matched = false;
        for (const auto &t : texts) {                   // --name=TEXT, or --name TEXT in two arguments
            const std::string pre = std::string(t.name) + "=";
            if (a.compare(0, pre.size(), pre) == 0) o.*t.value = a.substr(pre.size());
            else if (a == t.name && i + 1 < argc) o.*t.value = argv[++i];
            else continue;
            o.*t.have = matched = true;
            break;
        }
        for (const auto &s : switches)
            if (!matched && a == s.name) o.*s.on = matched = true;
        if (matched) continue;
        if (!numeric_flag(a, o, matched, error)) return false;
        if (matched) continue;
        if (a.compare(0, 8, "--pairs=") == 0) {         // no bare form: both numbers are required
            const std::string v = a.substr(8);
            const size_t comma = v.find(',');
            o.pairs = true;
            if (comma != std::string::npos && number(v.substr(0, comma), 0, UINT64_MAX, o.min_insert) &&
                number(v.substr(comma + 1), o.min_insert, UINT64_MAX, o.max_insert)) continue;
            error = "--pairs takes MIN,MAX with MIN <= MAX, not '" + v + "'";
            return false;
        }
        if (a == "--help" || a == "-h") { o.help = true; return true; }
        error = "unknown argument " + a;
        return false;
    }
    // what every option needs, in the order in which a command line that breaks several rules is answered
    const bool has_places = o.occurrences && o.max_places > 0;
    const struct { bool broken; const char *message; } rules[] = {
        {!o.have_graph || o.graph.empty(), "--graph is required"},
        {o.have_msa && o.msa_path.empty(), "--msa takes a FASTA file"},
        {o.chain && !(o.seeds && o.have_msa && has_places), "--chain needs --seeds, --msa and --occurrences[=M] with M > 0"},
        {o.strands && !o.seeds, "--strands needs --seeds"},
        {o.rows && !(o.seeds && o.have_msa), "--rows needs --seeds and --msa"},
        {o.by_row && !(o.chain && o.rows), "--by-row needs --chain and --rows"},
        {o.cigar && !o.align, "--cigar needs --align"},
        {o.align && !(o.chain && o.rows), "--align needs --chain and --rows"},
        {o.graph_align && !(o.chain && o.rows), "--graph-align needs --chain and --rows"},
        {o.graph_cigar && !o.graph_align, "--graph-cigar needs --graph-align"},
        {o.have_gaf && !o.graph_cigar, "--gaf needs --graph-cigar"},
        {o.mapq && !o.chain, "--mapq needs --chain"},
        {o.pairs && !(o.chain && o.strands), "--pairs needs --chain and --strands"},
        {o.pair_align && !(o.pairs && o.rows), "--pair-align needs --pairs and --rows"},
        {o.have_gaf && o.gaf_path.empty(), "--gaf takes a file"},
        {o.have_complement && !o.strands, "--complement needs --strands"},
        {o.have_complement && (o.complement.empty() || o.complement.size() % 2), "--complement takes pairs of characters"},
    };
    for (const auto &r : rules)
        if (r.broken) { error = r.message; return false; }
    return true;
}
