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
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <string>
#include <vector>
#include "../../../include/fbg_hip.h"
#include "xgfa_read.hpp"
#include "fasta.hpp"
#include "locate_options.hpp"

static int fail(const std::string &msg)
{
    std::cerr << "fbg_locate: " << msg << "\n";
    return EXIT_FAILURE;
}

static int usage(const std::string &msg)
{
    fail(msg);
    std::cerr << locate_usage();
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

// ---- what is searched, and what the stages give -------------------------------------------------------------------------

struct Reads {
    std::string data;                               // the patterns back to back
    std::vector<uint64_t> off{0};                   // [np + 1]
    uint64_t np = 0, nv = 0;                        // virtual reads: the patterns, then (--strands) their reverse complements
    const uint8_t *bytes() const { return (const uint8_t *)data.data(); }
};

struct Located { std::vector<uint64_t> count, pos; };
struct Places {                                     // the E / B lists, of the patterns or of the seeds
    std::vector<uint64_t> end_off, start_off, end_total, start_total;
    std::vector<uint32_t> restarts, at[6];          // end src / dst / offset, start src / dst / offset
    std::vector<uint32_t> coords[4];                // --msa: end row / column, start row / column
    std::vector<uint32_t> rows[2];                  // --rows: per start its supporting rows and the first of them
};
struct Seeds { std::vector<uint64_t> off, count; std::vector<uint32_t> q_start, length; };
struct Chains {
    std::vector<uint64_t> off;
    std::vector<uint32_t> score, anchor_place, anchor_seed;
    std::vector<uint32_t> chosen[2];                // --by-row: the chosen row and the rows that reach its score
    std::vector<uint32_t> rows[2];                  // --rows: supporting rows and the first of them
    std::vector<uint8_t> strand;                    // --strands, per pattern
    std::vector<uint32_t> best_score;
};
struct Pairs { std::vector<uint8_t> which; std::vector<uint32_t> out[3]; };    // the candidate, its score and columns per pair
struct Mates {                                      // --pair-align
    std::vector<uint32_t> read[5];                  // row, edits, t_start, t_end, insert
    std::vector<uint8_t> which;
    std::vector<uint32_t> out[3];                   // score, lo, hi
};
struct Mapq { std::vector<uint64_t> second_off; std::vector<uint32_t> second[3]; std::vector<uint8_t> quality; };
struct Runs { std::vector<uint64_t> off; std::vector<uint32_t> ops; };         // the CIGAR runs of every virtual read
struct RowAlign { std::vector<uint32_t> at[4]; Runs cigar; };                  // row, edits, t_start, t_end
struct GraphAlign {
    std::vector<uint32_t> at[5], path_nodes;        // edits, start node and offset, end node and offset
    std::vector<uint64_t> path_off;
    Runs cigar;
};
struct Results { Located located; Places places; Seeds seeds; Chains chains; Pairs pairs; Mates mates; Mapq mapq; RowAlign row; GraphAlign graph; };

// the library's contexts; released before printing starts
struct Engine {
    fbg_ctx *ctx = nullptr;
    fbg_pindex *ix = nullptr;
    ~Engine() { fbg_pindex_destroy(ix); fbg_ctx_destroy(ctx); }
};

// v as n + 1 zeros, so that data() is never null
template <class T> static T *sized(std::vector<T> &v, uint64_t n)
{
    v.assign(n + 1, 0);
    return v.data();
}

// ---- the stages: each sizes its arrays and makes its calls ------------------------------------------------------------------

typedef int Stage(fbg_pindex *ix, const LocateOptions &o, const Reads &r, Results &x);

static int stage_locate(fbg_pindex *ix, const LocateOptions &, const Reads &r, Results &x)
{
    return fbg_pindex_locate(ix, r.bytes(), r.off.data(), r.np, sized(x.located.count, r.np), sized(x.located.pos, r.np));
}

static int stage_occurrences(fbg_pindex *ix, const LocateOptions &o, const Reads &r, Results &x)
{
    Places &p = x.places;
    return fbg_pindex_occurrences(ix, r.bytes(), r.off.data(), r.np, o.max_places, sized(x.located.count, r.np), sized(x.located.pos, r.np),
                                  sized(p.restarts, r.np), sized(p.end_off, r.np), sized(p.start_off, r.np), sized(p.end_total, r.np),
                                  sized(p.start_total, r.np), nullptr);
}

static int stage_seeds(fbg_pindex *ix, const LocateOptions &o, const Reads &r, Results &x)
{
    const uint64_t max_places = o.occurrences ? o.max_places : 0;
    uint64_t *off = sized(x.seeds.off, r.nv);
    if (!o.strands) return fbg_pindex_seeds(ix, r.bytes(), r.off.data(), r.np, o.min_seed, max_places, off, nullptr);
    uint8_t table[256];
    for (int c = 0; c < 256; c++) table[c] = (uint8_t)c;
    for (size_t i = 0; i + 1 < o.complement.size(); i += 2) table[(uint8_t)o.complement[i]] = (uint8_t)o.complement[i + 1];
    return fbg_pindex_seeds_strands(ix, r.bytes(), r.off.data(), r.np, o.have_complement ? table : nullptr, o.min_seed, max_places, off,
                                    nullptr);
}

static int stage_seeds_fetch(fbg_pindex *ix, const LocateOptions &, const Reads &r, Results &x)
{
    Seeds &s = x.seeds;
    Places &p = x.places;
    const uint64_t ns = s.off[r.nv];
    return fbg_pindex_seeds_fetch(ix, sized(s.q_start, ns), sized(s.length, ns), sized(s.count, ns), sized(p.restarts, ns),
                                  sized(p.end_total, ns), sized(p.start_total, ns), sized(p.end_off, ns), sized(p.start_off, ns), nullptr);
}

// the places behind the offsets of the search that ran
static int stage_places(fbg_pindex *ix, const LocateOptions &o, const Reads &, Results &x)
{
    Places &p = x.places;
    uint32_t *a[6];
    for (int k = 0; k < 6; k++) a[k] = sized(p.at[k], k < 3 ? p.end_off.back() : p.start_off.back());
    return (o.seeds ? fbg_pindex_seeds_places : fbg_pindex_occurrences_fetch)(ix, a[0], a[1], a[2], a[3], a[4], a[5], nullptr);
}

// and their MSA cells
static int stage_coords(fbg_pindex *ix, const LocateOptions &o, const Reads &, Results &x)
{
    Places &p = x.places;
    uint32_t *a[4];
    for (int k = 0; k < 4; k++) a[k] = sized(p.coords[k], k < 2 ? p.end_off.back() : p.start_off.back());
    return (o.seeds ? fbg_pindex_seeds_msa : fbg_pindex_occurrences_msa)(ix, a[0], a[1], a[2], a[3], nullptr);
}

static int stage_chains(fbg_pindex *ix, const LocateOptions &o, const Reads &r, Results &x)
{
    Chains &c = x.chains;
    uint64_t *off = sized(c.off, r.nv);
    uint32_t *score = sized(c.score, r.nv);
    if (!o.by_row) return fbg_pindex_chains(ix, o.band, 0, off, score, nullptr);
    return fbg_pindex_chains_by_row(ix, o.band, 0, off, score, sized(c.chosen[0], r.nv), sized(c.chosen[1], r.nv), nullptr);
}

// adopts: the chains' offsets and scores become those of the pair-consistent chains
static int stage_pairs(fbg_pindex *ix, const LocateOptions &o, const Reads &r, Results &x)
{
    Pairs &p = x.pairs;
    const uint64_t pairs = r.np / 2;
    std::vector<uint64_t> rescue_off;
    return fbg_pindex_chains_pairs(ix, o.min_insert, o.max_insert, sized(p.which, pairs), sized(p.out[0], pairs), sized(p.out[1], pairs),
                                   sized(p.out[2], pairs), sized(rescue_off, r.nv), nullptr, nullptr, nullptr, nullptr, nullptr,
                                   x.chains.off.data(), x.chains.score.data(), nullptr, nullptr);
}

// on the adopted chains; writes nothing that a later stage reads
static int stage_pair_align(fbg_pindex *ix, const LocateOptions &o, const Reads &r, Results &x)
{
    Mates &m = x.mates;
    const uint64_t pairs = r.np / 2;
    return fbg_pindex_pairs_align(ix, o.min_insert, o.max_insert, (uint32_t)o.max_edits, 0, nullptr, sized(m.read[0], r.nv),
                                  sized(m.read[1], r.nv), sized(m.read[2], r.nv), sized(m.read[3], r.nv), sized(m.read[4], r.nv),
                                  sized(m.which, pairs), sized(m.out[0], pairs), sized(m.out[1], pairs), sized(m.out[2], pairs), nullptr,
                                  nullptr);
}

static int stage_chains_fetch(fbg_pindex *ix, const LocateOptions &, const Reads &r, Results &x)
{
    Chains &c = x.chains;
    return fbg_pindex_chains_fetch(ix, sized(c.anchor_place, c.off[r.nv]), sized(c.anchor_seed, c.off[r.nv]), nullptr);
}

static int stage_chain_strands(fbg_pindex *ix, const LocateOptions &, const Reads &r, Results &x)
{
    return fbg_pindex_chain_strands(ix, sized(x.chains.strand, r.np), sized(x.chains.best_score, r.np), nullptr, nullptr, nullptr, nullptr);
}

static int stage_mapq(fbg_pindex *ix, const LocateOptions &o, const Reads &r, Results &x)
{
    Mapq &q = x.mapq;
    const int rc = fbg_pindex_chains_mapq(ix, o.margin, sized(q.second_off, r.nv), sized(q.second[0], r.nv), sized(q.second[1], r.nv),
                                          sized(q.second[2], r.nv), sized(q.quality, r.nv), nullptr);
    return rc == FBG_OK && o.strands ? fbg_pindex_mapq_strands(ix, q.quality.data(), nullptr) : rc;
}

static int stage_seeds_rows(fbg_pindex *ix, const LocateOptions &, const Reads &, Results &x)
{
    Places &p = x.places;
    return fbg_pindex_seeds_rows(ix, sized(p.rows[0], p.start_off.back()), sized(p.rows[1], p.start_off.back()), nullptr);
}

static int stage_chains_rows(fbg_pindex *ix, const LocateOptions &, const Reads &r, Results &x)
{
    return fbg_pindex_chains_rows(ix, sized(x.chains.rows[0], r.nv), sized(x.chains.rows[1], r.nv), nullptr, nullptr);
}

static int stage_align(fbg_pindex *ix, const LocateOptions &o, const Reads &r, Results &x)
{
    std::vector<uint32_t> *a = x.row.at;
    return fbg_pindex_chains_align(ix, o.pad, 0, sized(a[0], r.nv), sized(a[1], r.nv), sized(a[2], r.nv), sized(a[3], r.nv), nullptr);
}

// the runs of an alignment stage (fbg_pindex_chains_cigar, fbg_pindex_chains_graph_cigar, and their _fetch)
static int fetch_runs(fbg_pindex *ix, uint64_t nv, Runs &runs, decltype(fbg_pindex_chains_cigar) *trace,
                      decltype(fbg_pindex_chains_cigar_fetch) *fetch)
{
    uint64_t total = 0;
    const int rc = trace(ix, nullptr, &total, nullptr);
    return rc == FBG_OK ? fetch(ix, sized(runs.off, nv), sized(runs.ops, total)) : rc;
}

static int stage_cigar(fbg_pindex *ix, const LocateOptions &, const Reads &r, Results &x)
{
    return fetch_runs(ix, r.nv, x.row.cigar, fbg_pindex_chains_cigar, fbg_pindex_chains_cigar_fetch);
}

static int stage_graph_align(fbg_pindex *ix, const LocateOptions &o, const Reads &r, Results &x)
{
    GraphAlign &g = x.graph;
    uint64_t total = 0;
    const int rc = fbg_pindex_chains_align_graph(ix, o.graph_pad, 0, nullptr, sized(g.at[0], r.nv), sized(g.at[1], r.nv), sized(g.at[2], r.nv),
                                                 sized(g.at[3], r.nv), sized(g.at[4], r.nv), nullptr, &total, nullptr);
    return rc == FBG_OK ? fbg_pindex_chains_align_graph_fetch(ix, sized(g.path_off, r.nv), sized(g.path_nodes, total)) : rc;
}

static int stage_graph_cigar(fbg_pindex *ix, const LocateOptions &, const Reads &r, Results &x)
{
    return fetch_runs(ix, r.nv, x.graph.cigar, fbg_pindex_chains_graph_cigar, fbg_pindex_chains_graph_cigar_fetch);
}

// The stages that the options ask for, in their order: a search, its places, then what the other options add to --seeds
// (each of them needs it).
static int run_stages(fbg_pindex *ix, const LocateOptions &o, const Reads &r, Results &x)
{
    const struct { bool wanted; Stage *run; } stages[] = {
        {!o.seeds && !o.occurrences, stage_locate},
        {!o.seeds && o.occurrences, stage_occurrences},
        {o.seeds, stage_seeds},
        {o.seeds, stage_seeds_fetch},
        {o.seeds || o.occurrences, stage_places},
        {o.have_msa && o.occurrences, stage_coords},
        {o.chain, stage_chains},
        {o.pairs, stage_pairs},
        {o.pair_align, stage_pair_align},
        {o.chain, stage_chains_fetch},
        {o.chain && o.strands, stage_chain_strands},
        {o.mapq, stage_mapq},
        {o.rows && o.occurrences, stage_seeds_rows},
        {o.rows && o.chain, stage_chains_rows},
        {o.align, stage_align},
        {o.cigar, stage_cigar},
        {o.graph_align, stage_graph_align},
        {o.graph_cigar, stage_graph_cigar},
    };
    for (const auto &s : stages) {
        const int rc = s.wanted ? s.run(ix, o, r, x) : FBG_OK;
        if (rc != FBG_OK) return rc;
    }
    return FBG_OK;
}

// ---- input ------------------------------------------------------------------------------------------------------------------

// the MSA of --msa and the inclusive block ends of the graph's segmentation, the last one n (fbg_minmax_dp's convention)
static bool read_msa_of_graph(const LocateOptions &o, Msa &msa, std::vector<uint64_t> &bounds, std::string &error)
{
    uint64_t gm = 0, gn = 0;
    std::vector<uint64_t> xs;
    if (!read_segmentation(o.graph, gm, gn, xs, error)) return false;
    if (!read_msa(o.msa_path, 1, true, false, msa)) { error = "cannot open " + o.msa_path; return false; }
    if (msa.m != gm || msa.n != gn) {
        error = o.msa_path + " does not fit " + o.graph + ": the MSA has " + std::to_string(msa.m) + " rows and " + std::to_string(msa.n) +
                " columns, the M line says " + std::to_string(gm) + " and " + std::to_string(gn);
        return false;
    }
    for (size_t i = 1; i < xs.size(); i++) {
        if (xs[i] < 2) { error = o.graph + ": malformed X line"; return false; }
        bounds.push_back(xs[i] - 2);
    }
    bounds.push_back(gn);
    return true;
}

static bool read_patterns(const LocateOptions &o, Reads &r, std::string &error)
{
    std::ifstream pf;
    if (o.have_patterns) {
        pf.open(o.patterns, std::ios::binary);
        if (!pf) { error = "cannot open " + o.patterns; return false; }
    }
    std::istream &in = o.have_patterns ? static_cast<std::istream &>(pf) : std::cin;
    std::ios_base::sync_with_stdio(false);
    while (true) {
        std::string p;
        in >> p;
        if (in.eof()) break;           // also drops a last token that ends the input (locate_patterns.cpp:47-53)
        if (!in) { error = "cannot read the patterns"; return false; }
        r.data += p;
        r.off.push_back(r.data.size());
    }
    r.np = r.off.size() - 1;
    r.nv = o.strands ? 2 * r.np : r.np;
    return true;
}

// The index of the graph or, with --msa, of the MSA's segmentation, which must be the graph that was read: `misfit` says
// where it is not.
static int build_index(Engine &e, const LocateOptions &o, const XgfaGraph &g, const Msa &msa, const std::vector<uint64_t> &bounds,
                       std::string &misfit)
{
    const uint64_t nodes = g.label_off.size() - 1;
    if (!o.have_msa)
        return fbg_pindex_build(e.ctx, (const uint8_t *)g.labels.data(), g.label_off.data(), nodes, g.edge_off.data(), g.edge_dst.data(), &e.ix);
    std::string why;
    if (bounds.size() > 1 && !std::is_sorted(bounds.begin(), bounds.end() - 1)) why = "the X line does not increase";
    int rc = fbg_msa_load_host(e.ctx, msa.cells.data(), msa.m, msa.n);
    if (rc == FBG_OK && why.empty())
        rc = o.rows ? fbg_pindex_build_segmentation_rows(e.ctx, bounds.data(), bounds.size(), &e.ix)
                    : fbg_pindex_build_segmentation(e.ctx, bounds.data(), bounds.size(), &e.ix);
    if (rc == FBG_OK && why.empty()) {
        std::vector<uint32_t> len(nodes + 1);
        if (fbg_pindex_node_count(e.ix) != nodes)
            why = "its segmentation has " + std::to_string(fbg_pindex_node_count(e.ix)) + " nodes, the graph " + std::to_string(nodes);
        else if ((rc = fbg_pindex_node_info(e.ix, len.data(), nullptr, nullptr)) == FBG_OK)
            for (uint64_t u = 0; u < nodes && why.empty(); u++)
                if (len[u] != g.label_off[u + 1] - g.label_off[u])
                    why = "node " + std::to_string(g.ids[u]) + " has " + std::to_string(g.label_off[u + 1] - g.label_off[u]) +
                          " symbols in the graph and " + std::to_string(len[u]) + " in the MSA";
    }
    if (!why.empty()) misfit = o.msa_path + " does not fit " + o.graph + ": " + why;
    return rc;
}

// ---- output -----------------------------------------------------------------------------------------------------------------

struct Printer {
    const LocateOptions &o;
    const XgfaGraph &g;
    const Reads &r;
    const Results &x;
    std::ostream &gaf;

    void places(uint64_t k, bool rows) const
    {
        const Places &p = x.places;
        const std::vector<uint64_t> *const off[2] = {&p.end_off, &p.start_off}, *const total[2] = {&p.end_total, &p.start_total};
        print_places(g, k, off, total, p.at, o.have_msa && o.occurrences ? p.coords : nullptr, rows ? p.rows : nullptr);
    }

    // the S / E / B lines of virtual read v
    void seeds(uint64_t v) const
    {
        const Seeds &s = x.seeds;
        for (uint64_t j = s.off[v]; j < s.off[v + 1]; j++) {
            std::cout << "S\t" << s.q_start[j] << '\t' << s.length[j] << '\t' << s.count[j] << '\t' << x.places.restarts[j] << '\n';
            if (o.occurrences) places(j, o.rows);
        }
    }

    // its C / A lines
    void chain(uint64_t v) const
    {
        const Chains &c = x.chains;
        std::cout << "C\t" << c.score[v] << '\t' << c.off[v + 1] - c.off[v];
        if (o.rows) print_row_set(c.rows[0][v], c.rows[1][v]);
        if (o.by_row) {
            if (c.chosen[0][v] == 0xffffffffu) std::cout << "\t*";
            else std::cout << '\t' << c.chosen[0][v];
            std::cout << '\t' << c.chosen[1][v];
        }
        std::cout << '\n';
        for (uint64_t i = c.off[v]; i < c.off[v + 1]; i++)
            std::cout << "A\t" << x.seeds.q_start[c.anchor_seed[i]] << '\t' << x.seeds.length[c.anchor_seed[i]] << '\t'
                      << x.places.coords[2][c.anchor_place[i]] << '\t' << x.places.coords[3][c.anchor_place[i]] << '\n';
    }

    // its Q line
    void mapq(uint64_t v) const
    {
        const Mapq &q = x.mapq;
        std::cout << "Q\t" << (unsigned)q.quality[v] << '\t' << q.second[0][v];
        if (q.second_off[v + 1] == q.second_off[v]) std::cout << "\t*\t*\n";
        else std::cout << '\t' << q.second[1][v] << '\t' << q.second[2][v] << '\n';
    }

    // its G line
    void row_alignment(uint64_t v) const
    {
        const RowAlign &a = x.row;
        if (a.at[1][v] == FBG_ALIGN_NONE) { std::cout << "G\t*\n"; return; }
        std::cout << "G\t" << a.at[0][v] << '\t' << a.at[1][v] << '\t' << a.at[2][v] << '\t' << a.at[3][v];
        if (o.cigar) {
            std::cout << '\t';
            print_runs(std::cout, a.cigar.ops, a.cigar.off[v], a.cigar.off[v + 1]);
        }
        std::cout << '\n';
    }

    // its H line with the path; false: H and *
    bool graph_alignment(uint64_t v) const
    {
        const GraphAlign &a = x.graph;
        if (a.at[0][v] == FBG_ALIGN_NONE) { std::cout << "H\t*\n"; return false; }
        std::cout << "H\t" << a.at[0][v] << '\t' << g.ids[a.at[1][v]] << '\t' << a.at[2][v] << '\t' << g.ids[a.at[3][v]] << '\t' << a.at[4][v]
                  << '\t';
        for (uint64_t i = a.path_off[v]; i < a.path_off[v + 1]; i++) std::cout << '>' << g.ids[a.path_nodes[i]];
        if (o.graph_cigar) {
            std::cout << '\t';
            print_runs(std::cout, a.cigar.ops, a.cigar.off[v], a.cigar.off[v + 1]);
        }
        std::cout << '\n';
        return true;
    }

    // the GAF record of that H line
    void gaf_record(uint64_t v) const
    {
        const GraphAlign &a = x.graph;
        const uint64_t k = v < r.np ? v : v - r.np, L = r.off[k + 1] - r.off[k];
        uint64_t plen = 0, match = 0, cols = 0;
        gaf << "read" << k << '\t' << L << "\t0\t" << L << '\t' << (v < r.np ? '+' : '-') << '\t';
        for (uint64_t i = a.path_off[v]; i < a.path_off[v + 1]; i++) {
            const uint32_t u = a.path_nodes[i];
            gaf << '>' << g.ids[u];
            plen += g.label_off[u + 1] - g.label_off[u];
        }
        for (uint64_t i = a.cigar.off[v]; i < a.cigar.off[v + 1]; i++) {
            cols += a.cigar.ops[i] >> 4;
            if ((a.cigar.ops[i] & 15) == FBG_CIGAR_EQ) match += a.cigar.ops[i] >> 4;
        }
        const uint32_t ve = a.at[3][v];
        gaf << '\t' << plen << '\t' << a.at[2][v] << '\t' << plen - (g.label_off[ve + 1] - g.label_off[ve]) + a.at[4][v] << '\t' << match
            << '\t' << cols << '\t' << (o.mapq ? (unsigned)x.mapq.quality[v] : 255u) << "\tNM:i:" << a.at[0][v] << "\tcg:Z:";
        print_runs(gaf, a.cigar.ops, a.cigar.off[v], a.cigar.off[v + 1]);
        gaf << '\n';
    }

    // its Y line
    void mate(uint64_t v) const
    {
        const Mates &m = x.mates;
        if (m.read[1][v] == FBG_ALIGN_NONE) { std::cout << "Y\t*\n"; return; }
        std::cout << "Y\t" << m.read[0][v] << '\t' << m.read[1][v] << '\t' << m.read[2][v] << '\t' << m.read[3][v] << '\t';
        if (m.read[4][v] == FBG_ALIGN_NONE) std::cout << "*\n";
        else std::cout << m.read[4][v] << '\n';
    }

    // every line of virtual read v
    void block(uint64_t v) const
    {
        seeds(v);
        if (!o.chain) return;
        chain(v);
        if (o.mapq) mapq(v);
        if (o.align) row_alignment(v);
        if (o.graph_align && graph_alignment(v) && o.have_gaf) gaf_record(v);
        if (o.pair_align) mate(v);
    }

    // the T line of pattern k
    void strand(uint64_t k) const
    {
        const uint8_t s = x.chains.strand[k];
        std::cout << "T\t" << (s == FBG_STRAND_NONE ? '*' : s ? '-' : '+') << '\t' << x.chains.best_score[k];
        if (o.mapq) std::cout << '\t' << (s == FBG_STRAND_NONE ? 0u : (unsigned)x.mapq.quality[s ? r.np + k : k]);
        std::cout << '\n';
    }

    // the Z / W lines of pair p
    void pair(uint64_t p) const
    {
        const Pairs &z = x.pairs;
        const Mates &w = x.mates;
        if (z.which[p] == 0xffu) std::cout << "Z\t*\n";
        else std::cout << "Z\t" << (unsigned)z.which[p] << '\t' << z.out[0][p] << '\t' << z.out[1][p] << '\t' << z.out[2][p] << '\n';
        if (o.pair_align && w.which[p] == 0xffu) std::cout << "W\t*\n";
        else if (o.pair_align)
            std::cout << "W\t" << (unsigned)w.which[p] << '\t' << w.out[0][p] << '\t' << w.out[1][p] << '\t' << w.out[2][p] << '\n';
    }

    // the answer of --seeds
    int seeded() const
    {
        const std::vector<uint64_t> &off = x.seeds.off;
        uint64_t found = 0;
        for (uint64_t k = 0; k < r.np; k++) {
            const uint64_t ns = off[k + 1] - off[k];
            const uint64_t nr = o.strands ? off[r.np + k + 1] - off[r.np + k] : 0;
            std::cout << "Pattern? " << ns << " seeds found.\n";
            if (ns + nr == 0 && o.error_on_not_found) {
                std::cerr << "Pattern has no seed.\n";
                std::cout.flush();
                return EXIT_FAILURE;
            }
            found += ns + nr != 0;
            block(k);
            if (!o.strands) continue;
            std::cout << "-\t" << nr << '\n';
            block(r.np + k);
            if (o.chain) strand(k);
            if (o.chain && o.pairs && k % 2) pair(k / 2);
        }
        std::cout << "Pattern? " << found << " out of " << r.np << " patterns seeded" << std::endl;
        return EXIT_SUCCESS;
    }

    // the answer without --seeds, locate_patterns' own
    int located() const
    {
        uint64_t found = 0;
        for (uint64_t k = 0; k < r.np; k++) {
            std::cout << "Pattern? " << x.located.count[k] << " occurrences found.\n";
            if (x.located.count[k] == 0) {
                std::cerr << "Pattern not found, pos = " << x.located.pos[k] << ".\n";
                if (o.error_on_not_found) { std::cout.flush(); return EXIT_FAILURE; }
            } else {
                found++;
                if (o.occurrences) places(k, false);
            }
        }
        std::cout << "Pattern? " << found << " out of " << r.np << " patterns found" << std::endl;
        return EXIT_SUCCESS;
    }
};

int main(int argc, char **argv)
{
    LocateOptions o;
    std::string error;
    if (!parse_locate_options(argc, argv, o, error)) return usage(error);
    if (o.help) { usage("pattern search in a founder graph"); return EXIT_SUCCESS; }

    std::ofstream gaf;
    if (o.have_gaf) {
        gaf.open(o.gaf_path, std::ios::binary | std::ios::trunc);
        if (!gaf) return fail("cannot write " + o.gaf_path);
    }
    XgfaGraph g;
    Msa msa;
    std::vector<uint64_t> bounds;
    Reads r;
    if (!read_xgfa_graph(o.graph, g, error) || (o.have_msa && !read_msa_of_graph(o, msa, bounds, error)) || !read_patterns(o, r, error))
        return fail(error);
    if (o.pairs && r.np % 2) return usage("--pairs takes an even number of patterns, mates interleaved");

    Results x;
    {
        Engine e;
        if (fbg_ctx_create(0, &e.ctx) != FBG_OK) return fail(fbg_last_error(nullptr));
        int rc = build_index(e, o, g, msa, bounds, error);
        if (!error.empty()) return fail(error);
        if (rc == FBG_OK) rc = run_stages(e.ix, o, r, x);
        if (rc != FBG_OK) return fail(fbg_last_error(e.ctx));
    }
    const Printer out{o, g, r, x, gaf};
    if (!o.seeds) return out.located();
    if (out.seeded() != EXIT_SUCCESS) return EXIT_FAILURE;
    if (o.have_gaf) {
        gaf.close();
        if (!gaf) return fail("cannot write " + o.gaf_path);
    }
    return EXIT_SUCCESS;
}
