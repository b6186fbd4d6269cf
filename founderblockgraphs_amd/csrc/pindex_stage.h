// pindex_stage.h -- which results of the pattern index are current (plain C++, no HIP: pindex.h includes it, and so does
// host/host_selftest.cpp for the CPU test of the table).
//
// A stage is the result that one producing call leaves in the index, made from the result of its parent stage.  done[s]
// says that the result of s is current.  A producing call begins its stage at its top, which makes the stage and
// everything made from it stale, and finishes it where it has succeeded; a call that reads a stage needs it, that is, the
// stage and every stage it was made from.  Where a current result lies (on_device) and the tables an index builds once
// (has_pref, has_tab) are no business of this table.
#pragma once

enum PsStage { PS_OCC, PS_SEEDS, PS_CHAINS, PS_BYROW, PS_ALIGN, PS_CIGAR, PS_GRAPH, PS_GCIGAR, PS_MAPQ, PS_COUNT };
#define PS_ROOT (-1)

// name: for the selftest; parent: a stage before its own entry, or PS_ROOT; call: the call that produces the stage
static const struct { const char *name; int parent; const char *call; } ps_table[PS_COUNT] = {
    {"OCC", PS_ROOT, "fbg_pindex_occurrences"},
    {"SEEDS", PS_ROOT, "fbg_pindex_seeds"},
    {"CHAINS", PS_SEEDS, "fbg_pindex_chains"},
    {"BYROW", PS_CHAINS, "fbg_pindex_chains_by_row"},
    {"ALIGN", PS_CHAINS, "fbg_pindex_chains_align"},
    {"CIGAR", PS_ALIGN, "fbg_pindex_chains_cigar"},
    {"GRAPH", PS_CHAINS, "fbg_pindex_chains_align_graph"},
    {"GCIGAR", PS_GRAPH, "fbg_pindex_chains_graph_cigar"},
    {"MAPQ", PS_CHAINS, "fbg_pindex_chains_mapq"},
};

// x and every stage below it are no longer done (a parent comes before its children, so one pass finds them all)
static inline void ps_begin(bool (&done)[PS_COUNT], PsStage x)
{
    bool gone[PS_COUNT] = {};
    for (int s = x; s < PS_COUNT; s++) {
        const int p = ps_table[s].parent;
        gone[s] = s == x || (p != PS_ROOT && gone[p]);
        if (gone[s]) done[s] = false;
    }
}

static inline void ps_finish(bool (&done)[PS_COUNT], PsStage x) { done[x] = true; }

// The first stage on the path from the root to y that is not done, or PS_COUNT where y and all its ancestors are
static inline int ps_missing(const bool (&done)[PS_COUNT], PsStage y)
{
    int miss = PS_COUNT;
    for (int s = y; s != PS_ROOT; s = ps_table[s].parent)
        if (!done[s]) miss = s;
    return miss;
}
