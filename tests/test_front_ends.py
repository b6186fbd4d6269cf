"""The two front ends of the pattern index as their callers see them, on the CPU: the signatures and argument rules of
PatternIndex.occurrences / .seeds / .chains (founderblockgraphs_amd/pindex.py), what the package exports, a fresh Chains,
and the command line of fbg_locate (csrc/host/locate_options.cpp) through founderblockgraphs_amd/fbg_host_selftest
locate-options.  Every expected name, default and message below is written out from the code as it stood before the front
ends were split into stages: a restructuring must leave them all as they are."""
import inspect
import os
import re
import subprocess

import pytest

import founderblockgraphs_amd
from founderblockgraphs_amd import api
from founderblockgraphs_amd.api import Chains, PatternIndex

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "founderblockgraphs_amd", "fbg_host_selftest")

SIGNATURES = {
    "occurrences": [("patterns", inspect.Parameter.empty), ("max_per_pattern", 64), ("msa", False)],
    "seeds": [("patterns", inspect.Parameter.empty), ("min_length", 1), ("max_per_seed", 0), ("msa", False), ("chain", False),
              ("band", None), ("min_score", 0), ("strands", False), ("complement", None), ("rows", False), ("by_row", False),
              ("mapq", False), ("mapq_margin", 0)],
    "chains": [("band", None), ("min_score", 0), ("rows", False), ("align", False), ("pad", 16), ("max_window", 0), ("cigar", False),
               ("by_row", False), ("graph", False), ("graph_pad", 16), ("max_cells", 0), ("select", None), ("graph_cigar", False),
               ("mapq", False), ("mapq_margin", 0), ("pairs", None), ("adopt_pairs", False), ("pair_align", False),
               ("pair_max_edits", 0xffffffff), ("pair_max_window", 0), ("pair_select", None)],
}


@pytest.mark.parametrize("name", sorted(SIGNATURES))
def test_signatures_and_defaults_stay(name):
    params = list(inspect.signature(getattr(PatternIndex, name)).parameters.values())
    assert params[0].name == "self"
    assert all(p.kind is inspect.Parameter.POSITIONAL_OR_KEYWORD for p in params)
    got = [(p.name, p.default) for p in params[1:]]
    assert got == SIGNATURES[name]
    assert all(type(g[1]) is type(w[1]) for g, w in zip(got, SIGNATURES[name]))      # False is not 0


# what founderblockgraphs_amd/__init__.py imports from .api
EXPORTED = ("Engine", "FbgError", "Group", "NoSegmentation", "Occurrences", "PatternIndex", "Seeds", "SegmentationCheck", "Validation",
            "as_msa", "complement_table", "graph_from_segmentation", "read_xgfa", "segment", "segment2elasticValid",
            "segment_elastic_heuristic", "segment_elastic_minmaxlength")


def test_every_exported_name_comes_from_api():
    for name in EXPORTED + ("Chains", "device_view"):
        assert hasattr(api, name), name
    for name in EXPORTED:
        assert getattr(founderblockgraphs_amd, name) is getattr(api, name), name
    from founderblockgraphs_amd import pindex
    for name in ("PatternIndex", "Occurrences", "Seeds", "Chains", "Validation", "complement_table", "_concat"):
        assert getattr(api, name) is getattr(pindex, name), name
    src = open(pindex.__file__).read()
    assert not re.search(r"^\s*(from\s+\.api|from\s+\.\s+import\s+.*\bapi\b|import\s+.*\bapi\b)", src, re.M)      # pindex stands below api


# the fields of Chains that a keyword of chains() asks for, by the paragraph of its docstring that describes them
OPTIONAL = ("strand best_score strand_counts chain_row n_best_rows n_rows first_row row_bits align_row edits t_start t_end best_edits "
            "align_ms cigar_off cigar_ops cigar_ms graph_edits graph_start graph_end graph_path_off graph_path_nodes best_graph_edits "
            "graph_ms graph_cigar_off graph_cigar_ops graph_cigar_ms second_score second_lo second_hi mapq second_off second_place "
            "second_seed mapq_stranded best_mapq mapq_ms pair_which pair_score pair_lo pair_hi rescue_score rescue_lo rescue_hi "
            "rescue_off rescue_place rescue_seed pair_stats pairs_ms mate_row mate_edits mate_start mate_end mate_insert mate_which "
            "mate_score mate_lo mate_hi mate_stats mate_ms").split()


def test_a_fresh_chains_has_no_optional_field():
    c = Chains("off", "score", "place", "seed", 1.5, 0.25)
    assert (c.chain_off, c.score, c.anchor_place, c.anchor_seed, c.device_ms, c.fetch_ms) == ("off", "score", "place", "seed", 1.5, 0.25)
    for f in OPTIONAL:
        assert getattr(c, f) is None, f
    assert c.by_row is False
    # the list above is the docstring's: every field it describes (six spaces, the names, two spaces or more, the text)
    described = []
    for line in Chains.__doc__.splitlines():
        m = re.match(r"      ([a-z_]+(?:, [a-z_]+)*)\s{2,}\S", line)
        if m:
            described += m.group(1).split(", ")
    assert sorted(described) == sorted(OPTIONAL + ["chain_off", "score", "anchor_place", "anchor_seed"])


def blank(**state):
    """A PatternIndex that no library call has made: an argument rule must answer before anything of it is used."""
    p = object.__new__(PatternIndex)
    for k, v in state.items():
        setattr(p, k, v)
    return p


PAIRED = dict(_seed_given=2)                         # as after seeds(strands=True)
PAIRED_ROWS = dict(_seed_given=2, _has_rows=True)    # on an index built with rows=True
PAIRS_NEEDS = "pairs=(min_insert, max_insert) with 0 <= min_insert <= max_insert"
EDITS_NEEDS = "pair_max_edits must fit 32 bits and pair_max_window must be 0 or more"
CHAINS_RULES = [
    ({}, dict(adopt_pairs=True), "adopt_pairs=True needs pairs=(min_insert, max_insert)"),
    ({}, dict(pairs=(0, 9)), "pairs= needs seeds(strands=True)"),
    (PAIRED, dict(pairs=(5, 3)), PAIRS_NEEDS),
    (PAIRED, dict(pairs=(-1, 3)), PAIRS_NEEDS),
    ({}, dict(pair_align=True), "pair_align=True needs pairs=(min_insert, max_insert)"),
    (PAIRED, dict(pairs=(0, 9), pair_align=True), "pair_align=True needs an index built with rows=True"),
    (PAIRED_ROWS, dict(pairs=(0, 9), pair_align=True, pair_max_edits=1 << 32), EDITS_NEEDS),
    (PAIRED_ROWS, dict(pairs=(0, 9), pair_align=True, pair_max_edits=-1), EDITS_NEEDS),
    (PAIRED_ROWS, dict(pairs=(0, 9), pair_align=True, pair_max_window=-1), EDITS_NEEDS),
    ({}, dict(mapq_margin=-1), "mapq_margin must be 0 or more"),
    ({}, dict(cigar=True), "cigar=True needs align=True"),
    ({}, dict(graph_cigar=True), "graph_cigar=True needs graph=True"),
    ({}, dict(band=-1), "band must be 0 or more, or None"),
    ({}, dict(min_score=-1), "min_score must be 0 or more"),
    ({}, dict(pad=-1), "pad and max_window must be 0 or more"),
    ({}, dict(max_window=-1), "pad and max_window must be 0 or more"),
    ({}, dict(graph_pad=-1), "graph_pad and max_cells must be 0 or more"),
    ({}, dict(max_cells=-1), "graph_pad and max_cells must be 0 or more"),
    # two rules broken: the earlier one answers
    ({}, dict(adopt_pairs=True, cigar=True), "adopt_pairs=True needs pairs=(min_insert, max_insert)"),
    ({}, dict(graph_cigar=True, cigar=True, max_cells=-1), "cigar=True needs align=True"),
    (PAIRED, dict(pairs=(0, 9), pair_align=True, mapq_margin=-1), "pair_align=True needs an index built with rows=True"),
]
SEEDS_RULES = [
    (dict(mapq=True), "mapq=True needs chain=True"),
    (dict(min_length=0), "min_length must be 1 or more"),
    (dict(max_per_seed=-1), "max_per_seed must be 0 or more"),
    (dict(complement={"A": "T"}), "complement needs strands=True"),
    (dict(mapq=True, min_length=0), "mapq=True needs chain=True"),
]


@pytest.mark.parametrize("case", range(len(CHAINS_RULES)))
def test_chains_argument_rules_answer_before_any_call(case):
    state, kwargs, message = CHAINS_RULES[case]
    with pytest.raises(ValueError) as e:
        PatternIndex.chains(blank(**state), **kwargs)
    assert str(e.value) == message


@pytest.mark.parametrize("case", range(len(SEEDS_RULES)))
def test_seeds_argument_rules_answer_before_any_call(case):
    kwargs, message = SEEDS_RULES[case]
    with pytest.raises(ValueError) as e:
        PatternIndex.seeds(blank(), ["ACGT"], **kwargs)
    assert str(e.value) == message


def test_occurrences_argument_rule_answers_before_any_call():
    with pytest.raises(ValueError) as e:
        PatternIndex.occurrences(blank(), ["ACGT"], max_per_pattern=-1)
    assert str(e.value) == "max_per_pattern must be 0 or more"


def test_pairs_takes_two_numbers():
    for bad in ((1,), (1, 2, 3)):
        with pytest.raises(ValueError):
            PatternIndex.chains(blank(**PAIRED), pairs=bad)


def test_tool_command_line():
    assert os.path.exists(EXE), "fbg_host_selftest is built by make -C founderblockgraphs_amd/csrc"
    r = subprocess.run([EXE, "locate-options"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and re.fullmatch(r"locate_options ok [1-9][0-9]+\n", r.stdout), r.stdout + r.stderr


def test_pointer_and_clamp_helpers_live_in_one_place():
    here = os.path.join(ROOT, "founderblockgraphs_amd")
    for name in ("api.py", "pindex.py"):
        src = open(os.path.join(here, name)).read()
        assert "data_as(" not in src and not re.search(r"min\(.*, 0xf{16}\)", src), name
        assert not re.search(r'getattr\(self, "_\w+", ', src), name
