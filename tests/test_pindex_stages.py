"""The table of the pattern index's stages (csrc/pindex_stage.h): which results a producing call makes stale, and when a
call finds what it needs, on the CPU: founderblockgraphs_amd/fbg_host_selftest pindex-stages (g++, no GPU).

The program prints the stage names, then per stage X the stages still done after "everything done, begin X", then per
subset of done stages (bit i of the mask: stage i) what every stage's need answers: "-" or the stage it names as missing."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "founderblockgraphs_amd", "fbg_host_selftest")

# the table, restated: a stage's result is made from its parent's
PARENT = dict(OCC=None, SEEDS=None, CHAINS="SEEDS", BYROW="CHAINS", ALIGN="CHAINS", CIGAR="ALIGN", GRAPH="CHAINS", GCIGAR="GRAPH",
              MAPQ="CHAINS")


def path(stage):
    """The stage and its ancestors, the root first."""
    return (path(PARENT[stage]) if PARENT[stage] else []) + [stage]


def test_begin_clears_a_stage_and_its_descendants_and_need_wants_every_ancestor():
    r = subprocess.run([EXE, "pindex-stages"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = [ln.split() for ln in r.stdout.splitlines()]
    assert lines[0][0] == "stages" and sorted(lines[0][1:]) == sorted(PARENT)
    names = lines[0][1:]
    begins = [ln for ln in lines if ln[0] == "begin"]
    assert [ln[1] for ln in begins] == names
    for ln in begins:
        assert ln[2:] == [s for s in names if ln[1] not in path(s)], ln          # exactly X and its descendants are gone
    needs = [ln for ln in lines if ln[0] == "need"]
    assert [int(ln[1]) for ln in needs] == list(range(1 << len(names)))
    for ln in needs:
        done = {s for i, s in enumerate(names) if int(ln[1]) >> i & 1}
        want = [next((a for a in path(s) if a not in done), "-") for s in names]  # the first missing call from the root on
        assert ln[2:] == want, ln
    assert len(lines) == 1 + len(begins) + len(needs)
