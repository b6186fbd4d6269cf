"""The size of a tie group by galloping (csrc/tie_extent.h, shared with rank_tail.hip's k_tie_groups and k_cand_region) against the plain count,
on the CPU: founderblockgraphs_amd/fbg_host_selftest tie-extent (g++, no GPU)."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "founderblockgraphs_amd", "fbg_host_selftest")


def test_tie_extent_equals_linear_count():
    """Groups of 1 .. 70 and 8191 .. 8194 slots (the cap is 8192: the answer stops at 8193) at the start of a sorted array, in
    its middle and ending exactly at `hi`, each also with `hi` inside the group: the same number as counting slot by slot,
    no read beyond `hi`, and a few dozen reads at the most."""
    r = subprocess.run([EXE, "tie-extent"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    mt = re.fullmatch(r"tie_extent ok (\d+)\n", r.stdout)
    assert mt, r.stdout
    assert int(mt.group(1)) >= 74 * 3                    # every size at every position


def test_probe_length_in_the_gpu_test_is_the_header_s():
    src = open(os.path.join(ROOT, "founderblockgraphs_amd", "csrc", "tie_extent.h")).read()
    probe = int(re.search(r"#define FBG_TIE_PROBE (\d+)", src).group(1))
    test = open(os.path.join(ROOT, "tests", "test_critical_path.py")).read()
    assert int(re.search(r"^TIE_PROBE = (\d+)", test, re.M).group(1)) == probe
