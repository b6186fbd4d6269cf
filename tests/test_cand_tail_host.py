"""The logic of the rank-order scan's tail by member (csrc/cand_tail.h: where tie groups begin in a sorted candidate list and where
their keys are found, the places of a group's members, the two running minima of a same-column run) against brute force, on the
CPU: founderblockgraphs_amd/fbg_host_selftest cand-tail (g++, no GPU).

The program prints "cand_tail ok GROUPS HEADS RUNS": tie groups of 2 .. 70 members ranked, once with all members K symbols long
and once with members that have fewer than K symbols left; group heads found and measured through candidate regions of 7, 64, 100
and 4096 entries that cut the groups; runs of 1 .. 200 members in one piece and in pieces of 64, 7 and 1."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "founderblockgraphs_amd", "fbg_host_selftest")


def test_cand_tail_header_equals_brute_force():
    r = subprocess.run([EXE, "cand-tail"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    words = r.stdout.split()
    assert words[:2] == ["cand_tail", "ok"], r.stdout
    groups, heads, runs = (int(w) for w in words[2:5])
    assert groups == 2 * 69                    # sizes 2 .. 70, with and without short members
    assert heads >= 4 * 69                     # a group of every size 2 .. 70 under each of the four region sizes, small ones besides
    assert runs == 200 * 4                     # lengths 1 .. 200, four piece sizes
