"""The sample of keys drawn before the sort of a gap-free MSA (suffix_sort.hip): its twins -- 2^20 keys minus the distinct ones
among them -- counted by one kernel with an open-addressing table (option twin_hash, csrc/twin_hash.h) and by sorting the
sample.  Same count, same verdict, same f; the table's slot choice and probing against a numpy model on the CPU."""
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import fbg_options, random_msa
from oracle import pyoracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "founderblockgraphs_amd", "fbg_host_selftest")

M, N_COLS = 64, 65600            # the sample is drawn from 2^22 symbols on: 64 * 65601 + 1 = 4198465
S = 1 << 20

_refs = {}


def _case(name):
    """An input and the oracle's f, computed once."""
    if name not in _refs:
        rng = np.random.default_rng({"iid": 1, "star": 2, "planted_rows": 3}[name])
        if name == "star":                       # a star phylogeny: every row the ancestor with 1 % substitutions
            msa = random_msa(rng, M, N_COLS, similar=0.99)
        else:
            msa = random_msa(rng, M, N_COLS)
            if name == "planted_rows":           # eight identical rows among 64
                msa[8:16] = msa[8]
        _refs[name] = {"msa": msa, "f": O.compute_f(msa)}
    return _refs[name]


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["iid", "star", "planted_rows"])
def test_twins_by_table_and_by_sort(engine, name):
    """twin_hash = 1 and 0, each with the MSD sort (msd_min = 1: it waits on the stream before the count is read) and with
    rocPRIM's sort, as a text of this length takes by default (nothing waits between the sample and the place that reads the
    count): the same sample_twins, the same kind of index, the oracle's f.  iid rows have few twins (estimated tie fraction
    twins * N / S^2 far below the 0.5 that decides), the star phylogeny nearly only twins (above it: the group-level scan is
    taken at once), eight planted rows lie in between."""
    ref = _case(name)
    N = M * (N_COLS + 1) + 1
    seen = {}
    for msd_min in (-1, 1):
        for twin_hash in (1, 0):
            with fbg_options(engine, {"twin_hash": twin_hash, "msd_min": msd_min}):
                assert np.array_equal(engine.elastic_f(ref["msa"]), ref["f"]), (msd_min, twin_hash)
                seen[msd_min, twin_hash] = (engine.get_option("sample_twins"), engine.get_option("index_kind"),
                                            engine.get_option("rank_lean_launched"))
    est = seen[-1, 1][0] * N / (S * S)
    print(name, "(msd_min, twin_hash) -> (sample_twins, index_kind, rank_lean_launched):", seen, "estimated tie fraction", est)
    for msd_min in (-1, 1):
        assert seen[msd_min, 1] == seen[msd_min, 0], seen
    assert seen[-1, 1][0] == seen[1, 1][0] >= 0, seen
    if name == "iid":
        assert est < 0.05, est
    elif name == "star":
        assert est > 0.5 and seen[-1, 1][1] == 1, (est, seen)
        assert seen[1, 1][2] == 0, seen                  # the slot-level scan was not tried
    else:
        assert 0.05 < est < 0.5, est


def _twins(keys, bits):
    path = os.path.join(os.environ.get("TMPDIR", "/tmp"), "fbg_twin_keys_%d.bin" % os.getpid())
    np.asarray(keys, dtype=np.uint64).tofile(path)
    try:
        r = subprocess.run([EXE, "twin-hash", path, str(bits)], capture_output=True, text=True)
    finally:
        os.unlink(path)
    assert r.returncode == 0, r.stdout + r.stderr
    mt = re.fullmatch(r"twin_hash (\d+) (\d+)\n", r.stdout)
    assert mt, r.stdout
    return int(mt.group(1)), int(mt.group(2))


def _slots(keys, bits):
    path = os.path.join(os.environ.get("TMPDIR", "/tmp"), "fbg_twin_slots_%d.bin" % os.getpid())
    np.asarray(keys, dtype=np.uint64).tofile(path)
    try:
        r = subprocess.run([EXE, "twin-slots", path, str(bits)], capture_output=True, text=True)
    finally:
        os.unlink(path)
    assert r.returncode == 0, r.stdout + r.stderr
    return np.array(r.stdout.split(), dtype=np.uint64)


def test_twin_table_counts_keys_minus_distinct_keys():
    """16384 keys into a table of 32768 words, as the kernel inserts them (one after the other here): the count is the number
    of keys minus the number of distinct keys -- with all keys equal, all distinct, keys that are all-ones (they cannot be
    stored and are counted apart), and keys chosen to share their first slot, whose probe sequences run into each other."""
    n, bits = 16384, 15
    rng = np.random.default_rng(7)
    ones = np.uint64(0xffffffffffffffff)
    cases = {}
    cases["all_equal"] = np.full(n, 12345, dtype=np.uint64)
    cases["all_distinct"] = rng.permutation(np.arange(1, 1 << 20, dtype=np.uint64))[:n] << np.uint64(20)
    cases["few_symbols"] = rng.integers(0, 4096, n).astype(np.uint64)           # keys that differ in their low bits only
    k = rng.integers(0, 1 << 62, n).astype(np.uint64)
    k[::7] = ones
    cases["all_ones_some"] = k
    k = rng.integers(0, 3000, n).astype(np.uint64)
    k[5] = ones
    cases["all_ones_once"] = k
    cases["all_ones_only"] = np.full(n, ones, dtype=np.uint64)
    # colliding keys: of 2^20 random keys those that share the most frequent first slot and the slots right behind it, each
    # twice, filled up with random keys
    pool = rng.integers(0, 1 << 63, 1 << 20).astype(np.uint64)
    slots = _slots(pool, bits)
    top = np.bincount(slots.astype(np.int64)).argmax()
    near = pool[(slots >= top) & (slots < top + 4)]
    assert np.sum(slots == top) >= 40, np.sum(slots == top)
    k = np.concatenate([near, near, pool[:n - 2 * len(near)]])
    cases["collide"] = rng.permutation(k)
    for name, keys in cases.items():
        assert len(keys) == n, name
        got, longest = _twins(keys, bits)
        want = n - len(np.unique(keys))
        print(name, "twins", got, "want", want, "longest probe sequence", longest)
        assert got == want, name
        assert longest <= (1 << bits), name
    assert _twins(cases["collide"], bits)[1] >= 40           # the probes did run along the cluster


def test_spare_bits_in_the_test_are_the_header_s():
    src = open(os.path.join(ROOT, "founderblockgraphs_amd", "csrc", "twin_hash.h")).read()
    assert int(re.search(r"#define FBG_TWIN_SPARE (\d+)", src).group(1)) == 1       # 16384 keys, 2^15 words above
