"""What a sort key is (csrc/keys.h: the builders the pack kernel and the MSD sorts share, the one-symbol rule of the samples, the
LCP of two keys) against the plain definition, on the CPU: founderblockgraphs_amd/fbg_host_selftest keys (g++, no GPU).

The definition: the b-bit codes of a position's first K symbols, most significant first; in the compact coding a separator and
everything behind it count as 0.  The program prints "keys ok GEOMETRIES TILES PAIRS": msd_build_keys, the pack kernel's two
steps (rolling, then symbol by symbol once a separator was seen), the 2-bit gather and the one-symbol rule over tiles with one
separator at every offset from the first symbol to beyond the last one any builder reads, with two separators and with none;
the rolling builder alone in the plain coding, where codes go up to 255; at b = 1 with K = 64 (all 64 bits), b = 2 with K = 1, 16,
25 (the last the gather takes) and 26 (the first it does not), b = 3, 5, 7 with K = 1 and 64 // b.  The LCP of two keys against a
comparison symbol by symbol, for b = 1 .. 8 with K = 1 and 64 // b, on pairs that part at every symbol."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "founderblockgraphs_amd", "fbg_host_selftest")


def test_keys_header_equals_the_definition():
    r = subprocess.run([EXE, "keys"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    words = r.stdout.split()
    assert words[:2] == ["keys", "ok"], r.stdout
    geometries, tiles, pairs = (int(w) for w in words[2:5])
    assert geometries == 11 + 13               # compact: the eleven geometries above; plain: those and b = 8 with K = 1 and 8
    # compact: a separator at each of max(K + 7, 40) + 1 offsets, a tile with two, a tile with none; plain: two tiles
    compact = [(1, 64), (2, 1), (2, 16), (2, 25), (2, 26), (3, 1), (3, 21), (5, 1), (5, 12), (7, 1), (7, 9)]
    assert tiles == sum(max(K + 7, 40) + 3 for _, K in compact) + 2 * 13
    assert pairs == sum(1 + 64 // b for b in range(1, 9))      # every symbol index of K = 1 and of K = 64 // b
