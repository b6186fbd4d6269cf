"""The ladder of sweeps of fbg_dp_minmax as a plan (csrc/dp_plan.h), on the CPU: founderblockgraphs_amd/fbg_host_selftest
dp_plan (g++, no GPU) reads "max_ext f0 n dp_literal dp_wave dp_safe_window dp_tile" per line and prints the rungs.

The rule below is stated from DESIGN.md 6, not from the header.  With bound = 2 max_ext + 2 and
R = 1 / 2 / 4 for bound <= 64 / 128 / 254, 8 / 16 for bound <= 512 / 1024 where f0 == 0, else 0 -- and 0 under dp_literal or when
f0 >= n -- the rungs are, in this order and each by a condition of its own:
  BYTES(Rt)  iff R != 0 and (not dp_wave or f0 != 0); Rt from the smallest of 1, 2, 4 with 64 Rt >= max_ext + 2 (4 beyond that),
             from R under dp_safe_window, doubling while Rt <= 4 and Rt <= R; dp_tile and f0 == 0 give Rt = 1 its tiled form
  WIDE(WS)   iff f0 < n, not dp_literal, not dp_wave, 256 < max_ext + 2 <= 16384, n >= 256; WS from the smallest of 1024 .. 16384
             that is >= max_ext + 2, up to 16384
  WAVE(R)    iff R != 0 and f0 == 0 and (R > 4 or dp_wave)
  LITERAL    always
dp_kind of a rung: 1, 3 + log2(WS / 1024), 2, 0."""
import os
import subprocess

from test_dp_edges import DP_LADDER

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "founderblockgraphs_amd", "fbg_host_selftest")
OPTIONS = ("dp_literal", "dp_wave", "dp_safe_window", "dp_tile")


def rule(max_ext, f0, n, dp_literal=0, dp_wave=0, dp_safe_window=0, dp_tile=0):
    bound = 2 * max_ext + 2
    R = 1 if bound <= 64 else 2 if bound <= 128 else 4 if bound <= 254 else 8 if f0 == 0 and bound <= 512 else \
        16 if f0 == 0 and bound <= 1024 else 0
    if dp_literal or f0 >= n:
        R = 0
    rungs = []
    if R != 0 and (not dp_wave or f0 != 0):
        rt = R if dp_safe_window else next((r for r in (1, 2, 4) if 64 * r >= max_ext + 2), 4)
        while rt <= 4 and rt <= R:
            rungs.append(("T1" if rt == 1 and dp_tile and f0 == 0 else f"B{rt}", 1))
            rt *= 2
    if f0 < n and not dp_literal and not dp_wave and 256 < max_ext + 2 <= 16384 and n >= 256:
        ws = next(w for w in (1024, 2048, 4096, 8192, 16384) if w >= max_ext + 2)
        while ws <= 16384:
            rungs.append((f"W{ws}", 3 + (ws // 1024).bit_length() - 1))
            ws *= 2
    if R != 0 and f0 == 0 and (R > 4 or dp_wave):
        rungs.append((f"V{R}", 2))
    rungs.append(("L", 0))
    return rungs


def plans(cases):
    text = "".join(f"{m} {f0} {n} {' '.join(str(opts.get(o, 0)) for o in OPTIONS)}\n" for m, f0, n, opts in cases)
    r = subprocess.run([EXE, "dp_plan"], input=text, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.splitlines()
    assert len(lines) == len(cases)
    return [[(w.split(":")[0], int(w.split(":")[1])) for w in line.split()] for line in lines]


def ladder_edges():
    """every max_ext on either side of every limit of DP_LADDER"""
    out = set()
    for lo, hi, _, _ in DP_LADDER:
        out |= {max(lo - 1, 0), lo, hi, hi + 1}
    return out


def test_plan_equals_the_rule():
    exts = sorted(ladder_edges() | {30, 31, 62, 63, 126, 127, 254, 255, 511, 512})
    cases = [(m, f0, n, opts) for m in exts for n in (255, 256, 4000) for f0 in (0, 1, n)
             for opts in [{}] + [{o: 1} for o in OPTIONS]]
    got = plans(cases)
    for case, g in zip(cases, got):
        m, f0, n, opts = case
        assert g == rule(m, f0, n, **opts), case
    seen = {name for g in got for name, _ in g}
    assert {"B1", "B2", "B4", "T1", "V1", "V2", "V4", "V8", "V16", "L"} | {f"W{1024 << k}" for k in range(5)} <= seen


def test_first_rung_is_the_ladder_table():
    """f0 = 0, default options, n as large as test_dp_edges' inputs: the first rung's dp_kind and limit are DP_LADDER's at both
    ends of every row (a byte rung's limit is 64 Rt, 255 for Rt = 4; a wide rung's its WS; the literal sweep has none)"""
    ends = [(m, row) for row in DP_LADDER for m in (row[0], row[1])]
    got = plans([(m, 0, max(3000, m + 2000), {}) for m, _ in ends])
    for (m, (_, _, kind, limit)), g in zip(ends, got):
        name, k = g[0]
        lim = None if name == "L" else int(name[1:]) if name[0] == "W" else 255 if name == "B4" else 64 * int(name[1:])
        assert (k, lim) == (kind, limit), (m, g)


def test_safe_window_beyond_the_byte_matrices_has_no_byte_rung():
    """the quirk dp_plan.h keeps: the byte rungs end at Rt = 4, so dp_safe_window with R = 8 or 16 starts above them"""
    got = plans([(m, 0, 4000, {"dp_safe_window": 1}) for m in (126, 127, 255, 256, 511)])
    assert [[name for name, _ in g] for g in got] == [
        ["B4", "L"], ["V8", "L"], ["W1024", "W2048", "W4096", "W8192", "W16384", "V8", "L"],
        ["W1024", "W2048", "W4096", "W8192", "W16384", "V16", "L"], ["W1024", "W2048", "W4096", "W8192", "W16384", "V16", "L"]]
