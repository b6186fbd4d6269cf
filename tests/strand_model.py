"""Both strands (include/fbg_hip.h, fbg_pindex_seeds_strands / fbg_pindex_chain_strands), restated in a few lines.

A table is 256 bytes; rc(P)[i] = table[P[L - 1 - i]]; the n given reads make 2n virtual reads, the given ones and then
their reverse complements; the strand of a read comes from the two chain scores and from whether the chains are empty."""

NONE = 0xff


def default_table():
    """A <-> T, C <-> G, a <-> t, c <-> g, every other byte itself."""
    t = bytearray(range(256))
    for a, b in ("AT", "CG", "at", "cg"):
        t[ord(a)], t[ord(b)] = ord(b), ord(a)
    return bytes(t)


def revcomp(read, table):
    """The table applied once to every symbol of the read taken back to front."""
    return bytes(table[c] for c in reversed(bytes(read)))


def virtual_reads(reads, table):
    reads = [bytes(r) for r in reads]
    return reads + [revcomp(r, table) for r in reads]


def pick(score0, score1, nonempty0, nonempty1):
    """-> (strand, score): the reverse strand only if it scores higher; NONE if the chain of that strand is empty."""
    t = 1 if score1 > score0 else 0
    return (t if (nonempty1 if t else nonempty0) else NONE), max(score0, score1)
