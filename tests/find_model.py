"""Helpers of the search tests: the expected hits of a pattern in the oracle's decoded bytes, by
bytes.find, and the patterns every file is searched for.  Nothing here runs the code under test."""
import re

import inputs

LENGTHS = [1, 2, 3, 4, 5, 15, 16, 17, 31, 32, 33, 64, 255, 256]
TILE = 4096   # start positions per workgroup of the scan
LINE = re.compile(r"^find: offset (\d+)$", re.M)
TOTALS = re.compile(r"^find: (\d+) hits, decoded bytes = (\d+)$", re.M)


def text(seed, n):
    return inputs.generate("text", seed, n)


def rand(seed, n):
    return inputs.generate("rand", seed, n)


def mixed_data() -> bytes:
    """at block 4096 the three random blocks decode to no bytes: sizes [4096, 4096, 0, 0, 0, 4096, 4096, 1808]"""
    return text(7, 8192) + rand(3, 12288) + text(9, 10000)


def hits(plain: bytes, pattern: bytes):
    """every offset p with plain[p:p + m] == pattern, overlapping ones too, ascending"""
    out, i = [], plain.find(pattern)
    while i >= 0:
        out.append(i)
        i = plain.find(pattern, i + 1)
    return out


def absent(plain: bytes, m: int = 6) -> bytes:
    """m bytes that do not occur in plain (checked)"""
    for seed in range(1, 50):
        p = rand(1000 + seed, m)
        if plain.find(p) < 0:
            return p
    raise AssertionError("no absent pattern found")


def starts(total: int, m: int, seams):
    """where the patterns of length m are cut from a run of `total` bytes: its two ends, around every record
    seam, around the tile seam, and one start at which the address's low four bits are all set"""
    S = {0, total - m, TILE - 1, TILE, 15 + 16 * 3}
    for s in seams:
        S |= {s - 1, s - m + 1, s - m // 2}
    return sorted(p for p in S if 0 <= p and p + m <= total)


def patterns(plain: bytes, seams, lengths=LENGTHS):
    """the distinct patterns cut from plain: every length at every start of starts()"""
    seen = []
    for m in lengths:
        for p in starts(len(plain), m, seams):
            pat = plain[p:p + m]
            if pat not in seen:
                seen.append(pat)
    return seen
