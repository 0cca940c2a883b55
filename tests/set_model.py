"""Helpers of the pattern-set tests: what the definitions of include/fcx.h say about the oracle's decoded bytes.
Hits are the sorted union of find_model.hits over the folded bytes, the selected lines come from
lines_model.starts, the filter's counters from the two tables' definition.  Nothing here runs the code under test."""
import bisect
import re

import find_model as fm
import grep_model as gm
import lines_model as lm

FOLD = bytes(b + 0x20 if 0x41 <= b <= 0x5A else b for b in range(256))
FOLD_BYTES = [0x40, 0x41, 0x5A, 0x5B, 0x60, 0x61, 0x7A, 0x7B, 0xC1, 0xE1]   # only 0x41 and 0x5A of these fold
FIND_TOTALS = re.compile(r"^find: (\d+) hits, decoded bytes = (\d+), patterns: (\d+)$", re.M)
GREP_TOTALS = re.compile(r"^grep: (\d+) lines, (\d+) bytes, (\d+) hits, decoded bytes = (\d+), patterns: (\d+)$", re.M)


def fold(data: bytes, on: bool) -> bytes:
    return data.translate(FOLD) if on else data


def counts(plain: bytes, patterns, on: bool = False):
    """per pattern the number of positions at which it occurs (overlapping ones too)"""
    text = fold(plain, on)
    return [len(fm.hits(text, fold(p, on))) for p in patterns]


def hits_any(plain: bytes, patterns, on: bool = False):
    """the positions at which at least one pattern occurs, ascending, each once"""
    text = fold(plain, on)
    out = set()
    for p in patterns:
        out.update(fm.hits(text, fold(p, on)))
    return sorted(out)


def judged(plain: bytes, patterns) -> int:
    return max(len(plain) - min(len(p) for p in patterns) + 1, 0)


def selected_any(plain: bytes, patterns, d: int, on: bool = False):
    """[(start, end)] of the lines that hold at least one hit, ascending, each once"""
    for p in patterns:
        assert bytes([d]) not in p and (not on or fold(bytes([d]), True) not in fold(p, True))
    s, T, out = lm.starts(plain, d), len(plain), []
    for p in hits_any(plain, patterns, on):
        j = bisect.bisect_right(s, p) - 1
        if not out or out[-1][0] != s[j]:
            out.append((s[j], s[j + 1] if j + 1 < len(s) else T))
    return out


def grep_stats(plain: bytes, patterns, d: int, on: bool = False, sel=None):
    """FCX_GREP_STATS of a set: lines, bytes, hits, judged, decoded"""
    sel = selected_any(plain, patterns, d, on) if sel is None else sel
    return [len(sel), sum(e - s for s, e in sel), len(hits_any(plain, patterns, on)), judged(plain, patterns), len(plain)]


def scan_stats(plain: bytes, patterns, on: bool = False):
    """the first four of FCX_SET_SCAN_STATS by their definitions: positions judged; of those, the positions p whose
    candidate mask T0[D'[p]] & T1[D'[p + 1]] is not zero (D' the folded bytes, 0 behind the end; bit k of T0[b] iff
    pat_k[0] == b, of T1[b] iff len_k < 2 or pat_k[1] == b); the (p, k) pairs of that mask with len_k > 2 and
    p + len_k <= T, which go to the full compare; hits"""
    text, pats, T = fold(plain, on), [fold(p, on) for p in patterns], len(plain)
    first = {}
    for k, p in enumerate(pats):
        first.setdefault(p[0], []).append(k)
    nj = judged(plain, patterns)
    cand = compares = 0
    for p in range(nj):
        b1 = text[p + 1] if p + 1 < T else 0
        ks = [k for k in first.get(text[p], ()) if len(pats[k]) < 2 or pats[k][1] == b1]
        cand += bool(ks)
        compares += sum(1 for k in ks if len(pats[k]) > 2 and p + len(pats[k]) <= T)
    return [nj, cand, compares, len(hits_any(plain, patterns, on))]


def common_head(plain: bytes) -> bytes:
    """the two lower-case letters that occur side by side most often in plain"""
    seen = {}
    for i in range(len(plain) - 1):
        h = plain[i:i + 2]
        if h.isalpha() and h.islower():
            seen[h] = seen.get(h, 0) + 1
    return max(sorted(seen), key=seen.get)


def absent_set(plain: bytes, n: int = 64, m: int = 6):
    """n distinct patterns of m bytes none of which occurs in plain, folded or not (checked); every one starts with
    the two bytes of common_head, so that the filter lets candidates through"""
    head = common_head(plain)
    out, seed = [], 0
    while len(out) < n:
        seed += 1
        p = head + fm.rand(2000 + seed, m - 2)
        if p not in out and fold(plain, True).find(fold(p, True)) < 0 and plain.find(p) < 0:
            out.append(p)
    return out


# ---- the crafted file: grep_model's 20000 bytes at block 5000 (its delimiters and marks stay where they are), with
# the plants of the mixed-length cases on top.  SHORT1 and SHORT3 are the short patterns, LONG pads the set to M = 256.
SHORT1, SHORT3 = b"\x16", b"\x17\x18\x19"
UP, UP_TEXT = b"QuErY", b"qUERy"      # a pattern given in mixed case, the text in another
FOLD_PAT = bytes(FOLD_BYTES)
N, BLOCK = gm.CRAFT_N, gm.CRAFT_BLOCK
DELIMS_AT = sorted(gm.CRAFT_DELIMS + [9900])   # one more: a delimiter inside the last M - 1 bytes of decode group 1
SET_PLANTS = {
    # SHORT1 / SHORT3 inside the last 255 bytes of the run, SHORT1 at T - 1
    "short patterns in the run's last M - 1 bytes": {SHORT1: [N - 150, N - 1], SHORT3: [N - 250]},
    # inside the last M - 1 bytes of decode group 0 (bounds 3000 and 1: a group is one record of 5000)
    "short patterns in a group's last M - 1 bytes": {SHORT1: [4800, 4999], SHORT3: [4900, 4995]},
    # a short hit with the delimiter behind it, both inside the bytes group 1 carries: the line (9001, 9901)
    "short hit, then the delimiter, inside the carry": {SHORT3: [9800]},
    # a short hit behind that delimiter, both inside the carry: the line (9901, 10501) starts inside the carry
    "delimiter, then a short hit, inside the carry": {SHORT1: [9950]},
    "ab and abc at one position, overlap at p and p + 1": {b"\x1a\x1b\x1c": [700], b"\x1b\x1c\x1d": [701]},
    "mixed case": {UP_TEXT: [1500, 15000]},
    "the fold's boundary bytes": {FOLD_PAT: [2000], FOLD_PAT.translate(FOLD): [2100]},
    "hits of two patterns in one line": {SHORT1: [3100], SHORT3: [3200]},
    "the long line's first and last group, different patterns": {SHORT1: [12300], SHORT3: [19800]},
}
LONG = bytes(range(0x80, 0xFF)) * 2 + b"\x80\x81"   # 256 bytes without a delimiter of the tests, not in the file


def crafted(d: int) -> bytes:
    data = bytearray(gm.crafted(d))
    data[9900] = d
    low = set(SHORT1 + SHORT3 + b"\x1a\x1b\x1c\x1d")
    for i, b in enumerate(data):   # the plants' bytes occur nowhere else
        if b in low and b != d:
            data[i] = 0x2E
    for plants in SET_PLANTS.values():
        for pat, at in plants.items():
            for p in at:
                assert d not in pat
                data[p:p + len(pat)] = pat
    return bytes(data)


def check_crafted(plain: bytes, d: int):
    """every plant, asserted in the oracle's decoded bytes"""
    assert len(plain) == N and [i for i, b in enumerate(plain) if b == d] == DELIMS_AT
    want = {}
    for plants in SET_PLANTS.values():
        for pat, at in plants.items():
            want.setdefault(pat, []).extend(at)
    for pat, at in want.items():
        assert fm.hits(plain, pat) == sorted(at), pat
    assert plain.find(LONG) < 0 and len(LONG) == 256
    L = lambda p: gm.line_of(plain, d, p)
    M = 256
    assert N - (M - 1) <= N - 250 and plain[N - 1:] == SHORT1
    assert BLOCK - (M - 1) <= 4800 and plain[4999:5000] == SHORT1
    assert L(9800) == (9001, 9901) and 10000 - (M - 1) <= 9800 < 9900 < 10000    # hit, then d, inside the carry of group 1
    assert L(9950) == (9901, 10501) and 10000 - (M - 1) <= 9900 < 9950 < 10000   # d, then the hit, inside it
    assert fm.hits(plain, gm.MARK)[3:6] == [4080, 4093, 4100]   # grep_model's marks stay: one lies across the tile seam
    assert L(3100) == L(3200) == (3001, 4501)
    assert L(12300) == L(19800) == (12154, 19990)
    assert L(N - 1) == (19990, N)   # the unterminated tail line holds SHORT1 at T - 1 (and grep_model's mark)
    assert hits_any(plain, [b"\x1a\x1b", b"\x1a\x1b\x1c", b"\x1b\x1c\x1d"]) == [700, 701]
    assert hits_any(plain, [UP], False) == [] and hits_any(plain, [UP], True) == [1500, 15000]
    # of the boundary bytes only 0x41 and 0x5A fold: the folded plant matches the unfolded pattern with the flag alone
    assert hits_any(plain, [FOLD_PAT], False) == [2000] and hits_any(plain, [FOLD_PAT], True) == [2000, 2100]
    assert FOLD_PAT.translate(FOLD) == bytes([0x40, 0x61, 0x7A, 0x5B, 0x60, 0x61, 0x7A, 0x7B, 0xC1, 0xE1])
