"""Helpers of the grep tests: what the definitions of include/fcx.h say about the oracle's decoded bytes.  The
selected lines come from lines_model.starts and find_model.hits, the multi-range decode's answer is a join of
slices.  Nothing here runs the code under test."""
import bisect
import re

import find_model as fm
import lines_model as lm

LENGTHS = [1, 4, 5, 16, 33, 255, 256]
DELIMS = [0x0A, 0x00, 0xFF]
MARK = b"\x11\x12\x13\x14\x15"   # in no text and no delimiter: the crafted hits
TOTALS = re.compile(r"^grep: (\d+) lines, (\d+) bytes, (\d+) hits, decoded bytes = (\d+)$", re.M)


def selected(plain: bytes, pattern: bytes, d: int):
    """[(start, end)] of the lines that hold at least one hit, ascending, each once"""
    assert bytes([d]) not in pattern
    s, T, out = lm.starts(plain, d), len(plain), []
    for p in fm.hits(plain, pattern):
        j = bisect.bisect_right(s, p) - 1
        if not out or out[-1][0] != s[j]:
            out.append((s[j], s[j + 1] if j + 1 < len(s) else T))
    return out


def stats(plain: bytes, pattern: bytes, d: int, sel=None):
    """FCX_GREP_STATS: lines, bytes, hits, judged, decoded"""
    sel = selected(plain, pattern, d) if sel is None else sel
    T = len(plain)
    return [len(sel), sum(e - s for s, e in sel), len(fm.hits(plain, pattern)), max(T - len(pattern) + 1, 0), T]


def join(plain: bytes, ranges) -> bytes:
    return b"".join(plain[s:e] for s, e in ranges)


def line_of(plain: bytes, d: int, p: int):
    """(start, end) of the line that holds offset p"""
    s = lm.starts(plain, d)
    j = bisect.bisect_right(s, p) - 1
    return s[j], s[j + 1] if j + 1 < len(s) else len(plain)


# the crafted file: 20000 bytes at block 5000; where the delimiters and the marks are planted
CRAFT_N, CRAFT_BLOCK = 20000, 5000
CRAFT_DELIMS = [60, 100, 101, 102, 200, 300, 3000, 4500, 5600, 9000, 10500, 12153, 19989]
CRAFT_MARKS = {
    "line 0, no delimiter in front": [10],
    "at a line's first byte": [201],
    "ending right in front of the delimiter": [295],
    "both sides of the tile seam 4095/4096": [4080, 4100],
    "across the tile seam": [4093],
    "both sides of a record seam": [4990, 5003],
    "both sides of a decode-group seam": [9990, 10010],
    "first and last group of the 7836-byte line": [12200, 19900],
    "the unterminated tail line": [19992],
}


def crafted(d: int) -> bytes:
    data = bytearray(lm.plant(fm.text(41 + d, CRAFT_N), d, CRAFT_DELIMS))
    for at in CRAFT_MARKS.values():
        for p in at:
            data[p:p + len(MARK)] = MARK
    return bytes(data)


def check_crafted(plain: bytes, d: int):
    """every plant, asserted in the oracle's decoded bytes"""
    assert len(plain) == CRAFT_N
    assert [i for i, b in enumerate(plain) if b == d] == CRAFT_DELIMS
    marks = sorted(p for at in CRAFT_MARKS.values() for p in at)
    assert fm.hits(plain, MARK) == marks
    L = lambda p: line_of(plain, d, p)
    assert L(10) == (0, 61) and L(201)[0] == 201 and L(295)[1] == 301 and plain[299] == MARK[-1]
    assert L(4080) == L(4100) == L(4093) == (3001, 4501)
    assert L(4990) == L(5003) == (4501, 5601) and L(9990) == L(10010) == (9001, 10501)
    assert L(12200) == L(19900) == (12154, 19990) and 19990 - 12154 == 7836
    assert L(19992) == (19990, CRAFT_N) and plain[-1] != d
    assert lm.lines(plain, d)[2:4] == [bytes([d])] * 2   # the run of empty lines
    sel = selected(plain, MARK, d)
    assert len(sel) == 7 and (101, 102) not in sel and (102, 103) not in sel
    return sel


def cut(plain: bytes, d: int, p: int, m: int):
    """the longest pattern of at most m bytes at p that holds no delimiter and stays inside (None: none)"""
    pat = plain[p:p + m]
    at = pat.find(bytes([d]))
    pat = pat if at < 0 else pat[:at]
    return pat or None
