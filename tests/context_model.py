"""Helpers of the context-grep tests: what the definitions of include/fcx.h (context and inverted grep) say about the
oracle's decoded bytes, over lines_model.starts and the set model's hits.  Nothing here runs the code under test."""
import bisect
import re

import lines_model as lm
import set_model as sm

TOTALS = re.compile(r"^grep: (\d+) blocks, (\d+) lines, (\d+) base lines, (\d+) bytes, (\d+) hits, decoded bytes = (\d+)$", re.M)
MAX_CONTEXT = 4096


def bounds(plain: bytes, d: int):
    """[(s_j, e_j)] of every line: an unterminated tail is a line, T == 0 has none"""
    s, T = lm.starts(plain, d), len(plain)
    e = s[1:] + [T]
    return [(a, b) for a, b in zip(s, e) if a < b]


def matching(plain: bytes, patterns, d: int, fold: bool = False):
    """the numbers of the lines that hold a hit, ascending"""
    for p in patterns:
        assert bytes([d]) not in p and (not fold or sm.fold(bytes([d]), True) not in sm.fold(p, True))
    s = lm.starts(plain, d)
    return sorted({bisect.bisect_right(s, p) - 1 for p in sm.hits_any(plain, patterns, fold)})


def base_lines(plain: bytes, patterns, d: int, fold=False, invert=False):
    L, m = len(bounds(plain, d)), set(matching(plain, patterns, d, fold))
    return [j for j in range(L) if (j in m) != invert]


def selected_lines(L: int, base, before: int, after: int):
    """line j is selected iff some base line k has j - after <= k <= j + before"""
    out = []
    for j in range(L):
        i = bisect.bisect_left(base, j - after)
        if i < len(base) and base[i] <= j + before:
            out.append(j)
    return out


def blocks(plain: bytes, patterns, d: int, fold=False, invert=False, before=0, after=0):
    """[(start, end, line, nlines)]: the maximal runs of consecutive selected lines, ascending"""
    b = bounds(plain, d)
    sel = selected_lines(len(b), base_lines(plain, patterns, d, fold, invert), before, after)
    out = []
    for j in sel:
        if out and out[-1][2] + out[-1][3] == j:
            out[-1] = (out[-1][0], b[j][1], out[-1][2], out[-1][3] + 1)
        else:
            out.append((b[j][0], b[j][1], j, 1))
    return out


def stats(plain: bytes, patterns, d: int, fold=False, invert=False, before=0, after=0, blk=None):
    """FCX_GREP_BLOCK_STATS: blocks, selected lines, bytes, base lines, hits, judged, decoded, lines"""
    blk = blocks(plain, patterns, d, fold, invert, before, after) if blk is None else blk
    return [len(blk), sum(x[3] for x in blk), sum(x[1] - x[0] for x in blk), len(base_lines(plain, patterns, d, fold, invert)),
            len(sm.hits_any(plain, patterns, fold)), sm.judged(plain, patterns), len(plain), len(bounds(plain, d))]


def join(plain: bytes, blk, sep: bytes = b"") -> bytes:
    """the blocks' bytes, `sep` between blocks (the command line's `--` line when a context is asked for)"""
    return sep.join(plain[x[0]:x[1]] for x in blk)


def separator(d: int, before: int, after: int) -> bytes:
    return b"--\n" if before or after else b""
