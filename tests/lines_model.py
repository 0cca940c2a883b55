"""Helpers of the line tests: what the definitions of include/fcx.h say about the oracle's decoded bytes, by
bytes.count and bytes.split, and the crafted files.  Nothing here runs the code under test."""
import re

import inputs

CHUNK_SRC = "my_compress_amd/csrc/fcx_lines.hip"
DELIMS = [0x0A, 0x00, 0xFF, 0x80, 0x20]
U64_MAX = 2**64 - 1
TOTALS = re.compile(r"^lines: (\d+) lines, (\d+) delimiters, decoded bytes = (\d+)$", re.M)
DONE = re.compile(r"^lines decompress bytes = (\d+) \(offset (\d+)\)$", re.M)
NUMBERED = re.compile(r"^find: offset (\d+) line (\d+)$", re.M)


def text(seed, n):
    return inputs.generate("text", seed, n)


def chunk_bytes(root) -> int:
    """kLChunk, read from the source: the decoded bytes a wave of k_lcount counts into one value"""
    src = (root / CHUNK_SRC).read_text()
    return int(re.search(r"constexpr uint32_t kLChunk = (\d+);", src).group(1))


def nl(plain: bytes, d: int, x: int = None) -> int:
    """delimiters in front of offset x (None: in all of plain)"""
    return plain.count(bytes([d]), 0, len(plain) if x is None else x)


def stats(plain: bytes, d: int):
    """FCX_LINES_STATS: delimiters, lines, decoded bytes, bytes behind the last delimiter"""
    n, T = nl(plain, d), len(plain)
    last = plain.rfind(bytes([d])) + 1   # (0 when there is none)
    return [n, n + (1 if T > 0 and plain[-1] != d else 0), T, T - last]


def lines(plain: bytes, d: int):
    """the lines, each with the delimiter that ends it; an unterminated tail is a line"""
    parts = plain.split(bytes([d]))
    out = [p + bytes([d]) for p in parts[:-1]]
    if parts[-1]:
        out.append(parts[-1])
    assert b"".join(out) == plain
    return out


def starts(plain: bytes, d: int):
    """s_j for 0 <= j <= nl(T)"""
    s, at = [0], plain.find(bytes([d]))
    while at >= 0:
        s.append(at + 1)
        at = plain.find(bytes([d]), at + 1)
    return s


def locate(plain: bytes, d: int, first: int, count: int):
    """(off, len) of lines [first, first + count); count U64_MAX or beyond: to the end"""
    L, T = lines(plain, d), len(plain)
    if first >= len(L):
        # s_first exists for first == nl(T) too (a file that ends with its delimiter): it is T
        return T, 0
    off = sum(len(x) for x in L[:first])
    take = L[first:min(first + count, len(L))]
    return off, sum(len(x) for x in take)


def line_off(plain: bytes, d: int, dec_off):
    return [nl(plain, d, x) for x in dec_off]


def ranks(plain: bytes, d: int, offsets):
    """nl(x) for many offsets at once: the number of delimiter positions below x, by bisection"""
    import bisect

    pos = [s - 1 for s in starts(plain, d)[1:]]
    return [bisect.bisect_left(pos, x) for x in offsets]


def crafted(d: int, chunk: int, n: int = 20000, block: int = 5000):
    """(data, the offsets that hold d): text with d planted at the run's ends, around the record seams, around
    the seams of the count's chunks (from the run's start and from a record's), at 15 / 16 within a 16-byte
    piece, 40 in a row across a record seam, and the traps of a word-wise count: stretches of d, d ^ 1, of
    d ^ 1, d and of d ^ 0x80.  Behind the last stretch no byte is d until the last one: a line longer than a
    record."""
    at = {0, n - 1, block - 1, block, 15, 16, chunk - 1, chunk, block + chunk - 1, block + chunk}
    at |= set(range(2 * block - 20, 2 * block + 20))
    b = bytearray(plant(text(31 + d, n), d, at))
    for i in range(64):
        b[12000 + i] = d if i % 2 == 0 else d ^ 1
        b[12100 + i] = d ^ 1 if i % 2 == 0 else d
        b[12200 + i] = d ^ 0x80
    at |= {12000 + i for i in range(0, 64, 2)} | {12100 + i for i in range(1, 64, 2)}
    return bytes(b), sorted(at)


def plant(data: bytes, d: int, at) -> bytes:
    """data with the byte d at every offset of `at`, and with every other byte equal to d changed"""
    b = bytearray(x if x != d else x ^ 0x55 for x in data)
    for p in at:
        b[p] = d
    return bytes(b)
