"""The cut rule of include/fcx.h as plain Python, for the tests of the cut calls: its own LIST parser, the rule twice
over (byte by byte, and vectorised in numpy through a cumulative tick count minus its value at each line's start) and
the stats.  Nothing here calls the library; test_cut_model.py pins both forms against each other and against GNU cut."""
import re

import numpy as np

import inputs

FIELDS, BYTES = 1, 2
MAX_COLUMN = 4096
SAT = MAX_COLUMN + 1   # every column from here on is selected or not with all the others


class ListError(ValueError):
    def __init__(self, offset, why):
        super().__init__(f"LIST offset {offset}: {why}")
        self.offset = offset


class Sel:
    """a compiled LIST: sel[k] for 1 <= k <= SAT (sel[SAT]: every column above MAX_COLUMN), mn, open_end"""

    def __init__(self, lst, complement: bool = False):
        lst = lst.encode() if isinstance(lst, str) else bytes(lst)
        sel = np.zeros(SAT + 1, dtype=bool)
        self.open_end = False
        if not lst:
            raise ListError(0, "empty list")
        at = 0
        for item in lst.split(b","):
            m = re.fullmatch(rb"([0-9]*)(-?)([0-9]*)", item)
            if m is None:
                bad = next(i for i, b in enumerate(item) if b not in b"0123456789-" or (b == 0x2D and b"-" in item[:i]))
                raise ListError(at + bad, "bad byte")
            lo, dash, hi = m.groups()
            if not lo and not hi:
                raise ListError(at, "empty item")
            if lo and int(lo) == 0:
                raise ListError(at, "zero")
            if hi and int(hi) == 0:
                raise ListError(at + len(lo) + 1, "zero")
            a = int(lo) if lo else 1
            if dash and not hi:
                if a > SAT:
                    raise ListError(at, "open item starts too far out")
                sel[a:] = True
                self.open_end = True
            else:
                b = int(hi) if dash else a
                if a > MAX_COLUMN or b > MAX_COLUMN:
                    raise ListError(at, "above the maximum")
                if b < a:
                    raise ListError(at, "descending")
                sel[a:b + 1] = True
            at += len(item) + 1
        if complement:
            sel[1:] = ~sel[1:]
        sel[0] = False
        if not sel.any():
            raise ListError(0, "nothing selected")
        self.sel = sel
        self.mn = int(np.argmax(sel))

    def __call__(self, k: int) -> bool:
        return bool(self.sel[min(k, SAT)])


def cut_py(plain: bytes, sel: Sel, mode: int, sep: int = 0x09, d: int = 0x0A):
    """the rule byte by byte: (the kept bytes, [kept, judged, delimiters, separators, separators kept])"""
    out = bytearray()
    ticks = nd = ns = nk = 0
    for b in plain:
        if b == d:
            out.append(b)
            nd += 1
            ticks = 0
        elif mode == FIELDS and b == sep:
            k = ticks + 2   # the column this separator opens
            ns += 1
            if sel(k) and k > sel.mn:
                out.append(b)
                nk += 1
            ticks += 1
        else:
            if sel(ticks + 1):
                out.append(b)
            if mode == BYTES:
                ticks += 1
    return bytes(out), [len(out), len(plain), nd, ns, nk]


def cut_np(plain: bytes, sel: Sel, mode: int, sep: int = 0x09, d: int = 0x0A):
    """the same through numpy: ticks(p) = ticks in [0, p) minus ticks in [0, s_j)"""
    a = np.frombuffer(plain, dtype=np.uint8)
    n = len(a)
    if n == 0:
        return b"", [0, 0, 0, 0, 0]
    isd = a == d
    issep = (a == sep) & ~isd if mode == FIELDS else np.zeros(n, dtype=bool)
    tick = issep if mode == FIELDS else ~isd
    before = np.concatenate(([0], np.cumsum(tick, dtype=np.int64)))   # ticks in [0, i)
    idx = np.arange(n, dtype=np.int64)
    nxt = np.maximum.accumulate(np.where(isd, idx + 1, 0))            # the start of the line behind position i
    start = np.concatenate(([0], nxt[:-1]))                            # s_j of the line that holds i
    ticks = before[:-1] - before[start]
    col = np.minimum(ticks + 1, SAT)
    opens = ticks + 2
    keep = isd | (~isd & ~issep & sel.sel[col]) | (issep & sel.sel[np.minimum(opens, SAT)] & (opens > sel.mn))
    return a[keep].tobytes(), [int(keep.sum()), n, int(isd.sum()), int(issep.sum()), int((issep & keep).sum())]


def make_sel(fields=None, byte_list=None, complement=False):
    return (FIELDS, Sel(fields, complement)) if fields is not None else (BYTES, Sel(byte_list, complement))


def table(n: int, d: int, sep: int, seed: int, width=(0, 9), fields=(1, 8)) -> bytes:
    """about n bytes of lines of random fields; every line is terminated and holds a separator"""
    rnd = np.random.RandomState(seed)
    alphabet = bytes(b for b in b"abcdefghijklmnopqrstuvwxyz0123456789 _-" if b not in (d, sep))
    out = bytearray()
    while len(out) < n:
        nf = rnd.randint(max(fields[0], 2), fields[1] + 1)
        cells = [bytes(alphabet[i] for i in rnd.randint(0, len(alphabet), rnd.randint(width[0], width[1] + 1))) for _ in range(nf)]
        out += bytes([sep]).join(cells) + bytes([d])
    return bytes(out)


def text(seed, n):
    return inputs.generate("text", seed, n)
