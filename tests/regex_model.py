"""Helpers of the regex-grep tests: what the definitions of include/fcx.h (regular-expression grep) say about the
oracle's decoded bytes.  A parser for the ERE subset, an NFA with empty moves simulated as a set of states per byte
(no DFA, no tables, no minimisation: a second implementation that shares nothing with fcx_regex.h), and hits, base
lines and blocks over context_model and lines_model.  Nothing here runs the code under test."""
import bisect

import context_model as cm
import lines_model as lm

CLASSES = {
    "alpha": lambda b: chr(b).isalpha(), "digit": lambda b: chr(b).isdigit(), "alnum": lambda b: chr(b).isalnum(),
    "upper": lambda b: chr(b).isupper(), "lower": lambda b: chr(b).islower(), "space": lambda b: chr(b) in " \t\n\v\f\r",
    "punct": lambda b: 32 < b < 127 and not chr(b).isalnum(), "xdigit": lambda b: chr(b) in "0123456789abcdefABCDEF",
    "word": lambda b: chr(b).isalnum() or b == 0x5F,
}
MAX_POSITIONS, MAX_COUNT = 1024, 255


class Refused(Exception):
    def __init__(self, why, offset=0):
        super().__init__(f"{why} at offset {offset}")
        self.offset = offset


def both_cases(b: int):
    c = chr(b)
    return {b, ord(c.swapcase())} if b < 128 and c.isalpha() else {b}


class Parser:
    """expr -> [(bol, eol, tree)] per top-level alternative; a tree is ("set", frozenset) | ("cat", [trees]) |
    ("alt", [trees]) | ("rep", tree, m, n or None)"""

    def __init__(self, expr: bytes, d: int, fold: bool):
        self.e, self.d, self.fold, self.at, self.alts = expr, d, fold, 0, []

    def named(self, name):
        s = {b for b in range(128) if CLASSES[name](b)}
        if self.fold:
            s = set().union(*[both_cases(b) for b in s]) if s else s
        return s - {self.d}

    def spelled(self, lo, hi, off):
        s = set(range(lo, hi + 1))
        if self.fold:
            s = set().union(*[both_cases(b) for b in s])
        if self.d in s:
            raise Refused("the delimiter in a literal or a set", off)
        return s

    def leaf(self, s, off):
        if not s:
            raise Refused("a set that matches no byte", off)
        return ("set", frozenset(s))

    def bracket(self):
        e, open_ = self.e, self.at - 1
        neg = self.at < len(e) and e[self.at] == 0x5E
        self.at += neg
        s, first = set(), True
        while True:
            if self.at >= len(e):
                raise Refused("unterminated bracket set", open_)
            c = e[self.at]
            if c == 0x5D and not first:
                self.at += 1
                break
            first = False
            if e[self.at:self.at + 2] == b"[:":
                q = e.find(b":]", self.at + 2)
                name = e[self.at + 2:q].decode("latin1") if q >= 0 else None
                if name not in CLASSES or name == "word":
                    raise Refused("unknown character class", self.at)
                s |= self.named(name)
                self.at = q + 2
                continue
            if e[self.at:self.at + 2] in (b"[.", b"[="):
                raise Refused("collating elements are not supported", self.at)
            self.at += 1
            hi = c
            if self.at + 1 < len(e) and e[self.at] == 0x2D and e[self.at + 1] != 0x5D:
                hi = e[self.at + 1]
                if hi < c or e[self.at + 1:self.at + 3] in (b"[:", b"[.", b"[="):
                    raise Refused("bad range", self.at)
                self.at += 2
            r = set(range(c, hi + 1))
            if self.fold:
                r = set().union(*[both_cases(b) for b in r])
            if not neg and self.d in r:
                raise Refused("the delimiter in a literal or a set", self.at - 1)
            s |= r
        if neg:
            s = set(range(256)) - s - {self.d}
        return self.leaf(s, open_)

    def atom(self, depth):
        e, off = self.e, self.at
        c = e[off]
        self.at += 1
        if c == 0x28:
            t = self.alt(depth + 1)
            if self.at >= len(e) or e[self.at] != 0x29:
                raise Refused("unmatched (", off)
            self.at += 1
            return t
        if c == 0x5B:
            return self.bracket()
        if c == 0x2E:
            return ("set", frozenset(set(range(256)) - {self.d}))
        if c in b"^$":
            raise Refused("an anchor that is not the first or last item of a top-level alternative", off)
        if c in b"*+?{":
            raise Refused("a repetition with nothing in front of it", off)
        if c == 0x5C:
            if self.at >= len(e):
                raise Refused("a trailing backslash", off)
            x = e[self.at]
            self.at += 1
            if x in b"wWsS":
                s = self.named("word" if x in b"wW" else "space")
                return self.leaf(set(range(256)) - s - {self.d} if x in b"WS" else s, off)
            if not (32 < x < 127) or chr(x).isalnum() or x in b"<>":
                raise Refused("an escape that is not supported", off)
            return self.leaf(self.spelled(x, x, off), off)
        return self.leaf(self.spelled(c, c, off), off)

    def count(self, off):
        e = self.e
        close = e.find(b"}", self.at)
        body = e[self.at:close].decode("latin1") if close >= 0 else ""
        parts = body.split(",")
        if close < 0 or len(parts) > 2 or not parts[0].isdigit() or (len(parts) == 2 and parts[1] and not parts[1].isdigit()) \
                or not all(ch in "0123456789," for ch in body):
            raise Refused("a malformed repetition count", off)
        self.at = close + 1
        m = int(parts[0])
        n = m if len(parts) == 1 else (int(parts[1]) if parts[1] else None)
        if m > MAX_COUNT or (n is not None and (n > MAX_COUNT or n < m)):
            raise Refused("a repetition count out of range", off)
        if n == 0:
            raise Refused("a repetition count of zero", off)
        return m, n

    def seq(self, depth):
        e, off, items, bol, eol = self.e, self.at, [], False, False
        if depth == 0 and self.at < len(e) and e[self.at] == 0x5E:
            bol = True
            self.at += 1
        while self.at < len(e) and e[self.at] not in b"|)":
            if depth == 0 and e[self.at] == 0x24 and (self.at + 1 == len(e) or e[self.at + 1] == 0x7C):
                eol = True
                self.at += 1
                break
            t = self.atom(depth)
            while self.at < len(e) and e[self.at] in b"*+?{":
                r, roff = e[self.at], self.at
                self.at += 1
                m, n = {0x2A: (0, None), 0x2B: (1, None), 0x3F: (0, 1)}.get(r) or self.count(roff)
                t = ("rep", t, m, n)
            items.append(t)
        if not items:
            raise Refused("the expression matches the empty string" if bol or eol else "an empty alternative", off)
        return bol, eol, ("cat", items)

    def alt(self, depth):
        out = []
        while True:
            bol, eol, t = self.seq(depth)
            out.append(t)
            if depth == 0:
                self.alts.append((bol, eol, t))
            if self.at < len(self.e) and self.e[self.at] == 0x7C:
                self.at += 1
                continue
            if depth == 0 and self.at < len(self.e):
                raise Refused("unmatched )", self.at)
            return ("alt", out)


class Nfa:
    """states are numbers; moves[s] = [(byte set, target)], empty[s] = [targets]"""

    def __init__(self, expr: bytes, d: int = 0x0A, fold: bool = False):
        if not 1 <= len(expr) <= 1024:
            raise Refused("expression length")
        p = Parser(expr, d, fold)
        p.alt(0)
        self.d, self.moves, self.empty, self.positions, self.alts = d, [], [], 0, []
        for bol, eol, t in p.alts:
            a, z = self.build(t)
            if z in self.closure({a}):
                raise Refused("the expression matches the empty string")
            self.alts.append((bol, eol, a, z))

    def state(self):
        self.moves.append([])
        self.empty.append([])
        return len(self.moves) - 1

    def build(self, t):
        a, z = self.state(), self.state()
        if t[0] == "set":
            self.positions += 1
            if self.positions > MAX_POSITIONS:
                raise Refused("more than 1024 positions after expanding the repetitions")
            self.moves[a].append((t[1], z))
        elif t[0] == "alt":
            for x in t[1]:
                xa, xz = self.build(x)
                self.empty[a].append(xa)
                self.empty[xz].append(z)
        elif t[0] == "cat":
            cur = a
            for x in t[1]:
                xa, xz = self.build(x)
                self.empty[cur].append(xa)
                cur = xz
            self.empty[cur].append(z)
        else:
            _, x, m, n = t
            cur = a
            for _i in range(m):
                xa, xz = self.build(x)
                self.empty[cur].append(xa)
                cur = xz
            if n is None:
                xa, xz = self.build(x)
                self.empty[cur] += [xa, z]
                self.empty[xz] += [xa, z]
            else:
                for _i in range(n - m):
                    xa, xz = self.build(x)
                    self.empty[cur] += [xa, z]
                    cur = xz
                self.empty[cur].append(z)
        return a, z

    def closure(self, states):
        seen, todo = set(states), list(states)
        while todo:
            for y in self.empty[todo.pop()]:
                if y not in seen:
                    seen.add(y)
                    todo.append(y)
        return seen

    def line_hits(self, body: bytes, base: int = 0):
        """the positions of `body` (one line without its delimiter) at which a match ends, + base"""
        out, active = [], set()
        free = self.closure({a for bol, _, a, _ in self.alts if not bol})
        at_start = self.closure({a for _, _, a, _ in self.alts})
        for p, byte in enumerate(body):
            active = active | (at_start if p == 0 else free)
            active = self.closure({y for s in active for bs, y in self.moves[s] if byte in bs})
            if any(z in active and (not eol or p == len(body) - 1) for _, eol, _, z in self.alts):
                out.append(base + p)
        return out


def hits(plain: bytes, nfa: Nfa):
    """every hit of the run, ascending"""
    out = []
    for s, e in cm.bounds(plain, nfa.d):
        b = e - 1 if plain[e - 1] == nfa.d else e
        out += nfa.line_hits(plain[s:b], s)
    return out


def base_lines(plain: bytes, nfa: Nfa, invert=False, h=None):
    s = lm.starts(plain, nfa.d)
    m = {bisect.bisect_right(s, p) - 1 for p in (hits(plain, nfa) if h is None else h)}
    return [j for j in range(len(cm.bounds(plain, nfa.d))) if (j in m) != invert]


def blocks(plain: bytes, nfa: Nfa, invert=False, before=0, after=0, h=None):
    """[(start, end, line, nlines)]: the maximal runs of consecutive selected lines, ascending"""
    b = cm.bounds(plain, nfa.d)
    out = []
    for j in cm.selected_lines(len(b), base_lines(plain, nfa, invert, h), before, after):
        if out and out[-1][2] + out[-1][3] == j:
            out[-1] = (out[-1][0], b[j][1], out[-1][2], out[-1][3] + 1)
        else:
            out.append((b[j][0], b[j][1], j, 1))
    return out


def stats(plain: bytes, nfa: Nfa, invert=False, before=0, after=0, blk=None, h=None):
    """FCX_GREP_BLOCK_STATS: blocks, selected lines, bytes, base lines, hits, judged, decoded, lines"""
    h = hits(plain, nfa) if h is None else h
    blk = blocks(plain, nfa, invert, before, after, h) if blk is None else blk
    return [len(blk), sum(x[3] for x in blk), sum(x[1] - x[0] for x in blk), len(base_lines(plain, nfa, invert, h)), len(h), len(plain),
            len(plain), len(cm.bounds(plain, nfa.d))]


# ---- the crafted file: 20000 bytes at block 5000 (tile seams at 4096 k, record and decode-group seams at 5000 k) ----
N, BLOCK = 20000, 5000
R_DELIMS = [60, 100, 101, 102, 200, 300, 3000, 4500, 5000, 9000, 9999, 10500, 12153, 19989]
PLANTS = {
    "^ at position 0": (0, b"#1;"),
    "e in front of a delimiter: a negated set behind it must not take the delimiter": (299, b"e"),
    "ends on the last byte in front of a tile seam": (4092, b"#12;"),
    "ends on the last byte of a record and a decode group; the delimiter behind it opens the next group": (4997, b"#7;"),
    "straddles a tile seam": (8190, b"#345;"),
    "the first byte of a group, the delimiter being the last byte of the group before": (10000, b"#55;"),
    "64 states: # behind 61 other bytes of the 7836-byte line": (12154 + 61, b"#"),
    "ends on the last byte of tile 2, inside the 7836-byte line": (12284, b"#90;"),
    "straddles a record seam and a decode-group seam": (14997, b"#6789;"),
    "a in tile 3 and b in tile 4 of the line that began in tile 2": (16382, b"axxxxb"),
    "$ at T - 1 of the unterminated tail": (19997, b"#9;"),
}
E_ANY, E_EOL, E_BOL, E_MIX = b"#[0-9]+;", b"#[0-9]+;$", b"^#[0-9]+;", b"^#[0-9]+;|;$"
E_FAR, E_NEG, E_64, E_2 = b"a[^b]{4}b", b"e[^a]", b"^[^#]{61}#", b"#"
CRAFT_EXPRS = [E_ANY, E_EOL, E_BOL, E_MIX, E_FAR, E_NEG, E_64, E_2]


def crafted(d: int) -> bytes:
    data = bytearray(lm.plant(lm.text(41 + d, N), d, R_DELIMS))
    for at, what in PLANTS.values():
        data[at:at + len(what)] = what
    return bytes(data)


def check_crafted(plain: bytes, d: int):
    """every plant, asserted in the oracle's decoded bytes"""
    assert len(plain) == N and [i for i, b in enumerate(plain) if b == d] == R_DELIMS and plain[-1] != d
    for at, what in PLANTS.values():
        assert plain[at:at + len(what)] == what
    H = lambda e: hits(plain, Nfa(e, d))
    assert H(E_ANY) == [2, 4095, 4999, 8194, 10003, 12287, 15002, 19999]
    assert H(E_EOL) == [4999, 19999] and plain[5000] == d and 5000 % BLOCK == 0
    assert H(E_BOL) == [2, 10003] and plain[9999] == d and 10000 % BLOCK == 0
    assert H(E_MIX) == [2, 4999, 10003, 19999]
    assert 16387 in H(E_FAR) and 16382 // 4096 == 3 and 16387 // 4096 == 4 and plain[12153] == d and d not in plain[12154:19989]
    assert 300 not in H(E_NEG) and plain[300] == d and all(plain[p] != d and plain[p - 1] == 0x65 for p in H(E_NEG))
    assert H(E_64) == [12154 + 61] and H(E_2) == sorted(at for at, w in PLANTS.values() if w[:1] == b"#")
