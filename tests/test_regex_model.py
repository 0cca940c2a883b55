"""regex_model pinned against two implementations that are not ours: the matching lines and the -v / -A / -B / -C output
against GNU grep (LC_ALL=C grep -aE, d = 0x0A), the match-end positions against Python's re on short lines.  Every
construct of the subset, each anchor, the fold and each refusal."""
import os
import random
import re
import subprocess

import pytest

import context_model as cm
import regex_model as rm

WORDS = [b"ERROR", b"error", b"Warn", b"at", b"foo", b"bar", b"foobar", b"abba", b"aab", b"b", b"a", b"x=1", b"key_1=val", b"42", b"7",
         b"0x1F", b"dead:beef", b"a.b", b"(x)", b"[y]", b"$HOME", b"^top", b"tab\there", b"caf\xc3\xa9", b"\xc1\xe1", b"Z", b"@", b"`", b"{z}",
         b"user@host.com", b"a+b*c?", b"back\\slash", b"--", b"end"]

# expressions valid in POSIX ERE and in Python's re alike, with the same meaning
BOTH = [b"foo", b"fo+", b"fo*b", b"(foo|bar)+", b"^foo", b"bar$", b"^foo$|^bar", b"a|b$", b"[0-9]+", b"[^0-9 ]+=", b"ERROR [0-9]+ at$",
        b"a.b", b"a\\.b", b"\\(x\\)", b"\\$HOME", b"\\^top", b"a{2}b", b"a{2,}", b"ab{1,2}a", b"(ab|ba){2}", b"x?=1", b"\\w+@\\w+\\.com$",
        b"\\W\\W", b"\\s\\S+\\s", b"^\\S+$", b"[a-c]{3}", b"[]x]", b"[^]a-z ]+", b"[a-]b", b"a[^b]{4}b", b"^.{5}$", b"(a|b)(a|b)a", b"\\{z\\}",
        b"((a))+b", b"\\\\s", b"caf\xc3\xa9", b"[\xc0-\xc2]\xe1", b"e(r+|n)d?", b"0x[0-9A-F]+"]
# what only POSIX spells
POSIX = [b"[[:alpha:]_][[:alnum:]_]*=", b"[[:digit:]]+$", b"^[[:upper:]]+ ", b"[[:space:]][[:lower:]]+[[:space:]]", b"[[:punct:]]{2}",
         b"0x[[:xdigit:]]+", b"[^[:alnum:][:space:]]", b"[\\]a", b"[[:alpha:]-]+:"]
REFUSED = [b"a*", b"^$", b"^", b"$", b"(a|)", b"a||b", b"|a", b"a|", b"()", b"a\nb", b"[a\n]", b"[\x00-\x20]x", b"\\1", b"(a)\\1", b"\\bfoo", b"foo\\b",
           b"\\<a", b"a\\>", b"\\d+", b"\\n", b"a^b", b"a$b", b"(^a)", b"(a$)", b"^*a", b"*a", b"+", b"a{", b"a{,3}", b"a{3,2}", b"a{256}", b"a{0}b", b"a{0,0}b", b"((((a{0}){255}){255}){255}){255}b", b"(a", b"a)",
           b"[a", b"[[:nope:]]", b"[b-a]", b"a\\", b"x?", b"(a?|b*)", b"(a{4}){20}{20}", b"[[.a.]]", b"\xe9*"]


def sample(seed: int, nlines: int, tail: bool = False) -> bytes:
    r = random.Random(seed)
    lines = []
    for _ in range(nlines):
        n = r.choice([0, 1, 1, 2, 3, 4, 6, 9])
        lines.append(r.choice([b" ", b"\t", b"  "]).join(r.choice(WORDS) for _ in range(n)))
    out = b"\n".join(lines) + b"\n"
    return out + b"foo bar 42" if tail else out


PLAIN = sample(3, 400)
TAIL = sample(4, 120, tail=True)


def gnu_grep(plain: bytes, expr: bytes, tmp_path, *flags):
    p = tmp_path / "in"
    p.write_bytes(plain)
    r = subprocess.run(["grep", "-aE", *flags, "-e", expr, str(p)], env=dict(os.environ, LC_ALL="C"), capture_output=True)
    assert r.returncode in (0, 1), r.stderr
    return r.stdout


def model_out(plain: bytes, expr: bytes, fold=False, invert=False, before=0, after=0):
    blk = rm.blocks(plain, rm.Nfa(expr, 0x0A, fold), invert, before, after)
    out = cm.join(plain, blk, cm.separator(0x0A, before, after))
    return out if not out or out.endswith(b"\n") else out + b"\n"   # (grep ends an unterminated last line)


@pytest.mark.parametrize("expr", BOTH + POSIX, ids=repr)
def test_matching_lines_are_gnu_greps(expr, tmp_path):
    for plain in (PLAIN, TAIL):
        assert model_out(plain, expr) == gnu_grep(plain, expr, tmp_path), expr
    assert model_out(PLAIN, expr, fold=True) == gnu_grep(PLAIN, expr, tmp_path, "-i"), expr
    assert model_out(PLAIN, expr, invert=True) == gnu_grep(PLAIN, expr, tmp_path, "-v"), expr


@pytest.mark.parametrize("opt", [(0, 1, 0), (0, 0, 2), (0, 3, 3), (1, 1, 1), (1, 0, 2)], ids=str)
def test_context_output_is_gnu_greps(opt, tmp_path):
    inv, b, a = opt
    for expr in (b"ERROR [0-9]+ at$", b"^foo", b"[[:punct:]]{2}", b"a[^b]{4}b", b"^\\S+$"):
        flags = (["-v"] if inv else []) + [f"-B{b}", f"-A{a}"]
        for plain in (PLAIN, TAIL):
            assert model_out(plain, expr, False, bool(inv), b, a) == gnu_grep(plain, expr, tmp_path, *flags), (expr, opt)


def top_level(expr: bytes):
    """[(bol, body, eol)] of the top-level alternatives (for expressions of BOTH)"""
    parts, depth, cur, i, in_set = [], 0, bytearray(), 0, False
    while i < len(expr):
        c = expr[i:i + 1]
        if in_set:
            in_set = not (c == b"]" and len(cur) - set_at > (2 if cur[set_at + 1:set_at + 2] == b"^" else 1))
        elif c == b"\\":
            cur += expr[i:i + 2]
            i += 2
            continue
        elif c == b"[":
            in_set, set_at = True, len(cur)
        elif c in b"()":
            depth += 1 if c == b"(" else -1
        elif c == b"|" and depth == 0:
            parts.append(bytes(cur))
            cur = bytearray()
            i += 1
            continue
        cur += c
        i += 1
    parts.append(bytes(cur))
    out = []
    for p in parts:
        bol, eol = p.startswith(b"^"), p.endswith(b"$") and not p.endswith(b"\\$")
        out.append((bol, p[bol:len(p) - eol], eol))
    return out


@pytest.mark.parametrize("fold", [False, True])
@pytest.mark.parametrize("expr", BOTH, ids=repr)
def test_match_ends_are_pythons(expr, fold):
    alts = [(bol, re.compile(b"(?:" + body + b")" + (b"" if bol else b"\\Z"), re.S | (re.I if fold else 0)), eol) for bol, body, eol in top_level(expr)]
    nfa = rm.Nfa(expr, 0x0A, fold)
    lines = [ln for ln in (PLAIN + TAIL).split(b"\n") if 0 < len(ln) <= 200][:150]
    assert len(lines) == 150
    for ln in lines:
        want = [p for p in range(len(ln))
                if any((rx.fullmatch(ln[:p + 1]) if bol else rx.search(ln[:p + 1])) and (not eol or p == len(ln) - 1) for bol, rx, eol in alts)]
        assert nfa.line_hits(ln) == want, (expr, ln)


@pytest.mark.parametrize("expr", REFUSED, ids=repr)
def test_refusals(expr):
    with pytest.raises(rm.Refused):
        rm.Nfa(expr, 0x0A)


def test_refusals_that_depend_on_the_delimiter_and_the_fold():
    rm.Nfa(b"a", 0x41)
    with pytest.raises(rm.Refused):
        rm.Nfa(b"a", 0x41, True)       # a folds to what the delimiter folds to
    with pytest.raises(rm.Refused):
        rm.Nfa(b"xAy", 0x61, True)
    with pytest.raises(rm.Refused):
        rm.Nfa(b"[a-c]", 0x42, True)
    rm.Nfa(b"[^a-c]x", 0x42, True)     # a negated set leaves the delimiter out instead
    assert rm.Nfa(b"[[:upper:]]", 0x42).line_hits(b"ABC") == [0, 2]   # as do the named classes and the shorthands
    assert rm.Nfa(b"\\w", 0x5F).line_hits(b"a_b") == [0, 2]
    assert rm.Nfa(b".", 0x00).line_hits(b"a\x00b") == [0, 2]
    with pytest.raises(rm.Refused):
        rm.Nfa(b"a" * 1025)
    rm.Nfa(b"(a{4}){16}{16}")           # 1024 positions
    with pytest.raises(rm.Refused):
        rm.Nfa(b"(a{4}){16}{16}a")


def test_hits_are_ends_inside_the_lines_body():
    plain = b"ab\n\nxab\nab"
    nfa = rm.Nfa(b"ab$|^x")
    assert rm.hits(plain, nfa) == [1, 4, 6, 9]
    assert rm.base_lines(plain, nfa) == [0, 2, 3] and rm.base_lines(plain, nfa, invert=True) == [1]
    assert rm.blocks(plain, nfa) == [(0, 3, 0, 1), (4, 10, 2, 2)]
    assert rm.stats(plain, nfa) == [2, 3, 9, 3, 4, 10, 10, 4]
