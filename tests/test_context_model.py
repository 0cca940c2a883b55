"""The context-grep model (context_model.py) against GNU grep and against the models it extends.  The GPU tests and the
command-line tests compare the code under test with this model, so the model itself is pinned here: hand-written
cases, `grep -a -n -F [-v] [-i] -A a -B b` over random small texts (the selected line numbers parsed from its `N:` /
`N-` prefixes, the blocks from its `--` lines), and the identities that tie it to grep_model and set_model."""
import os
import random
import re
import shutil
import subprocess

import pytest

import context_model as cm
import grep_model as gm
import lines_model as lm
import set_model as sm

GREP = shutil.which("grep")


def test_hand_cases():
    plain = b"a\nxb\nc\n\nd\nxe\nf"   # lines 0..6; 1 and 5 match `x`; 3 is empty; 6 is the unterminated tail
    B = lambda **kw: cm.blocks(plain, [b"x"], 0x0A, **kw)
    assert cm.bounds(plain, 0x0A) == [(0, 2), (2, 5), (5, 7), (7, 8), (8, 10), (10, 13), (13, 14)]
    assert B() == [(2, 5, 1, 1), (10, 13, 5, 1)]
    assert B(invert=True) == [(0, 2, 0, 1), (5, 10, 2, 3), (13, 14, 6, 1)]
    assert B(before=1) == [(0, 5, 0, 2), (8, 13, 4, 2)]
    assert B(after=1) == [(2, 7, 1, 2), (10, 14, 5, 2)]
    assert B(before=1, after=2) == [(0, 14, 0, 7)]        # 1 + 2 + 1 lines apart: the blocks touch
    assert B(before=1, after=1) == [(0, 7, 0, 3), (8, 14, 4, 3)]   # one unselected line between them
    assert B(before=4096, after=4096) == [(0, 14, 0, 7)]
    assert B(invert=True, after=1) == [(0, 14, 0, 7)]
    assert cm.stats(plain, [b"x"], 0x0A, invert=True) == [3, 5, 8, 5, 2, 14, 14, 7]
    assert cm.blocks(b"", [b"x"], 0x0A, invert=True) == [] and cm.bounds(b"", 0x0A) == []
    assert cm.blocks(b"abc", [b"x"], 0x0A, invert=True) == [(0, 3, 0, 1)]       # no delimiter: one line
    assert cm.blocks(b"x\n", [b"x"], 0x0A, after=3) == [(0, 2, 0, 1)]           # ends in a delimiter: no line behind it
    assert cm.blocks(b"\n\n", [b"x"], 0x0A, invert=True) == [(0, 2, 0, 2)]      # empty lines never match
    assert cm.join(plain, B(before=1, after=1), b"--\n") == b"a\nxb\nc\n--\nd\nxe\nf"


def grep_lines(text: bytes, patterns, d, fold, invert, before, after, tmp):
    """(selected line numbers 0-based, number of blocks or None when grep prints no separators) by GNU grep"""
    path = tmp / "text"
    path.write_bytes(text)
    cmd = [GREP, "-a", "-n", "-F", "-A", str(after), "-B", str(before)]
    cmd += ["-z"] * (d == 0) + ["-v"] * invert + ["-i"] * fold
    for p in patterns:
        cmd += ["-e", p.decode()]
    r = subprocess.run(cmd + [str(path)], stdout=subprocess.PIPE, env=dict(os.environ, LC_ALL="C"))
    assert r.returncode in (0, 1), r
    out, lines, seps = r.stdout, [], 0
    for rec in out.split(bytes([d])):
        while rec.startswith(b"--\n"):
            seps += 1
            rec = rec[3:]
        if d == 0x0A and rec == b"--":
            seps += 1
            continue
        if not rec:
            continue
        m = re.match(rb"(\d+)[:-]", rec)
        assert m, rec
        lines.append(int(m.group(1)) - 1)
    return lines, (seps + 1 if lines else 0) if before or after else None


@pytest.mark.skipif(GREP is None, reason="grep is not installed")
@pytest.mark.parametrize("d", [0x0A, 0x00])
def test_model_is_gnu_grep(d, tmp_path):
    rng = random.Random(1000 + d)
    for _ in range(200):
        nlines = rng.choice([0, 1, 2, 3, 5, 8, 13, 30])
        body = [bytes(rng.choice(b"abAB") for _ in range(rng.choice([0, 0, 1, 2, 3, 6]))) for _ in range(nlines)]
        text = bytes([d]).join(body) + (bytes([d]) if body and rng.random() < 0.6 else b"")
        patterns = rng.choice([[b"a"], [b"ab"], [b"b", b"aa"], [b"Ab"], [b"aB", b"ba", b"bbb"], [b"q"]])
        fold, invert = rng.random() < 0.3, rng.random() < 0.5
        before, after = rng.choice([0, 0, 1, 2, 3, 40]), rng.choice([0, 0, 1, 2, 3, 40])
        want, nblocks = grep_lines(text, patterns, d, fold, invert, before, after, tmp_path)
        blk = cm.blocks(text, patterns, d, fold, invert, before, after)
        got = [j for x in blk for j in range(x[2], x[2] + x[3])]
        assert got == want, (text, patterns, fold, invert, before, after)
        assert nblocks is None or len(blk) == nblocks, (text, patterns, fold, invert, before, after)
        b = cm.bounds(text, d)
        assert all((x[0], x[1]) == (b[x[2]][0], b[x[2] + x[3] - 1][1]) for x in blk)
        assert all(x[2] + x[3] < y[2] for x, y in zip(blk, blk[1:]))   # an unselected line between two blocks


@pytest.mark.parametrize("d", gm.DELIMS)
def test_zero_options_are_the_grep(d):
    plain = gm.crafted(d)
    blk = cm.blocks(plain, [gm.MARK], d)
    assert cm.join(plain, blk) == gm.join(plain, gm.selected(plain, gm.MARK, d))
    lines = [(b[0] + 0, b[1]) for b in cm.bounds(plain, d)]
    sel = [lines[j] for x in blk for j in range(x[2], x[2] + x[3])]
    assert sel == gm.selected(plain, gm.MARK, d) == sm.selected_any(plain, [gm.MARK], d)
    st, gs = cm.stats(plain, [gm.MARK], d, blk=blk), gm.stats(plain, gm.MARK, d)
    assert (st[1], st[2], st[4], st[5], st[6]) == tuple(gs) and st[3] == st[1] and st[7] == len(lm.lines(plain, d))


@pytest.mark.parametrize("d", gm.DELIMS)
def test_invert_partitions_the_lines(d):
    plain = sm.crafted(d)
    for pats, fold in (([gm.MARK], False), ([sm.SHORT1, sm.SHORT3], False), ([sm.UP], True)):
        L = len(cm.bounds(plain, d))
        m, b = cm.matching(plain, pats, d, fold), cm.base_lines(plain, pats, d, fold, invert=True)
        assert len(m) + len(b) == L == lm.stats(plain, d)[1] and sorted(m + b) == list(range(L))
        assert cm.stats(plain, pats, d, fold, True)[3] == L - len(m)
