"""cut_model's two forms of the cut rule against each other, and both against GNU cut (LC_ALL=C) where the rule claims
cut's bytes: terminated inputs in which every line holds a separator, for -f, -b and --complement.  The two documented
differences from GNU cut are pinned as differences."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import cut_model as km

CUT = shutil.which("cut")
LISTS = ["1", "2", "2,4", "1-3", "3-", "-2", "2-3,5-", "1,3,7-9", "9", "4096", "4097-", "1-4096", "2-"]


def gnu_cut(data: bytes, *args) -> bytes:
    env = dict(os.environ, LC_ALL="C")
    return subprocess.run([CUT, *args], input=data, stdout=subprocess.PIPE, check=True, env=env).stdout


def both(plain, fields=None, byte_list=None, complement=False, sep=0x2C, d=0x0A):
    mode, sel = km.make_sel(fields, byte_list, complement)
    a = km.cut_py(plain, sel, mode, sep, d)
    b = km.cut_np(plain, sel, mode, sep, d)
    assert a == b
    return a


def test_the_issue_examples():
    assert both(b"a,b,c,d\n", fields="2,4")[0] == b"b,d\n"
    assert both(b"a,b,c,d\n", fields="5")[0] == b"\n"
    assert both(b"a,b,c,d\n", fields="2,4")[1] == [4, 8, 1, 3, 1]
    assert both(b"abcdef\n", byte_list="2,4-5")[0] == b"bde\n"
    assert both(b"a,b,c\n", fields="1", complement=True)[0] == b"b,c\n"


@pytest.mark.parametrize("seed", range(4))
def test_the_two_forms_agree_on_random_bytes(seed):
    rnd = np.random.RandomState(seed)
    plain = bytes(rnd.choice(np.frombuffer(b",\nab\t\0", dtype=np.uint8), 3000, p=[0.2, 0.1, 0.3, 0.3, 0.05, 0.05]))
    for lst in LISTS:
        for comp in (False, True):
            for kw in ({"fields": lst}, {"byte_list": lst}):
                out, st = both(plain, complement=comp, **kw)
                assert st[0] == len(out) and st[1] == 3000 and st[2] == plain.count(b"\n")
    for d, sep in ((0x00, 0x2C), (0x61, 0x00), (0x0A, 0x09)):
        both(plain, fields="2-3", sep=sep, d=d)
        both(plain, byte_list="2-3", d=d)


def test_saturation_needs_no_more_than_the_bound():
    line = b",".join(b"%d" % (i % 10) for i in range(5001)) + b"\n"   # 5000 separators
    for lst, comp in (("4096", False), ("4097-", False), ("1-4096", False), ("2-", True), ("4097-", True)):
        out, st = both(line * 2, fields=lst, complement=comp)
        cells = line[:-1].split(b",")
        sel = km.Sel(lst, comp)
        want = b",".join(c for k, c in enumerate(cells, 1) if sel(k)) + b"\n"
        assert out == want * 2
    long = bytes(97 + i % 26 for i in range(5000)) + b"\n"
    for lst, comp in (("4096", False), ("4097-", False), ("1-4096", False), ("2-", True)):
        out, _ = both(long, byte_list=lst, complement=comp)
        sel = km.Sel(lst, comp)
        assert out == bytes(b for k, b in enumerate(long[:-1], 1) if sel(k)) + b"\n"


@pytest.mark.skipif(CUT is None, reason="no cut on this machine")
@pytest.mark.parametrize("seed", range(3))
def test_against_gnu_cut(seed):
    plain = km.table(6000, 0x0A, 0x2C, seed)
    assert plain.endswith(b"\n") and all(b"," in ln for ln in plain.split(b"\n")[:-1])
    for lst in LISTS:
        for comp in (False, True):
            extra = ["--complement"] if comp else []
            try:
                km.Sel(lst, comp)
            except km.ListError:
                continue
            assert both(plain, fields=lst, complement=comp)[0] == gnu_cut(plain, "-d,", "-f", lst, *extra), (lst, comp)
            assert both(plain, byte_list=lst, complement=comp)[0] == gnu_cut(plain, "-b", lst, *extra), (lst, comp)


@pytest.mark.skipif(CUT is None, reason="no cut on this machine")
def test_the_two_differences_from_gnu_cut():
    # a line with no separator and field 1 unselected: cut prints it whole, the rule gives an empty line
    plain = b"a,b\nnosep\nc,d\n"
    assert gnu_cut(plain, "-d,", "-f2") == b"b\nnosep\nd\n"
    assert both(plain, fields="2")[0] == b"b\n\nd\n"
    assert gnu_cut(plain, "-d,", "-f1") == both(plain, fields="1")[0] == b"a\nnosep\nc\n"   # (field 1 selected: the same)
    # an unterminated tail: cut adds the delimiter, the rule adds nothing
    assert gnu_cut(b"a,b\nc,d", "-d,", "-f2") == b"b\nd\n"
    assert both(b"a,b\nc,d", fields="2")[0] == b"b\nd"
    assert gnu_cut(b"abc\nde", "-b2") == b"b\ne\n" and both(b"abc\nde", byte_list="2")[0] == b"b\ne"


def test_list_parser():
    for ok in ("1", "4096", "4097-", "-4096", "1-4096", "1,1,1", "7-7"):
        km.Sel(ok)
    for bad, off in (("", 0), ("0", 0), ("1,0", 2), ("5-3", 0), ("4097", 0), ("1-4097", 0), ("4098-", 0), ("1,,2", 2), ("1,", 2),
                     (",1", 0), ("1 2", 1), ("a", 0), ("-", 0), ("1-2-3", 3), ("2-0", 2)):
        with pytest.raises(km.ListError) as e:
            km.Sel(bad)
        assert e.value.offset == off, bad
    with pytest.raises(km.ListError):
        km.Sel("1-", complement=True)
    s = km.Sel("3,5-", False)
    assert s.mn == 3 and s.open_end and s(3) and not s(4) and s(5) and s(100000)
    assert km.Sel("1-4096", True).mn == 4097 and km.Sel("2-", True).mn == 1 and km.Sel("2-", True).open_end
