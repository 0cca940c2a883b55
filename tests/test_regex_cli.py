"""The command line's regex grep: --grep-regex EXPR with --count, --delim, --ignore-case, --invert, --before, --after and
--context.  Without a HIP device an FCX7 file goes through the host decoder (fcx_cli_host.h: host_grep_regex, the
compiled table run byte by byte) and an FCX8 file fails loudly; with one both kinds go through
fcx_grep_regex_blocks_stream and fcx_decompress_ranges_stream, and the same assertions hold.  The no-device code and
the compiler also run as a stand-alone program under AddressSanitizer and UBSan (tools/regex_host_check.cpp).

The expected bytes never come from the code under test: the records are the oracle encoder's, their decoded bytes the
oracle decoder's (Truth of test_gpu_range.py), the blocks regex_model's over them, with GNU grep's `--` line between
two blocks when a context is asked for."""
import os
import subprocess
import sys

import pytest

import context_model as cm
import find_model as fm
import regex_model as rm
import set_model as sm
from test_cli import ROOT, gpu_present, run
from test_context_cli import host_compiler, options
from test_gpu_range import Truth


@pytest.fixture(scope="module")
def crafted():
    T = Truth("7", rm.crafted(0x0A), rm.BLOCK)
    rm.check_crafted(T.plain, 0x0A)
    return T


@pytest.fixture(scope="module")
def mixed():
    T = Truth("7", fm.mixed_data(), 4096)
    assert T.sizes == [4096, 4096, 0, 0, 0, 4096, 4096, 1808]   # three records in the middle decode to nothing
    return T


def agrees(tmp_path, T, expr: bytes, invert=False, before=0, after=0, fold=False, count=False, delim=None):
    """one run of the command line against the model: the output file's bytes and the totals line"""
    d = 0x0A if delim is None else delim
    (tmp_path / "in.fcx").write_bytes(T.blob)
    out = tmp_path / "out.txt"
    if out.exists():
        out.unlink()
    r = run(["-i", "in.fcx", "-o", "out.txt", "--grep-regex", expr.decode()] + options(invert, before, after, fold, count, delim), tmp_path)
    assert r.returncode == 0, r.stdout + r.stderr
    nfa = rm.Nfa(expr, d, fold)
    blk = rm.blocks(T.plain, nfa, invert, before, after)
    st = rm.stats(T.plain, nfa, invert, before, after, blk)
    if invert or before or after:
        assert [tuple(int(x) for x in t) for t in cm.TOTALS.findall(r.stdout)] == [(st[0], st[1], st[3], st[2], st[4], st[6])], r.stdout
    else:   # the set grep's line: lines, bytes, hits, decoded bytes, patterns
        assert [tuple(int(x) for x in t) for t in sm.GREP_TOTALS.findall(r.stdout)] == [(st[1], st[2], st[4], st[6], 1)], r.stdout
    if count:
        assert not out.exists() and r.stdout.count("\n") == 1, r.stdout
    else:
        assert out.read_bytes() == cm.join(T.plain, blk, cm.separator(d, before, after)), (expr, invert, before, after)
    return blk


def test_the_crafted_file(tmp_path, crafted):
    T = crafted
    for expr in rm.CRAFT_EXPRS:
        agrees(tmp_path, T, expr)
    assert len(agrees(tmp_path, T, rm.E_ANY, before=1, after=1)) > 1   # `--` lines are written
    agrees(tmp_path, T, rm.E_EOL, invert=True)
    agrees(tmp_path, T, rm.E_MIX, invert=True, before=2, after=1)
    agrees(tmp_path, T, rm.E_EOL, after=3)                             # from the unterminated tail's match backwards: none behind it
    agrees(tmp_path, T, rm.E_BOL, before=4096, after=4096)
    agrees(tmp_path, T, rm.E_FAR, count=True)
    agrees(tmp_path, T, b"A[^B]{3}b|THE ", fold=True, before=1, after=2)
    agrees(tmp_path, T, b"A[^B]{3}b|THE ", fold=True, invert=True, count=True)
    agrees(tmp_path, T, b"A[^B]{3}b|THE ", count=True)


def test_other_delimiters_and_records_of_no_bytes(tmp_path, mixed):
    T = mixed
    agrees(tmp_path, T, b"[a-z]+\\.$", before=1, after=1)
    agrees(tmp_path, T, b"^[A-Z][a-z]* ", invert=True, after=2)
    agrees(tmp_path, T, b"^the$|^and$", delim=0x20, before=2, after=2)
    agrees(tmp_path, T, b"^THE$|^aNd$", delim=0x20, fold=True, invert=True, before=1, count=True)
    agrees(tmp_path, T, b"e[^a]", delim=0x65 ^ 0x20)                     # d = E: the negated set leaves it out
    agrees(tmp_path, T, b"zzzzq", before=3, after=3)                     # no hit: no block, an empty file
    agrees(tmp_path, T, b"zzzzq", invert=True)                           # one block: the whole file


def test_fcx8_needs_a_device(tmp_path):
    T = Truth("8", rm.crafted(0x0A), rm.BLOCK)
    (tmp_path / "in.fcx").write_bytes(T.blob)
    r = run(["-i", "in.fcx", "-o", "out.txt", "--grep-regex", rm.E_MIX.decode(), "--context", "1"], tmp_path)
    if gpu_present():
        assert r.returncode == 0, r.stdout + r.stderr
        blk = rm.blocks(T.plain, rm.Nfa(rm.E_MIX), False, 1, 1)
        assert (tmp_path / "out.txt").read_bytes() == cm.join(T.plain, blk, b"--\n")
    else:
        assert r.returncode not in (0, 1) and ("HIP" in r.stderr or "GPU" in r.stderr), r.stderr
        assert "grep:" not in r.stdout


USAGE = [
    ("an expression that matches the empty string", ["--grep-regex", "a*"], "empty string"),
    ("an anchor inside a group", ["--grep-regex", "ab(^c)"], "offset 3"),
    ("a back-reference", ["--grep-regex", "(a)\\1"], "offset 3"),
    ("a word boundary", ["--grep-regex", "\\bfoo"], "offset 0"),
    ("an empty alternative", ["--grep-regex", "ab|"], "offset 3"),
    ("an unmatched bracket", ["--grep-regex", "x[a-z"], "offset 1"),
    ("the delimiter as a literal", ["--grep-regex", "a b", "--delim", "20"], "offset 1"),
    ("a folded literal that is the folded delimiter", ["--grep-regex", "xay", "--delim", "41", "--ignore-case"], "offset 1"),
    ("more than 64 states", ["--grep-regex", "^a{62}b"], "64 states"),
    ("an empty expression", ["--grep-regex", ""], "length"),
    ("--grep-regex twice", ["--grep-regex", "ab", "--grep-regex", "cd"], None),
    ("--grep-regex with --grep", ["--grep-regex", "ab", "--grep", "cd"], None),
    ("--grep-regex with --grep-set", ["--grep-regex", "ab", "--grep-set", "pats"], None),
    ("--grep-regex with --find", ["--grep-regex", "ab", "--find", "cd"], None),
    ("--grep-regex with --line-numbers", ["--grep-regex", "ab", "--line-numbers"], None),
    ("--grep-regex with --set-hex", ["--grep-regex", "ab", "--set-hex"], None),
    ("--grep-regex with -c", ["-c", "lz77", "--grep-regex", "ab"], None),
    ("--grep-regex with --count-lines", ["--grep-regex", "ab", "--count-lines"], None),
    ("a context above 4096", ["--grep-regex", "ab", "--before", "4097"], None),
]


@pytest.mark.parametrize("what,extra,says", USAGE, ids=[c[0] for c in USAGE])
def test_usage_errors(tmp_path, crafted, what, extra, says):
    (tmp_path / "in.fcx").write_bytes(crafted.blob)
    (tmp_path / "pats").write_bytes(b"ab\ncd\n")
    r = run(["-i", "in.fcx", "-o", "x"] + extra, tmp_path)
    assert r.returncode not in (0, 1) and "usage:" in r.stderr, r.stdout + r.stderr
    assert says is None or ("--grep-regex: " in r.stderr and says in r.stderr.split("usage:")[0]), r.stderr
    assert "grep:" not in r.stdout and "find:" not in r.stdout
    assert not (tmp_path / "x").exists()


def test_the_host_path_and_the_compiler_under_the_sanitizers(tmp_path):
    """tools/regex_host_check.py: the stand-alone program, one process per case, against the model"""
    cc = host_compiler()
    assert cc, "no C++ compiler: the library itself could not have been built"
    exe = tmp_path / "regex_host_check"
    src = [os.path.join(ROOT, "tools", "regex_host_check.cpp"), os.path.join(ROOT, "my_compress_amd", "csrc", "fcx_decode.cpp")]
    cmd = cc + ["-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
                "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "my_compress_amd", "csrc")] + src + ["-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "regex_host_check.py"), str(exe), str(tmp_path)], capture_output=True,
                       text=True, timeout=600, env=env)
    assert r.returncode == 0 and "runs agree with the model, no sanitizer report" in r.stdout, r.stdout + r.stderr


@pytest.mark.gpu
def test_gpu_regex_both_kinds(tmp_path, crafted, cuda):
    agrees(tmp_path, crafted, rm.E_MIX, invert=True, before=2, after=1)
    agrees(tmp_path, crafted, rm.E_FAR)
    agrees(tmp_path, crafted, b"A[^B]{3}b|THE ", fold=True, invert=True, count=True)
    T = Truth("8", rm.crafted(0x41), rm.BLOCK)
    agrees(tmp_path, T, rm.E_EOL, delim=0x41, invert=True, after=3)
    agrees(tmp_path, T, rm.E_ANY, delim=0x41, before=7, after=1)
    agrees(tmp_path, T, rm.E_64, delim=0x41, before=4096, after=4096, count=True)
