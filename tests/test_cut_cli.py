"""The command line's cut: --cut-fields LIST / --cut-bytes LIST with --sep, --delim, --complement and --count.  Without a
HIP device an FCX7 file goes through the host decoder (fcx_cli_host.h: host_cut, the rule of fcx_cut.h byte by byte)
and an FCX8 file fails loudly; with one both kinds go through fcx_cut_stream, and the same assertions hold.  The
no-device code and the LIST compiler also run as a stand-alone program under AddressSanitizer and UBSan
(tools/cut_host_check.cpp).

Behind exactly one grep option or --lines the cut is that of the selected blocks' bytes (fcx_cut_ranges_host; on the host
path the same rule over what the grep writes), with no `--` line between blocks.

The expected bytes never come from the code under test: the records are the oracle encoder's, their decoded bytes the
oracle decoder's (Truth of test_gpu_range.py), the blocks context_model's, regex_model's and lines_model's, the cut
cut_model's over them."""
import os
import subprocess
import sys

import pytest

import context_model as cm
import cut_model as km
import find_model as fm
import lines_model as lm
import regex_model as rm
from test_cli import ROOT, gpu_present, run
from test_context_cli import host_compiler
from test_gpu_range import Truth

sys.path.insert(0, os.path.join(ROOT, "tools"))
from cut_host_check import TOTALS   # noqa: E402


@pytest.fixture(scope="module")
def mixed():
    T = Truth("7", fm.mixed_data(), 4096)
    assert T.sizes == [4096, 4096, 0, 0, 0, 4096, 4096, 1808]   # three records in the middle decode to nothing
    return T


def agrees(tmp_path, T, fields=None, byte_list=None, sep=None, delim=None, complement=False, count=False):
    """one run of the command line against the model: the output file's bytes and the totals line"""
    (tmp_path / "in.fcx").write_bytes(T.blob)
    out = tmp_path / "out.txt"
    if out.exists():
        out.unlink()
    args = ["--cut-fields", fields] if fields is not None else ["--cut-bytes", byte_list]
    args += (["--sep", "%02x" % sep] if sep is not None else []) + (["--delim", "%02x" % delim] if delim is not None else [])
    args += (["--complement"] if complement else []) + (["--count"] if count else [])
    r = run(["-i", "in.fcx", "-o", "out.txt"] + args, tmp_path)
    assert r.returncode == 0, r.stdout + r.stderr
    mode, sel = km.make_sel(fields, byte_list, complement)
    want, st = km.cut_np(T.plain, sel, mode, 0x09 if sep is None else sep, 0x0A if delim is None else delim)
    assert [tuple(int(x) for x in t) for t in TOTALS.findall(r.stdout)] == [(st[0], st[2], st[3], st[4], st[1])], r.stdout
    if count:
        assert not out.exists() and r.stdout.count("\n") == 1, r.stdout
    else:
        assert out.read_bytes() == want, args
    return want


def test_the_mixed_file(tmp_path, mixed):
    T = mixed
    assert len(agrees(tmp_path, T, fields="2", sep=0x20)) > 100
    agrees(tmp_path, T, fields="1,3-4", sep=0x20)
    agrees(tmp_path, T, fields="2-", sep=0x20, complement=True)
    agrees(tmp_path, T, fields="3", sep=0x65, delim=0x20)
    agrees(tmp_path, T, fields="40-", sep=0x20, delim=0x00)         # no delimiter in the file: one line over every record
    agrees(tmp_path, T, fields="2")                                 # the default separator, 09: every line is one field
    agrees(tmp_path, T, byte_list="1-16")
    agrees(tmp_path, T, byte_list="3,40-", complement=True, delim=0x2E)
    agrees(tmp_path, T, byte_list="4097-", delim=0x00)
    agrees(tmp_path, T, fields="2", sep=0x20, count=True)
    agrees(tmp_path, T, byte_list="2-3", count=True)


def test_the_two_differences_from_gnu_cut(tmp_path):
    T = Truth("7", b"a,b\nnosep\nc,d", 4096)
    assert agrees(tmp_path, T, fields="2", sep=0x2C) == b"b\n\nd"


def behind(tmp_path, T, select, blocks, cut_args, count=False, **spec):
    """a cut behind a grep or --lines: the model's cut of the join of the model's blocks, no `--` line between them"""
    (tmp_path / "in.fcx").write_bytes(T.blob)
    out = tmp_path / "out.txt"
    if out.exists():
        out.unlink()
    r = run(["-i", "in.fcx", "-o", "out.txt"] + select + cut_args + (["--count"] if count else []), tmp_path)
    assert r.returncode == 0, r.stdout + r.stderr
    mode, sel = km.make_sel(spec.get("fields"), spec.get("byte_list"), spec.get("complement", False))
    want, st = km.cut_np(cm.join(T.plain, blocks), sel, mode, spec.get("sep", 0x09), spec.get("delim", 0x0A))
    assert [tuple(int(x) for x in t) for t in TOTALS.findall(r.stdout)] == [(st[0], st[2], st[3], st[4], st[1])], r.stdout
    if count:
        assert not out.exists()
    else:
        assert out.read_bytes() == want, (select, cut_args)
    return want


CUTS = {"fields": (["--cut-fields", "2-3", "--sep", "20"], {"fields": "2-3", "sep": 0x20}),
        "bytes": (["--cut-bytes", "1-16", "--complement"], {"byte_list": "1-16", "complement": True})}


@pytest.mark.parametrize("which", ["fields", "bytes"])
def test_a_cut_behind_a_grep(tmp_path, mixed, which):
    T, d = mixed, 0x0A
    args, spec = CUTS[which]
    word = T.plain[9000:9003]
    assert bytes([d]) not in word
    (tmp_path / "pats").write_bytes(word + b"\nthe\n")
    plain = cm.blocks(T.plain, [word], d)
    assert len(behind(tmp_path, T, ["--grep", word.decode()], plain, args, **spec)) > 0
    ctx = cm.blocks(T.plain, [word], d, False, False, 1, 2)
    assert len(ctx) > 1
    behind(tmp_path, T, ["--grep", word.decode(), "--before", "1", "--after", "2"], ctx, args, **spec)   # no `--` line
    behind(tmp_path, T, ["--grep-regex", "[a-z]+\\.$", "--context", "1"], rm.blocks(T.plain, rm.Nfa(b"[a-z]+\\.$", d), False, 1, 1), args, **spec)
    if which == "fields":
        behind(tmp_path, T, ["--grep-hex", word.hex()], plain, args, count=True, **spec)
        behind(tmp_path, T, ["--grep-set", "pats"], cm.blocks(T.plain, [word, b"the"], d), args, **spec)
        behind(tmp_path, T, ["--grep", word.decode(), "--invert"], cm.blocks(T.plain, [word], d, False, True), args, **spec)
        behind(tmp_path, T, ["--grep", "zzzzq"], [], args, **spec)                                        # nothing selected


def test_a_cut_behind_lines(tmp_path, mixed):
    T, d = mixed, 0x0A
    off, n = lm.locate(T.plain, d, 2, 5)
    for which in ("fields", "bytes"):
        args, spec = CUTS[which]
        behind(tmp_path, T, ["--lines", "3:5"], [(off, off + n)], args, count=which == "bytes", **spec)
    args, spec = CUTS["fields"]
    off, n = lm.locate(T.plain, d, 10 ** 6, 5)
    behind(tmp_path, T, ["--lines", "1000001:5"], [(off, off + n)], args, **spec)                             # behind the last line


def test_fcx8_needs_a_device(tmp_path):
    T = Truth("8", fm.text(7, 9000), 4096)
    (tmp_path / "in.fcx").write_bytes(T.blob)
    r = run(["-i", "in.fcx", "-o", "out.txt", "--cut-fields", "2", "--sep", "20"], tmp_path)
    if gpu_present():
        assert r.returncode == 0, r.stdout + r.stderr
        assert (tmp_path / "out.txt").read_bytes() == km.cut_np(T.plain, km.Sel("2"), km.FIELDS, 0x20, 0x0A)[0]
    else:
        assert r.returncode not in (0, 1) and ("HIP" in r.stderr or "GPU" in r.stderr), r.stderr
        assert "cut:" not in r.stdout


USAGE = [
    ("both cut options", ["--cut-fields", "1", "--cut-bytes", "2"], None),
    ("a cut option twice", ["--cut-fields", "1", "--cut-fields", "2"], None),
    ("an empty list", ["--cut-fields", ""], "offset 0"),
    ("a zero", ["--cut-bytes", "1,0"], "offset 2"),
    ("a descending range", ["--cut-fields", "1,5-3"], "offset 2"),
    ("a number above the maximum", ["--cut-fields", "4097"], "offset 0"),
    ("another byte", ["--cut-bytes", "1 2"], "offset 1"),
    ("the complement of everything", ["--cut-fields", "1-", "--complement"], "offset 0"),
    ("a separator that is the delimiter", ["--cut-fields", "1", "--sep", "0a"], "separator"),
    ("a separator that is the given delimiter", ["--cut-fields", "1", "--sep", "20", "--delim", "20"], "separator"),
    ("a separator of three digits", ["--cut-fields", "1", "--sep", "020"], None),
    ("--sep without a cut option", ["--sep", "20"], None),
    ("--sep with --cut-bytes", ["--cut-bytes", "1", "--sep", "20"], None),
    ("--complement without a cut option", ["--complement"], None),
    ("a cut with -c", ["-c", "lz77", "--cut-fields", "1"], None),
    ("a cut with --range", ["--cut-fields", "1", "--range", "0:5"], None),
    ("a cut with --list", ["--cut-bytes", "1", "--list"], None),
    ("a cut with --find", ["--cut-fields", "1", "--find", "ab"], None),
    ("a cut with --find-set", ["--cut-fields", "1", "--find-set", "pats"], None),
    ("a cut with --count-lines", ["--cut-fields", "1", "--count-lines"], None),
    ("a cut with a grep and --lines", ["--cut-fields", "1", "--grep", "ab", "--lines", "1:2"], None),
    ("a cut with two greps", ["--cut-fields", "1", "--grep", "ab", "--grep-regex", "cd"], None),
    ("a cut with --line-numbers", ["--cut-fields", "1", "--find", "ab", "--line-numbers"], None),
    ("a cut with --compare", ["--cut-fields", "1", "--compare", "in.fcx"], None),
    ("a cut with --verify", ["--cut-fields", "1", "--verify"], None),
    ("a cut with --repair", ["--cut-fields", "1", "--repair", "side"], None),
    ("a cut with --digest", ["--cut-fields", "1", "--digest", "dig"], None),
    ("a cut with --test", ["--cut-fields", "1", "--digest", "dig", "--test"], None),
]


@pytest.mark.parametrize("what,extra,says", USAGE, ids=[c[0] for c in USAGE])
def test_usage_errors(tmp_path, mixed, what, extra, says):
    (tmp_path / "in.fcx").write_bytes(mixed.blob)
    (tmp_path / "pats").write_bytes(b"ab\ncd\n")
    r = run(["-i", "in.fcx", "-o", "x"] + extra, tmp_path)
    assert r.returncode not in (0, 1) and "usage:" in r.stderr, r.stdout + r.stderr
    assert says is None or ("--cut-" in r.stderr and says in r.stderr.split("usage:")[0]), r.stderr
    assert "cut:" not in r.stdout
    assert not (tmp_path / "x").exists()


def test_the_host_path_and_the_compiler_under_the_sanitizers(tmp_path):
    """tools/cut_host_check.py: the stand-alone program, one process per case, against the model"""
    cc = host_compiler()
    assert cc, "no C++ compiler: the library itself could not have been built"
    exe = tmp_path / "cut_host_check"
    src = [os.path.join(ROOT, "tools", "cut_host_check.cpp"), os.path.join(ROOT, "my_compress_amd", "csrc", "fcx_decode.cpp")]
    cmd = cc + ["-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
                "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "my_compress_amd", "csrc")] + src + ["-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "cut_host_check.py"), str(exe), str(tmp_path)], capture_output=True,
                       text=True, timeout=600, env=env)
    assert r.returncode == 0 and "runs agree with the model, no sanitizer report" in r.stdout, r.stdout + r.stderr


@pytest.mark.gpu
def test_gpu_cut_both_kinds(tmp_path, mixed, cuda):
    agrees(tmp_path, mixed, fields="2-3", sep=0x20)
    agrees(tmp_path, mixed, byte_list="1-16", complement=True, count=True)
    T = Truth("8", fm.text(11, 300 * 256), 256)   # more records than one stream group
    agrees(tmp_path, T, fields="2", sep=0x20)
    agrees(tmp_path, T, byte_list="5-", delim=0x20)
    word = T.plain[70000:70003]
    assert b"\n" not in word
    blk = cm.blocks(T.plain, [word], 0x0A, False, False, 1, 1)
    behind(tmp_path, T, ["--grep", word.decode(), "--context", "1"], blk, ["--cut-fields", "2-", "--sep", "20"], fields="2-", sep=0x20)
    off, n = lm.locate(T.plain, 0x0A, 4, 300)
    behind(tmp_path, T, ["--lines", "5:300"], [(off, off + n)], ["--cut-bytes", "3-9"], count=True, byte_list="3-9")
