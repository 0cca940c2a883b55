"""The command line's context and inverted grep: --invert, --before N, --after N, --context N with --grep, --grep-hex or
--grep-set, combined with --ignore-case, --delim and --count.  Without a HIP device an FCX7 file goes through the host
decoder (fcx_cli_host.h: host_grep_blocks) and an FCX8 file fails loudly; with one both kinds go through
fcx_grep_blocks_stream and fcx_decompress_ranges_stream, and the same assertions hold.  The no-device code also runs as
a stand-alone program under AddressSanitizer and UBSan (tools/context_host_check.cpp).

The expected bytes never come from the code under test: the records are the oracle encoder's, their decoded bytes the
oracle decoder's (Truth of test_gpu_range.py), the blocks context_model's over them, with GNU grep's `--` line between
two blocks when a context is asked for."""
import os
import shutil
import subprocess

import pytest

import context_model as cm
import find_model as fm
import grep_model as gm
import set_model as sm
from test_cli import ROOT, gpu_present, run
from test_gpu_range import Truth


@pytest.fixture(scope="module")
def crafted():
    T = Truth("7", sm.crafted(0x0A), sm.BLOCK)
    sm.check_crafted(T.plain, 0x0A)
    return T


@pytest.fixture(scope="module")
def mixed():
    T = Truth("7", fm.mixed_data(), 4096)
    assert T.sizes == [4096, 4096, 0, 0, 0, 4096, 4096, 1808]   # three records in the middle decode to nothing
    return T


def options(invert, before, after, fold=False, count=False, delim=None):
    a = (["--invert"] if invert else []) + (["--ignore-case"] if fold else []) + (["--count"] if count else [])
    if before == after and before:
        a += ["--context", str(before)]
    else:
        a += (["--before", str(before)] if before else []) + (["--after", str(after)] if after else [])
    return a + (["--delim", "%02x" % delim] if delim is not None else [])


def agrees(tmp_path, T, pats, how: str, invert=False, before=0, after=0, fold=False, count=False, delim=None):
    """one run of the command line against the model: the output file's bytes and the totals line"""
    d = 0x0A if delim is None else delim
    (tmp_path / "in.fcx").write_bytes(T.blob)
    out = tmp_path / "out.txt"
    if out.exists():
        out.unlink()
    if how == "--grep-set":
        (tmp_path / "pats").write_bytes(b"".join(p.hex().encode() + b"\n" for p in pats))
        what = ["--grep-set", "pats", "--set-hex"]
    else:
        what = [how, pats[0].hex() if how == "--grep-hex" else pats[0].decode()]
    r = run(["-i", "in.fcx", "-o", "out.txt"] + what + options(invert, before, after, fold, count, delim), tmp_path)
    assert r.returncode == 0, r.stdout + r.stderr
    blk = cm.blocks(T.plain, pats, d, fold, invert, before, after)
    st = cm.stats(T.plain, pats, d, fold, invert, before, after, blk)
    assert [tuple(int(x) for x in t) for t in cm.TOTALS.findall(r.stdout)] == [(st[0], st[1], st[3], st[2], st[4], st[6])], r.stdout
    if count:
        assert not out.exists() and r.stdout.count("\n") == 1, r.stdout
    else:
        assert out.read_bytes() == cm.join(T.plain, blk, cm.separator(d, before, after)), (pats, invert, before, after)
    return blk


def test_the_crafted_file(tmp_path, crafted):
    T = crafted
    blk = agrees(tmp_path, T, [gm.MARK], "--grep-hex", before=1, after=1)
    assert len(blk) > 1                                        # `--` lines are written
    agrees(tmp_path, T, [gm.MARK], "--grep-hex", invert=True)  # no context: nothing between the blocks
    agrees(tmp_path, T, [gm.MARK], "--grep-hex", invert=True, before=2, after=1)
    agrees(tmp_path, T, [gm.MARK], "--grep-hex", after=3)      # into the unterminated tail
    agrees(tmp_path, T, [gm.MARK], "--grep-hex", before=7)
    agrees(tmp_path, T, [gm.MARK], "--grep-hex", before=4096, after=4096)
    agrees(tmp_path, T, [sm.SHORT1, sm.SHORT3, gm.MARK], "--grep-set", invert=True, before=1, count=True)
    agrees(tmp_path, T, [sm.UP], "--grep", fold=True, before=1, after=2)
    agrees(tmp_path, T, [sm.UP], "--grep", fold=True, invert=True, count=True)


def test_other_delimiters_and_records_of_no_bytes(tmp_path, mixed):
    T = mixed
    word = next(w for w in T.plain[:4000].split(b" ") if len(w) >= 4 and w.isalpha())
    across = gm.cut(T.plain, 0x0A, 8189, 7)     # in the line across the three records that decode to nothing
    agrees(tmp_path, T, [across], "--grep-hex", before=1, after=1)
    agrees(tmp_path, T, [across, fm.absent(T.plain)], "--grep-set", invert=True, after=2)
    agrees(tmp_path, T, [word], "--grep", delim=0x20, before=2, after=2)
    agrees(tmp_path, T, [word.upper()], "--grep", delim=0x20, fold=True, invert=True, before=1, count=True)
    agrees(tmp_path, T, [fm.absent(T.plain)], "--grep-hex", before=3, after=3)   # no hit: no block, an empty file
    agrees(tmp_path, T, [fm.absent(T.plain)], "--grep-hex", invert=True)         # one block: the whole file


def test_without_the_options_the_grep_is_the_old_one(tmp_path, crafted):
    (tmp_path / "in.fcx").write_bytes(crafted.blob)
    r = run(["-i", "in.fcx", "-o", "out.txt", "--grep-hex", gm.MARK.hex()], tmp_path)
    assert r.returncode == 0 and gm.TOTALS.findall(r.stdout) and "blocks" not in r.stdout
    assert (tmp_path / "out.txt").read_bytes() == gm.join(crafted.plain, gm.selected(crafted.plain, gm.MARK, 0x0A))


def test_fcx8_needs_a_device(tmp_path):
    T = Truth("8", gm.crafted(0x0A), gm.CRAFT_BLOCK)
    (tmp_path / "in.fcx").write_bytes(T.blob)
    r = run(["-i", "in.fcx", "-o", "out.txt", "--grep-hex", gm.MARK.hex(), "--invert", "--context", "1"], tmp_path)
    if gpu_present():
        assert r.returncode == 0, r.stdout + r.stderr
    else:
        assert r.returncode not in (0, 1) and ("HIP" in r.stderr or "GPU" in r.stderr), r.stderr
        assert "grep:" not in r.stdout


USAGE = [
    ("a value that is not a number", ["--grep", "ab", "--before", "x"]),
    ("a value with a sign", ["--grep", "ab", "--after", "-1"]),
    ("a value with a tail", ["--grep", "ab", "--context", "3x"]),
    ("an empty value", ["--grep", "ab", "--context", ""]),
    ("a value above 4096", ["--grep", "ab", "--before", "4097"]),
    ("a huge value", ["--grep", "ab", "--after", "99999999999999999999"]),
    ("--context above 4096", ["--grep-hex", "6162", "--context", "5000"]),
    ("--invert without a grep", ["--invert"]),
    ("--before with --find", ["--find", "ab", "--before", "1"]),
    ("--after with --find-set", ["--find-set", "pats", "--after", "1"]),
    ("--context with --count-lines", ["--count-lines", "--context", "1"]),
    ("--invert with --lines", ["--lines", "0:1", "--invert"]),
    ("--invert with -c", ["-c", "lz77", "--invert"]),
    ("a pattern with the delimiter", ["--grep", "a b", "--delim", "20", "--invert"]),
    ("a folded pattern with the folded delimiter", ["--grep", "xay", "--delim", "41", "--ignore-case", "--after", "1"]),
    ("--invert with --grep and --find", ["--grep", "ab", "--find", "cd", "--invert"]),
]


@pytest.mark.parametrize("what,extra", USAGE, ids=[c[0] for c in USAGE])
def test_usage_errors(tmp_path, crafted, what, extra):
    (tmp_path / "in.fcx").write_bytes(crafted.blob)
    (tmp_path / "pats").write_bytes(b"ab\ncd\n")
    r = run(["-i", "in.fcx", "-o", "x"] + extra, tmp_path)
    assert r.returncode not in (0, 1) and "usage:" in r.stderr, r.stdout + r.stderr
    assert "grep:" not in r.stdout and "find:" not in r.stdout
    assert not (tmp_path / "x").exists()


def test_the_largest_context_is_accepted(tmp_path, crafted):
    (tmp_path / "in.fcx").write_bytes(crafted.blob)
    r = run(["-i", "in.fcx", "--grep-hex", gm.MARK.hex(), "--context", "4096", "--count"], tmp_path)
    assert r.returncode == 0 and cm.TOTALS.findall(r.stdout), r.stdout + r.stderr


# ---- the no-device code as a stand-alone program under the sanitizers ----
def host_compiler():
    for name in ("c++", "g++", "clang++"):
        if shutil.which(name):
            return [shutil.which(name)]
    hipcc = os.environ.get("HIPCC") or os.path.join(os.environ.get("ROCM", "/opt/rocm"), "bin", "hipcc")
    return [hipcc] if os.path.exists(hipcc) else None


@pytest.fixture(scope="module")
def host_check(tmp_path_factory):
    cc = host_compiler()
    assert cc, "no C++ compiler: the library itself could not have been built"
    exe = tmp_path_factory.mktemp("host_check") / "context_host_check"
    src = [os.path.join(ROOT, "tools", "context_host_check.cpp"), os.path.join(ROOT, "my_compress_amd", "csrc", "fcx_decode.cpp")]
    cmd = cc + ["-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
                "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "my_compress_amd", "csrc")] + src + ["-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    return str(exe)


def check_run(exe, cwd, args):
    return subprocess.run([exe] + args, cwd=cwd, capture_output=True, text=True, timeout=600,
                          env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1"))


def test_the_host_path_under_the_sanitizers(tmp_path, crafted, mixed, host_check):
    clean = lambda r: "Sanitizer" not in r.stderr and "runtime error" not in r.stderr
    for T, pats, flags, d, before, after in (
        (crafted, [gm.MARK], "x", 0x0A, 1, 1),
        (crafted, [gm.MARK], "xv", 0x0A, 2, 1),
        (crafted, [gm.MARK], "x", 0x0A, 4096, 4096),
        (crafted, [sm.SHORT1, sm.SHORT3, sm.UP], "xiv", 0x0A, 0, 3),
        (mixed, [gm.cut(mixed.plain, 0x0A, 8189, 7)], "xv", 0x0A, 7, 0),
        (mixed, [fm.absent(mixed.plain)], "x", 0x20, 3, 3),
        (mixed, [fm.absent(mixed.plain)], "xv", 0x20, 0, 0),
    ):
        (tmp_path / "in.fcx").write_bytes(T.blob)
        (tmp_path / "pats").write_bytes(b"".join(p.hex().encode() + b"\n" for p in pats))
        r = check_run(host_check, tmp_path, ["in.fcx", "pats", flags, "%02x" % d, str(before), str(after), "out.txt"])
        assert r.returncode == 0 and clean(r), r.stdout + r.stderr
        fold, invert = "i" in flags, "v" in flags
        blk = cm.blocks(T.plain, pats, d, fold, invert, before, after)
        st = cm.stats(T.plain, pats, d, fold, invert, before, after, blk)
        assert (tmp_path / "out.txt").read_bytes() == cm.join(T.plain, blk, cm.separator(d, before, after))
        assert [tuple(int(x) for x in t) for t in cm.TOTALS.findall(r.stdout)] == [(st[0], st[1], st[3], st[2], st[4], st[6])]
        assert r.stdout.splitlines()[-1] == "counts: " + " ".join(str(c) for c in sm.counts(T.plain, pats, fold))
    # what the parsers refuse, and a damaged record: clean exits, no report
    (tmp_path / "in.fcx").write_bytes(crafted.blob)
    (tmp_path / "pats").write_bytes(gm.MARK.hex().encode() + b"\n")
    for args in (["in.fcx", "pats", "x", "0a", "4097", "0"], ["in.fcx", "pats", "x", "0a", "1", "z"], ["in.fcx", "pats", "x", "11", "1", "1"],
                 ["in.fcx", "pats", "x", "0a", "1"], ["nothing-here", "pats", "x", "0a", "1", "1"]):
        r = check_run(host_check, tmp_path, args)
        assert r.returncode == 2 and clean(r), (args, r.stdout + r.stderr)
    blob = bytearray(crafted.blob)
    a, b = 10 + crafted.rec_off[2] + 4, 10 + crafted.rec_off[3]
    blob[a:b] = b"\xFF" * (b - a)   # the third record's payload, its length prefix kept
    (tmp_path / "bad.fcx").write_bytes(bytes(blob))
    r = check_run(host_check, tmp_path, ["bad.fcx", "pats", "xv", "0a", "2", "2", "out.txt"])
    assert r.returncode == 1 and clean(r) and "grep:" not in r.stdout, r.stdout + r.stderr
    (tmp_path / "cut.fcx").write_bytes(crafted.blob[:-7])
    r = check_run(host_check, tmp_path, ["cut.fcx", "pats", "x", "0a", "2", "2"])
    assert r.returncode == 1 and clean(r), r.stdout + r.stderr


@pytest.mark.gpu
def test_gpu_context_both_kinds(tmp_path, crafted, cuda):
    agrees(tmp_path, crafted, [gm.MARK], "--grep-hex", invert=True, before=2, after=1)
    agrees(tmp_path, crafted, [sm.SHORT1, sm.SHORT3, gm.MARK], "--grep-set", before=1, after=1)
    agrees(tmp_path, crafted, [sm.UP], "--grep", fold=True, invert=True, count=True)
    T = Truth("8", gm.crafted(0xFF), gm.CRAFT_BLOCK)
    agrees(tmp_path, T, [gm.MARK], "--grep-hex", delim=0xFF, invert=True, after=3)
    agrees(tmp_path, T, [gm.MARK], "--grep-hex", delim=0xFF, before=7, after=1)
    agrees(tmp_path, T, [gm.MARK], "--grep-hex", delim=0xFF, before=4096, after=4096, count=True)
