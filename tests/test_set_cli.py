"""The command line's pattern sets: --find-set FILE, --grep-set FILE, --set-hex, --ignore-case, with --count and
--delim, in the decompress mode.  Without a HIP device an FCX7 file goes through the host decoder (fcx_cli_host.h:
host_find_set, host_grep_set) and an FCX8 file fails loudly; with one both kinds go through fcx_find_set_stream
and fcx_grep_set_stream, and the same assertions hold.

The expected bytes never come from the code under test: the records are the oracle encoder's, their decoded bytes
the oracle decoder's (Truth of test_gpu_range.py), hits and lines set_model's over them."""
import pytest

import find_model as fm
import grep_model as gm
import set_model as sm
from test_cli import gpu_present, run
from test_gpu_range import Truth

SIZES = [4096, 4096, 0, 0, 0, 4096, 4096, 1808]


@pytest.fixture(scope="module")
def mixed():
    T = Truth("7", fm.mixed_data(), 4096)
    assert T.sizes == SIZES
    return T


def pattern_file(tmp_path, pats, hexed: bool, trailing: bool = True) -> str:
    sep = b"\n"
    body = sep.join(p.hex().encode() if hexed else p for p in pats) + (sep if trailing else b"")
    (tmp_path / "pats").write_bytes(body)
    return "pats"


def call(tmp_path, blob: bytes, opt: str, pats, hexed=True, fold=False, count=False, delim=None, trailing=True):
    (tmp_path / "in.fcx").write_bytes(blob)
    out = tmp_path / "out.txt"
    if out.exists():
        out.unlink()
    args = ["-i", "in.fcx", "-o", "out.txt", opt, pattern_file(tmp_path, pats, hexed, trailing)]
    args += (["--set-hex"] if hexed else []) + (["--ignore-case"] if fold else []) + (["--count"] if count else [])
    args += ["--delim", "%02x" % delim] if delim is not None else []
    return run(args, tmp_path), out.read_bytes() if out.exists() else None


def find_agrees(tmp_path, T, pats, hexed=True, fold=False, count=False, trailing=True):
    r, out = call(tmp_path, T.blob, "--find-set", pats, hexed, fold, count, None, trailing)
    assert r.returncode == 0 and out is None, r.stdout + r.stderr
    want = sm.hits_any(T.plain, pats, fold)
    assert [int(x) for x in fm.LINE.findall(r.stdout)] == ([] if count else want), (pats, fold)
    assert [tuple(int(x) for x in t) for t in sm.FIND_TOTALS.findall(r.stdout)] == [(len(want), T.total, len(pats))], r.stdout
    assert r.stdout.rstrip().splitlines()[-1].startswith("find: %d hits" % len(want))
    return want


def grep_agrees(tmp_path, T, pats, hexed=True, fold=False, count=False, delim=None):
    d = 0x0A if delim is None else delim
    r, out = call(tmp_path, T.blob, "--grep-set", pats, hexed, fold, count, delim)
    assert r.returncode == 0, r.stdout + r.stderr
    want = sm.selected_any(T.plain, pats, d, fold)
    st = sm.grep_stats(T.plain, pats, d, fold, want)
    assert [tuple(int(x) for x in t) for t in sm.GREP_TOTALS.findall(r.stdout)] == [(st[0], st[1], st[2], st[4], len(pats))], r.stdout
    assert out == (None if count else gm.join(T.plain, want)), (pats, fold, count)
    return want


def mixed_sets(T):
    plain = T.plain
    words = [w for w in plain[:4000].split(b" ") if len(w) >= 4 and w.isalpha()][:5]
    across = gm.cut(plain, 0x0A, 8189, 7)     # in the line across the three records that decode to nothing
    tail = gm.cut(plain, 0x0A, T.total - 3, 3)
    return words, [across, tail, plain[100:101], fm.absent(plain)], [w.upper() for w in words[:2]] + [words[2].swapcase()]


def check_mixed(tmp_path, T):
    words, edges, upper = mixed_sets(T)
    assert sm.hits_any(T.plain, upper, False) != sm.hits_any(T.plain, upper, True)
    # (a run is a process, so they are few)
    find_agrees(tmp_path, T, words, hexed=False, trailing=False)
    find_agrees(tmp_path, T, edges, count=True)
    find_agrees(tmp_path, T, upper, hexed=False, fold=False)
    find_agrees(tmp_path, T, upper, hexed=False, fold=True)
    grep_agrees(tmp_path, T, edges)
    grep_agrees(tmp_path, T, upper, hexed=False, fold=True)
    grep_agrees(tmp_path, T, upper, fold=False, count=True)
    grep_agrees(tmp_path, T, [w for w in words if b" " not in w], hexed=False, delim=0x20)


def test_the_set_options_on_the_mixed_file(tmp_path, mixed):
    check_mixed(tmp_path, mixed)


def test_ignore_case_with_the_one_pattern_options(tmp_path, mixed):
    T = mixed
    word = mixed_sets(T)[0][0]
    (tmp_path / "in.fcx").write_bytes(T.blob)
    r = run(["-i", "in.fcx", "--find", word.upper().decode(), "--ignore-case", "--count"], tmp_path)
    want = sm.hits_any(T.plain, [word.upper()], True)
    assert want and r.returncode == 0, r.stdout + r.stderr
    assert [tuple(int(x) for x in t) for t in sm.FIND_TOTALS.findall(r.stdout)] == [(len(want), T.total, 1)]
    r = run(["-i", "in.fcx", "-o", "out.txt", "--grep-hex", word.upper().hex(), "--ignore-case"], tmp_path)
    sel = sm.selected_any(T.plain, [word.upper()], 0x0A, True)
    assert r.returncode == 0 and (tmp_path / "out.txt").read_bytes() == gm.join(T.plain, sel), r.stdout + r.stderr
    # without the flag the old options print the old totals
    r = run(["-i", "in.fcx", "--find", word.decode(), "--count"], tmp_path)
    assert fm.TOTALS.findall(r.stdout) and "patterns" not in r.stdout


def tail_file():
    t = bytearray(fm.text(7, 12288)[:10001])
    t[4095] = t[8191] = t[10000] = 0
    return Truth("8", bytes(t), 4096)


def test_fcx8_needs_a_device(tmp_path):
    T = tail_file()
    pats = [gm.cut(T.plain, 0x0A, 4090, 10), T.plain[:1]]
    for opt in ("--find-set", "--grep-set"):
        r, out = call(tmp_path, T.blob, opt, pats)
        if gpu_present():
            assert r.returncode == 0, r.stdout + r.stderr
        else:
            assert r.returncode not in (0, 1) and ("HIP" in r.stderr or "GPU" in r.stderr), r.stderr
            assert "find:" not in r.stdout and "grep:" not in r.stdout


def usage_cases():
    ok = b"ab\ncd\n"
    many = b"".join(b"p%02d\n" % i for i in range(65))
    return [
        ("an empty pattern line", b"ab\n\ncd\n", ["--find-set", "pats"]),
        ("two trailing line ends", b"ab\n\n", ["--grep-set", "pats"]),
        ("an empty file", b"", ["--find-set", "pats"]),
        ("65 patterns", many, ["--find-set", "pats"]),
        ("a pattern of 257 bytes", b"a" * 257 + b"\n", ["--find-set", "pats"]),
        ("a pattern with the delimiter", b"ab\nc d\n", ["--grep-set", "pats", "--delim", "20"]),
        ("a folded pattern with the folded delimiter", b"xay\n", ["--grep-set", "pats", "--delim", "41", "--ignore-case"]),
        ("both set options", ok, ["--find-set", "pats", "--grep-set", "pats"]),
        ("a set with --find", ok, ["--find-set", "pats", "--find", "ab"]),
        ("a set with --grep", ok, ["--grep-set", "pats", "--grep", "ab"]),
        ("a set with --grep-hex", ok, ["--find-set", "pats", "--grep-hex", "6162"]),
        ("--set-hex without a set", ok, ["--find", "ab", "--set-hex"]),
        ("--ignore-case without a search", ok, ["--ignore-case"]),
        ("bad hex", b"6162\n61zz\n", ["--find-set", "pats", "--set-hex"]),
        ("odd hex", b"616\n", ["--grep-set", "pats", "--set-hex"]),
        ("no such file", ok, ["--find-set", "nothing-here"]),
        ("a set with -c", ok, ["--find-set", "pats", "-c", "lz77"]),
        ("a set with --list", ok, ["--grep-set", "pats", "--list"]),
        ("a set with --line-numbers", ok, ["--find-set", "pats", "--line-numbers"]),
        ("--delim with --find-set", ok, ["--find-set", "pats", "--delim", "20"]),
    ]


@pytest.mark.parametrize("what,body,extra", usage_cases(), ids=[c[0] for c in usage_cases()])
def test_usage_errors(tmp_path, mixed, what, body, extra):
    (tmp_path / "in.fcx").write_bytes(mixed.blob)
    (tmp_path / "pats").write_bytes(body)
    r = run(["-i", "in.fcx", "-o", "x"] + extra, tmp_path)
    assert r.returncode not in (0, 1) and "usage:" in r.stderr, r.stdout + r.stderr
    assert "grep:" not in r.stdout and "find:" not in r.stdout
    assert not (tmp_path / "x").exists()


@pytest.mark.gpu
def test_gpu_sets_both_kinds(tmp_path, mixed, cuda):
    words, edges, upper = mixed_sets(mixed)
    find_agrees(tmp_path, mixed, edges)
    grep_agrees(tmp_path, mixed, upper, hexed=False, fold=True)
    T = tail_file()
    pats = [gm.cut(T.plain, 0x0A, 4090, 10), T.plain[:1], T.plain[5000:5003].upper()]
    pats = [p for p in pats if p and b"\n" not in p]
    find_agrees(tmp_path, T, pats, fold=True)
    grep_agrees(tmp_path, T, pats, fold=True)
