"""The command line's grep: --grep STRING, --grep-hex HEX, --count and --delim in the decompress mode.  Without a HIP
device an FCX7 file is cut into lines by the host decoder (fcx_cli_host.h: host_grep) and an FCX8 file fails
loudly; with one both kinds go through fcx_grep_stream and fcx_decompress_ranges_stream, and the same assertions
hold (the gpu twin).

The expected bytes never come from the code under test: the records are the oracle encoder's, their decoded bytes
the oracle decoder's (Truth of test_gpu_range.py), the lines grep_model.selected over them."""
import pytest

import find_model as fm
import grep_model as model
from test_cli import gpu_present, run
from test_gpu_range import Truth

SIZES = [4096, 4096, 0, 0, 0, 4096, 4096, 1808]


@pytest.fixture(scope="module")
def mixed():
    T = Truth("7", fm.mixed_data(), 4096)
    assert T.sizes == SIZES
    return T


def grep(tmp_path, blob: bytes, pat: bytes, hexed: bool, count: bool = False, delim: int = None):
    """(the run, the bytes of -o or None, its totals)"""
    (tmp_path / "in.fcx").write_bytes(blob)
    out = tmp_path / "out.txt"
    if out.exists():
        out.unlink()
    args = ["-i", "in.fcx", "-o", "out.txt"] + (["--grep-hex", pat.hex()] if hexed else ["--grep", pat.decode("latin-1")])
    args += (["--count"] if count else []) + (["--delim", "%02x" % delim] if delim is not None else [])
    r = run(args, tmp_path)
    return r, out.read_bytes() if out.exists() else None, [tuple(int(x) for x in t) for t in model.TOTALS.findall(r.stdout)]


def agrees(tmp_path, T: Truth, pat: bytes, hexed: bool, count: bool = False, delim: int = None):
    d = 0x0A if delim is None else delim
    want = model.selected(T.plain, pat, d)
    r, out, totals = grep(tmp_path, T.blob, pat, hexed, count, delim)
    assert r.returncode == 0, r.stdout + r.stderr
    st = model.stats(T.plain, pat, d, want)
    assert totals == [(st[0], st[1], st[2], st[4])], r.stdout + r.stderr
    assert r.stdout.rstrip().splitlines()[-1].startswith("grep: %d lines" % len(want))   # the totals come last
    assert out == (None if count else model.join(T.plain, want)), (pat, count, delim)
    return want


def mixed_patterns(T, full: bool):
    """(pattern, as hex digits?, with --count?, delimiter) of the mixed file; a run is a process, so they are few"""
    plain = T.plain
    yield plain[8189:8196], True, False, None   # in the line across the three records that decode to nothing
    yield plain[100:102], True, False, None
    word = next(w for w in plain.split(b" ") if len(w) >= 5 and w.isalnum())
    yield word, False, False, None
    yield word, False, True, None
    if not full:
        return
    yield b"e", False, False, None
    yield plain[T.total - 3:], True, False, None             # the tail line
    yield plain[:4], True, False, 0x20                       # another delimiter: "lines" are words
    yield plain[8189:8196].replace(b" ", b"")[:3], True, True, 0x20
    yield fm.absent(plain), True, False, None                # no line: an empty -o file


def check_mixed(tmp_path, T, full: bool = True):
    s, e = model.line_of(T.plain, 0x0A, 8192)
    assert s < 8192 < e
    for pat, hexed, count, delim in mixed_patterns(T, full):
        if bytes([0x0A if delim is None else delim]) not in pat:
            agrees(tmp_path, T, pat, hexed, count, delim)


def test_grep_on_the_mixed_file(tmp_path, mixed):
    check_mixed(tmp_path, mixed)


def test_the_longest_patterns_are_taken(tmp_path, mixed):
    for m in (255, 256):
        pat = mixed.plain[9000:9000 + m]   # (random bytes: the delimiter 0xFF is planted out of the way)
        d = next(x for x in range(255, 0, -1) if x not in pat)
        agrees(tmp_path, mixed, pat, True, False, d)


USAGE = [["--grep", "ab", "-c", "lz77"], ["--grep", "ab", "--range", "0:5"], ["--grep", "ab", "--list"],
         ["--grep", "ab", "--compare", "orig"], ["--grep", "ab", "-c", "lz77", "--verify"], ["--grep", "ab", "--repair", "side"],
         ["--grep", "ab", "--digest", "dig"], ["--grep", "ab", "--digest", "dig", "--test"], ["--grep", "ab", "--find", "ab"],
         ["--grep", "ab", "--find-hex", "6162"], ["--grep", "ab", "--count-lines"], ["--grep", "ab", "--lines", "1:2"],
         ["--grep", "ab", "--line-numbers"], ["--grep", "ab", "--find", "ab", "--line-numbers"], ["--grep", "ab", "--grep-hex", "6162"],
         ["--grep-hex", "6162", "-c", "lz77"], ["--grep-hex", "6162", "--list"], ["--grep-hex", "616"], ["--grep-hex", "61zz"],
         ["--grep-hex", ""], ["--grep", ""], ["--grep", "a" * 257], ["--grep-hex", "61" * 257], ["--grep"],
         ["--grep-hex", "610a62"], ["--grep", "a b", "--delim", "20"], ["--delim", "61", "--grep", "xay"], ["--grep-hex", "00", "--delim", "00"]]


@pytest.mark.parametrize("extra", USAGE, ids=[" ".join(x)[:40] for x in USAGE])
def test_invalid_flag_combinations_are_usage_errors(tmp_path, mixed, extra):
    (tmp_path / "in.fcx").write_bytes(mixed.blob)
    (tmp_path / "orig").write_bytes(fm.mixed_data())
    r = run(["-i", "in.fcx", "-o", "x"] + extra, tmp_path)
    assert r.returncode not in (0, 1) and "usage:" in r.stderr, r.stdout + r.stderr
    assert "grep:" not in r.stdout and "find:" not in r.stdout
    assert not (tmp_path / "x").exists() and not (tmp_path / "dig").exists() and not (tmp_path / "side").exists()


def test_a_damaged_record_fails_the_grep(tmp_path, mixed):
    q = mixed.rec_off[5] + 10
    sz = mixed.rec_off[6] - mixed.rec_off[5] - 4
    bad = mixed.blob[:q + 4] + b"\xFF" * sz + mixed.blob[q + 4 + sz:]
    r, out, totals = grep(tmp_path, bad, mixed.plain[100:102], True)
    assert r.returncode not in (0, 1) and totals == [], r.stdout + r.stderr


def tail_file():
    t = bytearray(fm.text(7, 12288)[:10001])
    t[4095] = t[8191] = t[10000] = 0
    return Truth("8", bytes(t), 4096)


def test_fcx8_needs_a_device(tmp_path):
    T = tail_file()
    assert T.sizes == [4095, 4095, 1808]
    pat = model.cut(T.plain, 0x0A, 4090, 10)
    r, out, totals = grep(tmp_path, T.blob, pat, True)
    if gpu_present():
        want = model.selected(T.plain, pat, 0x0A)
        assert r.returncode == 0 and out == model.join(T.plain, want) and len(totals) == 1, r.stdout + r.stderr
    else:
        assert r.returncode not in (0, 1) and ("HIP" in r.stderr or "GPU" in r.stderr), r.stderr
        assert totals == []


@pytest.mark.gpu
def test_gpu_grep_both_kinds(tmp_path, mixed, cuda):
    check_mixed(tmp_path, mixed, full=False)
    T = tail_file()
    for pat, count, delim in ((model.cut(T.plain, 0x0A, 4090, 10), False, None), (T.plain[:1], True, None), (T.plain[5000:5003], False, 0x00)):
        if bytes([0x0A if delim is None else delim]) not in pat:
            agrees(tmp_path, T, pat, True, count, delim)
