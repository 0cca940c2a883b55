"""The command line's lines: --count-lines, --lines A:N, --find --line-numbers and --delim in the decompress
mode.  Without a HIP device an FCX7 file is served by the host decoder record by record (fcx_cli_host.h:
host_lines, host_find_numbered) and an FCX8 file fails loudly; with one both kinds go through fcx_lines_stream,
fcx_lines_locate_stream and fcx_lines_of_stream, and the same assertions hold (the gpu twin).

The expectations never come from the code under test: the records are the oracle encoder's, their decoded
bytes the oracle decoder's (Truth of test_gpu_range.py), the lines bytes.split over them (lines_model.py)."""
import pytest

import find_model
import lines_model as model
from test_cli import gpu_present, run
from test_gpu_range import Truth

SIZES = [4096, 4096, 0, 0, 0, 4096, 4096, 1808]


@pytest.fixture(scope="module")
def mixed():
    T = Truth("7", find_model.mixed_data(), 4096)
    assert T.sizes == SIZES
    return T


def cli(tmp_path, blob: bytes, args):
    (tmp_path / "in.fcx").write_bytes(blob)
    out = tmp_path / "out.bin"
    if out.exists():
        out.unlink()
    r = run(["-i", "in.fcx", "-o", "out.bin"] + args, tmp_path)
    return r, (out.read_bytes() if out.exists() else None)


def check_count(tmp_path, T, d: int, given: bool):
    r, out = cli(tmp_path, T.blob, ["--count-lines"] + (["--delim", "%02x" % d] if given else []))
    assert r.returncode == 0 and out is None, r.stdout + r.stderr   # no -o file
    n, L, total, _ = model.stats(T.plain, d)
    assert [tuple(map(int, m)) for m in model.TOTALS.findall(r.stdout)] == [(L, n, total)], r.stdout + r.stderr


def check_lines(tmp_path, T, d: int, a: int, n, given: bool = True):
    """--lines A:N (A from 1; n None: "A:") writes the model's join and says how much from where"""
    r, out = cli(tmp_path, T.blob, ["--lines", "%d:%s" % (a, "" if n is None else n)] + (["--delim", "%02X" % d] if given else []))
    assert r.returncode == 0, r.stdout + r.stderr
    off, length = model.locate(T.plain, d, a - 1, model.U64_MAX if n is None else n)
    assert out == T.plain[off:off + length], (d, a, n)
    assert [tuple(map(int, m)) for m in model.DONE.findall(r.stdout)] == [(length, off)], r.stdout + r.stderr
    want = model.lines(T.plain, d)[a - 1:None if n is None else a - 1 + n]
    assert out == b"".join(want)


def check_numbered(tmp_path, T, pat: bytes, d: int):
    r, out = cli(tmp_path, T.blob, ["--find-hex", pat.hex(), "--line-numbers", "--delim", "%02x" % d])
    assert r.returncode == 0 and out is None, r.stdout + r.stderr
    hits = find_model.hits(T.plain, pat)
    want = [(p, model.nl(T.plain, d, p) + 1) for p in hits]   # K is 1-based
    assert [tuple(map(int, m)) for m in model.NUMBERED.findall(r.stdout)] == want, r.stdout + r.stderr
    assert find_model.LINE.findall(r.stdout) == []
    assert [tuple(map(int, m)) for m in find_model.TOTALS.findall(r.stdout)] == [(len(hits), T.total)]
    return want


def check_mixed(tmp_path, T, full: bool):
    """a run is a process, and with a device one that opens it: the long list is for the host decoder's path"""
    L = model.stats(T.plain, 0x0A)[1]
    across = model.nl(T.plain, 0x0A, 8192)   # the line that lies across the three empty records
    assert model.locate(T.plain, 0x0A, across, 1)[0] < 8192 < sum(model.locate(T.plain, 0x0A, across, 1))
    check_count(tmp_path, T, 0x0A, False)
    for a, n in ((1, 1), (across + 1, 1), (L, None)):
        check_lines(tmp_path, T, 0x0A, a, n, given=a != 1)
    check_lines(tmp_path, T, 0x20, 1, 2)
    assert check_numbered(tmp_path, T, T.plain[8189:8196], 0x0A) == [(8189, across + 1)]
    check_numbered(tmp_path, T, T.plain[100:102], 0x20)
    if not full:
        return
    check_lines(tmp_path, T, 0x0A, L + 1, 1)
    for d in model.DELIMS:
        check_count(tmp_path, T, d, True)
    for a, n in ((1, None), (across, 3), (L, 1), (L, 5), (L + 7, None), (2, 0)):
        check_lines(tmp_path, T, 0x0A, a, n)
    for d in (0x00, 0xFF, 0x80, 0x20):
        check_lines(tmp_path, T, d, 1, 2)
        check_lines(tmp_path, T, d, max(model.stats(T.plain, d)[1], 1), None)
    word = next(w for w in T.plain.split(b" ") if len(w) >= 5 and w.isalnum())
    assert len(check_numbered(tmp_path, T, word, 0x0A)) >= 1
    check_numbered(tmp_path, T, find_model.absent(T.plain), 0x0A)


def test_lines_on_the_mixed_file(tmp_path, mixed):
    check_mixed(tmp_path, mixed, full=not gpu_present())


def test_a_file_without_a_delimiter_is_one_line(tmp_path):
    data = model.plant(model.text(3, 5000), 0x0A, [])
    T = Truth("7", data, 4096)
    assert T.sizes == [4096, 904] and model.stats(T.plain, 0x0A) == [0, 1, 5000, 5000]
    check_count(tmp_path, T, 0x0A, True)
    check_lines(tmp_path, T, 0x0A, 1, None)
    check_lines(tmp_path, T, 0x0A, 2, None)


USAGE = [["--count-lines", "-c", "lz77"], ["--count-lines", "--range", "0:5"], ["--count-lines", "--list"],
         ["--count-lines", "--compare", "orig"], ["--count-lines", "--repair", "side"], ["--count-lines", "--digest", "dig"],
         ["--count-lines", "--digest", "dig", "--test"], ["--count-lines", "-c", "lz77", "--verify"], ["--count-lines", "--verify"],
         ["--lines", "1:2", "-c", "lz77", "--verify"], ["--lines", "1:2", "--verify"], ["--lines", "1:2", "--repair", "side"],
         ["--lines", "1:2", "--digest", "dig"], ["--lines", "1:2", "--digest", "dig", "--test"],
         ["--find", "ab", "--line-numbers", "--list"], ["--find", "ab", "--line-numbers", "-c", "lz77"], ["--count-lines", "--find", "ab"], ["--count-lines", "--lines", "1:2"],
         ["--lines", "1:2", "-c", "lz77"], ["--lines", "1:2", "--range", "0:5"], ["--lines", "1:2", "--list"],
         ["--lines", "1:2", "--find-hex", "6162"], ["--lines", "1:2", "--compare", "orig"], ["--lines", "0:2"], ["--lines", "1"],
         ["--lines", ":2"], ["--lines", "1:2:3"], ["--lines", "a:2"], ["--lines", "1:-2"], ["--lines", ""], ["--lines"],
         ["--line-numbers"], ["--line-numbers", "--count-lines"], ["--find", "ab", "--count", "--line-numbers"],
         ["--delim", "0a"], ["--delim", "0a", "--find", "ab"], ["--delim", "0a", "--list"], ["--count-lines", "--delim", "a"],
         ["--count-lines", "--delim", "0a0a"], ["--count-lines", "--delim", "zz"], ["--count-lines", "--delim", ""],
         ["--count-lines", "--delim"]]


@pytest.mark.parametrize("extra", USAGE, ids=[" ".join(x)[:40] for x in USAGE])
def test_invalid_flag_combinations_are_usage_errors(tmp_path, mixed, extra):
    (tmp_path / "in.fcx").write_bytes(mixed.blob)
    (tmp_path / "orig").write_bytes(find_model.mixed_data())
    r = run(["-i", "in.fcx", "-o", "x"] + extra, tmp_path)
    assert r.returncode not in (0, 1) and "usage:" in r.stderr, r.stdout + r.stderr
    assert "lines" not in r.stdout and "find:" not in r.stdout
    assert not (tmp_path / "x").exists() and not (tmp_path / "dig").exists() and not (tmp_path / "side").exists()


def test_a_damaged_record_fails_the_count(tmp_path, mixed):
    q = mixed.rec_off[5] + 10
    sz = mixed.rec_off[6] - mixed.rec_off[5] - 4
    bad = mixed.blob[:q + 4] + b"\xFF" * sz + mixed.blob[q + 4 + sz:]
    r, _ = cli(tmp_path, bad, ["--count-lines"])
    assert r.returncode not in (0, 1) and model.TOTALS.findall(r.stdout) == [], r.stdout + r.stderr


def tail_file():
    t = bytearray(model.text(7, 12288)[:10001])
    t[4095] = t[8191] = t[10000] = 0
    return Truth("8", bytes(t), 4096)


def check_fcx8(tmp_path, T):
    check_count(tmp_path, T, 0x0A, True)
    check_lines(tmp_path, T, 0x0A, model.nl(T.plain, 0x0A, 4095) + 1, 2)   # across the first seam: the record's tail zero is not there
    check_numbered(tmp_path, T, T.plain[4090:4100], 0x0A)


def test_fcx8_needs_a_device(tmp_path):
    T = tail_file()
    assert T.sizes == [4095, 4095, 1808]
    if gpu_present():
        check_fcx8(tmp_path, T)
        return
    for args in (["--count-lines"], ["--lines", "1:2"], ["--find", "the", "--line-numbers"]):
        r, out = cli(tmp_path, T.blob, args)
        assert r.returncode not in (0, 1) and ("HIP" in r.stderr or "GPU" in r.stderr), r.stderr
        assert "lines" not in r.stdout and "find:" not in r.stdout and not out


@pytest.mark.gpu
def test_gpu_lines_both_kinds(tmp_path, mixed, cuda):
    check_mixed(tmp_path, mixed, full=False)
    check_fcx8(tmp_path, tail_file())
