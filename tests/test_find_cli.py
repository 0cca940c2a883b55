"""The command line's search: --find STRING, --find-hex HEX and --count in the decompress mode.  Without a
HIP device an FCX7 file is searched by the host decoder record by record behind a rolling tail
(fcx_cli_host.h: host_find) and an FCX8 file fails loudly; with one both kinds go through fcx_find_stream,
and the same assertions hold (the gpu twins).

The expected offsets never come from the code under test: the records are the oracle encoder's, their
decoded bytes the oracle decoder's (Truth of test_gpu_range.py), the hits bytes.find over them."""
import pytest

import find_model as model
import oracle
from test_cli import gpu_present, run
from test_gpu_range import Truth

SIZES = [4096, 4096, 0, 0, 0, 4096, 4096, 1808]


@pytest.fixture(scope="module")
def mixed():
    T = Truth("7", model.mixed_data(), 4096)
    assert T.sizes == SIZES
    return T


def find(tmp_path, blob: bytes, pat: bytes, hexed: bool, count: bool = False):
    """(the run, the offsets of its lines, its totals)"""
    (tmp_path / "in.fcx").write_bytes(blob)
    args = ["-i", "in.fcx", "-o", "never"] + (["--find-hex", pat.hex()] if hexed else ["--find", pat.decode("latin-1")])
    r = run(args + (["--count"] if count else []), tmp_path)
    assert not (tmp_path / "never").exists()   # no -o file is written
    return r, [int(x) for x in model.LINE.findall(r.stdout)], [(int(h), int(d)) for h, d in model.TOTALS.findall(r.stdout)]


def agrees(tmp_path, blob: bytes, plain: bytes, pat: bytes, hexed: bool, count: bool = False):
    """the run (with --count: that run alone) says what bytes.find says"""
    want = model.hits(plain, pat)
    r, lines, totals = find(tmp_path, blob, pat, hexed, count)
    assert r.returncode == 0, r.stdout + r.stderr
    assert lines == ([] if count else want) and totals == [(len(want), len(plain))], r.stdout + r.stderr
    assert r.stdout.rstrip().splitlines()[-1].startswith("find: %d hits" % len(want))   # the totals come last
    return want


def mixed_patterns(T, full: bool):
    """(pattern, as hex digits?, with --count?) of the mixed file; a run is a process, so they are few"""
    plain = T.plain
    yield plain[8189:8196], True, False   # across the three records that decode to nothing
    yield plain[8189:8196], True, True
    yield plain[100:102], True, False
    word = next(w for w in plain.split(b" ") if len(w) >= 5 and w.isalnum())
    yield word, False, False
    if not full:
        return
    yield b" " + word[:2], False, True
    for m, count in ((1, True), (17, False), (256, False)):
        for p in (T.total - m, 8192 - m // 2):
            yield plain[p:p + m], True, count
    yield model.absent(plain), True, False


def check_mixed(tmp_path, T, full: bool = True):
    assert model.hits(T.plain, T.plain[8189:8196]) == [8189]
    for pat, hexed, count in mixed_patterns(T, full):
        agrees(tmp_path, T.blob, T.plain, pat, hexed, count)


def test_find_on_the_mixed_file(tmp_path, mixed):
    check_mixed(tmp_path, mixed)


def test_a_match_across_the_empty_records(tmp_path, mixed):
    pat = mixed.plain[8189:8196]
    r, lines, totals = find(tmp_path, mixed.blob, pat, True)
    assert r.returncode == 0 and lines == [8189] and totals == [(1, 18192)], r.stdout + r.stderr
    assert r.stdout.splitlines()[-2:] == ["find: offset 8189", "find: 1 hits, decoded bytes = 18192"]


USAGE = [["--find", "ab", "-c", "lz77"], ["--find", "ab", "--range", "0:5"], ["--find", "ab", "--list"],
         ["--find", "ab", "--compare", "orig"], ["--find", "ab", "-c", "lz77", "--verify"], ["--find", "ab", "--repair", "side"],
         ["--find", "ab", "--digest", "dig"], ["--find", "ab", "--digest", "dig", "--test"], ["--find", "ab", "--find-hex", "6162"],
         ["--find-hex", "6162", "-c", "lz77"], ["--find-hex", "6162", "--list"], ["--find-hex", "616"], ["--find-hex", "61zz"],
         ["--find-hex", ""], ["--find", ""], ["--find", "a" * 257], ["--find-hex", "61" * 257], ["--count"],
         ["--count", "--list"], ["--find"]]


@pytest.mark.parametrize("extra", USAGE, ids=[" ".join(x)[:40] for x in USAGE])
def test_invalid_flag_combinations_are_usage_errors(tmp_path, mixed, extra):
    (tmp_path / "in.fcx").write_bytes(mixed.blob)
    (tmp_path / "orig").write_bytes(model.mixed_data())
    r = run(["-i", "in.fcx", "-o", "x"] + extra, tmp_path)
    assert r.returncode not in (0, 1) and "usage:" in r.stderr, r.stdout + r.stderr
    assert "find:" not in r.stdout
    assert not (tmp_path / "x").exists() and not (tmp_path / "dig").exists() and not (tmp_path / "side").exists()


def test_the_longest_patterns_are_taken(tmp_path, mixed):
    for m in (255, 256):
        agrees(tmp_path, mixed.blob, mixed.plain, mixed.plain[4000:4000 + m], True)


def test_a_damaged_record_fails_the_search(tmp_path, mixed):
    q = mixed.rec_off[5] + 10
    sz = mixed.rec_off[6] - mixed.rec_off[5] - 4
    bad = mixed.blob[:q + 4] + b"\xFF" * sz + mixed.blob[q + 4 + sz:]
    r, lines, totals = find(tmp_path, bad, mixed.plain[100:102], True)
    assert r.returncode not in (0, 1) and totals == [], r.stdout + r.stderr


def tail_file():
    t = bytearray(model.text(7, 12288)[:10001])
    t[4095] = t[8191] = t[10000] = 0
    return Truth("8", bytes(t), 4096)


def test_fcx8_needs_a_device(tmp_path):
    T = tail_file()
    assert T.sizes == [4095, 4095, 1808]
    pat = T.plain[4090:4100]   # across the first seam: the record's tail zero is not there
    r, lines, totals = find(tmp_path, T.blob, pat, True)
    if gpu_present():
        want = model.hits(T.plain, pat)
        assert r.returncode == 0 and lines == want and totals == [(len(want), T.total)], r.stdout + r.stderr
    else:
        assert r.returncode not in (0, 1) and ("HIP" in r.stderr or "GPU" in r.stderr), r.stderr
        assert lines == [] and totals == []


@pytest.mark.gpu
def test_gpu_find_both_kinds(tmp_path, mixed, cuda):
    check_mixed(tmp_path, mixed, full=False)
    T = tail_file()
    for pat, count in ((T.plain[4090:4100], False), (T.plain[:1], True), (T.plain[T.total - 256:], False)):
        agrees(tmp_path, T.blob, T.plain, pat, True, count)
