"""The command line's round-trip check: --compare ORIGINAL in the decompress mode (and --verify with
-c, which needs a device: tests/test_gpu_verify.py).  Without a HIP device --compare runs on the
host decoder for FCX7 (fcx_cli_host.h, host_compare) and fails loudly for FCX8.

The expected lines never come from the code under test: the decoded bytes of a record are the
oracle decoder's (per_record of test_range_cli.py), and the pair (decoded bytes, first difference)
and the totals follow from those bytes and the original by expect() below."""
import re

import pytest

import inputs
import oracle
from test_cli import gpu_present, run
from test_range_cli import per_record

SAME = 0xFFFFFFFF
LINE = re.compile(r"^block (\d+): decoded (\d+) of (\d+) bytes, first difference at (\d+)$", re.M)
TOTAL = re.compile(r"^verify: (\d+) of (\d+) blocks differ, (\d+) input bytes in them \[(OK|FAIL)\]$", re.M)
EXTRA = re.compile(r"^original: (\d+) bytes after the last block$", re.M)


def first_diff(dec: bytes, blk: bytes) -> int:
    m = min(len(dec), len(blk))
    if dec[:m] == blk[:m]:
        return SAME if len(dec) == len(blk) else m
    for i in range(m):
        if dec[i] != blk[i]:
            return i
    return SAME if len(dec) == len(blk) else m


def expect(parts, orig: bytes, block: int):
    """from the decoded records and the original: ([(k, decoded, block length, first difference)] of the
    differing blocks, stats as fcx_verify_*: blocks, differ, first, size_differs, bytes, decoded; the
    original bytes behind the last record, counted into stats[4])"""
    rows, sized, nbytes = [], 0, 0
    for k, dec in enumerate(parts):
        blk = orig[k * block:(k + 1) * block]
        fd = 0 if k * block >= len(orig) else first_diff(dec, blk)
        sized += len(dec) != len(blk)
        if fd != SAME:
            rows.append((k, len(dec), len(blk), fd))
            nbytes += len(blk)
    extra = max(0, len(orig) - len(parts) * block)
    stats = [len(parts), len(rows), rows[0][0] if rows else None, sized, nbytes + extra, sum(len(p) for p in parts)]
    return rows, stats, extra


def check_compare(tmp_path, blob: bytes, orig: bytes, block: int, lz78: bool = False):
    """runs --compare and checks every line against expect(); returns (rows, stats)"""
    _, parts = per_record(blob, lz78)
    rows, stats, extra = expect(parts, orig, block)
    (tmp_path / "in.fcx").write_bytes(blob)
    (tmp_path / "orig").write_bytes(orig)
    r = run(["-i", "in.fcx", "-o", "never", "--compare", "orig", "-b", str(block)], tmp_path)
    assert [tuple(int(x) for x in m) for m in LINE.findall(r.stdout)] == rows, r.stdout + r.stderr
    assert [int(x) for x in EXTRA.findall(r.stdout)] == ([extra] if extra else []), r.stdout
    ok = stats[1] == 0 and stats[4] == 0
    assert TOTAL.findall(r.stdout) == [(str(stats[1]), str(stats[0]), str(stats[4]), "OK" if ok else "FAIL")], r.stdout + r.stderr
    assert r.returncode == (0 if ok else 1), r.stdout + r.stderr
    assert not (tmp_path / "never").exists()   # --compare writes no file
    return rows, stats


def mixed_data() -> bytes:
    return inputs.generate("text", 7, 8192) + inputs.generate("rand", 3, 12288) + inputs.generate("text", 9, 10000)


@pytest.fixture(scope="module")
def text():
    data = inputs.generate("text", 7, 20000)
    return data, oracle.compress_file(data, 4096)


def test_mixed_file_loses_its_random_blocks(tmp_path):
    data = mixed_data()
    rows, stats = check_compare(tmp_path, oracle.compress_file(data, 4096), data, 4096)
    assert rows == [(2, 0, 4096, 0), (3, 0, 4096, 0), (4, 0, 4096, 0)]
    assert stats == [8, 3, 2, 3, 12288, 4096 * 4 + 1808]
    r = run(["-i", "in.fcx", "-o", "never", "--compare", "orig", "-b", "4096"], tmp_path)
    assert "verify: 3 of 8 blocks differ, 12288 input bytes in them [FAIL]" in r.stdout.splitlines()
    assert "block 3: decoded 0 of 4096 bytes, first difference at 0" in r.stdout.splitlines()
    assert r.returncode == 1


def test_text_comes_back(tmp_path, text):
    data, blob = text
    rows, stats = check_compare(tmp_path, blob, data, 4096)
    assert rows == [] and stats[:2] == [5, 0]
    r = run(["-i", "in.fcx", "--compare", "orig", "-b", "4096"], tmp_path)
    assert "verify: 0 of 5 blocks differ, 0 input bytes in them [OK]" in r.stdout.splitlines() and r.returncode == 0


def test_one_repeated_byte_decodes_as_zeros(tmp_path):
    data = b"A" * 5000
    rows, _ = check_compare(tmp_path, oracle.compress_file(data, 4096), data, 4096)
    assert rows == [(0, 4096, 4096, 0), (1, 904, 904, 0)]   # both full size: only the bytes differ


@pytest.mark.parametrize("at", [4096 * 3 + 1234, 19999])
def test_edited_original_names_the_block_and_the_byte(tmp_path, text, at):
    data, blob = text
    edited = bytearray(data)
    edited[at] ^= 0x55
    rows, stats = check_compare(tmp_path, blob, bytes(edited), 4096)
    blen = min(4096, 20000 - at // 4096 * 4096)
    assert rows == [(at // 4096, blen, blen, at % 4096)] and stats[2] == at // 4096


def test_original_too_short_and_too_long(tmp_path, text):
    data, blob = text
    rows, stats = check_compare(tmp_path, blob, data[:-100], 4096)
    assert rows == [(4, 3616, 3516, 3516)] and stats[3] == 1
    rows, stats = check_compare(tmp_path, blob, data + b"x" * 100, 4096)
    assert rows == [(4, 3616, 3716, 3616)] and stats[4] == 3716   # the extra bytes are in the last block
    r = run(["-i", "in.fcx", "--compare", "orig", "-b", "4096"], tmp_path)
    assert "verify: 1 of 5 blocks differ, 3716 input bytes in them [FAIL]" in r.stdout.splitlines() and r.returncode == 1
    # bytes behind the last record's block are bytes the file does not hold: reported, and FAIL
    blob4 = oracle.compress_file(data[:16384], 4096)
    rows, stats = check_compare(tmp_path, blob4, data[:16384] + b"y" * 100, 4096)
    assert rows == [] and stats[1] == 0 and stats[4] == 100
    r = run(["-i", "in.fcx", "--compare", "orig", "-b", "4096"], tmp_path)
    assert "original: 100 bytes after the last block" in r.stdout.splitlines()
    assert "verify: 0 of 4 blocks differ, 100 input bytes in them [FAIL]" in r.stdout.splitlines() and r.returncode == 1
    # a record the original has no bytes for differs, with block length 0
    rows, _ = check_compare(tmp_path, blob, data[:8192], 4096)
    assert rows == [(2, 4096, 0, 0), (3, 4096, 0, 0), (4, 3616, 0, 0)]


def test_truncated_record_is_an_error_not_a_verdict(tmp_path, text):
    data, blob = text
    (tmp_path / "in.fcx").write_bytes(blob[:-50])
    (tmp_path / "orig").write_bytes(data)
    r = run(["-i", "in.fcx", "--compare", "orig", "-b", "4096"], tmp_path)
    assert r.returncode not in (0, 1) and r.stderr.strip(), r.stdout + r.stderr
    assert not TOTAL.search(r.stdout)


def test_compare_fcx8_fails_loudly_without_gpu(tmp_path):
    if gpu_present():
        pytest.skip("GPU present")
    (tmp_path / "x8").write_bytes(oracle.lz78_compress_file(b"hello hello hello", 1 << 20))
    (tmp_path / "orig").write_bytes(b"hello hello hello")
    r = run(["-i", "x8", "--compare", "orig"], tmp_path)
    assert r.returncode not in (0, 1) and ("HIP" in r.stderr or "GPU" in r.stderr), r.stderr
    assert not TOTAL.search(r.stdout)


@pytest.mark.parametrize("extra", [["--compare", "orig", "-c", "lz77"], ["--compare", "orig", "--range", "0:5"],
                                   ["--compare", "orig", "--list"], ["--compare", "orig", "-c", "lz78", "--verify"],
                                   ["--compare", "orig", "--verify"], ["--verify"], ["--verify", "--list"]])
def test_invalid_flag_combinations_are_usage_errors(tmp_path, text, extra):
    data, blob = text
    (tmp_path / "in.fcx").write_bytes(blob)
    (tmp_path / "orig").write_bytes(data)
    r = run(["-i", "in.fcx", "-o", "x"] + extra, tmp_path)
    assert r.returncode not in (0, 1) and "usage:" in r.stderr
    assert not (tmp_path / "x").exists()
