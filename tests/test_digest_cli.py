"""The command line's content digest: --digest FILE with --compare ORIGINAL writes the FCXD file, and a
decompress with --test --digest FILE [--repair R] says whether the file, repaired or not, still gives the
bytes that were digested, without the original.  Without a HIP device the FCX7 directions run on the host
decoder and the host CRC-32 (fcx_cli_host.h: host_digest_build, host_check) and FCX8 fails loudly; with one
they run on the device, and the same assertions hold.

The expected bytes never come from the code under test: the CRC-32 is zlib's, the records are the oracle
encoder's, their decoded bytes the oracle decoder's, and the FCXD file, the failing blocks and their numbers
follow from those by tests/digest_model.py and tests/repair_model.py."""
import re
import struct
import zlib

import pytest

import digest_model as model
import inputs
import oracle
import repair_model
from test_cli import gpu_present, run
from test_compare_cli import mixed_data
from test_range_cli import per_record

DIGEST = re.compile(r"^digest: (\d+) blocks, crc32 ([0-9A-F]{8})$", re.M)
LINE = re.compile(r"^block (\d+): (\d+) of (\d+) bytes, crc32 ([0-9A-F]{8}), expected ([0-9A-F]{8}|none)$", re.M)
EXTRA = re.compile(r"^digest: (\d+) bytes after the last block$", re.M)
VERDICT = re.compile(r"^test: (\d+) of (\d+) blocks fail, (\d+) input bytes in them \[(OK|FAIL)\]$", re.M)


def text(seed, n):
    return inputs.generate("text", seed, n)


def rand(seed, n):
    return inputs.generate("rand", seed, n)


def write_digest(tmp_path, data: bytes, block: int, blob: bytes = None) -> bytes:
    """--compare ORIGINAL --digest FILE: the FCXD file's bytes, checked against the model's"""
    blob = oracle.compress_file(data[:4 * block], block) if blob is None else blob   # (--compare needs a file; its verdict is not looked at)
    (tmp_path / "in.fcx").write_bytes(blob)
    (tmp_path / "orig").write_bytes(data)
    r = run(["-i", "in.fcx", "--compare", "orig", "--digest", "dig", "-b", str(block)], tmp_path)
    assert r.returncode in (0, 1), r.stdout + r.stderr
    got = (tmp_path / "dig").read_bytes()
    want = model.canonical(data, block)
    assert got == want
    assert DIGEST.findall(r.stdout) == [(str((len(data) + block - 1) // block), "%08X" % zlib.crc32(data))], r.stdout + r.stderr
    assert r.stdout.index("verify:") < r.stdout.index("digest:")
    return got


def check(tmp_path, blob: bytes, digest: bytes, repair: bytes = None, decompress: bool = False):
    """--test (or the decompress with --digest): (return code, stats as the verdict shows them, rows) and the
    run, compared with the model's by the caller"""
    (tmp_path / "in.fcx").write_bytes(blob)
    (tmp_path / "dig").write_bytes(digest)
    args = ["-i", "in.fcx", "--digest", "dig"] + (["-o", "out"] if decompress else ["--test", "-o", "never"])
    if repair is not None:
        (tmp_path / "side").write_bytes(repair)
        args += ["--repair", "side"]
    r = run(args, tmp_path)
    assert not (tmp_path / "never").exists()
    rows = [(int(k), int(m), int(n), int(c, 16)) for k, n, m, c, _ in LINE.findall(r.stdout)]
    extra = EXTRA.findall(r.stdout)
    verdict = VERDICT.findall(r.stdout)
    return r, rows, extra, verdict


def agrees(tmp_path, blob: bytes, digest: bytes, repair: bytes = None, **kw):
    """the run says what the model says; returns the model's (stats, rows)"""
    _, parts = per_record(blob, False)
    stats, rows = model.check(parts, digest, repair)
    r, got_rows, extra, verdict = check(tmp_path, blob, digest, repair, **kw)
    assert r.returncode in (0, 1), r.stdout + r.stderr
    want_rows = [x for x in rows if x[0] < len(parts)]
    assert got_rows == want_rows, r.stdout + r.stderr
    assert extra == [str(x[1]) for x in rows if x[0] == len(parts)]
    ok = stats[1] == 0 and stats[4] == 0
    assert verdict == [(str(stats[1]), str(stats[0]), str(stats[4]), "OK" if ok else "FAIL")], r.stdout + r.stderr
    assert r.returncode == (0 if ok else 1)
    # every line shows the digest file's value for its block
    want = [v for g in model.parse(digest)[1] for v in g]
    for k, _, _, _, exp in LINE.findall(r.stdout):
        assert exp == ("%08X" % want[int(k)] if int(k) < len(want) else "none")
    return stats, rows


@pytest.mark.parametrize("name", ["mixed", "text", "one byte"])
def test_writer_agrees_with_the_model(tmp_path, name):
    data = {"mixed": mixed_data(), "text": text(7, 20000), "one byte": b"A" * 5000}[name]
    d = write_digest(tmp_path, data, 4096)
    block, groups, (n, blocks, whole, _) = model.parse(d)
    assert (block, n, blocks, whole) == (4096, len(data), (len(data) + 4095) // 4096, zlib.crc32(data))
    assert len(d) == 16 + 8 + 4 * blocks + 8 + 24


def test_5000_blocks_of_one_byte_make_two_sections(tmp_path):
    data = rand(9, 5000)
    d = write_digest(tmp_path, data, 1, blob=oracle.compress_file(data[:8], 1))
    _, groups, (n, blocks, whole, _) = model.parse(d)
    assert [len(g) for g in groups] == [4096, 904] and (n, blocks, whole) == (5000, 5000, zlib.crc32(data))


def test_empty_original(tmp_path):
    d = write_digest(tmp_path, b"", 4096, blob=oracle.compress_file(b"", 4096))
    assert d == model.header(4096) + bytes(8) + struct.pack("<QQII", 0, 0, 0, 0)


class Pair:
    def __init__(self, data: bytes, block: int):
        self.data, self.block = data, block
        self.blob = oracle.compress_file(data, block)
        _, self.parts = per_record(self.blob, False)
        self.digest = model.canonical(data, block)

    def repair(self, orig: bytes = None) -> bytes:
        return repair_model.canonical("7", self.parts, self.data if orig is None else orig, self.block)


@pytest.fixture(scope="module")
def mixed():
    return Pair(mixed_data(), 4096)


def test_mixed_file_fails_its_random_blocks(tmp_path, mixed):
    stats, rows = agrees(tmp_path, mixed.blob, mixed.digest)
    assert [r[0] for r in rows] == [2, 3, 4] and stats[:5] == [8, 3, 2, 3, 12288]
    assert all(r[2] == 0 and r[3] == 0 for r in rows)   # each decodes to no bytes: length 0, the empty CRC-32


def test_with_its_repair_the_file_is_ok(tmp_path, mixed):
    stats, rows = agrees(tmp_path, mixed.blob, mixed.digest, mixed.repair())
    assert rows == [] and stats[1] == 0
    for size in (1, 3):   # the same digest in other sections
        assert agrees(tmp_path, mixed.blob, model.resection(mixed.digest, size), mixed.repair())[1] == []


def test_a_repair_from_other_data_fails(tmp_path, mixed):
    """a sidecar of the same kind, block size, length and record count: the repair's own checks cannot see it"""
    other = mixed.data[:8192] + rand(77, 12288) + mixed.data[20480:]
    side = mixed.repair(other)
    assert repair_model.apply(mixed.parts, side) == other   # (a valid repair: of another original)
    stats, rows = agrees(tmp_path, mixed.blob, mixed.digest, side)
    assert [r[0] for r in rows] == [2, 3, 4] and stats[1] == 3 and all(r[1] == r[2] == 4096 for r in rows)


def test_decompress_with_digest_writes_the_output_and_tests(tmp_path, mixed):
    agrees(tmp_path, mixed.blob, mixed.digest, mixed.repair(), decompress=True)
    assert (tmp_path / "out").read_bytes() == mixed.data
    other = mixed.data[:8192] + rand(77, 12288) + mixed.data[20480:]
    stats, _ = agrees(tmp_path, mixed.blob, mixed.digest, mixed.repair(other), decompress=True)
    assert (tmp_path / "out").read_bytes() == other and stats[1] == 3
    # without a repair: the plain decompress, its own size verdict, and the test's lines
    agrees(tmp_path, mixed.blob, mixed.digest, decompress=True)
    assert (tmp_path / "out").read_bytes() == b"".join(mixed.parts)


def flipped(p: Pair, k: int):
    """the file with one payload byte of record k flipped so that the oracle's decoder still decodes the
    record, to other bytes; a condition of the test, not a skip"""
    q = 10
    for _ in range(k):
        q += 4 + struct.unpack_from("<I", p.blob, q)[0]
    (sz,) = struct.unpack_from("<I", p.blob, q)
    for at in range(q + 4 + sz - 1, q + 4, -1):
        for bit in (1, 16):
            b = bytearray(p.blob)
            b[at] ^= bit
            dec = oracle.decompress_block(bytes(b[q + 4:q + 4 + sz]), (1 << 20) + 64)
            if dec is not None and dec != p.parts[k] and len(dec) <= p.block + 64:
                return bytes(b)
    raise AssertionError("no flip of record %d still decodes" % k)


def test_a_flipped_payload_byte_fails_exactly_its_block(tmp_path):
    p = Pair(text(7, 20000), 4096)
    assert agrees(tmp_path, p.blob, p.digest)[1] == []
    bad = flipped(p, 2)
    stats, rows = agrees(tmp_path, bad, p.digest)
    assert [r[0] for r in rows] == [2] and stats[1] == 1


def test_leftovers_on_either_side(tmp_path):
    p = Pair(text(7, 20000), 4096)
    longer = model.canonical(p.data + text(8, 5000), 4096)     # blocks behind the last record
    stats, rows = agrees(tmp_path, p.blob, longer)
    assert rows[-1][0] == 5 and stats[4] > 0
    shorter = model.canonical(p.data[:8192], 4096)             # records behind the last block
    stats, rows = agrees(tmp_path, p.blob, shorter)
    assert [r[:2] for r in rows] == [(2, 0), (3, 0), (4, 0)]


def patched(blob: bytes, at: int, fmt: str, value) -> bytes:
    b = bytearray(blob)
    struct.pack_into(fmt, b, at, value)
    return bytes(b)


def rejected():
    """(name, a digest file that must be refused)"""
    p = Pair(mixed_data(), 4096)
    d = p.digest
    block, groups, (n, blocks, whole, self_crc) = model.parse(d)
    vals = groups[0]
    yield "bad magic", b"FCXE" + d[4:]
    yield "unknown version", patched(d, 4, "<B", 2)
    yield "reserved byte", patched(d, 5, "<B", 1)
    yield "reserved u16", patched(d, 6, "<H", 1)
    yield "reserved u32", patched(d, 12, "<I", 1)
    yield "block size 0", patched(d, 8, "<I", 0)
    yield "section reserved", patched(d, 20, "<I", 1)
    yield "count above 4096", patched(d, 16, "<I", 4097)
    yield "one altered value", patched(d, 24 + 4 * 3, "<I", vals[3] ^ 1)
    yield "trailer n", patched(d, len(d) - 24, "<Q", n + 1)
    yield "trailer n another block", patched(d, len(d) - 24, "<Q", n + 4096)
    yield "trailer blocks", patched(d, len(d) - 16, "<Q", blocks + 1)
    yield "trailer whole", patched(d, len(d) - 8, "<I", whole ^ 1)
    yield "trailer self", patched(d, len(d) - 4, "<I", self_crc ^ 1)
    yield "truncated in the header", d[:10]
    yield "truncated in a section", d[:30]
    yield "truncated before the trailer", d[:len(d) - 24]
    yield "truncated in the trailer", d[:-3]
    yield "bytes behind the trailer", d + b"\0"
    yield "a value dropped", model.header(4096) + model.section(vals[:-1]) + d[24 + 4 * len(vals):]


@pytest.mark.parametrize("name", [n for n, _ in rejected()])
def test_rejected_digests(tmp_path, name, mixed):
    d = next(x for n, x in rejected() if n == name)
    r, rows, extra, verdict = check(tmp_path, mixed.blob, d, mixed.repair())
    assert r.returncode not in (0, 1), r.stdout + r.stderr
    assert re.search(r"^fcx: .*digest file", r.stderr, re.M), r.stderr
    assert verdict == [] and "[OK]" not in r.stdout


def test_a_repair_of_another_block_size_is_refused(tmp_path, mixed):
    side = repair_model.file_from_rows("7", 8192, [], len(mixed.data), len(mixed.parts))
    r, _, _, verdict = check(tmp_path, mixed.blob, mixed.digest, side)
    assert r.returncode not in (0, 1) and "repair" in r.stderr and verdict == []


def test_fcx8_needs_a_device(tmp_path):
    data = b"hello hello hello\0"
    blob = oracle.lz78_compress_file(data, 1 << 20)
    digest = model.canonical(data, 1 << 20)
    r, rows, _, verdict = check(tmp_path, blob, digest)
    if gpu_present():
        _, parts = per_record(blob, True)
        stats, want_rows = model.check(parts, digest)
        assert rows == want_rows and r.returncode == 1 and verdict[0][3] == "FAIL", r.stdout + r.stderr   # the tail zero is lost
    else:
        assert r.returncode not in (0, 1) and ("HIP" in r.stderr or "GPU" in r.stderr), r.stderr
        assert verdict == []


@pytest.mark.parametrize("extra", [["--test"], ["--test", "--digest"], ["--test", "--digest", "dig", "-c", "lz77"],
                                   ["--test", "--digest", "dig", "--compare", "orig"],
                                   ["--test", "--digest", "dig", "--range", "0:5"], ["--test", "--digest", "dig", "--list"],
                                   ["--digest", "dig", "--range", "0:5"], ["--digest", "dig", "--list"]])
def test_invalid_flag_combinations_are_usage_errors(tmp_path, mixed, extra):
    (tmp_path / "in.fcx").write_bytes(mixed.blob)
    (tmp_path / "orig").write_bytes(mixed.data)
    r = run(["-i", "in.fcx", "-o", "x"] + extra, tmp_path)
    assert r.returncode not in (0, 1) and "usage:" in r.stderr
    assert not (tmp_path / "x").exists() and not (tmp_path / "dig").exists()
