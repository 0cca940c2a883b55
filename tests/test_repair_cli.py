"""The command line's repair sidecar: --repair FILE with --compare ORIGINAL writes the FCXR file, and a
decompress that is given it returns the original bytes.  Without a HIP device both run on the host
decoder for FCX7 (fcx_cli_host.h: host_repair_build, host_repair_apply) and fail loudly for FCX8; with
one they run on the device, and the same assertions hold.

The expected bytes never come from the code under test: the records are the oracle encoder's, their
decoded bytes the oracle decoder's (per_record of test_range_cli.py), and the FCXR file follows from those
and the original by tests/repair_model.py."""
import re
import struct

import pytest

import inputs
import oracle
import repair_model as model
from test_cli import gpu_present, run
from test_compare_cli import mixed_data
from test_range_cli import per_record

REPORT = re.compile(r"^repair: (\d+) entries, (\d+) data bytes for (\d+) blocks$", re.M)


def text(seed, n):
    return inputs.generate("text", seed, n)


def rand(seed, n):
    return inputs.generate("rand", seed, n)


class Pair:
    """an FCX7 file of the oracle's, and what its decoder makes of each record"""

    def __init__(self, data: bytes, block: int):
        self.data, self.block = data, block
        self.blob = oracle.compress_file(data, block)
        _, self.parts = per_record(self.blob, False)

    def want(self, orig: bytes = None) -> bytes:
        return model.canonical("7", self.parts, self.data if orig is None else orig, self.block)


def build(tmp_path, p: Pair, orig: bytes = None) -> bytes:
    """--compare ORIGINAL --repair side: the sidecar's bytes, checked against the model's"""
    orig = p.data if orig is None else orig
    (tmp_path / "in.fcx").write_bytes(p.blob)
    (tmp_path / "orig").write_bytes(orig)
    r = run(["-i", "in.fcx", "--compare", "orig", "--repair", "side", "-b", str(p.block)], tmp_path)
    assert r.returncode in (0, 1), r.stdout + r.stderr
    side = (tmp_path / "side").read_bytes()
    want = p.want(orig)
    assert side == want
    _, _, groups, (n, records, entries, data_bytes) = model.parse(want)
    assert REPORT.findall(r.stdout) == [(str(entries), str(data_bytes), str(records))], r.stdout + r.stderr
    assert r.stdout.index("verify:") < r.stdout.index("repair:")
    assert (n, records) == (len(orig), len(p.parts))
    return side


def apply(tmp_path, p: Pair, side: bytes, orig: bytes):
    (tmp_path / "in.fcx").write_bytes(p.blob)
    (tmp_path / "side").write_bytes(side)
    r = run(["-i", "in.fcx", "-o", "out", "--repair", "side"], tmp_path)
    assert r.returncode == 0, r.stdout + r.stderr
    assert (tmp_path / "out").read_bytes() == orig
    assert "SUCCESS" in r.stdout


def round_trip(tmp_path, p: Pair, orig: bytes = None):
    """build, apply, and apply again through the same repair in other sections; returns the model's rows"""
    orig = p.data if orig is None else orig
    side = build(tmp_path, p, orig)
    assert model.apply(p.parts, side) == orig   # (the model agrees with itself)
    apply(tmp_path, p, side, orig)
    for how in ("split", "merge"):
        other = model.resection(side, how)
        if other != side:
            apply(tmp_path, p, other, orig)
    return model.plan(p.parts, orig, p.block)


def test_mixed_file_gets_its_random_blocks_back(tmp_path):
    p = Pair(mixed_data(), 4096)
    rows = round_trip(tmp_path, p)
    assert [r[:4] for r in rows] == [(2, 0, 4096, model.RAW), (3, 0, 4096, model.RAW), (4, 0, 4096, model.RAW)]
    # without the sidecar nothing changes: the plain decompress still loses the three blocks
    r = run(["-i", "in.fcx", "-o", "plain"], tmp_path)
    assert (tmp_path / "plain").read_bytes() == b"".join(p.parts) and len(b"".join(p.parts)) == len(p.data) - 12288


def test_one_repeated_byte_costs_two_fill_entries(tmp_path):
    p = Pair(b"A" * 5000, 4096)
    rows = round_trip(tmp_path, p)
    assert rows == [(0, 0, 4096, model.FILL, 65, b""), (1, 0, 904, model.FILL, 65, b"")]
    assert len(p.want()) == 16 + 16 + 2 * 32 + 40


@pytest.mark.parametrize("name", ["text", "zeros", "abc", "runs"])
def test_what_comes_back_has_no_entry(tmp_path, name):
    data = {"text": text(7, 20000), "zeros": bytes(12288), "abc": b"abc" * 4000,
            "runs": b"".join(bytes([97 + i % 7]) * (50 + 37 * i) for i in range(20))}[name]
    p = Pair(data, 4096)
    assert round_trip(tmp_path, p) == []
    assert len(p.want()) == 16 + 40   # header and trailer
    assert "repair: 0 entries, 0 data bytes for %d blocks" % len(p.parts) in run(
        ["-i", "in.fcx", "--compare", "orig", "--repair", "side", "-b", "4096"], tmp_path).stdout.splitlines()


@pytest.mark.parametrize("block,lost", [(16, [0, 1, 2]), (15, []), (4097, [])])
def test_the_lossy_edge(tmp_path, block, lost):
    p = Pair(rand(11, 3 * block), block)
    assert [r[0] for r in round_trip(tmp_path, p)] == lost


def test_a_kept_block_between_lost_ones(tmp_path):
    p = Pair(rand(32, 16384), 4096)
    rows = round_trip(tmp_path, p)
    assert [r[:3] for r in rows] == [(0, 0, 4096), (2, 0, 4096), (3, 0, 4096)]


@pytest.fixture(scope="module")
def text_pair():
    return Pair(text(7, 20000), 4096)


@pytest.mark.parametrize("at", [0, 1, 15, 16, 17, 4095])
def test_edited_original_keeps_the_decoded_prefix(tmp_path, text_pair, at):
    b = bytearray(text_pair.data)
    b[2 * 4096 + at] ^= 0x5A
    rows = round_trip(tmp_path, text_pair, bytes(b))
    assert [r[:3] for r in rows] == [(2, at, 4096 - at)]
    assert rows[0][3] == (model.FILL if at == 4095 else model.RAW)


def test_original_shorter_and_longer_within_the_last_block(tmp_path, text_pair):
    rows = round_trip(tmp_path, text_pair, text_pair.data[:-100])
    assert rows == [(4, 3516, 0, model.FILL, 0, b"")]   # truncate only
    rows = round_trip(tmp_path, text_pair, text_pair.data + b"xyz" * 33 + b"x")
    assert [r[:4] for r in rows] == [(4, 3616, 100, model.RAW)]
    rows = round_trip(tmp_path, text_pair, text_pair.data + b"x" * 100)
    assert rows == [(4, 3616, 100, model.FILL, ord("x"), b"")]


def test_an_original_the_repair_cannot_express_is_an_error(tmp_path, text_pair):
    (tmp_path / "in.fcx").write_bytes(text_pair.blob)
    for orig in (text_pair.data + b"y" * 1000, text_pair.data[:8192]):   # a block too many, blocks missing
        (tmp_path / "orig").write_bytes(orig)
        r = run(["-i", "in.fcx", "--compare", "orig", "--repair", "side", "-b", "4096"], tmp_path)
        assert r.returncode not in (0, 1) and "repair" in r.stderr, r.stdout + r.stderr
        assert not REPORT.search(r.stdout)


def many_entries():
    p = Pair(rand(5, 300 * 16), 16)
    assert len(model.plan(p.parts, p.data, 16)) >= 257
    return p


def patched(side: bytes, at: int, fmt: str, value) -> bytes:
    b = bytearray(side)
    struct.pack_into(fmt, b, at, value)
    return bytes(b)


def rejected():
    """(name, pair, a repair that must be refused)"""
    p = Pair(mixed_data(), 4096)
    side = p.want()
    kind, block, groups, (n, records, _, _) = model.parse(side)
    rows = groups[0]
    first = 16 + 16   # the first entry of the first section
    yield "wrong kind", p, patched(side, 5, "<B", ord("8"))
    yield "wrong block size", p, patched(side, 8, "<I", 8192)
    yield "trailer n off by one", p, patched(side, len(side) - 32, "<Q", n + 1)
    yield "trailer records off by one", p, patched(side, len(side) - 24, "<Q", records + 1)
    yield "descending blocks", p, model.file_from_rows("7", 4096, [[rows[1], rows[0], rows[2]]], n, records)
    yield "from + len off by one", p, patched(side, first + 20, "<I", 4095)
    yield "unknown entry kind", p, patched(side, first + 24, "<I", 2)
    yield "truncated in the trailer", p, side[:-10]
    yield "truncated in a section", p, side[:16 + 16 + 3 * 32 + 5000]
    yield "bytes behind the trailer", p, side + b"\0"
    m = many_entries()
    allrows = [r for g in model.parse(m.want())[2] for r in g]
    yield "a section of 257 entries", m, model.file_from_rows("7", 16, [allrows[:257], allrows[257:]] if len(allrows) > 257
                                                              else [allrows], len(m.data), len(m.parts))


@pytest.mark.parametrize("name", [n for n, _, _ in rejected()])
def test_rejected_repairs(tmp_path, name):
    """each exits with an error status and a message, and the -o file holds nothing but bytes of the
    repaired output: a prefix of the original, never a byte past it or a wrong one"""
    p, side = next((p, s) for n, p, s in rejected() if n == name)
    (tmp_path / "in.fcx").write_bytes(p.blob)
    (tmp_path / "side").write_bytes(side)
    r = run(["-i", "in.fcx", "-o", "out", "--repair", "side"], tmp_path)
    assert r.returncode not in (0, 1), r.stdout + r.stderr
    assert re.search(r"^fcx: .*repair", r.stderr, re.M), r.stderr
    assert "SUCCESS" not in r.stdout
    out = (tmp_path / "out").read_bytes()
    assert p.data.startswith(out)


def test_many_entries_make_two_sections(tmp_path):
    m = many_entries()
    rows = round_trip(tmp_path, m)
    groups = model.parse(m.want())[2]
    assert len(groups) == 2 and [r[0] >> 8 for r in groups[1]] == [1] * len(groups[1]) and len(rows) >= 257


def test_fcx8_needs_a_device(tmp_path):
    data = b"hello hello hello\0"
    blob = oracle.lz78_compress_file(data, 1 << 20)
    (tmp_path / "x8").write_bytes(blob)
    (tmp_path / "orig").write_bytes(data)
    r = run(["-i", "x8", "--compare", "orig", "--repair", "side"], tmp_path)
    if gpu_present():
        _, parts = per_record(blob, True)
        assert (tmp_path / "side").read_bytes() == model.canonical("8", parts, data, 1 << 20), r.stdout + r.stderr
        r = run(["-i", "x8", "-o", "out", "--repair", "side"], tmp_path)
        assert r.returncode == 0 and (tmp_path / "out").read_bytes() == data
    else:
        assert r.returncode not in (0, 1) and ("HIP" in r.stderr or "GPU" in r.stderr), r.stderr
        assert not REPORT.search(r.stdout)


@pytest.mark.parametrize("extra", [["--repair", "side", "--range", "0:5"], ["--repair", "side", "--list"],
                                   ["--repair", "side", "--compare", "orig", "--list"], ["--repair"]])
def test_invalid_flag_combinations_are_usage_errors(tmp_path, text_pair, extra):
    (tmp_path / "in.fcx").write_bytes(text_pair.blob)
    (tmp_path / "orig").write_bytes(text_pair.data)
    r = run(["-i", "in.fcx", "-o", "x"] + extra, tmp_path)
    assert r.returncode not in (0, 1) and "usage:" in r.stderr
    assert not (tmp_path / "x").exists() and not (tmp_path / "side").exists()
