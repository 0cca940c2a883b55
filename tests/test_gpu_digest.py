"""Content digests on the device: k_dgcrc (fcx_digest.hip) through fcx_digest_segments and fcx_digest_shard,
fcx_check_shard, their host and stream forms and the command line's --digest / --test, for FCX7 and FCX8.

Truth is never the code under test: a CRC-32 is zlib's; the decoded bytes of a record are the oracle decoder's
(per_record of test_range_cli.py); the FCXD bytes, the failing blocks and their numbers follow from those by
tests/digest_model.py, a repair by tests/repair_model.py."""
import ctypes
import io
import os
import re
import struct
import zlib

import numpy as np
import pytest

import digest_model as model
import inputs
import my_compress_amd as mc
import repair_model
from test_cli import run
from test_compare_cli import mixed_data
from test_digest_cli import LINE, VERDICT, flipped
from test_gpu_repair import Case, framed, pack, tail_zero_text
from test_range_cli import per_record

pytestmark = pytest.mark.gpu

FCX_ERR_ARG, FCX_ERR_FORMAT = -1, -4
SRC = open(os.path.join(os.path.dirname(mc.PKG_DIR), "my_compress_amd", "csrc", "fcx_digest.hip")).read()
ROWS = int(re.search(r"kDgRows = (\d+);", SRC).group(1))
THREADS = int(re.search(r"kDgThreads = (\d+);", SRC).group(1))
CHUNK = 16 * ROWS * THREADS   # bytes of a segment one k_dgcrc workgroup sums (kDgChunk)

LENGTHS = sorted({0, 1, 2, 3, 4, 5, 15, 16, 17, 31, 32, 33, 63, 64, 65, 255, 256, 257, CHUNK - 1, CHUNK, CHUNK + 1,
                  2 * CHUNK + 1, 65535, 65536, (1 << 20) - 1, 1 << 20, (1 << 20) + 8})
STARTS = (0, 1, 3, 7, 8, 13, 15)


def text(seed, n):
    return inputs.generate("text", seed, n)


def rand(seed, n):
    return inputs.generate("rand", seed, n)


@pytest.fixture(scope="module")
def dctx(cuda):
    d = mc.DContext(0)
    yield d
    d.close()


def stream():
    import torch

    return torch.cuda.current_stream().cuda_stream


def layout():
    """the packed segments: offsets (every real segment between two empty ones and behind a gap that puts its
    first byte at the wanted misalignment), and the indices of the real segments"""
    off, real, at = [0], [], 0

    def seg(n):
        nonlocal at
        at += n
        off.append(at)

    for n in LENGTHS:
        for s in STARTS:
            seg(16 + (s - at) % 16)   # a gap of poison: a segment whose value nobody looks at
            seg(0)
            real.append((len(off) - 1, at, n))
            assert at % 16 == s
            seg(n)
            seg(0)
    seg(37)
    return off, real


OFF, REAL = layout()
assert CHUNK == 65536 and len(REAL) == len(LENGTHS) * len(STARTS)


def contents(kind: str, rng) -> np.ndarray:
    """the bytes of every real segment, back to back"""
    total = sum(n for _, _, n in REAL)
    if kind == "rand":
        return rng.integers(0, 256, total, dtype=np.uint8)
    if kind in ("zeros", "ones"):
        return np.full(total, 0 if kind == "zeros" else 0xFF, dtype=np.uint8)
    a = np.zeros(total, dtype=np.uint8)   # a single set bit at the first, the last or a middle byte of each segment
    q = 0
    for _, _, n in REAL:
        if n:
            a[q + {"bit first": 0, "bit last": n - 1, "bit middle": n // 2}[kind]] = 0x10
        q += n
    return a


@pytest.mark.parametrize("kind", ["rand", "zeros", "ones", "bit first", "bit last", "bit middle"])
def test_segment_crc_against_zlib(dctx, cuda, kind):
    import torch

    body = contents(kind, np.random.default_rng(5))
    want, q = [], 0
    for _, _, n in REAL:
        want.append(zlib.crc32(body[q:q + n].tobytes()))
        q += n
    d_off = torch.tensor(OFF, dtype=torch.int64, device=cuda)
    got = []
    for poison in (0xA5, 0x3C):
        host = np.full(OFF[-1], poison, dtype=np.uint8)
        q = 0
        for _, at, n in REAL:
            host[at:at + n] = body[q:q + n]
            q += n
        d = torch.from_numpy(host).to(cuda)
        before = d.clone()
        d_crc = torch.full((len(OFF) - 1 + 2,), 0x5A5A5A5A, dtype=torch.int32, device=cuda)
        dctx.digest_segments(d.data_ptr(), d_off.data_ptr(), len(OFF) - 1, d_crc.data_ptr() + 4, stream())
        torch.cuda.synchronize()
        assert torch.equal(d, before)
        vals = d_crc.cpu().numpy().view(np.uint32)
        assert vals[0] == 0x5A5A5A5A and vals[-1] == 0x5A5A5A5A
        got.append([int(vals[1 + k]) for k, _, _ in REAL])
        assert all(vals[1 + k - 1] == 0 and vals[1 + k + 1] == 0 for k, _, _ in REAL)   # the empty neighbours
    bad = [(REAL[i][2], REAL[i][1] % 16, hex(got[0][i]), hex(want[i])) for i in range(len(REAL)) if got[0][i] != want[i]]
    assert not bad, bad[:8]
    assert got[0] == got[1]   # nothing outside a segment went into its value
    st = dctx.digest_stats()
    assert st["segments"] == len(OFF) - 1 and st["bytes"] == OFF[-1]


def test_segment_crc_slicing_variants_agree(dctx, cuda):
    import torch

    body = rand(21, OFF[-1])
    d = torch.frombuffer(bytearray(body), dtype=torch.uint8).to(cuda)
    d_off = torch.tensor(OFF, dtype=torch.int64, device=cuda)
    want = [zlib.crc32(body[OFF[k]:OFF[k + 1]]) for k in range(len(OFF) - 1)]
    try:
        for width in (8, 16, 4):
            dctx.set_digest_slice(width)
            d_crc = torch.zeros(len(OFF) - 1, dtype=torch.int32, device=cuda)
            dctx.digest_segments(d.data_ptr(), d_off.data_ptr(), len(OFF) - 1, d_crc.data_ptr(), stream())
            torch.cuda.synchronize()
            assert [int(v) for v in d_crc.cpu().numpy().view(np.uint32)] == want, width
    finally:
        dctx.set_digest_slice(0)
    bad = torch.tensor([0, 5, 3], dtype=torch.int64, device=cuda)
    assert mc.lib().fcx_digest_segments(dctx._h, ctypes.c_void_p(d.data_ptr()), ctypes.c_void_p(bad.data_ptr()), 2,
                                        ctypes.c_void_p(d.data_ptr()), None) == FCX_ERR_ARG


@pytest.mark.parametrize("block,n", [(1, 300), (7, 1000), (4096, 3 * 4096 + 5), (12293, 5 * 12293 + 77), (65536, 3 * 65536 + 1),
                                     (1 << 20, (2 << 20) + 4097)])
def test_digest_shard(dctx, cuda, block, n):
    import torch

    data = rand(block, n)
    for off in (0, 5):
        d = framed(cuda, data, off, 0xA5)
        nb = (n + block - 1) // block
        d_crc = torch.full((nb + 2,), 0x5A5A5A5A, dtype=torch.int32, device=cuda)
        whole = dctx.digest_shard(d.data_ptr() + off, n, block, d_crc.data_ptr() + 4, stream())
        vals = [int(v) for v in d_crc.cpu().numpy().view(np.uint32)]
        assert vals[0] == 0x5A5A5A5A and vals[-1] == 0x5A5A5A5A
        assert vals[1:-1] == model.block_crcs(data, block)
        assert vals[1:-1] == [mc.crc32(data[o:o + block]) for o in range(0, n, block)]   # the host mirror's
        assert whole == zlib.crc32(data) == mc.crc32(data)
    st = dctx.digest_stats()
    assert (st["segments"], st["bytes"]) == (nb, n)


def test_digest_shard_of_nothing_and_arguments(dctx, cuda):
    assert dctx.digest_shard(0, 0, 4096, 0, stream()) == 0
    lib, h = mc.lib(), dctx._h
    w = ctypes.c_uint32()
    assert lib.fcx_digest_shard(h, None, 10, 4096, None, ctypes.byref(w), None) == FCX_ERR_ARG
    assert lib.fcx_digest_shard(h, ctypes.c_void_p(16), 10, 0, ctypes.c_void_p(16), ctypes.byref(w), None) == FCX_ERR_ARG
    assert lib.fcx_digest_shard(h, ctypes.c_void_p(16), 10, (1 << 20) + 1, ctypes.c_void_p(16), ctypes.byref(w), None) == FCX_ERR_ARG
    assert mc.crc32_combine(zlib.crc32(b"abc"), zlib.crc32(b"defgh"), 5) == zlib.crc32(b"abcdefgh")


class Check:
    """a case's records and the CRC-32 of its blocks on the device"""

    def __init__(self, cuda, case: Case, data: bytes = None):
        import torch

        self.case, self.cuda = case, cuda
        self.d_rec = torch.frombuffer(bytearray(case.recs or b"\0"), dtype=torch.uint8).to(cuda)
        self.want = model.block_crcs(case.data if data is None else data, case.block)
        self.n = len(case.data if data is None else data)
        self.digest = model.canonical(case.data if data is None else data, case.block)

    def run(self, dctx, ents=(), data: bytes = b"", want=None, rc_only: bool = False):
        """(stats, rows) of fcx_check_shard, rows = [(block, resulting length, CRC-32)] of the blocks that fail by
        the pairs; the pairs of all blocks are compared with the model's by the caller"""
        import torch

        c = self.case
        want = self.want if want is None else want
        d_want = torch.tensor(want, dtype=torch.int64, device=self.cuda).to(torch.int32)
        d_e = framed(self.cuda, pack(ents), 64, 0x5A)
        d_d = framed(self.cuda, data, 37, 0x3C)
        keep = (d_e.clone(), d_d.clone(), self.d_rec.clone())
        d_b = torch.full((2 * c.n + 2,), 0x77777777, dtype=torch.int32, device=self.cuda)
        vals = (ctypes.c_uint64 * 6)()
        rc = mc.lib().fcx_check_shard(dctx._h, c.kind.encode(), ctypes.c_void_p(self.d_rec.data_ptr()), len(c.recs), c.n, self.n,
                                      c.block, ctypes.c_void_p(d_e.data_ptr() + 64), len(ents), ctypes.c_void_p(d_d.data_ptr() + 37),
                                      len(data), ctypes.c_void_p(d_want.data_ptr()), ctypes.c_void_p(d_b.data_ptr() + 4), vals,
                                      ctypes.c_void_p(stream()))
        assert torch.equal(d_e, keep[0]) and torch.equal(d_d, keep[1]) and torch.equal(self.d_rec, keep[2])
        if rc_only or rc:
            return rc
        b = d_b.cpu().numpy().view(np.uint32)
        assert b[0] == 0x77777777 and b[-1] == 0x77777777
        pairs = [(int(b[1 + 2 * k]), int(b[2 + 2 * k])) for k in range(c.n)]
        stats = mc.DContext._verify_stats(vals)
        return stats, pairs

    def agrees(self, dctx, ents=(), data: bytes = b"", repair: bytes = None, want=None):
        """fcx_check_shard says what the model says of the oracle decoder's bytes; returns the failing blocks"""
        c = self.case
        digest = self.digest if want is None else model.file_from_sections(c.block, [want], self.n, 0)
        res = model.results(c.parts, repair)
        stats, pairs = self.run(dctx, ents, data, want)
        assert pairs == [(len(r), zlib.crc32(r)) for r in res]
        mstats, rows = model.check(c.parts, digest, repair)
        assert [stats[k] for k in ("blocks", "differ", "first", "size_differs", "bytes", "decoded")] == mstats
        return [r[0] for r in rows]


def cases(kind: str):
    yield "mixed", Case(kind, mixed_data(), 4096)
    yield "one value", Case(kind, b"A" * 5000, 4096)
    yield "tail zero", Case(kind, tail_zero_text(12288, 4096), 4096)
    yield "text 3 MiB", Case(kind, text(3, 3 << 20), 1 << 20)


@pytest.mark.parametrize("name", ["mixed", "one value", "tail zero", "text 3 MiB"])
@pytest.mark.parametrize("kind", ["7", "8"])
def test_check_shard_without_and_with_the_repair(dctx, cuda, kind, name):
    c = next(x for n, x in cases(kind) if n == name)
    ck = Check(cuda, c)
    failing = ck.agrees(dctx)
    # the failing set is the differing set of the verification against the original
    d_o = framed(cuda, c.data, 0, 0xA5)
    import torch

    d_p = torch.zeros(2 * c.n, dtype=torch.int32, device=cuda)
    dctx.verify_shard(ck.d_rec.data_ptr(), len(c.recs), c.n, kind, d_o.data_ptr(), len(c.data), c.block, d_p.data_ptr(), stream())
    p = d_p.cpu().numpy().view(np.uint32)
    assert failing == [k for k in range(c.n) if p[2 * k + 1] != mc.VERIFY_SAME]
    if name == "tail zero" and kind == "8":
        assert failing == [0]
    if name == "one value" and kind == "7":
        assert failing == [0, 1]
    # with repair_build's repair nothing fails
    ents, data = repair_model.shard_repair(c.parts, c.data, c.block)
    side = repair_model.canonical(kind, c.parts, c.data, c.block)
    assert ck.agrees(dctx, ents, data, side) == []
    st = dctx.digest_stats()
    assert st["repaired"] == len(ents) and st["groups"] >= 1


@pytest.mark.parametrize("kind", ["7", "8"])
def test_tampering_fails_exactly_its_block(dctx, cuda, kind):
    base = mixed_data()
    b = bytearray(base)
    b[6 * 4096 + 100] ^= 0x55           # a RAW entry with a decoded prefix in front, whichever the codec
    b[7 * 4096 + 1000:] = b"Z" * (len(b) - 7 * 4096 - 1000)   # and a FILL entry behind its prefix
    c = Case(kind, base, 4096)
    orig = bytes(b)
    ck = Check(cuda, c, orig)
    ents, data = repair_model.shard_repair(c.parts, orig, 4096)
    side = repair_model.canonical(kind, c.parts, orig, 4096)
    assert ck.agrees(dctx, ents, data, side) == []
    raws = [e for e in ents if e[4] == repair_model.RAW]
    fills = [e for e in ents if e[4] == repair_model.FILL and e[3] > 0]
    assert raws and fills and any(e[2] > 0 for e in raws)

    def failing(ents, data, want=None):
        stats, pairs = ck.run(dctx, ents, data, want)
        w = ck.want if want is None else want
        bad = [k for k in range(c.n) if pairs[k] != (min(4096, ck.n - k * 4096), w[k])]
        assert stats["differ"] == len(bad) and stats["first"] == (bad[0] if bad else None)
        return bad

    for e in (raws[0], raws[-1]):       # one flipped RAW byte: the first and the last of an entry
        for at in (e[1], e[1] + e[3] - 1):
            d = bytearray(data)
            d[at] ^= 1
            assert failing(ents, bytes(d)) == [e[0]]
    f = fills[0]                         # one changed FILL value
    changed = [e if e != f else (f[0], f[1], f[2], f[3], f[4], f[5] ^ 1) for e in ents]
    assert failing(changed, data) == [f[0]]
    want = list(ck.want)                 # one changed expected value
    want[5] ^= 0x80000000
    assert failing(ents, data, want) == [5]


def test_a_flipped_record_fails_exactly_its_block(dctx, cuda):
    from test_digest_cli import Pair

    p = Pair(text(7, 20000), 4096)
    bad = flipped(p, 2)
    c = Case.__new__(Case)
    c.kind, c.data, c.block, c.blob = "7", p.data, 4096, bad
    _, c.parts = per_record(bad, False)
    c.recs, c.n = bad[10:], len(c.parts)
    assert Check(cuda, c).agrees(dctx) == [2]
    assert [r[0] for r in dctx.check_host(bad, p.digest)[1]] == [2]


def test_an_invalid_entry_is_a_format_error(dctx, cuda):
    c = Case("7", mixed_data(), 4096)
    ck = Check(cuda, c)
    ents, data = repair_model.shard_repair(c.parts, c.data, 4096)
    for i, change in ((0, {2: 1, 3: 4095}), (1, {4: 2}), (2, {0: c.n}), (2, {3: 4095}), (1, {1: len(data)})):
        bad = [tuple(change.get(j, v) for j, v in enumerate(e)) if k == i else e for k, e in enumerate(ents)]
        assert ck.run(dctx, bad, data, rc_only=True) == FCX_ERR_FORMAT
        msg = mc.lib().fcx_last_error().decode()
        assert f"repair: entry {i} of the records from 0 does not fit its record" == msg
    assert ck.run(dctx, [ents[1], ents[0], ents[2]], data, rc_only=True) == FCX_ERR_FORMAT
    # a record without an entry whose size is wrong is a failing block, not an error
    assert ck.agrees(dctx, ents[:1] + ents[2:], data, repair_model.file_from_rows(
        "7", 4096, [[r for r in repair_model.plan(c.parts, c.data, 4096) if r[0] != 3]], len(c.data), c.n)) == [3]
    lib, h = mc.lib(), dctx._h
    vals = (ctypes.c_uint64 * 6)()
    args = (ctypes.c_void_p(ck.d_rec.data_ptr()), len(c.recs))
    assert lib.fcx_check_shard(h, b"7", *args, c.n + 1, ck.n, 4096, None, 0, None, 0, ctypes.c_void_p(ck.d_rec.data_ptr()), None,
                               vals, None) == FCX_ERR_ARG
    assert lib.fcx_check_shard(h, b"9", *args, c.n, ck.n, 4096, None, 0, None, 0, ctypes.c_void_p(ck.d_rec.data_ptr()), None,
                               vals, None) == FCX_ERR_ARG


@pytest.mark.parametrize("kind", ["7", "8"])
def test_groups_do_not_change_the_result(dctx, cuda, kind):
    c = Case(kind, mixed_data(), 4096)
    ck = Check(cuda, c)
    ents, data = repair_model.shard_repair(c.parts, c.data, 4096)
    whole = (ck.run(dctx), ck.run(dctx, ents, data))
    assert dctx.verify_groups() == 1
    try:
        for bound, groups in ((1, c.n), (5000, None)):
            dctx.set_verify_group(bound)
            assert (ck.run(dctx), ck.run(dctx, ents, data)) == whole
            assert dctx.verify_groups() == (groups or dctx.verify_groups()) and dctx.verify_groups() > 1
            assert dctx.digest_stats()["groups"] == dctx.verify_groups()
    finally:
        dctx.set_verify_group(0)


@pytest.mark.parametrize("kind", ["7", "8"])
def test_host_and_stream_forms(dctx, cuda, kind):
    c = Case(kind, mixed_data(), 4096)
    want = model.canonical(c.data, 4096)
    assert dctx.digest_host(c.data, 4096) == want == mc.digest(c.data, 4096)
    sink = io.BytesIO()
    tr = dctx.digest_stream(io.BytesIO(c.data), sink, 4096)
    assert sink.getvalue() == want and tr == {"n": len(c.data), "blocks": c.n, "crc32": zlib.crc32(c.data)}
    p = mc.parse_digest(want)
    assert (p["block_bytes"], p["sections"], p["trailer"]["crc32"]) == (4096, model.parse(want)[1], zlib.crc32(c.data))
    assert dctx.digest_host(b"", 4096) == model.canonical(b"", 4096)
    big = rand(3, 5000)
    assert dctx.digest_host(big, 1) == model.canonical(big, 1)   # two sections
    side = repair_model.canonical(kind, c.parts, c.data, 4096)
    names = ("blocks", "differ", "first", "size_differs", "bytes", "decoded")
    for repair in (None, side):
        mstats, mrows = model.check(c.parts, want, repair)
        for stats, rows in (dctx.check_host(c.blob, want, repair), mc.check(c.blob, want, repair),
                            dctx.check_stream(io.BytesIO(c.blob), io.BytesIO(want), io.BytesIO(repair) if repair else None),
                            dctx.check_host(c.blob, model.resection(want, 3), repair)):
            assert [stats[k] for k in names] == mstats and rows == mrows
    # leftovers on either side, and files that must be refused
    longer = model.canonical(c.data + text(8, 5000), 4096)
    stats, rows = dctx.check_host(c.blob, longer, None)
    assert ([stats[k] for k in names], rows) == model.check(c.parts, longer)
    shorter = model.canonical(c.data[:8192], 4096)
    stats, rows = dctx.check_host(c.blob, shorter, None)
    assert ([stats[k] for k in names], rows) == model.check(c.parts, shorter)
    with pytest.raises(mc.FcxError, match="digest file"):
        dctx.check_host(c.blob, want[:-1], side)
    with pytest.raises(mc.FcxError, match="a value is damaged"):
        dctx.check_host(c.blob, want[:30] + bytes([want[30] ^ 1]) + want[31:], side)
    with pytest.raises(mc.FcxError, match="other codec"):
        dctx.check_host(c.blob, want, side[:5] + (b"8" if kind == "7" else b"7") + side[6:])
    with pytest.raises(mc.FcxError, match="trailer"):
        dctx.check_host(c.blob, want, side[:-32] + struct.pack("<Q", len(c.data) + 1) + side[-24:])


def test_fcx8_file_of_many_64k_records_crosses_the_stream_groups(dctx, cuda):
    block = 65536
    data = bytearray(inputs.mosaic(77, 260 * block + 999))
    for k in (3, 255, 256, 259):
        data[k * block + block - 1] = 0
        if data[k * block + block - 2] == 0:
            data[k * block + block - 2] = 1
    c = Case("8", bytes(data), block)
    short = [k for k in range(c.n) if c.sizes[k] != min(block, len(c.data) - k * block)]
    assert c.n == 261 and any(k < 256 for k in short) and any(k >= 256 for k in short)   # failing blocks in both groups
    want = model.canonical(c.data, block)
    assert dctx.digest_host(c.data, block) == want
    side = repair_model.canonical("8", c.parts, c.data, block)
    stats, rows = dctx.check_host(c.blob, want)                # the stream path reads the records as 256 + 5
    assert [r[0] for r in rows] == short and rows == model.check(c.parts, want)[1]
    ck = Check(cuda, c)
    assert ck.agrees(dctx) == short                            # the shard call over the whole run agrees
    stats, rows = dctx.check_host(c.blob, want, side)
    assert rows == [] and stats["differ"] == 0 and stats["bytes"] == 0 and stats["blocks"] == 261


@pytest.mark.parametrize("args,lz78", [(["-c", "lz77"], False), (["-c", "lz78"], True), (["-c", "lz77", "-g", "1"], False)])
def test_cli_digest_after_compress_and_test(tmp_path, cuda, args, lz78):
    data = mixed_data()
    (tmp_path / "plain").write_bytes(data)
    r = run(["-i", "plain", "-o", "comp", "-b", "4096", "--verify", "--repair", "side", "--digest", "dig"] + args, tmp_path)
    want = model.canonical(data, 4096)
    assert (tmp_path / "dig").read_bytes() == want, r.stdout + r.stderr
    assert "digest: 8 blocks, crc32 %08X" % zlib.crc32(data) in r.stdout.splitlines()
    assert r.stdout.index("verify:") < r.stdout.index("repair:") < r.stdout.index("digest:")
    blob = (tmp_path / "comp").read_bytes()
    _, parts = per_record(blob, lz78)
    side = (tmp_path / "side").read_bytes()
    for repair in (None, side):
        mstats, mrows = model.check(parts, want, repair)
        r = run(["-i", "comp", "--test", "--digest", "dig"] + (["--repair", "side"] if repair else []), tmp_path)
        rows = [(int(k), int(m), int(n), int(c, 16)) for k, n, m, c, _ in LINE.findall(r.stdout)]
        assert rows == mrows, r.stdout + r.stderr
        ok = mstats[1] == 0 and mstats[4] == 0
        assert VERDICT.findall(r.stdout) == [(str(mstats[1]), str(mstats[0]), str(mstats[4]), "OK" if ok else "FAIL")]
        assert r.returncode == (0 if ok else 1)
    r = run(["-i", "comp", "-o", "back", "--digest", "dig", "--repair", "side"], tmp_path)
    assert r.returncode == 0 and (tmp_path / "back").read_bytes() == data and "[OK]" in r.stdout, r.stdout + r.stderr
    r = run(["-i", "comp", "--compare", "plain", "--digest", "dig2", "-b", "4096"], tmp_path)
    assert (tmp_path / "dig2").read_bytes() == want


def test_one_context_for_verify_check_and_repair(dctx, cuda):
    import torch

    c = Case("7", mixed_data(), 4096)
    ck = Check(cuda, c)
    d_o = framed(cuda, c.data, 0, 0xA5)
    ents, data = repair_model.shard_repair(c.parts, c.data, 4096)
    side = repair_model.canonical("7", c.parts, c.data, 4096)
    d_e = framed(cuda, pack(ents), 0, 0x5A)
    d_d = framed(cuda, data, 0, 0x3C)
    for _ in range(2):
        st = dctx.verify_shard(ck.d_rec.data_ptr(), len(c.recs), c.n, "7", d_o.data_ptr(), len(c.data), 4096, 0, stream())
        assert (st["differ"], st["first"]) == (3, 2)
        assert ck.agrees(dctx) == [2, 3, 4]
        d_out = torch.zeros(len(c.data), dtype=torch.uint8, device=cuda)
        n = dctx.repair_apply_shard(ck.d_rec.data_ptr(), len(c.recs), c.n, "7", len(c.data), 4096, d_e.data_ptr(), len(ents),
                                    d_d.data_ptr(), len(data), d_out.data_ptr(), len(c.data), stream())
        assert n == len(c.data) and d_out.cpu().numpy().tobytes() == c.data
        assert ck.agrees(dctx, ents, data, side) == []
    dctx.set_profiling(True)
    try:
        ck.run(dctx, ents, data)
        assert [s for s, _ in dctx.stage_times()] == ["index", "decode", "digest", "summary"]
    finally:
        dctx.set_profiling(False)
