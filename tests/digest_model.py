"""The content digest in pure Python: what include/fcx.h says an FCXD file and a check are, restated for the
tests.

Truth is never the code under test.  The CRC-32 is zlib's; the decoded bytes of a record are the oracle
decoder's (per_record of test_range_cli.py); a repair is applied as tests/repair_model.py applies it.  From
those this writes the canonical FCXD bytes, reads them back, re-sections them, and says which blocks a check
must report and with what numbers."""
import struct
import zlib

import repair_model

HEADER_BYTES, TRAILER_BYTES, SECTION = 16, 24, 4096


def block_crcs(data: bytes, block: int):
    return [zlib.crc32(data[o:o + block]) for o in range(0, len(data), block)]


def header(block: int) -> bytes:
    return b"FCXD" + struct.pack("<BBHII", 1, 0, 0, block, 0)


def section(vals) -> bytes:
    return struct.pack("<II", len(vals), 0) + struct.pack("<%dI" % len(vals), *vals)


def trailer(n: int, blocks: int, whole: int, vals) -> bytes:
    return struct.pack("<QQII", n, blocks, whole, zlib.crc32(struct.pack("<%dI" % len(vals), *vals)))


def file_from_sections(block: int, groups, n: int, whole: int) -> bytes:
    vals = [v for g in groups for v in g]
    return header(block) + b"".join(section(g) for g in groups) + struct.pack("<II", 0, 0) + trailer(n, len(vals), whole, vals)


def canonical(data: bytes, block: int) -> bytes:
    """the FCXD file the writer must produce: sections of exactly 4096 values, but the last"""
    vals = block_crcs(data, block)
    return file_from_sections(block, [vals[i:i + SECTION] for i in range(0, len(vals), SECTION)], len(data), zlib.crc32(data))


def parse(blob: bytes):
    """(block, [sections as lists of values], (n, blocks, whole, self)) of a well-formed file"""
    assert blob[:4] == b"FCXD"
    version, z0, z1, block, z2 = struct.unpack_from("<BBHII", blob, 4)
    assert (version, z0, z1, z2) == (1, 0, 0, 0)
    q, groups = HEADER_BYTES, []
    while True:
        count, zero = struct.unpack_from("<II", blob, q)
        q += 8
        assert zero == 0
        if count == 0:
            assert q + TRAILER_BYTES == len(blob)
            return block, groups, struct.unpack_from("<QQII", blob, q)
        groups.append(list(struct.unpack_from("<%dI" % count, blob, q)))
        q += 4 * count


def resection(blob: bytes, size: int) -> bytes:
    """the same digest in sections of `size` values: other bytes, the same meaning"""
    block, groups, (n, _, whole, _) = parse(blob)
    vals = [v for g in groups for v in g]
    return file_from_sections(block, [vals[i:i + size] for i in range(0, len(vals), size)], n, whole)


def results(parts, repair: bytes = None):
    """[(resulting bytes)] per record: the decoded record, mended by its entry of the FCXR file when it has one"""
    by_block = {}
    if repair is not None:
        by_block = {r[0]: r for g in repair_model.parse(repair)[2] for r in g}
    out = []
    for k, dec in enumerate(parts):
        if k in by_block:
            _, frm, ln, kind, fill, raw = by_block[k]
            assert frm <= len(dec)
            dec = dec[:frm] + (raw if kind == repair_model.RAW else bytes([fill]) * ln)
        out.append(dec)
    return out


def check(parts, digest: bytes, repair: bytes = None):
    """(stats, rows) a check of the records must give: stats = [blocks, failing, first failing or None, wrong
    length, original bytes in failing blocks (and in digest blocks behind the last record), decoded bytes];
    rows = [(block, its length by the digest, resulting length, resulting CRC-32)] of the failing blocks, and
    last (records, bytes, 0, 0) when the digest has blocks behind the last record"""
    block, groups, (n, blocks, _, _) = parse(digest)
    want = [v for g in groups for v in g]
    rows, wrong, nbytes = [], 0, 0
    for k, res in enumerate(results(parts, repair)):
        blen = min(block, n - k * block) if k < blocks else 0
        wrong += len(res) != blen
        if k >= blocks or len(res) != blen or zlib.crc32(res) != want[k]:
            rows.append((k, blen, len(res), zlib.crc32(res)))
            nbytes += blen
    stats = [len(parts), len(rows), rows[0][0] if rows else None, wrong, nbytes, sum(len(p) for p in parts)]
    if blocks > len(parts):
        extra = n - len(parts) * block
        rows.append((len(parts), extra, 0, 0))
        stats[4] += extra
    return stats, rows
