"""The repair sidecar in pure Python: what include/fcx.h says a repair is, restated for the tests.

Truth is never the code under test.  From the oracle decoder's per-record bytes (per_record of
test_range_cli.py) and the original this builds the expected entries, their data and the canonical FCXR
bytes; it applies a repair; and it re-sections a valid FCXR file (every section split into one-entry
sections, or neighbouring sections merged), which changes the bytes and must not change the result."""
import struct

SAME = 0xFFFFFFFF
RAW, FILL = 0, 1
ENTRY = struct.Struct("<QQIIII")   # block, data_off, from, len, kind, fill
HEADER_BYTES, TRAILER_BYTES, WINDOW = 16, 40, 256


def first_diff(dec: bytes, blk: bytes) -> int:
    m = min(len(dec), len(blk))
    if dec[:m] != blk[:m]:
        return next(i for i in range(m) if dec[i] != blk[i])
    return SAME if len(dec) == len(blk) else m


def plan(parts, orig: bytes, block: int):
    """[(block, from, len, kind, fill, raw bytes)] of the records that do not come back, in block order"""
    assert len(parts) == (len(orig) + block - 1) // block, "a repair cannot express missing or extra blocks"
    rows = []
    for k, dec in enumerate(parts):
        blk = orig[k * block:(k + 1) * block]
        fd = first_diff(dec, blk)
        if fd == SAME:
            continue
        rest = blk[fd:]
        assert fd <= min(len(dec), len(blk))
        if len(set(rest)) <= 1:
            rows.append((k, fd, len(rest), FILL, rest[0] if rest else 0, b""))
        else:
            rows.append((k, fd, len(rest), RAW, 0, rest))
    return rows


def shard_repair(parts, orig: bytes, block: int):
    """what fcx_repair_build_shard writes: ([(block, data_off, from, len, kind, fill)], data)"""
    ents, data = [], b""
    for k, frm, ln, kind, fill, raw in plan(parts, orig, block):
        ents.append((k, len(data) if kind == RAW else 0, frm, ln, kind, fill))
        data += raw
    return ents, data


def header(kind: str, block: int) -> bytes:
    return b"FCXR" + struct.pack("<BBHII", 1, ord(kind), 0, block, 0)


def section(rows) -> bytes:
    """rows: [(block, from, len, kind, fill, raw)]"""
    ents, data = b"", b""
    for k, frm, ln, kind, fill, raw in rows:
        ents += ENTRY.pack(k, len(data) if kind == RAW else 0, frm, ln, kind, fill)
        data += raw
    return struct.pack("<IIQ", len(rows), 0, len(data)) + ents + data


def trailer(n: int, records: int, entries: int, data_bytes: int) -> bytes:
    return struct.pack("<IIQQQQ", 0xFFFFFFFF, 0, n, records, entries, data_bytes)


def file_from_rows(kind: str, block: int, groups, n: int, records: int) -> bytes:
    """groups: the sections as lists of rows"""
    rows = [r for g in groups for r in g]
    return (header(kind, block) + b"".join(section(g) for g in groups) +
            trailer(n, records, len(rows), sum(len(r[5]) for r in rows)))


def canonical(kind: str, parts, orig: bytes, block: int) -> bytes:
    """the FCXR file the writer must produce: one section per window of 256 blocks that has entries"""
    rows = plan(parts, orig, block)
    groups = []
    for r in rows:
        if groups and groups[-1][0][0] >> 8 == r[0] >> 8:
            groups[-1].append(r)
        else:
            groups.append([r])
    return file_from_rows(kind, block, groups, len(orig), len(parts))


def parse(blob: bytes):
    """(kind, block, [sections as lists of rows], (n, records, entries, data_bytes)) of a well-formed file"""
    assert blob[:4] == b"FCXR"
    _, kind, _, block, _ = struct.unpack_from("<BBHII", blob, 4)
    q, groups = HEADER_BYTES, []
    while True:
        ne, _, nd = struct.unpack_from("<IIQ", blob, q)
        if ne == 0xFFFFFFFF:
            return chr(kind), block, groups, struct.unpack_from("<QQQQ", blob, q + 8)
        q += 16
        ents = [ENTRY.unpack_from(blob, q + 32 * i) for i in range(ne)]
        q += 32 * ne
        data = blob[q:q + nd]
        q += nd
        groups.append([(k, frm, ln, kind_, fill, data[off:off + ln] if kind_ == RAW else b"")
                       for k, off, frm, ln, kind_, fill in ents])


def resection(blob: bytes, how: str) -> bytes:
    """the same repair in other sections: "split" one entry per section, "merge" as few sections as 256
    entries each allow"""
    kind, block, groups, (n, records, _, _) = parse(blob)
    rows = [r for g in groups for r in g]
    size = 1 if how == "split" else WINDOW
    return file_from_rows(kind, block, [rows[i:i + size] for i in range(0, len(rows), size)], n, records)


def apply(parts, blob: bytes) -> bytes:
    """the decoded records mended by the FCXR file `blob`"""
    _, block, groups, (n, records, _, _) = parse(blob)
    assert records == len(parts)
    by_block = {r[0]: r for g in groups for r in g}
    out = b""
    for k, dec in enumerate(parts):
        if k in by_block:
            _, frm, ln, kind, fill, raw = by_block[k]
            assert frm <= len(dec)
            out += dec[:frm] + (raw if kind == RAW else bytes([fill]) * ln)
        else:
            out += dec
    assert len(out) == n
    return out
