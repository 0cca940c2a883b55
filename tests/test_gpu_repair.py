"""The repair sidecar on the device: fcx_repair_build_shard / fcx_repair_apply_shard (fcx_repair.hip: k_rplan,
k_rscan, k_rgather, k_rmap, k_rcheck, k_rapply), their host and stream forms and the command line's
--repair, for FCX7 and FCX8.

The records come from the GPU encoders.  Truth is never the code under test: the decoded bytes of a record
are the oracle decoder's (per_record of test_range_cli.py); the entries, their data and the canonical FCXR
bytes follow from those and the original by tests/repair_model.py.  The original, the entries, the data and
the output each sit inside a larger allocation filled with a sentinel."""
import ctypes
import io
import struct

import pytest

import inputs
import my_compress_amd as mc
import oracle
import repair_model as model
from test_cli import run
from test_compare_cli import mixed_data
from test_range_cli import per_record

pytestmark = pytest.mark.gpu

FCX_ERR_ARG, FCX_ERR_CAPACITY, FCX_ERR_FORMAT = -1, -2, -4
CHUNK = 16384   # bytes of a block one k_rgather / k_rapply workgroup copies (kRChunk)
S_ORIG, S_ENT, S_DATA, S_OUT = 0xA5, 0x5A, 0x3C, 0xC3
FRONT = 64      # sentinel bytes in front of the entries (they hold u64: 8-byte aligned)


def text(seed, n):
    return inputs.generate("text", seed, n)


def rand(seed, n):
    return inputs.generate("rand", seed, n)


def tail_zero_text(n: int, block: int, blocks=(0,), seed: int = 7) -> bytes:
    """text whose listed blocks end in 0x00: FCX8 records that decode one byte short"""
    t = bytearray(text(seed, n))
    for k in blocks:
        t[k * block + block - 1] = 0
    return bytes(t)


class Case:
    """data compressed by the GPU encoder of `kind`, and what the oracle's decoder makes of each record"""

    def __init__(self, kind: str, data: bytes, block: int):
        self.kind, self.data, self.block = kind, data, block
        self.blob = mc.compress(data, block) if kind == "7" else mc.compress_lz78(data, block)
        _, self.parts = per_record(self.blob, kind == "8")
        assert all(p is not None for p in self.parts)
        self.recs = self.blob[10:]
        self.n = len(self.parts)
        assert self.n == (len(data) + block - 1) // block
        self.sizes = [len(p) for p in self.parts]


@pytest.fixture(scope="module")
def dctx(cuda):
    d = mc.DContext(0)
    yield d
    d.close()


def framed(cuda, payload: bytes, off: int, fill: int, tail: int = 64):
    """payload at byte `off` of a device allocation otherwise filled with `fill`"""
    import torch

    t = torch.full((off + len(payload) + tail,), fill, dtype=torch.uint8, device=cuda)
    if payload:
        t[off:off + len(payload)] = torch.frombuffer(bytearray(payload), dtype=torch.uint8).to(cuda)
    return t


def all_are(t, v) -> bool:
    return bool((t == v).all().item())


def pack(ents) -> bytes:
    return b"".join(model.ENTRY.pack(*e) for e in ents)


class Run:
    """a case's records on the device"""

    def __init__(self, cuda, case: Case):
        import torch

        self.case, self.cuda = case, cuda
        self.d_rec = torch.frombuffer(bytearray(case.recs or b"\0"), dtype=torch.uint8).to(cuda)
        self.stream = torch.cuda.current_stream().cuda_stream

    def build(self, dctx, orig: bytes, off: int = 37, cap: int = None, query: bool = False):
        """(rc, entries, data, verify stats) of repair_build_shard; every sentinel is checked.  cap: the data
        capacity (default: what the model says is needed); query: d_data == NULL, data_cap == 0"""
        import torch

        c = self.case
        d_o = framed(self.cuda, orig, off, S_ORIG)
        before = d_o.clone()
        cap = len(model.shard_repair(c.parts, orig, c.block)[1]) if cap is None else cap
        d_e = torch.full((FRONT + 32 * c.n + 64,), S_ENT, dtype=torch.uint8, device=self.cuda)
        d_d = torch.full((off + cap + 64,), S_DATA, dtype=torch.uint8, device=self.cuda)
        rc, ne, nd, vst = dctx.repair_build_shard(self.d_rec.data_ptr(), len(c.recs), c.n, c.kind, d_o.data_ptr() + off,
                                                  len(orig), c.block, d_e.data_ptr() + FRONT,
                                                  0 if query else d_d.data_ptr() + off, 0 if query else cap, self.stream)
        assert torch.equal(d_o, before)   # the original is only read
        assert ne <= c.n
        assert all_are(d_e[:FRONT], S_ENT) and all_are(d_e[FRONT + 32 * ne:], S_ENT)
        wrote = nd if rc == 0 and not query else 0
        assert all_are(d_d[:off], S_DATA) and all_are(d_d[off + wrote:], S_DATA)
        ents = [tuple(e) for e in mc.unpack_repair_entries(d_e[FRONT:FRONT + 32 * ne].cpu().numpy().tobytes(), ne)]
        return rc, ents, d_d[off:off + wrote].cpu().numpy().tobytes(), vst, nd

    def apply(self, dctx, ents, data: bytes, n: int, off_data: int = 37, off_out: int = 37, nentries: int = None,
              data_bytes: int = None, cap: int = None):
        """(rc, out_len, the n bytes at d_out, the whole allocation) of fcx_repair_apply_shard"""
        import torch

        c = self.case
        d_e = framed(self.cuda, pack(ents), FRONT, S_ENT)
        d_d = framed(self.cuda, data, off_data, S_DATA)
        keep = (d_e.clone(), d_d.clone())
        cap = n if cap is None else cap
        d_out = torch.full((off_out + max(n, cap) + 64,), S_OUT, dtype=torch.uint8, device=self.cuda)
        out_len = ctypes.c_uint64(0)
        rc = mc.lib().fcx_repair_apply_shard(dctx._h, c.kind.encode(), ctypes.c_void_p(self.d_rec.data_ptr()), len(c.recs),
                                             c.n, n, c.block, ctypes.c_void_p(d_e.data_ptr() + FRONT),
                                             len(ents) if nentries is None else nentries,
                                             ctypes.c_void_p(d_d.data_ptr() + off_data),
                                             len(data) if data_bytes is None else data_bytes,
                                             ctypes.c_void_p(d_out.data_ptr() + off_out), cap, ctypes.byref(out_len),
                                             ctypes.c_void_p(self.stream))
        assert torch.equal(d_e, keep[0]) and torch.equal(d_d, keep[1])   # the repair is only read
        assert all_are(d_out[:off_out], S_OUT) and all_are(d_out[off_out + n:], S_OUT)
        return rc, int(out_len.value), d_out[off_out:off_out + n].cpu().numpy().tobytes(), d_out

    def check(self, dctx, orig: bytes = None, offs=(37, 37, 37)):
        """build against the model, then apply back to the original; offs: byte offsets of d_orig, d_data,
        d_out in their allocations.  Returns the entries."""
        c = self.case
        orig = c.data if orig is None else orig
        want_e, want_d = model.shard_repair(c.parts, orig, c.block)
        rc, ents, data, vst, nd = self.build(dctx, orig, offs[0])
        assert rc == 0 and ents == want_e and data == want_d and nd == len(want_d)
        assert vst["differ"] == len(want_e) and vst["blocks"] == c.n
        st = dctx.repair_stats()
        assert (st["entries"], st["data_bytes"]) == (len(want_e), len(want_d))
        if want_e:   # (a build without entries stops before the plan: nothing is counted)
            assert st["fills"] == sum(e[4] == model.FILL for e in want_e)
        rc, out_len, out, _ = self.apply(dctx, ents, data, len(orig), offs[1], offs[2])
        assert rc == 0, mc.lib().fcx_last_error()
        assert out_len == len(orig) and out == orig
        st = dctx.repair_stats()
        assert st["entries"] == len(want_e) and st["fills"] == sum(e[4] == model.FILL for e in want_e)
        assert st["groups_direct"] + st["groups_staged"] >= 1 and (st["groups_staged"] > 0) == bool(want_e)
        return ents


def with_suffix(data: bytes, block: int, k: int, start: int, suffix: bytes) -> bytes:
    """block k of data with its bytes from `start` on replaced by suffix (to the block's end)"""
    blen = min(block, len(data) - k * block)
    assert start + len(suffix) == blen
    return data[:k * block + start] + suffix + data[k * block + blen:]


def other(v: int) -> int:
    return v ^ 0x80


def noisy(data: bytes, block: int, k: int, start: int, seed: int) -> bytes:
    """with_suffix with random bytes whose first differs from the byte that stands there (which a record
    that comes back decodes to): the first difference is at `start`"""
    blen = min(block, len(data) - k * block)
    return with_suffix(data, block, k, start, bytes([other(data[k * block + start])]) + rand(seed, blen - start)[1:])


@pytest.mark.parametrize("kind", ["7", "8"])
def test_the_cpu_cases_on_the_device(dctx, cuda, kind):
    mixed = Case(kind, mixed_data(), 4096)
    ents = Run(cuda, mixed).check(dctx)
    if kind == "7":
        assert ents == [(2, 0, 0, 4096, 0, 0), (3, 4096, 0, 4096, 0, 0), (4, 8192, 0, 4096, 0, 0)]
    ents = Run(cuda, Case(kind, b"A" * 5000, 4096)).check(dctx)
    if kind == "7":
        assert ents == [(0, 0, 0, 4096, 1, 65), (1, 0, 0, 904, 1, 65)]   # one distinct symbol decodes as zeros
    for data in (text(7, 20000), b"abc" * 4000):
        assert Run(cuda, Case(kind, data, 4096)).check(dctx) == []
    c = Case(kind, rand(32, 16384), 4096)
    ents = Run(cuda, c).check(dctx)
    if kind == "7":
        assert [e[0] for e in ents] == [0, 2, 3]
        assert Run(cuda, Case("7", bytes(12288), 4096)).check(dctx) == []
        for block, lost in ((16, [0, 1, 2]), (15, []), (4097, [])):
            assert [e[0] for e in Run(cuda, Case("7", rand(11, 3 * block), block)).check(dctx)] == lost


def test_fcx8_block_ending_in_zero_costs_one_fill_entry(dctx, cuda):
    c = Case("8", tail_zero_text(12288, 4096), 4096)
    assert c.sizes == [4095, 4096, 4096]
    assert Run(cuda, c).check(dctx) == [(0, 0, 4095, 1, 1, 0)]


@pytest.mark.parametrize("block", [12293, 65536])
@pytest.mark.parametrize("kind", ["7", "8"])
def test_alignment_of_source_and_destination(dctx, cuda, kind, block):
    """long RAW suffixes with d_orig, d_data and d_out at byte offsets 0, 1 and 37 in every pairing of the
    funnel shift's two sides; for FCX8 a record in front decodes a byte short, which misaligns the decoded
    side as well"""
    body = text(5, 3 * block + 7)
    c = Case(kind, body if kind == "7" else tail_zero_text(block, block) + body, block)
    k0 = 0 if kind == "7" else 1
    orig = c.data
    orig = noisy(orig, block, k0, 5, 1)                # nearly the whole block
    seam = CHUNK + 1 if block > 2 * CHUNK else 4097    # just behind a chunk seam, where the block has one
    orig = noisy(orig, block, k0 + 1, seam, 2)
    orig = noisy(orig, block, c.n - 1, 3, 4)           # in the last block of 7 bytes
    r = Run(cuda, c)
    for offs in ((0, 0, 0), (1, 1, 1), (37, 37, 37), (0, 1, 37), (37, 0, 1), (1, 37, 0)):
        ents = r.check(dctx, orig, offs)
    assert [(e[0], e[2], e[4]) for e in ents if e[0] >= k0] == [(k0, 5, 0), (k0 + 1, seam, 0), (c.n - 1, 3, 0)]


def test_suffix_starts_at_the_chunk_seam(dctx, cuda):
    block = 40000
    c = Case("7", text(11, 6 * block), block)
    orig = c.data
    for k, start in enumerate((CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK - 1, 2 * CHUNK, 2 * CHUNK + 1)):
        orig = noisy(orig, block, k, start, 20 + k)
    ents = Run(cuda, c).check(dctx, orig, (1, 37, 0))
    assert [(e[0], e[2], e[3], e[4]) for e in ents] == [
        (k, s, block - s, 0) for k, s in enumerate((CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK - 1, 2 * CHUNK, 2 * CHUNK + 1))]


@pytest.mark.parametrize("block", [4096, 4099])
def test_suffix_lengths_raw_and_fill(dctx, cuda, block):
    """suffixes of 1, 15, 16, 17, 31, 32 and 33 bytes: one value except the last byte is RAW, one value
    throughout is FILL"""
    lengths = (1, 15, 16, 17, 31, 32, 33)
    c = Case("7", text(13, 2 * len(lengths) * block), block)
    orig = c.data
    for i, n in enumerate(lengths):
        for j, raw in enumerate((True, False)):
            k = 2 * i + j
            v = other(c.data[k * block + block - n])   # differs from what the record decodes to there
            suffix = bytes([v]) * n
            if raw and n > 1:
                suffix = suffix[:-1] + bytes([v ^ 1])
            orig = with_suffix(orig, block, k, block - n, suffix)
    ents = Run(cuda, c).check(dctx, orig, (37, 1, 0))
    want = []
    for i, n in enumerate(lengths):
        want += [(2 * i, block - n, n, 0 if n > 1 else 1), (2 * i + 1, block - n, n, 1)]
    assert [(e[0], e[2], e[3], e[4]) for e in ents] == want
    # a long run of one value that ends in another byte: the vote that finds it is the last one
    big = Case("7", text(17, 3 * 70000), 70000)
    v = other(big.data[70000 + 10])
    orig = with_suffix(big.data, 70000, 1, 10, bytes([v]) * (70000 - 11) + bytes([v ^ 1]))
    orig = with_suffix(orig, 70000, 2, 10, bytes([other(big.data[140010])]) * (70000 - 10))
    ents = Run(cuda, big).check(dctx, orig, (1, 0, 37))
    assert [(e[0], e[2], e[4]) for e in ents] == [(1, 10, 0), (2, 10, 1)]


def test_groups_do_not_change_the_result(dctx, cuda):
    c = Case("7", mixed_data(), 4096)
    r = Run(cuda, c)
    orig = noisy(c.data, 4096, 6, 4000, 9)
    whole = r.check(dctx, orig)
    st = dctx.repair_stats()
    assert (st["groups_direct"], st["groups_staged"]) == (0, 1)
    try:
        dctx.set_verify_group(8192)   # records 0-1 | 2-5 (three of no bytes open the group) | 6-7: direct, staged, staged
        assert r.check(dctx, orig) == whole
        st = dctx.repair_stats()
        assert (st["groups_direct"], st["groups_staged"]) == (1, 2)
        dctx.set_verify_group(3 * 4096)   # records 0-4 (the three of no bytes count one each) | 5-7: both staged
        assert r.check(dctx, orig) == whole
        st = dctx.repair_stats()
        assert (st["groups_direct"], st["groups_staged"]) == (0, 2)
        dctx.set_verify_group(1)           # every record a group of its own
        assert r.check(dctx, orig) == whole
        st = dctx.repair_stats()
        assert (st["groups_direct"], st["groups_staged"]) == (c.n - 4, 4)
    finally:
        dctx.set_verify_group(0)
    # no entry at all: one full decode straight into d_out
    t = Case("8", text(7, 20000), 4096)
    assert Run(cuda, t).check(dctx) == []
    st = dctx.repair_stats()
    assert (st["groups_direct"], st["groups_staged"]) == (1, 0)


def test_size_query_then_exact_capacity(dctx, cuda):
    c = Case("7", mixed_data(), 4096)
    r = Run(cuda, c)
    want_e, want_d = model.shard_repair(c.parts, c.data, 4096)
    rc, ents, data, _, nd = r.build(dctx, c.data, query=True)
    assert rc == FCX_ERR_CAPACITY and nd == 12288 and ents == want_e and data == b""
    rc, ents, data, _, nd = r.build(dctx, c.data, cap=nd)
    assert rc == 0 and (ents, data) == (want_e, want_d)
    rc, ents, data, _, nd = r.build(dctx, c.data, cap=12287)   # (build() checks that the data sentinel is intact)
    assert rc == FCX_ERR_CAPACITY and nd == 12288 and data == b""
    # the counts alone: no entries array, no data
    d_o = framed(cuda, c.data, 0, S_ORIG)
    got = dctx.repair_build_shard(r.d_rec.data_ptr(), len(c.recs), c.n, "7", d_o.data_ptr(), len(c.data), 4096, 0, 0, 0,
                                  r.stream)
    assert got[:3] == (0, 3, 12288)
    # a query without RAW bytes succeeds
    a = Case("7", b"A" * 5000, 4096)
    rc, ents, data, _, nd = Run(cuda, a).build(dctx, a.data, query=True)
    assert rc == 0 and nd == 0 and len(ents) == 2


def test_apply_rejects_what_does_not_fit(dctx, cuda):
    c = Case("7", mixed_data(), 4096)
    r = Run(cuda, c)
    orig = noisy(c.data, 4096, 6, 4000, 9)
    ents, data = model.shard_repair(c.parts, orig, 4096)
    assert [e[0] for e in ents] == [2, 3, 4, 6]
    n = len(orig)

    def refused(e, d=data, **kw):
        rc, _, _, d_out = r.apply(dctx, e, d, n, **kw)
        assert rc == FCX_ERR_FORMAT, rc
        assert "repair" in mc.lib().fcx_last_error().decode()
        assert all_are(d_out, S_OUT)   # nothing was written

    def change(i, **f):
        names = ("block", "data_off", "start", "len", "kind", "fill")
        e = list(ents[i])
        for k, v in f.items():
            e[names.index(k)] = v
        return ents[:i] + [tuple(e)] + ents[i + 1:]

    rc, _, out, _ = r.apply(dctx, ents, data, n)
    assert rc == 0 and out == orig
    refused(change(3, block=c.n))                       # a block behind the run
    refused(change(3, block=2 ** 40))
    refused([ents[1], ents[0]] + ents[2:])              # descending
    refused(change(1, block=2))                         # not strictly ascending
    refused(change(0, kind=2))
    refused(change(3, start=4097, len=0))               # from > decoded bytes (and the block's)
    refused(change(0, start=1, len=4095))               # record 2 decodes to 0 bytes: from > decoded
    refused(change(3, len=95))                          # from + len != the block's length
    refused(change(3, len=97))
    refused(change(2, data_off=len(data) - 4095))       # RAW range runs past the data
    refused(change(2, data_off=2 ** 63))
    refused(ents, data_bytes=len(data) - 1)
    refused(ents[:1] + ents[2:], data)                  # record 3 decodes to 0 bytes and has no entry
    assert "record 3" in mc.lib().fcx_last_error().decode()
    refused(change(1, kind=2))
    assert "entry 1" in mc.lib().fcx_last_error().decode()
    # capacity and arguments
    rc, out_len, _, d_out = r.apply(dctx, ents, data, n, cap=n - 1)
    assert rc == FCX_ERR_CAPACITY and out_len == n and all_are(d_out, S_OUT)
    lib, h = mc.lib(), dctx._h
    one = ctypes.c_uint64()
    args = (ctypes.c_void_p(r.d_rec.data_ptr()), len(c.recs))
    assert lib.fcx_repair_apply_shard(h, b"7", *args, c.n + 1, n, 4096, None, 0, None, 0, None, 0, ctypes.byref(one), None) == FCX_ERR_ARG
    assert lib.fcx_repair_apply_shard(h, b"9", *args, c.n, n, 4096, None, 0, None, 0, None, 0, ctypes.byref(one), None) == FCX_ERR_ARG
    ne, nd = ctypes.c_uint32(), ctypes.c_uint64()
    d_o = framed(cuda, orig, 0, S_ORIG)
    assert lib.fcx_repair_build_shard(h, b"7", *args, c.n - 1, ctypes.c_void_p(d_o.data_ptr()), n, 4096, None, None, 0,
                                      ctypes.byref(ne), ctypes.byref(nd), None, None) == FCX_ERR_ARG
    assert lib.fcx_repair_build_shard(h, b"7", *args, c.n, ctypes.c_void_p(d_o.data_ptr()), n, 4096, None,
                                      ctypes.c_void_p(d_o.data_ptr()), 16, ctypes.byref(ne), ctypes.byref(nd), None,
                                      None) == FCX_ERR_ARG   # d_data without d_entries


@pytest.mark.parametrize("kind", ["7", "8"])
def test_apply_and_check_refuse_the_same_entry(dctx, cuda, kind):
    """one entry map (k_rmap behind launch_entry_map) under fcx_repair_apply_shard and fcx_check_shard: each
    invalid entry gets FCX_ERR_FORMAT from both, naming the same entry.  Every record decodes to its 1000 bytes,
    and the map refuses the entries before a byte is moved."""
    import torch

    c = Case(kind, text(5, 4000), 1000)
    assert c.sizes == [1000] * 4
    r = Run(cuda, c)
    good = (0, 0, 500, 500, model.FILL, 65)
    data = bytes(16)
    table = {   # name: (entries, the index of the first invalid one)
        "block out of range": ([good, (4, 0, 500, 500, model.FILL, 65)], 1),
        "blocks not ascending": ([good, (2, 0, 500, 500, model.FILL, 65), (2, 0, 500, 500, model.FILL, 65)], 2),
        "from beyond the decoded length": ([good, (1, 0, 1001, 0, model.FILL, 0)], 1),
        "from + len is not the block's length": ([(2, 0, 500, 499, model.FILL, 65)], 0),
        "RAW range outside the data": ([good, (3, 8, 990, 10, model.RAW, 0)], 1),
        "unknown kind": ([good, (1, 0, 500, 500, 2, 0)], 1),
    }
    d_crc = torch.zeros(4, dtype=torch.int32, device=cuda)
    vals = (ctypes.c_uint64 * 6)()
    for name, (ents, bad) in table.items():
        want = f"repair: entry {bad} of the records from 0 does not fit its record"
        rc, _, _, d_out = r.apply(dctx, ents, data, 4000)
        assert rc == FCX_ERR_FORMAT and mc.lib().fcx_last_error().decode() == want, name
        assert all_are(d_out, S_OUT), name
        d_e, d_d = framed(cuda, pack(ents), FRONT, S_ENT), framed(cuda, data, 37, S_DATA)
        rc = mc.lib().fcx_check_shard(dctx._h, kind.encode(), ctypes.c_void_p(r.d_rec.data_ptr()), len(c.recs), 4, 4000, 1000,
                                      ctypes.c_void_p(d_e.data_ptr() + FRONT), len(ents), ctypes.c_void_p(d_d.data_ptr() + 37),
                                      len(data), ctypes.c_void_p(d_crc.data_ptr()), None, vals, ctypes.c_void_p(r.stream))
        assert rc == FCX_ERR_FORMAT and mc.lib().fcx_last_error().decode() == want, name


@pytest.mark.parametrize("kind", ["7", "8"])
def test_host_and_stream_forms(dctx, cuda, kind):
    c = Case(kind, mixed_data(), 4096)
    orig = noisy(c.data, 4096, 6, 4000, 9)
    want = model.canonical(kind, c.parts, orig, 4096)
    side = dctx.repair_build_host(c.blob, orig, 4096)
    assert side == want
    assert dctx.repair_apply_host(c.blob, side) == orig
    for how in ("split", "merge"):
        assert dctx.repair_apply_host(c.blob, model.resection(side, how)) == orig
    sink = io.BytesIO()
    tr = dctx.repair_build_stream(io.BytesIO(c.blob), io.BytesIO(orig), sink, 4096)
    _, _, groups, trailer = model.parse(want)
    assert sink.getvalue() == want and tuple(tr[k] for k in ("n", "records", "entries", "data_bytes")) == trailer
    out = io.BytesIO()
    assert dctx.repair_apply_stream(io.BytesIO(c.blob), io.BytesIO(side), out) == len(orig) and out.getvalue() == orig
    assert mc.repair(c.blob, orig, 4096) == want and mc.decompress_repaired(c.blob, want) == orig
    p = mc.parse_repair(want)
    assert (p["kind"], p["block_bytes"], p["trailer"]["n"], p["trailer"]["records"]) == (kind, 4096, len(orig), c.n)
    assert [[tuple(e) for e in s[0]] for s in p["sections"]] == [
        [model.ENTRY.unpack_from(model.section(g), 16 + 32 * i) for i in range(len(g))] for g in groups]
    # an original the repair cannot express
    for bad in (orig + b"x" * 5000, orig[:8192]):
        with pytest.raises(mc.FcxError, match=r"\(-1\)"):
            dctx.repair_build_host(c.blob, bad, 4096)
    # a sidecar of the other codec, and one whose trailer disagrees
    with pytest.raises(mc.FcxError, match="other codec"):
        dctx.repair_apply_host(c.blob, want[:5] + (b"8" if kind == "7" else b"7") + want[6:])
    with pytest.raises(mc.FcxError, match="trailer"):
        dctx.repair_apply_host(c.blob, want[:-32] + struct.pack("<Q", len(orig) + 1) + want[-24:], cap=len(orig) + 64)


def test_fcx8_file_of_300_records_two_sections_two_groups(dctx, cuda):
    short = (3, 100, 255, 256, 299)
    c = Case("8", tail_zero_text(300 * 4096, 4096, short, seed=13), 4096)
    assert c.n == 300 and [k for k in range(300) if c.sizes[k] == 4095] == list(short)
    want = model.canonical("8", c.parts, c.data, 4096)
    groups = model.parse(want)[2]
    assert [[r[0] for r in g] for g in groups] == [[3, 100, 255], [256, 299]]
    assert mc.repair(c.blob, c.data, 4096) == want               # the stream path reads the records as 256 + 44
    assert mc.decompress_repaired(c.blob, want) == c.data
    for how in ("split", "merge"):
        assert mc.decompress_repaired(c.blob, model.resection(want, how)) == c.data
    # the shard calls over the whole run, in groups of ten records
    try:
        dctx.set_verify_group(10 * 4096)
        ents = Run(cuda, c).check(dctx)
        assert [e[0] for e in ents] == list(short) and dctx.repair_stats()["groups_staged"] == 4   # (255 and 256 share one)
    finally:
        dctx.set_verify_group(0)


@pytest.mark.parametrize("args,lz78", [(["-c", "lz77"], False), (["-c", "lz78"], True)])
def test_cli_repair_after_compress_and_back(tmp_path, cuda, args, lz78):
    data = mixed_data()
    (tmp_path / "plain").write_bytes(data)
    r = run(["-i", "plain", "-o", "comp", "-b", "4096", "--verify", "--repair", "side"] + args, tmp_path)
    blob = (tmp_path / "comp").read_bytes()
    assert blob == (oracle.lz78_compress_file(data, 4096) if lz78 else oracle.compress_file(data, 4096))
    _, parts = per_record(blob, lz78)
    want = model.canonical("8" if lz78 else "7", parts, data, 4096)
    assert (tmp_path / "side").read_bytes() == want, r.stdout + r.stderr
    _, _, _, (n, records, entries, data_bytes) = model.parse(want)
    assert f"repair: {entries} entries, {data_bytes} data bytes for {records} blocks" in r.stdout.splitlines()
    assert r.stdout.index("<Final>:") < r.stdout.index("verify:") < r.stdout.index("repair:")
    assert r.returncode == (1 if entries else 0)   # --verify's verdict stays
    r = run(["-i", "comp", "-o", "back", "--repair", "side"], tmp_path)
    assert r.returncode == 0 and (tmp_path / "back").read_bytes() == data, r.stdout + r.stderr
    r = run(["-i", "plain", "-o", "comp2", "-b", "4096", "--repair", "side2"] + args, tmp_path)   # without --verify
    assert r.returncode == 0 and (tmp_path / "side2").read_bytes() == want and "verify:" not in r.stdout
    (tmp_path / "side").write_bytes(want[:-3])
    r = run(["-i", "comp", "-o", "back", "--repair", "side"], tmp_path)
    assert r.returncode not in (0, 1) and "repair file" in r.stderr
    assert data.startswith((tmp_path / "back").read_bytes())


def test_one_context_for_verify_range_and_repair(dctx, cuda):
    import torch

    c = Case("7", mixed_data(), 4096)
    r = Run(cuda, c)
    d_o = framed(cuda, c.data, 0, S_ORIG)
    plain = b"".join(c.parts)
    for _ in range(2):
        st = dctx.verify_shard(r.d_rec.data_ptr(), len(c.recs), c.n, "7", d_o.data_ptr(), len(c.data), 4096, 0, r.stream)
        assert (st["differ"], st["first"]) == (3, 2)
        d_part = torch.empty(5000, dtype=torch.uint8, device=cuda)
        got = dctx.decompress_range_shard(r.d_rec.data_ptr(), len(c.recs), c.n, "7", 8000, 5000, d_part.data_ptr(), 5000,
                                          stream=r.stream)
        assert d_part[:got].cpu().numpy().tobytes() == plain[8000:13000]
        r.check(dctx)
