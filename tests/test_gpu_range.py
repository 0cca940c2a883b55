"""Random access into device-resident runs: fcx_index_shard and the fcx_decompress_range_* calls
(fcx_range.hip, the clipped k_dlz and k78d_expand forms) for FCX7 and FCX8.

Truth is never the code under test: the streams come from the oracle's encoders, the expected sizes
and bytes from oracle.decompress_block / oracle.lz78_decompress_block per record, the framing is
walked here.  The decoded size of a record is not the block size (the FCX7 early stop,
my_compress.cpp:2331-2335; the FCX8 tail-zero rule, :3701-3703), which is what the index is for."""
import ctypes
import io
import struct

import pytest

import inputs
import my_compress_amd as mc
import oracle

pytestmark = pytest.mark.gpu

FCX_ERR_ARG, FCX_ERR_CAPACITY, FCX_ERR_FORMAT = -1, -2, -4
BLOCK_CAP = (1 << 20) + 64
LZ_STEP = 8192   # output bytes of one k_dlz step


def text(seed, n):
    return inputs.generate("text", seed, n)


def walk(blob: bytes):
    """the framing of a whole file: (records without the header, [offset of each length prefix] + [end], payloads)"""
    recs = blob[10:]
    offs, payloads, q = [], [], 0
    while q < len(recs):
        (sz,) = struct.unpack_from("<I", recs, q)
        offs.append(q)
        payloads.append(recs[q + 4:q + 4 + sz])
        q += 4 + sz
    assert q == len(recs)
    return recs, offs + [q], payloads


class Truth:
    """one file and what the oracle says about it"""

    def __init__(self, kind: str, data: bytes, block: int):
        self.kind, self.block = kind, block
        if kind == "7":
            self.blob = oracle.compress_file(data, block)
            dec = lambda p: oracle.decompress_block(p, BLOCK_CAP)
        else:
            self.blob = oracle.lz78_compress_file(data, block)
            dec = lambda p: oracle.lz78_decompress_block(p, BLOCK_CAP)
        self.recs, self.rec_off, payloads = walk(self.blob)
        self.n = len(payloads)
        parts = [dec(p) for p in payloads]
        assert all(p is not None for p in parts)
        self.sizes = [len(p) for p in parts]
        self.dec_off = [0]
        for s in self.sizes:
            self.dec_off.append(self.dec_off[-1] + s)
        self.plain = b"".join(parts)
        self.total = len(self.plain)


def golden_case(golden, name):
    case = next(c for c in golden["cases"] if c["name"] == name)
    return inputs.make(case), case["block"]


@pytest.fixture(scope="module")
def files(golden):
    F = {}
    mixed = text(7, 8192) + inputs.generate("rand", 3, 12288) + text(9, 10000)
    F["f7_mixed"] = Truth("7", mixed, 4096)
    assert F["f7_mixed"].sizes == [4096, 4096, 0, 0, 0, 4096, 4096, 1808]
    F["f7_quirk"] = Truth("7", *golden_case(golden, "quirk_text_rand_text"))
    F["f7_rand1000"] = Truth("7", *golden_case(golden, "rand_s8_100000_b1000"))
    assert F["f7_rand1000"].n == 100 and F["f7_rand1000"].total == 3000
    F["f7_runs"] = Truth("7", inputs.generate("runs", 5, 200000), 65536)
    assert F["f7_runs"].sizes == [65536, 65536, 65536, 3392]
    F["f7_mosaic"] = Truth("7", inputs.mosaic(1, 150000), 65536)
    assert F["f7_mosaic"].sizes == [65536, 65536, 18928]
    F["f7_many"] = Truth("7", text(13, 300 * 1000), 1000)   # 300 records: two groups of the stream path
    assert F["f7_many"].n == 300
    F["f8_zeros"] = Truth("8", inputs.generate("zeros", 1, 100000), 65536)
    t = bytearray(text(7, 12288)[:10001])
    t[4095] = t[8191] = t[10000] = 0
    F["f8_tail"] = Truth("8", bytes(t), 4096)
    assert F["f8_tail"].sizes == [4095, 4095, 1808]
    F["f8_batch"] = Truth("8", text(11, 300 * 256), 256)   # more records than one batch of the decoder
    assert F["f8_batch"].sizes == [256] * 300 and mc.lz78_decode_batch_records() == 256
    return F


ALL = ["f7_mixed", "f7_quirk", "f7_rand1000", "f7_runs", "f7_mosaic", "f7_many", "f8_zeros", "f8_tail", "f8_batch"]


@pytest.fixture(scope="module")
def dctx(cuda):
    d = mc.DContext(0)
    yield d
    d.close()


class Run:
    """a file's records on the device, with an index built by fcx_index_shard"""

    def __init__(self, dctx, cuda, T: Truth, recs: bytes = None):
        import torch

        self.T = T
        self.recs = T.recs if recs is None else recs
        self.d_in = torch.frombuffer(bytearray(self.recs or b"\0"), dtype=torch.uint8).to(cuda)
        self.d_rec = torch.zeros(T.n + 1, dtype=torch.int64, device=cuda)
        self.d_dec = torch.zeros(T.n + 1, dtype=torch.int64, device=cuda)
        self.stream = torch.cuda.current_stream().cuda_stream

    def index(self, dctx):
        self.total = dctx.index_shard(self.d_in.data_ptr(), len(self.recs), self.T.n, self.T.kind,
                                      self.d_rec.data_ptr(), self.d_dec.data_ptr(), self.stream)
        return self

    def range_rc(self, dctx, off, n, cap, indexed=True, kind=None, rec=None, dec=None):
        """fcx_decompress_range_shard into a buffer of cap + 64 bytes of 0xA5: (rc, out_len, the buffer's bytes)"""
        import torch

        d_out = torch.full((cap + 64,), 0xA5, dtype=torch.uint8, device=self.d_in.device)
        got = ctypes.c_uint64(0)
        rec = (self.d_rec.data_ptr() if indexed else None) if rec is None else (rec or None)
        dec = (self.d_dec.data_ptr() if indexed else None) if dec is None else (dec or None)
        rc = mc.lib().fcx_decompress_range_shard(dctx._h, (kind or self.T.kind).encode(), ctypes.c_void_p(self.d_in.data_ptr()),
                                                 len(self.recs), self.T.n, ctypes.c_void_p(rec), ctypes.c_void_p(dec),
                                                 off, n, ctypes.c_void_p(d_out.data_ptr()), cap, ctypes.byref(got),
                                                 ctypes.c_void_p(self.stream))
        return rc, got.value, d_out.cpu().numpy().tobytes()

    def check(self, dctx, off, n, indexed=True):
        """the range against the slice of the oracle's decode; nothing past it is written"""
        want = self.T.plain[off:off + n]
        cap = len(want) + 37   # (larger than needed: the bytes behind the range must stay)
        rc, got, buf = self.range_rc(dctx, off, n, cap, indexed)
        assert rc == 0, (self.T.kind, off, n, mc.lib().fcx_last_error())
        assert got == len(want), (off, n, got, len(want))
        assert buf[:got] == want, f"range ({off}, {n}) of an FCX{self.T.kind} run differs from the oracle's slice"
        assert buf[got:] == b"\xA5" * (len(buf) - got), f"range ({off}, {n}): bytes behind the range were written"


@pytest.fixture(scope="module")
def runs(files, dctx, cuda):
    return {name: Run(dctx, cuda, files[name]).index(dctx) for name in ALL}


def full_decode(dctx, run):
    import torch

    d_out = torch.zeros(run.T.total + 64, dtype=torch.uint8, device=run.d_in.device)
    fn = dctx.decompress_shard if run.T.kind == "7" else dctx.decompress_lz78_shard
    got = fn(run.d_in.data_ptr(), len(run.recs), run.T.n, d_out.data_ptr(), run.T.total + 64, run.stream)
    return d_out[:got].cpu().numpy().tobytes()


# ---- 1. the index ----
@pytest.mark.parametrize("name", ALL)
def test_index_matches_framing_and_oracle_sizes(name, runs, dctx):
    run, T = runs[name], runs[name].T
    assert run.d_rec.cpu().tolist() == T.rec_off, "rec_off is not the framing walk"
    assert run.d_dec.cpu().tolist() == T.dec_off, "dec_off is not the running sum of the oracle's record sizes"
    assert run.total == T.total
    assert len(full_decode(dctx, run)) == run.total, "*total is not the full decoder's out_len"
    run.index(dctx)   # (again, for its counters; over the arrays it filled before)
    assert dctx.range_stats() == {"sized": T.n, "expanded": 0, "stored": 0, "built_index": 0}
    assert run.d_dec.cpu().tolist() == T.dec_off


# ---- 2. the ranges every file gets ----
def common_ranges(T: Truth):
    tot = T.total
    R = [(0, 0), (0, 1), (tot - 1, 1), (tot, 5), (tot + 10, 1), (0, tot), (0, tot + 100)]
    for k in sorted(set(T.dec_off[1:-1])):   # every inner boundary (empty records share one)
        if 3 <= k:
            R.append((k - 3, 7))
    return R


@pytest.mark.parametrize("name", ALL)
def test_common_ranges_with_an_index(name, runs, dctx):
    run = runs[name]
    for off, n in common_ranges(run.T):
        run.check(dctx, off, n)
    assert dctx.range_stats()["built_index"] == 0


@pytest.mark.parametrize("name", ["f7_mixed", "f7_runs", "f8_zeros", "f8_tail", "f8_batch"])
def test_ranges_without_an_index_give_the_same_bytes(name, runs, dctx):
    run, T = runs[name], runs[name].T
    R = common_ranges(T)
    for off, n in R[:7] + R[7::max(1, (len(R) - 7) // 5)]:
        run.check(dctx, off, n, indexed=False)
        st = dctx.range_stats()
        assert st["built_index"] == 1 and st["sized"] == T.n


def test_fcx7_empty_records_inside_the_range(runs, dctx):
    run = runs["f7_mixed"]   # records 2-4 decode to nothing: bytes 8192.. are record 5's
    for off, n in [(8000, 400), (8191, 2), (8192, 1), (4000, 9000), (8192, 4096)]:
        run.check(dctx, off, n)
        run.check(dctx, off, n, indexed=False)
    run.check(dctx, 8191, 2)
    assert dctx.range_stats()["expanded"] == 5   # records 1..5: the sub-run from the first to the last touched


# ---- 3. FCX7 at 64 KiB blocks: links behind the window, the 8192-byte LZ step ----
@pytest.mark.parametrize("name", ["f7_runs", "f7_mosaic"])
def test_fcx7_deep_ranges_and_step_boundaries(name, runs, dctx):
    run, T = runs[name], runs[name].T
    d1 = T.dec_off[1]
    R = [(8190, 4), (d1 + 8191, 2), (40000, 100), (d1 + 30000, 5000), (8192, 8192), (8191, 8194),
         (60000, 10000), (d1 + 65000, 70000), (16383, 1), (16384, 1), (T.total - 3000, 2999)]
    for off, n in R:
        run.check(dctx, off, n)
    run.check(dctx, 50000, 20000, indexed=False)


def test_fcx7_early_exit_of_the_last_record(runs, dctx):
    run, T = runs["f7_runs"], runs["f7_runs"].T
    d1 = T.dec_off[1]
    run.check(dctx, d1 - 100, 110)   # ends 10 bytes into record 1
    st = dctx.range_stats()
    assert st["expanded"] == 2
    assert st["stored"] == 110 and st["stored"] <= 100 + 10 + LZ_STEP
    run.check(dctx, d1, 10)
    assert dctx.range_stats()["stored"] <= 10 + LZ_STEP


# ---- 4. FCX8: long phrases, the tail-zero rule, the batch boundary ----
def longest_phrase(data: bytes):
    """(start, length) of the longest phrase of one block's parse"""
    lens, best, pos, at = [], 0, 0, 0
    for idx, _c in oracle.lz78_parse(data):
        ln = (lens[idx - 1] if idx else 0) + 1
        lens.append(ln)
        if ln > best:
            best, at = ln, pos
        pos += ln
    assert pos in (len(data), len(data) + 1)   # (+ 1: the parse closes an open phrase with a 0x00 char)
    return at, best


def test_fcx8_ranges_inside_long_phrases(runs, dctx):
    run = runs["f8_zeros"]
    p, ln = longest_phrase(bytes(65536))
    assert ln > 300 and p + ln <= 65536   # well past the 64 bytes one lane writes
    for off, n in [(p + 70, 1), (p + 3, 200), (p + 1, ln - 2), (p + 65, ln - 130), (p - 5, 10), (p + ln - 64, 64),
                   (p + ln - 65, 2), (p + ln - 5, 10), (p, ln), (65535 - 10, 20), (65535, 1), (65530, 30000)]:
        run.check(dctx, off, n)
    run.check(dctx, p + 3, 200, indexed=False)


def test_fcx8_tail_zero_boundaries(runs, dctx):
    run = runs["f8_tail"]
    for off, n in [(4090, 10), (4094, 2), (4095, 1), (8185, 10), (8189, 2), (4000, 5000), (9990, 100), (4094, 4097)]:
        run.check(dctx, off, n)
        run.check(dctx, off, n, indexed=False)


def test_fcx8_batch_boundary(runs, dctx):
    run = runs["f8_batch"]
    run.check(dctx, 254 * 256 + 100, 3 * 256)   # record 254 into record 257
    assert dctx.range_stats()["expanded"] == 4
    run.check(dctx, 254 * 256 + 100, 3 * 256, indexed=False)
    run.check(dctx, 299 * 256 + 17, 100)         # wholly inside record 299
    st = dctx.range_stats()
    assert st == {"sized": 0, "expanded": 1, "stored": 100, "built_index": 0}
    run.check(dctx, 10, 290 * 256)               # a sub-run of more than one batch


# ---- 5. damage outside the range ----
def test_damage_outside_the_range(files, runs, dctx, cuda):
    T, good = files["f7_mixed"], runs["f7_mixed"]
    recs = bytearray(T.recs)
    a, b = T.rec_off[5] + 4, T.rec_off[6]
    recs[a:b] = b"\xFF" * (b - a)   # record 5's payload, its length prefix kept
    bad = Run(dctx, cuda, T, bytes(recs))
    bad.d_rec, bad.d_dec = good.d_rec, good.d_dec   # the index of the intact file
    bad.check(dctx, 100, 7000)                      # records 0-1
    rc, _, _ = bad.range_rc(dctx, 100, 7000, 8000, indexed=False)
    assert rc == FCX_ERR_FORMAT
    rc, _, buf = bad.range_rc(dctx, 8000, 1000, 2000)   # touches record 5
    assert rc == FCX_ERR_FORMAT
    assert buf == b"\xA5" * len(buf)
    good.check(dctx, 8000, 1000)   # the context is as good as before


# ---- 6. errors ----
def test_errors(files, runs, dctx, cuda):
    import torch

    for name in ("f7_mixed", "f8_tail"):
        run, T = runs[name], runs[name].T
        rc, got, buf = run.range_rc(dctx, 5, 100, 99)
        assert (rc, got) == (FCX_ERR_CAPACITY, 100) and buf == b"\xA5" * len(buf)
        assert run.range_rc(dctx, 5, 100, 100)[0] == 0
        assert run.range_rc(dctx, 5, 100, 200, kind="9")[0] == FCX_ERR_ARG
        assert run.range_rc(dctx, 5, 100, 200, rec=0, dec=run.d_dec.data_ptr())[0] == FCX_ERR_ARG
        assert run.range_rc(dctx, 5, 100, 200, rec=run.d_rec.data_ptr(), dec=0)[0] == FCX_ERR_ARG
        # dec_off[k + 1] off by one for the touched record 1
        wrong = run.d_dec.clone()
        wrong[2:] += 1
        off = T.dec_off[1] + 10
        rc, _, buf = run.range_rc(dctx, off, 50, 100, dec=wrong.data_ptr())
        assert rc == FCX_ERR_FORMAT and b"index" in mc.lib().fcx_last_error()
        assert buf == b"\xA5" * len(buf)
        run.check(dctx, off, 50)
        # a rec_off that points outside the run
        wrong = run.d_rec.clone()
        wrong[1] = len(run.recs) - 2
        assert run.range_rc(dctx, off, 50, 100, rec=wrong.data_ptr())[0] == FCX_ERR_FORMAT
        # no records: total 0, an empty range
        got = ctypes.c_uint64(7)
        idx = torch.full((2,), 9, dtype=torch.int64, device=cuda)
        tot = ctypes.c_uint64(7)
        L = mc.lib()
        assert L.fcx_index_shard(dctx._h, T.kind.encode(), ctypes.c_void_p(run.d_in.data_ptr()), 0, 0,
                                 ctypes.c_void_p(idx.data_ptr()), ctypes.c_void_p(idx[1:].data_ptr()), ctypes.byref(tot),
                                 None) == 0
        assert tot.value == 0 and idx.cpu().tolist() == [0, 0]
        assert L.fcx_decompress_range_shard(dctx._h, T.kind.encode(), ctypes.c_void_p(run.d_in.data_ptr()), 0, 0, None, None,
                                            0, 10, ctypes.c_void_p(idx.data_ptr()), 16, ctypes.byref(got), None) == 0
        assert got.value == 0
    assert mc.lib().fcx_dctx_range_stats(None, None, 0) == FCX_ERR_ARG


# ---- 7. host and stream forms ----
@pytest.mark.parametrize("name", ["f7_mixed", "f7_runs", "f8_zeros", "f8_tail"])
def test_range_host(name, files, dctx):
    T = files[name]
    for off, n in [(0, T.total + 5), (T.total // 2 - 3, 1000), (T.total - 1, 1), (T.total, 4), (7, 0)]:
        assert dctx.decompress_range_host(T.blob, off, n) == T.plain[off:off + n]
    assert mc.decompress_range(T.blob, 11, 500) == T.plain[11:511]


class Counting(io.BytesIO):
    def __init__(self, b):
        super().__init__(b)
        self.count = 0

    def readinto(self, b):
        n = super().readinto(b)
        self.count += n
        return n


@pytest.mark.parametrize("name", ["f7_many", "f8_batch"])
def test_range_stream_reads_no_further_than_the_range(name, files, dctx):
    T = files[name]   # 300 records: a group of 256 and one of 44
    src, sink = Counting(T.blob), io.BytesIO()
    assert dctx.decompress_range_stream(src, sink, 1000, 5000) == 5000
    assert sink.getvalue() == T.plain[1000:6000]
    assert src.count == 10 + T.rec_off[256] < len(T.blob)   # the header and the first group
    lo = T.dec_off[250] + 5
    src, sink = Counting(T.blob), io.BytesIO()   # across the group boundary
    assert dctx.decompress_range_stream(src, sink, lo, T.dec_off[260] - lo) == T.dec_off[260] - lo
    assert sink.getvalue() == T.plain[lo:T.dec_off[260]] and src.count == len(T.blob)
    src, sink = Counting(T.blob), io.BytesIO()   # past the end: everything read, nothing written
    assert dctx.decompress_range_stream(src, sink, T.total + 1, 10) == 0 and sink.getvalue() == b""


# ---- 8. the full decode is what it was ----
def test_full_decode_unchanged_after_range_calls(runs, cuda):
    fresh, used = mc.DContext(0), mc.DContext(0)
    try:
        for name in ("f7_runs", "f7_mixed", "f8_zeros", "f8_batch"):
            run = runs[name]
            run.check(used, run.T.total // 3, 5000)
            run.check(used, run.T.total // 3, 5000, indexed=False)
            assert full_decode(used, run) == run.T.plain
            if run.T.kind == "7":
                stats = used.symbol_stats()
                assert full_decode(fresh, run) == run.T.plain
                assert stats == fresh.symbol_stats()
    finally:
        fresh.close()
        used.close()
