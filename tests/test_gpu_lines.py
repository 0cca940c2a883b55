"""Line access on device-resident runs: fcx_lines_index_shard, fcx_lines_locate_shard, fcx_decompress_lines_shard,
fcx_lines_of_shard and their host and stream forms (fcx_lines.hip: k_lcount, k_lbase, k_lrank, k_lselect) for
FCX7 and FCX8.

Truth is never the code under test: the files come from the oracle's encoders, `plain` is the join of the
oracle's decode of every record (Truth of test_gpu_range.py), and every expectation is bytes.count / bytes.split
over it (lines_model.py).

The files are the six of test_gpu_find.py and crafted ones: text with the delimiter planted where the kernels
change path (lines_model.crafted: the run's ends, record seams, the seams of k_lcount's chunks, 15 / 16 within a
piece, 40 empty lines across a record seam, the traps of a word-wise count, a line longer than a record and than
a group under the bound 3000), for each of the delimiters 0x0A, 0x00, 0xFF, 0x80, 0x20, with every plant asserted
in `plain`; a file without a delimiter; and the zeros file with 0x00, where every byte is a delimiter.  Every
call, the host and stream forms included, runs under the group bounds 0, 1 and 3000 (the module-level functions
make their own context and run at the default).  f7_many and f8_batch make 100 to 300 decode groups of a call
under a bound (some 50 ms a call), so there they get one delimiter and a shorter list of calls."""
import ctypes
import pathlib

import pytest

import find_model
import inputs
import lines_model as model
import my_compress_amd as mc
from test_gpu_range import Truth

pytestmark = pytest.mark.gpu

ARG, CAPACITY, FORMAT = r"\(-1\)", r"\(-2\)", r"\(-4\)"
GROUPS = [0, 1, 3000]
CANARY = 0x5A5A5A5A5A5A5A5A
U64_MAX = model.U64_MAX
CHUNK = model.chunk_bytes(pathlib.Path(__file__).resolve().parent.parent)
STANDARD = ["f7_mixed", "f7_runs", "f7_many", "f8_zeros", "f8_tail", "f8_batch"]
CRAFTED = ["c7_%02x" % d for d in model.DELIMS] + ["c8_0a", "c8_ff", "c7_none"]
NAMES = STANDARD + CRAFTED


@pytest.fixture(scope="module")
def files():
    F = {}
    F["f7_mixed"] = Truth("7", find_model.mixed_data(), 4096)
    assert F["f7_mixed"].sizes == [4096, 4096, 0, 0, 0, 4096, 4096, 1808]
    F["f7_runs"] = Truth("7", inputs.generate("runs", 5, 200000), 65536)
    assert F["f7_runs"].sizes == [65536, 65536, 65536, 3392]
    F["f7_many"] = Truth("7", model.text(13, 300 * 1000), 1000)
    assert F["f7_many"].sizes == [1000] * 300
    F["f8_zeros"] = Truth("8", inputs.generate("zeros", 1, 100000), 65536)
    assert F["f8_zeros"].total == 100000
    t = bytearray(model.text(7, 12288)[:10001])
    t[4095] = t[8191] = t[10000] = 0
    F["f8_tail"] = Truth("8", bytes(t), 4096)
    assert F["f8_tail"].sizes == [4095, 4095, 1808]
    F["f8_batch"] = Truth("8", model.text(11, 300 * 256), 256)
    assert F["f8_batch"].sizes == [256] * 300
    for name in CRAFTED[:-1]:
        d = int(name[3:], 16)
        data, at = model.crafted(d, CHUNK)
        T = F[name] = Truth(name[1], data, 5000)
        assert T.sizes == [5000] * 4 and T.plain == data
        assert all(T.plain[p] == d for p in at) and model.nl(T.plain, d) == len(at) == 114   # no plant was lost
        assert {0, T.total - 1, 4999, 5000, 15, 16, CHUNK - 1, CHUNK, 5000 + CHUNK - 1, 5000 + CHUNK} <= set(at)
        assert max(len(x) for x in model.lines(T.plain, d)) == 7836   # longer than a record, and than a group of 3000
        T.delims = [d]
    F["c7_none"] = Truth("7", model.plant(model.text(3, 5000), 0x0A, []), 4096)
    assert F["c7_none"].sizes == [4096, 904] and model.stats(F["c7_none"].plain, 0x0A) == [0, 1, 5000, 5000]
    F["c7_none"].delims = [0x0A]
    F["f8_zeros"].delims = [0x00, 0x0A]   # every byte a delimiter (Truth decides T: the tail-zero rule included), and none
    assert model.stats(F["f8_zeros"].plain, 0) == [100000, 100000, 100000, 0]
    for name in ("f7_mixed", "f7_runs", "f8_tail"):
        F[name].delims = model.DELIMS
    for name in ("f7_many", "f8_batch"):
        F[name].delims = [0x0A, 0x20]
    return F


@pytest.fixture(scope="module")
def dctx(cuda):
    d = mc.DContext(0)
    yield d
    d.set_verify_group(0)
    d.close()


class Dev:
    """a file's records on the device, and its index"""

    def __init__(self, cuda, T: Truth, recs: bytes = None):
        import torch

        self.T, self.cuda = T, cuda
        self.recs = T.recs if recs is None else recs
        self.d_in = torch.frombuffer(bytearray(self.recs), dtype=torch.uint8).to(cuda)
        self.run = (T.kind, self.d_in.data_ptr(), len(self.recs), T.n)
        self._index = {}

    def u64(self, values):
        import torch

        return torch.tensor(list(values), dtype=torch.int64, device=self.cuda)

    def line_index(self, dctx, d: int):
        """(stats, the n + 1 values, the canaries around them) of fcx_lines_index_shard"""
        import torch

        buf = torch.full((self.T.n + 1 + 16,), CANARY, dtype=torch.int64, device=self.cuda)
        st = dctx.lines_index_shard(*self.run, delim=d, d_line_off=buf.data_ptr() + 64)
        got = buf.cpu().tolist()
        return st, got[8:-8], got[:8] + got[-8:]

    def index(self, dctx, d: int):
        """the three device arrays of the run for delimiter d (made once, under the group bound of the moment)"""
        if d not in self._index:
            import torch

            ro = torch.zeros(self.T.n + 1, dtype=torch.int64, device=self.cuda)
            do = torch.zeros(self.T.n + 1, dtype=torch.int64, device=self.cuda)
            lo = torch.zeros(self.T.n + 1, dtype=torch.int64, device=self.cuda)
            dctx.index_shard(self.d_in.data_ptr(), len(self.recs), self.T.n, self.T.kind, ro.data_ptr(), do.data_ptr())
            dctx.lines_index_shard(*self.run, delim=d, d_line_off=lo.data_ptr())
            self._index[d] = (ro, do, lo)
        return self._index[d]

    def ptrs(self, dctx, d: int):
        return tuple(t.data_ptr() for t in self.index(dctx, d))


@pytest.fixture(scope="module")
def devs(files, cuda):
    return {name: Dev(cuda, T) for name, T in files.items()}


def delims_of(T, group):
    return T.delims[:1] if group and T.n > 8 else T.delims


def seam_line(T, d):
    """the line that holds the byte in front of a record seam in the middle of the run"""
    return model.nl(T.plain, d, max(T.dec_off[(T.n + 1) // 2] - 1, 0))


# ---- 1. the line column of the index ----
@pytest.mark.parametrize("group", GROUPS)
@pytest.mark.parametrize("name", NAMES)
def test_index(name, group, files, devs, dctx):
    T, dev = files[name], devs[name]
    dctx.set_verify_group(group)
    try:
        for d in delims_of(T, group):
            st, got, around = dev.line_index(dctx, d)
            want = model.line_off(T.plain, d, T.dec_off)
            assert got == want, (name, group, hex(d), [(k, a, b) for k, (a, b) in enumerate(zip(got, want)) if a != b][:5])
            assert around == [CANARY] * 16, "entries around d_line_off[0, nblocks] were written"
            assert [st[k] for k in mc.DContext.LINES_STATS] == model.stats(T.plain, d), (name, group, hex(d))
            cs = dctx.lines_stats()
            assert cs["bytes_counted"] == T.total and cs["records"] == T.n, (name, group, hex(d), cs)   # no byte twice or skipped
            assert cs["groups"] == dctx.verify_groups() and cs["offsets_ranked"] == T.n + 1 and cs["selects"] == 0
            assert dctx.lines_index_shard(*dev.run, delim=d) == st   # NULL: the counts alone
            assert dctx.lines_stats()["bytes_counted"] == T.total
        if group == 1:
            assert dctx.verify_groups() == T.n   # every record a group
    finally:
        dctx.set_verify_group(0)


# ---- 2. locate, with and without a given index ----
def locate_cases(T, d, light):
    L = model.stats(T.plain, d)[1]
    s = seam_line(T, d)
    firsts = [0, 1, s, L - 1, L, L + 5]
    if light:
        return [(0, 1), (s, 2), (1, U64_MAX), (L - 1, 1), (L, 5), (s, 0)]
    return [(f, c) for f in sorted({f for f in firsts if f >= 0}) for c in (0, 1, 2, max(s - f + 1, 3), U64_MAX)]


@pytest.mark.parametrize("group", GROUPS)
@pytest.mark.parametrize("name", NAMES)
def test_locate(name, group, files, devs, dctx):
    T, dev = files[name], devs[name]
    dctx.set_verify_group(group)
    try:
        for d in delims_of(T, group):
            index = dev.ptrs(dctx, d)
            for first, count in locate_cases(T, d, bool(group) and T.n > 8):
                want = model.locate(T.plain, d, first, count)
                assert dctx.lines_locate_shard(*dev.run, first, count, delim=d) == want, (name, group, hex(d), first, count)
                cs = dctx.lines_stats()
                assert cs["bytes_counted"] <= T.total and cs["groups"] <= dctx.verify_groups()
                assert dctx.lines_locate_shard(*dev.run, first, count, delim=d, index=index) == want, (name, group, hex(d), first, count, "index")
                cs = dctx.lines_stats()
                assert cs["records"] <= 2 and cs["groups"] <= 2 and cs["selects"] <= 2, cs   # two records at most are decoded
    finally:
        dctx.set_verify_group(0)


@pytest.mark.parametrize("group", GROUPS)
def test_locate_stops_behind_the_second_boundary(group, files, devs, dctx):
    T, dev = files["c7_0a"], devs["c7_0a"]
    dctx.set_verify_group(group)   # under a bound every record of 5000 bytes is a group; without one the run is
    try:
        assert dctx.lines_locate_shard(*dev.run, 0, 3) == model.locate(T.plain, 0x0A, 0, 3)   # both boundaries in record 0
        assert dctx.lines_stats()["groups"] == 1 and dctx.lines_stats()["bytes_counted"] == (5000 if group else T.total)
        assert dctx.lines_locate_shard(*dev.run, 0, None) == (0, T.total)   # "to the end": no rank that large, nothing decoded
        assert dctx.lines_stats()["groups"] == 0
        assert dctx.lines_locate_shard(*dev.run, 3, None) == model.locate(T.plain, 0x0A, 3, U64_MAX)
        assert dctx.lines_stats()["groups"] == 1
    finally:
        dctx.set_verify_group(0)


def damaged(T, k):
    """the records with record k's payload overwritten, its length prefix kept"""
    recs = bytearray(T.recs)
    a, b = T.rec_off[k] + 4, T.rec_off[k + 1]
    recs[a:b] = b"\xFF" * (b - a)
    return bytes(recs)


@pytest.mark.parametrize("group", GROUPS)
def test_a_damaged_record_fails_only_the_calls_that_touch_it(group, files, devs, cuda, dctx):
    dctx.set_verify_group(group)
    try:
        damaged_record_calls(files, devs, cuda, dctx, group)
    finally:
        dctx.set_verify_group(0)


def damaged_record_calls(files, devs, cuda, dctx, group):
    T, good = files["f7_mixed"], devs["f7_mixed"]
    d = 0x0A
    index = good.ptrs(dctx, d)   # the index of the undamaged run
    bad = Dev(cuda, T, damaged(T, 5))
    s = model.nl(T.plain, d, 4096)   # a line across the seam of records 0 and 1
    want = model.locate(T.plain, d, s, 2)
    assert want[0] < 4096 < want[0] + want[1] < 8192
    assert dctx.lines_locate_shard(*bad.run, s, 2, delim=d, index=index) == want   # record 5 is not touched
    assert dctx.lines_stats()["records"] <= 2
    import torch

    out = torch.full((want[1] + 8,), 0xEE, dtype=torch.uint8, device=cuda)
    assert dctx.decompress_lines_shard(*bad.run, s, 2, out.data_ptr(), want[1], delim=d, index=index) == want[1]
    assert bytes(out.cpu().tolist()) == T.plain[want[0]:want[0] + want[1]] + b"\xEE" * 8
    in5 = model.nl(T.plain, d, 10000)   # a line that starts in record 5
    assert 8192 <= model.starts(T.plain, d)[in5] < 10000
    calls = [lambda: dctx.lines_locate_shard(*bad.run, in5, 1, delim=d),   # no index: the call makes its own and decodes record 5
             lambda: dctx.lines_index_shard(*bad.run, delim=d),
             lambda: dctx.lines_locate_shard(*bad.run, in5, 1, delim=d, index=index)]
    if group == 0:   # one group holds every record: the lines of records 0 and 1 need record 5 decoded too
        calls.append(lambda: dctx.lines_locate_shard(*bad.run, s, 2, delim=d))
    for call in calls:
        with pytest.raises(mc.FcxError, match=FORMAT):
            call()
    assert dctx.lines_locate_shard(*good.run, s, 2, delim=d) == want   # the context is as good as before


@pytest.mark.parametrize("group", GROUPS)
def test_an_index_that_lies_is_a_format_error(group, files, devs, dctx):
    dctx.set_verify_group(group)
    try:
        lying_index_calls(files, devs, dctx)
    finally:
        dctx.set_verify_group(0)


def lying_index_calls(files, devs, dctx):
    T, dev = files["c7_0a"], devs["c7_0a"]
    d = 0x0A
    ro, do, lo = dev.index(dctx, d)
    true_lo = model.line_off(T.plain, d, T.dec_off)
    first = true_lo[1] + 2   # a line of record 1 ...
    assert true_lo[1] + 2 < true_lo[2]
    assert dctx.lines_locate_shard(*dev.run, first, 1, delim=d, index=(ro.data_ptr(), do.data_ptr(), lo.data_ptr())) == \
        model.locate(T.plain, d, first, 1)
    lie = lo.clone()
    lie[1:] += 5   # ... that the line column now promises of record 0: it holds 5 delimiters fewer than that
    with pytest.raises(mc.FcxError, match=FORMAT):
        dctx.lines_locate_shard(*dev.run, first, 1, delim=d, index=(ro.data_ptr(), do.data_ptr(), lie.data_ptr()))
    few = lo.clone()
    few[1] -= 1    # record 0 holds one more than the column says: the count of the touched record shows it
    with pytest.raises(mc.FcxError, match=FORMAT):
        dctx.lines_locate_shard(*dev.run, 2, 1, delim=d, index=(ro.data_ptr(), do.data_ptr(), few.data_ptr()))
    down = lo.clone()
    down[2] = 0    # does not ascend
    with pytest.raises(mc.FcxError, match=FORMAT):
        dctx.lines_locate_shard(*dev.run, 2, 1, delim=d, index=(ro.data_ptr(), do.data_ptr(), down.data_ptr()))
    short = do.clone()
    short[1] -= 10   # record 0 decodes to 10 bytes more than the index says
    with pytest.raises(mc.FcxError, match=FORMAT):
        dctx.lines_locate_shard(*dev.run, 2, 1, delim=d, index=(ro.data_ptr(), short.data_ptr(), lo.data_ptr()))
    far = ro.clone()
    far[1:] += 1 << 40   # record offsets far outside the run: never followed
    with pytest.raises(mc.FcxError, match=FORMAT):
        dctx.lines_locate_shard(*dev.run, first, 1, delim=d, index=(far.data_ptr(), do.data_ptr(), lo.data_ptr()))
    for k in range(3):   # an array that does not start at 0: no rank may be answered from it
        arrays = [ro, do, lo]
        arrays[k] = arrays[k] + 5
        with pytest.raises(mc.FcxError, match=FORMAT):
            dctx.lines_locate_shard(*dev.run, 3, 1, delim=d, index=tuple(a.data_ptr() for a in arrays))
    assert dctx.lines_locate_shard(*dev.run, first, 1, delim=d) == model.locate(T.plain, d, first, 1)


# ---- 3. decode by lines ----
@pytest.mark.parametrize("group", GROUPS)
@pytest.mark.parametrize("name", ["f7_mixed", "f8_tail", "f7_many", "c7_0a", "c8_ff", "c7_00", "c7_none", "f8_zeros"])
def test_decompress_lines(name, group, files, devs, cuda, dctx):
    import torch

    T, dev = files[name], devs[name]
    d = T.delims[0]
    lines = model.lines(T.plain, d)
    L, s = len(lines), seam_line(T, d)
    dctx.set_verify_group(group)
    try:
        index = dev.ptrs(dctx, d)
        for first, count in ((0, 1), (s, 1), (max(s - 1, 0), 3), (L - 1, None), (L - 1, 7), (L, 1), (0, 0)):
            want = b"".join(lines[first:None if count is None else first + count])
            for idx in (None, index):
                out = torch.full((len(want) + 8,), 0xEE, dtype=torch.uint8, device=cuda)
                got = dctx.decompress_lines_shard(*dev.run, first, count, out.data_ptr(), len(want), delim=d, index=idx)   # cap exact
                assert got == len(want) and bytes(out.cpu().tolist()) == want + b"\xEE" * 8, (name, group, first, count, idx is None)
                if want:   # one short: the length is reported, nothing is written
                    n = ctypes.c_uint64(0)
                    p = [ctypes.c_void_p(x) for x in (idx or (None, None, None))]
                    out.fill_(0xEE)
                    rc = mc.lib().fcx_decompress_lines_shard(dctx._h, T.kind.encode(), ctypes.c_void_p(dev.d_in.data_ptr()), len(dev.recs),
                                                             T.n, d, *p, first, U64_MAX if count is None else count,
                                                             ctypes.c_void_p(out.data_ptr()), len(want) - 1, ctypes.byref(n), None)
                    assert rc == -2 and n.value == len(want), (name, group, first, count)
                    assert bytes(out.cpu().tolist()) == b"\xEE" * (len(want) + 8)
    finally:
        dctx.set_verify_group(0)


# ---- 4. line numbers of offsets ----
def offsets_of(dev, dctx, T, d):
    """on the device: every hit of three patterns (fcx_find_shard), 0 and T, every dec_off, every delimiter and the byte behind it;
    sorted there, duplicates kept"""
    import torch

    parts = []
    for pat in (T.plain[100:102], T.plain[T.total // 2:T.total // 2 + 5], bytes([d])):
        n = dctx.find_shard(*dev.run, pat)
        hits = torch.zeros(max(n, 1), dtype=torch.int64, device=dev.cuda)
        assert dctx.find_shard(*dev.run, pat, d_hits=hits.data_ptr(), cap=n) == n
        parts.append(hits[:n])
    where = [s - 1 for s in model.starts(T.plain, d)[1:]]
    assert len(parts[2]) == len(where)
    parts.append(dev.u64([0, T.total] + T.dec_off + [p + 1 for p in where]))
    return torch.sort(torch.cat(parts)).values


@pytest.mark.parametrize("group", GROUPS)
@pytest.mark.parametrize("name", NAMES)
def test_line_numbers(name, group, files, devs, dctx):
    import torch

    T, dev = files[name], devs[name]
    dctx.set_verify_group(group)
    try:
        for d in delims_of(T, group):
            offs = offsets_of(dev, dctx, T, d)
            n = len(offs)
            out = torch.full((n + 16,), CANARY, dtype=torch.int64, device=dev.cuda)
            dctx.lines_of_shard(*dev.run, offs.data_ptr(), n, out.data_ptr() + 64, delim=d)
            got, host = out.cpu().tolist(), offs.cpu().tolist()
            want = model.ranks(T.plain, d, host)
            assert want[:3] == [model.nl(T.plain, d, x) for x in host[:3]] and want[-1] == model.nl(T.plain, d)
            assert got[8:-8] == want, (name, group, hex(d), [(i, host[i], a, b) for i, (a, b) in enumerate(zip(got[8:-8], want)) if a != b][:5])
            assert got[:8] + got[-8:] == [CANARY] * 16
            cs = dctx.lines_stats()
            assert cs["bytes_counted"] == T.total and cs["offsets_ranked"] == n
    finally:
        dctx.set_verify_group(0)


@pytest.mark.parametrize("group", GROUPS)
def test_bad_offsets_are_named(group, files, devs, dctx):
    import torch

    T, dev = files["c7_0a"], devs["c7_0a"]
    dctx.set_verify_group(group)
    try:
        out = torch.zeros(8, dtype=torch.int64, device=dev.cuda)
        for offs, bad in (([0, 5, 9000, 8999, 20000], 3), ([0, 5, 20000, 20001], 3), ([20001], 0), ([7, 3, 20001], 1)):
            with pytest.raises(mc.FcxError, match=ARG + ".*offset %d " % bad):
                dctx.lines_of_shard(*dev.run, dev.u64(offs).data_ptr(), len(offs), out.data_ptr())
        offs = [0, 0, 5, 5, 20000, 20000]   # duplicates and the run's end are fine
        dctx.lines_of_shard(*dev.run, dev.u64(offs).data_ptr(), len(offs), out.data_ptr())
        assert out.cpu().tolist()[:6] == model.ranks(T.plain, 0x0A, offs)
    finally:
        dctx.set_verify_group(0)


# ---- 5. the host and stream forms ----
def lines_host_raw(dctx, blob: bytes, d: int, first: int, count, cap: int):
    """fcx_decompress_lines_host: (rc, out_len, the cap + 8 bytes of the buffer)"""
    out = ctypes.create_string_buffer(b"\xEE" * (cap + 8), cap + 8)
    n = ctypes.c_uint64(0)
    rc = mc.lib().fcx_decompress_lines_host(dctx._h, blob, len(blob), d, first, U64_MAX if count is None else count, out, cap,
                                            ctypes.byref(n))
    return rc, n.value, out.raw


@pytest.mark.parametrize("group", GROUPS)
@pytest.mark.parametrize("name", NAMES)
def test_host_forms(name, group, files, dctx):
    """Under a bound a stream group of up to 256 records is many decode groups, so a later stream group starts from a
    decoded base, a delimiter count and a last delimiter that are not 0 and runs several decode groups on them."""
    T = files[name]
    light = bool(group) and T.n > 8
    dctx.set_verify_group(group)
    try:
        for d in T.delims[:1] if light else T.delims[:2]:
            st = dctx.count_lines(T.blob, bytes([d]))
            assert [st[k] for k in mc.DContext.LINES_STATS] == model.stats(T.plain, d), (name, group, hex(d))
            lines = model.lines(T.plain, d)
            L, s = len(lines), seam_line(T, d)
            cases = [(s, 2), (L - 1, 3)] if light else [(0, 1), (s, 2), (max(s - 1, 0), None), (L - 1, 3), (L, None), (1, 0)]
            for first, count in cases:
                want = b"".join(lines[first:None if count is None else first + count])
                assert dctx.decompress_lines(T.blob, first, count, bytes([d])) == want, (name, group, hex(d), first, count)
                assert dctx.lines_locate(T.blob, first, count, bytes([d])) == model.locate(T.plain, d, first, U64_MAX if count is None else count)
            where = [p - 1 for p in model.starts(T.plain, d)[1:]]
            if light:   # around the seam of the stream form's groups, the run's ends and every record boundary
                near = [p for p in where if abs(p - T.dec_off[256]) < 2000]
                offs = sorted([0, T.total] + T.dec_off + near + [p + 1 for p in near])
            else:
                offs = sorted([0, T.total] + T.dec_off + where[:2000] + [p + 1 for p in where[-2000:]])
            assert dctx.line_numbers(T.blob, offs, bytes([d])) == model.ranks(T.plain, d, offs), (name, group, hex(d))
            assert dctx.line_numbers(T.blob, [], bytes([d])) == []
            with pytest.raises(mc.FcxError, match=ARG + ".*offset 1 "):
                dctx.line_numbers(T.blob, [0, T.total + 1], bytes([d]))
            # the C ABI's one-call form: exact capacity, one short, canaries
            first, count = s, 2
            want = b"".join(lines[first:first + count])
            assert lines_host_raw(dctx, T.blob, d, first, count, len(want)) == (0, len(want), want + b"\xEE" * 8)
            if want:
                assert lines_host_raw(dctx, T.blob, d, first, count, len(want) - 1) == (-2, len(want), b"\xEE" * (len(want) + 7))
    finally:
        dctx.set_verify_group(0)


@pytest.mark.parametrize("group", GROUPS)
@pytest.mark.parametrize("name", ["f7_many", "f8_batch"])
def test_a_line_across_the_stream_forms_groups(name, group, files, dctx):
    T = files[name]   # 300 records: a stream group of 256 and one of 44; under a bound each is 44 to 256 decode groups
    d, s = 0x0A, T.dec_off[256]
    j = model.nl(T.plain, d, s)
    off, n = model.locate(T.plain, d, j, 1)
    assert off < s < off + n   # line j lies across the two stream groups
    dctx.set_verify_group(group)
    try:
        # its first boundary is found in the first stream group, its second is still open when the next one starts
        assert dctx.lines_locate(T.blob, j, 1) == (off, n)
        assert dctx.decompress_lines(T.blob, j, 1) == T.plain[off:off + n]
        assert dctx.decompress_lines(T.blob, j - 1, 3) == b"".join(model.lines(T.plain, d)[j - 1:j + 2])
        ends = [x for x in T.dec_off[250:262]]   # decode-group ends inside and at the seam of the stream groups
        offs = sorted([off, s - 1, s, s + 1, off + n - 1, off + n] + ends)
        assert dctx.line_numbers(T.blob, offs) == model.ranks(T.plain, d, offs)   # file-wide numbers
        assert dctx.line_numbers(T.blob, [off, s, off + n]) == [j, j, j + 1]
        st = dctx.count_lines(T.blob)   # the last delimiter lies in the second stream group
        assert [st[k] for k in mc.DContext.LINES_STATS] == model.stats(T.plain, d) and st["tail_bytes"] < T.total - s
        if group == 0:
            pat = T.plain[s - 3:s + 3]
            assert mc.find_lines(T.blob, pat) == [(p, model.nl(T.plain, d, p)) for p in find_model.hits(T.plain, pat)]
        o2, n2 = ctypes.c_uint64(0), ctypes.c_uint64(0)
        import io

        src = io.BytesIO(T.blob)

        def rd(_u, buf, cap):
            chunk = src.read(cap)
            ctypes.memmove(buf, chunk, len(chunk))
            return len(chunk)

        assert mc.lib().fcx_lines_locate_stream(dctx._h, mc.READ_FN(rd), None, len(T.blob) - 10, d, 1, 2, ctypes.byref(o2),
                                                ctypes.byref(n2)) == 0
        assert (o2.value, n2.value) == model.locate(T.plain, d, 1, 2)
        assert src.tell() < len(T.blob)   # both boundaries lie in the first group: the second was not read
    finally:
        dctx.set_verify_group(0)


def test_module_level_calls(files):
    T = files["f7_mixed"]
    st = mc.count_lines(T.blob)
    assert [st[k] for k in mc.DContext.LINES_STATS] == model.stats(T.plain, 0x0A)
    assert mc.decompress_lines(T.blob, 3, 4) == b"".join(model.lines(T.plain, 0x0A)[3:7])
    assert mc.decompress_lines(T.blob, 2, delim=b" ") == b"".join(model.lines(T.plain, 0x20)[2:])
    assert mc.line_numbers(T.blob, [0, 8192, T.total]) == [model.nl(T.plain, 0x0A, x) for x in (0, 8192, T.total)]
    pat = T.plain[8189:8196]
    assert mc.find_lines(T.blob, pat) == [(8189, model.nl(T.plain, 0x0A, 8189))]
    with pytest.raises(ValueError):
        mc.count_lines(T.blob, delim=256)
    with pytest.raises(ValueError):
        mc.count_lines(T.blob, delim=b"ab")


# ---- 6. one context for everything ----
def test_one_context_verify_find_lines_range_lines(files, devs, cuda):
    import torch

    T, dev = files["f7_mixed"], devs["f7_mixed"]
    pat = T.plain[8189:8196]
    d = mc.DContext(0)
    try:
        orig = find_model.mixed_data()
        d_orig = torch.frombuffer(bytearray(orig), dtype=torch.uint8).to(cuda)
        st = d.verify_shard(dev.d_in.data_ptr(), len(dev.recs), T.n, "7", d_orig.data_ptr(), len(orig), 4096)
        assert st["differ"] == 3
        assert d.find_shard(*dev.run, pat) == 1
        want = model.stats(T.plain, 0x0A)
        assert [d.lines_index_shard(*dev.run)[k] for k in mc.DContext.LINES_STATS] == want
        assert d.decompress_range_host(T.blob, 8000, 400) == T.plain[8000:8400]
        assert [d.lines_index_shard(*dev.run)[k] for k in mc.DContext.LINES_STATS] == want
        for group in GROUPS:   # vf.buf is shared, and regrown or not as the bound changes
            d.set_verify_group(group)
            assert d.lines_locate_shard(*dev.run, 5, 2) == model.locate(T.plain, 0x0A, 5, 2)
            assert d.find_shard(*dev.run, pat) == 1
            assert [d.count_lines(T.blob)[k] for k in mc.DContext.LINES_STATS] == want
            assert d.decompress_lines(T.blob, 20, 5) == b"".join(model.lines(T.plain, 0x0A)[20:25])
            assert d.decompress_range_host(T.blob, 8000, 400) == T.plain[8000:8400]
    finally:
        d.close()
