"""Matching lines of device-resident runs and the multi-range decode: fcx_grep_shard (fcx_grep.hip: k_gscan,
k_gtiles, k_gmark, k_gbase, k_gwrite), fcx_decompress_ranges_shard (fcx_ranges.hip: k_qlen, k_qchunks, k_qoff,
k_qtouch, k_qslice, k_qgather) and the host forms, for FCX7 and FCX8.

Truth is never the code under test: the files come from the oracle's encoders, `plain` is the join of the
oracle's decode of every record (Truth of test_gpu_range.py), the expected lines are grep_model.selected over
it (lines_model.starts and find_model.hits), and every call is compared in full: the five stats, every start
and every end.  The crafted file's plants are asserted in the oracle's bytes (grep_model.check_crafted).

Every call runs under the group bounds 0, 1 and 3000.  The files of 300 records make 100 to 300 decode groups
under a bound, some 50 ms a call, so there they get the light subset: one delimiter and the patterns around the
256-record seam and at the run's ends."""
import ctypes

import pytest

import find_model as fm
import grep_model as model
import inputs
import lines_model as lm
import my_compress_amd as mc
from test_gpu_range import Truth

pytestmark = pytest.mark.gpu

FCX_ERR_ARG, FCX_ERR_CAPACITY, FCX_ERR_FORMAT = -1, -2, -4
NAMES = ["f7_mixed", "f7_runs", "f7_many", "f8_zeros", "f8_tail", "f8_batch"]
GROUPS = [0, 1, 3000]
CANARY = 0x5A5A5A5A5A5A5A5A


@pytest.fixture(scope="module")
def files():
    F = {}
    F["f7_mixed"] = Truth("7", fm.mixed_data(), 4096)
    assert F["f7_mixed"].sizes == [4096, 4096, 0, 0, 0, 4096, 4096, 1808]
    F["f7_runs"] = Truth("7", inputs.generate("runs", 5, 200000), 65536)
    assert F["f7_runs"].sizes == [65536, 65536, 65536, 3392]
    F["f7_many"] = Truth("7", fm.text(13, 300 * 1000), 1000)
    assert F["f7_many"].sizes == [1000] * 300
    F["f8_zeros"] = Truth("8", inputs.generate("zeros", 1, 100000), 65536)
    assert F["f8_zeros"].total == 100000
    t = bytearray(fm.text(7, 12288)[:10001])
    t[4095] = t[8191] = t[10000] = 0
    F["f8_tail"] = Truth("8", bytes(t), 4096)
    assert F["f8_tail"].sizes == [4095, 4095, 1808]
    F["f8_batch"] = Truth("8", fm.text(11, 300 * 256), 256)
    assert F["f8_batch"].sizes == [256] * 300
    for d in model.DELIMS:
        for kind in "78":
            T = F[f"craft{kind}_{d:02x}"] = Truth(kind, model.crafted(d), model.CRAFT_BLOCK)
            assert T.sizes == [5000] * 4
            model.check_crafted(T.plain, d)
    F["f7_nodelim"] = Truth("7", lm.plant(fm.text(5, 9000), 0x0A, []), 4096)   # no 0x0A at all: one line
    assert 0x0A not in F["f7_nodelim"].plain and F["f7_nodelim"].total == 9000
    F["f7_xdxd"] = Truth("7", b"x\n" * 4096, 4096)   # every second byte the delimiter: T / 2 lines
    assert F["f7_xdxd"].plain == b"x\n" * 4096
    F["f7_tiny"] = Truth("7", fm.text(7, 100), 4096)
    assert F["f7_tiny"].sizes == [100]
    return F


@pytest.fixture(scope="module")
def dctx(cuda):
    d = mc.DContext(0)
    yield d
    d.set_verify_group(0)
    d.close()


class Dev:
    """a file's records on the device"""

    def __init__(self, cuda, T: Truth, recs: bytes = None):
        import torch

        self.T, self.cuda = T, cuda
        self.recs = T.recs if recs is None else recs
        self.d_in = torch.frombuffer(bytearray(self.recs), dtype=torch.uint8).to(cuda)
        self.stream = torch.cuda.current_stream().cuda_stream
        self.run = (T.kind, self.d_in.data_ptr(), len(self.recs), T.n)

    def grep(self, dctx, pat: bytes, d: int, cap: int = None, room: int = None, keep: bool = False):
        """fcx_grep_shard: (stats, [(start, end)] of the first min(cap, lines), what lies behind them in the two
        arrays); cap None: room for all and 3 more (one call)"""
        import torch

        if cap is None:
            cap = dctx.grep_shard(*self.run, pat, d)["lines"] + 3
        room = cap if room is None else room
        ds = torch.full((room + 8,), CANARY, dtype=torch.int64, device=self.cuda)
        de = torch.full((room + 8,), CANARY, dtype=torch.int64, device=self.cuda)
        st = dctx.grep_shard(*self.run, pat, d, d_start=ds.data_ptr() if cap else 0, d_end=de.data_ptr() if cap else 0, cap=cap,
                             stream=self.stream)
        s, e = ds.cpu().tolist(), de.cpu().tolist()
        k = min(cap, st["lines"])
        if keep:
            self.ds, self.de = ds, de
        return [st[n] for n in mc.DContext.GREP_STATS], list(zip(s[:k], e[:k])), s[k:] + e[k:]

    def index(self, dctx):
        import torch

        ro = torch.zeros(self.T.n + 1, dtype=torch.int64, device=self.cuda)
        do = torch.zeros(self.T.n + 1, dtype=torch.int64, device=self.cuda)
        dctx.index_shard(self.d_in.data_ptr(), len(self.recs), self.T.n, self.T.kind, ro.data_ptr(), do.data_ptr())
        return ro, do

    def ranges(self, dctx, ranges, index=None, cap: int = None, raw: bool = False):
        """fcx_decompress_ranges_shard over a host list of (start, end): the bytes; raw: (rc, out_len, the whole
        output buffer with its canaries)"""
        import torch

        n = len(ranges)
        ds = torch.tensor([r[0] for r in ranges] or [0], dtype=torch.int64, device=self.cuda)
        de = torch.tensor([r[1] for r in ranges] or [0], dtype=torch.int64, device=self.cuda)
        need = sum(max(e - s, 0) for s, e in ranges)
        cap = need if cap is None else cap
        out = torch.full((cap + 64,), 0xA5, dtype=torch.uint8, device=self.cuda)
        got = ctypes.c_uint64(7)
        ix = (None, None) if index is None else (ctypes.c_void_p(index[0].data_ptr()), ctypes.c_void_p(index[1].data_ptr()))
        k, p, ln, nb = self.run
        rc = mc.lib().fcx_decompress_ranges_shard(dctx._h, k.encode(), ctypes.c_void_p(p), ln, nb, *ix, ctypes.c_void_p(ds.data_ptr()),
                                                  ctypes.c_void_p(de.data_ptr()), n, ctypes.c_void_p(out.data_ptr()) if cap else None,
                                                  cap, ctypes.byref(got), ctypes.c_void_p(self.stream))
        buf = out.cpu().numpy().tobytes()
        if raw:
            return rc, got.value, buf
        assert rc == 0, mc.lib().fcx_last_error()
        assert got.value == need and buf[need:] == b"\xA5" * (len(buf) - need), "bytes behind d_out[sum) were written"
        return buf[:need]


@pytest.fixture(scope="module")
def devs(files, cuda):
    return {name: Dev(cuda, T) for name, T in files.items()}


def patterns_of(T: Truth, d: int, light: bool):
    """the distinct patterns without the delimiter cut from plain: the seven lengths at the run's two ends, around
    the first record seam and the 256-record seam, around the tile seam; light: the two ends and the 256 seam"""
    seams = [s for s in sorted(set(T.dec_off[1:-1]))]
    at = [T.dec_off[256]] if T.n > 256 else seams[:1]
    pats = []
    for m in model.LENGTHS:
        P = [0, T.total - m] + [x for s in at for x in (s - 1, s - m + 1, s - m // 2)]
        if not light:
            P += [fm.TILE - 1, fm.TILE - m // 2, seams[-1] - m // 2 if seams else 0]
        for p in P:
            pat = model.cut(T.plain, d, p, m) if 0 <= p < T.total else None
            if pat and pat not in pats:
                pats.append(pat)
    return pats + [fm.absent(T.plain)]


def check(dev: Dev, dctx, pat: bytes, d: int, what):
    want = model.selected(dev.T.plain, pat, d)
    st, got, behind = dev.grep(dctx, pat, d, cap=len(want) + 3)
    assert st == model.stats(dev.T.plain, pat, d, want), (what, len(pat), pat[:16], st)
    assert got == want, (what, len(pat), pat[:16])
    assert behind == [CANARY] * len(behind), (what, "entries behind min(cap, lines) were written")
    return want


# ---- 1. every file, three group bounds, three delimiters ----
@pytest.mark.parametrize("group", GROUPS)
@pytest.mark.parametrize("name", NAMES)
def test_patterns_cut_from_the_decoded_bytes(name, group, files, devs, dctx):
    T, dev = files[name], devs[name]
    light = group != 0 and T.n > 8
    dctx.set_verify_group(group)
    try:
        lengths = set()
        for d in ([0x0A] if light else model.DELIMS):
            for pat in patterns_of(T, d, light):
                check(dev, dctx, pat, d, (name, group, d))
                lengths.add(len(pat))
        if name == "f8_zeros":
            assert lengths >= set(model.LENGTHS)
        if group == 1:
            assert dctx.verify_groups() == T.n   # every record a group: state words span groups shorter than the pattern
    finally:
        dctx.set_verify_group(0)


@pytest.mark.parametrize("group", GROUPS)
@pytest.mark.parametrize("kind", ["7", "8"])
@pytest.mark.parametrize("d", model.DELIMS)
def test_the_crafted_lines(d, kind, group, files, devs, dctx):
    name = f"craft{kind}_{d:02x}"
    T, dev = files[name], devs[name]
    dctx.set_verify_group(group)
    try:
        sel = check(dev, dctx, model.MARK, d, (name, group))
        assert sel == model.check_crafted(T.plain, d)
        # one pattern cut per shape, the lengths in turn
        i = 0
        for shape, at in model.CRAFT_MARKS.items():
            for p in at:
                pat = model.cut(T.plain, d, p, model.LENGTHS[i % len(model.LENGTHS)])
                i += 1
                assert pat and model.line_of(T.plain, d, p) in check(dev, dctx, pat, d, (name, group, shape))
        # empty lines are never selected, whatever is searched for: the byte in front of and behind the run of them
        for p in (99, 103):
            assert not {(101, 102), (102, 103)} & set(check(dev, dctx, T.plain[p:p + 1], d, (name, group, "empty lines")))
        if group:
            assert dctx.verify_groups() == 4
    finally:
        dctx.set_verify_group(0)


@pytest.mark.parametrize("group", GROUPS)
def test_a_line_across_the_records_of_no_bytes(group, files, devs, dctx):
    T, dev = files["f7_mixed"], devs["f7_mixed"]
    assert T.dec_off[2] == T.dec_off[5] == 8192
    s, e = model.line_of(T.plain, 0x0A, 8192)
    assert s < 8192 < e   # the line spans records 2, 3 and 4
    dctx.set_verify_group(group)
    try:
        for pat in (T.plain[8189:8196], T.plain[s:s + 4], T.plain[e - 5:e - 1]):
            assert (s, e) in check(dev, dctx, pat, 0x0A, ("f7_mixed", group, "0-byte records"))
    finally:
        dctx.set_verify_group(0)


@pytest.mark.parametrize("group", GROUPS)
def test_the_corner_files(group, files, devs, dctx):
    dctx.set_verify_group(group)
    try:
        T, dev = files["f7_nodelim"], devs["f7_nodelim"]   # no delimiter: one line, end T
        for pat in (T.plain[:3], T.plain[4094:4099], T.plain[-4:]):
            assert check(dev, dctx, pat, 0x0A, "nodelim") == [(0, T.total)]
        assert check(dev, dctx, fm.absent(T.plain), 0x0A, "nodelim, absent") == []
        T, dev = files["f8_zeros"], devs["f8_zeros"]       # T - m + 1 hits, one line
        for m in (1, 33, 256):
            st, got, _ = dev.grep(dctx, bytes(m), 0x0A, cap=4)
            assert st == [1, T.total, T.total - m + 1, T.total - m + 1, T.total] and got == [(0, T.total)]
        T, dev = files["f7_xdxd"], devs["f7_xdxd"]         # T / 2 lines
        want = check(dev, dctx, b"x", 0x0A, "xdxd")
        assert want == [(2 * i, 2 * i + 2) for i in range(4096)]
        assert check(dev, dctx, b"x", 0x00, "xdxd, no delimiter") == [(0, 8192)]
        T, dev = files["f7_tiny"], devs["f7_tiny"]         # a pattern longer than the run; exactly the run
        if 0x0A not in T.plain:
            st, got, _ = dev.grep(dctx, T.plain + b"zz", 0x0A, cap=2)
            assert st == [0, 0, 0, 0, 100] and got == []
        st, got, _ = dev.grep(dctx, lm.plant(T.plain, 0xFF, []) + bytes(156), 0xFF, cap=2)
        assert st == [0, 0, 0, 0, 100] and got == []
    finally:
        dctx.set_verify_group(0)


def test_scratch_is_bitmaps_and_tile_words(files, devs, dctx):
    """the two worst cases run in two bitmaps of group bytes / 8 and 48 bytes per tile, whatever the hits or lines"""
    for name, pat in (("f7_xdxd", b"x"), ("f8_zeros", b"\0")):
        T, dev = files[name], devs[name]
        st = dctx.grep_shard(*dev.run, pat, 0x0A)
        assert st["lines"] == (4096 if name == "f7_xdxd" else 1) and st["hits"] == (4096 if name == "f7_xdxd" else T.total)
        tiles = (T.total + 256 + 4095) // 4096   # (one group: the run and the carry's room)
        assert dctx.grep_scratch() == tiles * (2 * 512 + 48) < 8 * st["hits"]


# ---- 2. cap ----
@pytest.mark.parametrize("name,pat_at", [("craft7_0a", None), ("f7_many", (0, 1))])
def test_cap(name, pat_at, files, devs, dctx):
    T, dev = files[name], devs[name]
    pat = model.MARK if pat_at is None else T.plain[pat_at[0]:pat_at[1]]
    want = model.selected(T.plain, pat, 0x0A)
    L = len(want)
    assert L >= 3
    for group in (0, 3000) if name != "f7_many" else (0,):
        dctx.set_verify_group(group)
        try:
            for cap in (0, 1, L - 1, L, L + 8):
                st, got, behind = dev.grep(dctx, pat, 0x0A, cap=cap, room=L + 8)
                assert st == model.stats(T.plain, pat, 0x0A, want) and got == want[:cap], (name, cap)
                assert behind == [CANARY] * len(behind), f"cap {cap}: entries behind min(cap, lines) were written"
        finally:
            dctx.set_verify_group(0)


def test_cap_cuts_a_line_whose_end_comes_groups_later(files, devs, dctx):
    """the 7836-byte line is the 6th: with cap 5 its end, found two groups on, must not be stored; with cap 6 it must"""
    T, dev = files["craft8_0a"], devs["craft8_0a"]
    want = model.selected(T.plain, model.MARK, 0x0A)
    dctx.set_verify_group(1)
    try:
        for cap in (5, 6):
            st, got, behind = dev.grep(dctx, model.MARK, 0x0A, cap=cap, room=9)
            assert got == want[:cap] and behind == [CANARY] * len(behind) and st[0] == 7
    finally:
        dctx.set_verify_group(0)


# ---- 3. chained on the device ----
@pytest.mark.parametrize("name", ["craft7_0a", "f7_many", "f8_batch", "f7_mixed"])
def test_starts_chain_into_line_numbers_and_both_into_the_ranges_decode(name, files, devs, dctx, cuda):
    import torch

    T, dev = files[name], devs[name]
    pat = model.MARK if name.startswith("craft") else T.plain[100:102]
    assert 0x0A not in pat
    want = model.selected(T.plain, pat, 0x0A)
    L = len(want)
    assert L >= 3
    for group in (0, 3000) if T.n <= 8 else (0,):
        dctx.set_verify_group(group)
        try:
            st, got, _ = dev.grep(dctx, pat, 0x0A, cap=L, keep=True)
            assert got == want
            d_lines = torch.zeros(L, dtype=torch.int64, device=cuda)
            dctx.lines_of_shard(*dev.run, dev.ds.data_ptr(), L, d_lines.data_ptr(), b"\n", dev.stream)
            assert d_lines.cpu().tolist() == lm.ranks(T.plain, 0x0A, [s for s, _ in want])
            out = torch.full((st[1] + 64,), 0xA5, dtype=torch.uint8, device=cuda)
            n = dctx.decompress_ranges_shard(*dev.run, dev.ds.data_ptr(), dev.de.data_ptr(), L, out.data_ptr(), st[1], stream=dev.stream)
            buf = out.cpu().numpy().tobytes()
            assert n == st[1] and buf[:n] == model.join(T.plain, want) and buf[n:] == b"\xA5" * 64
            assert dctx.ranges_stats()["ranges"] == L and dctx.ranges_stats()["bytes"] == n
        finally:
            dctx.set_verify_group(0)


@pytest.mark.parametrize("name", ["f7_many", "f8_batch", "craft8_0a"])
def test_grep_host_gives_the_lines_bytes(name, files, dctx):
    T = files[name]
    for pat in (T.plain[100:102], b" ", fm.absent(T.plain)) + ((model.MARK,) if name.startswith("craft") else ()):
        if 0x0A in pat:
            continue
        want = model.selected(T.plain, pat, 0x0A)
        st, got = dctx.grep_host(T.blob, pat)
        assert [st[n] for n in mc.DContext.GREP_STATS] == model.stats(T.plain, pat, 0x0A, want)
        assert got == model.join(T.plain, want)
    assert mc.grep(T.blob, b"e ") == model.join(T.plain, model.selected(T.plain, b"e ", 0x0A))


# ---- 4. the ranges decode on hand-made lists ----
def range_lists(T: Truth):
    t, off = T.total, T.dec_off
    seams = sorted({s + k for s in set(off[1:-1]) for k in (-1, 0, 1) if 0 <= s + k < t})
    return {
        "empty": [],
        "all": [(0, t)],
        "empty ranges between full ones": [(0, 0), (0, 10), (10, 10), (10, 10), (500, 900), (900, 900), (t, t)],
        "touching": [(5, 100), (100, 101), (101, 4096), (4096, 4097), (4097, 5000)],
        "ending at T": [(17, 18), (t - 3, t)],
        "one byte at every seam": [(s, s + 1) for s in seams[:400]],
        "across three groups": [(off[1] - 7, off[min(4, T.n)] - 1 if T.n > 3 else t - 1)],
        "only empty": [(3, 3), (t, t)],
    }


@pytest.mark.parametrize("group", GROUPS)
@pytest.mark.parametrize("name", ["f7_mixed", "craft8_0a", "f7_many", "f8_batch"])
def test_hand_made_range_lists(name, group, files, devs, dctx):
    T, dev = files[name], devs[name]
    index = dev.index(dctx)
    dctx.set_verify_group(group)
    try:
        for what, ranges in range_lists(T).items():
            if group and T.n > 8 and what in ("all", "across three groups"):
                ranges = [(T.dec_off[250] - 7, T.dec_off[258] + 1)]   # (a few groups of the many)
            for ix in (None, index):
                assert dev.ranges(dctx, ranges, ix) == model.join(T.plain, ranges), (name, group, what, ix is not None)
                st = dctx.ranges_stats()
                touched = [k for k in range(T.n) if any(max(s, T.dec_off[k]) < min(e, T.dec_off[k + 1]) for s, e in ranges)]
                assert st["ranges"] == len(ranges) and st["records_touched"] == len(touched), (name, group, what, st)
                assert st["records_decoded"] == len(touched) and st["bytes"] == sum(e - s for s, e in ranges)
                if group == 1:
                    assert st["groups"] == len(touched)
    finally:
        dctx.set_verify_group(0)


def test_many_short_ranges_and_more_than_one_scan_chunk(files, devs, dctx):
    """5000 ranges: the offsets' scan runs over five chunks of 1024; lengths 0 .. 40 at every alignment"""
    T, dev = files["f7_runs"], devs["f7_runs"]
    ranges, at = [], 3
    for i in range(5000):
        n = (i * 7) % 41
        ranges.append((at, at + n))
        at += n + (i % 3)
    assert at < T.total and len(ranges) > 4 * 1024
    for group in (0, 3000):
        dctx.set_verify_group(group)
        try:
            assert dev.ranges(dctx, ranges) == model.join(T.plain, ranges)
        finally:
            dctx.set_verify_group(0)


def test_the_output_may_sit_at_any_alignment(files, devs, dctx, cuda):
    import torch

    T, dev = files["f7_mixed"], devs["f7_mixed"]
    ranges = [(1, 40), (41, 43), (100, 4100), (8000, 8400), (12000, 12001)]
    want = model.join(T.plain, ranges)
    ds = torch.tensor([r[0] for r in ranges], dtype=torch.int64, device=cuda)
    de = torch.tensor([r[1] for r in ranges], dtype=torch.int64, device=cuda)
    for shift in range(17):
        out = torch.full((len(want) + 128,), 0xA5, dtype=torch.uint8, device=cuda)
        n = dctx.decompress_ranges_shard(*dev.run, ds.data_ptr(), de.data_ptr(), len(ranges), out.data_ptr() + shift, len(want),
                                         stream=dev.stream)
        buf = out.cpu().numpy().tobytes()
        assert n == len(want) and buf[shift:shift + n] == want and buf[:shift] + buf[shift + n:] == b"\xA5" * 128, shift


def test_a_damaged_record_outside_the_ranges(files, cuda, dctx):
    T = files["f7_mixed"]
    good = Dev(cuda, T)
    index = good.index(dctx)
    recs = bytearray(T.recs)
    a, b = T.rec_off[5] + 4, T.rec_off[6]
    recs[a:b] = b"\xFF" * (b - a)   # record 5's payload, its length prefix kept
    bad = Dev(cuda, T, bytes(recs))
    ranges = [(10, 500), (4000, 8192), (T.dec_off[6] + 1, T.total)]
    assert bad.ranges(dctx, ranges, index) == model.join(T.plain, ranges)      # with an index: record 5 is not decoded
    rc, _, buf = bad.ranges(dctx, ranges, None, raw=True)                     # without: the index pass meets it
    assert rc == FCX_ERR_FORMAT
    rc, _, buf = bad.ranges(dctx, [(8000, 8300)], index, raw=True)            # touched: the decode meets it
    assert rc == FCX_ERR_FORMAT
    assert good.ranges(dctx, ranges) == model.join(T.plain, ranges)            # the context is as good as before


def test_refusals_name_the_failing_range(files, devs, dctx):
    T, dev = files["f7_mixed"], devs["f7_mixed"]
    t = T.total
    for what, ranges, bad in (("descending", [(0, 5), (100, 200), (50, 60), (300, 400)], 2),
                              ("overlapping", [(0, 5), (100, 200), (199, 260)], 2),
                              ("end < start", [(0, 5), (10, 9), (20, 30)], 1),
                              ("end > T", [(0, 5), (10, 20), (t - 1, t + 1)], 2),
                              ("the first of two", [(7, 3), (2, 1)], 0)):
        for group in (0, 1):
            dctx.set_verify_group(group)
            try:
                rc, got, buf = dev.ranges(dctx, ranges, raw=True)
            finally:
                dctx.set_verify_group(0)
            assert rc == FCX_ERR_ARG and f"range {bad} ".encode() in mc.lib().fcx_last_error(), (what, mc.lib().fcx_last_error())
            assert buf == b"\xA5" * len(buf), what   # checked before anything is stored
    many = [(i * 3, i * 3 + 2) for i in range(3000)]
    many[2500] = (many[2500][0], many[2500][0] + 4)   # behind the first chunk of the scan
    rc, _, _ = dev.ranges(dctx, many, raw=True)
    assert rc == FCX_ERR_ARG and b"range 2501 " in mc.lib().fcx_last_error()


def test_short_capacity_and_the_size_query(files, devs, dctx):
    T, dev = files["f7_mixed"], devs["f7_mixed"]
    ranges = [(10, 500), (4000, 8200)]
    need = 490 + 4200
    for cap in (0, 1, need - 1):
        rc, got, buf = dev.ranges(dctx, ranges, cap=cap, raw=True)
        assert rc == FCX_ERR_CAPACITY and got == need and buf == b"\xA5" * len(buf), cap
    rc, got, buf = dev.ranges(dctx, ranges, cap=need + 5, raw=True)
    assert rc == 0 and got == need and buf[:need] == model.join(T.plain, ranges) and buf[need:] == b"\xA5" * (len(buf) - need)
    assert dctx.decompress_ranges_host(T.blob, ranges) == model.join(T.plain, ranges)
    assert dctx.decompress_ranges_host(T.blob, []) == b""


# ---- 5. one context for everything ----
def test_one_context_find_grep_lines_ranges_grep(files, devs, cuda):
    import torch

    T, dev = files["f7_mixed"], devs["f7_mixed"]
    pat = T.plain[8189:8196]
    want = model.selected(T.plain, pat, 0x0A)
    assert len(want) == 1
    d = mc.DContext(0)
    try:
        assert d.find_shard(*dev.run, pat) == 1
        assert dev.grep(d, pat, 0x0A, cap=2)[1] == want
        assert d.lines_index_shard(*dev.run)["decoded"] == T.total
        assert dev.ranges(d, want) == model.join(T.plain, want)
        assert dev.grep(d, pat, 0x0A, cap=2)[1] == want
        assert d.grep_host(T.blob, pat)[1] == model.join(T.plain, want)
        d.set_profiling(True)
        d.grep_shard(*dev.run, pat)
        assert [n for n, _ in d.stage_times()] == ["index", "decode", "scan", "select", "summary"]
        dev.ranges(d, want)
        assert [n for n, _ in d.stage_times()] == ["index", "map", "decode", "gather"]
    finally:
        d.close()


# ---- 6. the stream forms ----
def seam_file(kind: str, block: int, seed: int):
    """300 records; one line lies across the seam of the stream form's groups (record 256) with a mark on each side"""
    b, seam = bytearray(fm.text(seed, 300 * block)), 256 * block
    for i in range(seam - 150, seam + 150):
        if b[i] == 0x0A:
            b[i] = 0x20
    b[seam - 60:seam - 55] = b[seam + 40:seam + 45] = model.MARK
    T = Truth(kind, bytes(b), block)
    assert T.sizes == [block] * 300 and T.dec_off[256] == seam
    s, e = model.line_of(T.plain, 0x0A, seam)
    assert s < seam - 60 and seam + 45 < e and fm.hits(T.plain, model.MARK) == [seam - 60, seam + 40]
    return T


@pytest.fixture(scope="module")
def seam_files():
    return {"f7_many": seam_file("7", 1000, 13), "f8_batch": seam_file("8", 256, 11)}


def stream_grep(dctx, T: Truth, pat: bytes, d: int = 0x0A, want_lines: bool = True):
    import io

    st, got = dctx.grep_stream(io.BytesIO(T.blob), pat, d, len(T.blob) - 10, want_lines)
    return [st[n] for n in mc.DContext.GREP_STATS], got


@pytest.mark.parametrize("name", ["f7_many", "f8_batch"])
def test_a_line_across_the_stream_seam_is_reported_once(name, seam_files, dctx):
    T = seam_files[name]
    seam = T.dec_off[256]
    line = model.line_of(T.plain, 0x0A, seam)
    for window in (0, 7):
        dctx.set_find_window(window)
        try:
            for pat in (model.MARK, b"e ", T.plain[seam - 2:seam + 2], fm.absent(T.plain)):
                want = model.selected(T.plain, pat, 0x0A)
                st, got = stream_grep(dctx, T, pat)
                assert got == want and st == model.stats(T.plain, pat, 0x0A, want), (name, window, pat)
                assert stream_grep(dctx, T, pat, want_lines=False) == (st, [])
            assert stream_grep(dctx, T, model.MARK)[1] == [line]
        finally:
            dctx.set_find_window(0)
    assert mc.grep_ranges(T.blob, model.MARK) == (dict(zip(mc.DContext.GREP_STATS, model.stats(T.plain, model.MARK, 0x0A))), [line])
    assert mc.grep(T.blob, model.MARK) == T.plain[line[0]:line[1]]


@pytest.mark.parametrize("name", ["craft7_0a", "craft8_ff", "f7_mixed", "f7_nodelim", "f7_xdxd", "f8_zeros"])
def test_the_stream_form_with_a_window_of_7_lines(name, files, dctx):
    T = files[name]
    d = 0xFF if name.endswith("_ff") else 0x0A
    pats = {"f7_xdxd": [b"x"], "f8_zeros": [bytes(33)], "f7_nodelim": [T.plain[:3]], "f7_mixed": [T.plain[100:102], T.plain[8189:8196]]}
    dctx.set_find_window(7)
    try:
        for group in (0, 3000):
            dctx.set_verify_group(group)
            for pat in pats.get(name, [model.MARK, T.plain[99:100]]):
                want = model.selected(T.plain, pat, d)
                assert stream_grep(dctx, T, pat, d) == (model.stats(T.plain, pat, d, want), want), (name, group, pat[:8])
    finally:
        dctx.set_find_window(0)
        dctx.set_verify_group(0)


@pytest.mark.parametrize("name", ["f7_many", "f8_batch"])
def test_the_ranges_stream_form(name, seam_files, dctx):
    import io

    T = seam_files[name]
    t, seam = T.total, T.dec_off[256]
    lists = {
        "across the stream seam": [(3, 9), (seam - 100, seam + 100), (t - 5, t)],
        "only the second group": [(seam + 1, seam + 2)],
        "touching and empty": [(0, 0), (0, 50), (50, 51), (51, 51), (seam, seam), (seam, seam + 7)],
        "the selected lines": model.selected(T.plain, b"e ", 0x0A),
    }
    for what, ranges in lists.items():
        sink = io.BytesIO()
        assert dctx.decompress_ranges_stream(io.BytesIO(T.blob), sink, ranges, len(T.blob) - 10) == sum(e - s for s, e in ranges), what
        assert sink.getvalue() == model.join(T.plain, ranges), what
    src, sink = io.BytesIO(T.blob), io.BytesIO()
    assert dctx.decompress_ranges_stream(src, sink, [(10, 20)]) == 10 and sink.getvalue() == T.plain[10:20]
    assert src.tell() <= 10 + T.rec_off[256]   # the second stream group was not read
    with pytest.raises(mc.FcxError, match="range 1 ends behind"):
        dctx.decompress_ranges_stream(io.BytesIO(T.blob), io.BytesIO(), [(0, 4), (t - 1, t + 1)])
    assert dctx.decompress_ranges_stream(io.BytesIO(T.blob), io.BytesIO(), []) == 0
