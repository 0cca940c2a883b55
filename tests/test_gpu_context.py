"""Context and inverted grep on device-resident runs: fcx_grep_blocks_shard (fcx_context.hip: a select stage in
line-number space behind k_sscan and k_gtiles), its host and stream forms, for FCX7 and FCX8.

Truth is never the code under test: the files come from the oracle's encoders, `plain` is the join of the oracle's
decode of every record (Truth of test_gpu_range.py), the expected blocks and stats are context_model's over it (the
model itself is pinned against GNU grep in test_context_model.py), and every call is compared in full: the eight
stats, every start, end and first line, the canaries behind min(cap, blocks).  The crafted files' plants are asserted
in the oracle's bytes.  Calls run under the group bounds 0, 1 and 3000 in the shard, host and stream forms; the
answer must not depend on where records, tiles, decode groups or stream groups end."""
import ctypes
import functools
import io

import pytest

import context_model as cm
import find_model as fm
import grep_model as gm
import inputs
import lines_model as lm
import my_compress_amd as mc
import set_model as sm
from test_gpu_range import Truth

pytestmark = pytest.mark.gpu

FCX_ERR_ARG, FCX_ERR_FORMAT = -1, -4
GROUPS = [0, 1, 3000]
CANARY = 0x5A5A5A5A5A5A5A5A
KEYS = mc.DContext.GREP_BLOCK_STATS if hasattr(mc.DContext, "GREP_BLOCK_STATS") else ()
# (invert, before, after): {0, 1} x {0, 1, 2, 7} x {0, 1, 3}, and the largest context
GRID = [(i, b, a) for i in (0, 1) for b in (0, 1, 2, 7) for a in (0, 1, 3)] + [(0, 4096, 4096), (1, 4096, 4096)]

# ---- the crafted file of short lines: 64 KiB at block 4096, lines of 40 bytes (of 64 in [20000, 36000)) ----
SHORT_N, SHORT_BLOCK = 65536, 4096
SHORT_BASE = {
    "line 1: before-context is cut at line 0": 40,
    "three lines between two base lines: with before 2, after 1 their blocks touch": [400, 560],
    "four lines between two: one unselected line stays between the blocks": [1200, 1400],
    "the first line the second decode group sees (it starts at 4092 = 4096 - (m - 1))": 4092,
    "the line in front of a record's end: after-context runs across the group's end": 8120,
    "behind 250 lines of 64 bytes without a base line: before 200 reaches back over whole groups": 36000,
    "the third line from the end: after 3 runs across the last delimiter into the tail": 65440,
}
SHORT_OPTS = [(0, 3, 0), (0, 200, 0), (0, 2, 1), (0, 0, 3), (0, 3, 3), (1, 2, 1), (1, 0, 0), (0, 200, 200), (0, 4096, 0), (1, 4096, 4096)]


def short_lines(d: int = 0x0A) -> bytes:
    at, pos = {4091}, 0
    while pos < SHORT_N - 40:
        pos += 64 if 20000 <= pos < 36000 else 40
        at.add(pos - 1)
    data = bytearray(lm.plant(fm.text(77, SHORT_N), d, at))
    for v in SHORT_BASE.values():
        for s in [v] if isinstance(v, int) else v:
            data[s + 2:s + 2 + len(gm.MARK)] = gm.MARK
    return bytes(data)


def check_short(plain: bytes, d: int = 0x0A):
    """every plant, asserted in the oracle's decoded bytes"""
    s, b = lm.starts(plain, d), cm.bounds(plain, d)
    m = len(gm.MARK)
    assert len(plain) == SHORT_N and plain[-1] != d and 0 < SHORT_N - s[-1] < 40
    base = cm.base_lines(plain, [gm.MARK], d)
    starts = sorted(x for v in SHORT_BASE.values() for x in ([v] if isinstance(v, int) else v))
    assert [b[j][0] for j in base] == starts and len(fm.hits(plain, gm.MARK)) == len(starts)
    J = {b[j][0]: j for j in base}
    assert J[40] == 1
    assert J[560] - J[400] - 1 == 3 and J[1400] - J[1200] - 1 == 4
    two, one = cm.blocks(plain, [gm.MARK], d, before=2, after=1), None
    assert [x for x in two if x[2] <= J[400] < x[2] + x[3]] == [x for x in two if x[2] <= J[560] < x[2] + x[3]]
    lo, hi = [next(x for x in two if x[2] <= J[k] < x[2] + x[3]) for k in (1200, 1400)]
    assert lo != hi and lo[2] + lo[3] + 1 == hi[2]
    # the group seam a scan with the 5-byte mark sees: a group that is not the last judges, and takes the delimiters
    # of, the positions in front of its end - (m - 1)
    assert 4092 == SHORT_BLOCK - (m - 1) and plain[4091] == d and b[J[4092]][0] == 4092
    assert b[J[4092] - 3][0] < 4092 - 3 * 12 and b[J[4092] - 1][1] == 4092
    j = J[8120]
    assert b[j][1] == 8160 and b[j + 1][1] > 2 * SHORT_BLOCK > b[j + 1][0]      # after-context across the second record's end
    j = J[36000]
    assert j - base[base.index(j) - 1] > 250 and b[j - 200][1] <= 36000 - 3 * SHORT_BLOCK   # two whole groups and more in between
    assert b[j - 200][0] > 20000 and all(y - x == 64 for x, y in b[j - 200:j])
    assert J[65440] == len(b) - 3 and b[-1][1] == SHORT_N and b[-2][1] == s[-1]
    return base


@pytest.fixture(scope="module")
def files():
    F = {}
    for d in gm.DELIMS:
        for kind in "78":
            T = F[f"craft{kind}_{d:02x}"] = Truth(kind, gm.crafted(d), gm.CRAFT_BLOCK)
            assert T.sizes == [5000] * 4
            gm.check_crafted(T.plain, d)
    for kind in "78":
        T = F[f"short{kind}"] = Truth(kind, short_lines(), SHORT_BLOCK)
        assert T.sizes == [SHORT_BLOCK] * 16
        check_short(T.plain)
    F["f7_many"] = Truth("7", fm.text(13, 300 * 1000), 1000)
    assert F["f7_many"].sizes == [1000] * 300
    F["f8_batch"] = Truth("8", fm.text(11, 300 * 256), 256)
    assert F["f8_batch"].sizes == [256] * 300
    F["f7_nodelim"] = Truth("7", lm.plant(fm.text(5, 9000), 0x0A, []), 4096)   # no 0x0A at all: one line
    assert 0x0A not in F["f7_nodelim"].plain and F["f7_nodelim"].total == 9000
    F["f7_xdxd"] = Truth("7", b"x\n" * 4096, 4096)   # every line holds the pattern `x`; the file ends in a delimiter
    assert F["f7_xdxd"].plain == b"x\n" * 4096
    F["f7_tiny"] = Truth("7", fm.text(7, 100), 4096)
    assert F["f7_tiny"].sizes == [100]
    F["f7_empty"] = Truth("7", fm.rand(3, 3000), 1000)   # three records, T == 0
    assert F["f7_empty"].sizes == [0, 0, 0]
    t = fm.text(21, 9000)
    F["f8_enddelim"] = Truth("8", t[:t.rindex(b"\n") + 1], 4096)   # a file that ends in a delimiter
    assert F["f8_enddelim"].plain.endswith(b"\n") and F["f8_enddelim"].n >= 2
    xy = bytearray(b"x\n" * 4096)
    xy[400:8000:800] = b"y" * 10
    F["f7_xyxd"] = Truth("7", bytes(xy), 4096)   # 10 lines `y`, 4086 lines `x`
    assert F["f7_xyxd"].plain == bytes(xy) and xy.count(b"y") == 10
    return F


@pytest.fixture(scope="module")
def dctx(cuda):
    d = mc.DContext(0)
    yield d
    d.set_verify_group(0)
    d.set_find_window(0)
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

    def blocks(self, dctx, ps, d: int, opt, cap: int, keep: bool = False):
        """fcx_grep_blocks_shard: (stats, [(start, end, line)] of the first min(cap, blocks), what lies behind them in the
        three arrays, counts)"""
        import torch

        arr = [torch.full((cap + 8,), CANARY, dtype=torch.int64, device=self.cuda) for _ in range(3)]
        ptr = [a.data_ptr() if cap else 0 for a in arr]
        st, counts = dctx.grep_blocks_shard(*self.run, ps, d, bool(opt[0]), opt[1], opt[2], d_start=ptr[0], d_end=ptr[1], d_line=ptr[2],
                                            cap=cap, stream=self.stream)
        s, e, ln = (a.cpu().tolist() for a in arr)
        k = min(cap, st["blocks"])
        if keep:
            self.arr = arr
        return [st[n] for n in KEYS], list(zip(s[:k], e[:k], ln[:k])), s[k:] + e[k:] + ln[k:], counts


@pytest.fixture(scope="module")
def devs(files, cuda):
    return {name: Dev(cuda, T) for name, T in files.items()}


@functools.lru_cache(maxsize=None)
def _want(plain: bytes, pats: tuple, d: int, fold: bool, opt: tuple):
    blk = cm.blocks(plain, list(pats), d, fold, bool(opt[0]), opt[1], opt[2])
    return blk, cm.stats(plain, list(pats), d, fold, bool(opt[0]), opt[1], opt[2], blk)


def want_of(T: Truth, pats, d, fold, opt):
    return _want(T.plain, tuple(pats), d, fold, tuple(opt))


def check_shard(dev: Dev, dctx, ps, pats, d, fold, opt, what, cap=None):
    blk, stats = want_of(dev.T, pats, d, fold, opt)
    cap = len(blk) + 3 if cap is None else cap
    st, got, behind, counts = dev.blocks(dctx, ps, d, opt, cap)
    assert st == stats, (what, opt, st, stats)
    assert got == [x[:3] for x in blk][:cap], (what, opt)
    assert behind == [CANARY] * len(behind), (what, opt, "entries behind min(cap, blocks) were written")
    assert counts == sm.counts(dev.T.plain, pats, fold), (what, opt)


def check_stream_and_host(T: Truth, dctx, ps, pats, d, fold, opt, what):
    blk, stats = want_of(T, pats, d, fold, opt)
    gs, got, gc = dctx.grep_blocks_stream(io.BytesIO(T.blob), ps, d, bool(opt[0]), opt[1], opt[2], len(T.blob) - 10)
    assert got == blk, (what, opt, "stream")
    assert [gs[k] for k in KEYS] == stats and gc == sm.counts(T.plain, pats, fold), (what, opt, gs, stats)
    hs, out, hc = dctx.grep_blocks_host(T.blob, ps, d, bool(opt[0]), opt[1], opt[2])
    assert out == cm.join(T.plain, blk), (what, opt, "host")
    assert [hs[k] for k in KEYS] == stats and hc == gc, (what, opt, hs, stats)


def check_forms(name, files, devs, dctx, pats, d, fold, opts, group, window=7):
    T, dev = files[name], devs[name]
    dctx.set_verify_group(group)
    dctx.set_find_window(window)
    ps = mc.PatternSet(pats, fold)
    try:
        for opt in opts:
            check_shard(dev, dctx, ps, pats, d, fold, opt, (name, group))
            check_stream_and_host(T, dctx, ps, pats, d, fold, opt, (name, group, window))
    finally:
        ps.close()
        dctx.set_verify_group(0)
        dctx.set_find_window(0)


# ---- 1. grep_model's crafted file: every option of the grid, three delimiters, both kinds, three bounds, three forms ----
@pytest.mark.parametrize("group", GROUPS)
@pytest.mark.parametrize("kind", "78")
@pytest.mark.parametrize("d", gm.DELIMS)
def test_the_crafted_file_under_every_option(d, kind, group, files, devs, dctx):
    """the run of empty lines at 100..102 as context and as inverted base lines; context across the tile seam at 4096,
    the record seam at 5000 and the group seam at 10000; the 7836-byte line, longer than a 3000-byte group, inside a
    context window and as a base line; the unterminated tail as a base line and as after-context; line 0"""
    name = f"craft{kind}_{d:02x}"
    plain = files[name].plain
    inv = cm.base_lines(plain, [gm.MARK], d, invert=True)
    assert {2, 3} <= set(inv) and len(cm.bounds(plain, d)) - 1 not in inv and 0 not in inv   # empty lines: base lines with invert
    check_forms(name, files, devs, dctx, [gm.MARK], d, False, GRID, group)
    if group == 1:
        assert dctx.verify_groups() == 4   # every record a group


# ---- 2. the file of short lines: what a context that reaches into other decode groups can get wrong ----
@pytest.mark.parametrize("group", GROUPS)
@pytest.mark.parametrize("kind", "78")
def test_short_lines_across_decode_groups(kind, group, files, devs, dctx):
    name = f"short{kind}"
    T = files[name]
    blk = want_of(T, [gm.MARK], 0x0A, False, (0, 200, 0))[0]
    assert any(x[3] == 201 and x[1] - x[0] == 200 * 64 + 40 for x in blk)   # 200 lines of before-context over three records
    blk = want_of(T, [gm.MARK], 0x0A, False, (0, 3, 0))[0]
    assert any(x[0] < 4092 < x[1] and x[3] == 4 for x in blk)               # three lines into the group before
    check_forms(name, files, devs, dctx, [gm.MARK], 0x0A, False, SHORT_OPTS, group)
    if group:
        assert dctx.verify_groups() == 16


# ---- 3. 300 records: a context window and an open block across the 256-record seam of the stream form ----
def seam_pattern(T: Truth, d: int):
    """a pattern cut from the last line that starts in front of the 256-record seam, with few hits in the file"""
    seam = T.dec_off[256]
    s, e = gm.line_of(T.plain, d, seam - 1)
    for m in (8, 7, 6, 5):
        at = max(s, seam - 40)
        pat = gm.cut(T.plain, d, at, m)
        if pat and len(pat) == m and len(fm.hits(T.plain, pat)) <= 40:
            return pat
    raise AssertionError("no rare pattern in front of the seam")


@pytest.mark.parametrize("window", [0, 1])
@pytest.mark.parametrize("name", ["f7_many", "f8_batch"])
def test_the_stream_group_seam(name, window, files, devs, dctx):
    T = files[name]
    d, seam = 0x0A, T.dec_off[256]
    pat = seam_pattern(T, d)
    opts = [(0, 0, 0), (0, 2, 2), (0, 0, 3), (1, 1, 0), (1, 0, 0)]
    blk = want_of(T, [pat], d, False, (0, 2, 2))[0]
    assert any(x[0] < seam < x[1] for x in blk), "no block across the seam"
    assert any(x[0] < seam < x[1] for x in want_of(T, [pat], d, False, (1, 1, 0))[0])
    check_forms(name, files, devs, dctx, [pat], d, False, opts, 0, window)
    if window == 0:
        check_forms(name, files, devs, dctx, [pat], d, False, opts[1:2], 1, window)


# ---- 4. degenerate runs ----
@pytest.mark.parametrize("group", GROUPS)
def test_degenerate_runs(group, files, devs, dctx):
    L = lambda T: len(cm.bounds(T.plain, 0x0A))
    T = files["short7"]
    absent = fm.absent(T.plain)
    assert want_of(T, [absent], 0x0A, False, (0, 3, 3)) == ([], [0, 0, 0, 0, 0, T.total - 5, T.total, L(T)])   # no hit at all
    assert want_of(T, [absent], 0x0A, False, (1, 0, 0))[0] == [(0, T.total, 0, L(T))]
    check_forms("short7", files, devs, dctx, [absent], 0x0A, False, [(0, 0, 0), (0, 3, 3), (1, 0, 0), (1, 2, 2)], group)
    T = files["f7_xdxd"]                                                             # every line hit
    assert want_of(T, [b"x"], 0x0A, False, (1, 0, 0))[0] == [] and want_of(T, [b"x"], 0x0A, False, (1, 5, 5))[0] == []
    assert want_of(T, [b"x"], 0x0A, False, (0, 0, 0))[0] == [(0, 8192, 0, 4096)]
    check_forms("f7_xdxd", files, devs, dctx, [b"x"], 0x0A, False, [(0, 0, 0), (1, 0, 0), (1, 5, 5), (0, 1, 1)], group)
    T = files["f7_nodelim"]                                                          # a run without a delimiter: one line
    for pat in (T.plain[4090:4100], fm.absent(T.plain)):
        check_forms("f7_nodelim", files, devs, dctx, [pat], 0x0A, False, [(0, 0, 0), (1, 0, 0), (0, 2, 2), (1, 2, 2)], group)
    T = files["f7_tiny"]                                                             # the 100-byte file
    for pat in (T.plain[:100], T.plain[50:53], T.plain[97:100]):
        if b"\n" not in pat:
            check_forms("f7_tiny", files, devs, dctx, [pat], 0x0A, False, [(0, 0, 0), (1, 0, 0), (0, 1, 1), (1, 1, 1)], group)
    assert want_of(files["f7_empty"], [b"a"], 0x0A, False, (1, 1, 1)) == ([], [0] * 8)   # a run that decodes to 0 bytes
    check_forms("f7_empty", files, devs, dctx, [b"a"], 0x0A, False, [(0, 0, 0), (1, 0, 0), (1, 1, 1)], group)
    T = files["f8_enddelim"]                                                         # a file that ends in a delimiter
    last = cm.bounds(T.plain, 0x0A)[-1]
    pat = gm.cut(T.plain, 0x0A, last[0], 4) or b"e"
    assert last[1] == T.total and L(T) == T.plain.count(b"\n")
    check_forms("f8_enddelim", files, devs, dctx, [pat], 0x0A, False, [(0, 0, 0), (0, 0, 3), (1, 0, 0), (1, 1, 1), (0, 2, 0)], group)


def test_no_records(dctx):
    ps = mc.PatternSet([b"ab"])
    try:
        for kind in "78":
            st, counts = dctx.grep_blocks_shard(kind, 0, 0, 0, ps, invert=True, before=2, after=2)
            assert st == dict.fromkeys(KEYS, 0) and counts == [0]
        empty = mc.write_header(0, 0)
        assert dctx.grep_blocks_host(empty, ps, invert=True) == (dict.fromkeys(KEYS, 0), b"", [0])
        assert dctx.grep_blocks_stream(io.BytesIO(empty), ps, invert=True) == (dict.fromkeys(KEYS, 0), [], [0])
    finally:
        ps.close()


# ---- 5. identities ----
@pytest.mark.parametrize("group", GROUPS)
@pytest.mark.parametrize("name", ["craft7_0a", "craft8_ff", "short8", "f7_many"])
def test_zero_options_are_the_set_grep(name, group, files, devs, dctx):
    """stats lines, bytes, hits and judged equal fcx_grep_set_shard's; the blocks' bytes through
    fcx_decompress_ranges_shard equal grep_any(); the groups scanned are the same: the run is decoded once"""
    import torch

    T, dev = files[name], devs[name]
    d = int(name[-2:], 16) if name.startswith("craft") else 0x0A
    pats = [gm.MARK] if name != "f7_many" else [seam_pattern(T, d), b"the"]
    dctx.set_verify_group(group)
    ps = mc.PatternSet(pats)
    try:
        old, _ = dctx.grep_set_shard(*dev.run, ps, d)
        groups_old = dctx.set_scan_stats()
        blk = want_of(T, pats, d, False, (0, 0, 0))[0]
        st, got, _, _ = dev.blocks(dctx, ps, d, (0, 0, 0), len(blk), keep=True)
        sc = dctx.set_scan_stats()
        assert (st[1], st[2], st[4], st[5], st[6]) == tuple(old[k] for k in mc.DContext.GREP_STATS)
        assert sc == groups_old and sc["groups"] == dctx.verify_groups() and sc["final_passes"] == 1
        need = st[2]
        out = torch.full((need + 64,), 0xA5, dtype=torch.uint8, device=dev.cuda)
        n = dctx.decompress_ranges_shard(*dev.run, dev.arr[0].data_ptr(), dev.arr[1].data_ptr(), len(blk), out.data_ptr(), need,
                                         stream=dev.stream)
        buf = out.cpu().numpy().tobytes()
        assert n == need and buf[need:] == b"\xA5" * 64
        if group == 0:
            assert buf[:need] == mc.grep_any(T.blob, pats, bytes([d])) == mc.grep_context(T.blob, pats, bytes([d]))
        else:
            assert buf[:need] == cm.join(T.plain, blk)
    finally:
        ps.close()
        dctx.set_verify_group(0)


@pytest.mark.parametrize("group", GROUPS)
def test_64_patterns_with_folding_and_invert(group, files, devs, dctx):
    T = files["craft7_0a"]
    words = sorted({w.lower() for w in T.plain.translate(bytes(b if 0x41 <= b <= 0x5A or 0x61 <= b <= 0x7A else 0x20 for b in range(256))).split()
                    if 3 <= len(w) <= 8})
    pats = [w.upper() if i % 2 else w for i, w in enumerate(words[:63])] + [sm.UP]
    assert len(pats) == 64 and len(set(pats)) == 64
    assert 0 < len(cm.matching(T.plain, pats, 0x0A, True)) < len(cm.bounds(T.plain, 0x0A))
    check_forms("craft7_0a", files, devs, dctx, pats, 0x0A, True, [(1, 0, 0), (1, 1, 2), (0, 1, 0)], group)


def test_cap_below_the_blocks(files, devs, dctx):
    T, dev = files["short7"], devs["short7"]
    ps = mc.PatternSet([gm.MARK])
    try:
        for group in GROUPS:
            dctx.set_verify_group(group)
            for opt in ((0, 2, 1), (1, 0, 0), (0, 200, 0)):
                n = len(want_of(T, [gm.MARK], 0x0A, False, opt)[0])
                assert n >= 3
                for cap in (0, 1, n - 1, n):
                    check_shard(dev, dctx, ps, [gm.MARK], 0x0A, False, opt, ("cap", group, cap), cap)
    finally:
        ps.close()
        dctx.set_verify_group(0)


def test_the_module_functions(files):
    T = files["short8"]
    blk, stats = want_of(T, [gm.MARK], 0x0A, False, (1, 2, 1))
    assert mc.grep_context(T.blob, [gm.MARK], invert=True, before=2, after=1) == cm.join(T.plain, blk)
    st, got, counts = mc.grep_context_blocks(T.blob, [gm.MARK], invert=True, before=2, after=1)
    assert got == blk and [st[k] for k in KEYS] == stats and counts == [len(fm.hits(T.plain, gm.MARK))]
    T = files["craft7_00"]
    blk = want_of(T, [gm.MARK.lower()], 0x00, True, (0, 1, 1))[0]
    assert mc.grep_context(T.blob, [gm.MARK.lower()], b"\0", ignore_case=True, before=1, after=1) == cm.join(T.plain, blk)


# ---- 6. refusals ----
def test_refusals(files, devs, dctx):
    dev = devs["craft7_0a"]
    L = mc.lib()
    st = (ctypes.c_uint64 * 8)()
    k, p, ln, nb = dev.run

    def rc(pats, d, opts, fold=False):
        ps = mc.PatternSet(pats, fold)
        try:
            o = ctypes.byref(mc.GrepOpts(*opts)) if opts is not None else None
            return L.fcx_grep_blocks_shard(dctx._h, k.encode(), ctypes.c_void_p(p), ln, nb, d, ps.handle, o, None, None, None, 0, st,
                                           None, None)
        finally:
            ps.close()

    assert rc([b"ab"], 0x0A, (0, 4096, 4096)) == 0
    assert rc([b"ab"], 0x0A, (0, 4097, 0)) == FCX_ERR_ARG and b"FCX_GREP_MAX_CONTEXT" in L.fcx_last_error()
    assert rc([b"ab"], 0x0A, (1, 0, 4097)) == FCX_ERR_ARG
    assert rc([b"ab"], 0x0A, (2, 0, 0)) == FCX_ERR_ARG and b"flag" in L.fcx_last_error()
    assert rc([b"ab"], 0x0A, (3, 0, 0)) == FCX_ERR_ARG
    assert rc([b"ab"], 0x0A, None) == FCX_ERR_ARG and b"fcx_grep_blocks_shard" in L.fcx_last_error()
    assert rc([b"ab", b"c\nd"], 0x0A, (0, 0, 0)) == FCX_ERR_ARG and b"holds the delimiter" in L.fcx_last_error()
    assert rc([b"xay"], 0x41, (1, 1, 1)) == 0 and rc([b"xay"], 0x41, (1, 1, 1), True) == FCX_ERR_ARG
    ps = mc.PatternSet([b"ab"])
    try:
        o = ctypes.byref(mc.GrepOpts(0, 0, 0))
        one = ctypes.c_void_p(dev.d_in.data_ptr())   # cap > 0 with an array missing
        assert L.fcx_grep_blocks_shard(dctx._h, b"7", ctypes.c_void_p(p), ln, nb, 10, ps.handle, o, one, one, None, 4, st, None, None) == FCX_ERR_ARG
        assert L.fcx_grep_blocks_shard(dctx._h, b"9", ctypes.c_void_p(p), ln, nb, 10, ps.handle, o, None, None, None, 0, st, None, None) == FCX_ERR_ARG
        bad = ctypes.byref(mc.GrepOpts(0, 5000, 0))
        n = ctypes.c_uint64(0)
        blob = files["craft7_0a"].blob
        assert L.fcx_grep_blocks_host(dctx._h, blob, len(blob), 10, ps.handle, bad, None, 0, ctypes.byref(n), None, None) == FCX_ERR_ARG
        assert L.fcx_grep_blocks_host(dctx._h, blob, len(blob), 10, ps.handle, None, None, 0, ctypes.byref(n), None, None) == FCX_ERR_ARG
        with pytest.raises(mc.FcxError, match="FCX_GREP_MAX_CONTEXT"):
            dctx.grep_blocks_stream(io.BytesIO(blob), ps, after=4097)
        assert L.fcx_grep_blocks_host(dctx._h, blob, len(blob), 10, ps.handle, o, None, 0, ctypes.byref(n), None, None) == -2 and n.value > 0
    finally:
        ps.close()


def test_a_damaged_record(files, cuda, dctx):
    T = files["short7"]
    recs = bytearray(T.recs)
    a, b = T.rec_off[5] + 4, T.rec_off[6]
    recs[a:b] = b"\xFF" * (b - a)   # record 5's payload, its length prefix kept
    bad, good = Dev(cuda, T, bytes(recs)), Dev(cuda, T)
    ps = mc.PatternSet([gm.MARK])
    try:
        st = (ctypes.c_uint64 * 8)()
        k, p, ln, nb = bad.run
        o = ctypes.byref(mc.GrepOpts(1, 2, 2))
        args = (dctx._h, k.encode(), ctypes.c_void_p(p), ln, nb, 10, ps.handle)
        assert mc.lib().fcx_grep_set_shard(*args, None, None, 0, st, None, None) == FCX_ERR_FORMAT
        assert mc.lib().fcx_grep_blocks_shard(*args, o, None, None, None, 0, st, None, None) == FCX_ERR_FORMAT
        check_shard(good, dctx, ps, [gm.MARK], 0x0A, False, (1, 2, 2), "the context is as good as before")
    finally:
        ps.close()


# ---- 7. scratch does not grow with the hits, the lines or the blocks ----
def test_scratch_is_the_same_for_ten_hits_and_for_every_line_hit(files, devs, dctx):
    T, dev = files["f7_xyxd"], devs["f7_xyxd"]
    few, every = mc.PatternSet([b"y"]), mc.PatternSet([b"y", b"x"])
    try:
        seen = {}
        for opt in ((0, 2, 2), (1, 0, 0), (0, 0, 0)):
            for ps, hits in ((few, 10), (every, 4096)):
                st, _ = dctx.grep_blocks_shard(*dev.run, ps, 0x0A, bool(opt[0]), opt[1], opt[2])
                assert st["hits"] == hits and st["total_lines"] == 4096
                seen.setdefault(opt, []).append(dctx.grep_scratch())
        tiles = (T.total + 256 + 4095) // 4096 + 1   # (one group: the run and the carry's room)
        want = tiles * (2 * 512 + 48 + 3 * 512 + 56) + 8 * 4097 + 8 * 32
        assert all(v == [want, want] for v in seen.values()), seen
        assert want < 8 * 4096 * 3   # less than three u64 per line would take
    finally:
        few.close()
        every.close()
