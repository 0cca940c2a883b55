"""Regular-expression grep on device-resident runs: fcx_grep_regex_blocks_shard (fcx_regex.hip: a DFA scan by state-map
composition in front of k_gtiles and the select stage of fcx_context.hip), its host and stream forms, for FCX7 and FCX8.

Truth is never the code under test: the files come from the oracle's encoders, `plain` is the join of the oracle's
decode of every record (Truth of test_gpu_range.py), the expected hits, blocks and stats are regex_model's over it (an
NFA simulation pinned against GNU grep and Python's re in test_regex_model.py), and every call is compared in full:
the eight stats, every start, end and first line, the canaries behind min(cap, blocks).  The crafted files' plants are
asserted in the oracle's bytes.  Calls run under the group bounds 0, 1 and 3000 in the shard, host and stream forms;
the answer must not depend on where records, tiles, decode groups or stream groups end."""
import functools
import io

import pytest

import context_model as cm
import find_model as fm
import grep_model as gm
import lines_model as lm
import my_compress_amd as mc
import regex_model as rm
from regex_model import BLOCK, CRAFT_EXPRS, E_64, E_2, E_ANY, E_BOL, E_EOL, E_FAR, E_MIX, crafted
import set_model as sm
from test_gpu_range import Truth

pytestmark = pytest.mark.gpu

GROUPS = [0, 1, 3000]
CANARY = 0x5A5A5A5A5A5A5A5A
KEYS = mc.DContext.GREP_BLOCK_STATS
DELIMS = [0x0A, 0x00, 0x41]
# (the LZ78 reference drops a zero byte that opens a record, so the file with d = 0x00 at offset 5000 is FCX7 alone)
CRAFT = [(d, kind) for d in DELIMS for kind in "78" if (d, kind) != (0x00, "8")]
OPTS = [(0, 0, 0), (1, 0, 0), (0, 2, 1), (1, 1, 3)]
GRID = [(i, b, a) for i in (0, 1) for b in (0, 1, 2, 7) for a in (0, 1, 3)] + [(0, 4096, 4096), (1, 4096, 4096)]

@functools.lru_cache(maxsize=None)
def model(plain: bytes, expr: bytes, d: int, fold: bool):
    nfa = rm.Nfa(expr, d, fold)
    return nfa, rm.hits(plain, nfa)


@functools.lru_cache(maxsize=None)
def want(plain: bytes, expr: bytes, d: int, fold: bool, opt: tuple):
    nfa, h = model(plain, expr, d, fold)
    blk = rm.blocks(plain, nfa, bool(opt[0]), opt[1], opt[2], h)
    return blk, rm.stats(plain, nfa, bool(opt[0]), opt[1], opt[2], blk, h)


def seam_file() -> bytes:
    """f7_seam_empty's shape: 256 records of 1000 bytes that end in a match of E_EOL, then three records that decode to no byte"""
    b = bytearray(fm.text(13, 256000).replace(b"#", b"."))
    b[255996:256000] = b"#42;"
    b[254000:254004] = b"#1;\n"
    return bytes(b) + fm.rand(5, 3000)


BATCH = {"7": 1000, "8": 256}   # (FCX7 records of 256 bytes of text do not all decode to 256 bytes)


def batch_file(kind: str) -> bytes:
    """300 records: a match that ends in front of the stream form's group seam (record 256), the delimiter behind it
    being the next stream group's first byte, and a line start there"""
    b = bytearray(fm.text(11, 300 * BATCH[kind]).replace(b"#", b"."))
    seam = 256 * BATCH[kind]
    b[seam - 4:seam + 5] = b"#77;\n#78;"
    return bytes(b)


@pytest.fixture(scope="module")
def files():
    F = {}
    for d, kind in CRAFT:
        T = F[f"craft{kind}_{d:02x}"] = Truth(kind, crafted(d), BLOCK)
        assert T.sizes == [BLOCK] * 4
        rm.check_crafted(T.plain, d)
    nd = bytearray(lm.plant(fm.text(5, 9000), 0x0A, []))   # no 0x0A at all: one line of 9000 bytes over three tiles
    nd[4094:4100] = b"aaxxxb"
    nd[8190:8196] = b"ayyyyb"
    nd[8997:9000] = b"#3;"
    F["f7_nodelim"] = T = Truth("7", bytes(nd), 4096)
    assert 0x0A not in T.plain and T.total == 9000 and T.plain[4094:4100] == b"aaxxxb" and T.plain[8190:8196] == b"ayyyyb"
    h = model(T.plain, E_FAR, 0x0A, False)[1]
    assert 4099 in h and 8195 in h and 4094 // 4096 == 0 and 8190 // 4096 == 1 and 8195 // 4096 == 2
    assert model(T.plain, E_EOL, 0x0A, False)[1] == [8999]
    F["f7_xdxd"] = Truth("7", b"x\n" * 4096, 4096)
    assert F["f7_xdxd"].plain == b"x\n" * 4096
    F["f7_tiny"] = Truth("7", fm.text(7, 100), 4096)
    assert F["f7_tiny"].sizes == [100]
    F["f7_empty"] = Truth("7", fm.rand(3, 3000), 1000)   # three records, T == 0
    assert F["f7_empty"].sizes == [0, 0, 0]
    for kind in "78":
        T = F[f"f{kind}_batch"] = Truth(kind, batch_file(kind), BATCH[kind])
        seam = 256 * BATCH[kind]
        assert T.sizes == [BATCH[kind]] * 300 and T.dec_off[256] == seam and T.plain[seam - 4:seam + 5] == b"#77;\n#78;"
    F["f7_seam_empty"] = T = Truth("7", seam_file(), 1000)
    assert T.sizes == [1000] * 256 + [0] * 3 and T.plain[-4:] == b"#42;"
    fold = b"".join(bytes([b]) + b"x\n" for b in sm.FOLD_BYTES) + b"aX\n\xc1X\n\xe1x"
    F["f7_fold"] = Truth("7", fold, 4096)
    assert F["f7_fold"].plain == fold and set(sm.FOLD_BYTES) >= {0x40, 0x41, 0x5A, 0x5B, 0x60, 0x61, 0x7A, 0x7B, 0xC1}
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

    def __init__(self, cuda, T: Truth):
        import torch

        self.T, self.cuda = T, cuda
        self.d_in = torch.frombuffer(bytearray(T.recs), dtype=torch.uint8).to(cuda)
        self.stream = torch.cuda.current_stream().cuda_stream
        self.run = (T.kind, self.d_in.data_ptr(), len(T.recs), T.n)

    def arrays(self, cap):
        import torch

        arr = [torch.full((cap + 8,), CANARY, dtype=torch.int64, device=self.cuda) for _ in range(3)]
        return arr, [a.data_ptr() if cap else 0 for a in arr]

    def blocks(self, dctx, rx, opt, cap: int, keep: bool = False):
        """fcx_grep_regex_blocks_shard: (stats, [(start, end, line)] of the first min(cap, blocks), what lies behind them)"""
        arr, ptr = self.arrays(cap)
        st = dctx.grep_regex_blocks_shard(*self.run, rx, bool(opt[0]), opt[1], opt[2], d_start=ptr[0], d_end=ptr[1], d_line=ptr[2], cap=cap,
                                          stream=self.stream)
        s, e, ln = (a.cpu().tolist() for a in arr)
        k = min(cap, st["blocks"])
        if keep:
            self.arr = arr
        return [st[n] for n in KEYS], list(zip(s[:k], e[:k], ln[:k])), s[k:] + e[k:] + ln[k:]

    def set_blocks(self, dctx, ps, d, opt, cap: int):
        arr, ptr = self.arrays(cap)
        st, _ = dctx.grep_blocks_shard(*self.run, ps, d, bool(opt[0]), opt[1], opt[2], d_start=ptr[0], d_end=ptr[1], d_line=ptr[2], cap=cap,
                                       stream=self.stream)
        s, e, ln = (a.cpu().tolist() for a in arr)
        k = min(cap, st["blocks"])
        return [st[n] for n in KEYS], list(zip(s[:k], e[:k], ln[:k]))


@pytest.fixture(scope="module")
def devs(files, cuda):
    return {name: Dev(cuda, T) for name, T in files.items()}


def check_shard(dev: Dev, dctx, rx, expr, d, fold, opt, what, cap=None):
    blk, stats = want(dev.T.plain, expr, d, fold, tuple(opt))
    cap = len(blk) + 3 if cap is None else cap
    st, got, behind = dev.blocks(dctx, rx, opt, cap)
    assert st == stats, (what, expr, opt, st, stats)
    assert got == [x[:3] for x in blk][:cap], (what, expr, opt)
    assert behind == [CANARY] * len(behind), (what, expr, opt, "entries behind min(cap, blocks) were written")
    sc = dctx.regex_scan_stats()
    assert (sc["judged"], sc["hits"], sc["final_passes"]) == (stats[5], stats[4], 1), (what, expr, sc)


def check_stream_and_host(T: Truth, dctx, rx, expr, d, fold, opt, what):
    blk, stats = want(T.plain, expr, d, fold, tuple(opt))
    gs, got = dctx.grep_regex_blocks_stream(io.BytesIO(T.blob), rx, bool(opt[0]), opt[1], opt[2], len(T.blob) - 10)
    assert got == blk, (what, expr, opt, "stream")
    assert [gs[k] for k in KEYS] == stats, (what, expr, opt, gs, stats)
    assert dctx.regex_scan_stats()["final_passes"] == 1
    hs, out = dctx.grep_regex_blocks_host(T.blob, rx, bool(opt[0]), opt[1], opt[2])
    assert out == cm.join(T.plain, blk), (what, expr, opt, "host")
    assert [hs[k] for k in KEYS] == stats, (what, expr, opt, hs, stats)


def check_forms(name, files, devs, dctx, expr, d, fold, opts, group, window=7):
    T, dev = files[name], devs[name]
    dctx.set_verify_group(group)
    dctx.set_find_window(window)
    rx = mc.Regex(expr, d, fold)
    try:
        for opt in opts:
            check_shard(dev, dctx, rx, expr, d, fold, opt, (name, group))
            check_stream_and_host(T, dctx, rx, expr, d, fold, opt, (name, group, window))
    finally:
        rx.close()
        dctx.set_verify_group(0)
        dctx.set_find_window(0)


# ---- 1. the crafted file: seams, anchors, far-back state, 64 and 2 states, three delimiters, both kinds, three forms ----
@pytest.mark.parametrize("group", GROUPS)
@pytest.mark.parametrize("d,kind", CRAFT)
def test_the_crafted_file(d, kind, group, files, devs, dctx):
    name = f"craft{kind}_{d:02x}"
    assert mc.Regex(E_64, d).info()["states"] == 64 and mc.Regex(E_2, d).info()["states"] == 2
    for expr in CRAFT_EXPRS:
        check_forms(name, files, devs, dctx, expr, d, False, OPTS, group)
    if group == 1:
        assert dctx.verify_groups() == 4 and dctx.regex_scan_stats()["groups"] == 4   # every record a group


@pytest.mark.parametrize("group", GROUPS)
def test_entry_states_without_a_delimiter(group, files, devs, dctx):
    """one line of 9000 bytes over three tiles (and, under a bound, three decode groups): the state in front of a tile
    depends on bytes of the tiles before, up to the run's first byte for the anchored alternative"""
    for expr in (E_FAR, E_EOL, E_MIX, b"^[A-Z][^#]*#3;$", E_64):
        check_forms("f7_nodelim", files, devs, dctx, expr, 0x0A, False, [(0, 0, 0), (1, 0, 0), (0, 2, 2)], group)


# ---- 2. `$` and `^` at the stream form's seams ----
@pytest.mark.parametrize("window", [0, 1])
@pytest.mark.parametrize("kind", "78")
def test_the_stream_group_seam(kind, window, files, devs, dctx):
    name = f"f{kind}_batch"
    T = files[name]
    seam = T.dec_off[256]
    assert seam - 1 in model(T.plain, E_EOL, 0x0A, False)[1] and seam + 4 in model(T.plain, E_BOL, 0x0A, False)[1] and T.plain[seam] == 0x0A
    for expr in (E_EOL, E_BOL, E_ANY):
        check_forms(name, files, devs, dctx, expr, 0x0A, False, [(0, 0, 0), (0, 1, 1), (1, 0, 0)], 0, window)
    check_forms(name, files, devs, dctx, E_MIX, 0x0A, False, [(0, 1, 1)], 1, window)


@pytest.mark.parametrize("group", GROUPS)
def test_dollar_at_the_runs_end_behind_empty_groups(group, files, devs, dctx):
    """the match ends at T - 1 and the last stream group (the shard form: the last decode groups) decodes to no byte:
    only the final pass over the carried byte can set the hit"""
    T = files["f7_seam_empty"]
    assert model(T.plain, E_EOL, 0x0A, False)[1] == [254002, 255999]
    check_forms("f7_seam_empty", files, devs, dctx, E_EOL, 0x0A, False, [(0, 0, 0), (1, 0, 1)], group)


# ---- 3. the fold, negated sets, other shapes ----
@pytest.mark.parametrize("fold", [False, True])
def test_the_fold_at_its_edges(fold, files, devs, dctx):
    for expr in (b"ax", b"Zx", b"[a-z]x", b"[^a-z]x", b"\xc1x", b"[@`]X", b"\\wx$", b"[{[]x"):
        check_forms("f7_fold", files, devs, dctx, expr, 0x0A, fold, [(0, 0, 0), (1, 0, 0)], 0)
    check_forms("craft7_0a", files, devs, dctx, b"A[^B]{3}b|THE ", 0x0A, fold, [(0, 0, 0), (1, 1, 1)], 3000)
    check_forms("craft7_00", files, devs, dctx, b"A[^B]{3}b|THE ", 0x00, fold, [(0, 0, 0)], 1)


@pytest.mark.parametrize("group", GROUPS)
def test_degenerate_runs(group, files, devs, dctx):
    for expr, opts in ((b"x", [(0, 0, 0), (1, 0, 0), (1, 5, 5)]), (b"x$", [(0, 0, 0)]), (b"^x$", [(0, 1, 1)]), (b"y", [(0, 0, 0), (1, 0, 0)])):
        check_forms("f7_xdxd", files, devs, dctx, expr, 0x0A, False, opts, group)
    T = files["f7_tiny"]
    for expr in (b"[a-z]+ [a-z]+", b"^" + T.plain[:3].replace(b".", b"\\."), b"[a-z. ]$", E_64):
        check_forms("f7_tiny", files, devs, dctx, expr, 0x0A, False, [(0, 0, 0), (1, 0, 0), (0, 1, 1)], group)
    assert want(files["f7_empty"].plain, b"a", 0x0A, False, (1, 1, 1)) == ([], [0] * 8)
    check_forms("f7_empty", files, devs, dctx, b"a", 0x0A, False, [(0, 0, 0), (1, 1, 1)], group)


def test_no_records(dctx):
    rx = mc.Regex(b"ab+")
    try:
        for kind in "78":
            assert dctx.grep_regex_blocks_shard(kind, 0, 0, 0, rx, invert=True, before=2, after=2) == dict.fromkeys(KEYS, 0)
        empty = mc.write_header(0, 0)
        assert dctx.grep_regex_blocks_host(empty, rx, invert=True) == (dict.fromkeys(KEYS, 0), b"")
        assert dctx.grep_regex_blocks_stream(io.BytesIO(empty), rx, invert=True) == (dict.fromkeys(KEYS, 0), [])
    finally:
        rx.close()


# ---- 4. with no model: a regex that is one literal against the pattern set of that literal ----
@pytest.mark.parametrize("group", GROUPS)
def test_a_literal_is_the_one_pattern_set(group, files, devs, dctx):
    """identical blocks on every file and every option of the grid; identical stats but `judged`: a literal's match
    ends and match starts are equal in number"""
    dctx.set_verify_group(group)
    try:
        for name, dev in devs.items():
            d = int(name[-2:], 16) if name.startswith("craft") else 0x0A
            lit = b"#" if name.startswith(("craft", "f7_batch", "f8_batch", "f7_seam")) else dev.T.plain[1:3] if dev.T.total > 3 else b"ab"
            if d in lit:
                lit = b"x"
            rx, ps = mc.Regex(lit.replace(b".", b"\\."), d), mc.PatternSet([lit])
            try:
                for opt in GRID:
                    a, b = dev.blocks(dctx, rx, opt, 64)[:2], dev.set_blocks(dctx, ps, d, opt, 64)
                    assert a[1] == b[1] and a[0][:5] + a[0][6:] == b[0][:5] + b[0][6:], (name, lit, opt, a[0], b[0])
                    assert a[0][5] == dev.T.total and b[0][5] == max(dev.T.total - len(lit) + 1, 0)
            finally:
                rx.close()
                ps.close()
        # a literal that ends at T - 1 behind the empty groups: the regex's final pass sets what the set found three bytes earlier
        dev, lit = devs["f7_seam_empty"], b"42;"
        assert dev.T.plain.endswith(lit)
        rx, ps = mc.Regex(lit), mc.PatternSet([lit])
        try:
            for opt in GRID:
                a, b = dev.blocks(dctx, rx, opt, 64)[:2], dev.set_blocks(dctx, ps, 0x0A, opt, 64)
                assert a[1] == b[1] and a[0][:5] + a[0][6:] == b[0][:5] + b[0][6:], ("f7_seam_empty", lit, opt, a[0], b[0])
        finally:
            rx.close()
            ps.close()
    finally:
        dctx.set_verify_group(0)


# ---- 4b. more tiles than k_rentry has threads and than the scan kernels have workgroups ----
BIG_N, BIG_BLOCK, BIG_FLAT = 9 << 20, 1 << 20, 5 << 20
BIG_PLANTS = {4096 * 300 + 4094: b"axxxxb", 4096 * 1279 + 4093: b"ayyyyb", BIG_FLAT - 3: b"axxxxb", 4096 * 2100 + 4095: b"azzzzb"}


E_BIG_EOL, E_BIG_BOL = b"r\\. $", b"^[A-M]"


def big_data() -> bytes:
    """9 MiB of text in records of 1 MiB, the first 5 MiB without a delimiter: one line over 1280 tiles, then 1024 tiles
    of ordinary lines; E_FAR planted across tile seams, across the long line's end region and behind tile 2048"""
    b = bytearray(fm.text(17, BIG_N).replace(b"#", b"."))
    b[:BIG_FLAT] = bytes(b[:BIG_FLAT]).replace(b"\n", b" ")
    b[BIG_FLAT - 40:BIG_FLAT + 40] = bytes(b[BIG_FLAT - 40:BIG_FLAT + 40]).replace(b"\n", b" ")
    for at, what in BIG_PLANTS.items():
        b[at:at + len(what)] = what
    return bytes(b)


def big_hits(plain: bytes, expr: bytes):
    """the hits of three expressions whose match ends Python's re and numpy give exactly, overlapping ones included"""
    import re

    import numpy as np

    a = np.frombuffer(plain, dtype=np.uint8)
    if expr == E_FAR:   # (six bytes whatever matches: the end is the start + 5)
        return [m.start() + 5 for m in re.finditer(rb"(?=a[^b\n]{4}b)", plain)]
    if expr == E_BIG_EOL:
        behind = np.concatenate((a[1:] == 0x0A, [True]))
        ok = (a == 0x20) & behind
        ok[1:] &= a[:-1] == 0x2E
        ok[2:] &= a[:-2] == 0x72
        ok[:2] = False
        return np.flatnonzero(ok).tolist()
    assert expr == E_BIG_BOL
    first = np.concatenate(([True], a[:-1] == 0x0A))
    return np.flatnonzero((a >= 0x41) & (a <= 0x4D) & first).tolist()


@pytest.fixture(scope="module")
def big(cuda):
    out = {}
    for kind in "78":
        T = Truth(kind, big_data(), BIG_BLOCK)
        assert T.sizes == [BIG_BLOCK] * 9 and 0x0A not in T.plain[:BIG_FLAT + 40] and T.plain[BIG_FLAT + 40:].count(b"\n") > 1000
        assert all(T.plain[at:at + 6] == w for at, w in BIG_PLANTS.items())
        out[kind] = (T, Dev(cuda, T))
    return out


@pytest.mark.parametrize("group", [0, 1])
@pytest.mark.parametrize("kind", "78")
def test_thousands_of_tiles(kind, group, big, dctx):
    """one decode group of 2304 tiles (k_rentry's threads walk stretches of 9 tiles, k_rmap and k_rmark stride their
    2048 workgroups over them), or nine groups of 257 with the carried byte (stretches of 2); the first 1280 tiles are
    one line, so the state in front of a tile comes from far back"""
    T, dev = big[kind]
    for expr in (E_FAR, E_BIG_EOL, E_BIG_BOL):
        h = big_hits(T.plain, expr)
        assert 100 < len(h) and len(rm.base_lines(T.plain, rm.Nfa(expr), h=h)) < 11000
        if expr == E_FAR:
            assert all(at + 5 in h for at in BIG_PLANTS) and (4096 * 300 + 4094) // 4096 != (4096 * 300 + 4099) // 4096
        nfa = rm.Nfa(expr)
        rx = mc.Regex(expr)
        dctx.set_verify_group(group)
        try:
            for opt in ((0, 0, 0), (1, 1, 1)):
                blk = rm.blocks(T.plain, nfa, bool(opt[0]), opt[1], opt[2], h)
                stats = rm.stats(T.plain, nfa, bool(opt[0]), opt[1], opt[2], blk, h)
                st, got, behind = dev.blocks(dctx, rx, opt, len(blk) + 3)
                assert st == stats, (kind, group, expr, opt, st, stats)
                assert got == [x[:3] for x in blk] and behind == [CANARY] * len(behind), (kind, group, expr, opt)
                assert dctx.regex_scan_stats()["groups"] == (9 if group else 1)
                gs, gb = dctx.grep_regex_blocks_stream(io.BytesIO(T.blob), rx, bool(opt[0]), opt[1], opt[2], len(T.blob) - 10)
                assert gb == blk and [gs[k] for k in KEYS] == stats, (kind, group, expr, opt, "stream")
            hs, out = dctx.grep_regex_blocks_host(T.blob, rx)
            assert out == cm.join(T.plain, rm.blocks(T.plain, nfa, h=h)), (kind, group, expr, "host")
        finally:
            rx.close()
            dctx.set_verify_group(0)


# ---- 5. caps, chaining, reuse ----
def test_caps_and_the_chain_into_the_range_decode(files, devs, dctx):
    import torch

    T, dev = files["craft7_0a"], devs["craft7_0a"]
    rx = mc.Regex(E_ANY)
    try:
        for group in GROUPS:
            dctx.set_verify_group(group)
            for opt in ((0, 0, 0), (0, 2, 1), (1, 0, 0)):
                B = len(want(T.plain, E_ANY, 0x0A, False, opt)[0])
                assert B >= 2
                for cap in (0, 1, B - 1, B, B + 8):
                    check_shard(dev, dctx, rx, E_ANY, 0x0A, False, opt, ("cap", group, cap), cap)
        dctx.set_verify_group(1)
        blk, stats = want(T.plain, E_ANY, 0x0A, False, (0, 1, 1))
        st, got, _ = dev.blocks(dctx, rx, (0, 1, 1), len(blk), keep=True)
        need = st[2]
        out = torch.full((need + 64,), 0xA5, dtype=torch.uint8, device=dev.cuda)
        n = dctx.decompress_ranges_shard(*dev.run, dev.arr[0].data_ptr(), dev.arr[1].data_ptr(), len(blk), out.data_ptr(), need,
                                         stream=dev.stream)
        buf = out.cpu().numpy().tobytes()
        assert n == need and buf[need:] == b"\xA5" * 64 and buf[:need] == cm.join(T.plain, blk)
        assert mc.grep_regex(T.blob, E_ANY, before=1, after=1) == cm.join(T.plain, blk)
        gs, gb = mc.grep_regex_blocks(T.blob, E_ANY, before=1, after=1)
        assert gb == blk and [gs[k] for k in KEYS] == stats
        T0 = files["craft7_00"]
        blk0 = want(T0.plain, b"THE ", 0x00, True, (1, 0, 0))[0]
        assert mc.grep_regex(T0.blob, b"THE ", b"\0", ignore_case=True, invert=True) == cm.join(T0.plain, blk0)
    finally:
        rx.close()
        dctx.set_verify_group(0)


def test_one_context_through_set_regex_context_regex(files, devs, cuda):
    T, dev = files["craft8_0a"], devs["craft8_0a"]
    d = mc.DContext(0)
    rx, ps = mc.Regex(E_MIX), mc.PatternSet([b"#", b"the"])
    try:
        first, _ = d.grep_set_shard(*dev.run, ps, 0x0A)
        check_shard(dev, d, rx, E_MIX, 0x0A, False, (0, 1, 1), "behind a set grep")
        tiles = (T.total + 256 + 4095) // 4096 + 1   # (one group: the run and the carry's room)
        assert d.grep_scratch() == tiles * (2 * 512 + 48 + 3 * 512 + 56) + 8 * 4097 + 8 * 32 + tiles * (rx.info()["states"] + 1)
        blk = cm.blocks(T.plain, [b"#", b"the"], 0x0A, False, True, 1, 0)
        st, counts = d.grep_blocks_shard(*dev.run, ps, 0x0A, True, 1, 0)
        assert [st[k] for k in KEYS] == cm.stats(T.plain, [b"#", b"the"], 0x0A, False, True, 1, 0, blk)
        check_shard(dev, d, rx, E_MIX, 0x0A, False, (1, 0, 2), "behind a context grep")
        check_stream_and_host(T, d, rx, E_MIX, 0x0A, False, (0, 2, 0), "stream and host behind them")
        assert d.grep_set_shard(*dev.run, ps, 0x0A)[0] == first
    finally:
        rx.close()
        ps.close()
        d.close()
