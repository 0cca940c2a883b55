"""Pattern sets on device-resident runs: fcx_find_set_shard and fcx_grep_set_shard (fcx_set.hip: k_sscan in front of
the search's and the grep's downstream kernels), their host and stream forms, for FCX7 and FCX8.

Truth is never the code under test: the files come from the oracle's encoders, `plain` is the join of the oracle's
decode of every record (Truth of test_gpu_range.py), the expected hits, counts, lines and counters are set_model's
over it, and every call is compared in full: every hit, every count, every start and end, every stat.  The crafted
file's plants are asserted in the oracle's bytes (set_model.check_crafted).  Every call of a context's
methods, shard, host and stream form alike, runs under the group bounds 0, 1 and 3000; the module-level functions
make a context of their own and so run under the default bound."""
import ctypes
import io

import pytest

import find_model as fm
import grep_model as gm
import inputs
import my_compress_amd as mc
import set_model as sm
from test_gpu_range import Truth

pytestmark = pytest.mark.gpu

FCX_ERR_ARG = -1
NAMES = ["f7_mixed", "f7_runs", "f7_many", "f8_zeros", "f8_tail", "f8_batch"]
GROUPS = [0, 1, 3000]
CANARY = 0x5A5A5A5A5A5A5A5A
LENGTHS = [1, 2, 3, 4, 5, 8, 255, 256]
SMALL = 40000   # files up to this size get the filter's counters checked position by position


def seam_data(tail: bytes = b"") -> bytes:
    """256 records of 1000 bytes, the short patterns planted inside the last 255 bytes in front of the seam of the
    stream form's groups (record 256) and across it, then `tail`"""
    b = bytearray(fm.text(13, 256 * 1000).replace(sm.SHORT1, b".").replace(b"\x17", b"."))
    for p in (255800, 255999):
        b[p:p + 1] = sm.SHORT1
    for p in (255900, 255996):
        b[p:p + 3] = sm.SHORT3
    return bytes(b) + tail


@pytest.fixture(scope="module")
def files():
    F = {}
    F["f7_mixed"] = Truth("7", fm.mixed_data(), 4096)
    assert F["f7_mixed"].sizes == [4096, 4096, 0, 0, 0, 4096, 4096, 1808]
    F["f7_runs"] = Truth("7", inputs.generate("runs", 5, 200000), 65536)
    F["f7_many"] = Truth("7", fm.text(13, 300 * 1000), 1000)
    assert F["f7_many"].sizes == [1000] * 300
    F["f8_zeros"] = Truth("8", inputs.generate("zeros", 1, 100000), 65536)
    t = bytearray(fm.text(7, 12288)[:10001])
    t[4095] = t[8191] = t[10000] = 0
    F["f8_tail"] = Truth("8", bytes(t), 4096)
    assert F["f8_tail"].sizes == [4095, 4095, 1808]
    F["f8_batch"] = Truth("8", fm.text(11, 300 * 256), 256)
    assert F["f8_batch"].sizes == [256] * 300
    for d in gm.DELIMS:
        for kind in "78":
            T = F[f"craft{kind}_{d:02x}"] = Truth(kind, sm.crafted(d), sm.BLOCK)
            assert T.sizes == [5000] * 4
            sm.check_crafted(T.plain, d)
    F["f8_rand"] = Truth("8", fm.rand(3, 20000), 4096)   # (FCX8 keeps random bytes; FCX7 decodes such blocks to none)
    assert F["f8_rand"].plain == fm.rand(3, 20000)
    F["f7_tiny"] = Truth("7", fm.text(7, 100), 4096)
    assert F["f7_tiny"].sizes == [100]
    F["f7_empty"] = Truth("7", fm.rand(3, 3000), 1000)   # three records, T == 0
    assert F["f7_empty"].sizes == [0, 0, 0]
    F["f7_seam"] = Truth("7", seam_data(fm.text(5, 3000)), 1000)
    assert F["f7_seam"].sizes == [1000] * 259
    F["f7_seam_empty"] = Truth("7", seam_data(fm.rand(5, 3000)), 1000)   # the last stream group decodes to no bytes
    assert F["f7_seam_empty"].sizes == [1000] * 256 + [0] * 3
    for n in ("f7_seam", "f7_seam_empty"):
        assert fm.hits(F[n].plain, sm.SHORT1) == [255800, 255999] and fm.hits(F[n].plain, sm.SHORT3) == [255900, 255996]
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

    def find(self, dctx, ps, cap: int):
        """fcx_find_set_shard: (hits in the run, the first min(cap, hits), what lies behind them, counts)"""
        import torch

        out = torch.full((cap + 8,), CANARY, dtype=torch.int64, device=self.cuda)
        n, counts = dctx.find_set_shard(*self.run, ps, d_hits=out.data_ptr() if cap else 0, cap=cap, stream=self.stream)
        v = out.cpu().tolist()
        k = min(cap, n)
        return n, v[:k], v[k:], counts

    def grep(self, dctx, ps, d: int, cap: int, keep: bool = False):
        """fcx_grep_set_shard: (stats, [(start, end)] of the first min(cap, lines), what lies behind them, counts)"""
        import torch

        ds = torch.full((cap + 8,), CANARY, dtype=torch.int64, device=self.cuda)
        de = torch.full((cap + 8,), CANARY, dtype=torch.int64, device=self.cuda)
        st, counts = dctx.grep_set_shard(*self.run, ps, d, d_start=ds.data_ptr() if cap else 0, d_end=de.data_ptr() if cap else 0,
                                         cap=cap, stream=self.stream)
        s, e = ds.cpu().tolist(), de.cpu().tolist()
        k = min(cap, st["lines"])
        if keep:
            self.ds, self.de = ds, de
        return [st[n] for n in mc.DContext.GREP_STATS], list(zip(s[:k], e[:k])), s[k:] + e[k:], counts


@pytest.fixture(scope="module")
def devs(files, cuda):
    return {name: Dev(cuda, T) for name, T in files.items()}


def check_find(dev: Dev, dctx, pats, on: bool, what):
    """the shard form against the model: hits, counts, canaries, the scan's counters"""
    plain = dev.T.plain
    want, wc = sm.hits_any(plain, pats, on), sm.counts(plain, pats, on)
    ps = mc.PatternSet(pats, on)
    try:
        n, got, behind, counts = dev.find(dctx, ps, len(want) + 3)
        st = dctx.set_scan_stats()
    finally:
        ps.close()
    assert n == len(want) and got == want, (what, on, n, len(want))
    assert counts == wc and sum(counts) >= n, (what, on)
    assert behind == [CANARY] * len(behind), (what, "entries behind min(cap, hits) were written")
    assert st["judged"] == sm.judged(plain, pats) and st["hits"] == len(want), (what, on, st)
    assert st["final_passes"] == 1 and st["groups"] == dctx.verify_groups(), (what, st)
    if len(plain) <= SMALL:
        assert [st[k] for k in ("judged", "candidates", "compares", "hits")] == sm.scan_stats(plain, pats, on), (what, on, st)
    return want


def check_grep(dev: Dev, dctx, pats, d: int, on: bool, what):
    plain = dev.T.plain
    want = sm.selected_any(plain, pats, d, on)
    ps = mc.PatternSet(pats, on)
    try:
        st, got, behind, counts = dev.grep(dctx, ps, d, len(want) + 3)
        sc = dctx.set_scan_stats()
    finally:
        ps.close()
    assert st == sm.grep_stats(plain, pats, d, on, want), (what, on, st)
    assert got == want, (what, on)
    assert counts == sm.counts(plain, pats, on), (what, on)
    assert behind == [CANARY] * len(behind), (what, "entries behind min(cap, lines) were written")
    assert sc["judged"] == st[3] and sc["hits"] == st[2], (what, sc)
    return want


def check_both(dev, dctx, pats, d, what, folds=(False, True)):
    for on in folds:
        if all(bytes([d]) not in p and (not on or sm.fold(bytes([d]), True) not in sm.fold(p, True)) for p in pats):
            check_grep(dev, dctx, pats, d, on, what)
        check_find(dev, dctx, pats, on, what)


def cut_set(T: Truth, d: int):
    """up to 64 distinct patterns without the delimiter cut from plain, the eight lengths mixed: at the run's two
    ends, around the first record seam, the 256-record seam and the tile seam; one that does not occur"""
    seams = sorted(set(T.dec_off[1:-1]))
    at = ([T.dec_off[256]] if T.n > 256 else []) + seams[:1]
    pats, total = [], 0
    for m in LENGTHS:
        P = [0, T.total - m, fm.TILE - 1, fm.TILE - m // 2] + [x for s in at for x in (s - 1, s - m + 1, s - m // 2)]
        for p in P[:4 if m >= 255 else len(P)]:
            pat = gm.cut(T.plain, d, p, m) if 0 <= p < T.total else None
            if pat and pat not in pats and len(pats) < 63 and total + len(pat) <= 4000:
                pats.append(pat)
                total += len(pat)
    return pats + [fm.absent(T.plain)]


# ---- 1. every file of the search's tests, three group bounds, mixed lengths in one set ----
@pytest.mark.parametrize("group", GROUPS)
@pytest.mark.parametrize("name", NAMES)
def test_sets_cut_from_the_decoded_bytes(name, group, files, devs, dctx):
    T, dev = files[name], devs[name]
    dctx.set_verify_group(group)
    try:
        pats = cut_set(T, 0x0A)
        assert {len(p) for p in pats} >= ({1, 2, 3, 4, 5, 8} if name != "f8_zeros" else set(LENGTHS))
        check_both(dev, dctx, pats, 0x0A, (name, group))
        if group == 1:
            assert dctx.verify_groups() == T.n   # every record a group: the carry spans groups shorter than M
    finally:
        dctx.set_verify_group(0)


# ---- 2. the crafted file: mixed lengths at the run's tail and at group seams, one position, the fold, the grep ----
CRAFT_SETS = {
    "lengths 1 and 256": [sm.SHORT1, sm.LONG],
    "lengths 1, 3 and 256": [sm.SHORT1, sm.SHORT3, sm.LONG],
    "3 and 256, the mark across the tile seam": [sm.SHORT3, gm.MARK, sm.LONG],
    "ab, abc, abc again, bcd": [b"\x1a\x1b", b"\x1a\x1b\x1c", b"\x1a\x1b\x1c", b"\x1b\x1c\x1d", sm.LONG],
    "a pattern in upper case": [sm.UP.upper(), sm.SHORT1],
    "the fold's boundary bytes": [sm.FOLD_PAT, sm.FOLD_PAT.translate(sm.FOLD), sm.UP],
    "one short pattern": [sm.SHORT3],
}


@pytest.mark.parametrize("group", GROUPS)
@pytest.mark.parametrize("kind", ["7", "8"])
@pytest.mark.parametrize("d", gm.DELIMS)
def test_the_crafted_file(d, kind, group, files, devs, dctx):
    name = f"craft{kind}_{d:02x}"
    T, dev = files[name], devs[name]
    dctx.set_verify_group(group)
    try:
        for what, pats in CRAFT_SETS.items():
            check_both(dev, dctx, pats, d, (name, group, what))
        if group:
            assert dctx.verify_groups() == 4
        # the planted lines, by name
        sel = sm.selected_any(T.plain, [sm.SHORT1, sm.SHORT3, sm.LONG], d)
        for line in ((9001, 9901), (9901, 10501), (3001, 4501), (12154, 19990), (19990, sm.N)):
            assert sel.count(line) == 1
        # with and without the flag the same set answers differently
        assert sm.hits_any(T.plain, CRAFT_SETS["the fold's boundary bytes"], True) != sm.hits_any(T.plain, CRAFT_SETS["the fold's boundary bytes"], False)
    finally:
        dctx.set_verify_group(0)


# ---- 3. runs shorter than the patterns ----
@pytest.mark.parametrize("group", GROUPS)
def test_runs_shorter_than_the_patterns(group, files, devs, dctx):
    dctx.set_verify_group(group)
    try:
        T, dev = files["f7_tiny"], devs["f7_tiny"]   # T = 100 < M; the last bytes as short patterns
        tail3, tail1 = T.plain[-3:], T.plain[-1:]
        for pats in ([tail1, tail3, sm.LONG], [T.plain + b"zz", sm.LONG], [T.plain, tail3], [T.plain[:99] + b"\x01\x02"]):
            check_find(dev, dctx, pats, False, ("tiny", group))
            check_find(dev, dctx, pats, True, ("tiny", group))
        assert T.total - 3 in sm.hits_any(T.plain, [tail3]) and T.total - 1 in sm.hits_any(T.plain, [tail1])
        clean = [p for p in ([tail1, tail3, sm.LONG], [T.plain[-40:], sm.LONG]) if all(0x0A not in q for q in p)]
        for pats in clean:
            check_grep(dev, dctx, pats, 0x0A, False, ("tiny", group))
        T, dev = files["f7_empty"], devs["f7_empty"]   # T == 0
        assert check_find(dev, dctx, [b"a", sm.LONG], False, ("empty", group)) == []
        assert check_grep(dev, dctx, [b"a", sm.LONG], 0x0A, True, ("empty", group)) == []
    finally:
        dctx.set_verify_group(0)


# ---- 4. the filter ----
@pytest.mark.parametrize("group", GROUPS)
def test_the_filter(group, files, devs, dctx):
    dctx.set_verify_group(group)
    try:
        T, dev = files["f8_rand"], devs["f8_rand"]
        ones = [bytes([b]) for b in range(1, 256, 4)]   # 64 one-byte patterns: a quarter of the positions hit, in every lane
        assert len(ones) == 64
        want = check_find(dev, dctx, ones, False, ("64 one-byte patterns", group))
        assert len(want) > T.total // 5
        check_grep(dev, dctx, [p for p in ones if p != b"\x0d"], 0x0D, False, ("63 one-byte patterns, grep", group))
        T, dev = files["craft7_0a"], devs["craft7_0a"]
        head = sm.common_head(T.plain)
        at = fm.hits(T.plain, head)
        assert len(at) >= 4
        # 64 patterns that share their first two bytes: the filter passes all 64 at every occurrence of the two
        shared = [T.plain[at[0]:at[0] + 2 + i // 8] + bytes([0x80 + i]) for i in range(60)]
        shared += [T.plain[p:p + 7] for p in at[:4]]
        assert len({p[:2] for p in shared}) == 1 and len(shared) == 64
        check_find(dev, dctx, shared, False, ("64 patterns, one prefix", group))
        st = dctx.set_scan_stats()
        assert st["candidates"] == len(at) and st["compares"] == 64 * len(at) and 1 <= st["hits"] <= len(at)
        # 64 patterns none of which occurs: candidates, compares, no hit
        none = sm.absent_set(T.plain)
        assert check_find(dev, dctx, none, False, ("64 absent patterns", group)) == []
        st = dctx.set_scan_stats()
        assert st["candidates"] == len(at) and st["compares"] == 64 * len(at) and st["hits"] == 0
        assert check_grep(dev, dctx, none, 0x0A, True, ("64 absent patterns, grep", group)) == []
        # a hit across a record seam, one pattern per length
        seam = T.dec_off[1]
        for m in LENGTHS:
            pat = gm.cut(T.plain, 0x0A, seam - m // 2 - 1, m)
            check_both(dev, dctx, [pat, sm.SHORT1], 0x0A, ("record seam", m, group))
    finally:
        dctx.set_verify_group(0)


# ---- 5. refusals, cap and the chain into the multi-range decode ----
def test_grep_refuses_a_delimiter_in_a_pattern(files, devs, dctx):
    dev = devs["craft7_0a"]
    L = mc.lib()
    st = (ctypes.c_uint64 * 5)()

    def rc(pats, d, on):
        ps = mc.PatternSet(pats, on)
        try:
            k, p, ln, nb = dev.run
            return L.fcx_grep_set_shard(dctx._h, k.encode(), ctypes.c_void_p(p), ln, nb, d, ps.handle, None, None, 0, st, None, None)
        finally:
            ps.close()

    assert rc([b"ab", b"c\nd"], 0x0A, False) == FCX_ERR_ARG and b"holds the delimiter" in L.fcx_last_error()
    assert rc([b"ab", b"xay"], 0x41, False) == 0          # `a` is not `A` without the flag
    assert rc([b"ab", b"xay"], 0x41, True) == FCX_ERR_ARG and b"folded" in L.fcx_last_error()
    assert rc([b"xAy"], 0x41, True) == FCX_ERR_ARG
    assert rc([b"xay"], 0x61, True) == FCX_ERR_ARG


@pytest.mark.parametrize("group", GROUPS)
def test_cap_and_the_chain_into_the_ranges_decode(group, files, devs, dctx):
    import torch

    T, dev = files["craft8_0a"], devs["craft8_0a"]
    pats = [sm.SHORT1, sm.SHORT3, gm.MARK, sm.LONG]
    want = sm.selected_any(T.plain, pats, 0x0A)
    hits = sm.hits_any(T.plain, pats)
    n = len(want)
    dctx.set_verify_group(group)
    ps = mc.PatternSet(pats)
    try:
        for cap in (0, 1, n - 1, n, n + 8):
            st, got, behind, counts = dev.grep(dctx, ps, 0x0A, cap, keep=cap == n)
            assert st == sm.grep_stats(T.plain, pats, 0x0A, False, want) and got == want[:cap], (group, cap)
            assert behind == [CANARY] * len(behind) and counts == sm.counts(T.plain, pats)
        for cap in (0, 1, len(hits) - 1, len(hits) + 8):
            k, got, behind, counts = dev.find(dctx, ps, cap)
            assert k == len(hits) and got == hits[:cap] and behind == [CANARY] * len(behind), (group, cap)
        need = sum(e - s for s, e in want)
        out = torch.full((need + 64,), 0xA5, dtype=torch.uint8, device=dev.cuda)
        got = dctx.decompress_ranges_shard(*dev.run, dev.ds.data_ptr(), dev.de.data_ptr(), n, out.data_ptr(), need, stream=dev.stream)
        buf = out.cpu().numpy().tobytes()
        assert got == need and buf[:need] == gm.join(T.plain, want) and buf[need:] == b"\xA5" * 64
    finally:
        ps.close()
        dctx.set_verify_group(0)


# ---- 6. a set of one pattern is the search and the grep ----
@pytest.mark.parametrize("group", GROUPS)
@pytest.mark.parametrize("name", NAMES)
def test_a_set_of_one_pattern_is_the_one_pattern_call(name, group, files, devs, dctx):
    import torch

    T, dev = files[name], devs[name]
    dctx.set_verify_group(group)
    try:
        for m in (1, 5, 256):
            pat = gm.cut(T.plain, 0x0A, T.dec_off[1] - m // 2, m)
            ps = mc.PatternSet([pat])
            try:
                cap = len(fm.hits(T.plain, pat)) + 3
                old = torch.full((cap,), CANARY, dtype=torch.int64, device=dev.cuda)
                n_old = dctx.find_shard(*dev.run, pat, old.data_ptr(), cap, dev.stream)
                judged_old = dctx.find_stats()["judged"]
                n, got, _, counts = dev.find(dctx, ps, cap)
                assert n == n_old and got == old.cpu().tolist()[:n] and counts == [n]
                assert dctx.set_scan_stats()["judged"] == judged_old
                lines = len(gm.selected(T.plain, pat, 0x0A)) + 3
                os_ = torch.full((lines,), CANARY, dtype=torch.int64, device=dev.cuda)
                oe = torch.full((lines,), CANARY, dtype=torch.int64, device=dev.cuda)
                st_old = dctx.grep_shard(*dev.run, pat, 0x0A, os_.data_ptr(), oe.data_ptr(), lines, dev.stream)
                st, sel, _, _ = dev.grep(dctx, ps, 0x0A, lines)
                assert st == [st_old[k] for k in mc.DContext.GREP_STATS]
                assert sel == list(zip(os_.cpu().tolist(), oe.cpu().tolist()))[:st[0]]
            finally:
                ps.close()
    finally:
        dctx.set_verify_group(0)


@pytest.mark.parametrize("group", GROUPS)
def test_one_context_through_old_and_new_calls(group, files, devs, cuda):
    T, dev = files["craft7_0a"], devs["craft7_0a"]
    d = mc.DContext(0)
    d.set_verify_group(group)
    ps = mc.PatternSet([sm.SHORT1, sm.SHORT3, sm.LONG], True)
    try:
        first = (d.find_shard(*dev.run, gm.MARK), d.find_stats())
        assert first[0] == len(fm.hits(T.plain, gm.MARK))
        check_find(dev, d, [sm.SHORT1, sm.SHORT3, sm.LONG], True, "reuse")
        g = d.grep_shard(*dev.run, gm.MARK, 0x0A)
        assert [g[k] for k in mc.DContext.GREP_STATS] == gm.stats(T.plain, gm.MARK, 0x0A)
        check_grep(dev, d, [sm.SHORT1, sm.SHORT3, sm.LONG], 0x0A, True, "reuse")
        assert d.grep_shard(*dev.run, gm.MARK, 0x0A) == g
        assert (d.find_shard(*dev.run, gm.MARK), d.find_stats()) == first
        assert d.find(T.blob, gm.MARK)[1] == fm.hits(T.plain, gm.MARK)
    finally:
        ps.close()
        d.close()


# ---- 7. the host and the stream forms ----
def stream_both(dctx, T: Truth, pats, on: bool, d: int = 0x0A):
    ps = mc.PatternSet(pats, on)
    try:
        fs, hits, fc = dctx.find_set_stream(io.BytesIO(T.blob), ps, len(T.blob) - 10)
        sc = dctx.set_scan_stats()
        gs, lines, gc = dctx.grep_set_stream(io.BytesIO(T.blob), ps, d, len(T.blob) - 10)
        n, host_hits, hc = dctx.find_set(T.blob, ps)
        hs, out, oc = dctx.grep_set_host(T.blob, ps, d)
    finally:
        ps.close()
    want, sel, wc = sm.hits_any(T.plain, pats, on), sm.selected_any(T.plain, pats, d, on), sm.counts(T.plain, pats, on)
    assert hits == want and host_hits == want and n == len(want)
    assert fs == {"hits": len(want), "decoded": T.total, "records": T.n, "judged": sm.judged(T.plain, pats)}
    assert sc["judged"] == sm.judged(T.plain, pats) and sc["hits"] == len(want)
    assert fc == wc and gc == wc and hc == wc and oc == wc
    stats = sm.grep_stats(T.plain, pats, d, on, sel)
    assert lines == sel and [gs[k] for k in mc.DContext.GREP_STATS] == stats
    assert out == gm.join(T.plain, sel) and [hs[k] for k in mc.DContext.GREP_STATS] == stats
    return sc


@pytest.mark.parametrize("group", GROUPS)
@pytest.mark.parametrize("window", [0, 7])
@pytest.mark.parametrize("name", ["f7_seam", "f7_seam_empty"])
def test_short_patterns_at_the_stream_seam_count_once(name, window, group, files, dctx):
    """under a bound a stream group is cut into decode groups, so the carry, the delimiter bits of the judged positions
    alone and the held-back line pass from a stream group's last decode group, which is not final, into the next
    stream group or into the final pass"""
    T = files[name]
    dctx.set_find_window(window)
    dctx.set_verify_group(group)
    try:
        for on in (False, True):
            sc = stream_both(dctx, T, [sm.SHORT1, sm.SHORT3, sm.LONG], on)
            assert sc["final_passes"] == 1   # the carry behind the last group, which in f7_seam_empty decodes to no bytes
        stream_both(dctx, T, [gm.cut(T.plain, 0x0A, 255985, 10), gm.cut(T.plain, 0x0A, T.total - 3, 3), sm.SHORT1], False)
        sc = stream_both(dctx, T, [sm.SHORT1, b"q"], True)   # M == 1: nothing is carried, the end is still one final pass
        assert sc["final_passes"] == 1
    finally:
        dctx.set_find_window(0)
        dctx.set_verify_group(0)


@pytest.mark.parametrize("group", [1, 3000])
def test_trailing_records_of_no_bytes_in_the_shard_form(group, files, devs, dctx):
    """f7_seam_empty through the shard forms: the run's last decode groups hold no byte, so the final range is the carry"""
    dev = devs["f7_seam_empty"]
    dctx.set_verify_group(group)
    try:
        check_both(dev, dctx, [sm.SHORT1, sm.SHORT3, sm.LONG], 0x0A, ("f7_seam_empty", group))
        check_both(dev, dctx, [sm.SHORT3], 0x0A, ("f7_seam_empty, one length", group), folds=(False,))
    finally:
        dctx.set_verify_group(0)


@pytest.mark.parametrize("group", GROUPS)
@pytest.mark.parametrize("name", ["craft7_0a", "craft8_ff", "f7_tiny", "f7_empty", "f7_mixed"])
def test_the_host_and_stream_forms(name, group, files, dctx):
    T = files[name]
    d = int(name[-2:], 16) if name.startswith("craft") else 0x0A
    dctx.set_find_window(7)
    dctx.set_verify_group(group)
    try:
        sets = [[sm.SHORT1, sm.SHORT3, sm.LONG], [sm.UP, sm.FOLD_PAT]] if name.startswith("craft") else [[b"e", b"the", sm.LONG], [b"TH", b"qu"]]
        for pats in sets:
            for on in (False, True):
                stream_both(dctx, T, pats, on, d)
    finally:
        dctx.set_find_window(0)
        dctx.set_verify_group(0)


def test_the_module_functions(files):
    """(each makes a context of its own, so the group bound, a setting of a context, is the default here)"""
    T = files["craft7_0a"]
    pats = [sm.UP, sm.SHORT3]
    hits, counts = mc.find_any(T.blob, pats, ignore_case=True)
    assert hits == sm.hits_any(T.plain, pats, True) and counts == sm.counts(T.plain, pats, True)
    assert mc.find_any(T.blob, pats, max_hits=2)[0] == sm.hits_any(T.plain, pats)[:2]
    sel = sm.selected_any(T.plain, pats, 0x0A, True)
    assert mc.grep_any(T.blob, pats, ignore_case=True) == gm.join(T.plain, sel)
    st, lines, counts = mc.grep_any_ranges(T.blob, pats, ignore_case=True)
    assert lines == sel and counts == sm.counts(T.plain, pats, True)
