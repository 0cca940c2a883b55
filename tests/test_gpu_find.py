"""Search of device-resident runs: fcx_find_shard, fcx_find_host and fcx_find_stream (fcx_find.hip: k_fscan,
k_fbase, k_fwrite, k_fcarry) for FCX7 and FCX8.

Truth is never the code under test: the files come from the oracle's encoders, `plain` is the join of the
oracle's decode of every record (Truth of test_gpu_range.py), the expected hits are bytes.find over it
(find_model.hits), and every (file, pattern) pair is compared in full: the count and every offset.

The patterns are cut from `plain` (find_model.patterns): lengths 1 .. 256 at the run's two ends, around the
record seams (s - 1, s - m + 1, s - m // 2), around the tile seam (4095, 4096) and at an address whose low
four bits are set.  The files of up to 8 records take every seam; f7_many and f8_batch have 299 seams each,
and every length at every seam through six settings would be some 75000 calls, so there all 14 lengths go to
the first seam, the seams around the stream form's 256-record group (255, 256, 257) and the last one, and
test_every_seam_of_the_many_record_files gives each of the 299 seams one length in turn.  Under a group bound
(1 or 3000 bytes) those two files make 100 to 300 decode groups per call, some 50 ms each, so there they are
searched for seven of the lengths at the run's ends and around the 256-record seam (`cases`, light)."""
import ctypes
import io

import pytest

import find_model as model
import inputs
import my_compress_amd as mc
from test_gpu_range import Truth

pytestmark = pytest.mark.gpu

FCX_ERR_FORMAT = -4
NAMES = ["f7_mixed", "f7_runs", "f7_many", "f8_zeros", "f8_tail", "f8_batch"]
GROUPS = [0, 1, 3000]
CANARY = 0x5A5A5A5A5A5A5A5A


@pytest.fixture(scope="module")
def files():
    F = {}
    F["f7_mixed"] = Truth("7", model.mixed_data(), 4096)
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
    F["f7_tiny"] = Truth("7", model.text(7, 100), 4096)   # shorter than the longest pattern
    assert F["f7_tiny"].sizes == [100]
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

        self.T = T
        self.recs = T.recs if recs is None else recs
        self.d_in = torch.frombuffer(bytearray(self.recs), dtype=torch.uint8).to(cuda)
        self.stream = torch.cuda.current_stream().cuda_stream

    def find(self, dctx, pat: bytes, cap: int = None, room: int = None):
        """fcx_find_shard: (count, the first min(cap, count) offsets, the entries of d_hits behind them);
        cap None: room for all (a count call first)"""
        import torch

        args = (self.T.kind, self.d_in.data_ptr(), len(self.recs), self.T.n, pat)
        if cap is None:
            cap = dctx.find_shard(*args)
        if cap == 0 and room is None:
            return dctx.find_shard(*args), [], []
        room = cap if room is None else room
        d_hits = torch.full((room + 8,), CANARY, dtype=torch.int64, device=self.d_in.device)
        n = dctx.find_shard(*args, d_hits=d_hits.data_ptr(), cap=cap, stream=self.stream)
        got = d_hits.cpu().tolist()
        k = min(cap, n)
        return n, got[:k], got[k:]


@pytest.fixture(scope="module")
def devs(files, cuda):
    return {name: Dev(cuda, T) for name, T in files.items()}


def seams_of(T: Truth):
    s = sorted(set(T.dec_off[1:-1]))
    if len(s) <= 8:
        return s
    return [T.dec_off[k] for k in (1, 255, 256, 257, T.n - 1)]


LIGHT = [1, 4, 5, 16, 33, 255, 256]   # lengths of the many-record files under a group bound (below)


@pytest.fixture(scope="module")
def cases(files):
    """per (file, light?): [(pattern, its expected hits)], computed once.  light: what a file of 300 records
    is searched for when a group bound makes 100 or 300 decode groups of it, at some 50 ms a call: seven
    lengths at the run's ends and around the seam of the stream form's groups."""
    C = {}
    for name in NAMES:
        T = files[name]
        pats = model.patterns(T.plain, seams_of(T)) + [model.absent(T.plain)]
        C[name, False] = [(p, model.hits(T.plain, p)) for p in pats]
        assert all(h for _, h in C[name, False][:-1]) and C[name, False][-1][1] == []
        if T.n > 8:
            few = {T.plain[p:p + m] for m in LIGHT for p in (0, T.total - m, T.dec_off[256] - 1, T.dec_off[256] - m + 1,
                                                           T.dec_off[256] - m // 2) if p >= 0}
            C[name, True] = [c for c in C[name, False] if c[0] in few] + [C[name, False][-1]]
            assert len(C[name, True]) >= 20
    return C


def judged(T: Truth, m: int) -> int:
    return max(T.total - m + 1, 0)


# ---- 1. every pattern, every file, both forms, three group bounds ----
@pytest.mark.parametrize("group", GROUPS)
@pytest.mark.parametrize("form", ["shard", "host"])
@pytest.mark.parametrize("name", NAMES)
def test_patterns_cut_from_the_decoded_bytes(name, form, group, files, devs, cases, dctx):
    T, dev = files[name], devs[name]
    dctx.set_verify_group(group)
    try:
        for pat, want in cases[name, group != 0 and T.n > 8]:
            room = len(want) + 3   # (more than there are: one call gives the count and all offsets)
            if form == "shard":
                n, got, _ = dev.find(dctx, pat, cap=room)
            else:
                n, got = dctx.find(T.blob, pat, max_hits=room)
            assert n == len(want), (name, form, group, len(pat), pat[:16], n, len(want))
            assert got == want, (name, form, group, len(pat), pat[:16])
            st = dctx.find_stats()
            if form == "shard" or T.n <= 256:   # (the host form reports its last stream group)
                assert st["judged"] == judged(T, len(pat)), (name, form, group, len(pat), st)
                assert st["hits"] == len(want) and st["candidates"] >= len(want)
        if form == "shard" and group == 1:
            assert dctx.verify_groups() == T.n   # every record a group: the carry spans groups shorter than the pattern
    finally:
        dctx.set_verify_group(0)


def stream_find(dctx, blob: bytes, pat: bytes):
    """fcx_find_stream over memory: (stats, the offsets on_hit was called with)"""
    src = io.BytesIO(blob)

    def rd(_u, buf, cap):
        chunk = src.read(cap)
        ctypes.memmove(buf, chunk, len(chunk))
        return len(chunk)

    got = []
    cb = mc.HIT_FN(lambda _u, off: got.append(int(off)))
    stats = (ctypes.c_uint64 * 4)()
    rc = mc.lib().fcx_find_stream(dctx._h, mc.READ_FN(rd), None, len(blob) - 10, pat, len(pat), cb, None, stats)
    assert rc == 0, mc.lib().fcx_last_error()
    return [int(v) for v in stats], got


@pytest.mark.parametrize("name", ["f7_many", "f8_batch"])
def test_every_seam_of_the_many_record_files(name, files, devs, dctx):
    T, dev = files[name], devs[name]
    seen = set()
    for k in range(1, T.n):
        s, m = T.dec_off[k], model.LENGTHS[k % len(model.LENGTHS)]
        for p in (s - 1, s - m + 1, s - m // 2):
            pat = T.plain[p:p + m]
            if p < 0 or len(pat) < m or pat in seen:
                continue
            seen.add(pat)
            want = model.hits(T.plain, pat)
            n, got, _ = dev.find(dctx, pat)
            assert (n, got) == (len(want), want), (name, k, m, p)
            assert dctx.find_stats()["judged"] == judged(T, m)


@pytest.mark.parametrize("name", ["f7_many", "f8_batch"])
def test_the_stream_form_sums_its_groups(name, files, dctx):
    T = files[name]   # 300 records: a stream group of 256 and one of 44
    s = T.dec_off[256]
    for m in (2, 33, 256):
        for p in (s - 1, s - m + 1, s - m // 2):
            pat = T.plain[p:p + m]
            want = model.hits(T.plain, pat)
            stats, got = stream_find(dctx, T.blob, pat)
            assert got == want and p in want and s - m < p < s   # one hit lies across the two stream groups
            assert stats == [len(want), T.total, T.n, judged(T, m)]


# ---- 2. the cases the issue names ----
def test_overlapping_hits(files, devs, dctx):
    T, dev = files["f7_runs"], devs["f7_runs"]
    assert len(set(T.plain[:30])) == 1   # the file starts with a run of 30 equal bytes
    pat = T.plain[:3]
    want = model.hits(T.plain, pat)
    assert len(want) == 46898 and sum(1 for a, b in zip(want, want[1:]) if b - a < 3) == 45789
    n, got, _ = dev.find(dctx, pat)
    assert (n, got) == (len(want), want)


def test_every_position_a_candidate(files, devs, dctx):
    T, dev = files["f8_zeros"], devs["f8_zeros"]
    pat = bytes(256)
    n, got, _ = dev.find(dctx, pat)
    assert n == 99745 and got == list(range(99745)) == model.hits(T.plain, pat)
    st = dctx.find_stats()
    assert st["judged"] == st["candidates"] == st["hits"] == 99745


def test_a_pattern_longer_than_the_run(files, devs, dctx):
    T, dev = files["f7_tiny"], devs["f7_tiny"]
    for group in GROUPS:
        dctx.set_verify_group(group)
        assert dev.find(dctx, T.plain + bytes(156))[:2] == (0, [])
        assert dctx.find_stats()["judged"] == 0
        assert dctx.find(T.blob, T.plain + bytes(156)) == (0, [])
        assert dev.find(dctx, T.plain)[:2] == (1, [0])   # exactly the run
        assert dctx.find_stats()["judged"] == 1
    dctx.set_verify_group(0)


def test_spaces_of_the_many_record_file(files, devs, dctx):
    T, dev = files["f7_many"], devs["f7_many"]
    want = model.hits(T.plain, b" ")
    assert len(want) == 44438
    assert dev.find(dctx, b" ")[:2] == (44438, want)


# ---- 3. cap ----
@pytest.mark.parametrize("name,lo,hi", [("f7_mixed", 100, 102), ("f7_runs", 0, 3)])
def test_cap(name, lo, hi, files, devs, dctx):
    T, dev = files[name], devs[name]
    pat = T.plain[lo:hi]
    want = model.hits(T.plain, pat)
    H = len(want)
    assert H >= 2
    assert dev.find(dctx, pat, cap=0) == (H, [], [])   # NULL, 0: the count alone
    for cap in (1, H - 1, H, H + 5):
        n, got, behind = dev.find(dctx, pat, cap=cap, room=H + 5)
        assert n == H and got == want[:cap], (name, cap)
        assert behind == [CANARY] * len(behind), f"cap {cap}: entries behind d_hits[min(cap, hits)) were written"


# ---- 4. the stream form's window ----
def test_window_of_7_on_43_hits(files, dctx):
    T = files["f7_mixed"]
    pat = T.plain[100:102]
    want = model.hits(T.plain, pat)
    assert len(want) == 43
    dctx.set_find_window(7)
    try:
        assert dctx.find(T.blob, pat) == (43, want)
        assert dctx.find_stats()["windows"] == 7   # 43 hits by 7
        assert dctx.find(T.blob, pat, max_hits=10) == (43, want[:10])
        assert dctx.find(T.blob, pat, max_hits=0) == (43, [])
    finally:
        dctx.set_find_window(0)
    assert dctx.find(T.blob, pat) == (43, want)


def test_window_of_1000_on_the_spaces(files, dctx):
    T = files["f7_many"]
    want = model.hits(T.plain, b" ")
    assert len(want) == 44438
    dctx.set_find_window(1000)
    try:
        stats, got = stream_find(dctx, T.blob, b" ")
        assert got == want and stats == [44438, T.total, 300, T.total]
    finally:
        dctx.set_find_window(0)


# ---- 5. a damaged record ----
def test_a_damaged_record_is_a_format_error(files, cuda, dctx):
    import torch

    T = files["f7_mixed"]
    recs = bytearray(T.recs)
    a, b = T.rec_off[5] + 4, T.rec_off[6]
    recs[a:b] = b"\xFF" * (b - a)   # record 5's payload, its length prefix kept
    bad = Dev(cuda, T, bytes(recs))
    d_out = torch.zeros(T.total + 64, dtype=torch.uint8, device=cuda)
    got = ctypes.c_uint64(0)
    L = mc.lib()
    assert L.fcx_decompress_shard(dctx._h, ctypes.c_void_p(bad.d_in.data_ptr()), len(bad.recs), T.n,
                                  ctypes.c_void_p(d_out.data_ptr()), T.total + 64, ctypes.byref(got), None) == FCX_ERR_FORMAT
    n = ctypes.c_uint64(7)
    pat = T.plain[100:102]
    assert L.fcx_find_shard(dctx._h, b"7", ctypes.c_void_p(bad.d_in.data_ptr()), len(bad.recs), T.n, pat, 2, None, 0,
                            ctypes.byref(n), None) == FCX_ERR_FORMAT
    with pytest.raises(mc.FcxError):
        dctx.find(T.blob[:10] + bytes(recs), pat)
    assert Dev(cuda, T).find(dctx, pat)[0] == 43   # the context is as good as before


# ---- 6. one context for everything ----
def test_one_context_verify_find_range_find(files, devs, cuda):
    import torch

    T, dev = files["f7_mixed"], devs["f7_mixed"]
    pat = T.plain[8189:8196]   # across the three empty records
    want = model.hits(T.plain, pat)
    assert want == [8189]
    d = mc.DContext(0)
    try:
        orig = model.mixed_data()
        d_orig = torch.frombuffer(bytearray(orig), dtype=torch.uint8).to(cuda)
        st = d.verify_shard(dev.d_in.data_ptr(), len(dev.recs), T.n, "7", d_orig.data_ptr(), len(orig), 4096)
        assert st["differ"] == 3
        assert dev.find(d, pat)[:2] == (1, want)
        assert d.decompress_range_host(T.blob, 8000, 400) == T.plain[8000:8400]
        assert dev.find(d, pat)[:2] == (1, want)
        assert d.find(T.blob, pat) == (1, want)
    finally:
        d.close()
