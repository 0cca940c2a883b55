"""Cut on device-resident runs: fcx_cut_buffer, fcx_cut_shard, fcx_cut_ranges_shard (fcx_cut.hip: a segmented tick count
that resets at every delimiter and runs across tiles and groups, then a stable compaction of the kept bytes to any
output alignment) and the stream and host forms, for FCX7 and FCX8.

Truth is never the code under test: the files come from the oracle's encoders, `plain` is the join of the oracle's
decode of every record (Truth of test_gpu_range.py), the expected bytes and stats are cut_model's numpy form over it
(pinned against its per-byte form and GNU cut in test_cut_model.py), the blocks of the ranges form are context_model's
and regex_model's.  Every call is compared in full: every output byte, the six stats, the canaries behind
min(cap, total).  The crafted files' plants are asserted in the oracle's bytes.  Calls run under the group bounds 0, 1
and 3000 in the shard, host and stream forms; the answer must not depend on where records, tiles, decode groups or stream
groups end."""
import functools
import io

import numpy as np
import pytest

import context_model as cm
import cut_model as km
import find_model as fm
import my_compress_amd as mc
import regex_model as rm
from test_gpu_range import Truth

pytestmark = pytest.mark.gpu

GROUPS = [0, 1, 3000]
CANARY = 0xA5
KEYS = mc.DContext.CUT_STATS
N = 4 * 4096
EXPR = b"[a-z],[a-z]"
# (delimiter, separator, kind): the LZ78 reference drops a zero byte that opens a record, so a file with planted zeros is FCX7 alone
CRAFT = [(0x0A, 0x2C, "7"), (0x0A, 0x2C, "8"), (0x00, 0x09, "7"), (0x41, 0x00, "7")]
D_AT = sorted(set(range(301, N, 523)) | {8191, 8192, N - 1})
S_AT = sorted((set(range(7, N, 37)) | {4095, 4096, 8190, 12280, 12295}) - set(range(12281, 12295)) - set(D_AT))
SPECS = [("2", None, False), ("1,3-4", None, False), ("2-", None, True), ("5", None, False), (None, "1-16", False), (None, "3,40-", True)]


def spec_of(s, sep, d):
    """(fields, byte_list, complement) of SPECS -> the hashable key of want() and of cut_obj()"""
    return (s[0], s[1], sep, d, s[2])


@functools.lru_cache(maxsize=None)
def want(plain: bytes, spec):
    fields, byte_list, sep, d, comp = spec
    mode, sel = km.make_sel(fields, byte_list, comp)
    return km.cut_np(plain, sel, mode, sep, d)


def cut_obj(spec):
    fields, byte_list, sep, d, comp = spec
    return mc.Cut(fields, byte_list, bytes([sep]), bytes([d]), comp)


def plant(data: bytes, d: int, sep: int, d_at, s_at) -> bytes:
    """data with d and sep at the given offsets and nowhere else"""
    b = bytearray(x if x not in (d, sep) else 0x78 for x in data)
    for p in d_at:
        b[p] = d
    for p in s_at:
        b[p] = sep
    return bytes(b)


def crafted(d: int, sep: int) -> bytes:
    return plant(km.text(51 + d, N), d, sep, D_AT, S_AT)


def check_crafted(plain: bytes, d: int, sep: int):
    """the plants, asserted in the oracle's decoded bytes"""
    assert len(plain) == N and [i for i, b in enumerate(plain) if b == d] == D_AT and [i for i, b in enumerate(plain) if b == sep] == S_AT
    assert plain[4095] == sep and plain[4096] == sep            # a separator as a tile's (and a record's) last and first byte
    assert plain[8191] == d and plain[8192] == d                # the delimiter as a tile's last byte and as the next tile's first
    assert plain[12280] == sep and plain[12295] == sep and d not in plain[12281:12295] and sep not in plain[12281:12295]
    assert 12280 // 4096 == 2 and 12295 // 4096 == 3            # ... and a field across that tile and record seam


BATCH = {"7": 1000, "8": 256}


def batch_file(kind: str) -> bytes:
    """300 records with a field open across the stream form's group seam (record 256), the line's earlier separators
    in the group before"""
    n, seam = 300 * BATCH[kind], 256 * BATCH[kind]
    d_at = [p for p in range(211, n, 997) if not seam - 400 <= p < seam + 300]
    s_at = [p for p in range(5, n, 41) if not seam - 5 < p < seam + 6 and p not in d_at] + [seam - 5, seam + 6]
    return plant(km.text(11, n), 0x0A, 0x2C, d_at, s_at)


def long_line(mode: str) -> bytes:
    """one line whose tick count passes the bound in the second tile, then a short line"""
    if mode == "f":
        return b",".join(b"%d" % (i % 10) for i in range(5001)) + b"\nq,r,s\n"
    return bytes(97 + i % 26 for i in range(5000)) + b"\nqrs\n"


def step_file() -> bytes:
    """9 MiB whose first 5 MiB are one line"""
    chunk = km.table(60000, 0x0A, 0x20, 3)
    a = np.frombuffer(bytearray((chunk * ((9 << 20) // len(chunk) + 1))[:9 << 20]), dtype=np.uint8)
    head = a[:5 << 20]
    head[head == 0x0A] = 0x2E
    return a.tobytes()


def make_files():
    F = {}
    for d, sep, kind in CRAFT:
        T = F[f"craft{kind}_{d:02x}"] = Truth(kind, crafted(d, sep), 4096)
        assert T.sizes == [4096] * 4
        check_crafted(T.plain, d, sep)
    nd = plant(km.text(5, 9000), 0x0A, 0x2C, [], [100, 4000, 4095, 4096, 6000, 8191, 8192, 8990])
    F["f7_nodelim"] = T = Truth("7", nd, 4096)   # one line of 9000 bytes over three tiles, its separators in all three
    assert T.plain == nd and 0x0A not in T.plain and T.sizes == [4096, 4096, 808]
    for m in "fb":
        for kind in "78":
            T = F[f"f{kind}_long_{m}"] = Truth(kind, long_line(m), 4096)
            assert T.plain == long_line(m)
    assert long_line("f").index(b"\n") == 10001 and long_line("f")[:10001].count(b",") == 5000 and long_line("b").index(b"\n") == 5000
    for kind in "78":
        T = F[f"f{kind}_batch"] = Truth(kind, batch_file(kind), BATCH[kind])
        seam = 256 * BATCH[kind]
        assert T.sizes == [BATCH[kind]] * 300 and T.dec_off[256] == seam and T.plain == batch_file(kind)
        line = T.plain[T.plain.rfind(b"\n", 0, seam) + 1:T.plain.index(b"\n", seam)]
        assert b"," not in T.plain[seam - 4:seam + 6] and T.plain[seam - 5] == 0x2C and line.count(b",") > 10
    F["f7_seam_empty"] = T = Truth("7", batch_file("7")[:256000] + fm.rand(5, 3000), 1000)   # the last records decode to no byte
    assert T.sizes == [1000] * 256 + [0] * 3
    F["f7_empty"] = Truth("7", fm.rand(3, 3000), 1000)   # three records, T == 0
    assert F["f7_empty"].sizes == [0, 0, 0]
    F["f7_tail"] = Truth("7", b"a,b\nc,d", 4096)          # an unterminated tail
    F["f7_xsd"] = Truth("7", b"x,\n" * 4096, 4096)
    F["f7_nosep"] = Truth("7", b"a,b\nnosep\nc,d\n", 4096)   # a line with no separator
    for name in ("f7_tail", "f7_xsd", "f7_nosep"):
        assert F[name].total == {"f7_tail": 7, "f7_xsd": 12288, "f7_nosep": 14}[name]
    return F


@pytest.fixture(scope="module")
def files():
    return make_files()


@pytest.fixture(scope="module")
def dctx(cuda):
    d = mc.DContext(0)
    yield d
    d.set_verify_group(0)
    d.close()


class Dev:
    """a file's records on the device"""

    def __init__(self, cuda, T: Truth):
        import torch

        self.T, self.cuda = T, cuda
        self.d_in = torch.frombuffer(bytearray(T.recs), dtype=torch.uint8).to(cuda)
        self.stream = torch.cuda.current_stream().cuda_stream
        self.run = (T.kind, self.d_in.data_ptr(), len(T.recs), T.n)

    def out(self, cap):
        import torch

        return torch.full((cap + 64,), CANARY, dtype=torch.uint8, device=self.cuda)

    def cut(self, dctx, ct, cap: int, query: bool = False):
        """fcx_cut_shard: (total, stats, the first min(cap, total) bytes, what lies behind them)"""
        buf = self.out(cap)
        total, st = dctx.cut_shard(*self.run, ct, 0 if query else buf.data_ptr(), cap, self.stream)
        raw = buf.cpu().numpy().tobytes()
        k = min(cap, total)
        return total, [st[n] for n in KEYS], raw[:k], raw[k:]


@pytest.fixture(scope="module")
def devs(files, cuda):
    return {name: Dev(cuda, T) for name, T in files.items()}


def groups_of(sizes, bound: int) -> int:
    """the run core's groups: consecutive records whose decoded bytes (a record of none counts as one) fit the bound"""
    bound = bound or 256 << 20
    n, cost = 0, None
    for s in sizes:
        c = max(s, 1)
        if cost is None or cost + c > bound:
            n, cost = n + 1, 0
        cost += c
    return n


def check_forms(name, files, devs, dctx, spec, group, caps=()):
    T, dev = files[name], devs[name]
    out, stats = want(T.plain, spec)
    ct = cut_obj(spec)
    dctx.set_verify_group(group)
    try:
        total, st, got, behind = dev.cut(dctx, ct, len(out) + 5)
        assert total == len(out) and st == stats + [groups_of(T.sizes, group)], (name, spec, group, st, stats)
        assert got == out, (name, spec, group)
        assert behind == bytes([CANARY]) * len(behind), (name, spec, group, "bytes behind the output were written")
        assert [dctx.cut_stats()[k] for k in KEYS] == st and dctx.verify_groups() == st[5]
        if T.total:
            most = T.total if group == 0 else max(max(T.sizes), group)   # a keep bitmap and four words per tile of the largest group
            assert 0 < dctx.cut_scratch() <= (512 + 16) * (most // 4096 + 1), (name, group, dctx.cut_scratch())
        for cap in caps:
            query = cap == 0
            total, st, got, behind = dev.cut(dctx, ct, cap, query)
            assert total == len(out) and st[:5] == stats, (name, spec, group, cap)
            assert got == out[:cap] and behind == bytes([CANARY]) * len(behind), (name, spec, group, cap)
        # the stream form (groups of 256 records) and the host forms
        sink = io.BytesIO()
        gs = dctx.cut_stream(io.BytesIO(T.blob), sink, ct, len(T.blob) - 10)
        sgroups = sum(groups_of(T.sizes[i:i + 256], group) for i in range(0, T.n, 256))
        assert sink.getvalue() == out and [gs[k] for k in KEYS] == stats + [sgroups], (name, spec, group, "stream", gs)
        assert dctx.cut_stream(io.BytesIO(T.blob), None, ct) == gs
        total, hs, hout = dctx.cut_host(T.blob, ct)
        assert (total, hout) == (len(out), out) and [hs[k] for k in KEYS] == stats + [sgroups], (name, spec, group, "host")
        assert dctx.cut_host(T.blob, ct, size_only=True)[::2] == (len(out), b"")
    finally:
        ct.close()
        dctx.set_verify_group(0)


# ---- 1. the crafted file: separators and delimiters at the seams, three delimiters and separators, both kinds, three forms ----
@pytest.mark.parametrize("group", GROUPS)
@pytest.mark.parametrize("d,sep,kind", CRAFT)
def test_the_crafted_file(d, sep, kind, group, files, devs, dctx):
    name = f"craft{kind}_{d:02x}"
    total = len(want(files[name].plain, spec_of(SPECS[0], sep, d))[0])
    for i, s in enumerate(SPECS):
        check_forms(name, files, devs, dctx, spec_of(s, sep, d), group, caps=(0, 1, total - 1, total // 2 + 3) if i == 0 else ())
    if group == 1:
        assert dctx.verify_groups() == 4   # every record a group


@pytest.mark.parametrize("group", GROUPS)
def test_one_line_over_three_tiles(group, files, devs, dctx):
    """no delimiter at all: the column of a byte in the third tile counts separators of the first"""
    for s in SPECS + [("9", None, False), ("8-", None, False)]:
        check_forms("f7_nodelim", files, devs, dctx, spec_of(s, 0x2C, 0x0A), group)
    assert want(files["f7_nodelim"].plain, spec_of(("9", None, False), 0x2C, 0x0A))[0] == files["f7_nodelim"].plain[8991:]


# ---- 2. the counter saturates in the second tile ----
@pytest.mark.parametrize("group", [0, 3000])
@pytest.mark.parametrize("kind", "78")
@pytest.mark.parametrize("mode", "fb")
def test_the_saturated_count(mode, kind, group, files, devs, dctx):
    for lst, comp in (("4096", False), ("4097-", False), ("1-4096", False), ("2-", True), ("4097-", True), ("1-4096", True)):
        s = (lst, None, comp) if mode == "f" else (None, lst, comp)
        check_forms(f"f{kind}_long_{mode}", files, devs, dctx, spec_of(s, 0x2C, 0x0A), group)
    T = files[f"f{kind}_long_{mode}"]
    if mode == "f":   # field 4097 and on: the separator that opens 4097 is dropped, the later ones are kept
        cells = T.plain.split(b"\n")[0].split(b",")
        assert want(T.plain, spec_of(("4097-", None, False), 0x2C, 0x0A))[0] == b",".join(cells[4096:]) + b"\n\n"


# ---- 3. the stream form's seam, records of no bytes, T == 0, tails, tiny lines ----
@pytest.mark.parametrize("kind", "78")
def test_a_field_across_the_stream_group_seam(kind, files, devs, dctx):
    for group in (0, 3000):
        for s in SPECS[:3] + [(None, "1-16", False)]:
            check_forms(f"f{kind}_batch", files, devs, dctx, spec_of(s, 0x2C, 0x0A), group)


@pytest.mark.parametrize("group", GROUPS)
def test_small_and_empty_files(group, files, devs, dctx):
    for name in ("f7_seam_empty", "f7_empty", "f7_tail", "f7_xsd", "f7_nosep"):
        if name == "f7_seam_empty" and group == 1:
            continue   # (259 decode groups: the other bounds cover the file)
        for s in SPECS[:4] + [(None, "2", False)]:
            check_forms(name, files, devs, dctx, spec_of(s, 0x2C, 0x0A), group, caps=(0, 1) if name == "f7_tail" else ())
    f2 = spec_of(("2", None, False), 0x2C, 0x0A)
    assert want(files["f7_nosep"].plain, f2)[0] == b"b\n\nd\n"     # the first difference from GNU cut
    assert want(files["f7_tail"].plain, f2)[0] == b"b\nd"          # the second
    assert want(files["f7_xsd"].plain, f2)[0] == b"\n" * 4096


# ---- 4. fcx_cut_buffer: sizes around a piece and a tile, any alignment of the source and the destination ----
@pytest.mark.parametrize("n", [0, 1, 15, 16, 17, 4095, 4096, 4097])
def test_cut_buffer_sizes_and_alignments(n, cuda, dctx):
    import torch

    d, sep = 0x0A, 0x2C
    plain = crafted(d, sep)[4090:4090 + n] if n else b""
    stream = torch.cuda.current_stream().cuda_stream
    for s in (("2", None, False), (None, "2-5", False), ("1", None, True)):
        spec = spec_of(s, sep, d)
        out, stats = want(plain, spec)
        ct = cut_obj(spec)
        try:
            for so in (0, 1, 15):
                # around the source: delimiters and separators, which would change the answer if they were read
                src = torch.frombuffer(bytearray(b"\n," * 8 + b"\n" * so + plain + b",\n" * 16), dtype=torch.uint8).to(cuda)
                assert src.data_ptr() % 16 == 0
                for do in (0, 1, 15):
                    for cap in {len(out) + 3, max(len(out) - 1, 0), len(out) // 2}:
                        buf = torch.full((cap + 96,), CANARY, dtype=torch.uint8, device=cuda)
                        assert buf.data_ptr() % 16 == 0
                        total, st = dctx.cut_buffer(src.data_ptr() + 16 + so, n, ct, buf.data_ptr() + 16 + do if cap else 0, cap, stream)
                        raw = buf.cpu().numpy().tobytes()
                        k = min(cap, total)
                        assert total == len(out) and [st[x] for x in KEYS] == stats + [1 if n else 0], (n, s, so, do, cap, st)
                        assert raw[16 + do:16 + do + k] == out[:k], (n, s, so, do, cap)
                        assert raw[:16 + do] + raw[16 + do + k:] == bytes([CANARY]) * (len(raw) - k), (n, s, so, do, cap)
        finally:
            ct.close()


# ---- 5. fcx_cut_ranges_shard on the grep's arrays: zgrep | cut ----
@pytest.mark.parametrize("kind", "78")
def test_cut_of_the_greps_blocks(kind, files, devs, dctx, cuda):
    import torch

    name = f"craft{kind}_0a"
    T, dev = files[name], devs[name]
    d, sep = 0x0A, 0x2C
    word = T.plain[2000:2003]
    assert bytes([d]) not in word
    arr = [torch.zeros(4096, dtype=torch.int64, device=cuda) for _ in range(3)]
    ptr = [a.data_ptr() for a in arr]
    ps = mc.PatternSet([word, b"the"])
    rx = mc.Regex(EXPR, d)
    try:
        for invert, before, after in ((False, 0, 0), (True, 0, 0), (False, 1, 2), (True, 2, 0)):
            calls = [(cm.blocks(T.plain, [word, b"the"], d, False, invert, before, after),
                      lambda: dctx.grep_blocks_shard(*dev.run, ps, d, invert, before, after, d_start=ptr[0], d_end=ptr[1], d_line=ptr[2],
                                                     cap=4096, stream=dev.stream)[0]),
                     (rm.blocks(T.plain, rm.Nfa(EXPR, d), invert, before, after),
                      lambda: dctx.grep_regex_blocks_shard(*dev.run, rx, invert, before, after, d_start=ptr[0], d_end=ptr[1], d_line=ptr[2],
                                                           cap=4096, stream=dev.stream))]
            for blk, call in calls:
                st = call()
                assert st["blocks"] == len(blk) and 0 < len(blk) <= 4096, (invert, before, after)
                joined = cm.join(T.plain, blk)
                for group in (0, 3000):
                    dctx.set_verify_group(group)
                    for s in SPECS[:3] + [(None, "1-16", False)]:
                        spec = spec_of(s, sep, d)
                        out, stats = want(joined, spec)
                        ct = cut_obj(spec)
                        for cap in (len(out) + 7, 0, len(out) // 2):
                            buf = dev.out(cap)
                            total, cs = dctx.cut_ranges_shard(*dev.run, ptr[0], ptr[1], len(blk), ct, buf.data_ptr() if cap else 0, cap,
                                                              stream=dev.stream)
                            raw = buf.cpu().numpy().tobytes()
                            k = min(cap, total)
                            assert total == len(out) and [cs[x] for x in KEYS] == stats + [1], (s, cap, cs, stats)
                            assert raw[:k] == out[:k] and raw[k:] == bytes([CANARY]) * (len(raw) - k), (s, cap)
                        assert dctx.cut_scratch() >= len(joined)   # (the gathered ranges are scratch that grows with the selection)
                        assert dctx.cut_ranges_host(T.blob, [x[:2] for x in blk], ct)[::2] == (len(out), out)
                        ct.close()
                    dctx.set_verify_group(0)
    finally:
        ps.close()
        rx.close()
        dctx.set_verify_group(0)


# ---- 6. one size step: 9 MiB whose first 5 MiB are one line, as one group of 2304 tiles and as nine groups ----
def test_nine_mebibytes(cuda, dctx):
    data = step_file()
    T = Truth("7", data, 1 << 20)
    assert T.plain == data and T.sizes == [1 << 20] * 9 and data.index(b"\n") >= 5 << 20
    dev = Dev(cuda, T)
    for s in (("2", None, False), (None, "1-16", False), ("3-", None, True)):
        spec = spec_of(s, 0x20, 0x0A)
        out, stats = want(data, spec)
        ct = cut_obj(spec)
        try:
            for group, ngroups in ((0, 1), (1 << 20, 9)):
                dctx.set_verify_group(group)
                total, st, got, behind = dev.cut(dctx, ct, len(out) + 5)
                assert total == len(out) and st == stats + [ngroups], (s, group, st, stats)
                assert got == out and behind == bytes([CANARY]) * len(behind), (s, group)
                assert dev.cut(dctx, ct, 0, query=True)[:2] == (len(out), st)
        finally:
            ct.close()
            dctx.set_verify_group(0)
