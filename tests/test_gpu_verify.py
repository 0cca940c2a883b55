"""Round-trip verification on the device: fcx_verify_shard (fcx_verify.hip: k_vcompare, k_vsummary), its
host and stream forms and the command line's --verify / --compare, for FCX7 and FCX8.

The records come from the GPU encoders.  Truth is never the code under test: the decoded bytes of a
record are the oracle decoder's (per_record of test_range_cli.py), and the pair (decoded bytes, first
difference) of every record and the six totals follow from those bytes and the original by
want_pairs() here and expect() of test_compare_cli.py."""
import ctypes
import io

import pytest

import inputs
import my_compress_amd as mc
import oracle
from test_cli import run
from test_compare_cli import EXTRA, LINE, SAME, TOTAL, check_compare, expect, first_diff, mixed_data
from test_range_cli import per_record

pytestmark = pytest.mark.gpu

FCX_ERR_ARG, FCX_ERR_FORMAT = -1, -4
CHUNK = 16384   # bytes of a block one k_vcompare workgroup compares (kVChunk)
STATS = ("blocks", "differ", "first", "size_differs", "bytes", "decoded")


def text(seed, n):
    return inputs.generate("text", seed, n)


def rand(seed, n):
    return inputs.generate("rand", seed, n)


def want_pairs(parts, orig: bytes, block: int):
    return [(len(dec), first_diff(dec, orig[k * block:(k + 1) * block])) for k, dec in enumerate(parts)]


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


class Run:
    """a case's records on the device; check() verifies them against an original that sits, like the
    pairs, inside a larger allocation filled with a sentinel"""

    def __init__(self, cuda, case: Case):
        import torch

        self.case, self.cuda = case, cuda
        self.d_rec = torch.frombuffer(bytearray(case.recs or b"\0"), dtype=torch.uint8).to(cuda)
        self.stream = torch.cuda.current_stream().cuda_stream

    def call(self, dctx, orig: bytes, front: int = 37, blocks: bool = True):
        """(stats, pairs or None) of verify_shard; the sentinels around the original and the pairs are checked"""
        import torch

        c, n = self.case, len(orig)
        d_o = torch.full((front + n + 64,), 0xA5, dtype=torch.uint8, device=self.cuda)
        d_o[front:front + n] = torch.frombuffer(bytearray(orig or b"\0"), dtype=torch.uint8)[:n].to(self.cuda)
        before = d_o.clone()
        d_b = torch.full((2 * c.n + 16,), 0x5A5A5A5A, dtype=torch.int32, device=self.cuda)
        st = dctx.verify_shard(self.d_rec.data_ptr(), len(c.recs), c.n, c.kind, d_o.data_ptr() + front, n, c.block,
                               d_b.data_ptr() + 32 if blocks else 0, self.stream)
        assert torch.equal(d_o, before)   # the original is only read
        h = d_b.cpu().numpy().astype("uint32")
        assert (h[:8] == 0x5A5A5A5A).all() and (h[8 + 2 * c.n:] == 0x5A5A5A5A).all()
        if not blocks:
            assert (h == 0x5A5A5A5A).all()
            return st, None
        return st, [(int(h[8 + 2 * k]), int(h[9 + 2 * k])) for k in range(c.n)]

    def check(self, dctx, orig: bytes = None, front: int = 37):
        c = self.case
        orig = c.data if orig is None else orig
        st, pairs = self.call(dctx, orig, front)
        rows, stats, extra = expect(c.parts, orig, c.block)
        assert extra == 0
        assert pairs == want_pairs(c.parts, orig, c.block)
        assert [st[k] for k in STATS] == stats
        return st, pairs


def edited(data: bytes, *at):
    b = bytearray(data)
    for a in at:
        b[a] ^= 0x5A
    return bytes(b)


def tail_zero_text(n: int, block: int) -> bytes:
    """text whose block 0 ends in 0x00: an FCX8 record that decodes one byte short"""
    t = bytearray(text(7, n))
    t[block - 1] = 0
    return bytes(t)


@pytest.mark.parametrize("kind", ["7", "8"])
def test_the_cpu_cases_on_the_device(dctx, cuda, kind):
    mixed = Case(kind, mixed_data(), 4096)
    if kind == "7":
        assert mixed.sizes == [4096, 4096, 0, 0, 0, 4096, 4096, 1808]
    st, _ = Run(cuda, mixed).check(dctx)
    if kind == "7":
        assert (st["differ"], st["first"], st["bytes"]) == (3, 2, 12288)
    st, _ = Run(cuda, Case(kind, text(7, 20000), 4096)).check(dctx)
    assert st["differ"] == 0 and st["first"] is None and st["decoded"] == 20000
    a = Case(kind, b"A" * 5000, 4096)
    st, pairs = Run(cuda, a).check(dctx)
    if kind == "7":
        assert pairs == [(4096, 0), (904, 0)]   # the right length of zeros


def test_fcx8_block_ending_in_zero_is_one_byte_short(dctx, cuda):
    c = Case("8", tail_zero_text(12288, 4096), 4096)
    assert c.sizes == [4095, 4096, 4096]   # every later decoded offset is odd
    r = Run(cuda, c)
    st, pairs = r.check(dctx)
    assert pairs == [(4095, 4095), (4096, SAME), (4096, SAME)] and st["size_differs"] == 1
    for at in (4096, 4096 + 17, 8191, 12287):
        _, pairs = r.check(dctx, edited(c.data, at))
        assert pairs[at // 4096] == (4096, at % 4096)


@pytest.mark.parametrize("block", [8, 9, 16, 64])
def test_the_lossy_edge(dctx, cuda, block):
    c = Case("7", rand(11, 3 * block), block)
    assert c.sizes == ([block] * 3 if block < 16 else [0] * 3)
    st, pairs = Run(cuda, c).check(dctx)
    assert st["differ"] == (0 if block < 16 else 3)


def edit_places(blen: int):
    return sorted({p for p in (0, 15, 16, 63, 64, 1023, 1024, CHUNK - 1, CHUNK, 2 * CHUNK - 1, 2 * CHUNK, blen - 1) if p < blen})


# A random block in front decodes to 0 bytes only when it is all literals and its flag bytes are all 0xFF:
# 16 bytes or more, a multiple of 8, and small enough to hold no match.  That holds at 1000 and not at 1,
# 4097 or 40000 (checked on the oracle), so `lost` runs at 1000 and, in their place, at 4096; `short`
# misaligns the decoded side at every size above 1.
@pytest.mark.parametrize("block,lead", [(b, "none") for b in (1, 1000, 4097, 40000)] + [(1000, "lost"), (4096, "lost")] +
                         [(b, "short") for b in (1000, 4097, 40000)])
def test_alignment_of_both_sides(dctx, cuda, block, lead):
    """one edited byte per call, at the places where the compare changes path; `lost`: a random block that
    decodes to 0 bytes in front, `short`: an FCX8 block that decodes one byte short in front, so the
    decoded side is misaligned against the original"""
    body = text(5, 3 * block + 7)
    if lead == "none":
        c = Case("7", body, block)
        k0 = 0
    elif lead == "lost":
        c = Case("7", rand(3, block) + body, block)
        assert c.sizes[0] == 0 and c.sizes[1] == block
        k0 = 1
    else:
        c = Case("8", tail_zero_text(block, block) + body, block)
        assert c.sizes[0] == block - 1 and c.sizes[1] == block
        k0 = 1
    r = Run(cuda, c)
    r.check(dctx, front=0)
    r.check(dctx, front=64)
    for k in (k0 + 1, c.n - 1):   # a block in the middle, and the last one (7 bytes, or 1)
        blen = min(block, len(c.data) - k * block)
        for p in edit_places(blen):
            at = k * block + p
            _, pairs = r.check(dctx, edited(c.data, at), front=37 if p % 2 else 3)
            if c.parts[k] == c.data[k * block:k * block + blen]:   # (a block that comes back: the edit is the difference)
                assert pairs[k] == (blen, p), (k, p)


def test_the_minimum_wins(dctx, cuda):
    B = 1 << 20
    c = Case("7", rand(21, 3 * B), B)
    assert c.sizes == [B] * 3   # 1 MiB random blocks round-trip
    r = Run(cuda, c)
    st, _ = r.check(dctx)
    assert st["differ"] == 0
    # two workgroups; one wave's span of one step ([4096, 5120) of the block); one lane's 16 bytes
    for a, b in ((700001, 1048575), (4196, 4996), (4196, 4200)):
        st, pairs = r.check(dctx, edited(c.data, B + a, B + b))
        assert pairs == [(B, SAME), (B, a), (B, SAME)]
        assert (st["differ"], st["first"], st["bytes"]) == (1, 1, B)


def test_groups_do_not_change_the_result(dctx, cuda):
    c = Case("7", mixed_data(), 4096)
    r = Run(cuda, c)
    orig = edited(c.data, 6 * 4096 + 4000, 7 * 4096)
    whole = r.check(dctx, orig)
    assert dctx.verify_groups() == 1
    try:
        dctx.set_verify_group(8192)   # records 0-1, 2-5 (the zero-size ones open the group), 6-7
        assert r.check(dctx, orig) == whole
        assert dctx.verify_groups() == 3
        dctx.set_verify_group(1)      # every record a group of its own
        assert r.check(dctx, orig) == whole
        assert dctx.verify_groups() == c.n
        c8 = Case("8", tail_zero_text(12288, 4096), 4096)
        assert Run(cuda, c8).check(dctx, edited(c8.data, 5000)) is not None
        assert dctx.verify_groups() == 3
    finally:
        dctx.set_verify_group(0)


def test_pairs_are_optional(dctx, cuda):
    c = Case("7", mixed_data(), 4096)
    r = Run(cuda, c)
    st, none = r.call(dctx, c.data, blocks=False)
    assert none is None and st == r.check(dctx)[0]


def test_arguments(dctx, cuda):
    import torch

    c = Case("7", text(7, 20000), 4096)
    r = Run(cuda, c)
    d_o = torch.frombuffer(bytearray(c.data), dtype=torch.uint8).to(cuda)
    vals = (ctypes.c_uint64 * 6)()

    def rc(kind=b"7", rec_len=len(c.recs), nblocks=c.n, n=len(c.data), block=4096, ctx=dctx._h, stats=vals):
        return mc.lib().fcx_verify_shard(ctx, kind, ctypes.c_void_p(r.d_rec.data_ptr()), rec_len, nblocks,
                                         ctypes.c_void_p(d_o.data_ptr()), n, block, None, stats, None)

    assert rc() == 0 and list(vals) == [5, 0, 2 ** 64 - 1, 0, 0, 20000]
    assert rc(nblocks=c.n + 1) == FCX_ERR_ARG and rc(nblocks=c.n - 1) == FCX_ERR_ARG
    assert rc(kind=b"9") == FCX_ERR_ARG
    assert rc(block=0) == FCX_ERR_ARG and rc(block=(1 << 20) + 1) == FCX_ERR_ARG
    assert rc(ctx=None) == FCX_ERR_ARG and rc(stats=None) == FCX_ERR_ARG
    assert rc(rec_len=len(c.recs) - 10) == FCX_ERR_FORMAT   # the last record runs past the run
    assert "fcx_verify_shard" not in mc.lib().fcx_last_error().decode()   # (the decoders' own message)
    st = dctx.verify_shard(0, 0, 0, "7", 0, 0, 4096)   # nothing to do: no device memory is touched
    assert st == dict(zip(STATS, [0, 0, None, 0, 0, 0]))


@pytest.mark.parametrize("kind", ["7", "8"])
def test_verify_host(dctx, cuda, kind):
    c = Case(kind, mixed_data(), 4096)
    orig = edited(c.data, 100, 6 * 4096 + 1)
    st, pairs = dctx.verify_host(c.recs, c.n, kind, orig, 4096)
    rows, stats, _ = expect(c.parts, orig, 4096)
    assert pairs == want_pairs(c.parts, orig, 4096) and [st[k] for k in STATS] == stats


@pytest.mark.parametrize("kind", ["7", "8"])
def test_verify_stream_over_two_record_groups(dctx, cuda, kind):
    c = Case(kind, text(13, 300 * 4096), 4096)   # 300 records: the stream path reads them as 256 + 44
    assert c.n == 300

    def check(orig):
        st, bad = dctx.verify_stream(io.BytesIO(c.blob), io.BytesIO(orig), 4096)
        rows, stats, extra = expect(c.parts, orig, 4096)
        want = [(k, blen, dec, fd) for k, dec, blen, fd in rows] + ([(300, extra, 0, 0)] if extra else [])
        assert bad == want and [st[k] for k in STATS] == stats
        return st

    assert check(c.data)["differ"] == 0
    st = check(edited(c.data, 270 * 4096 + 5, 299 * 4096 + 4095))
    if kind == "7":
        assert (st["differ"], st["first"]) == (2, 270)   # numbered over the whole file
    check(c.data + b"x" * 100)          # bytes behind the last record: reported last, as block 300
    check(c.data[:260 * 4096 + 10])     # records the original has no bytes for
    assert mc.verify(c.blob, c.data, 4096)[0]["blocks"] == 300


def cli_lines(out: str):
    return ([tuple(int(x) for x in m) for m in LINE.findall(out)], [int(x) for x in EXTRA.findall(out)], TOTAL.findall(out))


@pytest.mark.parametrize("args,lz78", [(["-c", "lz77"], False), (["-c", "lz78"], True)])
def test_cli_verify_after_compress(tmp_path, cuda, args, lz78):
    data = mixed_data()
    (tmp_path / "plain").write_bytes(data)
    r = run(["-i", "plain", "-o", "comp", "-b", "4096", "--verify"] + args, tmp_path)
    blob = (tmp_path / "comp").read_bytes()
    assert blob == (oracle.lz78_compress_file(data, 4096) if lz78 else oracle.compress_file(data, 4096))
    _, parts = per_record(blob, lz78)
    rows, stats, _ = expect(parts, data, 4096)
    assert cli_lines(r.stdout) == (rows, [], [(str(stats[1]), "8", str(stats[4]), "FAIL" if rows else "OK")]), r.stdout + r.stderr
    assert r.returncode == (1 if rows else 0)
    assert r.stdout.index("<Final>:") < r.stdout.index("verify:")   # the compress printout comes first, as ever
    if not lz78:
        assert rows == [(2, 0, 4096, 0), (3, 0, 4096, 0), (4, 0, 4096, 0)]
        assert "verify: 3 of 8 blocks differ, 12288 input bytes in them [FAIL]" in r.stdout.splitlines()
    t = text(7, 20000)
    (tmp_path / "plain").write_bytes(t)
    r = run(["-i", "plain", "-o", "comp", "-b", "4096", "--verify"] + args, tmp_path)
    assert r.returncode == 0 and "verify: 0 of 5 blocks differ, 0 input bytes in them [OK]" in r.stdout.splitlines(), r.stdout + r.stderr


def test_cli_compare_on_the_device(tmp_path, cuda):
    data = mixed_data()
    rows, stats = check_compare(tmp_path, mc.compress(data, 4096), data, 4096)
    assert rows == [(2, 0, 4096, 0), (3, 0, 4096, 0), (4, 0, 4096, 0)] and stats[4] == 12288
    check_compare(tmp_path, mc.compress_lz78(data, 4096), edited(data, 9000), 4096, lz78=True)
