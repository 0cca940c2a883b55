"""The crafted FCX7 corpus (fcx7_corpus.py) through the GPU decoder (fcx_dec.hip): every vector
alone through fcx_decompress_shard against its verdict, the `same` set in one call at every payload
alignment, the segment decoder's counters on the two streams built to reach its second attempt and
its serial fallback, the host and stream entries, and the same table / symbol kernels reached from
the FCX8 decoder.  The yardstick is the oracle's restatement of my_decompress_file_lz77
(my_compress.cpp:2255-2393); all comparisons are on bytes, bit-exact."""
import ctypes
import io
import random
import struct

import pytest

import fcx7_corpus as cp
import fcx7_craft as craft
import inputs
import my_compress_amd as mc
import oracle

pytestmark = pytest.mark.gpu

FCX_ERR_FORMAT = -4
NAMES = [v.name for v in cp.corpus()]
SAME = [v for v in cp.corpus() if v.verdict == "same"]


@pytest.fixture(scope="module")
def dctx(cuda):
    d = mc.DContext(0)
    yield d
    d.close()


def shard_rc(dctx, cuda, recs: bytes, nrec: int, cap: int):
    """fcx_decompress_shard on device-resident records: (return code, decoded bytes)"""
    import torch

    d_in = torch.frombuffer(bytearray(recs or b"\0"), dtype=torch.uint8).to(cuda)
    d_out = torch.zeros(cap + 64, dtype=torch.uint8, device=cuda)
    got = ctypes.c_uint64(0)
    rc = mc.lib().fcx_decompress_shard(dctx._h, ctypes.c_void_p(d_in.data_ptr()), len(recs), nrec,
                                       ctypes.c_void_p(d_out.data_ptr()), cap, ctypes.byref(got),
                                       ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    return rc, d_out[:got.value].cpu().numpy().tobytes()


def check_good_record(dctx, cuda):
    v = cp.by_name("good_text")
    assert shard_rc(dctx, cuda, craft.record(v.payload), 1, cp.CAP) == (0, cp.want(v))


# ---- 1. every vector alone ----
@pytest.mark.parametrize("name", NAMES)
def test_vector_alone(name, dctx, cuda):
    v = cp.by_name(name)
    w = cp.want(v)
    rc, got = shard_rc(dctx, cuda, craft.record(v.payload), 1, cp.CAP)
    print(f"{name}: verdict {v.verdict}, oracle {'-' if w is None else len(w)}, GPU rc {rc}, {len(got)} B")
    if v.verdict == "same":
        assert rc == 0 and len(got) == len(w) and got == w
        # the settle loop ran as its host model says (rounds summed over the Huffman sub-streams)
        st = dctx.symbol_stats()
        fast = chain_step(v) if v.extra and "ts" in v.extra else None
        assert (st["rounds"], st["fallbacks"]) == craft.model_stats(v.payload, fast), st
    else:   # format, or one of the STRICTER conditions
        assert rc == FCX_ERR_FORMAT
        check_good_record(dctx, cuda)   # the same context still decodes


@pytest.mark.parametrize("name,recs,nrec", cp.record_vectors(), ids=[r[0] for r in cp.record_vectors()])
def test_hostile_framing(name, recs, nrec, dctx, cuda):
    assert shard_rc(dctx, cuda, recs, nrec, 2 * cp.CAP)[0] == FCX_ERR_FORMAT
    assert dctx.symbol_stats() == dict.fromkeys(mc.DContext.SYMBOL_STATS, 0)   # failed in the header pass
    check_good_record(dctx, cuda)


# ---- 2. the `same` set in one call ----
def same_shard(insert=None):
    """the `same` vectors as records, each after a pad record (the one-token payload n1 plus unused
    bytes, which decodes to one zero byte) sized so that payload i starts at offset i mod 16;
    (records, count, expected bytes, the payload offsets mod 16 seen)"""
    pad = cp.by_name("n1").payload
    assert cp.want(cp.by_name("n1")) == b"\0"
    recs, want, offs, n = bytearray(), bytearray(), set(), 0
    for i, v in enumerate(SAME):
        if insert is not None and i == len(SAME) // 2:
            recs += craft.record(insert.payload)
            n += 1
        k = (i % 16 - (len(recs) + 4 + len(pad) + 4)) % 16
        recs += craft.record(pad + bytes(k))
        want += b"\0"
        assert (len(recs) + 4) % 16 == i % 16
        offs.add((len(recs) + 4) % 16)
        recs += craft.record(v.payload)
        want += cp.want(v)
        n += 2
    return bytes(recs), n, bytes(want), offs


def test_same_vectors_in_one_call(dctx, cuda):
    recs, n, want, offs = same_shard()
    assert offs == set(range(16)) and n > 80
    rc, got = shard_rc(dctx, cuda, recs, n, len(want) + 64)
    assert rc == 0 and len(got) == len(want)
    assert got == want


@pytest.mark.parametrize("bad", ["p_past_start", "chain_ts33", "hostile_N_ffffffff"])
def test_one_bad_record_fails_the_call(bad, dctx, cuda):
    recs, n, want, _ = same_shard(insert=cp.by_name(bad))
    assert shard_rc(dctx, cuda, recs, n, len(want) + cp.CAP)[0] == FCX_ERR_FORMAT
    check_good_record(dctx, cuda)


# ---- 3. the segment decoder's counters: proof of the second attempt and of the serial fallback ----
def chain_step(v):
    return craft.chain_stepper(v.extra["ts"], v.extra["chars_words"])


def test_fallback_vector_takes_the_serial_fallback(dctx, cuda):
    v = cp.by_name("fallback")
    rc, got = shard_rc(dctx, cuda, craft.record(v.payload), 1, cp.CAP)
    st = dctx.symbol_stats()
    print(st)
    assert rc == 0 and got == cp.want(v)
    assert st["fallbacks"] >= 1 and st["fallbacks_chars"] >= 1
    # the host model of the settle loop: both attempts of the chars stream run out of rounds
    assert (st["rounds"], st["fallbacks"]) == craft.model_stats(v.payload, chain_step(v))
    assert st["fallbacks"] == st["fallbacks_flags"] + st["fallbacks_chars"] + st["fallbacks_p"] + st["fallbacks_golomb_bytes"]


def test_retry_vector_settles_in_the_second_attempt(dctx, cuda):
    v = cp.by_name("retry")
    rc, got = shard_rc(dctx, cuda, craft.record(v.payload), 1, cp.CAP)
    st = dctx.symbol_stats()
    print(st)
    assert rc == 0 and got == cp.want(v)
    assert st["fallbacks"] == 0 and st["golomb_fallbacks"] == 0
    assert st["rounds"] > craft.kDMaxRounds
    assert (st["rounds"], st["fallbacks"]) == craft.model_stats(v.payload, chain_step(v))


def test_text_block_needs_no_fallback(dctx, cuda):
    data = inputs.generate("text", 17, 1 << 20)
    p = oracle.compress_block(data)
    rc, got = shard_rc(dctx, cuda, craft.record(p), 1, cp.CAP)
    st = dctx.symbol_stats()
    print(st)
    assert rc == 0 and got == oracle.decompress_block(p, cp.CAP)
    assert st["fallbacks"] == 0 and st["golomb_fallbacks"] == 0
    assert st["rounds"] > 0 and st["golomb_rounds"] > 0


# ---- 4. the host and stream entries ----
class ShortReads(io.BytesIO):
    """a source that hands out at most 7001 bytes per read"""

    def readinto(self, b):
        return super().readinto(memoryview(b)[:7001])


def test_same_vectors_through_host_and_stream_entries(dctx, cuda):
    recs, n, want, _ = same_shard()
    blob = b"FCX7" + struct.pack("<IH", len(want), n) + recs
    assert dctx.decompress_host(blob, len(want) + 64) == want
    sink = io.BytesIO()
    total, got, nrec = dctx.decompress_stream(ShortReads(blob), sink)
    assert (total, got, nrec) == (len(want), len(want), n)
    assert sink.getvalue() == want


# ---- 5. k_dtable / k_dsyms reached from the FCX8 decoder: 31-bit char codes ----
def test_fcx8_chars_with_a_chain_tree(dctx, cuda):
    import torch
    from test_gpu_lz78_decode import parse

    rng = random.Random(5)
    data = bytes(rng.choice(b"abcdefghijklmnopqrstuvwxyz ,.") for _ in range(20000))
    p = oracle.lz78_compress_block(data)
    f = parse(p)
    chars = bytes(c for _, c in oracle.lz78_parse(data))
    off = f["cbm"] - 1
    assert p[off:] == oracle.huffman_stream(chars)   # the char sub-stream is the payload's tail
    used = sorted(set(chars))
    assert len(used) <= 32
    # (the block's own bytes last: they get the codes of 3 to 31 bits)
    syms = [b for b in range(255, 0, -1) if b not in used][:32 - len(used)] + used
    children, codes = craft.chain_tree(31, syms)
    q = p[:off] + craft.huff_stream(children, codes, chars)
    cap = len(data) + 64
    want = oracle.lz78_decompress_block(q, cap)
    assert want == oracle.lz78_decompress_block(p, cap)   # the same tokens, coded another way
    d_in = torch.frombuffer(bytearray(craft.record(q)), dtype=torch.uint8).to(cuda)
    d_out = torch.zeros(cap + 64, dtype=torch.uint8, device=cuda)
    got = dctx.decompress_lz78_shard(d_in.data_ptr(), len(q) + 4, 1, d_out.data_ptr(), cap,
                                     torch.cuda.current_stream().cuda_stream)
    assert d_out[:got].cpu().numpy().tobytes() == want
