"""The crafted FCX8 corpus (fcx8_corpus.py) through the GPU decoder (fcx_lz78_dec.hip): every vector
alone through fcx_lz78_decompress_shard against its verdict, the `same` set in one call with its
payloads at every alignment, the capacity edge, which record a failed call names, and the host,
stream and block entries.  The yardstick is the oracle's restatement of my_decompress_file_lz78
(my_compress.cpp:3478-3710); all comparisons are on bytes, bit-exact.

The segment decoder's counters are not asserted here: fcx_dctx_symbol_stats reports the FCX7
decoder's status words, the FCX8 decoder keeps its own (kW8Stats) and has no accessor, so the
groups_fallback / groups_retry vectors are checked on bytes; that their streams take those paths
is computed on the CPU (test_fcx8_crafted_host.py::test_group_streams_settle_as_claimed)."""
import ctypes
import io
import random
import struct

import pytest

import fcx8_corpus as cp
import fcx8_craft as craft
import my_compress_amd as mc

pytestmark = pytest.mark.gpu

FCX_ERR_CAPACITY, FCX_ERR_FORMAT = -2, -4
NAMES = [v.name for v in cp.corpus()]
SAME = [v for v in cp.corpus() if v.verdict == "same"]


@pytest.fixture(scope="module")
def dctx(cuda):
    d = mc.DContext(0)
    yield d
    d.close()


def shard_rc(dctx, cuda, recs: bytes, nrec: int, cap: int):
    """fcx_lz78_decompress_shard on device-resident records, the output buffer zero-filled and
    cap + 64 bytes long: (return code, decoded bytes, whether every byte past them is still zero)"""
    import torch

    d_in = torch.frombuffer(bytearray(recs or b"\0"), dtype=torch.uint8).to(cuda)
    d_out = torch.zeros(cap + 64, dtype=torch.uint8, device=cuda)
    got = ctypes.c_uint64(0)
    rc = mc.lib().fcx_lz78_decompress_shard(dctx._h, ctypes.c_void_p(d_in.data_ptr()), len(recs), nrec,
                                            ctypes.c_void_p(d_out.data_ptr()), cap, ctypes.byref(got),
                                            ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    clean = not bool(d_out[got.value:].any().item())
    return rc, d_out[:got.value].cpu().numpy().tobytes(), clean


def last_error() -> bytes:
    return mc.lib().fcx_last_error()


def check_good_record(dctx, cuda):
    v = cp.by_name("G_2")
    assert shard_rc(dctx, cuda, craft.record(v.payload), 1, cp.CAP) == (0, cp.want(v), True)


# ---- 1. every vector alone ----
@pytest.mark.parametrize("name", NAMES)
def test_vector_alone(name, dctx, cuda):
    v = cp.by_name(name)
    w = cp.want(v)
    rc, got, clean = shard_rc(dctx, cuda, craft.record(v.payload), 1, cp.CAP)
    print(f"{name}: verdict {v.verdict}, oracle {'-' if w is None else len(w)}, GPU rc {rc}, {len(got)} B")
    if v.verdict == "same":
        assert rc == 0 and len(got) == len(w) and got == w
        assert clean   # nothing written past the block (the dropped tail zero included)
    else:   # format, or one of the STRICTER conditions
        assert rc == FCX_ERR_FORMAT
        assert b"malformed record 1" in last_error()
        check_good_record(dctx, cuda)   # the same context still decodes


@pytest.mark.parametrize("name,recs,nrec", cp.record_vectors(), ids=[r[0] for r in cp.record_vectors()])
def test_hostile_framing(name, recs, nrec, dctx, cuda):
    rc, _, _ = shard_rc(dctx, cuda, recs, nrec, 3 * cp.CAP)
    assert rc == FCX_ERR_FORMAT
    bad = {"nblocks_plus_1": 3}.get(name, 2)
    assert b"malformed record %d" % bad in last_error()
    check_good_record(dctx, cuda)


# ---- 2. the `same` set in one call ----
def same_shard():
    """every `same` vector as a record, shuffled; the small ones (<= 4 KiB decoded) repeated until
    the shard has more than 3 kBatch records: (records, count, expected bytes, payload offsets mod 4)"""
    batch = cp.K["kBatch"]
    small = [v for v in SAME if len(cp.want(v)) <= 4096 and len(v.payload) <= 8192]
    order = list(SAME) + small * ((3 * batch + 40 - len(SAME)) // len(small) + 1)
    random.Random(8).shuffle(order)
    recs, want, offs = bytearray(), bytearray(), set()
    for v in order:
        offs.add((len(recs) + 4) % 4)
        recs += craft.record(v.payload)
        want += cp.want(v)
    return bytes(recs), len(order), bytes(want), offs


def test_same_vectors_in_one_call(dctx, cuda):
    recs, n, want, offs = same_shard()
    assert offs == {0, 1, 2, 3} and n > 3 * cp.K["kBatch"] and len(want) < 8 << 20
    rc, got, clean = shard_rc(dctx, cuda, recs, n, len(want) + 64)
    assert rc == 0 and len(got) == len(want)
    assert got == want and clean


def test_capacity_exact_and_one_short(dctx, cuda):
    recs, n, want, _ = same_shard()
    assert any(v.name.endswith("tail0") for v in SAME)   # (some records lose their tail zero)
    rc, got, clean = shard_rc(dctx, cuda, recs, n, len(want))
    assert rc == 0 and got == want and clean
    assert shard_rc(dctx, cuda, recs, n, len(want) - 1)[0] == FCX_ERR_CAPACITY
    check_good_record(dctx, cuda)


# ---- 3. which record a failed call names ----
# fcx.h: the first record that fails the earliest stage that fails.  The framing of the whole run
# comes first; then, batch after batch, the headers, the trees (group and char), the links and sizes.
# A later stage is not run once an earlier one failed, so within one batch a bad header at record 10
# is named before a bad link at record 6.
def named(dctx, cuda, bad: dict, tail: bytes = b""):
    """decode 3 kBatch + 5 good records with the 0-based places of `bad` replaced by those vectors;
    the 1-based record the call names"""
    good = craft.record(cp.by_name("two_tokens").payload)
    n = 3 * cp.K["kBatch"] + 5
    recs = [good] * n
    for i, name in bad.items():
        recs[i] = craft.record(cp.by_name(name).payload)
    rc, _, _ = shard_rc(dctx, cuda, b"".join(recs) + tail, n + (1 if tail else 0), cp.CAP + 4 * n)
    assert rc == FCX_ERR_FORMAT
    msg = last_error()
    assert b"malformed record " in msg
    return int(msg.split(b"malformed record ")[1].split()[0])


@pytest.mark.parametrize("kind", ["wcnt_0", "tree_orphan", "char_two_parents", "ix_eq_t_plus1", "chain_1448"])
def test_one_bad_record_is_named_in_every_batch(kind, dctx, cuda):
    B = cp.K["kBatch"]
    for i in (7, B + 9, 2 * B + 100, 3 * B + 4):
        assert named(dctx, cuda, {i: kind}) == i + 1
    check_good_record(dctx, cuda)


def test_bad_char_tree_is_named_through_its_stream(dctx, cuda):
    """the char trees report their stream's place in the batch (kW8BadStream): batch0 + q + 1"""
    B = cp.K["kBatch"]
    assert named(dctx, cuda, {B + 44: "char_child_below_base"}) == B + 45
    assert named(dctx, cuda, {B + 44: "char_two_parents", B + 45: "char_child_below_base"}) == B + 45


def test_two_bad_records(dctx, cuda):
    B = cp.K["kBatch"]
    # the same stage: the first one
    assert named(dctx, cuda, {5: "r_eq_wcnt", 9: "ix_eq_t_plus1"}) == 6
    assert named(dctx, cuda, {5: "wcnt_0", 9: "N_past_record"}) == 6
    assert named(dctx, cuda, {5: "char_two_parents", 9: "tree_orphan"}) == 6
    assert named(dctx, cuda, {5: "tree_two_parents", 9: "char_child_below_base"}) == 6
    # different stages, the earlier stage first in the run: the first one
    assert named(dctx, cuda, {5: "wcnt_0", 9: "ix_eq_t_plus1"}) == 6
    # different stages of one batch, the later stage first in the run: the earlier stage's record
    assert named(dctx, cuda, {5: "ix_eq_t_plus1", 9: "wcnt_0"}) == 10
    assert named(dctx, cuda, {5: "chain_1448", 9: "tree_root_child"}) == 10
    # different batches: the first one, whatever the stages
    assert named(dctx, cuda, {5: "ix_eq_t_plus1", B + 9: "wcnt_0"}) == 6
    # a record length past the input is found before any header is read
    n = 3 * B + 5
    assert named(dctx, cuda, {3: "wcnt_0"}, tail=struct.pack("<I", 9) + b"\1\0\0\0") == n + 1
    check_good_record(dctx, cuda)


# ---- 4. the other entries ----
class ShortReads(io.BytesIO):
    """a source that hands out at most 7001 bytes per read"""

    def readinto(self, b):
        return super().readinto(memoryview(b)[:7001])


def test_same_vectors_through_host_and_stream_entries(dctx, cuda):
    recs, n, want, _ = same_shard()
    blob = b"FCX8" + struct.pack("<IH", len(want), n) + recs
    assert mc.decompress_lz78(blob, len(want) + 64) == want          # fcx_lz78_decompress_host
    assert dctx.decompress_host(blob, len(want) + 64) == want
    sink = io.BytesIO()
    total, got, nrec = dctx.decompress_stream(ShortReads(blob), sink)
    assert (total, got, nrec) == (len(want), len(want), n)
    assert sink.getvalue() == want


@pytest.mark.parametrize("name", ["N_cap", "N_0_chars", "one_token_00", "phrase_edges", "size_cap_tail0", "good"])
def test_block_entry(name, cuda):
    v = cp.by_name(name)
    assert mc.my_decompress_file_lz78(v.payload, cp.CAP) == cp.want(v)
