"""The token-parallel FCX8 decoder (fcx_lz78_dec.hip) through the device API, the stream path, the
CLI and the host entry points.  The yardstick is the oracle's decoder (oracle.lz78_decompress_block
/ lz78_decompress_file, pinned against the reference compiled in place by tests/test_lz78.py) and
tests/golden/golden_lz78.json: never the encoder's input alone, the format drops a block's tail
zero and decodes a one-symbol char stream as zeros.  Reference: my_decompress_file_lz78
my_compress.cpp:3478-3710."""
import ctypes
import hashlib
import io
import json
import os
import struct
import subprocess

import pytest

import inputs
import my_compress_amd as mc
import oracle
from fcx8_craft import parse   # noqa: F401  (the payload layout; test_gpu_decode_crafted.py imports it from here)

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CLI = os.path.join(ROOT, "my_compress_amd", "bin", "my_compress")
STAGES = ["header", "index", "tables", "symbols", "links", "expand"]
FCX_ERR_CAPACITY, FCX_ERR_FORMAT = -2, -4


@pytest.fixture(scope="module")
def dctx(cuda):
    d = mc.DContext(0)
    d.set_profiling(True)
    yield d
    d.close()


def records(blob: bytes):
    """(records without the file header, their count)"""
    return blob[10:], struct.unpack_from("<H", blob, 8)[0]


def shard_rc(dctx, cuda, recs: bytes, nrec: int, cap: int):
    """fcx_lz78_decompress_shard on device-resident records: (return code, decoded bytes)"""
    import torch

    d_in = torch.frombuffer(bytearray(recs or b"\0"), dtype=torch.uint8).to(cuda)
    d_out = torch.zeros(cap + 64, dtype=torch.uint8, device=cuda)
    got = ctypes.c_uint64(0)
    rc = mc.lib().fcx_lz78_decompress_shard(dctx._h, ctypes.c_void_p(d_in.data_ptr()), len(recs), nrec,
                                            ctypes.c_void_p(d_out.data_ptr()), cap, ctypes.byref(got),
                                            ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    return rc, d_out[:got.value].cpu().numpy().tobytes()


def shard(dctx, cuda, recs: bytes, nrec: int, cap: int) -> bytes:
    import torch

    d_in = torch.frombuffer(bytearray(recs or b"\0"), dtype=torch.uint8).to(cuda)
    d_out = torch.zeros(cap + 64, dtype=torch.uint8, device=cuda)
    got = dctx.decompress_lz78_shard(d_in.data_ptr(), len(recs), nrec, d_out.data_ptr(), cap,
                                     torch.cuda.current_stream().cuda_stream)
    return d_out[:got].cpu().numpy().tobytes()


def check_stages(dctx):
    st = dctx.stage_times()
    assert [n for n, _ in st] == STAGES, st
    assert all(ms >= 0 for _, ms in st), st


# ---- 1. golden cases through the device API ----
def test_golden_cases_device_api(dctx, cuda):
    with open(os.path.join(HERE, "golden", "golden_lz78.json")) as f:
        g = json.load(f)
    bad = []
    for case in g["cases"]:
        if case["in_bytes"] > 1 << 20:
            continue
        recs, n = records(oracle.lz78_compress_file(inputs.make(case), case["block"]))
        out = shard(dctx, cuda, recs, n, case["in_bytes"] + 64)
        if len(out) != case["dec_bytes"] or hashlib.sha256(out).hexdigest() != case["dec_sha256"]:
            bad.append(case["name"])
    assert not bad, f"fcx_lz78_decompress_shard differs from the reference decoder on {bad}"


# ---- 2. shapes where each stage can go wrong ----
SHAPES = {
    "one_byte": (lambda: b"a", 1 << 20),                                    # N = 1
    "aaaa": (lambda: b"aaaa", 1 << 20),                                     # ts == 0
    "zeros3": (lambda: b"\0\0\0", 1 << 20),                                 # ts == 0 and the tail-zero rule
    "bytes256": (lambda: bytes(range(256)), 1 << 20),                       # 256 root phrases: wcnt = 1, one group
    "mosaic300": (lambda: inputs.mosaic(5, 300), 1 << 20),
    "two_groups": (lambda: inputs.mosaic(33, 5000), 1 << 20),               # 256 < wcnt <= 512: G = 2, 1-bit codes
    "zeros100k": (lambda: bytes(100000), 1 << 20),                          # deep parent chain, long phrases
    "abab": (lambda: b"ab" * 50000, 1 << 20),
    "rand_1m": (lambda: inputs.generate("rand", 3, 1 << 20), 1 << 20),      # > 1000 groups, 8-bit char codes
    "text_1m": (lambda: inputs.generate("text", 4, 1 << 20), 1 << 20),
    "text_65536": (lambda: inputs.generate("text", 5, 65536), 1 << 20),     # segment counts around 2^k
    "text_65537": (lambda: inputs.generate("text", 6, 65537), 1 << 20),
    "ragged_64k": (lambda: inputs.mosaic(9, (2 << 20) + 999), 1 << 16),     # payloads at every alignment
    "block_1": (lambda: inputs.mosaic(11, 5000), 1),                        # thousands of 1..3-token records
    "block_7": (lambda: inputs.mosaic(12, 5000), 7),
}


@pytest.mark.parametrize("name", list(SHAPES))
def test_shapes_vs_oracle(name, dctx, cuda):
    make, block = SHAPES[name]
    data = make()
    blob = oracle.lz78_compress_file(data, block)
    cap = len(data) + 64
    want = oracle.lz78_decompress_file(blob, cap)
    recs, n = records(blob)
    assert n == (len(data) + block - 1) // block
    if name in ("bytes256", "mosaic300", "two_groups"):   # the group stream appears past 256 used indices
        assert parse(recs[4:])["G"] == (2 if name == "two_groups" else 1)
    got = shard(dctx, cuda, recs, n, cap)
    assert len(got) == len(want) and got == want
    check_stages(dctx)   # (the decoder has one path: no serial fallback to count)


# ---- 3. a run that spans scratch batches ----
def test_run_spans_three_batches(dctx, cuda):
    batch = mc.lz78_decode_batch_records()
    nrec = 3 * batch + 5
    data = inputs.mosaic(21, nrec * 4096 - 123)
    blob = oracle.lz78_compress_file(data, 4096)
    recs, n = records(blob)
    assert n == nrec and (n + batch - 1) // batch >= 3
    cap = len(data) + 64
    assert shard(dctx, cuda, recs, n, cap) == oracle.lz78_decompress_file(blob, cap)
    check_stages(dctx)


def patch_u32(p: bytes, off: int, v: int) -> bytes:
    return p[:off] + struct.pack("<I", v) + p[off + 4:]


def one_record(p: bytes) -> bytes:
    return struct.pack("<I", len(p)) + p


def oracle_block(p: bytes, cap: int):
    try:
        return oracle.lz78_decompress_block(p, cap)
    except RuntimeError:
        return None


@pytest.fixture(scope="module")
def payload():
    p = oracle.lz78_compress_block(inputs.mosaic(32, 5000))
    f = parse(p)
    assert f["G"] > 1 and f["ts"] >= 3 and f["nw"] >= 2 and f["W"] >= 2
    return p, f


# ---- 4. exhausted streams: symbols a stream runs out of are 0 ----
@pytest.mark.parametrize("field", ["nw", "W"])
def test_exhausted_stream_matches_oracle(field, payload, dctx, cuda):
    p, f = payload
    off = f["nw_off"] if field == "nw" else f["W_off"]
    q = patch_u32(p, off, f[field] // 2)   # the bytes stay where they are: the bounds still hold
    cap = 5000 + 64
    want = oracle_block(q, cap)   # (bytes or failure: either way the oracle's verdict is the yardstick)
    rc, got = shard_rc(dctx, cuda, one_record(q), 1, cap)
    print(f"{field} halved: oracle {'fails' if want is None else len(want)}, GPU rc {rc}, {len(got)} B")
    if want is None:
        assert rc == FCX_ERR_FORMAT
    else:
        assert rc == 0 and got == want
    if field == "nw":   # the char stream ran out half way: the chars after that are zeros
        assert want is not None and want != oracle.lz78_decompress_block(p, cap)


# ---- 5. malformed records ----
def bad_payloads(p: bytes, f: dict) -> dict:
    G = f["G"]
    internal = [x for x in range(2 * f["ts"]) if (p[f["cbm"] + (x >> 3)] >> (x & 7)) & 1]
    assert len(internal) >= 2
    two = bytearray(p)
    two[f["cpairs"] + internal[1]] = p[f["cpairs"] + internal[0]]   # one node, two parents (and an orphan)
    return {
        "wcnt0": b"\0\0\0\0" + p[4:],
        "half": p[:len(p) // 2],
        "group_self": patch_u32(p, f["tree"], G + 0),   # node 0's left child is node 0
        "char_two_parents": bytes(two),
    }


@pytest.mark.parametrize("kind", ["wcnt0", "half", "group_self", "char_two_parents"])
def test_malformed_record_raises_and_context_survives(kind, payload, dctx, cuda):
    p, f = payload
    bad = bad_payloads(p, f)[kind]
    with pytest.raises(mc.FcxError):
        shard(dctx, cuda, one_record(bad), 1, 8192)
    assert b"malformed record 1" in mc.lib().fcx_last_error()
    assert shard(dctx, cuda, one_record(p), 1, 8192) == oracle.lz78_decompress_block(p, 8192)


def test_bad_record_is_named(payload, dctx, cuda):
    p, f = payload
    good = one_record(p)
    recs = good + good + one_record(bad_payloads(p, f)["half"]) + good
    rc, _ = shard_rc(dctx, cuda, recs, 4, 4 * 8192)
    assert rc == FCX_ERR_FORMAT
    assert b"malformed record 3" in mc.lib().fcx_last_error()


def test_capacity_one_byte_short(payload, dctx, cuda):
    p, _ = payload
    want = oracle.lz78_decompress_block(p, 8192)
    recs = one_record(p) * 2
    assert shard_rc(dctx, cuda, recs, 2, 2 * len(want)) == (0, want + want)
    rc, _ = shard_rc(dctx, cuda, recs, 2, 2 * len(want) - 1)
    assert rc == FCX_ERR_CAPACITY


# ---- 6. stream and CLI ----
class ShortReads(io.BytesIO):
    """a source that hands out at most 70001 bytes per read"""

    def readinto(self, b):
        return super().readinto(memoryview(b)[:70001])


def test_stream_fcx8(dctx, cuda):
    data = inputs.mosaic(41, (3 << 20) + 17)
    blob = oracle.lz78_compress_file(data, 1 << 16)
    sink = io.BytesIO()
    total, got, recs = dctx.decompress_stream(ShortReads(blob), sink)
    want = oracle.lz78_decompress_file(blob, len(data) + 64)
    assert (total, got, recs) == (len(data), len(want), (len(data) + 65535) // 65536)
    assert sink.getvalue() == want


def test_cli_decompresses_fcx8_through_the_stream(cuda, tmp_path):
    data = inputs.mosaic(43, (1 << 20) + 4321)
    (tmp_path / "plain").write_bytes(data)
    r = subprocess.run([CLI, "-i", "plain", "-o", "c8", "-c", "lz78", "-b", "65536"], cwd=tmp_path,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    blob = (tmp_path / "c8").read_bytes()
    r = subprocess.run([CLI, "-i", "c8", "-o", "back"], cwd=tmp_path, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    want = oracle.lz78_decompress_file(blob, len(data) + 64)
    assert (tmp_path / "back").read_bytes() == want
    assert ("SUCCESS" in r.stdout) == (len(want) == len(data)), r.stdout
    assert len(want) == len(data)   # (no block of this input ends in 0x00: the size line reads SUCCESS)


# ---- 7. host entry points ----
@pytest.mark.parametrize("kind,seed", [("rand", 7), ("text", 8)])
def test_host_entry_points_agree(kind, seed, dctx, cuda):
    data = inputs.generate(kind, seed, (1 << 20) + 777)
    blob = oracle.lz78_compress_file(data, 1 << 20)
    want = oracle.lz78_decompress_file(blob, len(data) + 64)
    assert mc.decompress_lz78(blob) == want
    assert dctx.decompress_host(blob, len(data) + 64) == want
