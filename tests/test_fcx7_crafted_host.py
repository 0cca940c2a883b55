"""The crafted FCX7 corpus (fcx7_corpus.py, built with fcx7_craft.py) on the CPU: the crafter against
the oracle, the host models against the decoder sources, and the whole corpus through the host
decoder fcx_decompress_block (fcx_decode.cpp) and the CLI's host path.  The yardstick is the
oracle's restatement of my_decompress_file_lz77 (my_compress.cpp:2255-2393, pinned in
test_oracle.py); all comparisons are on bytes."""
import ctypes
import os
import struct
import subprocess

import pytest

import fcx7_corpus as cp
import fcx7_craft as craft
import inputs
import my_compress_amd as mc
import oracle

FCX_ERR_FORMAT = -4
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "my_compress_amd", "bin", "my_compress")
NAMES = [v.name for v in cp.corpus()]


def host_block(p: bytes, cap: int = cp.CAP):
    """fcx_decompress_block: (return value, bytes)"""
    out = ctypes.create_string_buffer(cap)
    n = mc.lib().fcx_decompress_block(p, len(p), out, cap)
    return n, out.raw[:max(n, 0)]


# ---- the crafter against the oracle ----
@pytest.mark.parametrize("data", [b"abracadabra abracadabra abracadabra", inputs.generate("text", 3, 5000),
                                  inputs.mosaic(7, 3000)], ids=["abra", "text5000", "mosaic3000"])
def test_payload_of_parse_is_the_encoders_payload(data):
    p = craft.payload(craft.tokens_of(oracle.parse(data)))
    assert p == oracle.compress_block(data)
    assert craft.rebuild(craft.fields(p)) == p
    assert craft.model(craft.tokens_of(oracle.parse(data))) == data


def test_n0_is_the_17_byte_payload():
    assert len(cp.by_name("n0").payload) == 17 and cp.by_name("n0").payload == oracle.compress_block(b"")


@pytest.mark.parametrize("name", NAMES)
def test_verdicts_follow_the_oracle(name):
    """same / stricter: the oracle decodes (to model(tokens) where the vector has tokens);
    format: it fails"""
    v = cp.by_name(name)
    if v.no_oracle:
        assert v.verdict in ("format", "N>2^20")
        return
    w = cp.want(v)
    assert (w is None) == (v.verdict == "format"), f"{name}: oracle {'fails' if w is None else len(w)}"
    if v.tokens is not None:
        assert craft.model(v.tokens, v.pcnt) == w
    if w is not None:
        assert len(w) <= 1 << 20


def test_every_same_vector_has_two_distinct_flag_bytes():
    """(a one-symbol flags stream would decode as zeros: every token a match)"""
    for v in cp.corpus():
        if v.tokens is not None and len(v.tokens) > 8:
            assert len(set(craft.flag_bytes(v.tokens))) >= 2, v.name


# ---- the host models ----
def test_mirrored_constants_match_the_sources():
    names = ["kDMaxRounds", "kDMinSegBits", "kDRetryScale", "kDSymThreads"]
    assert craft.source_constants("fcx_dec_shared.h", names) == {n: getattr(craft, n) for n in names}
    names = ["kDLzThreads", "kDLzTile", "kDLzTPT"]
    assert craft.source_constants("fcx_dec.hip", names) == {n: getattr(craft, n) for n in names}


@pytest.mark.parametrize("name", ["fallback", "retry"])
def test_segment_vectors_settle_as_claimed(name):
    v = cp.by_name(name)
    step, nbits = craft.chain_stepper(v.extra["ts"], v.extra["chars_words"])
    how, rounds = craft.settle_rounds(step, nbits)
    print(f"{name}: {nbits} char bits, S0 {craft.seg_bits(nbits)}, {how} after {rounds} rounds")
    assert craft.seg_bits(nbits) == 256
    assert how == v.extra["claim"]
    assert rounds > craft.kDMaxRounds


def test_steppers_agree_and_short_codes_settle():
    v = cp.by_name("retry")
    fast, nbits = craft.chain_stepper(31, v.extra["chars_words"])
    slow, _ = craft.tree_stepper(craft.chain_tree(31, list(range(32)))[0], v.extra["chars_words"])
    assert all(fast(p) == slow(p) for p in range(0, nbits, 97))
    b8 = cp.by_name("chain_ts10")   # short codes resynchronise: first attempt
    step, nbits = craft.tree_stepper(b8.extra["children"], b8.extra["chars_words"])
    assert craft.settle_rounds(step, nbits)[0] == "first"


def test_lz_step_claims():
    steps = {n: craft.lz_steps(cp.by_name(n).tokens, cp.by_name(n).pcnt) for n in NAMES if cp.by_name(n).tokens}
    for n in (4096, 4097, 9000):   # whole windows of literals: the all-literal step
        assert steps[f"lit{n}_p2047_p1"][0] == ("fast", 4096)
    assert steps["lit4095_p2047_p1"][0][0] == "tile"
    assert steps["stop_at_token_4096"] == [("fast", 4096)]
    assert steps["stop_at_token_0"] == []
    # ~31 tokens per 8192-byte step: the window falls to its floor
    s = steps["p3_l257_x3900"]
    assert len(s) > 100 and all(x[0] == "tile" and x[1] in (31, 32, 34) for x in s[:-1]) and s[1][3] == 256
    # an all-literal step shorter than the history after a tile step: the refill reads both
    s = steps["window_floor_fast"]
    k = next(i for i, x in enumerate(s) if x[0] == "fast")
    assert k > 0 and s[k - 1][0] == "tile" and s[k][1] < 2048 and s[k + 1][0] == "tile", s
    assert steps["tile_then_p2047"][0] == ("tile", 4096, 4196, 4096)
    assert not any(x[0] == "stuck" for s in steps.values() for x in s)


# ---- the whole corpus through the host decoder ----
@pytest.mark.parametrize("name", NAMES)
def test_host_decoder_on_corpus(name):
    v = cp.by_name(name)
    n, got = host_block(v.payload)
    w = cp.want(v)
    print(f"{name}: verdict {v.verdict}, host {v.host}, oracle {'-' if w is None else len(w)}, host decoder {n}")
    if v.host == "same":
        assert w is not None and n == len(w) and got == w
    else:
        assert v.host == "format" and n == FCX_ERR_FORMAT


def test_host_decoder_hostile_headers_return_format():
    """N and G near 2^32 sized buffers (and a memset) before any check; now FCX_ERR_FORMAT"""
    hostile = [v for v in cp.corpus() if v.name.startswith("hostile_")]
    assert len(hostile) == 9
    for v in hostile:
        assert host_block(v.payload, 4096)[0] == FCX_ERR_FORMAT, v.name
    for n in (0xFFFFFFFF, 0xFFFFFFF8, (1 << 20) + 1):   # the 30-byte file of the report: N and little else
        assert host_block(struct.pack("<I", n) + bytes(16), 4096)[0] == FCX_ERR_FORMAT
    # N = 2^20 itself is inside the bound: a header that stops there is merely truncated
    assert host_block(struct.pack("<I", 1 << 20), 4096)[0] == FCX_ERR_FORMAT


def test_host_decoder_capacity():
    v = cp.by_name("good_text")
    w = cp.want(v)
    assert host_block(v.payload, len(w)) == (len(w), w)
    assert host_block(v.payload, len(w) - 1)[0] < 0


# ---- the CLI's host path (no GPU: the CLI decodes with fcx_decompress_block) ----
def _file(records: bytes, nrec: int, total: int) -> bytes:
    return b"FCX7" + struct.pack("<IH", total, nrec) + records


def _no_gpu() -> bool:
    h = ctypes.c_void_p()
    if mc.lib().fcx_dctx_create(ctypes.byref(h), 0) != 0:
        return True
    mc.lib().fcx_dctx_destroy(h)
    return False


def test_cli_hostile_framing_fails_cleanly(tmp_path):
    """a record length past the end of the file, a record count past the records, a length of
    4 GiB - 1: the CLI ends with an error and no signal, with or without a GPU"""
    good = craft.record(cp.by_name("good_text").payload)
    w = cp.want(cp.by_name("good_text"))
    files = {name: _file(recs, n, 2 * len(w)) for name, recs, n in cp.record_vectors()}
    files["record_length_ffffffff"] = _file(good + struct.pack("<I", 0xFFFFFFFF) + good[4:], 2, 2 * len(w))
    if not _no_gpu():   # (the GPU stream path reads an FCX7 file to its end, whatever the header counts)
        del files["nblocks_plus_1"]
    for name, blob in files.items():
        (tmp_path / name).write_bytes(blob)
        r = subprocess.run([CLI, "-i", name, "-o", "out"], cwd=tmp_path, capture_output=True, text=True, timeout=120)
        assert r.returncode != 0 and r.returncode > 0, (name, r.returncode, r.stderr)
    if _no_gpu():
        (tmp_path / "ok").write_bytes(_file(good + good, 2, 2 * len(w)))
        r = subprocess.run([CLI, "-i", "ok", "-o", "out"], cwd=tmp_path, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and (tmp_path / "out").read_bytes() == w + w
