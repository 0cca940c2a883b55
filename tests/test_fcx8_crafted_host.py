"""The crafted FCX8 corpus (fcx8_corpus.py, built with fcx8_craft.py) on the CPU: every declared
verdict against the oracle's restatement of my_decompress_file_lz78 (my_compress.cpp:3478-3710,
pinned in test_lz78.py), the plain model of the tokens as a third opinion, the builder against real
parses, and the STRICTER table against the decoder source.  There is no host FCX8 decoder: the GPU
side is test_gpu_lz78_decode_crafted.py.  All comparisons are on bytes."""
import os
import time

import pytest

import fcx8_corpus as cp
import fcx8_craft as craft
import inputs
import oracle

NAMES = [v.name for v in cp.corpus()]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def source(name="my_compress_amd/csrc/fcx_lz78_dec.hip") -> str:
    with open(os.path.join(ROOT, name)) as f:
        return f.read()


# ---- the builder against the oracle ----
@pytest.mark.parametrize("n", [300, 5000, 70000])
@pytest.mark.parametrize("kind", ["rand", "text", "zeros", "mosaic"])
def test_builder_round_trips_real_parses(kind, n):
    data = {"zeros": lambda: bytes(n), "mosaic": lambda: inputs.mosaic(33, n)}.get(
        kind, lambda: inputs.generate(kind, 7, n))()
    toks = oracle.lz78_parse(data)
    p, q = craft.payload(toks), oracle.lz78_compress_block(data)
    w = oracle.lz78_decompress_block(q, n + 64)
    # (the builder's group tree differs from the encoder's: the decoder does not care)
    assert oracle.lz78_decompress_block(p, n + 64) == w
    assert craft.model(toks) == w
    assert craft.rebuild(craft.fields(p)) == p and craft.rebuild(craft.fields(q)) == q
    assert craft.fields(q)["N"] == len(toks) and craft.fields(p)["gpos"] == craft.fields(q)["gpos"]


def test_model_examples_of_the_format():
    assert craft.model([(0, 65), (1, 66), (2, 67)]) == b"AABABC"          # idx == t: the parent is token t - 1
    assert craft.model([(0, 65), (2, 66), (1, 67)]) is None               # idx > t
    assert craft.model([(0, 0)]) == b"" and craft.model([(0, 97)]) == b""   # tail zero; one-symbol stream
    for d in (64, 65, 128, 129):
        w = cp.oracle_block(craft.payload(cp.chain(d)))
        assert len(w) == d * (d + 1) // 2 and w == craft.model(cp.chain(d))


def test_constants_follow_the_sources():
    K = craft.kernel_constants()
    assert K["kCapBlock"] == (1 << 20) + 8 and K["kGmax"] == 4100   # (what the named vectors chain_1447 / _1448 assume)
    assert K["kMaxDepth"] * (K["kMaxDepth"] + 1) // 2 > K["kCapBlock"] and cp.CAP >= 2 * K["kCapBlock"]


# ---- the verdicts ----
@pytest.mark.parametrize("name", NAMES)
def test_verdicts_follow_the_oracle(name):
    """same / a STRICTER key: the oracle decodes; format: it fails; tokens: the model agrees"""
    v = cp.by_name(name)
    if v.no_oracle:
        assert v.verdict == "format"
        return
    w = cp.want(v)
    assert (w is None) == (v.verdict == "format"), f"{name}: oracle {'fails' if w is None else len(w)}"
    if v.tokens is not None:
        assert craft.model(v.tokens) == w
    if v.verdict == "same":
        assert len(w) <= cp.CAPB


def test_every_stricter_key_is_used_and_its_line_is_in_the_source():
    text = source()
    used = {v.verdict for v in cp.corpus()}
    for key, (kernel, line, why) in cp.STRICTER.items():
        assert key in used, key
        assert line in text and kernel in text and why, key


def test_every_reject_condition_has_its_vectors():
    text = source()
    records = {r[0] for r in cp.record_vectors()}
    for line, names in cp.REJECTS.items():
        assert line in text, line
        for n in names:
            if n.startswith("record:"):
                assert n[7:] in records, n
            else:
                assert cp.by_name(n).verdict != "same", n
    # and no vector is rejected without a place in the table
    listed = {n for names in cp.REJECTS.values() for n in names}
    assert {v.name for v in cp.corpus() if v.verdict != "same"} - listed == {"wcnt_plus1_good"}   # (shifted fields)


def test_vector_claims():
    K = cp.K
    w = {n: cp.want(cp.by_name(n)) for n in ("N_cap", "size_cap", "size_cap_tail0", "size_cap_plus1_tail0", "chain_1447")}
    assert len(w["N_cap"]) == len(w["size_cap"]) == K["kCapBlock"] == len(w["size_cap_plus1_tail0"])
    assert len(w["size_cap_tail0"]) == K["kCapBlock"] - 1 and len(w["chain_1447"]) == 1447 * 1448 // 2
    assert len(cp.want(cp.by_name("chain_1448"))) == 1448 * 1449 // 2 > K["kCapBlock"]
    assert cp.want(cp.by_name("one_token_a")) == b"" and cp.want(cp.by_name("N_0_chars")) == b""
    assert cp.want(cp.by_name("ts_0")) == bytes(12)   # 13 bytes of phrases, all zeros, less the tail zero
    assert cp.want(cp.by_name("W_0")) != cp.want(cp.by_name("good"))
    # the phrase lengths the expansion kernels split at
    toks = cp.by_name("phrase_edges").tokens
    lens = []
    for ix, _ in toks:
        lens.append(1 + (lens[ix - 1] if ix else 0))
    L = K["kLong"]
    assert set(lens) >= {L - 1, L, L + 1, 2 * L - 1, 2 * L, 2 * L + 1, 3 * L + 1} and lens.count(L + 1) >= 3
    f = craft.fields(cp.by_name("pindex_two_pieces").payload)
    assert len(f["bitmap"]) > 16 * 1024 and f["wcnt"] == 8
    for B in (15, 16, 4095, 4096, 4097):
        assert len(craft.fields(cp.by_name(f"wcnt_bit_in_byte_{B}").payload)["bitmap"]) == B + 1


@pytest.mark.parametrize("name", ["groups_fallback", "groups_retry"])
def test_group_streams_settle_as_claimed(name):
    """k78d_groups runs seg_decode (fcx_dec_shared.h) on 32 Wg bits: its settle loop is the one
    fcx7_craft.settle_rounds models, walked with the chain tree's codes"""
    v = cp.by_name(name)
    step, nbits = craft.chain_stepper(v.extra["ts"], v.extra["words"])
    how, rounds = craft.settle_rounds(step, nbits)
    print(f"{name}: {nbits} group bits, S0 {craft.seg_bits(nbits)}, {how} after {rounds} rounds")
    assert how == v.extra["claim"]


def test_hostile_framing_fails_in_the_oracle():
    import struct

    for name, recs, n in cp.record_vectors():
        blob = b"FCX8" + struct.pack("<IH", 0, n) + recs
        with pytest.raises(RuntimeError):
            oracle.lz78_decompress_file(blob, 3 * cp.CAP)


def test_corpus_builds_in_seconds():
    t0 = time.perf_counter()
    cp._corpus()
    dt = time.perf_counter() - t0
    print(f"{len(NAMES)} vectors in {dt:.2f} s")
    assert len(NAMES) >= 75 and dt < 10
