"""The entropy stage (fcx_entropy.hip: k_tree, k_encode, k_headers) at the places where a stream
decides something, against the oracle: the crafted inputs of tests/entropy_craft.py (pinned on the
CPU by tests/test_entropy_craft.py: merge form, rounds, byte substitution or general coder, chunk
count, staging windows, the window seam, tail symbol counts, deepest code, stream lengths) through
Context.compress_shard, routed and with the general match unit forced (mode 3): the entropy stage
must not depend on who produced the streams.  Bar: the bytes equal oracle.compress_file's with the
exhaustive finder, at the block size a vector names and at 12293 (ragged tiles and chunks); then
the host decoder and the GPU decoder give back what the reference's decoder gives for those bytes,
which is the input except for the reference's one-symbol quirk (entropy_craft.one_symbol_flags).
Every input is a legal block; nothing here is built to fail."""
import pytest

import entropy_craft as craft
import my_compress_amd as mc
import oracle

pytestmark = pytest.mark.gpu

MODES = (3,)
_WANT = {}


def want_of(data: bytes, block: int):
    """(the oracle's file, what its decoder makes of it or None where it refuses), computed once"""
    key = (hash(data), len(data), block)
    if key not in _WANT:
        blob = oracle.compress_file(data, block)
        try:
            dec = oracle.decompress_file(blob, len(data) + 16)
        except RuntimeError:   # the reference cannot read some of its own blocks (a one-valued distances stream)
            dec = None
        _WANT[key] = (blob, dec)
    return _WANT[key]


@pytest.fixture(scope="module")
def ctxs():
    made = {}

    def get(block: int):
        if block not in made:
            made[block] = mc.Context(0, block, craft.MiB)
        return made[block]

    yield get
    for c in made.values():
        c.close()


@pytest.fixture(scope="module")
def dctx(cuda):
    ctx = mc.DContext(0)
    yield ctx
    ctx.close()


def compress(ctx, cuda, data: bytes, block: int) -> bytes:
    import torch

    d_in = torch.frombuffer(bytearray(data), dtype=torch.uint8).to(cuda)
    cap = mc.shard_bound(len(data), block)
    d_out = torch.empty(cap, dtype=torch.uint8, device=cuda)
    n = ctx.compress_shard(d_in.data_ptr(), len(data), d_out.data_ptr(), cap, torch.cuda.current_stream().cuda_stream)
    return mc.write_header(len(data), (len(data) + block - 1) // block) + d_out[:n].cpu().numpy().tobytes()


def run(ctx, dctx, cuda, data: bytes, block: int, what, routed: int = 2):
    """`data` with the general unit forced and then `routed` calls of mode 0 on the same context,
    every output compared with the oracle's; then the round trip of those bytes"""
    want, dec = want_of(data, block)
    try:
        for mode in MODES:
            ctx.set_match_mode(mode)
            got = compress(ctx, cuda, data, block)
            assert got == want, ("mode", mode, what, block, ctx.stats())
    finally:
        ctx.set_match_mode(0)
    for call in range(routed):
        got = compress(ctx, cuda, data, block)
        assert got == want, ("mode 0, call", call, what, block, ctx.stats())
    if dec is not None:
        assert mc.decompress(got) == dec, ("host decoder", what, block)
        assert dctx.decompress_host(got, len(data) + 16) == dec, ("GPU decoder", what, block)
    return dec


def run_vector(ctxs, dctx, cuda, name: str):
    _fam, block, data = craft.vectors()[name]
    dec = run(ctxs(block), dctx, cuda, data, block, name)
    # at its own block size a vector comes back whole, but for the reference's one-symbol quirk
    assert dec == (b"" if craft.one_symbol_flags(craft.profile(data)) else data), name
    if len(data) > craft.RAGGED:
        run(ctxs(craft.RAGGED), dctx, cuda, data, craft.RAGGED, name, routed=1)


@pytest.mark.parametrize("name", sorted(craft.family("no255")))
def test_long_general_coder_streams(cuda, ctxs, dctx, name):
    """66 and 128 chars chunks through the general coder: the look-back reaches past the 64 chunks
    one round reads; codes of 7 / 8 and of 7 / 8 / 9 bits, chunks on both sides of 65 536 bits"""
    run_vector(ctxs, dctx, cuda, name)


@pytest.mark.parametrize("name", sorted(craft.family("two_window")))
def test_two_staging_windows(cuda, ctxs, dctx, name):
    """a chunk of more than 65 600 bits: two staging windows, as the stream's last chunk and with a
    successor that merges its tail; `window_seam` ends 12 bits into the second window"""
    run_vector(ctxs, dctx, cuda, name)


@pytest.mark.parametrize("name", sorted(craft.family("forms")))
def test_merge_form_boundaries(cuda, ctxs, dctx, name):
    """exact chars histograms on both sides of the closed form's rule and of kJacobiMin, tie-heavy"""
    run_vector(ctxs, dctx, cuda, name)


@pytest.mark.parametrize("k", craft.BYTE8_K)
@pytest.mark.parametrize("r", craft.BYTE8_R)
def test_byte_substitution_tails(cuda, ctxs, dctx, r, k):
    """last chunks of 1, 2, 3, 4, 8191 and 8192 symbols, the first code byte at 0, 1 and 3 mod 4"""
    names = [n for n in craft.family("byte8") if n.startswith(f"byte8_k{k}_r{r}_")]
    assert len(names) == (3 if k == 1 else 2)
    for name in names:
        run_vector(ctxs, dctx, cuda, name)


@pytest.mark.parametrize("name", sorted(craft.family("deep")))
def test_deep_codes(cuda, ctxs, dctx, name):
    """codes of 16, 20 and 23 bits (the decoders' tables and segment decoder see them too), and
    the fullest chunk these builders know, 114 540 bits in two windows"""
    run_vector(ctxs, dctx, cuda, name)


def test_stream_lengths(cuda, ctxs, dctx):
    """flags and distances streams of 2 .. 34 bytes and of one round of k_tree's deep loads, give
    or take a byte; all-0xFF and 0x00-heavy streams (the register counters)"""
    for name in sorted(craft.family("lengths")):
        run_vector(ctxs, dctx, cuda, name)


def test_two_blocks_in_one_shard(cuda, ctxs, dctx):
    """a two-window block, then a no255 block: status rows and record offsets per block"""
    data = craft.two_blocks()
    assert run(ctxs(craft.TWO_BLOCKS), dctx, cuda, data, craft.TWO_BLOCKS, "two_blocks") == data


def test_one_context_family_after_family(cuda, dctx):
    """the chunk status words are cleared by k_tree in every call: a long stream, then short ones,
    then the long one again on one context, each call's bytes the oracle's (a context of its own,
    so the order of calls is this test's)"""
    order = ["no255_66", "two_window_128K_middle", "byte8_k1_r1_a1", "deepest_chunk", "len_ab5000", "window_seam",
             "half2_1M", "byte8_k3_r8191_a0", "no255_66"]
    V = craft.vectors()
    ctx = mc.Context(0, craft.MiB, craft.MiB)
    try:
        for name in order:
            data = V[name][2]
            want, _dec = want_of(data, craft.MiB)
            assert compress(ctx, cuda, data, craft.MiB) == want, name
    finally:
        ctx.close()
