"""k_encode's byte-substitution branch (fcx_entropy.hip: every chars code 8 bits) at every place its
LDS staging decides something, against the oracle: each lane shifts its 64 code bytes by the
chunk's byte offset in the output word and stores them as whole words at a swizzled index, the low
bits of a lane's first word coming from the lane before it.  So the inputs here move the byte
offset through 0 .. 3, end the stream on every kind of last lane and last chunk, put chars
segments read from the stream between segments read from the input, and run the same context
over them twice and after a text input.

The inputs are seeded shuffles of every byte value equally often (a block of plain random bytes
this small does not balance its histogram), at the block sizes 65536 and 12293, two or three
blocks a shard: full blocks, then one cut to a chosen token count.  What each one reaches is
asserted on the CPU with tests/entropy_craft.py's model of the record (profile: byte8, obyte,
chunks) before anything runs.  Bar: the bytes equal oracle.compress_file's.  Every input is a
legal block; nothing here is built to fail."""
import functools
import random

import numpy as np
import pytest

import entropy_craft as craft
import inputs
import my_compress_amd as mc
import oracle

pytestmark = pytest.mark.gpu

CHUNK = craft.CHUNK
SEG = 64                      # kSymL: the symbols of one lane, and of one chars segment descriptor
BLOCKS = (65536, 12293)
DELTAS = (0, 1, -1, 63, -63, 64, -64, 65, -65)
CAP = 4 * 65536


def balanced(n: int, seed: int) -> bytearray:
    """n bytes of a seeded shuffle of every byte value equally often"""
    s = list(range(256)) * (n // 256 + 1)
    random.Random(seed).shuffle(s)
    return bytearray(s[:n])


def plant(buf: bytearray, at: int, length: int, back: int) -> None:
    """a copy of `length` bytes from `back` bytes before"""
    buf[at:at + length] = buf[at - back:at - back + length]


@functools.lru_cache(maxsize=None)
def shard(block: int, seed: int, ntok_last: int, full: int = 1, plants: int = 0, mixed: bool = False) -> bytes:
    """`full` whole blocks and a last one cut to `ntok_last` tokens.  plants: that many three-byte
    copies near the start of the first block (each adds a flag byte value, so the flags stream's
    tree and with it the chars' first code byte move); mixed: a 3-byte and a 258-byte copy in the
    middle of the first block's first chunk"""
    parts = []
    for i in range(full):
        b = balanced(block, 100 * seed + i)
        if i == 0:
            for j in range(plants):
                plant(b, 40 + 21 * j, 3, 10)
            if mixed:
                plant(b, 2000, 3, 700)
                plant(b, 4000, 258, 1500)
        parts.append(bytes(b))
    # (balanced over its own length: the cut drops a few bytes a random match had taken)
    parts.append(craft.cut_tokens(bytes(balanced(min(block, ntok_last + 64), 100 * seed + 99)), ntok_last))
    assert len(parts[-1]) <= block
    return b"".join(parts)


@functools.lru_cache(maxsize=None)
def model(data: bytes, block: int):
    """entropy_craft's profile of every block, each chars stream through the byte substitution"""
    prs = craft.profiles(data, block)
    assert 2 <= len(prs) <= 4
    for pr in prs:
        assert pr["chars"]["byte8"], craft.row(pr)
    return prs


@functools.lru_cache(maxsize=None)
def want_of(data: bytes, block: int) -> bytes:
    return oracle.compress_file(data, block)


def ends_case(block: int, i: int):
    """the last block's chars: k whole chunks and DELTAS[i] symbols (k = 1 at 12293)"""
    k = 1 if block < 3 * CHUNK + 65 else 1 + i % 3
    return shard(block, 10 + i, k * CHUNK + DELTAS[i])


def align_case(block: int, e: int, plants: int):
    """the last block e bytes longer, `plants` short copies early in the first block"""
    return shard(block, 40 + e, CHUNK + 100 + e, plants=plants)


# (e, plants): the pairs the alignment test runs; the test asserts that they reach all four offsets
ALIGN = tuple((e, p) for e in range(4) for p in (e, e + 4))


@pytest.fixture(scope="module")
def ctxs(cuda):
    made = {b: mc.Context(0, b, CAP) for b in BLOCKS}
    yield made
    for c in made.values():
        c.close()


def compress(ctx, cuda, data: bytes, block: int) -> bytes:
    import torch

    d_in = torch.frombuffer(bytearray(data), dtype=torch.uint8).to(cuda)
    cap = mc.shard_bound(len(data), block)
    d_out = torch.empty(cap, dtype=torch.uint8, device=cuda)
    n = ctx.compress_shard(d_in.data_ptr(), len(data), d_out.data_ptr(), cap, torch.cuda.current_stream().cuda_stream)
    return mc.write_header(len(data), (len(data) + block - 1) // block) + d_out[:n].cpu().numpy().tobytes()


def twice(ctx, cuda, data: bytes, block: int, what):
    """the same input through the context twice in a row, each output the oracle's"""
    want = want_of(data, block)
    for call in range(2):
        assert compress(ctx, cuda, data, block) == want, (what, block, "call", call, ctx.stats())


@pytest.mark.parametrize("i", range(len(DELTAS)))
@pytest.mark.parametrize("block", BLOCKS)
def test_chunk_ends(cuda, ctxs, block, i):
    """chars counts of a whole number of chunks and that +- 1, 63, 64, 65: a last lane of 0, 1 and
    63 symbols, a last chunk of one word, of one lane, of one lane and a symbol"""
    d = DELTAS[i]
    data = ends_case(block, i)
    st = model(data, block)[-1]["chars"]
    assert st["n"] % CHUNK == d % CHUNK and st["chunks"] == -(-st["n"] // CHUNK)
    last = st["n"] - (st["chunks"] - 1) * CHUNK          # the last chunk's symbols
    assert last == (d if d > 0 else CHUNK + d)
    assert last % SEG == {0: 0, 1: 1, -1: 63, 63: 63, -63: 1, 64: 0, -64: 0, 65: 1, -65: 63}[d]   # the last lane's symbols
    assert d != 1 or int(st["nw"][-1]) == 1
    twice(ctxs[block], cuda, data, block, ("ends", d))


def test_every_staging_alignment(cuda, ctxs):
    """the chars' first code byte at 0, 1, 2 and 3 mod 4 of the output (sh0 = 0, 8, 16, 24), by the
    oracle's record layout, at both block sizes"""
    for block in BLOCKS:
        seen = set()
        for e, plants in ALIGN:
            data = align_case(block, e, plants)
            prs = model(data, block)
            seen |= {pr["chars"]["obyte"] % 4 for pr in prs}
            assert all(int(pr["chars"]["sh0"][0]) == 8 * (pr["chars"]["obyte"] % 4) for pr in prs)
        assert seen == {0, 1, 2, 3}, (block, seen)
        for e, plants in ALIGN:
            twice(ctxs[block], cuda, align_case(block, e, plants), block, ("align", e, plants))


def mixed_segments(block: bytes):
    """per chars segment of the block's first chunk: the input offset its symbols sit at minus their
    index in the stream when the segment is a run of literals, else None"""
    _p, l, _c = craft.parse_arrays(block)
    pos = np.concatenate(([0], np.cumsum(l.astype(np.int64) + 1)[:-1])) + l   # each token's char in the input
    out = []
    for s in range(0, min(len(l), CHUNK) - SEG + 1, SEG):
        out.append(int(pos[s]) - s if not l[s:s + SEG].any() else None)
    return out, l


@pytest.mark.parametrize("block", BLOCKS)
def test_mixed_segments(cuda, ctxs, block):
    """a 3-byte and a 258-byte copy inside a chunk: segments holding a match between runs of
    literals that lie 0, 3 and 3 + 257 bytes further on in the input than in the stream"""
    data = shard(block, 70, CHUNK + 7, mixed=True)
    model(data, block)
    segs, l = mixed_segments(data[:block])
    long = int(l[:CHUNK].max())   # (the format's longest match and the char after it take the 258 bytes)
    assert 3 in l[:CHUNK] and long == 257
    a, b, c = segs.index(0), segs.index(3), segs.index(3 + long)   # runs of literals at three offsets, in this order,
    assert a < b < c and None in segs[a:b] and None in segs[b:c]   # a segment with a match between each two
    twice(ctxs[block], cuda, data, block, "mixed")


@pytest.mark.parametrize("block", BLOCKS)
def test_after_a_text_input(cuda, ctxs, block):
    """a text input (the general coder: ORs into zeroed staging words, look-back, windows), then a
    byte-substitution input on the same context, and so on: no staged word depends on the call before"""
    text = inputs.generate("text", 9, 3 * block - 5)
    assert not all(pr["chars"]["byte8"] for pr in craft.profiles(text, block))
    ctx = ctxs[block]
    cases = [ends_case(block, 2), align_case(block, 3, 3), shard(block, 70, CHUNK + 7, mixed=True), ends_case(block, 7)]
    for n, data in enumerate(cases):
        assert compress(ctx, cuda, text, block) == want_of(text, block), ("text", n)
        assert compress(ctx, cuda, data, block) == want_of(data, block), ("after text", n, ctx.stats())
