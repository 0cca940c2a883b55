"""fcx8_craft — a token-level builder of FCX8 (LZ78) block payloads, for tests only.

Written from the format as oracle/lz78_oracle.c and DESIGN.md state it:

    payload = [u32 wcnt][bitmap][u32 G]( G > 1: [tree][u32 N][u32 W][W x u32 group words] | [u32 N] )[gpos][chars]

  bitmap   bit i = dictionary index i is used by some token (index 0: no parent); it ends with the
           byte of its wcnt-th set bit.  The r-th set bit (its rank) is written as group r >> 8 and
           in-group position r & 255
  tree     G - 1 nodes of (lc, rc) u32 pairs, the root being node G - 2; a child < G is the leaf of
           that group, else node child - G.  Group codes are root->leaf path bits, LSB-first
  gpos     N bytes, the in-group position of every token's index
  chars    the char of every token: the Huffman sub-stream of fcx7_craft (same serialisation)

A token is (idx, c): the phrase of dictionary entry idx (0: the empty phrase; token t makes entry
t + 1, so idx <= t) followed by the byte c.  model() is that definition and nothing else.
"""
import os
import re
import struct

import numpy as np

import oracle
from fcx7_craft import (CSRC, chain_stepper, chain_tree, full_tree8, huff_stream, record, seg_bits,  # noqa: F401
                        settle_rounds, shard, source_constants, tree_header)
from fcx7_craft import _sub, _unsub


def kernel_constants() -> dict:
    """the bounds of fcx_lz78_dec.hip, read from the sources: the corpus' edges follow the kernels"""
    k = source_constants("fcx_lz78_dec.hip", ["kBatch", "kLong", "kMaxDepth", "kLinkTPT"])
    k.update(source_constants("fcx_dec_shared.h", ["kDTblBits"]))
    with open(os.path.join(CSRC, "..", "..", "include", "fcx.h")) as f:
        m = re.search(r"#define\s+FCX_MAX_BLOCK_BYTES\s+\(1u\s*<<\s*(\d+)\)", f.read())
    block = 1 << int(m.group(1))
    with open(os.path.join(CSRC, "fcx_lz78_dec.hip")) as f:
        text = f.read()
    m = re.search(r"constexpr\s+uint32_t\s+kCapBlock\s*=\s*FCX_MAX_BLOCK_BYTES\s*\+\s*(\d+)\s*;", text)
    k["kCapBlock"] = block + int(m.group(1))
    m = re.search(r"constexpr\s+uint32_t\s+kGmax\s*=\s*FCX_MAX_BLOCK_BYTES\s*/\s*(\d+)\s*\+\s*(\d+)\s*;", text)
    k["kGmax"] = block // int(m.group(1)) + int(m.group(2))
    assert all(v is not None for v in k.values()), k
    return k


# ---------------------------------------------------------------------------------------------
def model(tokens, one_symbol_zero: bool = True):
    """the bytes the tokens mean: phrase t = phrase[idx - 1] + char, and a block that ends in 0x00
    loses that byte.  None where a token refers to itself or forward (idx > t).  The format does
    not store the symbol of a one-symbol char stream: such a block's chars decode as zeros."""
    if not tokens:
        return b""
    idx, chars = zip(*tokens)
    if one_symbol_zero and len(set(chars)) == 1:
        chars = bytes(len(chars))
    if not any(idx):
        out = bytearray(chars)
    else:
        out, start, ln = bytearray(), [], []
        for t, ix in enumerate(idx):
            if ix > t:
                return None
            start.append(len(out))
            if ix:
                s = start[ix - 1]
                out += out[s:s + ln[ix - 1]]
            out.append(chars[t])
            ln.append(len(out) - start[t])
    if out and out[-1] == 0:
        del out[-1]
    return bytes(out)


# ---------------------------------------------------------------------------------------------
# group trees: [(lc, rc)] of G - 1 nodes, the root last
def balanced_tree(G: int):
    """queue merge: the first two of the queue become the children of the next node"""
    q, tree, head = list(range(G)), [], 0
    while len(q) - head > 1:
        tree.append((q[head], q[head + 1]))
        head += 2
        q.append(G + len(tree) - 1)
    return tree


def chain_group_tree(G: int, leaves=None):
    """the degenerate chain of G - 1 nodes: leaves[i] (i < G - 1) has i ones and a zero, leaves[G - 1]
    has G - 1 ones (fcx7_craft.chain_stepper walks its codes with ts = G - 1)"""
    leaves = list(range(G)) if leaves is None else list(leaves)
    assert sorted(leaves) == list(range(G)) and G >= 2
    tree = []
    for k in range(G - 1):
        tree.append((leaves[G - 2 - k], leaves[G - 1] if k == 0 else G + k - 1))
    return tree


def tree_codes(tree, G: int) -> dict:
    """{group: (bits, length)} of the (lc, rc) form, root first in bit 0; a malformed tree yields the
    codes a walk from the root meets within 64 levels"""
    codes = {}
    stack = [(G - 2, 0, 0)]
    while stack:
        k, bits, d = stack.pop()
        if d >= 64 or not 0 <= k < len(tree):
            continue
        for side, ch in enumerate(tree[k]):
            b = bits | (side << d)
            if ch < G:
                codes.setdefault(ch, (b, d + 1))
            else:
                stack.append((ch - G, b, d + 1))
    return codes


def pack_bits(pairs) -> bytes:
    """(bits, length) codes LSB-first into whole u32 words"""
    s = "".join(format(b, "0%db" % ln)[::-1] if ln else "" for b, ln in pairs)
    nw = (len(s) + 31) // 32
    return int(s[::-1], 2).to_bytes(4 * nw, "little") if s else b""


def tree_bytes(tree) -> bytes:
    return b"".join(struct.pack("<II", lc, rc) for lc, rc in tree)


# ---------------------------------------------------------------------------------------------
def payload(tokens, *, extra_used=(), wcnt=None, bitmap=None, G=None, tree=None, N=None, W=None, group_words=None,
            gpos=None, chars_stream=None) -> bytes:
    """tokens (idx, char) as an FCX8 payload.  extra_used: indices that join the used set though no
    token refers to them (they shift the ranks, as in a real bitmap).  Every other keyword replaces
    one field as stored and nothing else: wcnt, bitmap (bytes), G (> 1 selects the layout with a
    tree), tree ([(lc, rc)], default balanced_tree(G)), N, W, group_words (bytes), gpos (bytes),
    chars_stream (bytes)."""
    idx = np.array([t[0] for t in tokens], dtype=np.int64)
    chars = bytes(t[1] for t in tokens)
    used = np.union1d(idx, np.asarray(extra_used, dtype=np.int64))
    assert len(used), "an FCX8 payload has at least one used index"
    rank = np.searchsorted(used, idx)
    if bitmap is None:
        bits = np.zeros(8 * (int(used[-1]) // 8 + 1), dtype=np.uint8)
        bits[used] = 1
        bitmap = np.packbits(bits, bitorder="little").tobytes()
    if wcnt is None:
        wcnt = len(used)
    if G is None:
        G = (len(used) + 255) // 256
    if gpos is None:
        gpos = (rank & 255).astype(np.uint8).tobytes()
    if N is None:
        N = len(tokens)
    if chars_stream is None:
        chars_stream = oracle.huffman_stream(chars)
    p = struct.pack("<I", wcnt) + bitmap + struct.pack("<I", G & 0xFFFFFFFF)
    if G > 1:
        if tree is None:
            tree = balanced_tree(G)
        if group_words is None:
            codes = tree_codes(tree, G)
            group_words = pack_bits(codes[int(g)] for g in rank >> 8)
        if W is None:
            W = len(group_words) // 4
        p += tree_bytes(tree) + struct.pack("<II", N, W) + group_words
    else:
        p += struct.pack("<I", N)
    return p + gpos + chars_stream


# ---- the payload layout my_decompress_file_lz78 reads (3478-3600) ----
def parse(p: bytes) -> dict:
    """field offsets of one payload: wcnt, bitmap, G, [tree, N, W, words], N, gpos, char header"""
    f = {"wcnt": struct.unpack_from("<I", p, 0)[0]}
    q, seen = 4, 0
    while True:   # the bitmap ends with the byte of its wcnt-th set bit
        seen += bin(p[q]).count("1")
        q += 1
        if seen >= f["wcnt"]:
            break
    f["G"] = G = struct.unpack_from("<I", p, q)[0]
    q += 4
    if G > 1:
        f["tree"] = q
        q += 8 * (G - 1)
        f["N"], f["W"] = struct.unpack_from("<II", p, q)
        f["W_off"] = q + 4
        q += 8 + 4 * f["W"]
    else:
        f["N"] = struct.unpack_from("<I", p, q)[0]
        q += 4
    f["gpos"] = q
    q += f["N"]
    f["ts"] = ts = p[q]
    f["cbm"] = q + 1
    f["cpairs"] = q + 1 + (2 * ts + 7) // 8
    f["nw_off"] = f["cpairs"] + 2 * ts
    f["nw"] = struct.unpack_from("<I", p, f["nw_off"])[0]
    assert f["nw_off"] + 4 + 4 * f["nw"] == len(p)
    return f


def fields(p: bytes) -> dict:
    """a well-formed payload as named fields: wcnt, bitmap, G, tree ([(lc, rc)] or None), N, W and
    group_words (None without a tree), gpos, chars (a sub-stream dict {ts, bitmap, pairs, W, words}
    as fcx7_craft.fields has them)"""
    o = parse(p)
    G = o["G"]
    f = {"wcnt": o["wcnt"], "G": G, "N": o["N"], "tree": None, "W": None, "group_words": None}
    if G > 1:
        f["bitmap"] = p[4:o["tree"] - 4]
        f["tree"] = [struct.unpack_from("<II", p, o["tree"] + 8 * j) for j in range(G - 1)]
        f["W"] = o["W"]
        f["group_words"] = p[o["W_off"] + 4:o["gpos"]]
    else:
        f["bitmap"] = p[4:o["gpos"] - 8]
    f["gpos"] = p[o["gpos"]:o["gpos"] + o["N"]]
    f["chars"], end = _sub(p, o["gpos"] + o["N"])
    assert end == len(p)
    return f


def rebuild(f: dict) -> bytes:
    """the fields laid end to end again, every count as stored (set the bytes as well to move them)"""
    p = struct.pack("<I", f["wcnt"]) + bytes(f["bitmap"]) + struct.pack("<I", f["G"])
    if f["tree"] is not None:
        p += tree_bytes(f["tree"]) + struct.pack("<II", f["N"], f["W"]) + bytes(f["group_words"])
    else:
        p += struct.pack("<I", f["N"])
    return p + bytes(f["gpos"]) + _unsub(f["chars"])
