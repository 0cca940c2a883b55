"""fcx7_craft — a token-level builder of FCX7 (LZ77) block payloads, for tests only.

Written from the format as oracle/fcx_oracle.c and DESIGN.md state it:

    payload = [u32 N][flags][chars][u32 pcnt][P bytes][u32 G][golomb]

  flags    bit t = token t is a literal; raw bytes when (N + 7) // 8 <= 1, else a Huffman sub-stream
  chars    the char of every token (absent when N = 0)
  P bytes  the 11-bit distances of the first pcnt match tokens, packed LSB-first, 11 pcnt // 8 + 1 bytes
  golomb   the Golomb-Rice (k = 2) words of their lengths, as 4 G bytes (absent when G = 0)
  a Huffman sub-stream = [u8 ts][ceil(2 ts / 8) B child-is-internal bitmap][ts x (u8 l, u8 r)]
                         [u32 W][W x u32 code words, root->leaf path bits LSB-first]
  with internal child k stored as (256 - real) + k, real = ts + 1, the root being node ts - 1.

A token is (p, l, c): l = None for a literal, else a match of l bytes at distance p (l = 0 is a
match token that copies nothing); c is the byte that follows.  The default sub-stream coders are
the oracle's own (oracle.huffman_stream / combine_bits / golomb_encode), so payload(tokens of
oracle.parse(d)) is oracle.compress_block(d) byte for byte.

Also here: host models of the two places of the GPU decoder whose path a stream chooses, the
segment decoder's settle loop (settle_rounds, fcx_dec_shared.h seg_decode) and k_dlz's stepping
(lz_steps, fcx_dec.hip), so that a vector's claim ("takes the serial fallback", "takes the
all-literal step with a short count") is computed, not assumed.
"""
import os
import re
import struct

import oracle

P_BITS = 11

# mirrors of fcx_dec_shared.h (test_fcx7_crafted_host.py fails if they drift)
kDMaxRounds = 12
kDMinSegBits = 256
kDRetryScale = 16
kDSymThreads = 1024
# mirrors of fcx_dec.hip's k_dlz
kDLzThreads = 1024
kDLzTile = 8192
kDLzTPT = 4

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "my_compress_amd", "csrc")


def source_constants(fname: str, names) -> dict:
    """`constexpr uint32_t NAME = VALUE;` of the kernel sources, also where one declaration
    holds several (`constexpr uint32_t A = 1, NAME = VALUE;`); None where VALUE is no literal"""
    with open(os.path.join(CSRC, fname)) as f:
        text = f.read()
    out = {}
    for n in names:
        m = re.search(r"constexpr\s+uint32_t\s+(?:\w+\s*=\s*[^,;]+,\s*)*" + n + r"\s*=\s*(\d+)\s*[,;]", text)
        out[n] = int(m.group(1)) if m else None
    return out


# ---------------------------------------------------------------------------------------------
def tokens_of(parsed):
    """oracle.parse()'s [p, l, c] (l = 0: literal) as crafter tokens"""
    return [(p, l if l else None, c) for p, l, c in parsed]


def lits(data: bytes):
    return [(0, None, c) for c in data]


def model(tokens, pcnt=None):
    """the bytes the tokens mean; stops like the reference at the first match token past the
    first `pcnt` pairs; None where a distance is 0 or reaches before the block start"""
    out = bytearray()
    seen = 0
    for p, l, c in tokens:
        if l is not None:
            if pcnt is not None and seen >= pcnt:
                break
            seen += 1
            if p == 0 or p > len(out):
                return None
            for _ in range(l):
                out.append(out[-p])
        out.append(c)
    return bytes(out)


def flag_bytes(tokens, flag_tail_bits=None) -> bytes:
    n = len(tokens)
    fl = bytearray((n + 7) // 8)
    for t, (_, l, _) in enumerate(tokens):
        if l is None:
            fl[t >> 3] |= 1 << (t & 7)
    if flag_tail_bits is not None and n % 8:
        tail = 0xFF & ~((1 << (n % 8)) - 1)
        fl[-1] = (fl[-1] & ~tail) | (tail if flag_tail_bits else 0)
    return bytes(fl)


def payload(tokens, pcnt=None, extra_pairs=(), flag_tail_bits=None, flags_stream=None, chars_stream=None,
            p_stream=None, golomb_stream=None, G=None) -> bytes:
    """pcnt: keep only the first pcnt (p, l) pairs, the flags unchanged (the decoder stops early);
    extra_pairs: (p, l) appended after the tokens' own, so that there are more pairs than match
    flags; flag_tail_bits: 0 / 1 for the unused bits of the last flags byte; *_stream: bytes that
    replace a whole sub-stream; G: the stored word count of the golomb stream"""
    n = len(tokens)
    fl = flag_bytes(tokens, flag_tail_bits)
    if flags_stream is None:
        flags_stream = oracle.huffman_stream(fl) if len(fl) > 1 else fl
    if chars_stream is None:
        chars_stream = oracle.huffman_stream(bytes(c for _, _, c in tokens))
    pairs = [(p, l) for p, l, _ in tokens if l is not None]
    if pcnt is not None:
        pairs = pairs[:pcnt]
    pairs += list(extra_pairs)
    if p_stream is None:
        p_stream = oracle.huffman_stream(oracle.combine_bits([p for p, _ in pairs], P_BITS))
    gw = oracle.golomb_encode([l for _, l in pairs])
    if golomb_stream is None:
        golomb_stream = oracle.huffman_stream(gw)
    if G is None:
        G = len(gw) // 4
    return (struct.pack("<I", n) + flags_stream + chars_stream + struct.pack("<I", len(pairs)) + p_stream +
            struct.pack("<I", G) + golomb_stream)


# ---------------------------------------------------------------------------------------------
# explicit trees.  children[k] = (left, right) of internal node k; a child < 256 is a leaf's symbol,
# 256 + j is internal node j; the root is the last node.  codes[sym] = (bits, length), root first in
# bit 0.
def tree_codes(children) -> dict:
    codes = {}
    stack = [(len(children) - 1, 0, 0)]
    while stack:
        k, bits, d = stack.pop()
        for side, ch in enumerate(children[k]):
            b = bits | (side << d)
            if ch < 256:
                codes[ch] = (b, d + 1)
            else:
                stack.append((ch - 256, b, d + 1))
    return codes


def chain_tree(ts: int, syms):
    """the degenerate chain of ts internal nodes: syms[i] (i < ts) has i ones and a zero, syms[ts]
    has ts ones; every internal child precedes its parent"""
    assert len(syms) == ts + 1 and len(set(syms)) == ts + 1
    children = []
    for k in range(ts):
        left = syms[ts - 1 - k]
        right = syms[ts] if k == 0 else 256 + (k - 1)
        children.append((left, right))
    return children, tree_codes(children)


def full_tree8(perm):
    """the complete depth-8 tree over the 256 byte values in leaf order `perm`: every code 8 bits"""
    base, children = {7: 0}, [None] * 255
    for lvl in range(6, -1, -1):
        base[lvl] = base[lvl + 1] + (1 << (lvl + 1))
    for lvl in range(8):
        for i in range(1 << lvl):
            if lvl == 7:
                children[base[7] + i] = (perm[2 * i], perm[2 * i + 1])
            else:
                children[base[lvl] + i] = (256 + base[lvl + 1] + 2 * i, 256 + base[lvl + 1] + 2 * i + 1)
    return children, tree_codes(children)


def pack_codes(codes, data) -> bytes:
    acc, pos = 0, 0
    for s in data:
        b, ln = codes[s]
        acc |= b << pos
        pos += ln
    nw = (pos + 31) // 32
    return acc.to_bytes(4 * nw, "little")


def tree_header(children) -> bytes:
    ts = len(children)
    real = ts + 1
    bm = bytearray((2 * ts + 7) // 8)
    pairs = bytearray()
    for k, lr in enumerate(children):
        for side, ch in enumerate(lr):
            x = 2 * k + side
            if ch >= 256:
                bm[x >> 3] |= 1 << (x & 7)
                pairs.append((256 - real) + (ch - 256))
            else:
                pairs.append(ch)
    return bytes([ts]) + bytes(bm) + bytes(pairs)


def huff_stream(children, codes, data, nwords=None) -> bytes:
    """a sub-stream from an explicit tree; nwords cuts the words short or pads them with zeros"""
    words = pack_codes(codes, data)
    if nwords is not None:
        words = (words + bytes(4 * nwords))[:4 * nwords]
    return tree_header(children) + struct.pack("<I", len(words) // 4) + words


# ---------------------------------------------------------------------------------------------
# fields / rebuild: a payload as a dict whose sub-streams are dicts {ts, bitmap, pairs, W, words}
# (the raw flags of N <= 8 are bytes); rebuild() lays the fields end to end again, so a changed W
# or ts moves what follows.  W is serialised as stored: set "words" as well to really remove them.
def _sub(p: bytes, q: int):
    ts = p[q]
    nbm = (2 * ts + 7) // 8
    s = {"ts": ts, "bitmap": bytearray(p[q + 1:q + 1 + nbm]), "pairs": bytearray(p[q + 1 + nbm:q + 1 + nbm + 2 * ts])}
    q += 1 + nbm + 2 * ts
    s["W"] = struct.unpack_from("<I", p, q)[0]
    s["words"] = p[q + 4:q + 4 + 4 * s["W"]]
    return s, q + 4 + 4 * s["W"]


def fields(p: bytes) -> dict:
    f = {"N": struct.unpack_from("<I", p, 0)[0]}
    q = 4
    nb = (f["N"] + 7) // 8
    if nb > 1:
        f["flags"], q = _sub(p, q)
    else:
        f["flags"] = p[q:q + nb]
        q += nb
    f["chars"] = None
    if f["N"]:
        f["chars"], q = _sub(p, q)
    f["pcnt"] = struct.unpack_from("<I", p, q)[0]
    f["P"], q = _sub(p, q + 4)
    f["G"] = struct.unpack_from("<I", p, q)[0]
    q += 4
    f["golomb"] = None
    if f["G"]:
        f["golomb"], q = _sub(p, q)
    assert q == len(p), (q, len(p))
    return f


def _unsub(s) -> bytes:
    if s is None:
        return b""
    if isinstance(s, (bytes, bytearray)):
        return bytes(s)
    return bytes([s["ts"]]) + bytes(s["bitmap"]) + bytes(s["pairs"]) + struct.pack("<I", s["W"]) + bytes(s["words"])


def rebuild(f: dict) -> bytes:
    return (struct.pack("<I", f["N"]) + _unsub(f["flags"]) + _unsub(f["chars"]) + struct.pack("<I", f["pcnt"]) +
            _unsub(f["P"]) + struct.pack("<I", f["G"]) + _unsub(f["golomb"]))


def sub_offset(f: dict, name: str) -> int:
    """byte offset of a sub-stream's ts in rebuild(f)"""
    order = ["flags", "chars", "P", "golomb"]
    q = 4
    for n in order:
        if n == "P" or n == "golomb":
            q += 4
        if n == name:
            return q
        q += len(_unsub(f[n]))
    raise KeyError(name)


def cut_words(f: dict, name: str, W: int) -> dict:
    """sub-stream `name` with W words, the others really removed"""
    g = dict(f)
    s = dict(f[name])
    s["W"] = W
    s["words"] = bytes(s["words"][:4 * W])
    g[name] = s
    return g


def record(p: bytes) -> bytes:
    return struct.pack("<I", len(p)) + p


def shard(records):
    """(the records back to back, their count)"""
    return b"".join(records), len(records)


# ---------------------------------------------------------------------------------------------
# host model of seg_decode's settle loop (fcx_dec_shared.h).  step(pos) -> the bit after the code
# that starts at pos, or None where code_step returns false.
def chain_stepper(ts: int, words: bytes):
    nbits = 8 * len(words)
    s = _bit_string(words)

    def step(pos):
        z = s.find("0", pos, pos + ts)
        ln = ts if z < 0 else z - pos + 1
        return None if pos + ln > nbits else pos + ln

    return step, nbits


def _bit_string(words: bytes) -> str:
    nbits = 8 * len(words)
    return bin(int.from_bytes(words, "little") | (1 << nbits))[3:][::-1]   # s[i] = bit i


def tree_stepper(children, words: bytes):
    nbits = 8 * len(words)
    s = _bit_string(words)
    root = len(children) - 1

    def step(pos):
        k = root
        for d in range(1, 33):   # huff_sym: codes of <= 32 bits
            if pos + d > nbits:
                return None
            ch = children[k][s[pos + d - 1] == "1"]
            if ch < 256:
                return pos + d
            k = ch - 256
        return None

    return step, nbits


def seg_bits(nbits: int) -> int:
    return max(kDMinSegBits, ((nbits + kDSymThreads - 1) // kDSymThreads + 31) & ~31)


def _jacobi(step, nbits: int, S: int):
    """(settled, rounds) of one attempt with segments of S bits"""
    T = kDSymThreads
    lo = [min(i * S, nbits) for i in range(T)]
    hi = [min(lo[i] + S, nbits) for i in range(T)]

    def walk(i, start):
        pos = start
        while pos < hi[i]:
            pos = step(pos)
            if pos is None:
                return nbits
        return pos

    st = list(lo)
    mine = list(lo)
    ex = [walk(i, lo[i]) for i in range(T)]
    for rnd in range(kDMaxRounds):
        moved = False
        for i in range(T - 1):
            if st[i + 1] != ex[i]:
                st[i + 1] = ex[i]
                moved = True
        if not moved:
            return True, rnd + 1
        for i in range(T):
            if st[i] != mine[i]:
                mine[i] = st[i]
                ex[i] = walk(i, mine[i])
    return False, kDMaxRounds


def settle_rounds(step, nbits: int):
    """('first' | 'retry' | 'fallback', rounds counted as the kernel counts them)"""
    S0 = seg_bits(nbits)
    ok, r = _jacobi(step, nbits, S0)
    if ok:
        return "first", r
    ok, r2 = _jacobi(step, nbits, S0 * kDRetryScale)
    return ("retry" if ok else "fallback"), r + r2


def sub_children(sub) -> list:
    """the children of a parsed sub-stream (fields()), as huff_stream and tree_stepper take them"""
    ts = sub["ts"]
    out = []
    for k in range(ts):
        pair = []
        for x in (2 * k, 2 * k + 1):
            v = sub["pairs"][x]
            if (sub["bitmap"][x >> 3] >> (x & 7)) & 1:
                v = 256 + v - (256 - (ts + 1))
            pair.append(v)
        out.append(tuple(pair))
    return out


def model_stats(p: bytes, chars_step=None):
    """(settle rounds, serial fallbacks) that k_dsyms counts for a well-formed payload, summed over
    its Huffman sub-streams; chars_step: a faster stepper for the chars stream"""
    f = fields(p)
    count = {"flags": (f["N"] + 7) // 8, "chars": f["N"], "P": P_BITS * f["pcnt"] // 8 + 1, "golomb": 4 * f["G"]}
    rounds = fallbacks = 0
    for name, n in count.items():
        sub = f[name]
        if not isinstance(sub, dict) or sub["ts"] == 0 or n == 0:
            continue   # raw flags, an absent stream, a one-symbol stream: no segment decode
        children = sub_children(sub)
        codes = tree_codes(children)
        if len(codes) == 256 and all(ln == 8 for _, ln in codes.values()):
            continue   # every code 8 bits: k_dsyms substitutes bytes
        step, nbits = chars_step if (name == "chars" and chars_step) else tree_stepper(children, sub["words"])
        how, r = settle_rounds(step, nbits)
        rounds += r
        fallbacks += how == "fallback"
    return rounds, fallbacks


# ---------------------------------------------------------------------------------------------
# host model of k_dlz's stepping (fcx_dec.hip): which kind of step takes which tokens
def lz_steps(tokens, pcnt=None):
    """[("fast", tokens) | ("tile", tokens, bytes, next window)] over the tokens decoded"""
    n_eff, seen = len(tokens), 0
    if pcnt is not None:
        for t, (_, l, _) in enumerate(tokens):
            if l is not None:
                if seen == pcnt:
                    n_eff = t
                    break
                seen += 1
    full = kDLzTPT * kDLzThreads
    tc, window, steps = 0, full, []
    while tc < n_eff:
        limit = min(n_eff, tc + window)
        toks = tokens[tc:limit]
        if all(l is None for _, l, _ in toks):
            steps.append(("fast", limit - tc))
            tc, window = limit, full
            continue
        off = taken = 0
        for _, l, _ in toks:
            ln = 1 if l is None else l + 1
            if off + ln > kDLzTile:
                break
            off += ln
            taken += 1
        if taken == 0:
            steps.append(("stuck", 0, 0, 0))
            break
        window = min(full, max(256, 5 * kDLzTile * taken // (4 * max(off, 1))))
        steps.append(("tile", taken, off, window))
        tc += taken
    return steps
