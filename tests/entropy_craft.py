"""Crafted inputs for the entropy stage (fcx_entropy.hip: k_tree, k_encode), a host model that says
where each of them goes, and the models of k_tree's three merge forms (no GPU here).

The model, `profile(block)`, is built from the oracle alone: its parse gives the four streams'
source bytes (the flag bytes, the chars, the 11-bit distances, the golomb words), its own
sub-streams give the trees, and from those follow what the kernels branch on:

  k_tree    the merge form (`closed` when sw[0] + sw[1] > sw[real - 1]; `fixed` for nint >=
            kJacobiMin, with its rounds; `serial` otherwise), the deepest code, the stream length
            (16-byte loads kDeep deep over kTreeT threads, then a byte tail)
  k_encode  `byte8` (all 256 codes 8 bits: the byte substitution) or the general coder; per chunk of
            kChunk symbols its bits T, its first bit sh0 in the output word, its words nw and its
            staging windows ceil(nw / kEncWords); the chunk that ends fewer than 32 bits into its
            last window (`seam`: the `prevlast` branch)

The kernels' constants are read from their sources, so a change there moves the predicates.
tests/test_entropy_craft.py pins every builder on the CPU; tests/test_gpu_entropy_edges.py runs
them through the encoder.  Seeds go through random.Random(seed) only (randbytes, shuffle).
"""
import bisect
import ctypes
import functools
import os
import random
import re
import struct

import numpy as np

import fcx7_craft as f7
import oracle

INF = 2**32 - 1
MiB = 1 << 20
NAMES = ("flags", "chars", "P", "golomb")
RAGGED = 12293


# ---------------------------------------------------------------------------------------------
# the kernels' constants
def _expression(fname: str, name: str, known: dict) -> int:
    """`constexpr uint32_t NAME = <expression over known names>;` evaluated in integers"""
    with open(os.path.join(f7.CSRC, fname)) as f:
        m = re.search(r"constexpr\s+uint32_t\s+" + name + r"\s*=\s*([^;]+);", f.read())
    expr = m.group(1)
    assert re.fullmatch(r"[\w\s+\-*/()]+", expr), expr
    names = set(re.findall(r"[A-Za-z_]\w*", expr))
    assert names <= set(known), (expr, names - set(known))
    return int(eval(expr.replace("/", "//"), {"__builtins__": {}}, dict(known)))


def constants() -> dict:
    K = f7.source_constants("fcx_device.h", ["kChunk", "kStreams"])
    K.update(f7.source_constants("fcx_entropy.hip", ["kTreeT", "kJacobiMin", "kJacobiMax", "kDeep", "kEncT"]))
    assert all(v is not None for v in K.values()), K
    K["kEncWords"] = _expression("fcx_entropy.hip", "kEncWords", K)
    K["kDeepBytes"] = 16 * K["kDeep"] * K["kTreeT"]   # the bytes one round of k_tree's deep loads counts
    K["kMaxCodeLen"] = 32                              # above it k_tree raises kErrCodeLen
    return K


K = constants()
CHUNK = K["kChunk"]


# ---------------------------------------------------------------------------------------------
# k_tree's merge forms (moved from test_merge_forms.py, which checks them against the oracle).
# Each returns the children (left, right) of every internal node as ("L", symbol) or
# ("I", creation index).
def sorted_leaves(w):
    """(weight, symbol) of the symbols with weight > 0, stably sorted by weight (458-498)"""
    return sorted(((x, s) for s, x in enumerate(w) if x > 0), key=lambda t: (t[0], t[1]))


def serial(leaves):
    L = [x for x, _ in leaves]
    n = len(L)
    I, kids = [], []
    lq = iq = 0
    for k in range(n - 1):
        pick = []
        for _ in range(2):
            if lq < n and (iq >= len(I) or L[lq] <= I[iq]):
                pick.append((L[lq], ("L", leaves[lq][1])))
                lq += 1
            else:
                pick.append((I[iq], ("I", iq)))
                iq += 1
        I.append(pick[0][0] + pick[1][0])
        kids.append((pick[0][1], pick[1][1]))
    return kids


def closed(leaves):
    n = len(leaves)
    L = [x for x, _ in leaves]
    if n < 2 or not L[0] + L[1] > L[-1]:
        return None
    ident = lambda i: ("L", leaves[i][1]) if i < n else ("I", i - n)
    return [(ident(2 * k), ident(2 * k + 1)) for k in range(n - 1)]


def fixed_point(leaves, max_rounds=400):
    n = len(leaves)
    L = [x for x, _ in leaves]
    I = [INF] * (n - 1)
    for rounds in range(1, max_rounds + 1):
        P = [None] * (2 * n - 1)
        for t, x in enumerate(L):   # a leaf after the internal nodes lighter than it
            P[t + bisect.bisect_left(I, x)] = (x, ("L", leaves[t][1]))
        for j, x in enumerate(I):   # an internal node after the leaves no heavier than it
            P[j + bisect.bisect_right(L, x)] = (x, ("I", j))
        nI = [INF if INF in (P[2 * k][0], P[2 * k + 1][0]) else P[2 * k][0] + P[2 * k + 1][0] for k in range(n - 1)]
        if nI == I:
            return [(P[2 * k][1], P[2 * k + 1][1]) for k in range(n - 1)], rounds
        I = nI
    return None, max_rounds


def depths(kids) -> dict:
    """symbol -> code length of a merge model's tree (the root is the last node)"""
    out = {}
    stack = [(len(kids) - 1, 0)] if kids else []
    while stack:
        k, d = stack.pop()
        for kind, x in kids[k]:
            if kind == "L":
                out[x] = d + 1
            else:
                stack.append((x, d + 1))
    return out


def tree_form(w):
    """(form, rounds) k_tree's rule selects for the weights w: `none` (fewer than two leaves),
    `closed`, `fixed` (rounds: the iteration that sees no change; past kJacobiMax the kernel falls
    to the serial merge, form `fixed>serial`) or `serial`"""
    leaves = sorted_leaves(w)
    real = len(leaves)
    nint = real - 1 if real >= 2 else 0
    if not nint:
        return "none", 0
    if leaves[0][0] + leaves[1][0] > leaves[-1][0]:
        return "closed", 0
    if nint >= K["kJacobiMin"]:
        _, rounds = fixed_point(leaves)
        return ("fixed" if rounds <= K["kJacobiMax"] else "fixed>serial"), rounds
    return "serial", 0


# ---------------------------------------------------------------------------------------------
# the model
def parse_arrays(block: bytes):
    """oracle.parse as arrays (distance, length, char); length 0: a literal"""
    n = len(block)
    p = (ctypes.c_uint32 * (n + 1))()
    l = (ctypes.c_uint32 * (n + 1))()
    c = (ctypes.c_uint8 * (n + 1))()
    N = oracle.orc().orc_lz77_parse(block, n, oracle.FINDER_EXHAUSTIVE, p, l, c)
    return (np.frombuffer(p, dtype=np.uint32)[:N].copy(), np.frombuffer(l, dtype=np.uint32)[:N].copy(),
            np.frombuffer(c, dtype=np.uint8)[:N].copy())


def sources(block: bytes) -> dict:
    """the bytes each stream codes: f7.flag_bytes, the chars, oracle.combine_bits and
    oracle.golomb_encode over the oracle's tokens"""
    p, l, c = parse_arrays(block)
    m = l > 0
    flags = np.packbits(~m, bitorder="little").tobytes()   # == f7.flag_bytes (test_entropy_craft.py)
    return {"N": len(c), "pcnt": int(m.sum()), "flags": flags, "chars": c.tobytes(),
            "P": oracle.combine_bits(p[m].tolist(), f7.P_BITS), "golomb": oracle.golomb_encode(l[m].tolist())}


def token_count(block: bytes) -> int:
    return len(parse_arrays(block)[2])


def profile(block: bytes, rec_off: int = 0) -> dict:
    """per stream of one block's record, which starts `rec_off` bytes into the shard's output:
    n, hist, real, form, rounds, lens, deepest, byte8, active (Huffman-coded at all), chunks, and per
    chunk bits, sh0, nw, windows; seam: the chunks (not the stream's last) that take the
    `prevlast` branch.  Also `N`, `pcnt`, `record` (the oracle's record bytes, length included)."""
    src = sources(block)
    subs, active = {}, {}
    for name in NAMES:
        s = src[name]
        active[name] = {"flags": len(s) > 1, "chars": src["N"] > 0, "P": True, "golomb": len(s) > 0}[name]
        subs[name] = oracle.huffman_stream(s) if active[name] else (s if name == "flags" else b"")
    payload = (struct.pack("<I", src["N"]) + subs["flags"] + subs["chars"] + struct.pack("<I", src["pcnt"]) + subs["P"] +
               struct.pack("<I", len(src["golomb"]) // 4) + subs["golomb"])
    assert payload == oracle.compress_block(block), "the model's streams are not the oracle's payload"
    out = {"N": src["N"], "pcnt": src["pcnt"], "record": f7.record(payload)}
    q = rec_off + 4 + 4
    for name in NAMES:
        if name in ("P", "golomb"):
            q += 4
        s = np.frombuffer(src[name], dtype=np.uint8)
        st = {"n": len(s), "active": active[name], "src": src[name]}
        out[name] = st
        if not active[name]:
            q += len(subs[name])
            continue
        hist = np.bincount(s, minlength=256)
        sub, _ = f7._sub(subs[name], 0)
        lens = np.zeros(256, dtype=np.int64)
        if sub["ts"]:
            for sym, (_, ln) in f7.tree_codes(f7.sub_children(sub)).items():
                lens[sym] = ln
        form, rounds = tree_form(hist.tolist())
        obyte = q + 1 + (2 * sub["ts"] + 7) // 8 + 2 * sub["ts"] + 4
        q += len(subs[name])
        byte8 = bool((lens == 8).all())
        starts = np.arange(0, len(s), CHUNK)
        bits = np.add.reduceat(lens[s], starts)
        assert int(bits.sum()) <= 32 * sub["W"] < int(bits.sum()) + 32
        g0 = 8 * obyte + np.concatenate(([0], np.cumsum(bits)[:-1]))
        sh0 = g0 & 31
        nw = (sh0 + bits + 31) >> 5
        windows = -(-nw // K["kEncWords"])
        e_last = sh0 + bits - 32 * K["kEncWords"] * (windows - 1)   # end bit inside the last window
        seam = [int(c) for c in np.flatnonzero((windows > 1) & (e_last > 0) & (e_last < 32)) if c != len(starts) - 1]
        st.update(hist=hist, real=int((hist > 0).sum()), form=form, rounds=rounds, lens=lens,
                  deepest=int(lens.max()), byte8=byte8, obyte=obyte, chunks=len(starts), bits=bits, sh0=sh0, nw=nw,
                  windows=windows, seam=[] if byte8 else seam, W=sub["W"])
    assert q == rec_off + len(out["record"])
    return out


def profiles(data: bytes, block: int) -> list:
    """profile of every block of a shard, each at its record's offset"""
    out, off = [], 0
    for bs in range(0, len(data), block):
        out.append(profile(data[bs:bs + block], off))
        off += len(out[-1]["record"])
    return out


def row(pr: dict, name: str = "chars") -> dict:
    """the line DESIGN.md's table holds for a stream"""
    st = pr[name]
    return {"n": st["n"], "real": st["real"], "form": st["form"], "rounds": st["rounds"], "chunks": st["chunks"],
            "windows": int(st["windows"].max()), "deepest": st["deepest"], "byte8": st["byte8"],
            "max_bits": int(st["bits"].max())}


# ---------------------------------------------------------------------------------------------
# builders.  Every one is deterministic from its arguments and returns bytes.
def _draw(rng: random.Random, n: int, alphabet, weights=None) -> np.ndarray:
    """n values of `alphabet`, uniform or by integer weights, from rng.randbytes"""
    alphabet = np.asarray(alphabet, dtype=np.uint8)
    u = np.frombuffer(rng.randbytes(4 * n), dtype="<u4").astype(np.int64)
    if weights is None:
        return alphabet[u % len(alphabet)]
    cum = np.cumsum(np.asarray(weights, dtype=np.int64))
    return alphabet[np.searchsorted(cum, u % cum[-1], side="right")]


def cut_tokens(data: bytes, ntok: int) -> bytes:
    """the prefix of `data` whose oracle parse is the first `ntok` tokens of data's"""
    _p, l, _c = parse_arrays(data)
    assert ntok <= len(l), (ntok, len(l))
    out = data[:int((l[:ntok].astype(np.int64) + 1).sum())]
    assert token_count(out) == ntok
    return out


def no255(n: int, seed: int = 1, ntok: int = None) -> bytes:
    """random bytes without the value 255 (codes of 7 and 8 bits: the general coder on a chars stream
    as long as the input); `ntok`: cut to that many tokens"""
    data = _draw(random.Random(seed), n, range(255)).tobytes()
    return cut_tokens(data, ntok) if ntok is not None else data


def half2(n: int, seed: int = 2, ntok: int = None) -> bytes:
    """random bytes, the values 0 and 1 at half the others' weight: codes of 7, 8 and 9 bits that
    average 8, so chunks land on both sides of 65 536 bits.  (no255's source with one value at half
    weight keeps to 7 and 8 bits and below 65 536: the model says so, hence this one)"""
    data = _draw(random.Random(seed), n, range(256), [1, 1] + [2] * 254).tobytes()
    return cut_tokens(data, ntok) if ntok is not None else data


NO255_CHUNKS = 66                             # look-back over more than 64 earlier chunks
NO255_NTOK = (NO255_CHUNKS - 1) * CHUNK + 1   # the fewest tokens with that many chunks (a last chunk of 1)


def no255_small() -> bytes:
    return no255(NO255_NTOK + 4096, 2, NO255_NTOK)


def half2_small() -> bytes:
    return half2(NO255_NTOK + 4096, 2, NO255_NTOK)


def two_window(n: int, common: int, seed: int = 1, where: str = "tail") -> bytes:
    """random bytes over `common` values, and n / 8 random bytes over the other 256 - common: the
    rare values' codes are long, and a chunk of them needs a second staging window.  where =
    `tail`: the rare part last; `middle`: in the middle, so the two-window chunk has a successor"""
    rng = random.Random(seed)
    rare = n // 8
    a = _draw(rng, n - rare, range(common)).tobytes()
    b = _draw(rng, rare, range(common, 256)).tobytes()
    if where == "tail":
        return a + b
    h = len(a) // 2
    return a[:h] + b + a[h:]


# the window seam: two_window(128 KiB, 8 common values, `middle`) with only `rare` bytes of the rare
# part: the chunk that holds them grows by about 6.5 bits per byte, through the 31 bits right of
# the first window's end.  The search is bounded (8 seeds x 300 lengths, a time limit); SEAM is its
# first hit, after about 100 profiles (test_entropy_craft.py runs the search again)
SEAM_N, SEAM_COMMON = 128 * 1024, 8
SEAM_SEEDS = range(1, 9)
SEAM_RARE = range(8800, 9100)
SEAM = (1, 8901)


def window_seam(seed: int, rare: int) -> bytes:
    """window_seam(*SEAM): a chunk with a successor that ends fewer than 32 bits into its second
    staging window (profile()'s `seam`)"""
    rng = random.Random(seed)
    a = _draw(rng, SEAM_N - 16384, range(SEAM_COMMON)).tobytes()
    b = _draw(rng, 16384, range(SEAM_COMMON, 256)).tobytes()
    h = len(a) // 2
    return a[:h] + b[:rare] + a[h:]


def seam_search(limit_s: float = 60.0):
    """the first (seed, rare) of SEAM_SEEDS x SEAM_RARE whose chars stream has a seam chunk, or None"""
    import time

    t0 = time.monotonic()
    for seed in SEAM_SEEDS:
        for rare in SEAM_RARE:
            if profile(window_seam(seed, rare))["chars"]["seam"]:
                return seed, rare
            if time.monotonic() - t0 > limit_s:
                return None
    return None


def _all_literal(symbols, seed0: int, tries: int = 200) -> bytes:
    """an order of the multiset `symbols` that the oracle parses without a match: a shuffle, taken
    from the front, skipping over a symbol that would repeat a trigram (a match needs one); the
    first seed from seed0 that gets through"""
    for seed in range(seed0, seed0 + tries):
        rest = list(symbols)
        random.Random(seed).shuffle(rest)
        out, seen = [], set()
        while rest:
            for j in range(len(rest) - 1, max(-1, len(rest) - 65), -1):
                if len(out) < 2 or (out[-2], out[-1], rest[j]) not in seen:
                    break
            else:
                break
            out.append(rest.pop(j))
            if len(out) >= 3:
                seen.add(tuple(out[-3:]))
        data = bytes(out)
        if not rest and token_count(data) == len(data):
            return data
    raise AssertionError("no all-literal order in the seed range")


def exact_histogram(weights, seed: int = 0) -> bytes:
    """an all-literal input whose chars histogram is `weights` over symbols chosen by the seed"""
    syms = list(range(256))
    random.Random(1000 + seed).shuffle(syms)
    multiset = [syms[i] for i, w in enumerate(weights) for _ in range(w)]
    return _all_literal(multiset, seed)


def form_edge_weights(wmax: int):
    return [10, 10] + [11 + i % 9 for i in range(253)] + [wmax]


def form_edge(wmax: int) -> bytes:
    """256 symbols, w0 + w1 = 20 against a heaviest leaf of wmax: the closed form at 19 only"""
    return exact_histogram(form_edge_weights(wmax), wmax)


LEAF_COUNTS = (2, 3, 63, 64, 65, 66, 255, 256)
TIES = {"small": (1, 2, 3, 5, 8), "pow2": (1, 2, 4, 8, 16, 32)}


def leaf_count_weights(real: int, ties: str):
    cyc = TIES[ties][:3] if real <= 3 else TIES[ties]
    return [cyc[i % len(cyc)] for i in range(real)]


def leaf_count(real: int, ties: str) -> bytes:
    """`real` leaves with weights cycling through {1, 2, 3, 5, 8} (ties between leaves) or through
    powers of two (ties between leaves and internal nodes)"""
    return exact_histogram(leaf_count_weights(real, ties), 10 * real + len(ties))


BYTE8_R = (1, 2, 3, 4, CHUNK - 1, 0)
BYTE8_K = (1, 3)


def byte8_tail(r: int, k: int, align: int, tries: int = 40) -> bytes:
    """balanced bytes (a shuffle of every value equally often) cut to 8192 k + r tokens, with the
    chars' first code byte at `align` mod 4 in the record (sh0 = 8 align).  What precedes the chars
    is the flags stream, so the search goes over seeds and over 0 .. 7 three-byte copies planted
    near the start: each adds a flag byte of its own to that stream's tree and words"""
    ntok = CHUNK * k + r
    for seed in range(tries):
        s = list(range(256)) * (ntok // 256 + 2)
        random.Random(7919 * seed + r + k).shuffle(s)
        for plants in range(8):
            buf = bytearray(s)
            for i in range(plants):
                q = 40 + 21 * i
                buf[q:q + 3] = buf[q - 10:q - 7]
            data = cut_tokens(bytes(buf), ntok)
            pr = profile(data)
            st = pr["chars"]
            # (and the reference's decoder takes its encoder's block back: a distances stream of one
            # byte value, say, decodes as zeros)
            if st["byte8"] and st["obyte"] % 4 == align and oracle.decompress_block(pr["record"][4:], len(data)) == data:
                return data
    raise AssertionError("no seed in range")


def geometric(n: int = 256 * 1024, values: int = 30, seed: int = 4) -> bytes:
    """random bytes with p_k ~ 2^-k over `values` values"""
    return _draw(random.Random(seed), n, range(values), [1 << (values - k) for k in range(values)]).tobytes()


FIB_D = 16          # the trigram alphabet: values 0 .. 15
FIB_K = 256         # distinct trigrams: a unit's match is 4 k <= 2047 back, and 8 k is out of the window


def trigram_units(xs, k: int = FIB_K, seed: int = 5) -> bytes:
    """a preamble of k distinct trigrams over the values < 16, then the units T_(i mod k) + xs[i]
    (every xs[i] >= 16 and xs[i] != xs[i - k]): each unit parses as (match of 3, char xs[i])"""
    rng = random.Random(seed)
    tri = rng.sample(range(FIB_D ** 3), k)
    T = [bytes((t // 256, t // 16 % 16, t % 16)) for t in tri]
    assert all(x >= FIB_D for x in xs) and all(xs[i] != xs[i - k] for i in range(k, len(xs)))
    return b"".join(T) + b"".join(T[i % k] + bytes((x,)) for i, x in enumerate(xs))


def interleave(multiset_sorted, k: int):
    """the sorted multiset laid out so that out[i] != out[i - k]: the rows t = i // k of even t are
    filled first, then the odd ones, so row neighbours lie about half the multiset apart"""
    n = len(multiset_sorted)
    order = [i for i in range(n) if (i // k) % 2 == 0] + [i for i in range(n) if (i // k) % 2 == 1]
    out = [None] * n
    for j, i in enumerate(order):
        out[i] = multiset_sorted[j]
    return out


def chain_weights(fixed, budget: int):
    """unit-char weights that make the deepest tree `budget` units afford on top of the leaves
    `fixed` (the preamble's own chars, which no unit can avoid).  Equal leaves cannot chain, so the
    fixed ones are left to merge into one bush of weight B; below it a Fibonacci run 1, 1, 2, 3, ...
    lighter in all than the lightest fixed leaf (a chain that then sinks into the bush), above it the
    slowest run that still chains: each merge must take the chain c and one leaf, so the leaf after
    next is c + 1 (a leaf goes first on a tie)"""
    low, s = [], 0
    a, b = 1, 1
    while s + a < min(fixed):
        low.append(a)
        s += a
        a, b = b, a + b
    c = sum(fixed) + s            # the bush, the low chain inside it
    high = [c + 1, c + 2]
    c += high[0]
    while sum(low) + sum(high) + c + 1 <= budget:
        high.append(c + 1)
        c += high[-2]
    return low + high


def fibonacci_chars(budget: int = (MiB - 4096) // 4, k: int = FIB_K) -> bytes:
    """units whose chars make the deepest codes a block of 1 MiB affords (chain_weights over the
    chars the preamble's parse leaves in the histogram)"""
    pre = trigram_units([], k)
    fixed = np.bincount(parse_arrays(pre)[2], minlength=256)
    w = chain_weights([int(x) for x in fixed if x], budget)
    multiset = [FIB_D + i for i, x in enumerate(w) for _ in range(x)]
    return trigram_units(interleave(multiset, k), k)


def uniform_units(pcnt: int, k: int = FIB_K, seed: int = 6) -> bytes:
    """`pcnt` units with random chars: a distances stream of 11 pcnt // 8 + 1 bytes"""
    rng = random.Random(seed)
    xs = []
    for i in range(pcnt):
        x = FIB_D + rng.randrange(256 - FIB_D)
        while i >= k and x == xs[i - k]:
            x = FIB_D + rng.randrange(256 - FIB_D)
        xs.append(x)
    return trigram_units(xs, k, seed)


def few_matches(pcnt: int) -> bytes:
    """96 distinct bytes, then `pcnt` of their trigrams, each followed by a byte of its own: exactly
    pcnt matches of 3"""
    base = bytes(range(96))
    assert 3 * pcnt <= len(base)
    return base + b"".join(base[3 * i:3 * i + 3] + bytes((128 + i,)) for i in range(pcnt))


FLAG_LENGTHS = (2, 15, 16, 17, 31, 33)
# 11 pcnt // 8 + 1 skips 15, 33 and 32769: their neighbours
P_LENGTHS = {2: 1, 14: 10, 16: 11, 17: 12, 31: 22, 32: 23, 34: 24, K["kDeepBytes"] - 1: 23830, K["kDeepBytes"]: 23831,
             K["kDeepBytes"] + 2: 23832}


def stream_lengths() -> dict:
    """name -> input.  `flagsL` / `flagsL_full`: all-literal, L flag bytes of 0xFF (the last one
    partial, or full: then the flags stream has one symbol); `flagsL_rand`: random bytes cut to a
    token count that gives kDeepBytes - 1, kDeepBytes, kDeepBytes + 1 flag bytes; `pL`: units whose
    distances stream is L bytes; `ab*`: two-byte periods (0x00-heavy flags, long golomb codes)"""
    out = {}
    for L in FLAG_LENGTHS:
        out[f"flags{L}"] = _all_literal([(37 * i + 11) % 256 for i in range(8 * L - 3)], L)
        out[f"flags{L}_full"] = _all_literal([(37 * i + 11) % 256 for i in range(8 * L)], L)
    big = random.Random(11).randbytes(8 * K["kDeepBytes"] + 4096)
    for d in (-1, 0, 1):
        L = K["kDeepBytes"] + d
        out[f"flags{L}_rand"] = cut_tokens(big, 8 * L if d <= 0 else 8 * (L - 1) + 1)
    pre = int((parse_arrays(uniform_units(0))[1] > 0).sum())   # the preamble's own matches
    for L, pcnt in P_LENGTHS.items():
        assert f7.P_BITS * pcnt // 8 + 1 == L
        out[f"p{L}"] = uniform_units(pcnt - pre) if pcnt > pre else few_matches(pcnt)
    out["ab5000"] = b"ab" * 5000
    out["ab70001"] = (b"ab" * 35001)[:70001]
    return out


DEEP_RARE = 224     # values of the rare chunk (the chain above it and the low run take the other 16)


def deepest_chunk(k: int = FIB_K) -> bytes:
    """the fullest chunk a block of 1 MiB affords, as far as this file knows how: kChunk literals
    spread evenly over DEEP_RARE values (chunk 0 of the chars), then units whose chars chain above
    that bush (chain_weights).  The reachability statement about a third staging window rests on it"""
    syms = list(range(256 - DEEP_RARE, 256))
    head = _all_literal([syms[i % DEEP_RARE] for i in range(CHUNK)], 3)
    pre = trigram_units([], k)
    fixed = [int(x) for x in np.bincount(parse_arrays(pre)[2], minlength=256) if x]
    fixed += [CHUNK // DEEP_RARE + (i < CHUNK % DEEP_RARE) for i in range(DEEP_RARE)]
    w = chain_weights(fixed, (MiB - CHUNK - 4096) // 4)
    assert FIB_D + len(w) <= 256 - DEEP_RARE
    multiset = [FIB_D + i for i, x in enumerate(w) for _ in range(x)]
    return head + trigram_units(interleave(multiset, k), k)


# ---------------------------------------------------------------------------------------------
# the histogram families of the reachability sweep (test_entropy_craft.py): at most 2^20 symbols,
# at least kJacobiMin + 1 leaves (fewer never enter the fixed point)
def scaled(w, total: int = MiB):
    """w scaled down to at most `total` symbols, no leaf lost"""
    s = sum(w)
    if s <= total:
        return list(w)
    f = (total - len([x for x in w if x])) / s
    return [max(1, int(x * f)) if x else 0 for x in w]


def sweep_histograms():
    """(family, weights over 256 symbols)"""
    fib = [1, 1]
    while len(fib) < 40:
        fib.append(fib[-1] + fib[-2])
    pad = lambda w: list(w) + [0] * (256 - len(w))
    for m in range(16, 29):                       # a Fibonacci chain and equal leaves beside it
        for extra in (65 - m, 128 - m, 256 - m):
            for c in (1, 2, fib[m // 2], fib[m - 1]):
                if sum(fib[:m]) + extra * c <= MiB:
                    yield f"fib{m}+{extra}x{c}", pad(fib[:m] + [c] * extra)
    for r in (64, 100, 128, 200, 247):            # chain_weights over a bush of equal leaves
        for c in (1, 2, 5, 33, 100):
            w = chain_weights([c] * r, MiB)
            if len(w) + r <= 256:
                yield f"chain{r}x{c}", pad([c] * r + w)
    for q in (0.5, 0.55, 0.618, 0.7, 0.8, 0.9, 0.95, 0.98):   # geometric
        for n in (65, 100, 256):
            yield f"geo{q}/{n}", pad(scaled([max(1, int((MiB // 2) * q ** k)) for k in range(n)]))
    for n in (65, 256):                           # doubled Fibonacci: every weight twice (ties)
        w = sorted((fib[:n // 2] * 2 + [1] * n)[:n])
        yield f"fib2/{n}", pad(scaled(w))


def deep_codes() -> dict:
    """the deep-code inputs: name -> bytes"""
    return {"geometric": geometric(), "fibonacci": fibonacci_chars(), "deepest_chunk": deepest_chunk()}


# ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def vectors() -> dict:
    """name -> (family, block, data): every crafted input at the block size it is built for"""
    V = {}
    V["no255_66"] = ("no255", MiB, no255_small())
    V["no255_1M"] = ("no255", MiB, no255(MiB))
    V["half2_66"] = ("no255", MiB, half2_small())
    V["half2_1M"] = ("no255", MiB, half2(MiB))
    for n, common in ((128 * 1024, 8), (256 * 1024, 16)):
        for where in ("tail", "middle"):
            V[f"two_window_{n >> 10}K_{where}"] = ("two_window", MiB, two_window(n, common, 1, where))
    V["window_seam"] = ("two_window", MiB, window_seam(*SEAM))
    for wmax in (19, 20, 21):
        V[f"form_edge_{wmax}"] = ("forms", 65536, form_edge(wmax))
    for real in LEAF_COUNTS:
        for ties in TIES:
            V[f"leaves_{real}_{ties}"] = ("forms", 65536, leaf_count(real, ties))
    for k in BYTE8_K:
        for r in BYTE8_R:
            for align in (0, 1, 3) if k == 1 else (0, 1):
                V[f"byte8_k{k}_r{r}_a{align}"] = ("byte8", 65536, byte8_tail(r, k, align))
    for name, data in deep_codes().items():
        V[name] = ("deep", MiB, data)
    for name, data in stream_lengths().items():
        V["len_" + name] = ("lengths", MiB, data)
    return V


def family(name: str) -> dict:
    return {k: v for k, v in vectors().items() if v[0] == name}


TWO_BLOCKS = 128 * 1024


def two_blocks() -> bytes:
    """two blocks of 128 KiB in one shard: a two-window block (the rare part in the middle), then a
    no255 block (16 chunks through the general coder)"""
    return two_window(TWO_BLOCKS, 8, 1, "middle") + no255(TWO_BLOCKS, 3)


def one_symbol_flags(pr: dict) -> bool:
    """an all-literal block of a multiple of 8 tokens: every flag byte 0xFF, a flags stream of one
    symbol, which the reference's decoder reads as zeros (match tokens without a pair): it decodes
    to nothing.  The encoder's bytes are checked all the same"""
    return pr["pcnt"] == 0 and pr["N"] > 8 and pr["N"] % 8 == 0
