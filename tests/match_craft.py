"""Builders of adversarial inputs for the match search, and CPU predicates over them (no GPU here).

Every builder aims at one place where the search decides something (fcx_match.hip, fcx_device.h,
fcx_parse.hip): the per-query extension budget (kExtBudget = 24, counted through pass A and pass B
of the bucket scan), the skip rule for a candidate right of the best, the slab bounds of a query's
bucket range, the 4-byte-key unit's 3-byte fallback (kNeed3), and the run tables' budgets
(kRunBudget = 512 runs per window, kRunTile = 1024 image runs, kStRunCap = 1020 in the stitch).
tests/test_match_craft.py pins on the CPU, with the oracle, that each input reaches its place;
tests/test_gpu_match_edges.py runs them through every match unit.

Seeds go through inputs.generate / inputs._lcg and random.Random(seed).randrange only.
"""
import random

import numpy as np

import inputs
import oracle

TILE, HALO, WIN, MAXL = 4096, 2048, 2047, 258
SLAB = 512            # positions per insertion pass of the bucket sort
STRIDE = 56           # staircase: bytes from one copy to the next (36 copies inside the window)
EXT_BUDGET = 24       # kExtBudget
RUN_BUDGET, RUN_TILE, ST_RUN_CAP = 512, 1024, 1020


# ---- planted copies (moved from test_gpu_sparse_filter.py) ----
def plant(buf: bytearray, p: int, d: int, length: int) -> bool:
    """copy `length` bytes from p - d to p, byte by byte (d < length gives a period-d run)"""
    if p - d < 0 or p < 0 or p + length > len(buf):
        return False
    for i in range(length):
        buf[p + i] = buf[p - d + i]
    return True


def geometry(n: int, block: int):
    """block ranges and the tile starts inside blocks (not the block starts themselves)"""
    blocks = [(bs, min(bs + block, n)) for bs in range(0, n, block)]
    tiles = [bs + t for bs, be in blocks for t in range(TILE, be - bs, TILE)]
    return blocks, tiles


def planted_input(seed: int, ntiles: int, block: int, length: int, d: int) -> bytes:
    n = ntiles * TILE
    buf = bytearray(inputs.generate("rand", seed, n))
    blocks, tiles = geometry(n, block)
    pick = lambda lst, i: lst[i % len(lst)]
    b_last, b_mid = blocks[-1], blocks[len(blocks) // 2]
    plant(buf, pick(tiles, 0), d, length)                    # on a tile start: the candidate in the halo
    plant(buf, pick(tiles, 1) - 1, d, length)                # one position before a tile start
    plant(buf, pick(tiles, 2) - 1 + d, d, length)            # the source straddles a tile boundary
    plant(buf, b_mid[0], d, length)                          # block position 0 (nothing may cross blocks)
    plant(buf, b_last[0] + 1, d, length)                     # block position 1
    plant(buf, 1, d, length)                                 # ... of the first block (d = 1 only)
    plant(buf, b_last[1] - length, d, length)                # ending at the block's end
    plant(buf, b_mid[1] - 3, d, 3)                           # fewer than 4 bytes left in the block
    return bytes(buf)


# ---- slab-edge plants: the counter snapshots that bound a query's bucket range ----
SLAB_LENGTHS = (3, 12, 258)
SLAB_DISTANCES = (2046, 2047, 2048)
SLAB_DELTAS = (-1, 0, 1)


def slab_edge_input(seed: int, block: int, length: int, d: int, delta: int, ntiles: int = 4) -> bytes:
    """planted_input's scheme (rand bytes, chunks copied from p - d to p) with the copies of one tile
    at the offsets 512 k + delta, k = 1..7: the query's first or last position of an insertion slab,
    its candidate at the window's far edge, five slabs back.  The plants go in position order, so
    a later one whose source lies in an earlier one copies the finished bytes."""
    n = ntiles * TILE
    buf = bytearray(inputs.generate("rand", seed, n))
    tiles = geometry(n, block)[1]
    t0 = tiles[1 % len(tiles)]
    for k in range(1, 8):
        plant(buf, t0 + SLAB * k + delta, d, length)
    return bytes(buf)


# ---- preconditions from the oracle ----
def token_map(data: bytes, block: int = 65536) -> dict:
    """token start -> (distance, length) of the oracle's greedy parse (length 0: a literal)"""
    out = {}
    for bs in range(0, len(data), block):
        pos = bs
        for p, l, _c in oracle.parse(data[bs:bs + block]):
            out[pos] = (p, l)
            pos += l + 1
    return out


# ---- extension budget and skip rule: K copies of a stem's prefix, 56 bytes apart ----
ORDERS = ("up", "down", "flat")
STAIR_KS = (23, 24, 25, 36)
STAIR_QS = (TILE + 2100, 2 * TILE + 3, 2 * TILE + SLAB - 1, 2 * TILE + SLAB)
FLAT_LEN = 17


def stair_len(order: str, K: int, k: int) -> int:
    return {"up": 12 + k, "down": 12 + K - 1 - k, "flat": FLAT_LEN}[order]


def stair_token(order: str, K: int):
    """the oracle's (distance, length) at q"""
    return {"up": (STRIDE, 12 + K - 1), "down": (STRIDE * K, 12 + K - 1), "flat": (STRIDE * K, FLAT_LEN)}[order]


def _guard(buf: bytearray, p: int, site: int) -> None:
    """four bytes >= 0x80 before p that occur at no other site: no match reaches p from the left"""
    buf[p - 4:p] = bytes((0x80 + site, 0xA8 + site, 0xD0 + site, 0x80 + site))


def _stairs(buf: bytearray, rng, q: int, K: int, order: str, head: bytes, guards: bool) -> None:
    """the stem (`head` + random bytes) at q and its K copies at q - 56 (K - k), in place"""
    assert 1 <= K <= 36 and q - STRIDE * K >= 4 and q + 12 + K + 1 <= len(buf)
    stem = bytearray(head) + bytearray(rng.randrange(256) for _ in range(12 + K - len(head)))
    buf[q:q + len(stem)] = stem
    if guards:
        _guard(buf, q, K)
    for k in range(K):
        c, ln = q - STRIDE * (K - k), stair_len(order, K, k)
        buf[c:c + ln] = stem[:ln]
        buf[c + ln] = (stem[ln] + 1 + rng.randrange(255)) & 0xFF       # the copy ends here
        if guards:
            _guard(buf, c, k)
        elif buf[c - 1] == buf[q - 1]:                                  # ... and does not start earlier
            buf[c - 1] = (buf[q - 1] + 1 + rng.randrange(255)) & 0xFF


def staircase(seed: int, K: int, order: str, q: int, filler: str = "rand") -> bytes:
    """three tiles of filler; a random stem at q and K copies of its prefixes at q - 56 (K - k),
    k = 0 .. K-1, of length 12 + k (`up`: oldest shortest, in arrival order every candidate needs an
    extension), 12 + K-1 - k (`down`: oldest longest, every later one can be skipped) or 17 (`flat`:
    the leftmost wins).  The byte after a copy differs from the stem's; the byte before it differs
    from the byte before q; in text, four guard bytes before q and every copy make q a token start."""
    buf = bytearray(inputs.generate(filler, seed, 3 * TILE))
    _stairs(buf, random.Random(seed), q, K, order, b"", filler != "rand")
    return bytes(buf)


def stair_seed(K: int) -> int:
    """the staircases' seed (tests/test_match_craft.py checks every case of it on the CPU)"""
    return 1 + K


def stair_copies(q: int, K: int):
    return [q - STRIDE * (K - k) for k in range(K)]


def extensions_in_order(data: bytes, q: int, cands) -> int:
    """scan_candidate's rule over the candidates of q in the given arrival order: the long
    extensions a query spends (a candidate of >= 12 bytes extends unless it lies right of a best of
    >= 12 bytes and its byte at the best length differs from the query's; the cap is far here)"""
    best_len, best_pos, spent = 0, None, 0
    for j in cands:
        if data[j:j + 12] != data[q:q + 12]:
            continue
        if best_len >= 12 and j > best_pos and data[j + best_len] != data[q + best_len]:
            continue
        spent += 1
        ln = 12
        while ln < MAXL - 1 and data[j + ln] == data[q + ln]:
            ln += 1
        if ln > best_len or (ln == best_len and j < best_pos):
            best_len, best_pos = ln, j
    return spent


def window_repeats(data: bytes, q: int) -> int:
    """positions of the staged window of q's tile, [t0 - 2048, t0 + 4096), whose 3-byte key occurred
    earlier in it (first block): a lower bound of the keys the sparse unit's filter flags there,
    whatever the order its atomics run in (fcx_sparse_filter.h: of equal keys at most one is not
    flagged)"""
    t0 = q - q % TILE
    lo, hi = max(0, t0 - HALO), min(len(data) - 2, t0 + TILE)
    seen, rep = set(), 0
    for x in range(lo, hi):
        key = data[x:x + 3]
        rep += key in seen
        seen.add(key)
    return rep


SF_FLAG_CAP = 64      # kSfFlagCap: flagged keys per window up to which the sparse unit keeps a tile


def cut_by_block(data: bytes, block: int, at: int, seed: int, kind: str = "rand") -> bytes:
    """`data` behind a lead of `kind` bytes that puts its position `at` on a block start: the
    candidates left of `at` fall out of the window, and the last tile of every block is ragged"""
    assert 0 <= at < block
    return inputs.generate(kind, seed, block - at) + data


# ---- hot keys: one key ~68 times per window, every other bucket range ~1 entry ----
MARKER4, MARKER3 = b"#k:=", b"#k:"
HOT_Q = TILE + 2384            # the planted variants' query marker (a multiple of 30)
HOT_OLD, HOT_RECENT = 1980, 60
HOT_CONT = 14
HOT_VARIANTS = ("equal", "recent_longer", "old_longer")


def hot_winner(variant: str, marker: bytes):
    """the oracle's (distance, length) at HOT_Q"""
    return (HOT_RECENT if variant == "recent_longer" else HOT_OLD, len(marker) + HOT_CONT)


def hot_key(seed: int, marker: bytes, every: int = 30, variant=None, stairs=None) -> bytes:
    """three tiles of rand with `marker` every `every` bytes: the marker queries are their wave's hot
    queries (pass B of the bucket scan) and the oracle's match is the leftmost of ~68 equal
    candidates, at the window's far edge.  `variant`: a 14-byte continuation after the marker at
    HOT_Q, copied after an old marker (1980 back) and a recent one (60 back) -- `equal`: both whole
    (the old one wins); `recent_longer`: the old one a byte short; `old_longer`: the recent one a
    byte short.  `stairs` = (K, order): a staircase on HOT_Q whose stem starts with the marker, so
    its K long candidates sit among the ~68 short ones of the same bucket range."""
    n = 3 * TILE
    buf = bytearray(inputs.generate("rand", seed, n))
    for p in range(every, n - len(marker), every):
        buf[p:p + len(marker)] = marker
    rng = random.Random(seed)
    m = len(marker)
    assert HOT_Q % every == 0 and HOT_OLD % every == 0 and HOT_RECENT % every == 0
    if variant is not None:
        cont = bytes(rng.randrange(256) for _ in range(HOT_CONT + 1))
        buf[HOT_Q + m:HOT_Q + m + HOT_CONT + 1] = cont
        short = {"equal": (), "recent_longer": (HOT_OLD,), "old_longer": (HOT_RECENT,)}[variant]
        for d in (HOT_OLD, HOT_RECENT):
            ln = HOT_CONT - (d in short)
            buf[HOT_Q - d + m:HOT_Q - d + m + ln] = cont[:ln]
            buf[HOT_Q - d + m + ln] = (cont[ln] + 1 + rng.randrange(255)) & 0xFF
    if stairs is not None:
        _stairs(buf, rng, HOT_Q, stairs[0], stairs[1], marker, False)
    return bytes(buf)


def marker_sites(data: bytes, marker: bytes, every: int = 30):
    return [p for p in range(every, len(data) - len(marker), every) if data[p:p + len(marker)] == marker]


# ---- run tables ----
def run_ramp(seed: int, ntiles: int = 8, lo: int = 1, hi: int = 14, alphabet: bytes = b"abc") -> bytes:
    """runs whose mean length grows linearly from `lo` to `hi` over the buffer (a run at position p
    of mean m is 1 .. 2 m - 1 bytes long); a run's byte is never the previous run's.  Neighbouring
    positions fall on both sides of every run budget somewhere along the ramp."""
    n = ntiles * TILE
    r = inputs._lcg(seed)
    out = bytearray()
    prev = None
    while len(out) < n:
        mean = lo + (hi - lo) * len(out) / n
        ln = 1 + (next(r) >> 8) % max(1, int(2 * mean - 1 + 0.5))
        byte = alphabet[(next(r) >> 8) % len(alphabet)]
        if byte == prev:
            byte = alphabet[(alphabet.index(byte) + 1 + (next(r) >> 8) % (len(alphabet) - 1)) % len(alphabet)]
        out += bytes([byte]) * ln
        prev = byte
    return bytes(out[:n])


RUN_PATTERNS = {
    "a4b4": b"aaaabbbb",                    # window runs peak at exactly 512
    "a4b3": b"aaaabbb",                     # 585
    "a5b3c4": b"aaaaabbbcccc",              # ext walks several equal runs up to the cap
    "a3b5c2a3b4d": b"aaabbbbbccaaabbbbd",   # a near-repeat: ext ends on a length mismatch
    "a8b8": b"aaaaaaaabbbbbbbb",            # 256 runs per window, 800 per image: inside every budget
}
RUN_PERIOD_N = 5 * TILE + 123
RUN_PERIOD_LEAD = 1500


def run_periods() -> dict:
    """name -> bytes: each pattern cut at 5 tiles + 123 (the block end and the sentinel are met with
    a shrinking cap), and again behind 1500 bytes of another value (`z_` names: the windows of the
    first 2047 positions begin inside that run, so their first run is clipped)"""
    out = {}
    for name, pat in RUN_PATTERNS.items():
        body = (pat * (RUN_PERIOD_N // len(pat) + 1))[:RUN_PERIOD_N]
        out[name] = body
        out["z_" + name] = b"z" * RUN_PERIOD_LEAD + body
    return out


# ---- predicates: plain counts over the bytes ----
def _starts(data: bytes) -> np.ndarray:
    """prefix sums S with S[i] = number of run starts in data[1 .. i] (a change of byte value)"""
    a = np.frombuffer(data, dtype=np.uint8)
    s = np.zeros(len(a), dtype=np.int64)
    if len(a) > 1:
        s[1:] = np.cumsum(a[1:] != a[:-1])
    return s


def _runs(S: np.ndarray, lo, hi):
    """runs of data[lo .. hi] inclusive (lo <= hi; arrays or scalars)"""
    return 1 + S[hi] - S[lo]


def window_runs(data: bytes, block: int) -> np.ndarray:
    """for each position x: the runs of its window [max(block start, x - 2047), x] left of x's own
    run -- the candidates' runs, the count that run_match and run_match_wave hold against
    kRunBudget (the window's runs, the own one included, are one more)"""
    S = _starts(data)
    x = np.arange(len(data), dtype=np.int64)
    return _runs(S, np.maximum(x - x % block, x - WIN), x) - 1


def image_runs(data: bytes, block: int) -> list:
    """per tile: the runs of its staged image [t0 - 2048, t0 + 4096 + 260) clipped to the block"""
    S = _starts(data)
    out = []
    for bs in range(0, len(data), block):
        be = min(bs + block, len(data))
        for t0 in range(bs, be, TILE):
            out.append(int(_runs(S, max(bs, t0 - HALO), min(be, t0 + TILE + 260) - 1)))
    return out


def stitch_runs(data: bytes, block: int) -> np.ndarray:
    """for each position t: the runs of [t - 2047, t + 258) clipped to the block (the stitch's table
    holds them and a sentinel)"""
    S = _starts(data)
    t = np.arange(len(data), dtype=np.int64)
    bs = t - t % block
    be = np.minimum(bs + block, len(data))
    return _runs(S, np.maximum(bs, t - WIN), np.minimum(be, t + MAXL) - 1)
