"""The crafted FCX7 corpus: one list of named payloads that test_fcx7_crafted_host.py (CPU) and
test_gpu_decode_crafted.py (GPU) both run.  Every vector carries its expected verdict, fixed by
one rule and nothing else:

  same      the oracle returns bytes and the stream is inside the decoder's stated domain: the
            decoder returns success and those bytes
  format    the oracle fails: the decoder returns FCX_ERR_FORMAT
  stricter  the oracle returns bytes, the stream is outside the GPU decoder's stated domain (the
            STRICTER table, the only conditions allowed): the GPU returns FCX_ERR_FORMAT; the host
            decoder's verdict for the same vector is stated next to it

A decoder may never return bytes that differ from the oracle's.  The oracle is not run on the
vectors marked no_oracle (N or G near 2^32: it would allocate and clear gigabytes); they are
`format` by the field bounds both decoders state.  The declared verdicts are checked against the
oracle on the CPU (test_fcx7_crafted_host.py::test_verdicts_follow_the_oracle).
"""
import random
import struct
from collections import namedtuple

import fcx7_craft as craft
import inputs
import oracle

Vector = namedtuple("Vector", "name payload verdict host tokens pcnt no_oracle extra")

# condition -> the line of fcx_dec.hip that rejects it
STRICTER = {
    "l>=258": "k_dlen: `longl = longl || l >= kMaxL` (a longer match cannot fit an LZ step)",
    "depth>32": "k_dtable: `if (pv == 0xFFFF || d >= 31)` in the walk to the root, `if (d > 32)` per leaf",
    "two-parents": "k_dtable: `if (par[k] != 0xFFFF) bad = 1;   // two parents`",
    "child-order": "k_dtable: `if (v < 256 - real || k >= x / 2)` (a child precedes its parent)",
    "orphan": "k_dtable: `if (pv == 0xFFFF || d >= 31)` (a node without a parent never reaches the root)",
    "G>bound": "k_dhead: `(uint64_t)G <= (67ull * pcnt + 31) / 32 + 1`",
    "N>2^20": "k_dhead: `N <= kMaxTokensPerBlock`",
}

CAP = (1 << 20) + 64   # every vector decodes to at most 1 MiB


def rb(n: int, seed: int) -> bytes:
    """n bytes of a skewed 256-symbol source (code lengths of about 4 to 14 bits)"""
    rng = random.Random(seed)
    return bytes(min(rng.randrange(256), rng.randrange(256), rng.randrange(256)) for _ in range(n))


def _corpus():
    V = []

    def add(name, p, verdict, host=None, tokens=None, pcnt=None, no_oracle=False, extra=None):
        assert verdict in ("same", "format") or verdict in STRICTER, verdict
        if host is None:
            assert verdict in ("same", "format"), name
            host = verdict
        assert name not in [v.name for v in V]
        V.append(Vector(name, p, verdict, host, tokens, pcnt, no_oracle, extra))

    def tok(name, tokens, verdict="same", host=None, pcnt=None, **kw):
        add(name, craft.payload(tokens, pcnt=pcnt, **kw), verdict, host, tokens, pcnt)

    L = craft.lits

    # ---- tokens the encoder never emits, and the edges of k_dlz ----
    c = iter(rb(4000, 1))
    tok("short_lens", L(rb(20, 2)) + [(1, 0, next(c)), (2, 1, next(c)), (3, 2, next(c)), (5, 3, next(c)),
                                      (7, 4, next(c)), (9, 255, next(c)), (290, 256, next(c)), (2, 257, next(c)),
                                      (1, 0, next(c)), (100, 1, next(c)), (64, 2, next(c)), (1, 257, next(c)),
                                      (1000, 0, next(c))] + L(rb(13, 3)))
    tok("l0_p1_first", [(1, 0, 65)] + L(rb(20, 4)), "format")
    tok("p2047_at_2047", L(rb(2047, 5)) + [(2047, 5, next(c))] + L(rb(10, 6)) + [(2046, 3, next(c)),
                                                                                 (2047, 257, next(c))])
    tok("p_past_start", L(rb(100, 7)) + [(101, 3, next(c))] + L(rb(9, 8)), "format")
    tok("p_zero", L(rb(100, 9)) + [(0, 3, next(c))] + L(rb(9, 10)), "format")
    tok("p1_l257_x200", [(0, None, 7)] + [(1, 257, next(c)) for _ in range(200)])
    tok("p3_l257_x3900", L(b"abc") + [(3, 257, (17 * i) & 0xFF) for i in range(3900)])
    for n in (1, 2047, 2048, 4095, 4096, 4097, 9000):
        tok(f"lit{n}_p2047_p1", L(rb(n, 20 + n)) + [(2047, 9, next(c)), (1, 7, next(c))] + L(rb(11, 11)),
            "format" if n < 2047 else "same")
    # a tile step, then a match that is the first byte of the next step, source at history index 1
    tok("tile_then_p2047", L(rb(10, 12)) + [(1, 100, next(c))] + L(rb(4085, 13)) + [(2047, 20, next(c))] +
        L(rb(5, 14)))
    # a match whose source straddles the history / tile boundary
    tok("straddle", L(rb(4096, 15)) + L(rb(10, 16)) + [(20, 40, next(c))] + L(rb(5, 17)))
    # long matches shrink the window to its floor; an all-literal window of 256 then refills the
    # history from both the old history and the chars
    tok("window_floor_fast", L(b"xyz") + [(3, 257, next(c)) for _ in range(31)] + L(rb(700, 18)) +
        [(2047, 30, next(c)), (1, 5, next(c))] + L(rb(3, 19)))
    add("n0", craft.payload([]), "format")   # (the decoder reads pcnt as the absent chars stream's header)
    add("n1", craft.payload([(0, None, 65)]), "same")   # one-symbol chars: decodes as a zero byte
    tok("n8", L(rb(3, 30)) + [(2, 3, next(c))] + L(rb(4, 31)))
    tok("n9", L(rb(3, 32)) + [(2, 3, next(c))] + L(rb(5, 33)))
    tok("n16", L(rb(7, 34)) + [(5, 4, next(c))] + L(rb(8, 35)))
    tok("n17", L(rb(7, 36)) + [(5, 4, next(c))] + L(rb(9, 37)))
    t13 = L(rb(5, 38)) + [(3, 3, next(c)), (1, 0, next(c))] + L(rb(6, 39))
    tok("tail_ones_n13", t13, flag_tail_bits=1)
    tok("tail_zeros_n13", t13, flag_tail_bits=0)

    # ---- early stop ----
    rng = random.Random(40)
    E = L(rb(30, 41))
    for i in range(20):
        E += [(rng.randrange(1, 30), rng.choice([0, 1, 3, 17, 257]), next(c))] + L(rb(rng.randrange(0, 12), 42 + i))
    E += L(rb(9 - len(E) % 8, 70))   # N % 8 == 1: seven unused flag bits
    assert len(E) % 8 == 1
    nm = sum(1 for _, l, _ in E if l is not None)
    tok("pcnt_short_by_1", E, pcnt=nm - 1)
    tok("pcnt_short_by_all", E, pcnt=0)
    tok("stop_at_token_0", [(1, 3, next(c))] + L(rb(20, 71)), pcnt=0)
    tok("stop_at_token_4096", L(rb(4096, 72)) + [(5, 3, next(c))] + L(rb(20, 73)), pcnt=0)
    tok("stop_at_last_token", E + [(4, 6, next(c))], pcnt=nm)
    # more pairs than match flags (at least as many as the unused flag bits): the surplus is ignored
    tok("surplus_pairs", E, extra_pairs=[(5, 3), (1, 257), (2047, 0), (9, 9), (1, 1), (2, 200), (3, 30), (4, 4)])
    A = L(rb(50, 74))
    tok("pcnt0_g0", A)
    tok("pcnt0_g1_garbage", A, golomb_stream=oracle.huffman_stream(b"\xde\xad\xbe\xef"), G=1)
    add("pcnt0_g2", craft.payload(A, golomb_stream=oracle.huffman_stream(b"\xde\xad\xbe\xef\x01\x02\x03\x04"), G=2),
        "G>bound", host="format")

    # ---- exhausted streams: W cut with the words really removed ----
    text = inputs.generate("text", 31, 6000)
    good = craft.payload(craft.tokens_of(oracle.parse(text)))
    f = craft.fields(good)
    assert all(f[n]["ts"] > 0 and f[n]["W"] >= 4 for n in ("flags", "chars", "P", "golomb"))
    add("good_text", good, "same")
    # the symbols the words run out of are 0: chars turn to zeros, flags to match flags, distances
    # to p = 0; zero golomb bytes are codes of l = 0 (three zero bits each), so values never run out
    # (a cut golomb stream decodes: shorter matches, until a distance reaches before the start)
    expect = {"flags_half": "same", "flags_zero": "format", "chars_half": "same", "chars_zero": "same",
              "P_half": "format", "P_zero": "format", "golomb_half": "same", "golomb_zero": "format"}
    for name in ("flags", "chars", "P", "golomb"):
        for tag, W in (("half", f[name]["W"] // 2), ("zero", 0)):
            add(f"exhausted_{name}_{tag}", craft.rebuild(craft.cut_words(f, name, W)), expect[f"{name}_{tag}"])
        s = f[name]
        add(f"cut_in_{name}_header", good[:craft.sub_offset(f, name) + 1 + len(s["bitmap"])], "format")

    # ---- trees (chars stream) ----
    def tree_vec(name, children, codes, data, verdict="same", host=None, nwords=None, matches=True, model=True):
        toks = L(data)
        if matches:   # two matches among the literals (the chars stream still holds every token's char)
            toks[40] = (7, 3, data[40])
            toks[90] = (33, 0, data[90])
        cs = craft.huff_stream(children, codes, data, nwords)
        add(name, craft.payload(toks, chars_stream=cs), verdict, host, toks if model else None, None,
            False, {"children": children, "chars_words": cs[len(craft.tree_header(children)) + 4:]})

    perm = list(range(256))
    random.Random(50).shuffle(perm)
    for ts in (2, 10, 11, 31, 32, 33, 40):
        syms = perm[:ts + 1]
        rng = random.Random(51 + ts)
        # the deepest and the shallowest leaves, and a geometric mix of the rest
        data = bytes([syms[ts], syms[0], syms[ts - 1], syms[ts]] +
                     [syms[min(ts, int(rng.expovariate(0.25)))] for _ in range(195)] + [syms[ts], syms[0], syms[ts]])
        assert len(data) % 8 != 0
        ch, cd = craft.chain_tree(ts, syms)
        tree_vec(f"chain_ts{ts}", ch, cd, data, "same" if ts <= 32 else "depth>32", "same")
    syms = perm[:6]
    ch, cd = craft.chain_tree(5, syms)
    data = bytes(syms[i % 6] for i in range(203))
    two = list(ch)
    two[3] = (ch[3][0], 256 + 1)        # node 1 gets a second parent, node 2 none
    tree_vec("tree_two_parents", two, cd, data, "two-parents", "same", matches=False, model=False)
    selfc = list(ch)
    selfc[3] = (ch[3][0], 256 + 3)      # node 3 is its own right child
    tree_vec("tree_self_child", selfc, cd, data, "child-order", "same", matches=False, model=False)
    below = craft.payload(L(data), chars_stream=craft.huff_stream(ch, cd, data))
    fb = craft.fields(below)
    assert fb["chars"]["pairs"][2 * 4 + 1] == (256 - 6) + 3   # the root's right child: node 3
    fb["chars"]["pairs"][2 * 4 + 1] = 0                     # an internal child below 256 - real
    add("tree_child_below_base", craft.rebuild(fb), "format")
    # a complete depth-8 tree: k_dsyms' byte substitution, with words for exactly, fewer and more
    # symbols than the stream's count
    ch8, cd8 = craft.full_tree8(perm)
    data = rb(1003, 60)
    tree_vec("bytes8_exact", ch8, cd8, data)
    tree_vec("bytes8_words_short", ch8, cd8, data, nwords=125, matches=False, model=False)
    tree_vec("bytes8_words_long", ch8, cd8, data, nwords=300)

    # ---- segment decoder paths (claims checked with craft.settle_rounds) ----
    syms = perm[:32]
    ch31, cd31 = craft.chain_tree(31, syms)
    for name, run, reps in (("fallback", 3500, 2), ("retry", 300, 8)):
        toks = []
        for r in range(reps):
            toks += L(bytes([syms[31]]) * run) + L(bytes(syms[(3 * r + i) % 31] for i in range(7)))
            toks += [(run // 2 + r, 5 + r, syms[(r + 1) % 31])]   # (varied: a one-symbol sub-stream decodes as zeros)
        cs = craft.huff_stream(ch31, cd31, bytes(t[2] for t in toks))
        add(name, craft.payload(toks, chars_stream=cs), "same", None, toks, None, False,
            {"ts": 31, "chars_words": cs[len(craft.tree_header(ch31)) + 4:], "claim": name})
    tok("golomb_all_257", L(rb(5, 61)) + [(1 + i % 5, 257, next(c)) for i in range(300)])
    tok("golomb_all_3", L(rb(10, 62)) + [(1 + i % 9, 3, next(c)) for i in range(300)])
    tok("golomb_r1_r2", L(rb(10, 63)) + [(1 + i % 9, (5, 6, 9, 10, 1, 2, 253, 254)[i % 8], next(c)) for i in range(200)])
    g1 = [(0xFF, 0x00)]
    add("golomb_all_ones", craft.payload(L(rb(10, 64)) + [(2, 3, next(c)) for _ in range(10)],
                                         golomb_stream=craft.huff_stream(g1, craft.tree_codes(g1), b"\xff" * 8), G=2),
        "format")

    # ---- lengths outside the GPU decoder's domain ----
    small = [(1 + i % 7, 3, next(c)) for i in range(50)]
    tok("l258", L(rb(300, 65)) + small[:5] + [(9, 258, next(c)), (2, 257, next(c))], "l>=258", "same")
    tok("l1200", L(rb(300, 66)) + small + [(1, 1200, next(c))] + L(rb(4, 67)), "l>=258", "same")
    tok("l1200_alone", L(rb(300, 68)) + [(1, 1200, next(c))], "G>bound", "format")

    # ---- hostile header fields: one field of good_text changed ----
    for tag, n in (("2p20_plus_1", (1 << 20) + 1), ("fffffff8", 0xFFFFFFF8), ("ffffffff", 0xFFFFFFFF)):
        add(f"hostile_N_{tag}", struct.pack("<I", n) + good[4:], "format", no_oracle=True)
    g = dict(f)
    g["pcnt"] = f["N"] + 1
    add("hostile_pcnt_N_plus_1", craft.rebuild(g), "format")
    g = dict(f)
    g["G"] = 0xFFFFFFFF
    add("hostile_G_ffffffff", craft.rebuild(g), "format", no_oracle=True)
    for name in ("flags", "chars", "P", "golomb"):
        g = dict(f)
        g[name] = dict(f[name], W=0x40000001)
        add(f"hostile_W_{name}", craft.rebuild(g), "format")
    return V


_cache = {}


def corpus():
    if "v" not in _cache:
        _cache["v"] = _corpus()
    return _cache["v"]


def by_name(name):
    return next(v for v in corpus() if v.name == name)


def want(v):
    """the oracle's bytes of a vector (None: it fails, or is not to be run), computed once"""
    if v.name not in _cache:
        _cache[v.name] = None if v.no_oracle else oracle.decompress_block(v.payload, CAP)
    return _cache[v.name]


def record_vectors():
    """hostile framing, for the entries that take records: (name, records, count); all `format`"""
    good = craft.record(by_name("good_text").payload)
    longer = struct.pack("<I", len(good) - 4 + 1) + good[4:]
    return [("record_length_plus_1", good + longer, 2), ("nblocks_plus_1", good + good, 3)]
