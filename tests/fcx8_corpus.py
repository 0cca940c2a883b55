"""The crafted FCX8 corpus: one list of named payloads that test_fcx8_crafted_host.py (CPU) and
test_gpu_lz78_decode_crafted.py (GPU) both run.  Every vector carries its expected verdict, fixed by
one rule and nothing else:

  same      the oracle returns bytes and the stream is inside the decoder's stated domain: the
            decoder returns success and those bytes
  format    the oracle fails: the decoder returns FCX_ERR_FORMAT
  a key of STRICTER
            the oracle returns bytes, the stream is outside the GPU decoder's stated domain (the
            STRICTER table, the only conditions allowed): the GPU returns FCX_ERR_FORMAT

A decoder may never return bytes that differ from the oracle's.  The oracle (and the GPU) get
CAP = 2 MiB + 64 for every vector, so that a short capacity is in no verdict.  The oracle is not run
on the vectors marked no_oracle (wcnt, G or N near 2^32: it sizes buffers by wcnt and N before it
looks at the record length); they are `format` by the field bounds the decoder states.  The declared
verdicts are checked against the oracle on the CPU (test_fcx8_crafted_host.py).

Next to every vector that is not `same` stands the line of fcx_lz78_dec.hip that stops it before an
index derived from it is used ("stop:").  There is no host FCX8 decoder: one verdict column.
"""
import random
import struct
from collections import namedtuple

import numpy as np

import fcx8_craft as craft
import oracle
from fcx7_corpus import rb
from fcx7_craft import _sub, _unsub

Vector = namedtuple("Vector", "name payload verdict tokens no_oracle extra")

K = craft.kernel_constants()
CAPB, GMAX, LONG, TBL = K["kCapBlock"], K["kGmax"], K["kLong"], K["kDTblBits"]

# condition -> (kernel, the line of fcx_lz78_dec.hip that rejects it, why the decoder may)
STRICTER = {
    "wcnt>cap+2": ("k78d_head", "ok = ok && wcnt != 0 && wcnt <= kCapBlock + 2;",
                   "a block of <= kCapBlock tokens uses at most that many indices (scratch is sized by wcnt)"),
    "G>kGmax": ("k78d_head", "if (G > kGmax || !room(8ull * (G - 1) + 8)) ok = false;",
                "a <= 1 MiB block has at most kGmax groups of 256 ranks (the tree lives in shared memory)"),
    "N>cap": ("k78d_head", "if (ok && (N > kCapBlock || !room(N))) ok = false;",
              "every token decodes to at least one byte: the block would pass the reference's buffer"),
    "size>cap": ("k78d_links", "bad = __syncthreads_or(deep || run > kCapBlock);   // decoded size past the reference's buffer",
                 "the decoded size is tested before the tail-zero rule takes a byte off"),
    "depth>32": ("k78d_gtable", "if (pv == kNone || d >= 31) { bad = 1; break; }",
                 "a node more than 31 steps below the root: a group code of more than 32 bits"),
    "orphan": ("k78d_gtable", "if (pv == kNone || d >= 31) { bad = 1; break; }",
               "a node without a parent never reaches the root, whether a code walks there or not"),
    "two-parents": ("k78d_gtable", "!= kNone) bad = 1;   // two parents",
                    "the links are no tree, whether a code walks there or not"),
    "root-child": ("k78d_gtable", "if (tid == 0 && par[root] != kNone) bad = 1;   // the root is nobody's child",
                   "a cycle through the root"),
    "child>=2G-1": ("k78d_gtable", "if (k >= nodes) { bad = 1; v = 0; }",
                    "a child id past the nodes is rejected where it stands, not where a code walks"),
    "char-tree": ("lz78_decompress_shard_at", "dec_launch_tables8(d_in, nds, S->ds, S->ctbl, S->cchild, err, badq, st);",
                  "the char trees go through the FCX7 decoder's k_dtable: its stricter conditions hold here too"),
}

CAP = (2 << 20) + 64

# every reject condition of the k78d_* kernels (as written in fcx_lz78_dec.hip) -> the vectors that
# reach it; "record:" names are record_vectors().  test_fcx8_crafted_host.py checks the lines and names.
REJECTS = {
    "if (off + 4 > in_len || ld_u32le(in, off) > in_len - off - 4)": ["record:record_length_plus_1", "record:nblocks_plus_1"],
    "bool ok = len >= 4;": ["record:record_of_0", "record:record_of_3"],
    "ok = ok && wcnt != 0 && wcnt <= kCapBlock + 2;": ["wcnt_0", "wcnt_cap_plus3", "wcnt_ffffffff"],
    "ok = found;": ["wcnt_plus1_bare", "record:record_of_4"],
    "if (room(4)) {": ["wcnt_bit_in_last_byte"],
    "if (G > kGmax || !room(8ull * (G - 1) + 8)) ok = false;": ["G_kGmax_plus1", "G_ffffffff", "cut_in_tree"],
    "if (room(4ull * W)) {": ["W_40000001"],
    "} else if (room(4)) {": ["cut_before_N"],
    "if (ok && (N > kCapBlock || !room(N))) ok = false;": ["N_cap_plus1", "N_fffffff8", "N_ffffffff", "N_past_record"],
    "if (room(1)) {": ["N_0_no_chars"],
    "if (room((uint64_t)hdr + 4)) {": ["cut_in_char_bitmap", "cut_in_char_pairs", "cut_before_nw"],
    "if (room((uint64_t)hdr + 4 + 4ull * nw)) {": ["nw_40000001"],
    "if (k >= nodes) { bad = 1; v = 0; }": ["tree_child_2G_minus_1", "tree_child_ffffffff", "tree_child_2G_minus_1_walked"],
    "!= kNone) bad = 1;   // two parents": ["tree_two_parents", "tree_lc_eq_rc_nodes", "tree_self_child"],
    "if (tid == 0 && par[root] != kNone) bad = 1;   // the root is nobody's child": ["tree_root_child"],
    "if (pv == kNone || d >= 31) { bad = 1; break; }": ["tree_orphan", "chain_G34"],
    "if (r >= R.wcnt) bad = true;": ["r_eq_wcnt", "r_far_past"],
    "if (ix > t) { bad = true; ix = 0; }": ["ix_eq_t_plus1", "forward_ref_late", "index_past_N"],
    "deep = deep || n > kMaxDepth;": ["chain_past_kMaxDepth"],
    "bad = __syncthreads_or(deep || run > kCapBlock);": ["chain_1448", "size_cap_plus1", "size_cap_plus1_tail0"],
    "if (o > cap) atomicOr(err, kDErrOutCap);": [],   # test_gpu_lz78_decode_crafted.py::test_capacity_exact_and_one_short
    "dec_launch_tables8(d_in, nds, S->ds, S->ctbl, S->cchild, err, badq, st);": ["char_two_parents", "char_child_below_base"],
}


def rand_tokens(n: int, seed: int, roots: float = 0.1):
    """n tokens with parents drawn from all earlier entries (phrases of about ln n bytes)"""
    rng = random.Random(seed)
    cs = rb(n, seed + 1000)
    return [(0 if rng.random() < roots else rng.randrange(0, t + 1), cs[t]) for t in range(n)]


def chain(d: int, seed: int = 0):
    """token t has idx = t: a parent chain of depth d, d (d + 1) / 2 bytes"""
    return [(t, 1 + (t * 7 + seed) % 250) for t in range(d)]


def roots(n: int):
    return list(zip(bytes(n), (b"abcdefghijk" * (n // 11 + 1))[:n]))


def sized(total: int, last_char: int):
    """tokens that decode to `total` bytes without a deep chain: a chain of 300, then phrases of 301"""
    k, rem = divmod(total - 300 * 301 // 2, 301)
    t = chain(300) + [(300, 1 + i % 200) for i in range(k)]
    if rem:
        t.append((rem - 1, 7))
    t[-1] = (t[-1][0], last_char)
    return t


def _corpus():
    V = []

    def add(name, p, verdict, tokens=None, no_oracle=False, extra=None):
        assert verdict in ("same", "format") or verdict in STRICTER, verdict
        assert name not in [v.name for v in V], name
        V.append(Vector(name, p, verdict, tokens, no_oracle, extra))

    def tok(name, tokens, verdict="same", extra=None, **kw):
        """a vector of tokens and nothing else (extra_used is no override: the tokens mean the same)"""
        assert set(kw) <= {"extra_used"}
        add(name, craft.payload(tokens, **kw), verdict, tokens, False, extra)

    u32 = lambda v: struct.pack("<I", v)   # noqa: E731
    T40, T300, T3000 = rand_tokens(40, 1), rand_tokens(300, 2), rand_tokens(3000, 3)
    good = craft.payload(T3000)
    f = craft.fields(good)
    o = craft.parse(good)
    assert f["G"] >= 6 and f["chars"]["ts"] >= 5 and f["W"] >= 4
    tok("good", T3000)
    small = craft.payload(T40)
    assert craft.fields(small)["G"] == 1

    # ---- header (k78d_head): one field of a good payload changed ----
    # stop: `ok = ok && wcnt != 0 && wcnt <= kCapBlock + 2;`
    add("wcnt_0", u32(0) + good[4:], "format")
    # stop: `ok = found;` (the popcount scan ends at the record's end without the wcnt-th bit)
    add("wcnt_plus1_bare", u32(f["wcnt"] + 1) + f["bitmap"], "format")
    # (the scan runs on into G and the tree, whose bytes then are the bitmap's tail: both decoders
    # read the same shifted fields; stop: the `room()` of a field that no longer fits)
    add("wcnt_plus1_good", u32(f["wcnt"] + 1) + good[4:], "format")
    add("wcnt_ffffffff", u32(0xFFFFFFFF) + good[4:], "format", no_oracle=True)   # stop: as wcnt_0
    abc = [(0, 65), (1, 66), (2, 67)]
    tok("wcnt_cap_plus2", abc, extra_used=np.arange(CAPB + 2))
    tok("wcnt_cap_plus3", abc, "wcnt>cap+2", extra_used=np.arange(CAPB + 3))
    # stop: `if (room(4))` before G is read
    add("wcnt_bit_in_last_byte", u32(f["wcnt"]) + f["bitmap"], "format")
    for B in (15, 16, 4095, 4096, 4097):   # lane and piece boundaries of k78d_head's popcount scan
        tok(f"wcnt_bit_in_byte_{B}", T40, extra_used=(8 * (B // 2) + 1, 8 * B + 5))
    add("G_0", craft.payload(T40, G=0), "same")
    tok("G_1", T40)
    t600 = rand_tokens(600, 4)
    assert craft.fields(craft.payload(t600))["G"] == 2
    tok("G_2", t600)
    add("G_kGmax", craft.payload(T40, G=GMAX), "same")
    add("G_kGmax_plus1", craft.payload(T40, G=GMAX + 1), "G>kGmax")
    g = dict(f, G=0xFFFFFFFF)
    add("G_ffffffff", craft.rebuild(g), "format", no_oracle=True)   # stop: `if (G > kGmax || ...`
    add("G_more_than_wcnt", craft.payload(T40, G=3), "same")
    high = tuple(range(1000, 1560))   # used indices no token refers to, past the referenced ones
    assert craft.fields(craft.payload(T40, extra_used=high))["G"] == 3
    add("G_less_than_wcnt", craft.payload(T40, extra_used=high, G=2), "same")
    tok("N_cap", roots(CAPB))
    add("N_cap_plus1", craft.payload(roots(CAPB + 1)), "N>cap")
    # stop: `if (ok && (N > kCapBlock || !room(N))) ok = false;`
    add("N_past_record", craft.rebuild(dict(f, N=len(good))), "format")
    add("N_fffffff8", craft.rebuild(dict(f, N=0xFFFFFFF8)), "format", no_oracle=True)   # stop: as N_past_record
    add("N_ffffffff", craft.rebuild(dict(f, N=0xFFFFFFFF)), "format", no_oracle=True)
    some_chars = oracle.huffman_stream(b"abcab")
    add("N_0_chars", craft.payload([], extra_used=(0,), chars_stream=some_chars), "same")
    # stop: `if (room(1))` of the char header sets ok = false
    add("N_0_no_chars", craft.payload([], extra_used=(0,), chars_stream=b""), "format")
    add("N_0_G3", craft.payload([], extra_used=(0,), G=3, chars_stream=some_chars), "same")
    add("W_0", craft.payload(T3000, W=0, group_words=b""), "same")   # every token falls in group 0
    five = [(0, 70), (1, 71), (0, 72), (2, 73), (3, 74)]
    w5 = craft.fields(craft.payload(five, extra_used=high))["group_words"]
    assert len(w5) == 4
    add("W_surplus", craft.payload(five, extra_used=high, group_words=w5 + bytes(range(1, 29))), "same")
    # stop: `if (G > kGmax || !room(8ull * (G - 1) + 8)) ok = false;` and, without a tree, `} else if (room(4)) {`
    add("cut_in_tree", good[:o["tree"] + 12], "format")
    add("cut_before_N", small[:craft.parse(small)["gpos"] - 2], "format")
    # stop: `if (room(4ull * W))`
    add("W_40000001", craft.rebuild(dict(f, W=0x40000001)), "format")
    # stop: the three `room()` of the char header
    add("cut_in_char_bitmap", good[:o["cbm"] + 1], "format")
    add("cut_in_char_pairs", good[:o["cpairs"] + 3], "format")
    add("cut_before_nw", good[:o["nw_off"] + 2], "format")
    add("nw_40000001", craft.rebuild(dict(f, chars=dict(f["chars"], W=0x40000001))), "format")
    s, _ = _sub(oracle.huffman_stream(bytes(c for _, c in T40)), 0)
    s = dict(s, W=s["W"] + 40, words=s["words"] + bytes(range(160)))
    assert s["W"] > 40
    add("nw_surplus", craft.payload(T40, chars_stream=_unsub(s)), "same")
    tok("ts_0", [(0, 97), (1, 97), (2, 97), (0, 97), (3, 97), (1, 97)])   # a one-symbol stream: zeros

    # ---- index (k78d_pindex) ----
    piece = 8 * 16 * 1024   # bits of one 16 KiB piece
    n = piece + 40
    tok("pindex_two_pieces", roots(n) + [(piece - 1, 80), (piece, 81), (5, 82), (piece + 20, 83), (piece - 8 * 16, 84),
                                         (n + 3, 85), (300, 86)])
    bm = bytearray(craft.fields(craft.payload(T40, extra_used=(162,)))["bitmap"])
    assert len(bm) == 21 and bm[20] == 0x04
    bm[20] |= 0xF8   # set bits past the wcnt-th in its byte: the `rank < R.wcnt` stop
    add("pindex_bits_past_wcnt", craft.payload(T40, extra_used=(162,), bitmap=bytes(bm)), "same")

    # ---- group tree (k78d_gtable) ----
    # k78d_gtable's walk accepts a node d <= 31 steps below the root, so a chain of 32 nodes (G = 33,
    # the longest code 32 bits) is the deepest it takes and 33 nodes (G = 34, 33 bits) the next one;
    # group 0, which the tokens use most, has the longest code
    for G in (33, 34):
        rev = list(range(G - 1, -1, -1))
        add(f"chain_G{G}", craft.payload(t600, extra_used=np.arange(256 * (G - 1) + 1), tree=craft.chain_group_tree(G, rev)),
            "same" if G == 33 else "depth>32")
    # codes of kDTblBits - 1, kDTblBits and kDTblBits + 1 bits (and 8 and 12): the wide table's boundary
    G = TBL + 3
    t1300 = rand_tokens(1300, 5)
    tr = craft.chain_group_tree(G, list(range(G - 1, -1, -1)))
    cd = craft.tree_codes(tr, G)
    assert {cd[ix >> 8][1] for ix, _ in t1300} >= {TBL - 1, TBL, TBL + 1}   # (every index used: rank = index)
    add("wide_table_edge", craft.payload(t1300, extra_used=np.arange(256 * (G - 1) + 1), tree=tr), "same")
    # malformed trees no code of the stream walks into: G = 5, group 0's code is the root's left leaf
    ex5 = np.arange(256 * 4 + 1)
    ch5 = craft.chain_group_tree(5)   # [(3, 4), (2, 5), (1, 6), (0, 7)]
    assert ch5 == [(3, 4), (2, 5), (1, 6), (0, 7)]
    w40 = craft.fields(craft.payload(T40, extra_used=ex5, tree=ch5))["group_words"]

    def tree5(name, nodes, verdict):
        t = list(ch5)
        for k, pair in nodes.items():
            t[k] = pair
        add(name, craft.payload(T40, extra_used=ex5, tree=t, group_words=w40), verdict)

    tree5("tree_two_parents", {2: (5, 6)}, "two-parents")         # node 0 under node 1 and node 2
    tree5("tree_lc_eq_rc_nodes", {1: (5, 5)}, "two-parents")
    tree5("tree_self_child", {0: (5, 4)}, "two-parents")          # node 0 under itself and node 1
    tree5("tree_orphan", {1: (2, 3)}, "orphan")                   # node 0 has no parent
    tree5("tree_root_child", {0: (3, 5 + 3)}, "root-child")
    tree5("tree_child_2G_minus_1", {0: (3, 2 * 5 - 1)}, "child>=2G-1")
    tree5("tree_child_ffffffff", {0: (3, 0xFFFFFFFF)}, "child>=2G-1")
    tree5("tree_leaf_twice", {0: (3, 3)}, "same")                 # lc == rc, and leaf 4 has no code
    tree5("tree_leaf_unreached", {0: (3, 0)}, "same")             # group 0 has two codes
    # the same bad child where group 0's code walks into it: the oracle objects too.
    # stop: `if (k >= nodes) { bad = 1; v = 0; }`
    rev5 = craft.chain_group_tree(5, [4, 3, 2, 1, 0])
    wrev = craft.fields(craft.payload(T40, extra_used=ex5, tree=rev5))["group_words"]
    bad5 = list(rev5)
    assert bad5[0] == (1, 0)
    bad5[0] = (1, 2 * 5 - 1)
    add("tree_child_2G_minus_1_walked", craft.payload(T40, extra_used=ex5, tree=bad5, group_words=wrev), "format")

    # ---- group symbols (k78d_groups): the segment decoder on wide codes ----
    # a chain of 31 nodes, group 0 has the code of 31 ones and group g >= 1 has g - 1 ones and a zero:
    # runs of the deepest code, then mixed codes (the idea of the FCX7 corpus's fallback / retry)
    G = 32
    tr = craft.chain_group_tree(G, list(range(1, G)) + [0])
    for name, run, reps in (("groups_fallback", 3500, 2), ("groups_retry", 300, 8)):
        toks = []
        for r in range(reps):
            toks += [(min(len(toks) + i, i % 5), 33 + i % 90) for i in range(run)]
            for i in range(7):
                t = len(toks)
                grp = 1 + (3 * r + i) % min(13, max(1, (t - 40) // 256))   # (its indices lie before token t)
                toks.append((256 * grp + (5 * i + r) % 200, 40 + i))
        p = craft.payload(toks, extra_used=np.arange(256 * (G - 1) + 1), tree=tr)
        add(name, p, "same", toks, False, {"ts": G - 1, "words": craft.fields(p)["group_words"], "claim": name[7:]})

    # ---- links (k78d_links) ----
    tok("r_last", T300)   # the largest used index is referenced: r == wcnt - 1
    f3 = craft.fields(craft.payload(T300))
    wc = f3["wcnt"]
    assert f3["G"] == 1 and wc < 255
    t_last = next(t for t in range(300) if f3["gpos"][t] == wc - 1)
    for name, r in (("r_eq_wcnt", wc), ("r_far_past", 255)):
        gp = bytearray(f3["gpos"])
        gp[t_last] = r
        # stop: `if (r >= R.wcnt) bad = true;`
        add(name, craft.rebuild(dict(f3, gpos=gp)), "format")
    tok("ix_eq_t", abc)
    # stop: `if (ix > t) { bad = true; ix = 0; }`
    tok("ix_eq_t_plus1", [(0, 65), (2, 66), (1, 67)], "format")
    fw = list(T3000)
    fw[2990] = (2995, fw[2990][1])
    tok("forward_ref_late", fw, "format")                  # stop: as ix_eq_t_plus1
    tok("index_past_N", T40 + [(50, 66)], "format")        # stop: as ix_eq_t_plus1 (N = 41)
    d = 1
    while (d + 1) * (d + 2) // 2 <= CAPB:
        d += 1
    assert d < K["kMaxDepth"]   # (1447 for kCapBlock = 2^20 + 8)
    tok(f"chain_{d}", chain(d, 1))
    tok(f"chain_{d + 1}", chain(d + 1, 1), "size>cap")
    # past kMaxDepth the walk itself stops (`n <= kMaxDepth`), and `deep` holds as well as `run > kCapBlock`
    tok("chain_past_kMaxDepth", chain(K["kMaxDepth"] + 11, 1), "size>cap")
    tok("size_cap", sized(CAPB, 9))
    tok("size_cap_tail0", sized(CAPB, 0))
    tok("size_cap_plus1", sized(CAPB + 1, 9), "size>cap")
    # the oracle drops the tail zero and returns kCapBlock bytes; the kernel tests `run` first
    tok("size_cap_plus1_tail0", sized(CAPB + 1, 0), "size>cap")
    per = 1024 * K["kLinkTPT"]   # tokens per round of k78d_links' scan
    for n in (per - 1, per, per + 1):
        tok(f"N_{n}", rand_tokens(n, 6 + n))

    # ---- expansion (k78d_expand, k78d_expand_long) ----
    base = chain(3 * LONG + 8, 2)   # phrases of every length up to 3 kLong + 8: 63, 64, 65, 127, 128, 129, 193
    br = []
    for ix in (LONG, LONG, 2 * LONG, 2 * LONG, LONG - 1, LONG + 1, 2 * LONG - 1, 2 * LONG + 1, 3 * LONG, 3 * LONG + 1):
        br.append((ix, 100 + len(br)))       # parent: the chain's depth-ix token; siblings for kLong and 2 kLong
    n0 = len(base)
    br += [(n0 + 1, 120), (n0 + 3, 121), (n0 + 11, 122)]   # children of the branches
    tok("phrase_edges", base + br)
    tok("long_last_tail0", chain(150, 3) + [(100, 0)])     # a 101-byte phrase last, its final byte dropped
    tok("chain_last_tail0", chain(130, 4)[:-1] + [(129, 0)])
    tok("one_token_00", [(0, 0)])
    tok("one_token_a", [(0, 97)])     # a one-symbol char stream decodes as a zero, which the tail rule drops
    tok("two_tokens", [(0, 97), (0, 98)])

    # ---- char trees (the FCX7 decoder's k_dtable, reached through dec_launch_tables8) ----
    p3 = craft.payload(T300)
    s = f3["chars"]
    internal = [x for x in range(2 * s["ts"]) if (s["bitmap"][x >> 3] >> (x & 7)) & 1]
    assert len(internal) >= 2
    two = bytearray(s["pairs"])
    two[internal[1]] = two[internal[0]]   # one node, two parents (and an orphan)
    add("char_two_parents", craft.rebuild(dict(f3, chars=dict(s, pairs=two))), "char-tree")
    root_x = [x for x in internal if x >> 1 == s["ts"] - 1]
    assert root_x
    low = bytearray(s["pairs"])
    low[root_x[0]] = 0   # an internal child below 256 - real, on a path the codes walk
    # stop: k_dtable `if (v < 256 - real || k >= x / 2) { bad = 1; v = 0; }`
    add("char_child_below_base", craft.rebuild(dict(f3, chars=dict(s, pairs=low))), "format")
    assert craft.rebuild(f3) == p3
    return V


_cache = {}


def corpus():
    if "v" not in _cache:
        _cache["v"] = _corpus()
    return _cache["v"]


def by_name(name):
    return next(v for v in corpus() if v.name == name)


def oracle_block(p: bytes, cap: int = CAP):
    try:
        return oracle.lz78_decompress_block(p, cap)
    except RuntimeError:
        return None


def want(v):
    """the oracle's bytes of a vector (None: it fails, or is not to be run), computed once"""
    if v.name not in _cache:
        _cache[v.name] = None if v.no_oracle else oracle_block(v.payload)
    return _cache[v.name]


def record_vectors():
    """hostile framing, for the entries that take records: (name, records, count); all `format`.
    stop: k78d_index `if (off + 4 > in_len || ld_u32le(in, off) > in_len - off - 4)`, and for the
    short records k78d_head `bool ok = len >= 4;` and its wcnt / popcount-scan tests"""
    good = craft.record(by_name("G_2").payload)
    longer = struct.pack("<I", len(good) - 4 + 1) + good[4:]
    out = [("record_length_plus_1", good + longer, 2), ("nblocks_plus_1", good + good, 3)]
    for n, body in ((0, b""), (3, b"\1\0\0"), (4, b"\1\0\0\0")):
        out.append((f"record_of_{n}", good + craft.record(body) + good, 3))
    return out
