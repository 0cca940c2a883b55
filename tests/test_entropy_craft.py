"""tests/entropy_craft.py pinned on the CPU: every crafted input reaches the place of the entropy
stage it is built for, by the model built from the oracle (entropy_craft.profile), so that a later
edit of a builder, or of a kernel constant, cannot silently stop reaching an edge.  The GPU side
is tests/test_gpu_entropy_edges.py.  No case here may skip: a builder that misses its place fails."""
import numpy as np
import pytest

import entropy_craft as craft
import fcx7_craft as f7
import inputs
import oracle
import test_merge_forms

K = craft.K
CHUNK = craft.CHUNK
V = craft.vectors()


def prof(name):
    _fam, block, data = V[name]
    assert len(data) <= block, name   # one block at the block size the vector names
    return craft.profile(data)


def lens_used(st):
    return sorted(set(st["lens"][st["hist"] > 0].tolist()))


# ---- the model itself ----
def test_constants_come_from_the_sources():
    assert K["kChunk"] == 8192 and K["kTreeT"] == 256 and K["kDeep"] == 8
    assert (K["kJacobiMin"], K["kJacobiMax"]) == (64, 40)
    assert K["kEncWords"] == K["kChunk"] // 4 + 2 == 2050
    assert K["kDeepBytes"] == 32768


def test_model_streams_are_the_crafters_and_the_oracles():
    """sources() restates f7.flag_bytes and the token walk with arrays: the same bytes; profile()
    itself asserts that its streams, coded by oracle.huffman_stream, are oracle.compress_block"""
    for data in (inputs.mosaic(9, 20000), inputs.generate("text", 3, 5000), b"ab" * 300, bytes(range(7))):
        toks = f7.tokens_of(oracle.parse(data))
        src = craft.sources(data)
        pairs = [(p, l) for p, l, _ in toks if l is not None]
        assert src["flags"] == f7.flag_bytes(toks)
        assert src["chars"] == bytes(c for _, _, c in toks)
        assert src["P"] == oracle.combine_bits([p for p, _ in pairs], f7.P_BITS)
        assert src["golomb"] == oracle.golomb_encode([l for _, l in pairs])
        pr = craft.profile(data, 1234)
        assert pr["record"][4:] == f7.payload(toks)
        # the words of every coded stream lie where the model says: W words at obyte
        for name in craft.NAMES:
            st = pr[name]
            if st["active"]:
                sub = f7.fields(pr["record"][4:])["P" if name == "P" else name]
                at = st["obyte"] - 1234
                assert pr["record"][at - 4:at] == sub["W"].to_bytes(4, "little")
                assert pr["record"][at:at + 4 * sub["W"]] == bytes(sub["words"])


def test_every_vector_stays_inside_the_kernels_limits():
    """no crafted stream needs more than kJacobiMax rounds or a code above 32 bits"""
    for name, (_fam, block, data) in V.items():
        for pr in craft.profiles(data, block):
            for s in craft.NAMES:
                st = pr[s]
                if st["active"]:
                    assert st["form"] != "fixed>serial" and st["rounds"] <= K["kJacobiMax"], (name, s)
                    assert st["deepest"] <= K["kMaxCodeLen"], (name, s)
                    assert int(st["windows"].max()) <= 2, (name, s)


def test_every_vector_decodes_back_in_the_oracle():
    """at its own block size; the all-literal vectors of a multiple of 8 tokens are the reference's
    one-symbol quirk and decode to nothing"""
    quirks = []
    for name, (_fam, block, data) in V.items():
        pr = craft.profile(data)
        got = oracle.decompress_block(pr["record"][4:], len(data) + 16)
        if craft.one_symbol_flags(pr):
            quirks.append(name)
            assert got == b"", name
        else:
            assert got == data, name
    assert sorted(quirks) == sorted(["form_edge_21", "leaves_66_small"] + [f"len_flags{n}_full" for n in craft.FLAG_LENGTHS])


def test_two_blocks():
    a, b = craft.profiles(craft.two_blocks(), craft.TWO_BLOCKS)
    assert int(a["chars"]["windows"].max()) == 2 and a["chars"]["chunks"] == 6
    assert not b["chars"]["byte8"] and b["chars"]["chunks"] == 16 and int(b["chars"]["windows"].max()) == 1
    assert b["chars"]["obyte"] > len(a["record"])   # the second record's offsets start behind the first


# ---- 1. the general coder on a long chars stream ----
@pytest.mark.parametrize("name", sorted(craft.family("no255")))
def test_long_general_coder_streams(name):
    st = prof(name)["chars"]
    assert not st["byte8"] and st["chunks"] > 64 and int(st["windows"].max()) == 1
    if name.endswith("_66"):   # the fewest tokens with 66 chunks: the last chunk holds one symbol
        assert st["chunks"] == craft.NO255_CHUNKS and st["n"] % CHUNK == 1
    else:
        assert st["chunks"] == 128
    full = st["bits"][:-1]
    if name.startswith("no255"):
        assert st["real"] == 255 and lens_used(st) == [7, 8] and st["form"] == "closed"
        assert 65400 < full.min() and full.max() < 65536   # one window, just under the staging's 65 600
    else:
        assert st["real"] == 256 and lens_used(st) == [7, 8, 9] and st["form"] == "fixed"
        assert (full < 65536).sum() >= 10 and (full > 65536).sum() >= 10
        assert full.max() < 32 * K["kEncWords"] - 31


# ---- 2. two staging windows ----
@pytest.mark.parametrize("name", sorted(craft.family("two_window")))
def test_two_windows(name):
    _fam, _block, data = V[name]
    st = prof(name)["chars"]
    w = st["windows"]
    assert int(w.max()) == 2 and not st["byte8"]
    two = np.flatnonzero(w == 2)
    if "middle" in name or name == "window_seam":
        # the two-window chunk has a successor that starts inside a word: it publishes its tail,
        # and the successor merges it
        assert any(c + 1 < st["chunks"] and st["sh0"][c + 1] != 0 for c in two), (two, st["sh0"])
    if "tail" in name:
        assert two[-1] >= st["chunks"] - 2
    # the control: at the ragged block size no chunk of any block leaves the first window
    for pr in craft.profiles(data, craft.RAGGED):
        assert int(pr["chars"]["windows"].max()) == 1


def test_window_seam():
    """a chunk, not the stream's last, that ends fewer than 32 bits into its second window: k_encode
    publishes its tail from ws[0] and the previous window's last word (`prevlast`)"""
    st = prof("window_seam")["chars"]
    assert st["seam"] and all(c < st["chunks"] - 1 for c in st["seam"])
    for c in st["seam"]:
        e = int(st["sh0"][c] + st["bits"][c]) - 32 * K["kEncWords"]
        assert 0 < e < 32 and st["windows"][c] == 2
    # no other vector gets there
    for name, (_fam, block, data) in V.items():
        if name != "window_seam":
            assert not any(pr[s].get("seam") for pr in craft.profiles(data, block) for s in craft.NAMES), name


def test_window_seam_search_finds_the_committed_seed():
    assert craft.seam_search(60.0) == craft.SEAM


# ---- 3. form boundaries ----
@pytest.mark.parametrize("wmax,form", [(19, "closed"), (20, "fixed"), (21, "fixed")])
def test_form_edge(wmax, form):
    pr = prof(f"form_edge_{wmax}")
    st = pr["chars"]
    assert pr["N"] == st["n"] == sum(craft.form_edge_weights(wmax)) and pr["pcnt"] == 0   # all literal
    assert sorted(st["hist"].tolist()) == sorted(craft.form_edge_weights(wmax))
    sw = sorted(st["hist"].tolist())
    assert sw[0] + sw[1] - sw[-1] == 20 - wmax
    assert st["form"] == form and st["real"] == 256
    # equality (20) is not the closed form, and still gives 256 codes of 8 bits: the byte
    # substitution behind the fixed point
    assert st["byte8"] == (wmax <= 20)


@pytest.mark.parametrize("ties", sorted(craft.TIES))
@pytest.mark.parametrize("real", craft.LEAF_COUNTS)
def test_leaf_counts(real, ties):
    pr = prof(f"leaves_{real}_{ties}")
    st = pr["chars"]
    w = craft.leaf_count_weights(real, ties)
    assert pr["pcnt"] == 0 and st["real"] == real and sorted(x for x in st["hist"].tolist() if x) == sorted(w)
    nint = real - 1
    want = "closed" if real == 2 else ("fixed" if nint >= K["kJacobiMin"] else "serial")
    assert st["form"] == want, (st["form"], want)
    assert len(set(w)) < len(w) or real == 2 or real == 3   # ties between leaves
    if ties == "pow2" and real > 3:   # and between a leaf and an internal node
        leaves = craft.sorted_leaves(st["hist"].tolist())
        kids = craft.serial(leaves)
        wt = {("L", s): x for x, s in leaves}
        for k, (a, b) in enumerate(kids):
            wt[("I", k)] = wt[a] + wt[b]
        assert {wt[("I", k)] for k in range(len(kids))} & set(w)


# ---- 4. byte-substitution tails ----
@pytest.mark.parametrize("name", sorted(craft.family("byte8")))
def test_byte8_tails(name):
    k, r, align = (int(x[1:]) for x in name.split("_")[1:])
    st = prof(name)["chars"]
    assert st["byte8"] and st["n"] == CHUNK * k + r
    assert st["chunks"] == k + (r > 0)
    assert (st["sh0"] == 8 * align).all()
    last = st["n"] - CHUNK * (st["chunks"] - 1)
    assert last == (r or CHUNK)
    assert st["nw"][-1] == (8 * align + 8 * last + 31) // 32


def test_byte8_one_word_chunks_both_ways():
    """a last chunk of one word (`nw == 1`) that starts on a word boundary, and one that does not"""
    seen = set()
    for name in craft.family("byte8"):
        st = prof(name)["chars"]
        if st["nw"][-1] == 1:
            seen.add(bool(st["sh0"][-1]))
    assert seen == {False, True}


# ---- 5. deep codes ----
def test_deep_codes():
    g = prof("geometric")["chars"]
    assert g["deepest"] >= 16
    pr = prof("fibonacci")
    f = pr["chars"]
    assert f["deepest"] >= 20 and f["deepest"] == 23
    assert pr["N"] - pr["pcnt"] < 3 * craft.FIB_K   # every unit parsed as (match of 3, char)
    d = prof("deepest_chunk")["chars"]
    assert d["form"] == "fixed" and d["deepest"] == 20 and d["rounds"] == 21
    # chunk 0, with a successor, takes two windows and is the fullest chunk these builders know:
    # 114 540 bits, a third window needs more than 131 200
    assert d["windows"][0] == 2 and int(d["bits"].argmax()) == 0
    assert 110000 < int(d["bits"][0]) < 64 * K["kEncWords"]


# ---- stream lengths ----
def test_stream_lengths():
    L = {name[4:]: prof(name) for name in craft.family("lengths")}
    for n in craft.FLAG_LENGTHS:
        for full in ("", "_full"):
            pr = L[f"flags{n}{full}"]
            assert pr["flags"]["n"] == n and pr["pcnt"] == 0
            assert pr["flags"]["hist"][0xFF] == n - (not full) and pr["flags"]["real"] == 2 - bool(full)
    for d in (-1, 0, 1):
        n = K["kDeepBytes"] + d
        st = L[f"flags{n}_rand"]["flags"]
        assert st["n"] == n and st["hist"][0xFF] > n - 100 and st["real"] > 2
    for n, pcnt in craft.P_LENGTHS.items():
        pr = L[f"p{n}"]
        assert pr["pcnt"] == pcnt and pr["P"]["n"] == n
    assert {2, 16, 17, 31, K["kDeepBytes"] - 1, K["kDeepBytes"]} <= set(craft.P_LENGTHS)
    for name in ("ab5000", "ab70001"):
        st = L[name]["flags"]
        assert st["hist"][0] >= st["n"] - 1          # every token but the first two a match
        assert L[name]["golomb"]["hist"][0xFF] > L[name]["golomb"]["n"] // 2


# ---- the sweep behind "unreachable" ----
def test_sweep_rounds_and_depths():
    """histograms of at most 2^20 symbols and at least 65 leaves (fewer never enter the fixed
    point): the worst round count and the deepest code stay under kJacobiMax and 32.  Measured:
    26 rounds and 25 bits (a Fibonacci chain of 22 beside 43 equal leaves); the rounds were the
    tree's height + 1 throughout.  The depth is also bounded outright: a Huffman code of d bits needs
    F(d + 2) symbols, and F(31) > 2^20, so d <= 28."""
    def families():
        yield from craft.sweep_histograms()
        for i, w in enumerate(test_merge_forms.histograms()):
            if sum(1 for x in w if x) > K["kJacobiMin"]:
                yield f"merge_forms{i}", craft.scaled(w)
        for name, (_fam, block, data) in V.items():
            st = craft.profile(data[:block])["chars"]
            if st["real"] > K["kJacobiMin"]:
                yield name, st["hist"].tolist()

    worst, deepest, count = (0, None), (0, None), 0
    for name, w in families():
        assert sum(w) <= craft.MiB and sum(1 for x in w if x) > K["kJacobiMin"], name
        leaves = craft.sorted_leaves(w)
        kids, rounds = craft.fixed_point(leaves)
        assert kids == craft.serial(leaves), name
        d = max(craft.depths(kids).values())
        worst, deepest, count = max(worst, (rounds, name)), max(deepest, (d, name)), count + 1
    print(f"SWEEP histograms={count} worst_rounds={worst} deepest_code={deepest}")
    assert count > 400
    assert worst[0] == 26 and deepest[0] == 25, (worst, deepest)
    assert worst[0] <= K["kJacobiMax"] and deepest[0] <= K["kMaxCodeLen"]
    fib = [1, 1]
    while fib[-1] <= craft.MiB:
        fib.append(fib[-1] + fib[-2])
    assert len(fib) == 31 and len(fib) - 3 <= K["kMaxCodeLen"]   # fib[-1] = F(31): d + 2 <= 30
