#!/usr/bin/env python3
"""Timing of the pattern sets' device calls, on device-resident runs, beside fcx_find_shard and
fcx_grep_shard of the same library.

  legs      those of tools/findbench.py and tools/grepbench.py (rand and text, FCX7 at 1 MiB and 64 KiB blocks, FCX8
            at 1 MiB), delimiter 0x0A, every call count only.  Per leg:
            one       a set of one 8-byte pattern against fcx_find_shard and fcx_grep_shard of that pattern, alternated
                      three times and judged by the A/B rule (the set's values against the one-pattern call's min-max
                      range widened by its width on each side)
            sets      P = 1, 8 and 64 patterns of 8 bytes cut from the data, and 64 that do not occur but share their
                      first two bytes with the data: the whole fcx_find_set_shard call, its stage table and the scan's
                      counters; scan(P = 64) / scan(P = 1)
            calls     the 64 cut patterns in one fcx_find_set_shard call against 64 calls of fcx_find_shard
            fold      the 64 cut patterns with FCX_SET_FOLD_ASCII against the same set without it
            grep      fcx_grep_set_shard of the 64 cut patterns, whole call and stage table

Each figure is the median of --reps calls after --warmup calls, device events around the call (the calls
synchronise their stream).  Before anything is timed every leg's hits, counts and lines are compared with the
definitions of include/fcx.h over the full decoder's bytes on the host (bytes.find per pattern, numpy for the union
and the lines).  Needs a GPU: there is no fallback.

  python tools/setbench.py [--mib 1024] [--reps 10] [--warmup 2] [--commit ID] [--out profiles/set.json]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from findbench import FORMATS, LEGS   # noqa: E402
from grepbench import DELIM, GrepBench   # noqa: E402

FOLD = bytes(b + 0x20 if 0x41 <= b <= 0x5A else b for b in range(256))


def model(dec: bytes, patterns, fold: bool):
    """(hits, counts, starts, ends): the union of the patterns' positions, the per-pattern counts and the lines
    that hold a hit, by the definitions over the decoder's bytes"""
    import numpy as np

    text = dec.translate(FOLD) if fold else dec
    T, per, counts = len(dec), [], []
    for p in patterns:
        p = p.translate(FOLD) if fold else p
        h, i = [], text.find(p)
        while i >= 0:
            h.append(i)
            i = text.find(p, i + 1)
        per.append(np.array(h, dtype=np.int64))
        counts.append(len(h))
    hits = np.unique(np.concatenate(per)) if per else np.zeros(0, dtype=np.int64)
    dpos = np.flatnonzero(np.frombuffer(dec, dtype=np.uint8) == DELIM)
    lines = np.unique(np.searchsorted(dpos, hits, side="left"))
    bounds = np.concatenate(([0], dpos + 1, [T])).astype(np.int64)
    return hits, counts, bounds[lines], np.minimum(bounds[lines + 1], T)


def cut(src: bytes, k: int, m: int = 8):
    """k distinct patterns of m bytes without the delimiter, cut at even steps from the middle half of src"""
    out, at, step = [], len(src) // 4, max((len(src) // 2) // (k + 1), m)
    while len(out) < k:
        p = src[at:at + m]
        if DELIM not in p and len(p) == m and p not in out:
            out.append(p)
            at += step
        else:
            at += 1
    return out


def absent(src: bytes, dec: bytes, k: int, m: int = 8):
    """k patterns that do not occur in dec, folded or not, each starting with two bytes that src holds side by side"""
    import random

    rng, out, text = random.Random(7), [], dec.translate(FOLD)
    head = src[len(src) // 2:len(src) // 2 + 2]
    while DELIM in head:
        head = bytes([0x61, 0x62])
    while len(out) < k:
        p = head + bytes(rng.choice(b"\x01\x02\x03\x04\x05\x06\x07\x08") for _ in range(m - 2))
        if p not in out and dec.find(p) < 0 and text.find(p.translate(FOLD)) < 0:
            out.append(p)
    return out


class SetBench(GrepBench):
    def ab_pair(self, base, other):
        r = {"one_pattern_ms": [], "set_ms": []}   # the A/B rule: alternate three times
        for _ in range(3):
            r["one_pattern_ms"].append(round(self.once(base), 4))
            r["set_ms"].append(round(self.once(other), 4))
        lo, hi = min(r["one_pattern_ms"]), max(r["one_pattern_ms"])
        r["band_ms"] = [round(lo - (hi - lo), 4), round(hi + (hi - lo), 4)]
        r["set_inside"] = [r["band_ms"][0] <= v <= r["band_ms"][1] for v in r["set_ms"]]
        return r

    def checked(self, run, dec, pats, fold):
        """a set, its calls compared with the model before they are timed"""
        torch, dc, sid, mc = self.torch, self.dc, self.sid, self.mc
        hits, counts, s, e = model(dec, pats, fold)
        ps = mc.PatternSet(pats, fold)
        d_hits = torch.zeros(max(len(hits), 1), dtype=torch.int64, device=self.dev)
        n, got = dc.find_set_shard(*run, ps, d_hits.data_ptr(), len(hits), sid)
        assert n == len(hits) and got == counts, "not the model's hits or counts"
        assert bool((d_hits[:n].cpu() == torch.from_numpy(hits)).all()), "not the model's offsets"
        sc = dc.set_scan_stats()
        assert sc["judged"] == max(len(dec) - min(map(len, pats)) + 1, 0) and sc["hits"] == n
        L = len(s)
        d_s = torch.zeros(max(L, 1), dtype=torch.int64, device=self.dev)
        d_e = torch.zeros(max(L, 1), dtype=torch.int64, device=self.dev)
        st, gc = dc.grep_set_shard(*run, ps, DELIM, d_s.data_ptr(), d_e.data_ptr(), L, sid)
        assert (st["lines"], st["bytes"], st["hits"]) == (L, int((e - s).sum()), n) and gc == counts, "not the model's lines"
        assert d_s[:L].cpu().numpy().tolist() == s.tolist() and d_e[:L].cpu().numpy().tolist() == e.tolist(), "not the model's lines"
        return ps, {"patterns": len(pats), "fold": fold, "hits": n, "lines": L, "sum_counts": sum(counts), "scan_stats": sc}

    def row(self, host, d_plain, n, fmt, block):
        dc, sid = self.dc, self.sid
        nb = (n + block - 1) // block
        d_rec, m = self.records(d_plain, n, fmt, block)
        dec = self.decoded(d_rec, m, nb, fmt, n)
        src = dec if len(dec) >= 1 << 16 else bytes(memoryview(host.numpy())[:1 << 16])
        run = (fmt, d_rec.data_ptr(), m, nb)
        cuts = cut(src, 64)
        sets = {"P1": cuts[:1], "P8": cuts[:8], "P64": cuts, "P64_absent": absent(src, dec, 64)}
        row = {"records": nb, "compressed_bytes": m, "decoded_bytes": len(dec), "sets": {}}
        keep = {}
        for name, pats in sets.items():
            ps, info = self.checked(run, dec, pats, False)
            keep[name] = ps
            fn = lambda ps=ps: dc.find_set_shard(*run, ps, 0, 0, sid)
            info["find_set_count_only"] = self.timed(fn)
            info["stages_ms"] = self.staged(fn)
            row["sets"][name] = info
        s1, s64 = row["sets"]["P1"]["stages_ms"]["scan"], row["sets"]["P64"]["stages_ms"]["scan"]
        row["scan_P64_over_P1"] = round(s64 / s1, 4) if s1 else None
        row["scan_P64_absent_over_P1"] = round(row["sets"]["P64_absent"]["stages_ms"]["scan"] / s1, 4) if s1 else None
        # 1. a set of one against the one-pattern calls
        one, pat = keep["P1"], cuts[0]
        find1 = lambda: dc.find_shard(*run, pat, 0, 0, sid)
        grep1 = lambda: dc.grep_shard(*run, pat, DELIM, 0, 0, 0, sid)
        fset1 = lambda: dc.find_set_shard(*run, one, 0, 0, sid)
        gset1 = lambda: dc.grep_set_shard(*run, one, DELIM, 0, 0, 0, sid)
        assert fset1()[0] == find1() and gset1()[0] == grep1()
        assert dc.set_scan_stats()["judged"] == grep1()["judged"]
        row["one"] = {"find_shard": self.timed(find1), "find_set_shard": self.timed(fset1), "find_ab": self.ab_pair(find1, fset1),
                      "grep_shard": self.timed(grep1), "grep_set_shard": self.timed(gset1), "grep_ab": self.ab_pair(grep1, gset1),
                      "find_stages_ms": self.staged(find1), "find_set_stages_ms": self.staged(fset1)}
        # 3. one call of 64 against 64 calls of one
        many = lambda: [dc.find_shard(*run, p, 0, 0, sid) for p in cuts]
        assert sum(many()) == row["sets"]["P64"]["sum_counts"]
        t64, tset = self.timed(many), row["sets"]["P64"]["find_set_count_only"]
        row["calls"] = {"sixty_four_find_shard_calls": t64, "one_find_set_shard_call": tset,
                        "ratio": round(t64["median_ms"] / tset["median_ms"], 2)}
        # 4. the fold
        fps, finfo = self.checked(run, dec, cuts, True)
        ffn = lambda: dc.find_set_shard(*run, fps, 0, 0, sid)
        finfo["find_set_count_only"] = self.timed(ffn)
        finfo["stages_ms"] = self.staged(ffn)
        row["fold"] = {"on": finfo, "off_median_ms": tset["median_ms"], "off_scan_ms": s64,
                       "on_over_off": round(finfo["find_set_count_only"]["median_ms"] / tset["median_ms"], 4)}
        # the grep of the 64
        gfn = lambda: dc.grep_set_shard(*run, keep["P64"], DELIM, 0, 0, 0, sid)
        row["grep"] = {"grep_set_count_only": self.timed(gfn), "stages_ms": self.staged(gfn)}
        for ps in list(keep.values()) + [fps]:
            ps.close()
        return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mib", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--commit", default="unknown", help="the commit measured, for the record")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert a.reps >= 10, "the median of at least 10 runs"
    b = SetBench(a)
    res = {"mib": a.mib, "reps": a.reps, "warmup": a.warmup, "commit": a.commit,
           "command": f"python tools/setbench.py --mib {a.mib} --reps {a.reps} --warmup {a.warmup}",
           "timer": "device events around each call (median); the calls synchronise their stream",
           "device": b.torch.cuda.get_device_name(0), "set": {}}
    n = a.mib << 20
    for kind, seed in LEGS:
        host, d_plain = b.plain(kind, seed, n)
        for fmt, block in FORMATS:
            key = f"{kind}_fcx{fmt}_b{block}"
            res["set"][key] = b.row(host, d_plain, n, fmt, block)
            print("set", key, json.dumps(res["set"][key]), flush=True)
            if a.out:   # (kept leg by leg: a long run leaves what it has)
                with open(a.out, "w") as f:
                    json.dump(res, f, indent=1)
                    f.write("\n")
        del d_plain, host
    b.dc.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
