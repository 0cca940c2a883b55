#!/usr/bin/env python3
"""Timing of the grep's and the multi-range decode's device calls, on device-resident runs, beside
fcx_find_shard, fcx_decompress_range_shard and the full decode of the same library.

  legs      those of tools/findbench.py (rand and text, FCX7 at 1 MiB and 64 KiB blocks, FCX8 at 1 MiB), 8-byte
            pattern cut from the data, delimiter 0x0A.  Per leg: the whole fcx_grep_shard call against
            fcx_find_shard, both count only, alternated three times and judged by the A/B rule (grep's values
            against find's min-max range widened by its width on each side); both stage tables; then the ranges
            decode of the selected lines, sparse (the 8-byte pattern's few lines) and dense (a 1-byte pattern that
            selects most lines), each beside fcx_decompress_range_shard of one range of as many bytes and beside
            the full decode, with the records touched and decoded.
  worst     the two worst cases of the scratch: every second byte the delimiter (T / 2 lines), and a run of one
            byte value searched for that byte (T hits, one line): time and the scratch reserved.

Each figure is the median of --reps calls after --warmup calls, device events around the call (the calls
synchronise their stream).  Before anything is timed every leg's lines are compared with the model over the full
decoder's bytes on the host (the definitions of include/fcx.h in numpy: the delimiters' positions, the hits, the
distinct lines that hold one), and the ranges decode's bytes with the join of the slices.  Needs a GPU: there is
no fallback.

  python tools/grepbench.py [--mib 1024] [--reps 10] [--warmup 2] [--commit ID] [--out profiles/grep.json]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from findbench import FORMATS, LEGS, Bench   # noqa: E402

DELIM = 0x0A


def model(dec: bytes, pattern: bytes):
    """(hits, starts, ends) of the selected lines by the definitions, in numpy over the decoder's bytes"""
    import numpy as np

    a = np.frombuffer(dec, dtype=np.uint8)
    T = len(dec)
    if len(pattern) == 1:
        hits = np.flatnonzero(a == pattern[0])
    else:
        h, i = [], dec.find(pattern)
        while i >= 0:
            h.append(i)
            i = dec.find(pattern, i + 1)
        hits = np.array(h, dtype=np.int64)
    dpos = np.flatnonzero(a == DELIM)
    lines = np.unique(np.searchsorted(dpos, hits, side="left"))   # the delimiters in front of each hit: its line
    bounds = np.concatenate(([0], dpos + 1, [T])).astype(np.int64)
    return len(hits), bounds[lines], np.minimum(bounds[lines + 1], T)


class GrepBench(Bench):
    def ab(self, base, other):
        r = {"find_ms": [], "grep_ms": []}   # the A/B rule: alternate three times
        for _ in range(3):
            r["find_ms"].append(round(self.once(base), 4))
            r["grep_ms"].append(round(self.once(other), 4))
        lo, hi = min(r["find_ms"]), max(r["find_ms"])
        r["band_ms"] = [round(lo - (hi - lo), 4), round(hi + (hi - lo), 4)]
        r["grep_inside"] = [r["band_ms"][0] <= v <= r["band_ms"][1] for v in r["grep_ms"]]
        return r

    def ranges_leg(self, run, dec, pattern, n, fmt):
        torch, dc, sid = self.torch, self.dc, self.sid
        hits, s, e = model(dec, pattern)
        L, nbytes = len(s), int((e - s).sum())
        d_s = torch.zeros(max(L, 1), dtype=torch.int64, device=self.dev)
        d_e = torch.zeros(max(L, 1), dtype=torch.int64, device=self.dev)
        st = dc.grep_shard(*run, pattern, DELIM, d_s.data_ptr(), d_e.data_ptr(), L, sid)
        assert (st["lines"], st["bytes"], st["hits"]) == (L, nbytes, hits), "not the model's totals"
        assert d_s[:L].cpu().numpy().tolist() == s.tolist() and d_e[:L].cpu().numpy().tolist() == e.tolist(), "not the model's lines"
        d_out = torch.empty(max(nbytes, 1) + 64, dtype=torch.uint8, device=self.dev)
        ranges = lambda: dc.decompress_ranges_shard(*run, d_s.data_ptr(), d_e.data_ptr(), L, d_out.data_ptr(), nbytes, None, sid)
        assert ranges() == nbytes
        got = d_out[:nbytes].cpu().numpy().tobytes()
        assert got == b"".join(dec[a:b] for a, b in zip(s.tolist(), e.tolist())), "not the join of the slices"
        rs = dc.ranges_stats()
        one = lambda: dc.decompress_range_shard(run[1], run[2], run[3], fmt, 0, nbytes, d_out.data_ptr(), max(nbytes, 1), 0, 0, sid)
        row = {"pattern_bytes": len(pattern), "lines": L, "bytes": nbytes, "hits": hits, "ranges_stats": rs,
               "ranges": self.timed(ranges), "one_range_of_as_many_bytes": self.timed(one), "ranges_stages_ms": self.staged(ranges)}
        return row

    def row(self, host, d_plain, n, fmt, block, dense_byte):
        torch, dc, sid = self.torch, self.dc, self.sid
        nb = (n + block - 1) // block
        d_rec, m = self.records(d_plain, n, fmt, block)
        dec = self.decoded(d_rec, m, nb, fmt, n)
        src = dec if len(dec) >= 4096 else bytes(memoryview(host.numpy())[:4096])
        at = len(src) // 2
        while DELIM in src[at:at + 8]:
            at += 1
        pattern = src[at:at + 8]
        run = (fmt, d_rec.data_ptr(), m, nb)
        hits, s, e = model(dec, pattern)
        grep = lambda: dc.grep_shard(*run, pattern, DELIM, 0, 0, 0, sid)
        find = lambda: dc.find_shard(*run, pattern, 0, 0, sid)
        st = grep()
        assert (st["lines"], st["bytes"], st["hits"], st["judged"], st["decoded"]) == (
            len(s), int((e - s).sum()), hits, max(len(dec) - 8 + 1, 0), len(dec)), "not the model's totals"
        assert find() == hits
        d_full = torch.empty(n + nb * 8 + 64, dtype=torch.uint8, device=self.dev)
        full_fn = dc.decompress_shard if fmt == "7" else dc.decompress_lz78_shard
        full = lambda: full_fn(d_rec.data_ptr(), m, nb, d_full.data_ptr(), d_full.numel(), sid)
        row = {"records": nb, "compressed_bytes": m, "decoded_bytes": len(dec), "grep_stats": st, "scratch_bytes": dc.grep_scratch(),
               "grep_count_only": self.timed(grep), "find_count_only": self.timed(find), "full_decode": self.timed(full)}
        row["grep_stages_ms"] = self.staged(grep)
        row["find_stages_ms"] = self.staged(find)
        row["ab"] = self.ab(find, grep)
        row["grep_over_find"] = round(row["grep_count_only"]["median_ms"] / row["find_count_only"]["median_ms"], 4)
        if len(dec) >= 4096:
            row["sparse"] = self.ranges_leg(run, dec, pattern, n, fmt)
            row["dense"] = self.ranges_leg(run, dec, bytes([dense_byte]), n, fmt)
        return row

    def worst(self, data: bytes, pattern: bytes, lines: int, hits: int):
        torch, dc, sid = self.torch, self.dc, self.sid
        n, block = len(data), 1 << 20
        host = torch.frombuffer(bytearray(data), dtype=torch.uint8)
        d_rec, m = self.records(host.to(self.dev), n, "7", block)
        run = ("7", d_rec.data_ptr(), m, (n + block - 1) // block)
        grep = lambda: dc.grep_shard(*run, pattern, DELIM, 0, 0, 0, sid)
        st = grep()
        assert (st["lines"], st["hits"], st["bytes"], st["decoded"]) == (lines, hits, n, n), st
        return {"decoded_bytes": n, "lines": lines, "hits": hits, "scratch_bytes": dc.grep_scratch(),
                "eight_bytes_per_hit": 8 * hits, "grep_count_only": self.timed(grep), "grep_stages_ms": self.staged(grep)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mib", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--commit", default="unknown", help="the commit measured, for the record")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert a.reps >= 10, "the median of at least 10 runs"
    b = GrepBench(a)
    res = {"mib": a.mib, "reps": a.reps, "warmup": a.warmup, "commit": a.commit,
           "command": f"python tools/grepbench.py --mib {a.mib} --reps {a.reps} --warmup {a.warmup}",
           "timer": "device events around each call (median); the calls synchronise their stream",
           "device": b.torch.cuda.get_device_name(0), "grep": {}, "worst": {}}
    n = a.mib << 20
    for kind, seed in LEGS:
        host, d_plain = b.plain(kind, seed, n)
        dense = 0x65 if kind == "text" else int(host[12345]) if int(host[12345]) != DELIM else 0x41
        for fmt, block in FORMATS:
            key = f"{kind}_fcx{fmt}_b{block}"
            res["grep"][key] = b.row(host, d_plain, n, fmt, block, dense)
            print("grep", key, json.dumps(res["grep"][key]), flush=True)
        del d_plain, host
    w = min(n, 256 << 20)
    res["worst"]["every_second_byte_the_delimiter"] = b.worst(b"x\n" * (w // 2), b"x", w // 2, w // 2)
    res["worst"]["one_byte_value_one_line"] = b.worst(bytes(w), b"\0", 1, w)   # (zeros: what such a block decodes to)
    print("worst", json.dumps(res["worst"]), flush=True)
    b.dc.close()
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
