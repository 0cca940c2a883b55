#!/usr/bin/env python3
"""Timing of the line calls, on device-resident runs, beside the search and fcx_check_shard.

  legs      those of tools/findbench.py (rand and text, FCX7 at 1 MiB and 64 KiB blocks, FCX8 at 1 MiB; delimiter
            0x0A), records compressed once by the GPU codec, and zeros as FCX8 with the delimiter 0x00: every
            byte a delimiter.  Per leg: fcx_lines_index_shard (the whole call and its stage table),
            fcx_lines_of_shard over the hits of an 8-byte pattern (the first 16 Mi), fcx_lines_locate_shard for ten lines in the
            middle of the run with and without a given index, fcx_find_shard for the one-byte pattern of the
            delimiter (the count alone) and fcx_check_shard of the same run, both with their stage tables.
  verdicts  the count stage against the search's scan stage for the same byte, alternated three times: each
            count value at or below the upper end of the scan stage's min-max range widened by its width
            (one-sided: the count does strictly less); and the count stage over the digest stage of
            fcx_check_shard, recorded, not gated.

Each figure is the median of --reps calls after --warmup calls, device events around the call (the calls
synchronise their stream).  Before anything is timed the counts are compared with bytes.count over the full
decoder's bytes on the host.  Needs a GPU: there is no fallback.

  python tools/linesbench.py [--mib 1024] [--reps 10] [--warmup 2] [--commit ID] [--out profiles/lines.json]
"""
import argparse
import json
import os
import sys
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from findbench import FORMATS, LEGS, Bench   # noqa: E402


class LinesBench(Bench):
    def row(self, host, d_plain, n, fmt, block, d=0x0A):
        torch, dc, sid = self.torch, self.dc, self.sid
        nb = (n + block - 1) // block
        d_rec, m = self.records(d_plain, n, fmt, block)
        dec = self.decoded(d_rec, m, nb, fmt, n)
        ndec, nl = len(dec), dec.count(bytes([d]))
        last = dec.rfind(bytes([d])) + 1
        want = {"delimiters": nl, "lines": nl + (1 if ndec and last != ndec else 0), "decoded": ndec, "tail_bytes": ndec - last}
        pattern = dec[ndec // 2:ndec // 2 + 8] if ndec >= 16 else b"\0" * 8
        run = (fmt, d_rec.data_ptr(), m, nb)
        idx = [torch.zeros(nb + 1, dtype=torch.int64, device=self.dev) for _ in range(3)]
        dc.index_shard(d_rec.data_ptr(), m, nb, fmt, idx[0].data_ptr(), idx[1].data_ptr(), sid)
        index = lambda: dc.lines_index_shard(*run, d, idx[2].data_ptr(), sid)
        assert index() == want, "not the host count"
        assert dc.lines_stats()["bytes_counted"] == ndec
        dec_off = idx[1].tolist()
        assert idx[2].tolist()[::max(nb // 16, 1)] == [dec.count(bytes([d]), 0, x) for x in dec_off[::max(nb // 16, 1)]], "not the host line index"
        nhits = min(dc.find_shard(*run, pattern), 1 << 24)   # (the first 16 Mi of them: the zeros leg has a hit at every byte)
        d_hits = torch.zeros(max(nhits, 1), dtype=torch.int64, device=self.dev)
        d_lines = torch.zeros(max(nhits, 1), dtype=torch.int64, device=self.dev)
        dc.find_shard(*run, pattern, d_hits.data_ptr(), nhits, sid)
        of = lambda: dc.lines_of_shard(*run, d_hits.data_ptr(), nhits, d_lines.data_ptr(), d, sid)
        of()
        step = max(nhits // 16, 1)
        assert d_lines[:nhits:step].tolist() == [dec.count(bytes([d]), 0, x) for x in d_hits[:nhits:step].tolist()], "not the host ranks"
        first = want["lines"] // 2
        ptrs = tuple(t.data_ptr() for t in idx)
        located = dc.lines_locate_shard(*run, first, 10, d)
        assert located == dc.lines_locate_shard(*run, first, 10, d, ptrs)
        assert dec[located[0]:located[0] + located[1]].count(bytes([d])) == min(10, max(nl - first, 0)), "not ten lines"
        del dec
        mv = memoryview(host.numpy())
        d_crc = torch.tensor([zlib.crc32(mv[o:o + block]) for o in range(0, n, block)], dtype=torch.int64).to(torch.int32).to(self.dev)
        count1 = lambda: dc.find_shard(*run, bytes([d]), 0, 0, sid)
        check = lambda: dc.check_shard(d_rec.data_ptr(), m, nb, fmt, n, block, d_crc.data_ptr(), 0, 0, 0, 0, 0, sid)
        assert count1() == nl
        row = {"records": nb, "compressed_bytes": m, "delimiter": d, "expected": want, "pattern_hits": nhits, "located": list(located),
               "lines_index": self.timed(index), "lines_of_hits": self.timed(of) if nhits else None,
               "locate": self.timed(lambda: dc.lines_locate_shard(*run, first, 10, d)),
               "locate_indexed": self.timed(lambda: dc.lines_locate_shard(*run, first, 10, d, ptrs)),
               "find_delimiter_count_only": self.timed(count1), "check": self.timed(check)}
        row["lines_index_stages_ms"] = self.staged(index)
        row["find_stages_ms"] = self.staged(count1)
        row["check_stages_ms"] = self.staged(check)
        dg = row["check_stages_ms"]["digest"]
        row["count_over_digest"] = round(row["lines_index_stages_ms"]["count"] / dg, 4) if dg else None
        ab = {"scan_ms": [], "count_ms": []}   # alternate three times, stage against stage
        for _ in range(3):
            ab["scan_ms"].append(self.staged(count1)["scan"])
            ab["count_ms"].append(self.staged(index)["count"])
        lo, hi = min(ab["scan_ms"]), max(ab["scan_ms"])
        ab["bound_ms"] = round(hi + (hi - lo), 4)
        ab["count_at_or_below"] = [v <= ab["bound_ms"] for v in ab["count_ms"]]
        row["ab"] = ab
        return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mib", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--commit", default="unknown", help="the commit measured, for the record")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    b = LinesBench(a)
    res = {"mib": a.mib, "reps": a.reps, "warmup": a.warmup, "commit": a.commit,
           "command": f"python tools/linesbench.py --mib {a.mib} --reps {a.reps} --warmup {a.warmup}",
           "timer": "device events around each call (median); the calls synchronise their stream",
           "device": b.torch.cuda.get_device_name(0), "lines": {}}
    n = a.mib << 20

    def leg(key, *args):
        res["lines"][key] = b.row(*args)
        print("lines", key, json.dumps(res["lines"][key]), flush=True)
        if a.out:   # (kept leg by leg)
            with open(a.out, "w") as f:
                json.dump(res, f, indent=1)
                f.write("\n")

    for kind, seed in LEGS:
        host, d_plain = b.plain(kind, seed, n)
        for fmt, block in FORMATS:
            leg(f"{kind}_fcx{fmt}_b{block}", host, d_plain, n, fmt, block)
        del d_plain, host
    host, d_plain = b.plain("zeros", 0, n)
    leg("zeros_fcx8_b1048576_every_byte", host, d_plain, n, "8", 1 << 20, 0x00)
    b.dc.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
