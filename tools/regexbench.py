#!/usr/bin/env python3
"""Timing of the regex grep's device call, on device-resident runs, beside fcx_grep_blocks_shard of the
same library.

  legs      those of tools/setbench.py (rand and text, FCX7 at 1 MiB and 64 KiB blocks, FCX8 at 1 MiB), delimiter 0x0A,
            every call count only, zero options.  Per leg:
            literal   a regex that is one 8-byte literal cut from the data against fcx_grep_blocks_shard of the
                      one-pattern set, alternated three times and judged by the A/B rule (the regex's values against
                      the set call's min-max range widened by its width on each side); the whole-call ratio and both
                      stage tables
            states    the whole call and its stage table for expressions of 4, 17, 33 and 64 DFA states;
                      scan(S) / decode and scan(S = 64) / scan(S = 4)
            --split X (the text FCX7 1 MiB leg alone, under a kernel trace) runs one expression, the literal or one of
                      the four, --reps times and nothing else, so that the trace's per-kernel averages split the scan
                      stage into k_rmap, k_rentry and k_rmark; --add-split X=CSV then copies them from the trace's
                      kernel statistics into the JSON of --out, with the command line of the trace (no GPU needed)

Each figure is the median of --reps calls after --warmup calls, device events around the call (the calls synchronise
their stream).  Before anything is timed every expression's blocks (every start, end and first line), selected lines,
base lines, bytes and the judged positions are compared with the definitions of include/fcx.h over the full decoder's
bytes on the host: Python's re for the matches (the negated sets spelled with the delimiter), numpy for the lines;
the number of hits is compared for the literal, whose match ends are as many as its occurrences (overlapping ones
included).  Needs a GPU: there is no fallback.

  python tools/regexbench.py [--mib 256] [--reps 10] [--warmup 2] [--commit ID] [--out profiles/regex.json]
  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o X -- python tools/regexbench.py --split X
  python tools/regexbench.py --out profiles/regex.json --add-split X=DIR/.../X_kernel_stats.csv [--add-split ...]
"""
import argparse
import csv
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from findbench import FORMATS, LEGS   # noqa: E402
from grepbench import DELIM, GrepBench   # noqa: E402

SPLIT_COMMAND = "rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o X -- python tools/regexbench.py --split X --mib {mib} --reps {reps}"
# (ours, Python's with the delimiter spelled out, DFA states)
STATES = [(b"the", b"the", 4), (b"a[^b]{3}b", b"a[^b\n]{3}b", 17), (b"a[^b]{4}b", b"a[^b\n]{4}b", 33),
          (b"a[^b]{4}b|[c-e]{5}", b"a[^b\n]{4}b|[c-e]{5}", 64)]


def model(dec: bytes, py_expr: bytes):
    """(starts, ends, first lines, selected lines) of the blocks with zero options: the maximal runs of lines in which
    a match ends, by Python's re and numpy over the decoder's bytes"""
    import numpy as np

    a = np.frombuffer(dec, dtype=np.uint8)
    T = len(dec)
    ends = np.fromiter((m.end() - 1 for m in re.finditer(py_expr, dec)), dtype=np.int64)
    dpos = np.flatnonzero(a == DELIM)
    lines = np.unique(np.searchsorted(dpos, ends, side="left"))   # the delimiters in front of a match's end: its line
    bounds = np.concatenate(([0], dpos + 1, [T])).astype(np.int64)
    if len(lines) == 0:
        return lines, lines, lines, 0
    first = np.concatenate(([True], np.diff(lines) > 1))
    last = np.concatenate((np.diff(lines) > 1, [True]))
    return bounds[lines[first]], np.minimum(bounds[lines[last] + 1], T), lines[first], len(lines)


def literal_of(src: bytes) -> bytes:
    """8 letters or blanks cut from the middle of the data (what does not occur, where the data holds no such run)"""
    at = len(src) // 2
    while not re.fullmatch(rb"[A-Za-z ]{8}", src[at:at + 8]) and at + 8 < len(src):
        at += 1
    return src[at:at + 8] if re.fullmatch(rb"[A-Za-z ]{8}", src[at:at + 8]) else b"qjxzvkwq"


def occurrences(dec: bytes, lit: bytes) -> int:
    """the positions at which lit occurs, overlapping occurrences included"""
    return sum(1 for _ in re.finditer(b"(?=" + re.escape(lit) + b")", dec))


def add_split(out: str, pairs):
    """the three scan kernels' rows of a trace's kernel statistics into the JSON"""
    with open(out) as f:
        res = json.load(f)
    res["split_command"] = SPLIT_COMMAND.format(mib=res["mib"], reps=res["reps"])
    res.setdefault("split", {"leg": "text_fcx7_b1048576", "unit": "ms per launch"})
    for pair in pairs:
        name, path = pair.split("=", 1)
        rows = {}
        with open(path, newline="") as f:
            for r in csv.DictReader(f):
                for k in ("k_rmap", "k_rentry", "k_rmark"):
                    if r["Name"].startswith(f"fcx::{k}("):
                        rows[k] = {"calls": int(r["Calls"]), "average_ms": round(float(r["AverageNs"]) / 1e6, 4),
                                   "min_ms": round(int(r["MinNs"]) / 1e6, 4), "max_ms": round(int(r["MaxNs"]) / 1e6, 4)}
        assert len(rows) == 3, (path, rows)
        rows["sum_of_averages_ms"] = round(sum(v["average_ms"] for v in rows.values()), 4)
        res["split"][name] = rows
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


class RegexBench(GrepBench):
    def ab_pair(self, base, other):
        r = {"set_ms": [], "regex_ms": []}   # the A/B rule: alternate three times
        for _ in range(3):
            r["set_ms"].append(round(self.once(base), 4))
            r["regex_ms"].append(round(self.once(other), 4))
        lo, hi = min(r["set_ms"]), max(r["set_ms"])
        r["band_ms"] = [round(lo - (hi - lo), 4), round(hi + (hi - lo), 4)]
        r["regex_inside"] = [r["band_ms"][0] <= v <= r["band_ms"][1] for v in r["regex_ms"]]
        return r

    def checked(self, run, dec, expr, py_expr, states, hits=None):
        """a regex, its call compared with the model before it is timed"""
        torch, dc, sid, mc = self.torch, self.dc, self.sid, self.mc
        s, e, ln, nsel = model(dec, py_expr)
        rx = mc.Regex(expr)
        assert states is None or rx.info()["states"] == states, rx.info()
        B = len(s)
        arr = [torch.zeros(max(B, 1), dtype=torch.int64, device=self.dev) for _ in range(3)]
        st = dc.grep_regex_blocks_shard(*run, rx, d_start=arr[0].data_ptr(), d_end=arr[1].data_ptr(), d_line=arr[2].data_ptr(), cap=B,
                                        stream=sid)
        assert (st["blocks"], st["lines"], st["base_lines"], st["bytes"]) == (B, nsel, nsel, int((e - s).sum())), "not the model's totals"
        assert (st["judged"], st["decoded"]) == (len(dec), len(dec)) and (hits is None or st["hits"] == hits), "not the model's totals"
        for got, want in zip(arr, (s, e, ln)):
            assert got[:B].cpu().numpy().tolist() == want.tolist(), "not the model's blocks"
        return rx, {"states": rx.info()["states"], "classes": rx.info()["classes"], "blocks": B, "lines": nsel, "hits": st["hits"]}

    def row(self, host, d_plain, n, fmt, block):
        dc, sid, mc = self.dc, self.sid, self.mc
        nb = (n + block - 1) // block
        d_rec, m = self.records(d_plain, n, fmt, block)
        dec = self.decoded(d_rec, m, nb, fmt, n)
        src = dec if len(dec) >= 1 << 16 else bytes(memoryview(host.numpy())[:1 << 16])
        run = (fmt, d_rec.data_ptr(), m, nb)
        row = {"records": nb, "compressed_bytes": m, "decoded_bytes": len(dec), "states": {}}
        # 1. a literal against the one-pattern set
        lit = literal_of(src)
        rx, info = self.checked(run, dec, lit, lit, None, hits=occurrences(dec, lit))
        ps = mc.PatternSet([lit])
        rcall = lambda: dc.grep_regex_blocks_shard(*run, rx, stream=sid)
        scall = lambda: dc.grep_blocks_shard(*run, ps, DELIM, stream=sid)
        a, b = rcall(), scall()[0]
        assert all(a[k] == b[k] for k in a if k != "judged"), (a, b)
        info.update({"regex": self.timed(rcall), "set": self.timed(scall), "ab": self.ab_pair(scall, rcall),
                     "regex_stages_ms": self.staged(rcall), "set_stages_ms": self.staged(scall)})
        info["regex_over_set"] = round(info["regex"]["median_ms"] / info["set"]["median_ms"], 4)
        row["literal"] = info
        rx.close()
        ps.close()
        # 2. the scan with the number of states
        for expr, py_expr, states in STATES:
            rx, info = self.checked(run, dec, expr, py_expr, states)
            call = lambda rx=rx: dc.grep_regex_blocks_shard(*run, rx, stream=sid)
            info["call"] = self.timed(call)
            info["stages_ms"] = self.staged(call)
            dms = info["stages_ms"].get("decode")
            info["scan_over_decode"] = round(info["stages_ms"]["scan"] / dms, 4) if dms else None
            row["states"][f"S{states}"] = info
            rx.close()
        s4, s64 = row["states"]["S4"]["stages_ms"]["scan"], row["states"]["S64"]["stages_ms"]["scan"]
        row["scan_S64_over_S4"] = round(s64 / s4, 4) if s4 else None
        return row

    def split(self, host, d_plain, n, fmt, block, which):
        """nothing but reps calls of one expression, for a kernel trace around the process"""
        nb = (n + block - 1) // block
        d_rec, m = self.records(d_plain, n, fmt, block)
        run = (fmt, d_rec.data_ptr(), m, nb)
        expr = literal_of(self.decoded(d_rec, m, nb, fmt, n)) if which == "literal" else {f"S{s}": e for e, _py, s in STATES}[which]
        rx = self.mc.Regex(expr)
        for _ in range(self.a.reps):
            self.dc.grep_regex_blocks_shard(*run, rx, stream=self.sid)
        rx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mib", type=int, default=256)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--commit", default="unknown", help="the commit measured, for the record")
    ap.add_argument("--out", default=None)
    ap.add_argument("--split", choices=["literal"] + [f"S{s}" for _e, _p, s in STATES], help="the text FCX7 1 MiB leg alone, one expression, for a kernel trace")
    ap.add_argument("--add-split", action="append", default=[], metavar="X=CSV", help="a trace's kernel statistics into the JSON of --out")
    a = ap.parse_args()
    assert a.reps >= 10, "the median of at least 10 runs"
    if a.add_split:
        add_split(a.out, a.add_split)
        return
    b = RegexBench(a)
    n = a.mib << 20
    if a.split:
        host, d_plain = b.plain("text", 3, n)
        b.split(host, d_plain, n, "7", 1 << 20, a.split)
        b.dc.close()
        return
    res = {"mib": a.mib, "reps": a.reps, "warmup": a.warmup, "commit": a.commit,
           "command": f"python tools/regexbench.py --mib {a.mib} --reps {a.reps} --warmup {a.warmup}",
           "timer": "device events around each call (median); the calls synchronise their stream",
           "device": b.torch.cuda.get_device_name(0), "regex": {}}
    for kind, seed in LEGS:
        host, d_plain = b.plain(kind, seed, n)
        for fmt, block in FORMATS:
            key = f"{kind}_fcx{fmt}_b{block}"
            res["regex"][key] = b.row(host, d_plain, n, fmt, block)
            print("regex", key, json.dumps(res["regex"][key]), flush=True)
            if a.out:   # (kept leg by leg: a long run leaves what it has)
                with open(a.out, "w") as f:
                    json.dump(res, f, indent=1)
                    f.write("\n")
        del d_plain, host
    b.dc.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
