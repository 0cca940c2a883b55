#!/usr/bin/env python3
"""Timing of the context grep's device call, on a device-resident text run, beside fcx_grep_set_shard of
the same library on the same run and pattern set.

  legs      text, FCX7 at 1 MiB blocks and FCX8 at 1 MiB, delimiter 0x0A, 8 patterns of 8 bytes cut from the data,
            every call count only.  Per leg the whole call and the stage table (index, decode, scan, select, summary)
            of fcx_grep_set_shard (the yardstick: decode and scan are shared) and of fcx_grep_blocks_shard with zero
            options, with the invert flag, and with before = after = 3.

Each whole-call figure is the median, minimum and maximum of --reps calls after --warmup calls, device events around
the call (the calls synchronise their stream); each stage figure likewise over --reps profiled calls.  Before
anything is timed the eight stats of every option are compared with the definitions of include/fcx.h in numpy over
the full decoder's bytes on the host.  Needs a GPU: there is no fallback.

  python tools/contextbench.py [--mib 256] [--reps 10] [--warmup 2] [--commit ID] [--out profiles/context.json]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from grepbench import DELIM, GrepBench   # noqa: E402
from setbench import cut   # noqa: E402

OPTIONS = {"zero": (False, 0, 0), "invert": (True, 0, 0), "context3": (False, 3, 3)}


def model(dec: bytes, patterns, invert: bool, before: int, after: int):
    """the eight stats by the definitions, in numpy over the decoder's bytes"""
    import numpy as np

    T, per = len(dec), []
    for p in patterns:
        h, i = [], dec.find(p)
        while i >= 0:
            h.append(i)
            i = dec.find(p, i + 1)
        per.append(np.array(h, dtype=np.int64))
    hits = np.unique(np.concatenate(per))
    dpos = np.flatnonzero(np.frombuffer(dec, dtype=np.uint8) == DELIM)
    bounds = np.concatenate(([0], dpos + 1, [T])).astype(np.int64)
    if len(bounds) > 1 and bounds[-1] == bounds[-2]:
        bounds = bounds[:-1]   # the file ends in a delimiter: no line behind it
    L = len(bounds) - 1
    base = np.zeros(L, dtype=bool)
    base[np.searchsorted(dpos, hits, side="left")] = True
    if invert:
        base = ~base
    c = np.concatenate(([0], np.cumsum(base)))
    j = np.arange(L)
    sel = c[np.minimum(j + before, L - 1) + 1] - c[np.maximum(j - after, 0)] > 0
    starts = sel & ~np.concatenate(([False], sel[:-1]))
    lens = np.diff(bounds)
    return {"blocks": int(starts.sum()), "lines": int(sel.sum()), "bytes": int(lens[sel].sum()), "base_lines": int(base.sum()),
            "hits": len(hits), "judged": max(T - min(map(len, patterns)) + 1, 0), "decoded": T, "total_lines": L}


class ContextBench(GrepBench):
    def staged_many(self, fn):
        runs = [self.staged(fn) for _ in range(self.a.reps)]
        return {k: {"median_ms": round(statistics.median(r[k] for r in runs), 4), "min_ms": min(r[k] for r in runs),
                    "max_ms": max(r[k] for r in runs)} for k in runs[0]}

    def row(self, host, d_plain, n, fmt, block):
        dc, sid = self.dc, self.sid
        nb = (n + block - 1) // block
        d_rec, m = self.records(d_plain, n, fmt, block)
        dec = self.decoded(d_rec, m, nb, fmt, n)
        run = (fmt, d_rec.data_ptr(), m, nb)
        pats = cut(dec, 8)
        ps = self.mc.PatternSet(pats)
        row = {"records": nb, "compressed_bytes": m, "decoded_bytes": len(dec), "patterns": len(pats)}
        grep = lambda: dc.grep_set_shard(*run, ps, DELIM, 0, 0, 0, sid)
        row["grep_set_shard"] = {"stats": grep()[0], "call": self.timed(grep), "stages": self.staged_many(grep)}
        for name, (inv, before, after) in OPTIONS.items():
            fn = lambda inv=inv, before=before, after=after: dc.grep_blocks_shard(*run, ps, DELIM, inv, before, after, stream=sid)
            st = fn()[0]
            assert st == model(dec, pats, inv, before, after), ("not the model's stats", name, st)
            row[name] = {"stats": st, "scratch_bytes": dc.grep_scratch(), "call": self.timed(fn), "stages": self.staged_many(fn)}
            row[name]["call_over_grep_set"] = round(row[name]["call"]["median_ms"] / row["grep_set_shard"]["call"]["median_ms"], 4)
        ps.close()
        return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mib", type=int, default=256)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--commit", default="unknown", help="the commit measured, for the record")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert a.reps >= 10, "the median of at least 10 runs"
    b = ContextBench(a)
    res = {"mib": a.mib, "reps": a.reps, "warmup": a.warmup, "commit": a.commit,
           "command": f"python tools/contextbench.py --mib {a.mib} --reps {a.reps} --warmup {a.warmup}",
           "timer": "device events around each call (median, min, max); the calls synchronise their stream",
           "device": b.torch.cuda.get_device_name(0), "context": {}}
    n = a.mib << 20
    host, d_plain = b.plain("text", 3, n)
    for fmt, block in (("7", 1 << 20), ("8", 1 << 20)):
        key = f"text_fcx{fmt}_b{block}"
        res["context"][key] = b.row(host, d_plain, n, fmt, block)
        print("context", key, json.dumps(res["context"][key]), flush=True)
        if a.out:   # (kept leg by leg: a long run leaves what it has)
            with open(a.out, "w") as f:
                json.dump(res, f, indent=1)
                f.write("\n")
    b.dc.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
