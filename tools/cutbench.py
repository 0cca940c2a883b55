#!/usr/bin/env python3
"""Timing of the cut's device calls, on device-resident runs, beside the decode stage of the same call
and the count stage of fcx_lines_index_shard on the same file.

  legs      those of tools/grepbench.py (rand and text, FCX7 at 1 MiB and 64 KiB blocks, FCX8 at 1 MiB), delimiter
            0x0A.  Per leg: fcx_cut_shard with the fields list 2 and the separator 0x20, with the byte list 1-16, and
            the size query of the first (no gather); the whole call and its stage table (index, decode, cut, summary);
            the cut stage against the decode stage, and against the count stage of fcx_lines_index_shard (one read of
            the group, where the cut reads it three times and writes the kept bytes once).
  --kernels one leg's cut calls alone, a few times and untimed: for a kernel trace of its own
            (rocprofv3 --kernel-trace --stats -- python tools/cutbench.py --kernels), which splits the cut stage by
            kernel.

Each figure is the median of --reps calls after --warmup calls, device events around the call (the calls synchronise
their stream).  Before anything is timed every output is compared with cut_model's numpy form over the full decoder's
bytes on the host, taken in pieces that end at a delimiter.  Needs a GPU: there is no fallback.

  python tools/cutbench.py [--mib 256] [--reps 10] [--warmup 2] [--commit ID] [--out profiles/cut.json]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import cut_model as km   # noqa: E402
from grepbench import FORMATS, LEGS, Bench   # noqa: E402  (grepbench's helpers: the legs and the timing of findbench)

DELIM, SEP = 0x0A, 0x20
SPECS = {"fields_2": ("2", None), "bytes_1_16": (None, "1-16")}
PIECE = 16 << 20


def model(dec: bytes, fields, byte_list):
    """(the cut's bytes, the five stats) by the rule in numpy, over pieces that end at a delimiter: a column never
    depends on the lines before its own"""
    mode, sel = km.make_sel(fields, byte_list)
    out, st, at = [], [0] * 5, 0
    while at < len(dec):
        end = min(at + PIECE, len(dec))
        if end < len(dec):
            end = dec.find(bytes([DELIM]), end - 1) + 1 or len(dec)
        o, s = km.cut_np(dec[at:end], sel, mode, SEP, DELIM)
        out.append(o)
        st = [a + b for a, b in zip(st, s)]
        at = end
    return b"".join(out), st


class CutBench(Bench):
    def row(self, d_plain, n, fmt, block, check=True):
        torch, dc, sid = self.torch, self.dc, self.sid
        nb = (n + block - 1) // block
        d_rec, m = self.records(d_plain, n, fmt, block)
        dec = self.decoded(d_rec, m, nb, fmt, n)
        run = (fmt, d_rec.data_ptr(), m, nb)
        d_out = torch.empty(len(dec) + 64, dtype=torch.uint8, device=self.dev)
        row = {"records": nb, "compressed_bytes": m, "decoded_bytes": len(dec)}
        calls = {}
        for name, (fields, byte_list) in SPECS.items():
            ct = self.mc.Cut(fields, byte_list, bytes([SEP]), bytes([DELIM]))
            self.cuts.append(ct)
            calls[name] = lambda ct=ct: dc.cut_shard(*run, ct, d_out.data_ptr(), len(dec), sid)
            if name == "fields_2":
                calls["fields_2_size_query"] = lambda ct=ct: dc.cut_shard(*run, ct, 0, 0, sid)
            if check:
                want, st = model(dec, fields, byte_list)
                total, got = calls[name]()
                assert total == len(want) and [got[k] for k in dc.CUT_STATS[:5]] == st, (name, total, got, st)
                assert d_out[:total].cpu().numpy().tobytes() == want, "not the model's bytes"
                row[name + "_stats"] = got
        if not self.a.kernels:
            lines = lambda: dc.lines_index_shard(*run, DELIM, 0, sid)
            row["lines_index"] = self.timed(lines)
            row["lines_index_stages_ms"] = self.staged(lines)
            for name, fn in calls.items():
                row[name] = self.timed(fn)
                st = row[name + "_stages_ms"] = self.staged(fn)
                if st.get("decode"):
                    row[name + "_cut_over_decode"] = round(st["cut"] / st["decode"], 4)
                if row["lines_index_stages_ms"].get("count"):
                    row[name + "_cut_over_count"] = round(st["cut"] / row["lines_index_stages_ms"]["count"], 4)
            row["scratch_bytes"] = dc.cut_scratch()
        else:
            for fn in calls.values():
                for _ in range(5):
                    fn()
        return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mib", type=int, default=256)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--commit", default="unknown", help="the commit measured, for the record")
    ap.add_argument("--kernels", action="store_true", help="the text leg at FCX7 and 1 MiB blocks alone, untimed: for a kernel trace")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert a.reps >= 10, "the median of at least 10 runs"
    b = CutBench(a)
    b.cuts = []
    res = {"mib": a.mib, "reps": a.reps, "warmup": a.warmup, "commit": a.commit,
           "command": f"python tools/cutbench.py --mib {a.mib} --reps {a.reps} --warmup {a.warmup}",
           "timer": "device events around each call (median); the calls synchronise their stream",
           "device": b.torch.cuda.get_device_name(0), "cut": {}}
    n = a.mib << 20
    for kind, seed in LEGS:
        if a.kernels and kind != "text":
            continue
        host, d_plain = b.plain(kind, seed, n)
        for fmt, block in FORMATS[:1] if a.kernels else FORMATS:
            key = f"{kind}_fcx{fmt}_b{block}"
            res["cut"][key] = b.row(d_plain, n, fmt, block, check=not a.kernels)
            print("cut", key, json.dumps(res["cut"][key]), flush=True)
        del d_plain, host
    for ct in b.cuts:
        ct.close()
    b.dc.close()
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
