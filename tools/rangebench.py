#!/usr/bin/env python3
"""Timing of the random-access calls against the full decode, on device-resident runs.

Per leg (rand, text, runs: the bench legs' streams and seeds) and per format (FCX7 at 1 MiB and
64 KiB blocks, FCX8 at 1 MiB), all in one process on records compressed once by the GPU codec:

  full      fcx_decompress_shard / fcx_lz78_decompress_shard of the whole run (the baseline);
  index     fcx_index_shard alone;
  indexed   fcx_decompress_range_shard of 4 KiB, 1 MiB and 64 MiB at a mid-run offset, with that index;
  unindexed the same three ranges with no index (each call builds its own).

Each figure is the median of --reps calls after --warmup calls, timed with device events around
the call on the stream the call runs on; the calls synchronise the stream themselves, so this is
the time of the call, launch gaps included.  Every range is compared with the slice of the full
decode before it is timed.  Needs a GPU: there is no fallback.

  python tools/rangebench.py [--mib 1024] [--reps 10] [--warmup 2] [--commit ID] [--out profiles/range_decode.json]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

LEGS = (("rand", 4), ("text", 3), ("runs", 5))
FORMATS = (("7", 1 << 20), ("7", 1 << 16), ("8", 1 << 20))
RANGES = (4 << 10, 1 << 20, 64 << 20)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mib", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--commit", default="unknown", help="the commit measured, for the record")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert a.reps >= 10, "the median of at least 10 runs"

    import torch

    import inputs
    import my_compress_amd as mc

    assert torch.cuda.is_available(), "rangebench needs a GPU"
    dev = torch.device("cuda:0")
    n = a.mib << 20
    sid = torch.cuda.current_stream().cuda_stream
    dc = mc.DContext(0)

    def timed(fn):
        for _ in range(a.warmup):
            fn()
        ms = []
        for _ in range(a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4)}

    res = {"mib": a.mib, "reps": a.reps, "warmup": a.warmup, "commit": a.commit,
           "device": torch.cuda.get_device_name(0),
           # (what was measured; where the result was written is not part of it)
           "command": f"python tools/rangebench.py --mib {a.mib} --reps {a.reps} --warmup {a.warmup}",
           "timer": "device events around each call (median); the calls synchronise their stream", "legs": {}}
    host = torch.empty(n, dtype=torch.uint8).pin_memory()
    for kind, seed in LEGS:
        inputs.generate_into(kind, seed, host.data_ptr(), n)
        d_plain = host.to(dev)
        for fmt, block in FORMATS:
            nb = (n + block - 1) // block
            if fmt == "7":
                cap = mc.shard_bound(n, block)
                d_rec = torch.empty(cap, dtype=torch.uint8, device=dev)
                ctx = mc.Context(0, block, n)
                m = ctx.compress_shard(d_plain.data_ptr(), n, d_rec.data_ptr(), cap, sid)
                ctx.close()
                full = lambda: dc.decompress_shard(d_rec.data_ptr(), m, nb, d_back.data_ptr(), n + 64, sid)
            else:
                cap = mc.lz78_bound(n, block)
                d_rec = torch.empty(cap, dtype=torch.uint8, device=dev)
                m = mc.lz78_compress_shard(d_plain.data_ptr(), n, block, d_rec.data_ptr(), cap, sid)
                mc.lz78_release()
                full = lambda: dc.decompress_lz78_shard(d_rec.data_ptr(), m, nb, d_back.data_ptr(), n + 64, sid)
            d_back = torch.zeros(n + 64, dtype=torch.uint8, device=dev)
            d_idx = torch.zeros(2 * (nb + 1), dtype=torch.int64, device=dev)
            p_rec, p_dec = d_idx.data_ptr(), d_idx[nb + 1:].data_ptr()
            d_part = torch.zeros(max(RANGES) + 64, dtype=torch.uint8, device=dev)
            total = full()
            index = lambda: dc.index_shard(d_rec.data_ptr(), m, nb, fmt, p_rec, p_dec, sid)
            assert index() == total
            row = {"records": nb, "compressed_bytes": m, "decoded_bytes": total,
                   "full": timed(full), "index": timed(index), "indexed": {}, "unindexed": {}}
            off = total // 2 + 12345
            for ln in RANGES:
                for name, pr, pd in (("indexed", p_rec, p_dec), ("unindexed", 0, 0)):
                    call = lambda: dc.decompress_range_shard(d_rec.data_ptr(), m, nb, fmt, off, ln, d_part.data_ptr(),
                                                             ln, pr, pd, sid)
                    got_n = call()
                    assert got_n == min(ln, total - off) and torch.equal(d_part[:got_n], d_back[off:off + got_n]), \
                        f"{kind} FCX{fmt} b{block}: range ({off}, {ln}) differs from the full decode"
                    t = timed(call)
                    t["stats"] = dc.range_stats()
                    row[name][str(ln)] = t
            key = f"fcx{fmt}_b{block}"
            res["legs"].setdefault(kind, {})[key] = row
            print(kind, key, json.dumps(row), flush=True)
            del d_rec, d_back, d_idx, d_part
        del d_plain
    dc.close()
    line = json.dumps(res)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
    print(line)


if __name__ == "__main__":
    main()
