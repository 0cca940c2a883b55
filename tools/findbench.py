#!/usr/bin/env python3
"""Timing of the search's device call, on device-resident runs, beside fcx_check_shard.

  legs      those of tools/digestbench.py's check (rand and text, FCX7 at 1 MiB and 64 KiB blocks, FCX8 at
            1 MiB), records compressed once by the GPU codec.  Per leg: fcx_find_shard for an 8-byte pattern
            cut from the data (the count alone, and with room for every hit) and fcx_check_shard of the same
            run, each with its stage table (one more call with the context's profiling on); the scan stage
            over the digest stage; and the A/B rule: check and find alternated three times, each find value
            against check's min-max range widened by its width on each side.
  zeros     FCX8 at 1 MiB, a pattern of 256 zero bytes: every position a candidate, the full compare everywhere.

Each figure is the median of --reps calls after --warmup calls, device events around the call (the calls
synchronise their stream).  Before anything is timed the hits are compared with bytes.find over the full
decoder's bytes on the host.  Needs a GPU: there is no fallback.

  python tools/findbench.py [--mib 1024] [--reps 10] [--warmup 2] [--commit ID] [--out profiles/find.json]
"""
import argparse
import json
import os
import statistics
import sys
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

LEGS = (("rand", 4), ("text", 3))
FORMATS = (("7", 1 << 20), ("7", 1 << 16), ("8", 1 << 20))


class Bench:
    def __init__(self, a):
        import torch

        import my_compress_amd as mc

        assert torch.cuda.is_available(), "findbench needs a GPU"
        self.a, self.torch, self.mc = a, torch, mc
        self.dev = torch.device("cuda:0")
        self.sid = torch.cuda.current_stream().cuda_stream
        self.dc = mc.DContext(0)

    def once(self, fn):
        torch = self.torch
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    def timed(self, fn):
        for _ in range(self.a.warmup):
            fn()
        ms = [self.once(fn) for _ in range(self.a.reps)]
        return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4)}

    def staged(self, fn):
        self.dc.set_profiling(True)
        fn()
        st = {name: round(ms, 4) for name, ms in self.dc.stage_times()}
        self.dc.set_profiling(False)
        return st

    def plain(self, kind, seed, n):
        import inputs

        host = self.torch.empty(n, dtype=self.torch.uint8).pin_memory()
        inputs.generate_into(kind, seed, host.data_ptr(), n)
        return host, host.to(self.dev)

    def records(self, d_plain, n, fmt, block):
        torch, mc = self.torch, self.mc
        if fmt == "7":
            cap = mc.shard_bound(n, block)
            d_rec = torch.empty(cap, dtype=torch.uint8, device=self.dev)
            ctx = mc.Context(0, block, n)
            m = ctx.compress_shard(d_plain.data_ptr(), n, d_rec.data_ptr(), cap, self.sid)
            ctx.close()
        else:
            cap = mc.lz78_bound(n, block)
            d_rec = torch.empty(cap, dtype=torch.uint8, device=self.dev)
            m = mc.lz78_compress_shard(d_plain.data_ptr(), n, block, d_rec.data_ptr(), cap, self.sid)
            mc.lz78_release()
        return d_rec, m

    def decoded(self, d_rec, m, nb, fmt, n):
        """the full decoder's bytes on the host"""
        d_out = self.torch.empty(n + nb * 8 + 64, dtype=self.torch.uint8, device=self.dev)
        fn = self.dc.decompress_shard if fmt == "7" else self.dc.decompress_lz78_shard
        got = fn(d_rec.data_ptr(), m, nb, d_out.data_ptr(), d_out.numel(), self.sid)
        return d_out[:got].cpu().numpy().tobytes()

    def row(self, host, d_plain, n, fmt, block, pattern=None):
        torch, dc, sid = self.torch, self.dc, self.sid
        nb = (n + block - 1) // block
        d_rec, m = self.records(d_plain, n, fmt, block)
        dec = self.decoded(d_rec, m, nb, fmt, n)
        if pattern is None:   # 8 bytes of the decoded data, or of the input when nothing decodes
            src = dec if len(dec) >= 16 else bytes(memoryview(host.numpy())[:4096])
            pattern = src[len(src) // 2:len(src) // 2 + 8]
        ndec = len(dec)
        if dec.count(0) == ndec and pattern.count(0) == len(pattern):   # zeros in zeros: every position
            want = range(max(ndec - len(pattern) + 1, 0))
        else:
            want, i = [], dec.find(pattern)
            while i >= 0:
                want.append(i)
                i = dec.find(pattern, i + 1)
        del dec
        mv = memoryview(host.numpy())
        d_crc = torch.tensor([zlib.crc32(mv[o:o + block]) for o in range(0, n, block)], dtype=torch.int64).to(torch.int32).to(self.dev)
        fargs = (fmt, d_rec.data_ptr(), m, nb, pattern)
        d_hits = torch.zeros(max(len(want), 1), dtype=torch.int64, device=self.dev)
        count = lambda: dc.find_shard(*fargs, 0, 0, sid)
        find = lambda: dc.find_shard(*fargs, d_hits.data_ptr(), d_hits.numel(), sid)
        check = lambda: dc.check_shard(d_rec.data_ptr(), m, nb, fmt, n, block, d_crc.data_ptr(), 0, 0, 0, 0, 0, sid)
        assert count() == len(want) and find() == len(want), "not the host search's count"
        if isinstance(want, range):
            assert bool((d_hits[:len(want)] == torch.arange(len(want), device=self.dev)).all()), "not every position in order"
        else:
            assert d_hits[:len(want)].tolist() == want, "not the host search's offsets"
        fstats = dc.find_stats()
        row = {"records": nb, "compressed_bytes": m, "decoded_bytes": ndec,
               "pattern_bytes": len(pattern), "hits": len(want), "find_stats": fstats,
               "find": self.timed(find), "find_count_only": self.timed(count), "check": self.timed(check)}
        row["find_stages_ms"] = self.staged(find)
        row["check_stages_ms"] = self.staged(check)
        dg = row["check_stages_ms"]["digest"]
        row["scan_over_digest"] = round(row["find_stages_ms"]["scan"] / dg, 4) if dg else None
        row["find_over_check"] = round(row["find"]["median_ms"] / row["check"]["median_ms"], 4)
        ab = {"check_ms": [], "find_ms": []}   # the A/B rule: alternate three times
        for _ in range(3):
            ab["check_ms"].append(round(self.once(check), 4))
            ab["find_ms"].append(round(self.once(find), 4))
        lo, hi = min(ab["check_ms"]), max(ab["check_ms"])
        ab["band_ms"] = [round(lo - (hi - lo), 4), round(hi + (hi - lo), 4)]
        ab["find_inside"] = [ab["band_ms"][0] <= v <= ab["band_ms"][1] for v in ab["find_ms"]]
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
    assert a.reps >= 10, "the median of at least 10 runs"
    b = Bench(a)
    res = {"mib": a.mib, "reps": a.reps, "warmup": a.warmup, "commit": a.commit,
           "command": f"python tools/findbench.py --mib {a.mib} --reps {a.reps} --warmup {a.warmup}",
           "timer": "device events around each call (median); the calls synchronise their stream",
           "device": b.torch.cuda.get_device_name(0), "find": {}}
    n = a.mib << 20
    for kind, seed in LEGS:
        host, d_plain = b.plain(kind, seed, n)
        for fmt, block in FORMATS:
            key = f"{kind}_fcx{fmt}_b{block}"
            res["find"][key] = b.row(host, d_plain, n, fmt, block)
            print("find", key, json.dumps(res["find"][key]), flush=True)
        del d_plain, host
    host, d_plain = b.plain("zeros", 0, n)
    res["find"]["zeros_fcx8_b1048576_all_candidates"] = b.row(host, d_plain, n, "8", 1 << 20, bytes(256))
    print("find zeros", json.dumps(res["find"]["zeros_fcx8_b1048576_all_candidates"]), flush=True)
    b.dc.close()
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
