#!/usr/bin/env python3
"""Timing of the round-trip verification against the full decode and the index, on device-resident runs.

Per leg (rand, text: the bench legs' streams and seeds) and per format (FCX7 at 1 MiB and 64 KiB
blocks, FCX8 at 1 MiB), all in one process on records compressed once by the GPU codec:

  full      fcx_decompress_shard / fcx_lz78_decompress_shard of the whole run;
  index     fcx_index_shard alone;
  verify    fcx_verify_shard of the run against the bytes that were compressed (index + the full decode
            in groups of <= 256 MiB + the compare pass + the summary).

Each figure is the median of --reps calls after --warmup calls, timed with device events around
the call on the stream the call runs on; the calls synchronise the stream themselves, so this is
the time of the call, launch gaps included.  One more verify call runs with the context's profiling
on and gives the stages (index, decode, compare, summary: device events around each, summed over
the groups); `compare_share_of_decode` is its compare time over its decode time.  `over_budget` says
whether verify took more than index + full + 25 % of full.  Before anything is timed the verdict is
checked against a comparison of the full decode with the input by torch.  Needs a GPU: there is no
fallback.

--group-mib sets the bound of a group's decoded bytes (fcx_dctx_set_verify_group) for the whole run.

  python tools/verifybench.py [--mib 1024] [--reps 10] [--warmup 2] [--group-mib 0] [--commit ID] [--out profiles/verify.json]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

LEGS = (("rand", 4), ("text", 3))
FORMATS = (("7", 1 << 20), ("7", 1 << 16), ("8", 1 << 20))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mib", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--commit", default="unknown", help="the commit measured, for the record")
    ap.add_argument("--group-mib", type=int, default=0, help="bound of a group's decoded bytes (0: the default, 256 MiB)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert a.reps >= 10, "the median of at least 10 runs"

    import torch

    import inputs
    import my_compress_amd as mc

    assert torch.cuda.is_available(), "verifybench needs a GPU"
    dev = torch.device("cuda:0")
    n = a.mib << 20
    sid = torch.cuda.current_stream().cuda_stream
    dc = mc.DContext(0)
    dc.set_verify_group(a.group_mib << 20)

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

    res = {"mib": a.mib, "reps": a.reps, "warmup": a.warmup, "commit": a.commit, "group_mib": a.group_mib or 256,
           "device": torch.cuda.get_device_name(0),
           # (what was measured; where the result was written is not part of it)
           "command": f"python tools/verifybench.py --mib {a.mib} --reps {a.reps} --warmup {a.warmup}" +
                      (f" --group-mib {a.group_mib}" if a.group_mib else ""),
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
            d_pairs = torch.zeros(2 * nb, dtype=torch.int32, device=dev)
            total = full()
            index = lambda: dc.index_shard(d_rec.data_ptr(), m, nb, fmt, d_idx.data_ptr(), d_idx[nb + 1:].data_ptr(), sid)
            verify = lambda: dc.verify_shard(d_rec.data_ptr(), m, nb, fmt, d_plain.data_ptr(), n, block,
                                             d_pairs.data_ptr(), sid)
            assert index() == total
            st = verify()
            assert st["blocks"] == nb and st["decoded"] == total
            if total == n and n % block == 0:   # every record full size: the verdict against torch's comparison
                bad = int((d_back[:n].view(nb, block) != d_plain.view(nb, block)).any(dim=1).sum().item())
                assert st["differ"] == bad, f"{kind} FCX{fmt} b{block}: {st['differ']} blocks differ, torch says {bad}"
            row = {"records": nb, "compressed_bytes": m, "decoded_bytes": total, "stats": st, "groups": dc.verify_groups(),
                   "full": timed(full), "index": timed(index), "verify": timed(verify)}
            dc.set_profiling(True)
            verify()
            row["verify_stages_ms"] = {name: round(ms, 4) for name, ms in dc.stage_times()}
            dc.set_profiling(False)
            sg = row["verify_stages_ms"]
            row["compare_share_of_decode"] = round(sg["compare"] / sg["decode"], 4) if sg["decode"] else None
            f, i, v = (row[k]["median_ms"] for k in ("full", "index", "verify"))
            row["verify_over_index_plus_full"] = round(v / (i + f), 4)
            row["over_budget"] = v > i + 1.25 * f
            key = f"fcx{fmt}_b{block}"
            res["legs"].setdefault(kind, {})[key] = row
            print(kind, key, json.dumps(row), flush=True)
            del d_rec, d_back, d_idx, d_pairs
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
