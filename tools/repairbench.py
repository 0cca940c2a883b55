#!/usr/bin/env python3
"""Timing of the repair sidecar's device calls against the verification and the full decode, on
device-resident runs (the legs of tools/verifybench.py: rand and text, FCX7 at 1 MiB and 64 KiB blocks,
FCX8 at 1 MiB), plus rand at 4 KiB blocks, where most blocks are lost.

Per leg and format, in one process on records compressed once by the GPU codec:

  full      fcx_decompress_shard / fcx_lz78_decompress_shard of the whole run;
  index     fcx_index_shard alone;
  verify    fcx_verify_shard;
  build     fcx_repair_build_shard into buffers of the size its size query gave;
  apply     fcx_repair_apply_shard with that repair.

Each figure is the median of --reps calls after --warmup calls, device events around the call (the calls
synchronise their stream).  One more build and apply run with the context's profiling on and give the
stage tables.  Before anything is timed the applied output is compared with the input by torch.  Needs a
GPU: there is no fallback.

The gate (--gate PARENT_LIB): on the runs without entries, fcx_repair_apply_shard of this tree's library
(N) against fcx_index_shard + the full decode into the same buffers with the parent commit's library (P),
each sample a fresh process, alternating P N P N P N.  Every N median must lie inside P's min-max range
widened by that range's width on each side.

  python tools/repairbench.py [--mib 1024] [--reps 10] [--warmup 2] [--gate PARENT_LIB] [--commit ID] [--out profiles/repair.json]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

LEGS = (("rand", 4), ("text", 3))
FORMATS = (("7", 1 << 20), ("7", 1 << 16), ("8", 1 << 20))
GATE_RUNS = (("rand", "7", 1 << 20), ("text", "7", 1 << 20), ("text", "7", 1 << 16), ("text", "8", 1 << 20))   # no entries
LOST = ("rand", 4, "7", 4096, 64)   # most blocks lost: leg, seed, format, block, MiB (262144 records a GiB: 64 MiB of it at most)


class Bench:
    def __init__(self, a):
        import torch

        import my_compress_amd as mc

        assert torch.cuda.is_available(), "repairbench needs a GPU"
        self.a, self.torch, self.mc = a, torch, mc
        self.dev = torch.device("cuda:0")
        self.sid = torch.cuda.current_stream().cuda_stream
        self.dc = mc.DContext(0)

    def timed(self, fn):
        torch, a = self.torch, self.a
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

    def plain(self, kind, seed, n):
        import inputs

        host = self.torch.empty(n, dtype=self.torch.uint8).pin_memory()
        inputs.generate_into(kind, seed, host.data_ptr(), n)
        return host.to(self.dev)

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

    def calls(self, d_rec, m, n, fmt, block):
        """the parent's two calls into the buffers the apply uses: (index + full decode, d_back)"""
        torch, dc, sid = self.torch, self.dc, self.sid
        nb = (n + block - 1) // block
        d_back = torch.zeros(n + 64, dtype=torch.uint8, device=self.dev)
        d_idx = torch.zeros(2 * (nb + 1), dtype=torch.int64, device=self.dev)
        dec = dc.decompress_shard if fmt == "7" else dc.decompress_lz78_shard
        full = lambda: dec(d_rec.data_ptr(), m, nb, d_back.data_ptr(), n + 64, sid)
        index = lambda: dc.index_shard(d_rec.data_ptr(), m, nb, fmt, d_idx.data_ptr(), d_idx[nb + 1:].data_ptr(), sid)
        return full, index, d_back, d_idx

    def row(self, d_plain, n, fmt, block):
        torch, dc, sid = self.torch, self.dc, self.sid
        nb = (n + block - 1) // block
        d_rec, m = self.records(d_plain, n, fmt, block)
        full, index, d_back, d_idx = self.calls(d_rec, m, n, fmt, block)
        d_ent = torch.zeros(32 * nb, dtype=torch.uint8, device=self.dev)
        args = (d_rec.data_ptr(), m, nb, fmt, d_plain.data_ptr(), n, block)
        _, ne, nd, st = dc.repair_build_shard(*args, d_ent.data_ptr(), 0, 0, sid)   # the size query
        d_data = torch.zeros(max(nd, 16), dtype=torch.uint8, device=self.dev)
        build = lambda: dc.repair_build_shard(*args, d_ent.data_ptr(), d_data.data_ptr(), nd, sid)
        apply = lambda: dc.repair_apply_shard(d_rec.data_ptr(), m, nb, fmt, n, block, d_ent.data_ptr(), ne, d_data.data_ptr(),
                                              nd, d_back.data_ptr(), n + 64, sid)
        verify = lambda: dc.verify_shard(*args, 0, sid)
        assert build()[:3] == (0, ne, nd) and apply() == n
        assert torch.equal(d_back[:n], d_plain), f"FCX{fmt} b{block}: the repaired output is not the input"
        row = {"records": nb, "compressed_bytes": m, "entries": ne, "data_bytes": nd, "differ": st["differ"],
               "sidecar_bytes": 16 + 40 + 32 * ne + nd + 16 * len({int(b) >> 8 for b in
                                                                   d_ent[:32 * ne].view(torch.int64)[::4].tolist()}),
               "full": self.timed(full), "index": self.timed(index), "verify": self.timed(verify),
               "build": self.timed(build), "apply": self.timed(apply)}
        dc.set_profiling(True)
        build()
        row["build_stages_ms"] = {name: round(ms, 4) for name, ms in dc.stage_times()}
        apply()
        row["apply_stages_ms"] = {name: round(ms, 4) for name, ms in dc.stage_times()}
        dc.set_profiling(False)
        row["repair_stats"] = dc.repair_stats()
        row["build_over_verify"] = round(row["build"]["median_ms"] / row["verify"]["median_ms"], 4)
        row["apply_over_index_plus_full"] = round(row["apply"]["median_ms"] /
                                                  (row["index"]["median_ms"] + row["full"]["median_ms"]), 4)
        return row


def sample(a):
    """one gate sample, in this process: P the parent's calls, N the apply without entries"""
    b = Bench(a)
    n = a.mib << 20
    out = {}
    cache = {}
    for kind, fmt, block in GATE_RUNS:
        if kind not in cache:
            cache.clear()
            cache[kind] = b.plain(kind, dict(LEGS)[kind], n)
        d_plain = cache[kind]
        nb = (n + block - 1) // block
        d_rec, m = b.records(d_plain, n, fmt, block)
        full, index, d_back, d_idx = b.calls(d_rec, m, n, fmt, block)
        if a.sample == "P":
            fn = lambda: (index(), full())
        else:
            assert b.dc.repair_build_shard(d_rec.data_ptr(), m, nb, fmt, d_plain.data_ptr(), n, block, 0, 0, 0, b.sid)[1] == 0
            fn = lambda: b.dc.repair_apply_shard(d_rec.data_ptr(), m, nb, fmt, n, block, 0, 0, 0, 0, d_back.data_ptr(),
                                                 n + 64, b.sid)
        fn()
        assert b.torch.equal(d_back[:n], d_plain)
        out[f"{kind}_fcx{fmt}_b{block}"] = b.timed(fn)["median_ms"]
        del d_rec, d_back, d_idx
    print("SAMPLE " + json.dumps(out), flush=True)


def gate(a):
    order, runs = "PNPNPN", []
    for side in order:
        env = dict(os.environ)
        if side == "P":
            env["FCX_LIB"] = os.path.abspath(a.gate)
        else:
            env.pop("FCX_LIB", None)
        cmd = [sys.executable, os.path.abspath(__file__), "--sample", side, "--mib", str(a.mib), "--reps", str(a.reps),
               "--warmup", str(a.warmup)]
        r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900)
        line = [x for x in r.stdout.splitlines() if x.startswith("SAMPLE ")]
        assert r.returncode == 0 and line, r.stdout[-2000:] + r.stderr[-2000:]
        runs.append((side, json.loads(line[0][7:])))
        print(side, line[0], flush=True)
    # "inside": the rule as it stands; "slower": an N above the allowed range, which is what the rule guards
    # against (an N below the range is outside it too, and is reported as such: it is faster than every P)
    res = {"order": order, "rule": "every N inside [min P - w, max P + w], w = max P - min P", "runs": {}, "inside": True,
           "slower": False}
    for key in runs[0][1]:
        p = [v[key] for s, v in runs if s == "P"]
        nn = [v[key] for s, v in runs if s == "N"]
        w = max(p) - min(p)
        lo, hi = min(p) - w, max(p) + w
        res["runs"][key] = {"P_ms": p, "N_ms": nn, "allowed_ms": [round(lo, 4), round(hi, 4)],
                            "inside": all(lo <= x <= hi for x in nn), "above": [x for x in nn if x > hi],
                            "below": [x for x in nn if x < lo]}
        res["inside"] = res["inside"] and res["runs"][key]["inside"]
        res["slower"] = res["slower"] or bool(res["runs"][key]["above"])
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mib", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--commit", default="unknown", help="the commit measured, for the record")
    ap.add_argument("--gate", default=None, metavar="PARENT_LIB", help="the parent commit's libfcx.so: run the gate too")
    ap.add_argument("--sample", default=None, choices=["P", "N"], help="(internal) one gate sample in this process")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert a.reps >= 10, "the median of at least 10 runs"
    if a.sample:
        return sample(a)
    res = {"mib": a.mib, "reps": a.reps, "warmup": a.warmup, "commit": a.commit,
           "command": f"python tools/repairbench.py --mib {a.mib} --reps {a.reps} --warmup {a.warmup}" +
                      (" --gate PARENT_LIB" if a.gate else ""),
           "timer": "device events around each call (median); the calls synchronise their stream", "legs": {}}
    if a.gate:   # first, before this process holds the device's memory
        res["gate"] = gate(a)
    b = Bench(a)
    res["device"] = b.torch.cuda.get_device_name(0)
    n = a.mib << 20
    for kind, seed in LEGS:
        d_plain = b.plain(kind, seed, n)
        for fmt, block in FORMATS:
            row = b.row(d_plain, n, fmt, block)
            res["legs"].setdefault(kind, {})[f"fcx{fmt}_b{block}"] = row
            print(kind, f"fcx{fmt}_b{block}", json.dumps(row), flush=True)
        del d_plain
    # (the GPU decoder refuses some streams the reference would decode; a run that holds
    # such a record cannot be verified or repaired, so the size is lowered until the run decodes)
    kind, seed, fmt, block, mib = LOST
    refused = {}
    for mib in (m for m in (mib, mib // 4, mib // 16, 1) if m <= a.mib):
        try:
            row = b.row(b.plain(kind, seed, mib << 20), mib << 20, fmt, block)
        except b.mc.FcxError as e:
            refused[f"{mib} MiB"] = str(e)
            continue
        row["mib"] = mib
        row["refused_at"] = refused
        res["legs"][kind][f"fcx{fmt}_b{block}"] = row
        print(kind, f"fcx{fmt}_b{block}", json.dumps(row), flush=True)
        break
    b.dc.close()
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
