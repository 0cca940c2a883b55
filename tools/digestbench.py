#!/usr/bin/env python3
"""Timing of the content digest's device calls, on device-resident runs.

  digest    fcx_digest_shard over --mib MiB of rand, text and zeros at 1 MiB and 64 KiB blocks, with the
            slicing round of k_dgcrc at 4 (the default), 8 and 16 bytes: ms, and ms per GiB;
  check     on the legs of tools/repairbench.py (rand and text, FCX7 at 1 MiB and 64 KiB blocks, FCX8 at
            1 MiB), records compressed once by the GPU codec: fcx_check_shard without a repair and with the
            repair fcx_repair_build_shard makes, beside fcx_verify_shard, each with its stage table (one more
            call with the context's profiling on).  --parent-lib PARENT_LIB: fcx_verify_shard of the parent
            commit's library as well, in a process of its own on the same inputs.

Each figure is the median of --reps calls after --warmup calls, device events around the call (the calls
synchronise their stream).  Before anything is timed the values are compared with zlib's on the host and the
check's verdict with the verification's.  Needs a GPU: there is no fallback.

  python tools/digestbench.py [--mib 1024] [--reps 10] [--warmup 2] [--parent-lib PARENT_LIB] [--commit ID] [--out profiles/digest.json]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

DIGEST_LEGS = (("rand", 4), ("text", 3), ("zeros", 0))
CHECK_LEGS = (("rand", 4), ("text", 3))
BLOCKS = (1 << 20, 1 << 16)
FORMATS = (("7", 1 << 20), ("7", 1 << 16), ("8", 1 << 20))


class Bench:
    def __init__(self, a):
        import torch

        import my_compress_amd as mc

        assert torch.cuda.is_available(), "digestbench needs a GPU"
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

    def digest_row(self, host, d_plain, n, block):
        torch, dc = self.torch, self.dc
        nb = (n + block - 1) // block
        d_crc = torch.zeros(nb, dtype=torch.int32, device=self.dev)
        call = lambda: dc.digest_shard(d_plain.data_ptr(), n, block, d_crc.data_ptr(), self.sid, whole=False)
        mv = memoryview(host.numpy())
        want = [zlib.crc32(mv[o:o + block]) for o in range(0, n, block)]
        whole = zlib.crc32(mv)
        row = {"blocks": nb}
        for width in (4, 8, 16):
            dc.set_digest_slice(width)
            assert dc.digest_shard(d_plain.data_ptr(), n, block, d_crc.data_ptr(), self.sid) == whole
            assert [int(v) & 0xFFFFFFFF for v in d_crc.tolist()] == want, f"slice {width}: not zlib's values"
            t = self.timed(call)
            t["ms_per_gib"] = round(t["median_ms"] * (1 << 30) / n, 4)
            t["gb_per_s"] = round(n / t["median_ms"] / 1e6, 1)
            row[f"slice{width}"] = t
        dc.set_digest_slice(0)
        return row, d_crc

    def check_row(self, d_plain, n, fmt, block, d_crc):
        torch, dc, sid = self.torch, self.dc, self.sid
        nb = (n + block - 1) // block
        d_rec, m = self.records(d_plain, n, fmt, block)
        vargs = (d_rec.data_ptr(), m, nb, fmt, d_plain.data_ptr(), n, block)
        d_ent = torch.zeros(32 * nb, dtype=torch.uint8, device=self.dev)
        _, ne, nd, vst = dc.repair_build_shard(*vargs, d_ent.data_ptr(), 0, 0, sid)   # the size query
        d_data = torch.zeros(max(nd, 16), dtype=torch.uint8, device=self.dev)
        assert dc.repair_build_shard(*vargs, d_ent.data_ptr(), d_data.data_ptr(), nd, sid)[:3] == (0, ne, nd)
        cargs = (d_rec.data_ptr(), m, nb, fmt, n, block, d_crc.data_ptr())
        verify = lambda: dc.verify_shard(*vargs, 0, sid)
        check = lambda: dc.check_shard(*cargs, 0, 0, 0, 0, 0, sid)
        mended = lambda: dc.check_shard(*cargs, d_ent.data_ptr(), ne, d_data.data_ptr(), nd, 0, sid)
        st = check()
        assert (st["differ"], st["first"], st["bytes"]) == (vst["differ"], vst["first"], vst["bytes"]), (st, vst)
        assert mended()["differ"] == 0
        row = {"records": nb, "compressed_bytes": m, "entries": ne, "data_bytes": nd, "failing": st["differ"],
               "verify": self.timed(verify), "check": self.timed(check), "check_repaired": self.timed(mended)}
        row["verify_stages_ms"] = self.staged(verify)
        row["check_stages_ms"] = self.staged(check)
        row["check_repaired_stages_ms"] = self.staged(mended)
        row["check_over_verify"] = round(row["check"]["median_ms"] / row["verify"]["median_ms"], 4)
        row["digest_stage_ms_per_gib"] = round(row["check_stages_ms"]["digest"] * (1 << 30) / n, 4)
        row["compare_stage_ms_per_gib"] = round(row["verify_stages_ms"]["compare"] * (1 << 30) / n, 4)
        return row

    def verify_row(self, d_plain, n, fmt, block):
        """(--sample) the loaded library's fcx_verify_shard alone"""
        d_rec, m = self.records(d_plain, n, fmt, block)
        nb = (n + block - 1) // block
        verify = lambda: self.dc.verify_shard(d_rec.data_ptr(), m, nb, fmt, d_plain.data_ptr(), n, block, 0, self.sid)
        return {"verify": self.timed(verify), "verify_stages_ms": self.staged(verify)}


def sample(a):
    b = Bench(a)
    n = a.mib << 20
    out = {}
    for kind, seed in CHECK_LEGS:
        _, d_plain = b.plain(kind, seed, n)
        for fmt, block in FORMATS:
            out[f"{kind}_fcx{fmt}_b{block}"] = b.verify_row(d_plain, n, fmt, block)
        del d_plain
    print("SAMPLE " + json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mib", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--commit", default="unknown", help="the commit measured, for the record")
    ap.add_argument("--parent-lib", default=None, metavar="PARENT_LIB", help="the parent commit's libfcx.so: its fcx_verify_shard too")
    ap.add_argument("--sample", action="store_true", help="(internal) fcx_verify_shard of the loaded library, in this process")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert a.reps >= 10, "the median of at least 10 runs"
    if a.sample:
        return sample(a)
    res = {"mib": a.mib, "reps": a.reps, "warmup": a.warmup, "commit": a.commit,
           "command": f"python tools/digestbench.py --mib {a.mib} --reps {a.reps} --warmup {a.warmup}" +
                      (" --parent-lib PARENT_LIB" if a.parent_lib else ""),
           "timer": "device events around each call (median); the check and verify calls synchronise their stream",
           "digest": {}, "check": {}}
    if a.parent_lib:   # first, before this process holds the device's memory
        env = dict(os.environ, FCX_LIB=os.path.abspath(a.parent_lib))
        cmd = [sys.executable, os.path.abspath(__file__), "--sample", "--mib", str(a.mib), "--reps", str(a.reps),
               "--warmup", str(a.warmup)]
        r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900)
        line = [x for x in r.stdout.splitlines() if x.startswith("SAMPLE ")]
        assert r.returncode == 0 and line, r.stdout[-2000:] + r.stderr[-2000:]
        res["parent_verify"] = json.loads(line[0][7:])
        print("parent", line[0], flush=True)
    b = Bench(a)
    res["device"] = b.torch.cuda.get_device_name(0)
    n = a.mib << 20
    for kind, seed in DIGEST_LEGS:
        host, d_plain = b.plain(kind, seed, n)
        crcs = {}
        for block in BLOCKS:
            row, crcs[block] = b.digest_row(host, d_plain, n, block)
            res["digest"].setdefault(kind, {})[f"b{block}"] = row
            print("digest", kind, f"b{block}", json.dumps(row), flush=True)
        if (kind, seed) in CHECK_LEGS:
            for fmt, block in FORMATS:
                row = b.check_row(d_plain, n, fmt, block, crcs[block])
                key = f"{kind}_fcx{fmt}_b{block}"
                if a.parent_lib:
                    row["parent_verify"] = res["parent_verify"][key]
                    row["check_over_parent_verify"] = round(row["check"]["median_ms"] / row["parent_verify"]["verify"]["median_ms"], 4)
                res["check"][key] = row
                print("check", key, json.dumps(row), flush=True)
        del d_plain, host
    res.pop("parent_verify", None)
    b.dc.close()
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
