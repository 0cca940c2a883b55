"""Throughput of the FCX8 (LZ78) decoder on one GPU: rand and text, 1 MiB blocks.

Two figures per kind, from data compressed once with the GPU codec (its scratch released
before any timing):
  device-resident  fcx_lz78_decompress_shard timed with device events around the call: two
                   warm-up calls, the median of --reps calls, then one profiled call for the
                   per-stage times of fcx_dctx_stage (profiling synchronises per batch, so it
                   is kept out of the timed calls), and the decoder scratch the first call
                   allocated, per token of its largest batch;
  host to host     fcx_lz78_decompress_host, wall clock, same counts.

The bar is another build of the library measured in the same session: --parent-lib PATH runs
that library (through FCX_LIB, in child processes of its own) before and after this tree's,
--rounds times each, alternating; a library without the device entry point reports host to
host only.  Every worker also reports the sha256 of what it decoded, and the driver checks
that all builds decoded the same bytes.

  python tools/lz78_decode_bench.py [--mib 256] [--reps 5] [--parent-lib PATH] [--rounds 2]
                                    [--out profiles/lz78_decode.json]
"""
import argparse
import ctypes
import hashlib
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

BLOCK = 1 << 20


def token_counts(recs: bytes, nrec: int):
    """N of every record (the payload layout of my_decompress_file_lz78, 3478-3600)"""
    import numpy as np

    out, q = [], 0
    for _ in range(nrec):
        ln = int.from_bytes(recs[q:q + 4], "little")
        p = q + 4
        wcnt = int.from_bytes(recs[p:p + 4], "little")
        bm = np.frombuffer(recs, dtype=np.uint8, count=min(ln - 4, (BLOCK + 16) // 8 + 8), offset=p + 4)
        cum = np.cumsum(np.unpackbits(bm, bitorder="little"))
        last = int(np.searchsorted(cum, wcnt))   # position of the wcnt-th set bit
        r = p + 4 + last // 8 + 1
        G = int.from_bytes(recs[r:r + 4], "little")
        r += 4 + (8 * (G - 1) if G > 1 else 0)
        out.append(int.from_bytes(recs[r:r + 4], "little"))
        q += 4 + ln
    return out


def worker(args):
    import torch

    import inputs
    import my_compress_amd as mc

    L = mc.lib()
    has_shard = hasattr(L, "fcx_lz78_decompress_shard")
    n = args.mib << 20
    res = {"lib": os.path.relpath(mc.lib_path(), ROOT), "mib": args.mib, "block_bytes": BLOCK, "reps": args.reps, "kinds": {}}
    for kind in ("rand", "text"):
        data = inputs.generate(kind, 4, n)
        blob = mc.compress_lz78(data, BLOCK)   # (releases the compress scratch)
        nrec = (n + BLOCK - 1) // BLOCK
        cap = n + 64
        r = {"compressed_bytes": len(blob)}
        # host to host
        out = ctypes.create_string_buffer(cap)
        got = ctypes.c_uint64()
        times = []
        for it in range(2 + args.reps):
            t0 = time.perf_counter()
            rc = L.fcx_lz78_decompress_host(blob, len(blob), out, cap, ctypes.byref(got))
            dt = time.perf_counter() - t0
            assert rc == 0, L.fcx_last_error()
            if it >= 2:
                times.append(dt)
        r["decoded_bytes"] = got.value
        r["sha256"] = hashlib.sha256(out.raw[:got.value]).hexdigest()
        r["host_to_host"] = {"ms": [round(t * 1e3, 3) for t in times],
                             "median_ms": round(statistics.median(times) * 1e3, 3),
                             "MBps_median": round(n / statistics.median(times) / 1e6, 1),
                             "MBps_min": round(n / max(times) / 1e6, 1), "MBps_max": round(n / min(times) / 1e6, 1)}
        del out
        if has_shard:
            recs = blob[10:]
            d_in = torch.frombuffer(bytearray(recs), dtype=torch.uint8).to("cuda:0")
            d_out = torch.zeros(cap, dtype=torch.uint8, device="cuda:0")
            stream = torch.cuda.current_stream().cuda_stream
            d = mc.DContext(0)
            torch.cuda.synchronize()
            free0 = torch.cuda.mem_get_info()[0]
            ms = []
            for it in range(2 + args.reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                m = d.decompress_lz78_shard(d_in.data_ptr(), len(recs), nrec, d_out.data_ptr(), cap, stream)
                e1.record()
                e1.synchronize()
                if it == 0:
                    scratch = free0 - torch.cuda.mem_get_info()[0]
                if it >= 2:
                    ms.append(e0.elapsed_time(e1))
            assert m == r["decoded_bytes"]
            assert hashlib.sha256(d_out[:m].cpu().numpy().tobytes()).hexdigest() == r["sha256"]
            d.set_profiling(True)
            d.decompress_lz78_shard(d_in.data_ptr(), len(recs), nrec, d_out.data_ptr(), cap, stream)
            stages = d.stage_times()
            d.close()
            toks = token_counts(recs, nrec)
            batch = mc.lz78_decode_batch_records()
            big = max(sum(toks[i:i + batch]) for i in range(0, nrec, batch))
            r["device_resident"] = {"ms": [round(t, 3) for t in ms], "median_ms": round(statistics.median(ms), 3),
                                    "MBps_median": round(n / statistics.median(ms) / 1e3, 1),
                                    "stages_ms_profiled_call": {k: round(v, 3) for k, v in stages},
                                    "tokens": sum(toks), "batch_records": batch, "tokens_largest_batch": big,
                                    "scratch_bytes": scratch, "scratch_bytes_per_token": round(scratch / big, 2)}
            del d_in, d_out
        res["kinds"][kind] = r
        print(kind, json.dumps(r), file=sys.stderr, flush=True)
    print(json.dumps(res))


def run_worker(args, lib):
    env = dict(os.environ)
    if lib:
        env["FCX_LIB"] = lib
    else:
        env.pop("FCX_LIB", None)
    cmd = [sys.executable, os.path.abspath(__file__), "--worker", "--mib", str(args.mib), "--reps", str(args.reps)]
    p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=1500)
    sys.stderr.write(p.stderr)
    if p.returncode != 0:
        raise SystemExit(f"worker failed ({p.returncode}) for {lib or 'this tree'}")
    return json.loads(p.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mib", type=int, default=256)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lz78_decode.json"))
    ap.add_argument("--worker", action="store_true")
    args = ap.parse_args()
    if args.reps < 5:
        raise SystemExit("--reps must be at least 5")
    if args.worker:
        return worker(args)
    runs = []
    for rnd in range(args.rounds if args.parent_lib else 1):
        if args.parent_lib:
            runs.append(("parent", run_worker(args, os.path.abspath(args.parent_lib))))
        runs.append(("new", run_worker(args, None)))
    res = {"mib": args.mib, "block_bytes": BLOCK, "runs": [{"build": b, **r} for b, r in runs], "summary": {}}
    for kind in ("rand", "text"):
        shas = {r["kinds"][kind]["sha256"] for _, r in runs}
        assert len(shas) == 1, f"{kind}: the builds decoded different bytes"
        s = {}
        for b in ("parent", "new"):
            h = [r["kinds"][kind]["host_to_host"]["MBps_median"] for bb, r in runs if bb == b]
            allh = [n for bb, r in runs if bb == b for n in
                    (r["kinds"][kind]["host_to_host"]["MBps_min"], r["kinds"][kind]["host_to_host"]["MBps_max"])]
            if h:
                s[b + "_host_to_host_MBps"] = {"medians": h, "min": min(allh), "max": max(allh)}
        dev = [r["kinds"][kind]["device_resident"]["MBps_median"] for b, r in runs if "device_resident" in r["kinds"][kind]]
        if dev:
            s["new_device_resident_MBps"] = dev
        res["summary"][kind] = s
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res["summary"]))


if __name__ == "__main__":
    main()
