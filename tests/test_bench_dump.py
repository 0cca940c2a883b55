"""bench.py's --dump-outputs files and its plain / --full split.  dump_outputs runs on any torch
device, so its format is checked on the CPU; the GPU test runs a small plain benchmark end to end."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FILES = ("out_bytes", "stream_sums", "stream_sample_offsets", "stream_sample")


def load(d):
    return {k: np.load(os.path.join(d, k + ".npy")) for k in FILES}


def stream_of(n, seed):
    import torch

    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 256, (n + 100,), dtype=torch.uint8, generator=g)   # (capacity past the stream's end)


@pytest.mark.parametrize("total", [0, 1, 4096, 65537, (4 << 20) + 4097])   # empty, one piece, odd tail, sampled
def test_dump_outputs_format(tmp_path, total):
    import bench

    s = stream_of(total, 7)
    bench.dump_outputs(str(tmp_path / "a"), s, total)
    bench.dump_outputs(str(tmp_path / "b"), s.clone(), total)
    a, b = load(tmp_path / "a"), load(tmp_path / "b")
    assert sorted(os.listdir(tmp_path / "a")) == sorted(k + ".npy" for k in FILES)
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a")) <= 64 << 20
    for k in FILES:
        assert a[k].dtype in (np.float32, np.float64)
        assert np.array_equal(a[k], b[k]), k   # the same bytes give the same files
    assert a["out_bytes"].tolist() == [total]
    ref = s[:total].numpy().astype(np.int64)
    nseg = (total + 65535) // 65536
    assert a["stream_sums"].shape == (nseg, 2)
    pad = np.concatenate([ref, np.zeros(nseg * 65536 - total, np.int64)]).reshape(nseg, 65536)
    assert np.array_equal(a["stream_sums"][:, 0], pad.sum(1))
    assert np.array_equal(a["stream_sums"][:, 1], (pad * np.arange(1, 65537)).sum(1))
    offs = a["stream_sample_offsets"].astype(np.int64)
    assert a["stream_sample"].shape == (len(offs), 4096)
    for o, row in zip(offs, a["stream_sample"]):   # each piece holds the stream's bytes, zeros past its end
        want = np.zeros(4096, np.int64)
        want[:max(0, min(4096, total - o))] = ref[o:o + 4096]
        assert np.array_equal(row, want)
    if total <= 4 << 20:   # a short stream is dumped whole
        assert len(offs) == max(1, (total + 4095) // 4096)


def test_dump_outputs_sees_one_byte(tmp_path):
    import bench

    total = 300000
    s = stream_of(total, 9)
    t = s.clone()
    t[total - 1] ^= 1
    bench.dump_outputs(str(tmp_path / "a"), s, total)
    bench.dump_outputs(str(tmp_path / "b"), t, total)
    a, b = load(tmp_path / "a"), load(tmp_path / "b")
    assert not np.array_equal(a["stream_sums"], b["stream_sums"])
    t[total - 1] ^= 1
    t[total] ^= 255   # past the stream's end: not part of the output
    bench.dump_outputs(str(tmp_path / "c"), t, total)
    c = load(tmp_path / "c")
    assert all(np.array_equal(a[k], c[k]) for k in FILES)


@pytest.mark.gpu
def test_plain_run_is_lean_and_dumps(tmp_path, cuda):
    """a plain run on 64 MiB: the headline keys, none of the --full measurements, the dump files"""
    cmd = [sys.executable, "bench.py", "--gpus", "1", "--steps", "3", "--warmup", "1", "--global-mib", "64",
           "--dump-outputs", str(tmp_path / "d")]
    out = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [x for x in out.stdout.splitlines() if x.strip()]
    assert len(lines) == 1
    line = json.loads(lines[0])
    assert line["steps"] == 3 and line["warmup"] == 1 and line["full"] is False
    assert line["unit"] == "MB/s" and line["higher_is_better"] is True and line["dtype"] == "u8"
    assert line["ms_per_step"] > 0
    assert line["value"] == pytest.approx((64 << 20) / (line["ms_per_step"] * 1e-3) / 1e6, rel=1e-9)
    for k in ("roofline", "cpu_baseline", "decode", "host_path", "cold_call", "bit_exact_vs_reference"):
        assert line.get(k) is None, k
    for k in ("legs", "lz78", "transition", "text", "mix"):
        assert k not in line, k
    d = load(tmp_path / "d")
    total = int(d["out_bytes"][0])
    assert total == round(line["ratio"] * (64 << 20)) and total > 64 << 20   # (rand does not compress)
    assert d["stream_sums"].shape == ((total + 65535) // 65536, 2)
    assert d["stream_sample"].shape == (1024, 4096) and d["stream_sample"].max() <= 255
