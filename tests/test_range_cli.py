"""The command line's random access: --range OFF:LEN and --list in the decompress mode.  Without a
HIP device both run on the host decoder for FCX7 (record by record) and fail loudly for FCX8; the
gpu twins take fcx_decompress_range_stream and fcx_index_shard.  The expected bytes and sizes are
the oracle's, per record."""
import re
import struct

import pytest

import inputs
import oracle
from test_cli import gpu_present, run

SIZES = [4096, 4096, 0, 0, 0, 4096, 4096, 1808]
RANGES = [(8190, 4), (4000, 9000), (0, 30000), (18191, 1), (18192, 5)]
LINE = re.compile(r"^record (\d+): compressed (\d+) bytes, decoded (\d+) bytes, decoded offset (\d+)$", re.M)


def per_record(blob: bytes, lz78: bool):
    """([payload bytes], [decoded bytes]) of the records of a whole file, by the oracle"""
    q, comp, parts = 10, [], []
    while q < len(blob):
        (sz,) = struct.unpack_from("<I", blob, q)
        p = blob[q + 4:q + 4 + sz]
        parts.append(oracle.lz78_decompress_block(p, (1 << 20) + 64) if lz78 else oracle.decompress_block(p, (1 << 20) + 64))
        comp.append(sz)
        q += 4 + sz
    return comp, parts


@pytest.fixture(scope="module")
def mixed():
    data = inputs.generate("text", 7, 8192) + inputs.generate("rand", 3, 12288) + inputs.generate("text", 9, 10000)
    blob = oracle.compress_file(data, 4096)
    comp, parts = per_record(blob, False)
    assert [len(p) for p in parts] == SIZES
    return blob, comp, b"".join(parts)


def check_range(tmp_path, blob, plain, off, n):
    (tmp_path / "in.fcx").write_bytes(blob)
    r = run(["-i", "in.fcx", "-o", "part", "--range", f"{off}:{n}"], tmp_path)
    assert r.returncode == 0, r.stdout + r.stderr
    want = plain[off:off + n]
    assert (tmp_path / "part").read_bytes() == want
    assert f"range decompress bytes = {len(want)} (offset {off})" in r.stdout.splitlines()


def check_list(tmp_path, blob, comp, sizes):
    (tmp_path / "in.fcx").write_bytes(blob)
    r = run(["-i", "in.fcx", "-o", "never", "--list"], tmp_path)
    assert r.returncode == 0, r.stdout + r.stderr
    rows = [tuple(int(x) for x in m) for m in LINE.findall(r.stdout)]
    offs = [sum(sizes[:k]) for k in range(len(sizes))]
    assert rows == [(k, comp[k], sizes[k], offs[k]) for k in range(len(sizes))]
    assert f"records = {len(sizes)}, compressed bytes = {sum(comp)}, decoded bytes = {sum(sizes)}" in r.stdout
    assert not (tmp_path / "never").exists()   # --list writes no file


def test_range_on_the_mixed_file(tmp_path, mixed):
    blob, _, plain = mixed
    for off, n in RANGES:
        check_range(tmp_path, blob, plain, off, n)


def test_list_prints_the_decoded_sizes(tmp_path, mixed):
    blob, comp, _ = mixed
    check_list(tmp_path, blob, comp, SIZES)


def test_range_on_fcx8_fails_loudly_without_gpu(tmp_path):
    if gpu_present():
        pytest.skip("GPU present")
    (tmp_path / "x8").write_bytes(oracle.lz78_compress_file(b"hello hello hello", 1 << 20))
    for extra in (["--range", "0:5"], ["--list"]):
        r = run(["-i", "x8", "-o", "y"] + extra, tmp_path)
        assert r.returncode != 0 and ("HIP" in r.stderr or "GPU" in r.stderr), r.stderr


@pytest.mark.parametrize("arg", ["12", "a:b", "-1:5", "1:", ":1", "1:2:3", "1:2x", "99999999999999999999:1"])
def test_malformed_range_is_a_usage_error(arg, tmp_path, mixed):
    (tmp_path / "in.fcx").write_bytes(mixed[0])
    r = run(["-i", "in.fcx", "-o", "part", "--range", arg], tmp_path)
    assert r.returncode != 0 and "usage:" in r.stderr
    assert not (tmp_path / "part").exists()


def test_range_or_list_with_compress_is_a_usage_error(tmp_path):
    (tmp_path / "plain").write_bytes(b"hello hello hello hello")
    for extra in (["--range", "0:5"], ["--list"]):
        r = run(["-i", "plain", "-o", "x", "-c", "lz77"] + extra, tmp_path)
        assert r.returncode != 0 and "usage:" in r.stderr
        assert not (tmp_path / "x").exists()
    r = run(["-i", "plain", "-o", "x", "--list", "--range", "0:5"], tmp_path)
    assert r.returncode != 0 and "usage:" in r.stderr


def test_damaged_record_fails_the_host_range_only_when_read(tmp_path, mixed):
    if gpu_present():
        pytest.skip("GPU present")   # (the stream path checks every record of the groups it reads)
    blob, _, plain = mixed
    q = 10
    for _ in range(5):
        q += 4 + struct.unpack_from("<I", blob, q)[0]
    (sz,) = struct.unpack_from("<I", blob, q)
    bad = blob[:q + 4] + b"\xFF" * sz + blob[q + 4 + sz:]   # record 5's payload
    check_range(tmp_path, bad, plain, 100, 7000)           # ends in record 1: record 5 is never read
    (tmp_path / "in.fcx").write_bytes(bad)
    r = run(["-i", "in.fcx", "-o", "part", "--range", "8000:1000"], tmp_path)
    assert r.returncode != 0 and "block 6" in r.stderr


@pytest.mark.gpu
def test_gpu_range_and_list_both_kinds(tmp_path, mixed, cuda):
    blob, comp, plain = mixed
    for off, n in RANGES[:3]:
        check_range(tmp_path, blob, plain, off, n)
    check_list(tmp_path, blob, comp, SIZES)
    t = bytearray(inputs.generate("text", 7, 12288)[:10001])
    t[4095] = t[8191] = t[10000] = 0
    blob8 = oracle.lz78_compress_file(bytes(t), 4096)
    comp8, parts8 = per_record(blob8, True)
    assert [len(p) for p in parts8] == [4095, 4095, 1808]
    for off, n in [(4090, 10), (8189, 2000)]:
        check_range(tmp_path, blob8, b"".join(parts8), off, n)
    check_list(tmp_path, blob8, comp8, [4095, 4095, 1808])
