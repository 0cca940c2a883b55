#!/usr/bin/env python3
"""Driver of the stand-alone host check of the line code (tools/lines_host_check.cpp): runs the given binary,
and nothing else, on the mixed file of the tests and compares every run with tests/lines_model.py over the
oracle's decode.  Build the binary with the sanitizers first (the command line is in lines_host_check.cpp):

  python tools/lines_host_check.py ./lines_host_check [WORKDIR]

Runs, per delimiter 0x0A, 0x00, 0xFF, 0x80, 0x20: the count; nine 1-based ranges (both ends of the file, the line
across the three records that decode to nothing, behind the last line, an empty range); three patterns with
their line numbers.  Then five argument strings the parsers refuse (exit status 2) and a damaged record (1).
Any sanitizer report in a run's stderr fails the driver.  No GPU, and no library loaded into Python under a
sanitizer: the binary is a process of its own."""
import os
import pathlib
import subprocess
import sys
import tempfile

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

import find_model   # noqa: E402
import lines_model as m   # noqa: E402
from test_gpu_range import Truth   # noqa: E402


def main():
    exe = os.path.abspath(sys.argv[1])
    work = pathlib.Path(sys.argv[2] if len(sys.argv) > 2 else tempfile.mkdtemp())
    T = Truth("7", find_model.mixed_data(), 4096)
    assert T.sizes == [4096, 4096, 0, 0, 0, 4096, 4096, 1808]
    (work / "in.fcx").write_bytes(T.blob)

    def run(*args):
        r = subprocess.run([exe, str(work / "in.fcx"), *args], capture_output=True, text=True)
        assert "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, r.stderr
        return r

    runs = 0
    for d in m.DELIMS:
        hh = "%02x" % d
        nl, L, total, _ = m.stats(T.plain, d)
        r = run(hh, "count")
        assert r.returncode == 0 and [tuple(map(int, x)) for x in m.TOTALS.findall(r.stdout)] == [(L, nl, total)], r.stdout + r.stderr
        across = m.nl(T.plain, d, 8192)
        for a, c in ((1, 1), (1, None), (across + 1, 1), (max(across, 1), 3), (L, 1), (L, None), (L + 1, 2), (L + 9, None), (3, 0)):
            r = run(hh, "lines", "%d:%s" % (a, "" if c is None else c), str(work / "out"))
            off, n = m.locate(T.plain, d, a - 1, m.U64_MAX if c is None else c)
            assert r.returncode == 0 and (work / "out").read_bytes() == T.plain[off:off + n], (d, a, c, r.stderr)
            assert [tuple(map(int, x)) for x in m.DONE.findall(r.stdout)] == [(n, off)], r.stdout
        for pat in (T.plain[8189:8196], T.plain[100:102], bytes([d])):
            r = run(hh, "find", pat.hex())
            want = [(p, m.nl(T.plain, d, p) + 1) for p in find_model.hits(T.plain, pat)]
            assert r.returncode == 0 and [tuple(map(int, x)) for x in m.NUMBERED.findall(r.stdout)] == want, (d, pat)
        runs += 13
    for bad in (("0a", "lines", "0:1", "x"), ("0a", "lines", "1", "x"), ("a", "count"), ("0a0", "count"), ("0a", "lines", "1:2:3", "x")):
        assert run(*bad).returncode == 2, bad
    q, sz = T.rec_off[5] + 10, T.rec_off[6] - T.rec_off[5] - 4
    (work / "in.fcx").write_bytes(T.blob[:q + 4] + b"\xFF" * sz + T.blob[q + 4 + sz:])
    assert run("0a", "count").returncode == 1
    print(f"lines_host_check: {runs + 6} runs agree with the model, no sanitizer report")


if __name__ == "__main__":
    main()
