#!/usr/bin/env python3
"""Driver of the stand-alone host check of the cut (tools/cut_host_check.cpp): runs the given binary, and nothing else,
one process per case, and compares every run with tests/cut_model.py over the oracle's decode.  Build the binary with
the sanitizers first (the command line is in cut_host_check.cpp):

  python tools/cut_host_check.py ./cut_host_check [WORKDIR]

Runs: the compiler alone on every list the model accepts and refuses (mn, the open end, the offset it names); the cut of
the mixed file of the tests (three records in the middle decode to nothing, lines cross the records) and of a line
whose count saturates, for fields, bytes and complements under three delimiter / separator pairs; the totals alone; a
damaged record (exit status 1).  Any sanitizer report in a run's stderr fails the driver.  No GPU, and no library
loaded into Python under a sanitizer: the binary is a process of its own."""
import os
import pathlib
import re
import subprocess
import sys
import tempfile

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

import cut_model as km   # noqa: E402
import find_model   # noqa: E402
from test_gpu_range import Truth   # noqa: E402

TOTALS = re.compile(r"^cut: (\d+) bytes, (\d+) delimiters, (\d+) separators \((\d+) kept\), decoded bytes = (\d+)$", re.M)
ACCEPTED = ["1", "4096", "4097-", "-4096", "1-4096", "1,1,1", "7-7", "2,4", "3-", "-2", "2-3,5-"]
REFUSED = ["", "0", "1,0", "5-3", "4097", "1-4097", "4098-", "1,,2", "1,", ",1", "1 2", "a", "-", "1-2-3", "2-0", "1;2", "0-", "-0"]
LISTS = ["2", "1,3-4", "2-", "7", "1-16", "3,40-", "4096", "4097-", "1-4096"]


def main():
    exe = os.path.abspath(sys.argv[1])
    work = pathlib.Path(sys.argv[2] if len(sys.argv) > 2 else tempfile.mkdtemp())

    def run(*args):
        r = subprocess.run([exe, *args], capture_output=True, text=True)
        assert "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, r.stderr
        return r

    runs = 0
    for lst in ACCEPTED:
        for m in "fbFB":
            want = km.Sel(lst, m in "FB")
            r = run("-", m, lst, "2c", "0a")
            assert r.returncode == 0 and r.stdout == "mn %d open %d\n" % (want.mn, want.open_end), (lst, m, r.stdout, r.stderr)
            runs += 1
    for lst in REFUSED:
        try:
            km.Sel(lst)
            raise AssertionError(lst)
        except km.ListError as e:
            r = run("-", "f", lst, "2c", "0a")
            assert r.returncode == 2 and r.stderr.startswith("LIST offset %d: " % e.offset), (lst, r.stderr)
            runs += 1
    assert run("-", "F", "1-", "2c", "0a").returncode == 2 and run("-", "f", "1", "0a", "0a").returncode == 2
    assert run("-", "b", "1", "0a", "0a").returncode == 0 and run("-", "x", "1", "2c", "0a").returncode == 2

    mixed = Truth("7", find_model.mixed_data(), 4096)
    assert mixed.sizes == [4096, 4096, 0, 0, 0, 4096, 4096, 1808]
    long = Truth("7", b",".join(b"%d" % (i % 10) for i in range(5001)) + b"\nq,r,s\nnosep\ntail,x", 4096)
    for T, pairs in ((mixed, ((0x20, 0x0A), (0x65, 0x20), (0x00, 0x2E))), (long, ((0x2C, 0x0A),))):
        (work / "in.fcx").write_bytes(T.blob)
        for sep, d in pairs:
            for lst in LISTS:
                for m in "fbFB":
                    mode = km.FIELDS if m in "fF" else km.BYTES
                    out, st = km.cut_np(T.plain, km.Sel(lst, m in "FB"), mode, sep, d)
                    assert km.cut_py(T.plain, km.Sel(lst, m in "FB"), mode, sep, d) == (out, st)
                    r = run(str(work / "in.fcx"), m, lst, "%02x" % sep, "%02x" % d, str(work / "out"))
                    assert r.returncode == 0 and (work / "out").read_bytes() == out, (lst, m, sep, d, r.stderr)
                    assert [tuple(map(int, x)) for x in TOTALS.findall(r.stdout)] == [(st[0], st[2], st[3], st[4], st[1])], r.stdout
                    runs += 1
            r = run(str(work / "in.fcx"), "f", "2", "%02x" % sep, "%02x" % d, "-")
            st = km.cut_np(T.plain, km.Sel("2"), km.FIELDS, sep, d)[1]
            assert r.returncode == 0 and [tuple(map(int, x)) for x in TOTALS.findall(r.stdout)] == [(st[0], st[2], st[3], st[4], st[1])]
            runs += 1
    T = mixed
    q, sz = T.rec_off[5] + 10, T.rec_off[6] - T.rec_off[5] - 4
    (work / "in.fcx").write_bytes(T.blob[:q + 4] + b"\xFF" * sz + T.blob[q + 4 + sz:])
    assert run(str(work / "in.fcx"), "f", "2", "20", "0a", "-").returncode == 1
    print(f"cut_host_check: {runs + 5} runs agree with the model, no sanitizer report")


if __name__ == "__main__":
    main()
