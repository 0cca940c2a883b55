#!/usr/bin/env python3
"""Driver of the stand-alone host check of the grep code (tools/grep_host_check.cpp): runs the given binary, and
nothing else, on the mixed file of the tests and compares every run with tests/grep_model.py over the oracle's
decode.  Build the binary with the sanitizers first (the command line is in grep_host_check.cpp):

  python tools/grep_host_check.py ./grep_host_check [WORKDIR]

Runs, per delimiter 0x0A, 0x00, 0xFF, 0x20: patterns of 1 to 256 bytes cut at the file's two ends, in the line
across the three records that decode to nothing and around a record seam, with and without an output file, and
one that does not occur.  Then five argument strings the parsers refuse (exit status 2) and a damaged record (1).
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
import grep_model as m   # noqa: E402
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
    for d in (0x0A, 0x00, 0xFF, 0x20):
        hh = "%02x" % d
        pats = [find_model.absent(T.plain)]
        for i, p in enumerate((0, 100, 4090, 8189, 8192 - 128, 12000, T.total - 256, T.total - 1)):
            pat = m.cut(T.plain, d, p, m.LENGTHS[i % len(m.LENGTHS)])
            if pat:
                pats.append(pat)
        for pat in pats:
            want = m.selected(T.plain, pat, d)
            st = m.stats(T.plain, pat, d, want)
            for out in (True, False):
                r = run(hh, pat.hex(), *([str(work / "out")] if out else []))
                assert r.returncode == 0, r.stderr
                assert [tuple(map(int, x)) for x in m.TOTALS.findall(r.stdout)] == [(st[0], st[1], st[2], st[4])], (d, pat, r.stdout)
                if out:
                    assert (work / "out").read_bytes() == m.join(T.plain, want), (d, pat)
                runs += 1
    for bad in (("0a", "610a"), ("0a", "61z"), ("a", "61"), ("0a", ""), ("0a", "61" * 257)):
        assert run(*bad).returncode == 2, bad
    q, sz = T.rec_off[5] + 10, T.rec_off[6] - T.rec_off[5] - 4
    (work / "in.fcx").write_bytes(T.blob[:q + 4] + b"\xFF" * sz + T.blob[q + 4 + sz:])
    assert run("0a", "6162").returncode == 1
    print(f"grep_host_check: {runs + 6} runs agree with the model, no sanitizer report")


if __name__ == "__main__":
    main()
