#!/usr/bin/env python3
"""Driver of the stand-alone host check of the pattern-set code (tools/set_host_check.cpp): runs the given binary,
and nothing else, on the mixed file of the tests and on the crafted file of tests/set_model.py, and compares every
run with set_model over the oracle's decode.  Build the binary with the sanitizers first (the command line is in
set_host_check.cpp):

  python tools/set_host_check.py ./set_host_check [WORKDIR]

Runs: sets of mixed lengths (1 to 256 bytes) cut at the files' ends, seams and plants, as text and as hex, with and
without the fold, find and grep (with and without an output file, three delimiters); 64 patterns; then the pattern
files and arguments the parser and the set compiler refuse (exit status 2) and a damaged record (1).  Any sanitizer
report in a run's stderr fails the driver.  No GPU, and no library loaded into Python under a sanitizer: the binary
is a process of its own."""
import os
import pathlib
import re
import subprocess
import sys
import tempfile

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

import find_model as fm   # noqa: E402
import grep_model as gm   # noqa: E402
import set_model as sm   # noqa: E402
from test_gpu_range import Truth   # noqa: E402

COUNTS = re.compile(r"^counts:((?: \d+)*)$", re.M)


def main():
    exe = os.path.abspath(sys.argv[1])
    work = pathlib.Path(sys.argv[2] if len(sys.argv) > 2 else tempfile.mkdtemp())
    runs = 0

    def run(*args):
        r = subprocess.run([exe, *args], capture_output=True, text=True)
        assert "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, r.stderr
        return r

    def check(T, pats, d, fold, hexed):
        nonlocal runs
        (work / "in.fcx").write_bytes(T.blob)
        (work / "pats").write_bytes(b"\n".join(p.hex().encode() if hexed else p for p in pats) + b"\n")
        flags = ("x" if hexed else "") + ("i" if fold else "") or "-"
        wc = sm.counts(T.plain, pats, fold)
        r = run("find", str(work / "in.fcx"), str(work / "pats"), flags)
        want = sm.hits_any(T.plain, pats, fold)
        assert r.returncode == 0, r.stderr
        assert [int(x) for x in fm.LINE.findall(r.stdout)] == want, (pats, fold)
        assert [tuple(map(int, x)) for x in sm.FIND_TOTALS.findall(r.stdout)] == [(len(want), T.total, len(pats))]
        assert [int(x) for x in COUNTS.findall(r.stdout)[0].split()] == wc
        runs += 1
        if any(bytes([d]) in p or (fold and sm.fold(bytes([d]), True) in sm.fold(p, True)) for p in pats):
            assert run("grep", str(work / "in.fcx"), str(work / "pats"), flags, "%02x" % d).returncode == 2
            runs += 1
            return
        sel = sm.selected_any(T.plain, pats, d, fold)
        st = sm.grep_stats(T.plain, pats, d, fold, sel)
        for out in (True, False):
            r = run("grep", str(work / "in.fcx"), str(work / "pats"), flags, "%02x" % d, *([str(work / "out")] if out else []))
            assert r.returncode == 0, r.stderr
            assert [tuple(map(int, x)) for x in sm.GREP_TOTALS.findall(r.stdout)] == [(st[0], st[1], st[2], st[4], len(pats))], r.stdout
            assert [int(x) for x in COUNTS.findall(r.stdout)[0].split()] == wc
            if out:
                assert (work / "out").read_bytes() == gm.join(T.plain, sel), (pats, d, fold)
            runs += 1

    M = Truth("7", fm.mixed_data(), 4096)
    assert M.sizes == [4096, 4096, 0, 0, 0, 4096, 4096, 1808]
    for d in (0x0A, 0x00, 0x20):
        pats = [fm.absent(M.plain)]
        for i, p in enumerate((0, 100, 4090, 8189, 8192 - 128, 12000, M.total - 256, M.total - 3, M.total - 1)):
            pat = gm.cut(M.plain, d, p, [1, 2, 3, 4, 5, 8, 255, 256, 3][i])
            if pat and b"\n" not in pat:
                pats.append(pat)
        for fold in (False, True):
            check(M, pats, d, fold, True)
        words = [w for w in M.plain[:4000].split(b" ") if len(w) >= 4 and w.isalpha()][:6]
        check(M, [w.upper() for w in words], d, True, False)
        check(M, [w.swapcase() for w in words], d, False, False)
    for d in gm.DELIMS:
        C = Truth("7", sm.crafted(d), sm.BLOCK)
        sm.check_crafted(C.plain, d)
        for pats in ([sm.SHORT1, sm.SHORT3, sm.LONG], [b"\x1a\x1b", b"\x1a\x1b\x1c", b"\x1a\x1b\x1c", b"\x1b\x1c\x1d"],
                     [sm.FOLD_PAT, sm.UP], sm.absent_set(C.plain), [bytes([b]) for b in range(0x20, 0x60)]):
            for fold in (False, True):
                check(C, pats, d, fold, True)
    (work / "in.fcx").write_bytes(M.blob)
    bad = {"empty line": b"ab\n\ncd\n", "two line ends": b"ab\n\n", "nothing": b"", "65": b"".join(b"p%02d\n" % i for i in range(65)),
           "257": b"a" * 257 + b"\n", "4097": b"".join(b"%03d" % i + b"a" * 253 + b"\n" for i in range(16)) + b"b\n"}
    for what, body in bad.items():
        (work / "pats").write_bytes(body)
        assert run("find", str(work / "in.fcx"), str(work / "pats"), "-").returncode == 2, what
        runs += 1
    for body in (b"616\n", b"61zz\n", b"61\n\n62\n"):
        (work / "pats").write_bytes(body)
        assert run("find", str(work / "in.fcx"), str(work / "pats"), "x").returncode == 2, body
        runs += 1
    (work / "pats").write_bytes(b"xay\n")
    assert run("grep", str(work / "in.fcx"), str(work / "pats"), "i", "41").returncode == 2
    assert run("grep", str(work / "in.fcx"), str(work / "pats"), "-", "41").returncode == 0
    q, sz = M.rec_off[5] + 10, M.rec_off[6] - M.rec_off[5] - 4
    (work / "in.fcx").write_bytes(M.blob[:q + 4] + b"\xFF" * sz + M.blob[q + 4 + sz:])
    assert run("find", str(work / "in.fcx"), str(work / "pats"), "-").returncode == 1
    assert run("grep", str(work / "in.fcx"), str(work / "pats"), "-", "0a").returncode == 1
    print(f"set_host_check: {runs + 4} runs agree with the model, no sanitizer report")


if __name__ == "__main__":
    main()
