#!/usr/bin/env python3
"""Driver of the stand-alone host check of the regex code (tools/regex_host_check.cpp): runs the given binary, and
nothing else, one process per case, and compares every run with tests/regex_model.py (an NFA simulation that shares
nothing with the compiler).  Build the binary with the sanitizers first (the command line is in regex_host_check.cpp):

  python tools/regex_host_check.py ./regex_host_check [WORKDIR]

Runs: every expression of tests/test_regex_model.py with and without the fold (the compiler accepts it, and the
match ends in a buffer of sample lines are the model's), every refusal there (exit status 2), the state limits, the
crafted file of regex_model and the mixed file of the tests through the no-device grep under several options and
three delimiters, arguments the parsers refuse and a damaged record (1).  Any sanitizer report in a run's stderr fails
the driver.  No GPU, and no library loaded into Python under a sanitizer: the binary is a process of its own."""
import os
import pathlib
import subprocess
import sys
import tempfile

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

import context_model as cm   # noqa: E402
import find_model as fm   # noqa: E402
import regex_model as rm   # noqa: E402
from test_gpu_range import Truth   # noqa: E402
from test_regex_model import BOTH, PLAIN, POSIX, REFUSED   # noqa: E402


def main():
    exe = os.path.abspath(sys.argv[1])
    work = pathlib.Path(sys.argv[2] if len(sys.argv) > 2 else tempfile.mkdtemp())
    runs = 0

    def run(*args):
        nonlocal runs
        r = subprocess.run([exe, *args], capture_output=True, text=True)
        assert "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, r.stderr
        runs += 1
        return r

    lines, sample = [ln for ln in PLAIN.split(b"\n") if ln], b""
    for ln in lines:   # as many whole lines as 256 bytes hold, the last one unterminated
        if len(sample) + len(ln) + 1 > 256:
            break
        sample += ln + b"\n"
    sample = sample[:-1]
    for expr in BOTH + POSIX:
        for fold in (False, True):
            flags = "i" if fold else "-"
            r = run("hits", expr.hex(), flags, "0a", sample.hex())
            want = rm.hits(sample, rm.Nfa(expr, 0x0A, fold))
            assert r.returncode == 0 and r.stdout == "hits:" + "".join(f" {p}" for p in want) + "\n", (expr, fold, r.stdout, want)
    for expr in REFUSED:
        r = run("compile", expr.hex(), "-", "0a")
        assert r.returncode == 2 and r.stdout.startswith("refused: "), (expr, r.stdout)
    for expr, d, flags, ok in ((b"^a{61}b", "0a", "-", "regex: 64 states, 4 classes\n"), (b"^a{62}b", "0a", "-", None), (b"a", "41", "-", "regex: 2 states, 2 classes\n"),
                               (b"a", "41", "i", None), (b"a[^b]{4}b", "00", "i", "regex: 33 states, 4 classes\n"), (b"a.{20}b", "0a", "-", None)):
        r = run("compile", expr.hex(), flags, d)
        assert (r.returncode, r.stdout) == (0, ok) if ok else r.returncode == 2, (expr, r.stdout)

    def grep(T, expr, d, fold, invert, before, after):
        (work / "in.fcx").write_bytes(T.blob)
        flags = ("i" if fold else "") + ("v" if invert else "") or "-"
        nfa = rm.Nfa(expr, d, fold)
        h = rm.hits(T.plain, nfa)
        blk = rm.blocks(T.plain, nfa, invert, before, after, h)
        st = rm.stats(T.plain, nfa, invert, before, after, blk, h)
        for out in (True, False):
            r = run("grep", str(work / "in.fcx"), expr.hex(), flags, "%02x" % d, str(before), str(after), *([str(work / "out")] if out else []))
            assert r.returncode == 0, r.stderr
            assert [tuple(int(x) for x in t) for t in cm.TOTALS.findall(r.stdout)] == [(st[0], st[1], st[3], st[2], st[4], st[6])], (expr, r.stdout)
            if out:
                assert (work / "out").read_bytes() == cm.join(T.plain, blk, cm.separator(d, before, after)), (expr, d, flags, before, after)

    for d in (0x0A, 0x00, 0x41):
        C = Truth("7", rm.crafted(d), rm.BLOCK)
        rm.check_crafted(C.plain, d)
        for expr in rm.CRAFT_EXPRS:
            grep(C, expr, d, False, False, 0, 0)
        grep(C, rm.E_MIX, d, False, True, 2, 1)
        grep(C, rm.E_FAR, d, False, False, 1, 3)
        if d != 0x41:
            grep(C, b"A[^B]{3}b|THE ", d, True, True, 0, 0)
    M = Truth("7", fm.mixed_data(), 4096)
    assert M.sizes == [4096, 4096, 0, 0, 0, 4096, 4096, 1808]
    for expr, d, opt in ((b"[a-z]+\\.$", 0x0A, (False, 0, 0)), (b"^[A-Z][a-z]* ", 0x0A, (True, 1, 1)), (b"e[^a]", 0x20, (False, 2, 2)),
                         (b"^the$|^and$", 0x20, (False, 0, 4096)), (b"zzzzq", 0x0A, (True, 0, 0)), (b"zzzzq", 0x0A, (False, 3, 3))):
        grep(M, expr, d, False, *opt)
    (work / "in.fcx").write_bytes(M.blob)
    for args in (["grep", "in.fcx", "6162", "-", "0a", "4097", "0"], ["grep", "in.fcx", "6162", "-", "0a", "1", "z"], ["grep", "in.fcx", "616", "-", "0a", "1", "1"],
                 ["grep", "in.fcx", "6162", "-", "0a", "1"], ["grep", "nothing-here", "6162", "-", "0a", "1", "1"], ["hits", "6162", "-", "0", "6162"]):
        assert subprocess.run([exe, *args], cwd=work, capture_output=True, text=True).returncode == 2, args
        runs += 1
    q, sz = M.rec_off[5] + 10, M.rec_off[6] - M.rec_off[5] - 4
    (work / "in.fcx").write_bytes(M.blob[:q + 4] + b"\xFF" * sz + M.blob[q + 4 + sz:])
    r = run("grep", str(work / "in.fcx"), b"the".hex(), "v", "0a", "2", "2", str(work / "out"))
    assert r.returncode == 1 and "grep:" not in r.stdout
    print(f"regex_host_check: {runs} runs agree with the model, no sanitizer report")


if __name__ == "__main__":
    main()
