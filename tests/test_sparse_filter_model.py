"""The sparse unit's repeat filter (my_compress_amd/csrc/fcx_sparse_filter.h) on the host, through
libfcx.so's development export: the same hash the kernel compiles, keys inserted in position order.

Two properties the kernel's exactness and its speed on random data rest on:
  * the flagged-key cap is at least twice the largest flagged count of any tile window over the
    first 64 MiB of the seed-4 random stream (the headline input), so random data never leaves the
    sparse path;
  * of two equal keys in a window at least one is flagged, wherever they lie.
"""
import ctypes
import random

import numpy as np
import pytest

import inputs
import my_compress_amd as mc

TILE, HALO, EXTRA = 4096, 2048, 2   # the kernel's window: 2048 halo + 4096 + 2 key positions


@pytest.fixture(scope="module")
def model():
    L = mc.lib()
    L.fcx_debug_sparse_filter.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p,
                                          ctypes.POINTER(ctypes.c_uint32)]

    def run(buf: np.ndarray, start: int, nkeys: int, want_flags: bool = False):
        """keys at buf[start .. start + nkeys) (buf holds nkeys + 2 bytes from start)"""
        assert start + nkeys + 2 <= buf.size
        out = (ctypes.c_uint32 * 4)()
        flags = np.zeros(nkeys, dtype=np.uint8) if want_flags else None
        rc = L.fcx_debug_sparse_filter(ctypes.c_void_p(buf.ctypes.data + start), nkeys,
                                       ctypes.c_void_p(flags.ctypes.data) if want_flags else None, out)
        assert rc == 0
        return {"flagged": out[0], "cap": out[1], "rcap": out[2], "k": out[3], "flags": flags}

    return run


def test_random_stream_stays_below_half_the_cap(model):
    n = 64 << 20
    buf = np.frombuffer(inputs.generate("rand", 4, n), dtype=np.uint8)
    worst, total, tiles, cap = 0, 0, 0, None
    for t0 in range(0, n, TILE):
        lo = max(0, t0 - HALO)
        nkeys = min(t0 + TILE + EXTRA, n - 2) - lo
        r = model(buf, lo, nkeys)
        cap = r["cap"]
        worst = max(worst, r["flagged"])
        total += r["flagged"]
        tiles += 1
    print(f"k = {r['k']}: flagged per window mean {total / tiles:.2f}, max {worst}, cap {cap}, R capacity {r['rcap']}")
    assert 2 * worst <= cap, (worst, cap)
    assert r["rcap"] >= 2 * 64   # the 64 match positions sparse_parse accepts, a candidate each


def test_one_of_every_equal_pair_is_flagged(model):
    rng = random.Random(20)
    nkeys = HALO + TILE + EXTRA
    base = np.frombuffer(inputs.generate("rand", 77, nkeys + 2), dtype=np.uint8)
    # positions at the window's edges, the halo / tile boundary, and seeded ones anywhere
    edge = [0, 1, 2, HALO - 3, HALO - 1, HALO, HALO + 1, nkeys - 4, nkeys - 1]
    pairs = [(a, b) for a in edge for b in edge if a + 3 <= b]
    while len(pairs) < 300:
        a, b = sorted(rng.sample(range(nkeys), 2))
        if a + 3 <= b:
            pairs.append((a, b))
    for a, b in pairs:
        buf = base.copy()
        buf[b:b + 3] = buf[a:a + 3]
        r = model(buf, 0, nkeys, want_flags=True)
        assert r["flags"][a] or r["flags"][b], (a, b)
        assert r["flagged"] == int(r["flags"].sum())
