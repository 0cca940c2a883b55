"""The LZ78 encoder's scratch plan (my_compress_amd/csrc/fcx_lz78.hip: geometry, field list, batch rule)
through libfcx.so's development export fcx_debug_lz78_plan: pure host arithmetic, no GPU.  The expected
values are worked out by hand from the rules the encoder has always applied and from the field sizes in
the comments of its `struct Scratch`."""
import ctypes

import pytest

import my_compress_amd as mc

MIB, GIB = 1 << 20, 1 << 30
BUDGET = 64 * GIB          # scratch of one batch
REC78 = 19 * 4             # struct Rec78: 19 u32


@pytest.fixture(scope="module")
def L():
    lib = mc.lib()
    lib.fcx_debug_lz78_plan.argtypes = [ctypes.c_uint32, ctypes.c_uint64, ctypes.POINTER(ctypes.c_uint64)]
    return lib


def plan(L, block, n):
    out = (ctypes.c_uint64 * 7)()
    assert L.fcx_debug_lz78_plan(block, n, out) == 0
    return dict(zip(("cap_log2", "Gmax", "tiles", "bmw", "dense1", "per_block", "batch"), list(out)))


def field_bytes(B, cap_log2, Gmax, tiles, bmw, dense1):
    """one block's scratch: the fields of struct Scratch in its order, sizes from its comments"""
    return sum([
        8 << cap_log2,                 # slot      u64 x 2^cap_log2
        (4 << 16) if dense1 else 0,    # d1        u32 x 2^16, null below 64 KiB
        4 * B,                         # idx       u32 x B
        B,                             # c         u8 x B
        4 * bmw,                       # bm        u32 x bmw
        4 * bmw,                       # rbase     u32 x bmw
        2 * B,                         # grp       u16 x B
        B,                             # gpos      u8 x B
        4 * Gmax,                      # gcnt      u32 x Gmax
        4 * 256,                       # chist     u32 x 256
        4 * Gmax,                      # gcode     u32 x Gmax
        Gmax,                          # glen      u8 x Gmax
        4 * 256,                       # ccode     u32 x 256
        256,                           # clen      u8 x 256
        4 * 2 * Gmax,                  # tree      u32 x 2 Gmax
        4 * 2 * Gmax,                  # par       u32 x 2 Gmax
        4 * Gmax,                      # iw        u32 x Gmax
        576,                           # chdr      u8 x 576
        4 * 2 * tiles,                 # tbits     u32 x 2 tiles
        4 * (B + 2),                   # gstage    u32 x (B + 2)
        4 * (B + 2),                   # cstage    u32 x (B + 2)
        REC78,                         # rec       Rec78
        8,                             # off       u64
    ])


def old_estimate(B, cap_log2, dense1):
    """the bound the call applied before: (8 << cap_log2) + 256 KiB + 64 Gmax + 24 B + 4096"""
    return (8 << cap_log2) + ((1 << 18) if dense1 else 0) + 64 * max(1024, B // 256 + 2) + 24 * B + 4096


# B: cap_log2, Gmax, tiles, bmw, dense1, by hand
GEOMETRY = {
    1: (10, 1024, 1, 2, 0),
    255: (10, 1024, 1, 9, 0),
    4096: (13, 1024, 1, 130, 0),          # 2^12 < 4098
    65535: (17, 1024, 8, 2049, 0),        # 2^16 < 65537; 65536 tokens fill 8 tiles
    65536: (17, 1024, 9, 2050, 1),
    MIB: (21, 4098, 129, 32770, 1),       # 2^20 < 2^20 + 2
}


@pytest.mark.parametrize("B", sorted(GEOMETRY))
def test_fields(L, B):
    cap_log2, Gmax, tiles, bmw, dense1 = GEOMETRY[B]
    # the hand values follow the rules
    assert cap_log2 == min(c for c in range(10, 32) if (1 << c) >= B + 2)
    assert Gmax == max(1024, B // 256 + 2)
    assert tiles == -(-(B + 1) // 8192)
    assert bmw == B // 32 + 2
    assert dense1 == (B >= 65536)
    p = plan(L, B, B)
    assert (p["cap_log2"], p["Gmax"], p["tiles"], p["bmw"], p["dense1"]) == GEOMETRY[B]
    assert p["per_block"] == field_bytes(B, *GEOMETRY[B])
    assert p["per_block"] <= old_estimate(B, cap_log2, dense1)


@pytest.mark.parametrize("B,n,batch", [
    (MIB, GIB, 1024),
    (65536, 20 * MIB + 999, 321),
    (4096, GIB, 262144),
    (MIB, 3 * GIB, 1024),
])
def test_batch(L, B, n, batch):
    assert plan(L, B, n)["batch"] == batch


def test_batch_bound_by_budget(L):
    # 1 KiB blocks of 1 GiB: the one case where the budget bound the rule before
    p = plan(L, 1024, GIB)
    assert old_estimate(1024, 11, 0) == 110592
    assert p["batch"] >= BUDGET // 110592 == 621378
    assert p["batch"] * p["per_block"] <= BUDGET
    assert p["batch"] <= GIB // 1024
