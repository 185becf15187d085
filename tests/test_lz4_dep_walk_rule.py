"""The lz4 dependency kernel's walk over a block's output positions without a GPU:
libarchive_amd/csrc/la_lz4_dep_walk.h compiled as it stands (tests/mock_gpu/lz4_dep_walk_shim.c) and compared with the
one-step walk  while (q + 1 < bound && pos[q + 1] <= x) q++  that it replaces in la_lz4_deps.hip.

Ascending 16-bit position arrays of ns = 1 .. 20 and 4093 .. 4096 entries (equal neighbours included), once with the
last position at 65 535, the entries behind ns filled with 0 and with 0xFFFF: they are never initialised in the kernel
and must decide nothing.  For ns <= 20 every start q, every bound 0 .. ns and x on, one below and one above every
position; for the large arrays every start and bound within 12 entries of the array's ends and of each other (a walk
reads nothing in front of q + 1 and nothing at or behind the bound, so the distance between the two and to the array's
ends is what a look can get wrong), with x around every position a look from q can see, the block's last positions,
0, 65 535 and values above 16 bits -- among them walks over all 4 096 entries, the loop behind the first look.

The same sweep runs once more as a stand-alone program under -fsanitize=address,undefined, its arrays heap blocks of
exactly the size the header asks for -- 4 096 positions and the entries of one look behind them, which in the kernel are
the first match starts of the same LDS array -- so no read of a look leaves them.  A host program; nothing is preloaded
into Python."""
import ctypes as C
import os
import random
import subprocess

import pytest

import mock_build

HERE = os.path.dirname(os.path.abspath(__file__))
SHIM = os.path.join(HERE, "mock_gpu", "lz4_dep_walk_shim.c")
MAIN = os.path.join(HERE, "mock_gpu", "lz4_dep_walk_main.c")


@pytest.fixture(scope="module")
def lib():
    out = os.path.join(mock_build.out_dir(), "liblz4_dep_walk_rule.so")
    subprocess.check_call([os.environ.get("CC", "cc"), "-O2", "-Wall", "-std=gnu11", "-fPIC", "-shared", "-o", out, SHIM])
    lib = C.CDLL(out)
    for name in ("dw_cap", "dw_look", "dw_walk", "dw_naive", "dw_sweep", "dw_sweep_all"):
        getattr(lib, name).restype = C.c_uint32
    lib.dw_walk.argtypes = lib.dw_naive.argtypes = [C.POINTER(C.c_uint16), C.c_uint32, C.c_uint32, C.c_uint32]
    lib.dw_sweep.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint64, C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)]
    lib.dw_sweep_all.argtypes = [C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)]
    assert lib.dw_cap() == 4096 and 2 <= lib.dw_look() <= 8
    return lib


@pytest.mark.parametrize("ns", list(range(1, 21)) + [4093, 4094, 4095, 4096])
def test_walk_by_looks_is_the_one_step_walk(lib, ns):
    total = 0
    for to_end in (0, 1):
        for garbage in (0, 0xFFFF):
            what, cases = (C.c_uint32 * 8)(), C.c_uint64(0)
            rc = lib.dw_sweep(ns, to_end, garbage, 0xD1A0000 + ns * 4 + to_end + 2 * (garbage != 0), what, C.byref(cases))
            assert rc == 0, "ns %d q %d bound %d x %d: one-step walk %d, by looks %d (tail at 65535: %d, garbage %#x)" % (
                tuple(what[:6]) + (to_end, garbage))
            total += cases.value
    if ns <= 20:    # every q, every bound, at least x on, below and above the positions around q, and the six fixed ones
        assert total >= 4 * ns * (ns + 1) * 9


def test_the_same_from_python(lib):
    """a few walks in plain sight: a look that stops inside, at its last entry, at the bound, behind garbage, and a walk
    of 75 steps over 4-byte sequences"""
    cap = lib.dw_cap()

    def walk(positions, q, bound, x, garbage=0):
        arr = (C.c_uint16 * (cap + lib.dw_look()))(*(list(positions) + [garbage] * (cap + lib.dw_look() - len(positions))))
        got = lib.dw_walk(arr, q, bound, x)
        assert got == lib.dw_naive(arr, q, bound, x)
        return got

    p = [0, 10, 20, 30, 40, 50, 60, 70, 80, 90]
    assert walk(p, 0, 10, 35) == 3 and walk(p, 0, 10, 40) == 4 and walk(p, 0, 10, 39) == 3
    assert walk(p, 0, 10, 1000) == 9 and walk(p, 0, 3, 1000) == 2 and walk(p, 0, 1, 1000) == 0 and walk(p, 0, 0, 1000) == 0
    assert walk(p, 5, 10, 0) == 5 and walk(p, 5, 3, 1000) == 5 and walk(p, 9, 10, 1000) == 9
    assert walk(p[:3], 0, 3, 1000, garbage=0) == 2 and walk(p[:3], 0, 3, 5, garbage=0) == 0
    four = [4 * i for i in range(200)]
    assert walk(four, 10, 200, 4 * 85 + 3) == 85 and walk(four, 10, 60, 4 * 85 + 3) == 59
    rnd = random.Random(0xD1A)
    full = sorted(rnd.randrange(65536) for _ in range(cap - 1)) + [65535]
    assert walk(full, 0, cap, 65535) == cap - 1 and walk(full, cap - 3, cap, 65535) == cap - 1
    assert walk(full, cap - 1, cap, 65535) == cap - 1 and walk(full, 0, cap - 1, 0xFFFFFFFF) == cap - 2


def test_sweep_under_sanitizers(lib, tmp_path):
    """the whole sweep as a program of its own with -fsanitize=address,undefined: a look that read outside the array, or
    shifted by too much, would end it"""
    exe = str(tmp_path / "lz4_dep_walk_asan")
    subprocess.check_call(["gcc", "-O1", "-g", "-std=gnu11", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-fno-omit-frame-pointer", "-o", exe, SHIM, MAIN])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    what, cases = (C.c_uint32 * 8)(), C.c_uint64(0)
    assert lib.dw_sweep_all(what, C.byref(cases)) == 0
    assert int(out.stdout) == cases.value > 100000
