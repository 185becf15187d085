"""The schedule of a split last lz4 expand slice without a GPU: libarchive_amd/csrc/la_lz4_slices.h compiled as it stands
(tests/mock_gpu/lz4_slices_shim.c) and checked against a model that marks the slice's blocks group by group.

For every period 4 .. 20, every set of up to four group bounds, every offset of the slice's first block inside the
period and random frame layouts (frames of 0 .. 3 P + 1 blocks, frames in front of the slice, one that ends exactly at
its first block, one that straddles it): the groups partition the slice and the launch grids hold exactly the groups'
blocks, each once; a hash pass reads no block outside the groups launched so far; the passes of a frame cover its
blocks once, in order, each as far as the run of ready blocks goes; the carry index is unique among frames with blocks.
The same properties once more from Python on a few cases, so that a failure can be read without the C."""
import ctypes as C
import os
import subprocess

import pytest

import mock_build

HERE = os.path.dirname(os.path.abspath(__file__))


class Split(C.Structure):
    _fields_ = [("first", C.c_uint32), ("last", C.c_uint32), ("period", C.c_uint32), ("n_groups", C.c_uint32),
                ("bound", C.c_uint32 * 5)]


@pytest.fixture(scope="module")
def lib():
    out = os.path.join(mock_build.out_dir(), "liblz4_slices_rule.so")
    subprocess.check_call([os.environ.get("CC", "cc"), "-O2", "-Wall", "-std=gnu11", "-fPIC", "-shared", "-o", out,
                           os.path.join(HERE, "mock_gpu", "lz4_slices_shim.c")])
    lib = C.CDLL(out)
    for name in ("sl_period", "sl_group_blocks", "sl_grid_x", "sl_grid_y", "sl_block", "sl_ready", "sl_pass_lo",
                 "sl_carry_index", "sl_max_groups", "sl_check_period"):
        getattr(lib, name).restype = C.c_uint32
    lib.sl_check_period.argtypes = [C.c_uint32, C.c_uint64, C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)]
    assert lib.sl_max_groups() == 4
    return lib


@pytest.mark.parametrize("P", range(4, 21))
def test_every_bound_set_and_offset(lib, P):
    what, cases = (C.c_uint32 * 8)(), C.c_uint64(0)
    rc = lib.sl_check_period(P, 0x51CE0000 + P, 3, what, C.byref(cases))
    assert rc == 0, "check %d failed: P %d, bound mask %#x, offset %d, layout %d, group %d, frame %d" % ((rc,) + tuple(what[:6]))
    sets = sum(1 for m in range(1 << (P - 1)) if bin(m).count("1") <= 3)
    assert cases.value == sets * P * 3


def test_period_from_the_batch_shape(lib):
    assert lib.sl_period(262144, 16384) == 16 and lib.sl_period(128, 8) == 16
    assert lib.sl_period(64, 16) == 4 and lib.sl_period(64, 1) == 64
    assert lib.sl_period(48, 16) == 0 and lib.sl_period(130, 2) == 0        # 3 and 65: outside 4 .. 64
    assert lib.sl_period(129, 8) == 0 and lib.sl_period(16, 0) == 0          # not a whole number; no frames


def test_sixteenths_become_bounds(lib):
    def init(P, six):
        sp = Split()
        lib.sl_init(C.byref(sp), 32, 96, P, (C.c_uint32 * len(six))(*six), len(six))
        return list(sp.bound[:sp.n_groups + 1])
    assert init(16, (8, 13, 16)) == [0, 8, 13, 16]
    assert init(16, (12, 16)) == [0, 12, 16]
    assert init(4, (8, 13, 16)) == [0, 2, 3, 4]
    assert init(5, (1, 2, 16)) == [0, 5]                # bounds that round to nothing are dropped
    assert init(64, (8, 13, 16)) == [0, 32, 52, 64]
    assert init(7, (16,)) == [0, 7]


def test_the_same_from_python(lib):
    """P = 16, bounds (8, 13, 16), the slice shifted by 5 against the frames: what each pass takes, in plain sight"""
    first, P, bound = 37, 16, (0, 8, 13, 16)
    frames, at = [], 20
    for nb in (5, 12, 0, 16, 1, 2, 3, 15, 16, 17, 33, 49, 7):
        frames.append((at, nb))
        at += nb
    last = at
    group = {i: max(g for g in range(3) if bound[g] <= (i - first) % P) for i in range(first, last)}
    used = set()
    for fb, nb in frames:
        if nb == 0 or fb + nb <= first:
            continue
        pos = 0
        for g in range(3):
            lo = lib.sl_pass_lo(first, P, bound[g], fb, nb)
            hi = lib.sl_ready(first, P, bound[g + 1], fb, nb)
            assert lo == pos <= hi <= nb
            assert all(fb + k < first or group[fb + k] <= g for k in range(lo, hi))
            assert hi == nb or group[fb + hi] > g
            pos = hi
        assert pos == nb
        ci = lib.sl_carry_index(first, fb, nb)
        assert ci == fb + nb - 1 - first and ci not in used
        used.add(ci)
