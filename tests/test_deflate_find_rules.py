"""The candidate rule of the block-start finder (libarchive_amd/csrc/la_deflate_find_dev.h), compiled for the host
(tests/mock_gpu/deflate_find_shim.cpp), against the plain-Python model of tests/deflate_find_support.py at EVERY bit
of its inputs, and against zlib's own list of block starts (inflate with Z_BLOCK): the rule may call a false position a
candidate, it may never miss a true non-final dynamic block start.  The quick form (what the first kernel pass tests) must
hold wherever the full rule does."""
import ctypes as C
import random
import subprocess

import pytest

import deflate_build as B
import deflate_find_support as F
import mock_build

NOISE_SEED = 20261019


@pytest.fixture(scope="module")
def rules():
    lib = C.CDLL(mock_build.rules("libdeflate_find_rules.so"))
    lib.deflate_find_scan.argtypes = [C.c_char_p, C.c_uint64, C.c_char_p]
    lib.deflate_find_scan.restype = C.c_uint64
    return lib


def scan(lib, data):
    out = C.create_string_buffer(max(8 * len(data), 1))
    n = lib.deflate_find_scan(bytes(data), len(data), out)
    flags = out.raw[:8 * len(data)]
    full = [p for p, f in enumerate(flags) if f & 2]
    assert len(full) == n
    assert all(flags[p] & 1 for p in full), "a candidate the quick test refuses"
    return full, sum(1 for f in flags if f & 1)


@pytest.fixture(scope="module")
def inputs():
    """name -> (bytes, is a deflate body).  The bodies are cut to 48 KiB: several blocks, and a last header that the cut
    may run through."""
    text = F.word_text(400000, seed=11)
    return {
        "noise": (random.Random(NOISE_SEED).randbytes(32768), False),
        "level6": (F.raw_deflate(text, 6)[:49152], True),
        "level9": (F.raw_deflate(text, 9)[:49152], True),
        "level1": (F.raw_deflate(text, 1)[:49152], True),
    }


@pytest.mark.parametrize("name", ["noise", "level6", "level9", "level1"])
def test_header_agrees_with_the_model_at_every_bit(rules, inputs, name):
    data, is_body = inputs[name]
    full, quick = scan(rules, data)
    assert full == F.model_candidates(data), name
    assert quick < len(data) * 8 // 500, "the quick test lets through far more than one position in about 2 200"
    if is_body:
        text = F.word_text(400000, seed=11)
        level = {"level6": 6, "level9": 9, "level1": 1}[name]
        whole = F.raw_deflate(text, level)
        # a true start counts when its whole header lies in front of the cut: the model says which
        true = [p for p in F.true_candidates(whole, behind=-1) if p < 8 * len(data) and F.is_candidate(data, p)]
        missing = [p for p in true if p not in set(full)]
        assert not missing, missing
        if level != 1:
            assert len(true) >= 2, "the input holds too few dynamic blocks to show anything"
        # and where the cut does not interfere the model itself must know every true start
        uncut = [p for p in F.true_candidates(whole, behind=-1) if p + 8 * F.HEADER_BYTES < 8 * len(data)]
        assert all(F.is_candidate(data, p) for p in uncut)


def _header_cases():
    text = list(b"a dynamic block, hand made. ")
    ll2 = [0] * 286
    ll2[65], ll2[256], ll2[257] = 2, 2, 1
    only_eob = [0] * 257
    only_eob[256] = 1
    ll3 = [0] * 257
    ll3[65], ll3[66], ll3[256] = 1, 1, 1
    ll4 = [0] * 257
    ll4[65], ll4[256] = 2, 2
    no_eob = [0] * 257
    no_eob[65], no_eob[66] = 1, 1
    clc4 = [0] * 19
    clc4[0], clc4[18], clc4[17], clc4[16] = 1, 2, 3, 3
    all8 = [8] * 255 + [0, 8]
    three = [2 if s in (16, 17, 18, 8) else 0 for s in range(19)]
    first16 = [2 if s in (16, 3, 0, 18) else 0 for s in range(19)]
    D, ST_DATA = B.Dynamic, B.ST_DATA
    return [
        # (HCLEN 4 sends lengths for 16, 17, 18 and 0 only: every code length is 0, there is no end-of-block code)
        ("hclen-4", D(None, None, [], hlit=257, hdist=1, hclen=4, clc_lens=clc4, plan=[(18, 127), (17, 7), (0, 0), (16, 3), (18, 93)],
                      refuse=ST_DATA, eob=False, final=0), False),
        ("hclen-19", B._dyn_auto(text, hclen=19, final=0), True),
        ("one-distance-code", D(ll2, [1], [65, (0, 0, 0, 0), 65], final=0), True),
        ("empty-distance-code", B._dyn_auto(text, hdist=1, final=0), True),
        ("one-bit-literal-code", D(only_eob, [1], [], final=0), True),
        ("over-subscribed", D(ll3, [1], [], refuse=ST_DATA, final=0), False),
        ("incomplete", D(ll4, [1], [65], refuse=ST_DATA, final=0), False),
        ("repeat-with-nothing-before-it", D([0] * 257, [0], [], hlit=257, hdist=1, clc_lens=first16, plan=[(16, 3), (3, 0)], refuse=ST_DATA,
                                            eob=False, final=0), False),
        ("repeat-past-hlit-plus-hdist", D(all8, [0], [], hlit=257, hdist=1, clc_lens=three, plan=[(8, 0)] * 254 + [(16, 3)], refuse=ST_DATA,
                                          eob=False, final=0), False),
        ("no-end-of-block-code", D(no_eob, [1], [65], refuse=ST_DATA, eob=False, final=0), False),
        # the same accepted header with BFINAL set is no candidate: nothing starts behind a final block
        ("final", B._dyn_auto(text, hclen=19, final=1), False),
    ]


@pytest.mark.parametrize("lead", [0, 3])
def test_hand_built_headers(rules, lead):
    """lead nine-bit literals of a fixed block in front: the header starts at bit 0 of the stream, or in mid-byte"""
    for name, block, want in _header_cases():
        blocks = ([B.Fixed([200, 201, 250][:lead], final=0)] if lead else []) + [block, B.Fixed([], final=1)]
        image, _, _, _, info = B.build(blocks)
        image += bytes(8)
        at = info["block_bits"][1 if lead else 0]
        full, _ = scan(rules, image)
        assert full == F.model_candidates(image), name
        assert (at in full) == want, (name, at, full)
        verdict, _, _, _ = __import__("deflate_support").zlib_inflate(image)
        assert (verdict != "data") == (want or name == "final"), (name, verdict)


def test_sanitizer_program(inputs, tmp_path):
    """the same header over the same inputs in a program of its own under AddressSanitizer and UBSan, every input in a heap
    buffer of exactly its size"""
    names = sorted(inputs)
    paths = []
    for n in names:
        p = tmp_path / (n + ".bin")
        p.write_bytes(inputs[n][0])
        paths.append(str(p))
    r = subprocess.run([mock_build.program("deflate_find_asan")] + paths, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    for n, line in zip(names, r.stdout.splitlines()):
        size, quick, cands, possum = (int(x) for x in line.split())
        want = F.model_candidates(inputs[n][0])
        assert (size, cands, possum) == (len(inputs[n][0]), len(want), sum(want)), n
        assert quick >= cands
