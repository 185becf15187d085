"""The hand-built bzip2 streams of tests/bzip2_build.py through the device ABI (la_gpu_bzip2_scan / la_gpu_bzip2_decode, by
the parallel and the serial chase, in slots of the stream's own level and of level 9) and through the filter
(la_api.cat).

What is expected comes from the builder's model, whose sha256 per case is libbz2 1.0.8's by
tests/golden/bzip2_handbuilt.json (tests/test_bzip2_handbuilt.py keeps that file honest where that libbz2 is at hand),
so a GPU machine is held to libbz2's answers without needing a particular libbz2."""
import hashlib
import json
import os

import numpy as np
import pytest

import bzip2_build as B
import bzip2_support as BS
import la_api

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "bzip2_handbuilt.json")
LA_ST_OK, LA_ST_BZ2_DATA, LA_ST_BZ2_TRUNCATED, LA_ST_BZ2_BAD_CRC, LA_ST_BZ2_REFUTED = 0, 20, 21, 22, 23
STOP_TABLE, STOP_ENTRY, STOP_SHORT = 0, 1, 3
SERIAL = 1
NONE = 0xFFFFFFFF
NAMES = [c.name for c in B.handbuilt_cases()]


@pytest.fixture(scope="module")
def cases():
    return {c.name: c for c in B.handbuilt_cases()}


@pytest.fixture(scope="module")
def gold():
    return {r["name"]: r for r in json.load(open(GOLDEN))}


def _sha(b):
    return hashlib.sha256(b).hexdigest()


def _entries(image, marks):
    """(indices of the stream's own units in the candidate table, indices of the planted ones)"""
    magics = BS.find_magics(image)
    real = [magics.index(m) for m in marks]
    return magics, real, [i for i in range(len(magics)) if i not in real]


def _check_abi(gpu_ctx, c, row, options, slot_level):
    from libarchive_amd import bzip2
    what = (c.name, options, slot_level)
    assert _sha(c.image) == row["image_sha256"], what
    out, res, st, _ = bzip2.decode_image(gpu_ctx, c.image, slot_level=slot_level, options=options)
    magics, real, planted = _entries(c.image, c.marks)
    assert len(res) == len(magics), what
    for i in planted:
        assert int(res["status"][i]) == LA_ST_BZ2_REFUTED and int(res["out_len"][i]) == 0, what
    if c.name.startswith("false-"):
        assert planted, what
    if c.valid:
        assert out == c.plain and (len(out), _sha(out)) == (row["out_len"], row["out_sha256"]), (what, len(out), len(c.plain))
        for i in real:
            assert int(res["status"][i]) == LA_ST_OK and int(res["crc"][i]) == int(res["stored_crc"][i]), (what, i)
        assert int(st["stop"]) == STOP_SHORT and int(st["first_bad"]) == NONE and int(st["total_out"]) == len(c.plain), what
        assert int(st["start_bit"]) == len(c.image) * 8 == row["total_in"] * 8 and int(st["open"]) == 0, what
        return
    bad = real[c.bad]
    for i in real[:c.bad]:
        assert int(res["status"][i]) == LA_ST_OK and int(res["crc"][i]) == int(res["stored_crc"][i]), (what, i)
    if c.cls == "crc" or c.end_run:
        assert int(st["first_bad"]) == bad, (what, int(st["first_bad"]), int(st["stop"]))
        assert int(res["status"][bad]) == (LA_ST_BZ2_DATA if c.end_run else LA_ST_BZ2_BAD_CRC), what
    else:
        assert (int(st["stop"]), int(st["stop_entry"]), int(st["first_bad"])) == (STOP_ENTRY, bad, NONE), (what, int(st["stop"]), int(st["stop_entry"]))
        assert int(res["status"][bad]) == (LA_ST_BZ2_TRUNCATED if c.cls == "truncated" else LA_ST_BZ2_DATA), (what, int(res["status"][bad]))
    # what is delivered in front of the error is what libbz2 wrote there
    want = (len(c.plain), row["written_sha256"]) if c.end_run else (row["out_len"], row["out_sha256"])
    assert int(st["total_out"]) == len(out) and (len(out), _sha(out)) == want and out == c.plain, (what, len(out), want[0])


@pytest.mark.parametrize("options", [0, SERIAL], ids=["parallel_chase", "serial_chase"])
@pytest.mark.parametrize("name", NAMES)
def test_abi(gpu_ctx, cases, gold, name, options):
    c = cases[name]
    for slot_level in sorted({c.level, 9}):
        _check_abi(gpu_ctx, c, gold[name], options, slot_level)


def test_the_catalogue_is_the_recorded_one(cases, gold):
    assert sorted(cases) == sorted(gold) and len(cases) >= 70 and sum(1 for c in cases.values() if not c.valid) >= 25


@pytest.mark.parametrize("options", [0, SERIAL], ids=["parallel_chase", "serial_chase"])
def test_packed_streams(gpu_ctx, cases, options):
    """64 small valid cases as concatenated streams in one image, one call: blocks decoded beside each other in separate
    workgroups do not disturb one another"""
    from libarchive_amd import bzip2
    small = [c for c in cases.values() if c.valid and c.level == 1 and len(c.image) <= 1200 and len(c.plain) <= 4096]
    assert len(small) >= 40
    picked = (small + small)[:64]
    image = b"".join(c.image for c in picked)
    plain = b"".join(c.plain for c in picked)
    marks, off = [], 0
    for c in picked:
        marks += [(off * 8 + b, k) for b, k in c.marks]
        off += len(c.image)
    magics, real, planted = _entries(image, marks)
    assert len(planted) >= 32
    out, res, st, _ = bzip2.decode_image(gpu_ctx, image, slot_level=1, options=options)
    assert len(res) == len(magics) and out == plain
    assert [int(res["status"][i]) for i in planted] == [LA_ST_BZ2_REFUTED] * len(planted)
    assert all(int(res["status"][i]) == LA_ST_OK and int(res["crc"][i]) == int(res["stored_crc"][i]) for i in real)
    assert int(st["stop"]) == STOP_SHORT and int(st["first_bad"]) == NONE and int(st["total_out"]) == len(plain)
    dst = np.concatenate(([0], np.cumsum([len(c.plain) for c in picked])))
    firsts = [real[sum(len(c.marks) for c in picked[:k])] for k in range(len(picked))]
    assert [int(res["dst_off"][i]) for i in firsts] == [int(x) for x in dst[:-1]]


@pytest.mark.parametrize("name", NAMES)
def test_filter(gpu_ctx, cases, gold, name):
    """la_api.cat gives what the reference's read loop over libbz2 gave when the golden file was recorded"""
    c, row = cases[name], gold[name]
    data, rc, msg = la_api.as_reference_tuple(la_api.cat(c.image))
    assert [len(data), _sha(data), rc, msg] == row["reference_cat"], (name, len(data), rc, msg)
    if c.valid:
        assert data == c.plain
    else:       # the reference hands out whole 64 KiB blocks in front of an error
        assert data == c.plain[:len(c.plain) & ~0xFFFF]


@pytest.mark.parametrize("part", range(6))
def test_cut_at_every_byte(gpu_ctx, part):
    """the prefix stream (two blocks, the second at an unaligned bit, a false block magic in the first one's selectors)
    cut at every byte: nothing is delivered in front of the cut, as the reference, whose first 64 KiB block never fills
    (tests/test_bzip2_handbuilt.py holds this expectation to the reference's loop)"""
    image, plains, _ = B.prefix_stream()
    assert la_api.as_reference_tuple(la_api.cat(image)) == (b"".join(plains), 0, "")
    for cut in range(14 + part, len(image), 6):
        assert la_api.as_reference_tuple(la_api.cat(image[:cut])) == (b"", la_api.ARCHIVE_FATAL, "truncated bzip2 input"), cut


def test_abi_cut_at_every_byte(gpu_ctx):
    """the prefix stream cut at every byte through the device ABI: the unit the cut falls in is LA_ST_BZ2_TRUNCATED (never
    a data error: no bit behind the source's end counts), the blocks in front of it are delivered, and where the cut
    leaves fewer than 48 bits of the next magic the table simply ends (LA_BZ2_STOP_TABLE).  The second block starts at an
    unaligned bit, and the false magic in the first block's selectors stays refuted in every prefix that holds it."""
    from libarchive_amd import bzip2
    image, plains, marks = B.prefix_stream()
    ends = [marks[1][0], marks[2][0], marks[2][0] + 80]     # where each unit's last bit is read
    assert marks[1][0] % 8
    for cut in range(14, len(image)):
        out, res, st, _ = bzip2.decode_image(gpu_ctx, image[:cut], slot_level=1)
        magics = BS.find_magics(image[:cut])
        assert len(res) == len(magics), cut
        unit = next(k for k in range(3) if cut * 8 < ends[k])
        assert out == b"".join(plains[:unit]) and int(st["total_out"]) == len(out) and int(st["first_bad"]) == NONE, cut
        if marks[unit] in magics:
            i = magics.index(marks[unit])
            assert (int(st["stop"]), int(st["stop_entry"]), int(res["status"][i])) == (STOP_ENTRY, i, LA_ST_BZ2_TRUNCATED), cut
        else:
            assert int(st["stop"]) == STOP_TABLE and int(st["start_bit"]) == marks[unit][0], cut
        for i, m in enumerate(magics):
            if m not in marks:
                assert int(res["status"][i]) == LA_ST_BZ2_REFUTED and int(res["out_len"][i]) == 0, cut
