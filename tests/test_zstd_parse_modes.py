"""The reader the entropy tests of the device compressor take their census from (zstd_parse_modes.py), checked against
libzstd's own output before anything the device writes is judged with it: frames made by the image's libzstd at
levels 1, 3 and 19 over text, a skewed 256-symbol source, gaussian floats and the generator's five kinds, 1 KiB to
256 KiB, must come back from the reader's own reconstruction, and together they must have taken the reader through an
FSE-form Huffman tree and through FSE_Compressed and RLE sequence tables."""
import random

import pytest

import zstd_entropy_inputs as I
import zstd_parse_modes as PM
import zstd_support as Z


def _shapes():
    rnd = random.Random(0x9A5E)
    shapes = [("text", I.text(rnd, 262144)), ("skewed256", I.skewed256(rnd, 262144)), ("gaussian_f32", I.gaussian_f32(5, 262144))]
    shapes += [("gen%d" % k, Z.gen(rnd, 65536, k)) for k in range(5)]
    return shapes


SHAPES = _shapes()
CENSUS = {"tree_fse": 0, "tree_direct": 0, "fse": 0, "rle": 0, "predefined": 0, "repeat": 0, "frames": 0}


def _sizes(name, data):
    return [n for n in (1024, 20000, 65536, 262144) if n <= len(data)]


@pytest.mark.parametrize("name,data", SHAPES, ids=[n for n, _ in SHAPES])
def test_libzstd_frames_reconstruct(name, data):
    z = Z.libzstd()
    if z is None:
        pytest.fail("no libzstd.so.1 in this image")
    for n in _sizes(name, data):
        for level in (1, 3, 19):
            img = Z.zstd_compress(z, data[:n], level)
            frames = PM.parse(img)
            assert PM.plain_of(frames) == data[:n], (name, n, level)
            CENSUS["frames"] += 1
            for b in PM.compressed_blocks(frames):
                if b["lit"]["tree"]:
                    CENSUS["tree_" + b["lit"]["tree"]] += 1
                    if b["lit"]["tree"] == "fse":
                        assert sum(abs(c) for c in b["lit"]["weight_norm"]) == 1 << b["lit"]["weight_al"]
                for kind in ("ll", "of", "ml"):
                    if b["modes"]:
                        CENSUS[PM.MODE_NAMES[b["modes"][kind]]] += 1
                        if b["modes"][kind] == 2:
                            assert sum(abs(c) for c in b["norms"][kind]) == 1 << b["als"][kind]


def test_census_of_the_libzstd_frames():
    """(runs behind the frames above: the counters are theirs)"""
    assert CENSUS["frames"] >= 3 * len(SHAPES), "run together with test_libzstd_frames_reconstruct"
    assert CENSUS["tree_fse"] > 0, "no FSE-form Huffman tree among libzstd's frames: that path of the reader is untested"
    assert CENSUS["fse"] > 0, "no FSE_Compressed sequence table among libzstd's frames"
    assert CENSUS["rle"] > 0, "no RLE sequence table among libzstd's frames"
    assert CENSUS["predefined"] > 0, "no predefined sequence table among libzstd's frames"


def test_refusals():
    """what the reader does not take is an error, not a wrong answer"""
    z = Z.libzstd()
    img = bytearray(Z.zstd_compress(z, SHAPES[0][1][:20000], 3))
    with pytest.raises(PM.ParseError):
        PM.parse(bytes(img[:4]) + b"\x2b" + bytes(img[5:]))         # reserved bit and dictionary id
    with pytest.raises(PM.ParseError):
        PM.parse(b"\x00" + bytes(img))                               # no magic
