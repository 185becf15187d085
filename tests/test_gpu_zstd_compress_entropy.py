"""The entropy flags of the device zstd compressor: LA_ZSTDC_FULL_ALPHABET (Huffman literals for any alphabet, the tree
description direct or FSE-coded) and LA_ZSTDC_FIT_TABLES (Predefined / RLE / FSE_Compressed sequence tables per block).

Every image must come back from everything that reads the format -- libzstd one-shot and streaming in 1 000-byte
pieces, the oracle, the device's wave and lane kernels and, for the three-block frames, the block-parallel path -- and
from the plain reader zstd_parse_modes.py, which test_zstd_parse_modes.py holds against libzstd first.  What the
compressor decided is then read from the parsed images alone: the census names each form the flags exist for, the
size checks hold what follows from the format, and the digests of tests/golden/zstd_compress_parent.json (taken from
the library as it was before the flags existed) pin every image written without them."""
import collections
import hashlib
import json
import os

import numpy as np
import pytest

import test_gpu_zstd_compress as T
import zstd_entropy_inputs as I
import zstd_parse_modes as PM
import zstd_support as Z

pytestmark = pytest.mark.gpu

CHECKSUM, RAW_LITERALS, FULL, FIT = 1, 2, 4, 8
OPT_LANE, OPT_BLOCKS = 2, 4
SHAPES = [(131072, 1), (4096, 3), (1000, 2)]
FLAGS = [FULL, FIT, FULL | FIT, FULL | FIT | CHECKSUM]
INPUTS = T.INPUTS + I.entropy_inputs()
DATA = dict(INPUTS)
assert len(DATA) == len(INPUTS)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "zstd_compress_parent.json")

_IMAGES = {}


def image(gpu_ctx, name, shape, flags, parsed=True):
    """(image, parsed frames) of one input; the image is made once per session"""
    key = (name, shape, flags)
    if key not in _IMAGES:
        _IMAGES[key] = [T.compress(gpu_ctx, DATA[name], shape[0], shape[1], flags), None]
    e = _IMAGES[key]
    if not parsed or e[1] is not None:
        return e[0], e[1]
    frames = PM.parse(e[0])
    if flags in (FULL, FIT):        # the census reads these again
        e[1] = frames
    return e[0], frames


def device_decode(gpu_ctx, img, n, options):
    import torch
    from libarchive_amd import zstd
    frames, end_kind, consumed, dst_bytes = zstd.index_image(img)
    assert consumed == len(img) and int(frames["dst_cap"].sum()) == n
    d_src = torch.from_numpy(np.frombuffer(img, dtype=np.uint8).copy()).cuda()
    plan = zstd.ZstdDevicePlan(gpu_ctx, d_src, frames, dst_bytes)
    plan.run(options)
    res = plan.results()
    assert (res["status"] == 0).all(), (options, res["status"])
    assert (res["out_len"] == frames["dst_cap"]).all()
    dst = plan.d_dst.cpu().numpy()
    return b"".join(dst[int(f["dst_off"]):int(f["dst_off"]) + int(f["dst_cap"])].tobytes() for f in frames)


def blocks_of(gpu_ctx, flags, names=None, shapes=SHAPES):
    """(input name, shape, block record) of every compressed block written under `flags`"""
    for name, _ in INPUTS:
        if names is None or name in names:
            for shape in shapes:
                for b in PM.compressed_blocks(image(gpu_ctx, name, shape, flags)[1]):
                    yield name, shape, b


# ---------------------------------------------------------------- 1. round trip
@pytest.mark.parametrize("shape", SHAPES, ids=["%dx%d" % s for s in SHAPES])
@pytest.mark.parametrize("name", [n for n, _ in INPUTS])
def test_round_trip_through_every_reader(gpu_ctx, name, shape):
    z, o = Z.libzstd(), Z.oracle_lib()
    if z is None:
        pytest.fail("no libzstd.so.1 in this image")
    data, n = DATA[name], len(DATA[name])
    for flags in FLAGS:
        img, frames = image(gpu_ctx, name, shape, flags)
        where = (name, shape, flags)
        assert Z.zstd_decompress(z, img, n + 16) == data, where
        assert Z.zstd_stream_decompress(z, img, in_chunk=1000) == (data, "ok"), where
        assert Z.oracle_decode(o, img, n + 16) == (0, data, ""), where
        assert device_decode(gpu_ctx, img, n, 0) == data, where
        assert device_decode(gpu_ctx, img, n, OPT_LANE) == data, where
        if shape[1] == 3:
            assert device_decode(gpu_ctx, img, n, OPT_BLOCKS) == data, where
        assert PM.plain_of(frames) == data, where
        assert all(f["checksum"] == (1 if flags & CHECKSUM else 0) and f["single"] == 1 for f in frames), where


# ---------------------------------------------------------------- 2. census
def _huffman(b):
    return b["lit"]["type"] == 2


def test_census_full_alphabet(gpu_ctx):
    seen = collections.Counter()
    for name, shape, b in blocks_of(gpu_ctx, FULL):
        lit = b["lit"]
        assert lit["type"] != 3, "treeless literals are never written"
        if name == "flat_256" and shape[0] >= 4096:
            hist = collections.Counter(lit["data"])
            if lit["type"] == 0 and len(hist) > 128 and len(set(hist.values())) == 1:
                seen["equal weights, more than 128 symbols: raw"] += 1
        if not _huffman(b):
            continue
        nw, tree = len(lit["weights"]), lit["tree"]
        direct_bytes = 1 + (nw + 1) // 2
        if tree == "fse":
            assert lit["tree_bytes"] - 1 < 128
            assert sum(lit["weight_norm"]) == 1 << lit["weight_al"] and lit["weight_al"] <= 6
            assert sum(1 for c in lit["weight_norm"] if c) >= 2
            assert nw > 128 or lit["tree_bytes"] < direct_bytes, "the FSE form where the direct form is not larger"
            if nw > 128:
                seen["more than 128 weights, header byte below 128"] += 1
            else:
                seen["at most 128 weights, FSE form smaller than direct"] += 1
        else:
            assert nw <= 128
            if len(set(lit["weights"])) > 1:
                seen["direct form kept"] += 1
            elif name == "flat_128":
                seen["equal weights, at most 128 symbols: direct"] += 1
        for largest in (129, 200, 255):
            if nw == largest:
                seen["largest symbol %d" % largest] += 1
    for line in ("more than 128 weights, header byte below 128", "largest symbol 129", "largest symbol 200",
                 "largest symbol 255", "at most 128 weights, FSE form smaller than direct", "direct form kept",
                 "equal weights, more than 128 symbols: raw", "equal weights, at most 128 symbols: direct"):
        assert seen[line] > 0, "no block under LA_ZSTDC_FULL_ALPHABET shows: " + line


def test_census_fit_tables(gpu_ctx):
    seen = collections.Counter()
    for name, shape, b in blocks_of(gpu_ctx, FIT):
        if not b["nseq"]:
            continue
        modes, als, norms = b["modes"], b["als"], b["norms"]
        assert 3 not in modes.values(), "Repeat_Mode is never written"
        for kind in ("ll", "of", "ml"):
            if modes[kind] == 2:
                assert 5 <= als[kind] <= {"ll": 9, "of": 8, "ml": 9}[kind]
                assert all(c >= 0 for c in norms[kind]) and sum(norms[kind]) == 1 << als[kind], (name, shape, kind)
                assert sum(1 for c in norms[kind] if c) >= 2, "FSE_Compressed_Mode for a single symbol"
                used = {s[{"ll": 3, "ml": 4, "of": 5}[kind]] for s in b["seqs"]}
                assert all(norms[kind][c] > 0 for c in used)
                seen[kind + " FSE_Compressed"] += 1
                if als[kind] == 5:
                    seen["accuracy log 5"] += 1
                if als[kind] >= 8:
                    seen["accuracy log 8 or more"] += 1
            elif modes[kind] == 1:
                assert len({s[{"ll": 3, "ml": 4, "of": 5}[kind]] for s in b["seqs"]}) == 1
                seen[kind + " RLE"] += 1
            elif any(m != 0 for m in modes.values()):
                seen[kind + " predefined beside a fitted field"] += 1
        if b["nseq"] < 8 and all(m == 0 for m in modes.values()):
            seen["fewer than 8 sequences, all predefined"] += 1
    lines = [k + t for k in ("ll", "of", "ml") for t in (" FSE_Compressed", " RLE", " predefined beside a fitted field")]
    for line in lines + ["fewer than 8 sequences, all predefined", "accuracy log 5", "accuracy log 8 or more"]:
        assert seen[line] > 0, "no block under LA_ZSTDC_FIT_TABLES shows: " + line


# ---------------------------------------------------------------- 3. sizes
def test_both_flags_never_larger(gpu_ctx):
    for name, _ in INPUTS:
        for shape in SHAPES:
            plain = len(image(gpu_ctx, name, shape, 0, parsed=False)[0])
            both = len(image(gpu_ctx, name, shape, FULL | FIT, parsed=False)[0])
            assert both <= plain, (name, shape, both, plain)


def test_full_alphabet_smaller_on_high_bytes(gpu_ctx):
    for name in ("skewed256", "utf8_text"):
        for shape in SHAPES:
            plain = len(image(gpu_ctx, name, shape, 0, parsed=False)[0])
            full = len(image(gpu_ctx, name, shape, FULL, parsed=False)[0])
            assert full < plain, (name, shape, full, plain)


def test_fit_tables_smaller_on_one_code_sequences(gpu_ctx):
    shape = (131072, 1)
    img, frames = image(gpu_ctx, "rows", shape, FIT)
    (b,) = PM.compressed_blocks(frames)
    assert b["nseq"] >= 4096
    assert len({s[5] for s in b["seqs"]}) == 1 and len({s[4] for s in b["seqs"]}) == 1     # one offset code, one match-length code
    assert len(img) < len(image(gpu_ctx, "rows", shape, 0, parsed=False)[0])


# ---------------------------------------------------------------- 4. the flag-less path did not move
def test_flagless_images_are_the_parents(gpu_ctx):
    with open(GOLDEN) as f:
        golden = json.load(f)
    assert len(golden) == 6 * 3 * 4
    for key, digest in sorted(golden.items()):
        name, bs, bpf, flags = key.split("/")
        img = T.compress(gpu_ctx, DATA[name], int(bs), int(bpf), int(flags))
        assert hashlib.sha256(img).hexdigest() == digest, key


# ---------------------------------------------------------------- 5. nor did the entropy flags' images
GOLDEN_ENTROPY = os.path.join(os.path.dirname(GOLDEN), "zstd_compress_entropy_parent.json")


def pinned_entropy_images(gpu_ctx):
    """(key, image) of everything tests/golden/zstd_compress_entropy_parent.json pins -- written by
    tools/record_zstd_entropy_digests.py from the library as it was before the two copies of the sequence chain became
    one --: every image of this module, from its cache, and the block of test_sequences_that_cost_more_than_they_save,
    seeded as there, which drives the sequence bit writer past its room, through either instance of the kernel"""
    for name, _ in INPUTS:
        for shape in SHAPES:
            for flags in FLAGS:
                yield "%s/%d/%d/%d" % (name, shape[0], shape[1], flags), image(gpu_ctx, name, shape, flags, parsed=False)[0]
    import random
    import zstd_edge_inputs as E
    rnd = random.Random(0xC057)
    T._text(rnd, 131072)
    costly = E.costly_block(rnd)
    for flags in (CHECKSUM, FULL | FIT | CHECKSUM):
        yield "costly_block/131072/1/%d" % flags, T.compress(gpu_ctx, costly, 131072, 1, flags)


def test_entropy_images_are_the_parents(gpu_ctx):
    with open(GOLDEN_ENTROPY) as f:
        golden = json.load(f)
    assert len(golden) == 28 * 3 * 4 + 2
    seen = 0
    for key, img in pinned_entropy_images(gpu_ctx):
        assert hashlib.sha256(img).hexdigest() == golden[key], key
        seen += 1
    assert seen == len(golden)
