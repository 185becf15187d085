"""LA_ZSTD_OPT_BLOCK_PARALLEL (la_zstd_blocks.hip): the blocks of a Zstandard frame decoded in parallel, with the
frame kernels behind it for whatever it hands back.  The contract: per frame the same (status, out_len, bytes) as
option 0, `path == 1` where the block path finished the frame, `path == 0` and the frame kernel's status where it did
not -- it never refuses a frame itself and never accepts what the wave kernel refuses.

Frames are the hand-built ones of tests/zstd_build.py (expected statuses as in test_gpu_zstd_handbuilt.py), shapes
built here at the places where a stage can go wrong, libzstd's own frames, and one stream through the filter
(LA_ZSTD_BLOCKS=1)."""
import random

import numpy as np
import pytest

import la_api
import zstd_build as B
import zstd_support as Z
from test_gpu_zstd_handbuilt import GUARD, REFUSED_CAP, _expected_status

pytestmark = pytest.mark.gpu

OPT_NO_VERIFY, OPT_LANE, OPT_BLOCKS = 1, 2, 4
ZB_MAX_WAVES = 4096             # la_zstd_blocks.hip: the largest grid of the per-block kernels (one wave per block)
ARCHIVE_FILTER_ZSTD = 14


@pytest.fixture(scope="module")
def cases():
    return B.handbuilt_cases()


def run_table(gpu_ctx, entries, options):
    """entries: [(image, dst_cap)], one slot per frame with 64 guard bytes between slots (the layout of
    test_gpu_zstd_handbuilt.run_table).  Returns [(status, out_len, bytes, path)] and checks the guard."""
    import torch
    from libarchive_amd import zstd
    frames = np.zeros(len(entries), dtype=zstd.ZSTD_FRAME_DTYPE)
    src, so, do = [], 0, 64
    for i, (img, cap) in enumerate(entries):
        frames[i] = (so, len(img), do, cap)
        src.append(img)
        so += len(img)
        do += ((cap + 15) & ~15) + 64
    image = b"".join(src) + bytes(64)
    d_src = torch.from_numpy(np.frombuffer(image, dtype=np.uint8).copy()).cuda()
    plan = zstd.ZstdDevicePlan(gpu_ctx, d_src, frames, do)
    plan.d_dst.fill_(GUARD)
    plan.batch.src_bytes = so
    plan.run(options)
    res = plan.results()
    dst = plan.d_dst.cpu().numpy()[:do]
    untouched = np.ones(do, dtype=bool)
    out = []
    for i, (img, cap) in enumerate(entries):
        st, n, off = int(res["status"][i]), int(res["out_len"][i]), int(frames["dst_off"][i])
        assert n <= cap, i
        untouched[off:off + (n if st == 0 else cap)] = False
        out.append((st, n, dst[off:off + n].tobytes(), int(res["path"][i])))
    assert (dst[untouched] == GUARD).all(), "bytes outside the frames' slots changed"
    return out


def both(gpu_ctx, entries, extra=0):
    """the table under the block path and under the frame kernel alone; the verdicts and bytes must be the same"""
    blk, ref = run_table(gpu_ctx, entries, OPT_BLOCKS | extra), run_table(gpu_ctx, entries, extra)
    for i, (a, b) in enumerate(zip(blk, ref)):
        assert a[:3] == b[:3], (i, a[:2], b[:2])
        assert b[3] == 0, i
        assert a[3] in (0, 1) and (a[0] == 0 or a[3] == 0), (i, "the block path reports success only")
    return blk


def test_every_handbuilt_case_like_the_wave_kernel(gpu_ctx, cases):
    o = Z.oracle_lib()
    entries, want = [], []
    for c in cases:
        entries.append((c.image, len(c.plain) if c.valid else REFUSED_CAP))
        want.append((c.name, _expected_status(o, c), c.plain, c.valid))
    entries.append((B.skippable(b"skip me", 3), 16)); want.append(("skippable", B.ST_OK, b"", False))
    for name, blocks in (("raw", [B.Raw(B.HIST)]), ("rle", [B.Raw(b"ab"), B.Rle(5, 300)]),
                         ("sequences", [B.Raw(B.HIST), B.Comp(b"abcdef", [(2, 5, 3 + 7), (1, 6, 3 + 9)])]),
                         ("literals-only", [B.Raw(B.HIST), B.Comp(b"abcdef" * 9, [])])):
        img, plain = B.frame(blocks)
        entries.append((img, len(plain))); want.append(("fits-" + name, B.ST_OK, plain, True))
        entries.append((img, len(plain) - 1)); want.append(("one-byte-short-" + name, B.ST_OUT_FULL, None, False))
    assert sum(1 for c in cases if c.valid) == 643 and len(cases) == 811
    got = both(gpu_ctx, entries)
    handed_back = []
    for (name, status, plain, valid), g in zip(want, got):
        assert g[0] == status, (name, g[0], status)
        if status == B.ST_OK:
            assert g[1] == len(plain) and g[2] == plain, name
        else:
            assert g[3] == 0, name
        if valid and g[3] != 1:
            handed_back.append(name)
    assert not handed_back, ("valid frames were handed back", len(handed_back), handed_back[:20])


def _block_spans(img):
    """[(first byte, end) of every block's content] of the frame at the head of img"""
    fhd = img[4]
    single = (fhd >> 5) & 1
    p = 5 + (0 if single else 1) + (0, 1, 2, 4)[fhd & 3] + (single if fhd >> 6 == 0 else (0, 2, 4, 8)[fhd >> 6])
    spans = []
    while True:
        bh = int.from_bytes(img[p:p + 3], "little")
        size = 1 if (bh >> 1) & 3 == 1 else bh >> 3
        spans.append((p + 3, p + 3 + size))
        p += 3 + size
        if bh & 1:
            return spans


def test_shapes_at_the_stages_edges(gpu_ctx):
    rnd = random.Random(0xB10C)
    other = bytes(rnd.randrange(256) for _ in range(64))
    text = bytes(97 + min(int(rnd.expovariate(0.4)), 25) for _ in range(3000))
    sq = [(2, 5, 3 + 7)] * 3 + [(1, 6, 3 + 9)]
    valid = {
        "match-from-frame-byte-0": [B.Raw(B.HIST), B.Raw(b"0123456789"), B.Comp(b"", [(0, 5, 3 + 74)])],
        "match-straddles-two-earlier-blocks": [B.Raw(B.HIST), B.Raw(other), B.Comp(b"", [(0, 20, 3 + 74)])],
        # the largest match a block can hold (Block_Maximum_Size), offset 1, on the block's first byte
        "offset-1-ml-128k-on-a-blocks-first-byte": [B.Raw(B.HIST), B.Comp(b"", [(0, B.BLOCK_MAX, 3 + 1)])],
        "copy-of-a-copy-of-a-copy": [B.Raw(B.HIST), B.Comp(b"", [(0, 30, 3 + 64)]), B.Comp(b"", [(0, 30, 3 + 30)]),
                                     B.Comp(b"", [(0, 30, 3 + 30)])],
        "repeat-tables-over-other-blocks": [
            B.Raw(B.HIST),
            B.Comp(text[:700], sq, ll=B.Table("fse"), of=B.Table("fse"), ml=B.Table("fse"),
                   lit=B.Lit("huf", streams=1, weights=B.huf_weights_for(text))),
            B.Comp(b"no sequences", []), B.Raw(b"raw between"), B.Rle(7, 40),
            B.Comp(text[700:2200], sq[:3], ll=B.Table("repeat"), of=B.Table("repeat"), ml=B.Table("repeat"),
                   lit=B.Lit("treeless", streams=4))],
        "one-block": [B.Comp(b"abcdefgh", [(8, 9, 3 + 3)])],
        "empty-last-raw-block": [B.Raw(B.HIST), B.Comp(b"xy", [(1, 4, 3 + 9)]), B.Raw(b"")],
    }
    entries, names, plains = [], [], []
    for name, blocks in valid.items():
        for cs in (False, True):
            kw = {"window": (8, 0), "single": False} if "128k" in name else {}
            img, plain = B.frame(blocks, checksum=cs, **kw)
            entries.append((img, len(plain))); names.append(name); plains.append(plain)
    refused = {
        "match-one-byte-in-front-of-the-frame": [B.Raw(B.HIST), B.Raw(b"0123456789"), B.Comp(b"", [(0, 5, 3 + 75)])],
        # the largest Match_Length the codes can say is more than a block may produce
        "offset-1-ml-131074": [B.Raw(B.HIST), B.Comp(b"", [(0, 131074, 3 + 1)])],
        "repeat-without-a-definer": [B.Raw(B.HIST), B.Comp(b"abcdef", [(2, 5, 3 + 7)], ll=B.Table("repeat"))],
        # block 2 leaves repeat offset 1 behind; block 3 asks for rep[0] - 1
        "carried-rep0-less-1-is-0": [B.Raw(B.HIST), B.Comp(b"ab", [(1, 4, 3 + 1)]), B.Comp(b"", [(0, 3, 3)])],
    }
    for name, blocks in refused.items():
        img, _ = B.frame(blocks, strict=False, window=(8, 0), single=False)
        entries.append((img, REFUSED_CAP)); names.append(name); plains.append(None)
    got = both(gpu_ctx, entries)
    for name, plain, g in zip(names, plains, got):
        if plain is not None:
            assert (g[0], g[1], g[3]) == (B.ST_OK, len(plain), 1) and g[2] == plain, name
        else:
            assert (g[0], g[3]) == (B.ST_CORRUPT, 0), name


def test_a_frame_beyond_the_block_capacity_is_handed_back(gpu_ctx):
    """300 raw blocks of one byte: 1200-odd bytes of frame, 4 + src_len / 16 + dst_cap / 65536 = 79 block entries"""
    many, many_plain = B.frame([B.Raw(bytes([i & 0xFF])) for i in range(300)], single=False, window=(0, 0))
    assert 4 + len(many) // 16 + len(many_plain) // 65536 == 79
    a, ap = B.frame([B.Raw(B.HIST), B.Comp(b"abcdef", [(2, 5, 3 + 7), (1, 6, 3 + 9)]), B.Rle(3, 100)], checksum=True)
    b, bp = B.frame([B.Raw(B.HIST), B.Comp(b"", [(0, 30, 3 + 64)]), B.Comp(b"", [(0, 30, 3 + 30)])])
    got = both(gpu_ctx, [(a, len(ap)), (many, len(many_plain)), (b, len(bp))])
    assert [(g[0], g[3]) for g in got] == [(0, 1), (0, 0), (0, 1)]
    assert [g[2] for g in got] == [ap, many_plain, bp]


def test_batches_beyond_the_grids_stride(gpu_ctx, cases):
    """more frames than the per-frame kernels' grid, and more blocks than the per-block kernels' (ZB_MAX_WAVES)"""
    o = Z.oracle_lib()
    small = [c for c in cases if len(c.image) <= 400 and (not c.valid or len(c.plain) <= 4096)]
    status = {c.name: _expected_status(o, c) for c in small}
    pick = [small[(i * 7) % len(small)] for i in range(4100)]
    got = both(gpu_ctx, [(c.image, len(c.plain) if c.valid else 4096 + 64) for c in pick])
    for c, g in zip(pick, got):
        assert g[0] == status[c.name], (c.name, g[0])
        assert g[3] == (1 if c.valid else 0), c.name
        if c.valid:
            assert g[2] == c.plain, c.name
    # three frames of 1500 blocks each: raw, RLE and compressed blocks in turn, every match into the block before
    rnd = random.Random(77)
    blocks = [B.Raw(B.HIST)]
    for i in range(1500):
        blocks.append([B.Raw(bytes(rnd.randrange(256) for _ in range(61))), B.Rle(i & 0xFF, 40),
                       B.Comp(b"abcdefgh", [(3, 30, 3 + 45), (2, 7, 1)])][i % 3])
    img, plain = B.frame(blocks, checksum=True)
    assert 3 * len(blocks) > ZB_MAX_WAVES and len(blocks) < 4 + len(img) // 16 + len(plain) // 65536
    got = both(gpu_ctx, [(img, len(plain))] * 3)
    assert [(g[0], g[3]) for g in got] == [(0, 1)] * 3 and all(g[2] == plain for g in got)


def test_options_beside_the_block_path(gpu_ctx, cases):
    c = next(x for x in cases if x.name == "bad-checksum")
    img, plain = B.frame([B.Raw(B.HIST), B.Comp(b"literals", [(4, 5, 3 + 10), (2, 3, 1)])], checksum=True)
    assert len(img) == len(c.image) and img[:-4] == c.image[:-4]
    assert run_table(gpu_ctx, [(c.image, len(plain))], OPT_BLOCKS) == [(B.ST_BAD_CHECKSUM, 0, b"", 0)]
    assert run_table(gpu_ctx, [(c.image, len(plain))], OPT_BLOCKS | OPT_NO_VERIFY) == [(B.ST_OK, len(plain), plain, 1)]
    # handed-back frames by the lane kernel: one refusal of every status, a valid frame in front of and behind each
    o = Z.oracle_lib()
    by_status = {}
    for x in cases:
        if not x.valid and len(x.image) < 4096:
            by_status.setdefault(_expected_status(o, x), x)
    assert set(by_status) >= {11, 12, 13, 15, 16, 17}
    entries, want = [(img, len(plain))], [(0, 1)]
    for st, x in sorted(by_status.items()):
        entries += [(x.image, REFUSED_CAP), (img, len(plain))]
        want += [(st, 0), (0, 1)]
    entries.append((img, len(plain) - 1)); want.append((B.ST_OUT_FULL, 0))
    got = both(gpu_ctx, entries, OPT_LANE)
    assert [(g[0], g[3]) for g in got] == want


def test_libzstd_frames(gpu_ctx):
    z = Z.libzstd()
    if z is None:
        pytest.skip("no libzstd.so.1 in this image (test inputs are made with it)")
    rnd = random.Random(0x25D)
    entries, plains = [], []
    for kind in range(5):
        d = Z.gen(rnd, (1 << 20) + 1, kind)
        for level in (1, 3, 19):
            entries.append((Z.zstd_compress(z, d, level), len(d))); plains.append(d)
    got = run_table(gpu_ctx, entries, OPT_BLOCKS)
    for i, (g, d) in enumerate(zip(got, plains)):
        assert (g[0], g[1], g[3]) == (0, len(d), 1) and g[2] == d, (i // 3, i % 3, g[0], g[1], g[3])


def test_a_lone_frame_through_the_filter(gpu_ctx, monkeypatch):
    z = Z.libzstd()
    if z is None:
        pytest.skip("no libzstd.so.1 in this image (test inputs are made with it)")
    rnd = random.Random(0xF117)
    plain = Z.gen(rnd, 3 << 20, 1)
    img = Z.zstd_compress(z, plain, 3)
    assert len(img) > (1 << 20), "the frame must end behind the bidder's look-ahead"
    monkeypatch.setenv("LA_ZSTD_BLOCKS", "1")
    monkeypatch.delenv("LA_GPU_BID", raising=False)
    r = la_api.cat(img)
    assert ARCHIVE_FILTER_ZSTD in [c for c, _ in r.filters]
    assert la_api.as_reference_tuple(r) == (plain, 0, "")
    # a byte flipped inside block 5: the same answer as the frame kernel alone gives
    spans = _block_spans(img)
    assert len(spans) > 8
    at = spans[5][0] + (spans[5][1] - spans[5][0]) // 2
    bad = img[:at] + bytes([img[at] ^ 0x5A]) + img[at + 1:]
    got = la_api.as_reference_tuple(la_api.cat(bad))
    monkeypatch.delenv("LA_ZSTD_BLOCKS")
    monkeypatch.setenv("LA_GPU_BID", "all")
    assert got == la_api.as_reference_tuple(la_api.cat(bad))
    assert got != (plain, 0, ""), "the flipped byte changed nothing"
