"""Large lz4 batches: the sliced expand sequence and the parse kernel's two LDS shapes.

A batch of 32 768 blocks or more is expanded in four slices, and a batch of more waves than the chip holds of
the parse kernel's wide shape may be parsed in its narrow one (la_launch_lz4_parse_staged).  Every image here is
a small synthetic stream repeated, with hand-built frames between the repeats so that each of them meets another
slice: a stored block, a bad block checksum, a bad content checksum, a block of more than 4 096 sequences and a
chain of dependent blocks that straddles a slice boundary.  What the device hands back is compared with the
general-only path, with the first-generation parse, with the oracle on the unique pieces and with an image of
the same pieces that is small enough to go through in one slice."""
import random

import numpy as np
import pytest

import oracle_lib as O
import streams as S

pytestmark = pytest.mark.gpu

TILE_FRAMES, BPF, BS = 64, 16, 8192
TILE_BLOCKS = TILE_FRAMES * BPF
DEP_BLOCKS = 900
SLICED_MIN = 4 * 8192          # la_api.hip: batches from this size on are expanded in four slices
WIDE_WAVES = 256 * 6           # la_lz4_parse.hip: waves the chip holds of the wide parse shape


def _big_block_frame():
    """three copies of a 64 KiB block of 13 107 sequences (1 literal + 4-byte match each)"""
    rnd = random.Random(4)
    seqs, plain = bytearray(), bytearray()
    while len(plain) < 65536 - 64:
        lit = rnd.randbytes(1)
        off = rnd.randint(1, min(len(plain) + 1, 65535))
        seqs += bytes([0x10]) + lit + off.to_bytes(2, "little")
        plain += lit
        for _ in range(4):
            plain.append(plain[-off])
    fin = rnd.randbytes(65536 - len(plain))
    seqs += bytes([0xF0]) + bytes([len(fin) - 15]) + fin if len(fin) >= 15 else bytes([len(fin) << 4]) + fin
    plain += fin
    return S.lz4_frame([(bytes(plain), S.lz4_block(bytes(seqs), bsum=True))] * 3, flg=0x74)


def _specials():
    rnd = random.Random(60)
    a, b = rnd.randbytes(3000), rnd.randbytes(500) * 9
    enc = lambda d, **kw: (d, S.lz4_block(S.lz4_compress_block(d), bsum=True, **kw))
    sp = {}
    sp["stored"] = S.lz4_frame([(a, S.lz4_block(a, stored=True, bsum=True)), enc(b)], flg=0x74)
    sp["dependent"] = S.lz4_dependent_frame([rnd.randbytes(rnd.randint(40, 300)) for _ in range(DEP_BLOCKS)])
    sp["bad_block_sum"] = S.lz4_frame([enc(b), enc(a, bad_sum=True)], flg=0x74)
    sp["bad_content_sum"] = S.lz4_frame([enc(a), enc(b)], flg=0x74, bad_content=True)
    sp["big"] = _big_block_frame()
    return sp


N_SPECIAL_BLOCKS = {"stored": 2, "dependent": DEP_BLOCKS, "bad_block_sum": 2, "bad_content_sum": 2, "big": 3}


@pytest.fixture(scope="module")
def pieces():
    tile, tile_plain = S.synth_lz4_stream(0x4C413336, 0, TILE_FRAMES, blocks_per_frame=BPF, block_size=BS, nthreads=4)
    ref, res = O.lz4_stream_decode(tile, tile_plain.size + 16)
    assert res.rc == 0 and ref.tobytes() == tile_plain.tobytes()
    return tile, tile_plain, _specials()


def _build(pieces, ntiles, after):
    """image of ntiles repeats with special `name` behind repeat after[name]; -> image, {name: first block}, {name: frame}"""
    tile, _, sp = pieces
    parts, first_block, frame = [], {}, {}
    nb = nf = 0
    for t in range(ntiles):
        parts.append(tile)
        nb += TILE_BLOCKS
        nf += TILE_FRAMES
        for name, k in after.items():
            if k == t:
                first_block[name], frame[name] = nb, nf
                parts.append(np.frombuffer(sp[name][0], dtype=np.uint8))
                nb += N_SPECIAL_BLOCKS[name]
                nf += 1
    return np.concatenate(parts), first_block, frame, nb


def _run(ctx, image, options):
    """-> per-block and per-frame arrays, summary, decoded slab (device tensor), index"""
    import torch
    from libarchive_amd import _native as N
    from libarchive_amd.lz4 import Lz4DevicePlan
    idx = N.lz4_index(image, at_eof=True)
    d_src = torch.from_numpy(image).to("cuda:0")
    plan = Lz4DevicePlan(ctx, d_src, idx)
    plan.run(options)
    out_len, dst_off, bst, fst = [a.copy() for a in plan.arrays()]
    sm = plan.summary().copy()
    return dict(out_len=out_len, dst_off=dst_off, bst=bst, fst=fst, sm=sm, dst=plan.d_dst[:int(dst_off[-1])], idx=idx)


def _same(a, b):
    import torch
    for k in ("out_len", "dst_off", "bst", "fst"):
        assert np.array_equal(a[k], b[k]), k
    assert a["sm"].tobytes() == b["sm"].tobytes()
    assert torch.equal(a["dst"], b["dst"])


def _slice_of(block, n):
    return max(i for i in range(4) if n * i // 4 <= block)


def _check(gpu_ctx, pieces, ntiles, after, small):
    from libarchive_amd import _native as N
    tile, tile_plain, sp = pieces
    image, fb, fr, nb = _build(pieces, ntiles, after)
    r = _run(gpu_ctx, image, 0)
    n = len(r["idx"].blocks)
    assert n == nb >= SLICED_MIN
    # the specials meet all four slices, and the chain of dependent blocks crosses a boundary
    assert [_slice_of(fb[k], n) for k in ("stored", "bad_block_sum", "bad_content_sum", "big")] == [0, 1, 2, 3]
    assert _slice_of(fb["dependent"], n) + 1 == _slice_of(fb["dependent"] + DEP_BLOCKS - 1, n)
    # (a) the general kernel alone, and the first-generation parse
    _same(r, _run(gpu_ctx, image, N.LA_LZ4_OPT_GENERAL_ONLY))
    _same(r, _run(gpu_ctx, image, N.LA_LZ4_OPT_PARSE_V1))
    # (b) the oracle on the unique pieces: every repeat of the tile, every special that decodes
    dst = r["dst"].cpu().numpy()
    off = r["dst_off"]
    starts = [t * TILE_BLOCKS + sum(N_SPECIAL_BLOCKS[k] for k in after if after[k] < t) for t in range(ntiles)]
    for s0 in starts:
        a = int(off[s0])
        assert np.array_equal(dst[a:a + tile_plain.size], tile_plain), "repeat at block %d" % s0
    for name in ("stored", "dependent", "bad_content_sum", "big"):
        ref, _ = O.lz4_stream_decode(sp[name][0], len(sp[name][1]) + 16)
        a = int(off[fb[name]])
        assert ref.tobytes() == sp[name][1] == dst[a:a + len(sp[name][1])].tobytes(), name
    # expected verdicts, and nothing else failed
    bad_block = fb["bad_block_sum"] + 1
    assert np.flatnonzero(r["bst"]).tolist() == [bad_block] and r["bst"][bad_block] == 1      # LA_ST_LZ4_BAD_BLOCK_SUM
    bad_frames = np.flatnonzero(r["fst"]).tolist()      # (a frame that lost a block may fail its content checksum as well)
    assert r["fst"][fr["bad_content_sum"]] == 4 and set(bad_frames) <= {fr["bad_content_sum"], fr["bad_block_sum"]}
    assert int(r["sm"]["n_bad_units"]) == 1 and int(r["sm"]["first_bad_unit"]) == bad_block
    assert int(r["sm"]["n_bad_frames"]) == len(bad_frames) and int(r["sm"]["first_bad_frame"]) == min(bad_frames)
    assert int(r["sm"]["total_out"]) == int(off[n])
    # (c) the same pieces in a batch that goes through in one slice
    s_r, s_fb, s_fr = small
    for name, cnt in N_SPECIAL_BLOCKS.items():
        a, b = fb[name], s_fb[name]
        assert np.array_equal(r["out_len"][a:a + cnt], s_r["out_len"][b:b + cnt]), name
        assert np.array_equal(r["bst"][a:a + cnt], s_r["bst"][b:b + cnt]), name
        assert r["fst"][fr[name]] == s_r["fst"][s_fr[name]], name
        assert np.array_equal(r["dst_off"][a:a + cnt + 1] - r["dst_off"][a], s_r["dst_off"][b:b + cnt + 1] - s_r["dst_off"][b]), name
    assert np.array_equal(r["out_len"][:TILE_BLOCKS], s_r["out_len"][:TILE_BLOCKS])
    return n


@pytest.fixture(scope="module")
def small(gpu_ctx, pieces):
    """31 repeats + the specials: just under the size that is sliced"""
    image, fb, fr, nb = _build(pieces, 31, {"stored": 2, "dependent": 7, "bad_block_sum": 12, "bad_content_sum": 20, "big": 28})
    assert nb < SLICED_MIN
    r = _run(gpu_ctx, image, 0)
    del r["dst"]
    return r, fb, fr


def test_sliced_batch(gpu_ctx, pieces, small):
    n = _check(gpu_ctx, pieces, 33, {"stored": 2, "dependent": 7, "bad_block_sum": 12, "bad_content_sum": 20, "big": 28}, small)
    assert (n + 63) // 64 <= WIDE_WAVES      # parsed in the wide shape


def test_sliced_batch_parsed_in_the_narrow_shape(gpu_ctx, pieces, small):
    """more waves than one round of the wide shape, not more than one round of the narrow one"""
    n = _check(gpu_ctx, pieces, 98, {"stored": 2, "dependent": 23, "bad_block_sum": 30, "bad_content_sum": 55, "big": 80}, small)
    assert WIDE_WAVES < (n + 63) // 64 <= 256 * 8
