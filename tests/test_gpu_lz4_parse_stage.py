"""GPU parity for the staged lz4 parse (la_lz4_parse.hip): how its lanes hand table entries to the sequence table
(a stage per lane, written out in groups on a fixed cadence of trips, the last incomplete group at the end) and how
they read the payload out of the LDS ring (chunks on the image's grid, row indices that wrap).

Every image is decoded with default options and with LA_LZ4_OPT_PARSE_V1 (the first-generation parse, which reads
global memory per lane and has neither stage nor ring); the two runs must agree in out_len, the sequence count and
every table entry of every block (fetched through la_gpu_lz4_debug_deps), block and frame statuses and the decoded
slab, and the outcome must be the oracle's and the bytes the generator meant.

The launcher picks the kernel's shape by the number of waves in the batch: each image goes through once as it is
and once with NARROW_PAD_FRAMES frames of tiny blocks behind it, which makes the batch large enough for the shape
the big batches get (la_launch_lz4_parse_staged)."""
import random
import struct

import numpy as np
import pytest

import oracle_lib as O
import streams as S
from test_gpu_lz4_depchains import lz4_block_from_sequences

pytestmark = pytest.mark.gpu

ST_OK, ST_BAD_BLOCK_SUM, ST_DECODE = 0, 1, 2
WIDE_WAVES = 256 * 6                    # la_lz4_parse.hip: more waves than this and the narrow shape may be chosen
PAD_BPF = 64
NARROW_PAD_FRAMES = WIDE_WAVES + 1      # 64 blocks each: one wave more than the wide shape takes in one round
TCAP = 22000                            # table entries fetched per block (a 64 KiB payload holds fewer)


def _tail(rnd, n=5):
    return rnd.randbytes(n)


def block_of(rnd, nseq, lit=(0, 6), ml=(4, 12)):
    """a block of exactly nseq table entries: nseq - 1 sequences with a match and the closing literals"""
    seqs, n = [], 0
    for k in range(nseq - 1):
        l = rnd.randbytes(rnd.randint(*lit) or (1 if n == 0 else 0))
        n += len(l)
        seqs.append((l, rnd.randint(1, n), rnd.randint(*ml)))
        n += seqs[-1][2]
    return lz4_block_from_sequences(seqs, _tail(rnd))


def frame(blocks, flg=0x74):
    """blocks: (encoded, decoded[, dict(stored=, bad_sum=)]); block checksums and content checksum on"""
    return S.lz4_frame([(b[1], S.lz4_block(b[0], bsum=True, **(b[2] if len(b) > 2 else {}))) for b in blocks], flg=flg)


_pad = None


def pad_frames():
    """NARROW_PAD_FRAMES frames of 64 literal-only blocks of 13 payload bytes -> (image bytes, decoded bytes)"""
    global _pad
    if _pad is None:
        lit = bytes(range(65, 77))
        img, plain = S.lz4_frame([(lit, S.lz4_block(bytes([0xC0]) + lit, bsum=True))] * PAD_BPF, flg=0x74)
        _pad = (img * NARROW_PAD_FRAMES, plain * NARROW_PAD_FRAMES)
    return _pad


def _run(ctx, img, opt, nb_tables):
    from libarchive_amd.lz4 import decode_image
    out, rc, msg, plan = decode_image(ctx, img, options=opt)
    out_len, dst_off, bst, fst = [a.copy() for a in plan.arrays()]
    tabs = [ctx.lz4_debug_deps(plan.batch, b, cap=TCAP)[0].copy() for b in range(min(nb_tables, plan.n_blocks))]
    slab = plan.d_dst[:int(dst_off[-1])].cpu().numpy()
    return dict(out=out.tobytes(), rc=rc, msg=msg, out_len=out_len, dst_off=dst_off, bst=bst, fst=fst, tabs=tabs, slab=slab)


def _same(a, b):
    for k in ("out_len", "dst_off", "bst", "fst", "slab"):
        assert np.array_equal(a[k], b[k]), k
    assert (a["out"], a["rc"], a["msg"]) == (b["out"], b["rc"], b["msg"])
    assert [len(t) for t in a["tabs"]] == [len(t) for t in b["tabs"]], "sequence counts"
    for i, (x, y) in enumerate(zip(a["tabs"], b["tabs"])):
        assert np.array_equal(x, y), ("table entries of block", i)


def parity(ctx, img, nblocks, cap=1 << 23):
    """both parse generations on `img` as it is and with the pad behind it, against each other and the oracle;
    returns the default run on the bare image"""
    from libarchive_amd import _native as N
    ref, res = O.lz4_stream_decode(img, cap)
    r = _run(ctx, img, 0, nblocks)
    _same(r, _run(ctx, img, N.LA_LZ4_OPT_PARSE_V1, nblocks))
    assert (r["out"], r["rc"], r["msg"]) == (ref.tobytes(), res.rc, res.errmsg.decode())
    pimg, pplain = pad_frames()
    big = _run(ctx, img + pimg, 0, nblocks)
    assert len(big["out_len"]) == nblocks + PAD_BPF * NARROW_PAD_FRAMES > WIDE_WAVES * 64
    _same(big, _run(ctx, img + pimg, N.LA_LZ4_OPT_PARSE_V1, nblocks))
    # the blocks of `img` come out of the large batch as they came out of the small one
    assert np.array_equal(big["out_len"][:nblocks], r["out_len"]) and np.array_equal(big["bst"][:nblocks], r["bst"])
    assert [t.tolist() for t in big["tabs"]] == [t.tolist() for t in r["tabs"]]
    assert np.array_equal(big["slab"][:r["slab"].size], r["slab"])
    if r["rc"] == 0 and not r["bst"].any():
        assert big["out"] == r["out"] + pplain and big["rc"] == 0
    return r


def check_good(ctx, blocks, nseq=None):
    """one frame of blocks that all decode: bytes are the generator's, sequence counts as given"""
    img, plain = frame(blocks)
    r = parity(ctx, img, len(blocks))
    assert (r["rc"], r["msg"]) == (0, "") and r["out"] == plain and not r["bst"].any() and not r["fst"].any()
    if nseq is not None:
        assert [len(t) for t in r["tabs"]] == list(nseq)
    return r


# ---------------------------------------------------------------- sequence counts around the stage

def test_sequence_counts_around_group_and_stage(gpu_ctx):
    """1 .. 33 entries: around the group of four, the stage of eight, two flush cadences, the wide shape's sixteen"""
    rnd = random.Random(0x5701)
    counts = (1, 3, 4, 5, 7, 8, 9, 12, 15, 16, 17, 33)
    check_good(gpu_ctx, [block_of(rnd, n) for n in counts], counts)


def test_wave_of_counts_1_to_64(gpu_ctx):
    """every lane reaches its flush points on other trips"""
    rnd = random.Random(0x5702)
    check_good(gpu_ctx, [block_of(rnd, n) for n in range(1, 65)], range(1, 65))


def test_wave_with_idle_lanes(gpu_ctx):
    rnd = random.Random(0x5703)
    counts = [rnd.randint(1, 40) for _ in range(37)]
    check_good(gpu_ctx, [block_of(rnd, n) for n in counts], counts)


def test_unequal_progress(gpu_ctx):
    """one block of four-byte sequences only (32 trips per 128 payload bytes) between blocks of long literal runs:
    lanes far apart in the ring, and lanes held over many trips"""
    rnd = random.Random(0x5704)
    dense = lz4_block_from_sequences([(rnd.randbytes(1), 1 + (k % 3 if k else 0), 4) for k in range(1000)], _tail(rnd))
    assert len(dense[0]) == 4 * 1000 + 6

    def runs():
        seqs, n = [], 0
        for ll in (1300, 1290, 1310):
            n += ll
            seqs.append((rnd.randbytes(ll), rnd.randint(1, n), 5))
            n += 5
        return lz4_block_from_sequences(seqs, _tail(rnd))

    blocks = [runs() for _ in range(64)]
    blocks[17] = dense
    r = check_good(gpu_ctx, blocks)
    assert len(r["tabs"][17]) == 1001 and len(r["tabs"][16]) == 4


# ---------------------------------------------------------------- the ring

def _lead_for(sk):
    """payload bytes of a stored first block that puts the second block's payload at image offset = sk (mod 128):
    magic 4 + descriptor 3 + size word 4 + payload + checksum 4 + size word 4"""
    n = (sk - 19) % 128
    return n if n else 128


def aligned_block(rnd, sk, kind, span=1152):
    """a block whose payload, staged at sk, puts one feature on every 64-byte grid point B up to `span` (every chunk
    boundary of both round sizes, every wrap of a 256-byte ring): kind 'token' -- a token on byte B - 1; 'offset' --
    an offset's two bytes on B - 1 and B; 'litext' / 'matchext' -- a length-extension byte on B"""
    seqs, out = [(b"ab", 1, 300)], 302
    pos = 7                                     # payload position behind the sequences so far
    hits = 0

    def push(lit, off, mlen):
        nonlocal pos, out
        ll, ml = len(lit), mlen - 4
        pos += 1 + (1 if ll >= 15 else 0) + ll + 2 + (1 if ml >= 15 else 0)
        assert ll < 270 and ml < 270
        out += ll + mlen
        seqs.append((lit, off, mlen))

    for B in range(64, span + 1, 64):
        T = B - sk                              # payload position of grid point B
        ll = rnd.randint(0, 9) if kind != "litext" else rnd.randint(15, 40)
        mlen = rnd.randint(4, 18) if kind != "matchext" else rnd.randint(19, 60)
        start = {"token": T - 1, "offset": T - 2 - ll, "litext": T - 1, "matchext": T - 3 - ll}[kind]
        gap = start - pos
        if gap != 0 and gap < 3:
            continue
        while gap > 17:
            push(rnd.randbytes(5), rnd.randint(1, out), 4)
            gap -= 8
        if gap:
            push(rnd.randbytes(gap - 3), rnd.randint(1, out), 4)
        assert pos == start
        off = rnd.randint(257, out) | 1
        push(rnd.randbytes(ll), off if off <= out + ll else 257, mlen)
        hits += 1
    assert hits >= span // 64 - 2
    return lz4_block_from_sequences(seqs, _tail(rnd))


@pytest.mark.parametrize("sk", [0, 1, 63, 64, 127])
def test_features_on_every_chunk_boundary_and_ring_wrap(gpu_ctx, sk):
    rnd = random.Random(0x5710 + sk)
    lead = rnd.randbytes(_lead_for(sk))
    blocks = [(lead, lead, dict(stored=True))]
    blocks += [aligned_block(rnd, sk, kind) for kind in ("token", "offset", "litext", "matchext")]
    img, plain = frame(blocks)
    assert (img.index(blocks[1][0]) - sk) % 128 == 0
    r = parity(gpu_ctx, img, len(blocks))
    assert (r["rc"], r["msg"]) == (0, "") and r["out"] == plain and len(r["tabs"][0]) == 0


def test_literal_runs_longer_than_the_ring(gpu_ctx):
    """300 and 1 000 literal bytes in front of a match: the offset is not staged while the token's chunk is current"""
    rnd = random.Random(0x5720)
    blocks = []
    for ll in (300, 1000):
        for first in (0, 3):                # as the block's first sequence and behind short ones
            seqs, n = [], 0
            for k in range(first):
                seqs.append((rnd.randbytes(2), 1, 4))
                n += 6
            seqs.append((rnd.randbytes(ll), rnd.randint(1, n + ll), 9))
            seqs.append((rnd.randbytes(3), 7, 4))
            blocks.append(lz4_block_from_sequences(seqs, _tail(rnd)))
    neighbours = [block_of(rnd, rnd.randint(2, 30)) for _ in range(20)]
    check_good(gpu_ctx, neighbours[:10] + blocks + neighbours[10:])


def test_block_ends_on_a_chunk_boundary_and_a_13_byte_payload(gpu_ctx):
    rnd = random.Random(0x5721)
    tiny = lz4_block_from_sequences([(b"abcd", 1, 8)], _tail(rnd))
    assert len(tiny[0]) == 13
    lead = rnd.randbytes(_lead_for(0))
    seqs, n, size = [], 0, 0
    for k in range(39):
        seqs.append((rnd.randbytes(3), rnd.randint(1, n + 3), 6))
        n += 9
        size += 6
    on_grid = lz4_block_from_sequences(seqs, _tail(rnd, 256 - size - 2))      # token, one extension byte, 20 literals
    assert len(on_grid[0]) == 256
    blocks = [(lead, lead, dict(stored=True)), on_grid, tiny, block_of(rnd, 9)]
    img, plain = frame(blocks)
    assert img.index(on_grid[0]) % 128 == 0
    r = parity(gpu_ctx, img, len(blocks))
    assert (r["rc"], r["msg"]) == (0, "") and r["out"] == plain and [len(t) for t in r["tabs"]] == [0, 40, 2, 9]


# ---------------------------------------------------------------- table edges

def test_dense_tables_and_complete_last_groups(gpu_ctx):
    """blocks of three-byte sequences only (no literals: the most entries a payload can hold, the slot as full as it
    gets) with counts on both sides of a multiple of 8, so that the last group is complete, one short or one over"""
    rnd = random.Random(0x5730)
    blocks, counts = [], (8, 15, 16, 17, 24, 32, 40, 63, 64, 65, 4096)
    for n in counts:
        seqs = [(b"xyzw", 2, 4)] + [(b"", rnd.randint(1, 8), 4) for _ in range(n - 2)]
        blocks.append(lz4_block_from_sequences(seqs, _tail(rnd)))
        assert len(blocks[-1][0]) == 7 + 3 * (n - 2) + 6
    check_good(gpu_ctx, blocks, counts)


def _run_rows(ctx, img, rows, options, sample):
    """decodes `img` through a hand-built block table: row i of the table is block rows[i] of the image's own index
    (no frames); -> out_len, block status, slab, {row: table entries} for the rows in `sample`"""
    import torch
    from libarchive_amd import _native as N
    from libarchive_amd.lz4 import Lz4DevicePlan
    image = np.frombuffer(img, dtype=np.uint8)
    idx = N.lz4_index(image, at_eof=True)
    blocks = idx.blocks[np.asarray(rows)].copy()
    cap = int(blocks["dst_cap"].astype(np.uint64).sum())
    hand = N.Lz4Index(blocks, idx.frames[:0].copy(), idx.end_kind, idx.consumed, cap)
    plan = Lz4DevicePlan(ctx, torch.from_numpy(image.copy()).to("cuda:0"), hand)
    plan.run(options)
    out_len, dst_off, bst, _ = [a.copy() for a in plan.arrays()]
    tabs = {i: ctx.lz4_debug_deps(plan.batch, i, cap=TCAP)[0].copy() for i in sample}
    return out_len, bst, plan.d_dst[:int(dst_off[-1])].cpu().numpy(), tabs


@pytest.mark.parametrize("shape", ["wide", "narrow"])
def test_table_cap_cuts_off_the_last_blocks(gpu_ctx, shape):
    """The workspace's table holds src_bytes / 3 + 8 n entries, which bounds the slots only of blocks that do not
    share payload bytes.  A table whose rows name the same eight blocks over and over runs out of slots: the rows
    that still fit are parsed into the table as ever, every row behind them is eligible without a slot, reports
    0xFFFFFFFF sequences (la_gpu_lz4_debug_deps answers 0 for it: no table) and is decoded by the general kernel.  Both
    parse generations must draw the line at the same row and decode every row."""
    from libarchive_amd import _native as N
    rnd = random.Random(0x5732)
    counts = (2, 5, 9, 17, 33, 12, 4, 8)
    blocks = [block_of(rnd, n, lit=(2, 6)) for n in counts]
    img, _ = frame(blocks)
    n = 64 * 3 if shape == "wide" else 64 * (WIDE_WAVES + 1)
    rows = [i % 8 for i in range(n)]
    sample = sorted(set(list(range(24)) + list(range(n - 24, n)) + list(range(0, n, max(1, n // 160)))))
    out_len, bst, slab, tabs = _run_rows(gpu_ctx, img, rows, 0, sample)
    v_len, v_bst, v_slab, v_tabs = _run_rows(gpu_ctx, img, rows, N.LA_LZ4_OPT_PARSE_V1, sample)
    # every row decodes, whichever kernel expands it: the bytes are the generator's (= the oracle's, see check_good)
    ref, res = O.lz4_stream_decode(img, 1 << 20)
    plain = b"".join(b[1] for b in blocks)
    assert res.rc == 0 and ref.tobytes() == plain
    assert not bst.any() and not v_bst.any()
    assert out_len.tolist() == [len(blocks[r][1]) for r in rows] == v_len.tolist()
    assert slab.tobytes() == plain * (n // 8) and np.array_equal(slab, v_slab)
    # rows with a slot have their sequences in the table, rows without report none; the line is one row, the same in both
    fits = [len(tabs[i]) > 0 for i in sample]
    assert fits[0] and not fits[-1], "the first row has a slot, the last has none"
    cut = fits.index(False)
    assert not any(fits[cut:]), "no row behind the first one without a slot has one"
    assert [len(v_tabs[i]) > 0 for i in sample] == fits
    for i in sample[:cut]:
        assert len(tabs[i]) == counts[rows[i]] and np.array_equal(tabs[i], v_tabs[i]), i
    # the rows that fit are parsed as the same blocks are in a table of their own
    own = _run(gpu_ctx, img, 0, 8)
    for i in sample[:cut]:
        assert np.array_equal(tabs[i], own["tabs"][rows[i]]), i


def test_stored_and_failing_blocks_between_parsed_ones(gpu_ctx):
    """a stored block and a block whose payload fails take no table entries and leave their neighbours' alone"""
    rnd = random.Random(0x5731)
    raw = rnd.randbytes(333)
    bad = bytes([0x10]) + b"A" + b"\x00\x00" + bytes([0x50]) + b"12345"      # offset 0
    blocks = [block_of(rnd, 9), (raw, raw, dict(stored=True)), block_of(rnd, 12), (bad, b""), block_of(rnd, 5)]
    img, _ = frame(blocks)
    r = parity(gpu_ctx, img, len(blocks))
    assert (r["rc"], r["msg"]) == (-30, "lz4 decompression failed")
    assert r["out"] == blocks[0][1] + raw + blocks[2][1]
    assert r["bst"].tolist() == [ST_OK, ST_OK, ST_OK, ST_DECODE, ST_OK]
    assert [len(t) for t in r["tabs"]] == [9, 0, 12, 0, 5]
    assert r["out_len"].tolist() == [len(blocks[0][1]), 333, len(blocks[2][1]), 0, len(blocks[4][1])]


# ---------------------------------------------------------------- checksums

@pytest.mark.parametrize("where", ["first_lane", "last_lane", "short_block"])
def test_wrong_block_checksum(gpu_ctx, where):
    """LA_ST_LZ4_BAD_BLOCK_SUM, also where the payload would fail to decode as well: the checksum is looked at first"""
    rnd = random.Random(0x5740)
    blocks = [block_of(rnd, rnd.randint(2, 20)) for _ in range(64)]
    lane = {"first_lane": 0, "last_lane": 63, "short_block": 31}[where]
    if where == "short_block":
        enc = bytes([0x10]) + b"A" + b"\x00\x00" + bytes([0x50]) + b"12345"      # 10 bytes, offset 0 on top
        assert len(enc) < 16
        blocks[lane] = (enc, b"", dict(bad_sum=True))
    else:
        blocks[lane] = blocks[lane] + (dict(bad_sum=True),)
    img, _ = frame(blocks)
    r = parity(gpu_ctx, img, 64)
    assert (r["rc"], r["msg"]) == (-30, "malformed lz4 data")
    assert r["out"] == b"".join(b[1] for b in blocks[:lane])
    want = [ST_OK] * 64
    want[lane] = ST_BAD_BLOCK_SUM
    assert r["bst"].tolist() == want
    good = [i for i in range(64) if i != lane]
    assert all(r["out_len"][i] == len(blocks[i][1]) for i in good)


# ---------------------------------------------------------------- a corrupt chain among valid neighbours

@pytest.mark.parametrize("fault", ["offset_zero", "offset_beyond_output"])
def test_corrupt_chain_in_one_lane(gpu_ctx, fault):
    rnd = random.Random(0x5750)
    blocks = [block_of(rnd, rnd.randint(2, 40)) for _ in range(64)]
    seqs, n = [], 0
    for k in range(21):
        seqs.append((rnd.randbytes(2), rnd.randint(1, n + 2), 5))
        n += 7
    enc = bytearray(lz4_block_from_sequences(seqs, _tail(rnd))[0])
    at = 5 * 13 + 3                         # the offset of the fourteenth sequence (each takes 5 payload bytes)
    assert enc[at - 3] == 0x21
    enc[at:at + 2] = struct.pack("<H", 0 if fault == "offset_zero" else 13 * 7 + 2 + 1)
    blocks[29] = (bytes(enc), b"")
    img, _ = frame(blocks)
    r = parity(gpu_ctx, img, 64)
    assert (r["rc"], r["msg"]) == (-30, "lz4 decompression failed")
    assert r["bst"].tolist() == [ST_DECODE if i == 29 else ST_OK for i in range(64)]
    assert r["out_len"].tolist() == [0 if i == 29 else len(blocks[i][1]) for i in range(64)]
    assert r["slab"].tobytes() == b"".join(b[1] for b in blocks)
    assert len(r["tabs"][29]) == 0 and len(r["tabs"][28]) > 0 and len(r["tabs"][30]) > 0


# ---------------------------------------------------------------- a seeded sweep

def test_sweep_of_generated_blocks(gpu_ctx):
    """200 blocks of 1 to 64 KiB from the generator, five frame layouts behind each other"""
    layouts = ((6, 7, 1024), (2, 16, 65536), (10, 5, 20000), (36, 1, 4097), (5, 8, 8192))     # frames, blocks each, size
    parts, plains, nb = [], [], 0
    for k, (nf, bpf, bs) in enumerate(layouts):
        img, plain = S.synth_lz4_stream(0x57600 + k, 0, nf, blocks_per_frame=bpf, block_size=bs, nthreads=2)
        parts.append(img.tobytes())
        plains.append(plain.tobytes())
        nb += nf * bpf
    assert nb == 200
    img, plain = b"".join(parts), b"".join(plains)
    r = parity(gpu_ctx, img, nb, cap=len(plain) + 16)
    assert (r["rc"], r["msg"]) == (0, "") and r["out"] == plain and not r["bst"].any() and not r["fst"].any()
    assert all(len(t) > 0 for t in r["tabs"])
