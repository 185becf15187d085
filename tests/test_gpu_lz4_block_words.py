"""GPU parity for the block words of the lz4 expand step.  The window kernel, the in-order kernel and the general
kernel open with one fetch of everything they know about a block -- the words of its table row, its
status, decoded length, sequence count, slab offset and table offset (la_lz4_load_block_words, la_dev.h) -- and ask
la_lz4_route with what came back.  The fetch is unconditional: it reads every array for every block below n, whatever
state the block is in, where the kernels used to read a word only when the routing test got that far.  The cases here
are the ones where that could read or route wrongly: batches of one and two blocks, every route side by side with each
kind of block as the batch's first and last, rows without a table slot (sequence count 0xFFFFFFFF), a slab that ends in
front of the last block, an empty batch, and gzip members through the deflate front end, whose job carries no
dependency words.

Every image is decoded four ways -- default options, LA_LZ4_OPT_SEARCH_IN_EXPAND, LA_LZ4_OPT_EXPAND_INORDER and
LA_LZ4_OPT_GENERAL_ONLY -- and each is compared with the oracle (bytes, return code, message) and, block by block, with
the bytes the generator meant: a block behind a failing one is in the slab although the stream ended in front of it.
For the window blocks the dependency words and the literal plans are fetched and compared with the rules restated in
test_gpu_lz4_deps.py and lz4_literal_plan_rule.py."""
import functools
import random
import zlib

import numpy as np
import pytest

import lz4_literal_plan_rule as R
import oracle_lib as O
import streams as S
from test_gpu_gzip import ST_OK as GZ_OK, gpu_inflate, trailer
from test_gpu_lz4_depchains import lz4_block_from_sequences
from test_gpu_lz4_deps import _random_block, rule_words
from test_gpu_lz4_parse_stage import block_of

pytestmark = pytest.mark.gpu

ST_OK, ST_DECODE = 0, 2
GUARD = 0xA5
KINDS = ("stored", "bad_offset_zero", "bad_offset_far", "window", "segmented", "general", "full", "dependent")


def _options():
    from libarchive_amd import _native as N
    return (0, N.LA_LZ4_OPT_SEARCH_IN_EXPAND, N.LA_LZ4_OPT_EXPAND_INORDER, N.LA_LZ4_OPT_GENERAL_ONLY)


# ---------------------------------------------------------------- blocks by kind

class Blk:
    """one row of the batch: payload, the bytes it decodes to (b"" when the parse fails it), how it is framed and which
    route it takes"""

    def __init__(self, kind, enc, plain, stored=False, fails=False, window=False):
        self.kind, self.enc, self.plain, self.stored, self.fails, self.window = kind, enc, plain, stored, fails, window


@functools.lru_cache(maxsize=None)
def _block(kind, seed):
    rnd = random.Random(0xB10C00 + seed)
    if kind == "stored":
        raw = rnd.randbytes(rnd.randint(1, 700))
        return Blk(kind, raw, raw, stored=True)
    if kind == "bad_offset_zero":
        return Blk(kind, bytes([0x10]) + b"A" + b"\x00\x00" + bytes([0x50]) + b"12345", b"", fails=True)
    if kind == "bad_offset_far":    # offset 9 with one byte of output
        return Blk(kind, bytes([0x1f]) + b"a" + b"\x09\x00" + b"\x0a" + b"\x50" + b"bcdef", b"", fails=True)
    if kind == "window":
        return Blk(kind, *_random_block(rnd, rnd.randint(40, 2500)), window=True)
    if kind == "segmented":         # 4 097 sequences: one more than an LDS segment holds
        seqs, n = [], 0
        for k in range(4096):
            lit = rnd.randbytes(rnd.randint(1, 2))
            n += len(lit)
            seqs.append((lit, rnd.randint(1, min(n, 3000)), rnd.randint(4, 8)))
            n += seqs[-1][2]
        return Blk(kind, *lz4_block_from_sequences(seqs, rnd.randbytes(5)))
    if kind == "general":           # few long sequences: 512 decoded bytes per sequence and more
        return Blk(kind, *lz4_block_from_sequences([(rnd.randbytes(2), 2, 4000), (rnd.randbytes(3), 1000, 1500)], rnd.randbytes(5)))
    if kind == "full":              # exactly 65 536 bytes: the 16-bit end position reads 0
        seqs, n = [], 0
        for k in range(2000):
            n += 4
            seqs.append((rnd.randbytes(4), rnd.randint(1, n), 28))
            n += 28
        enc, plain = lz4_block_from_sequences(seqs, rnd.randbytes(65536 - n))
        assert len(plain) == 65536
        return Blk(kind, enc, plain, window=True)
    raise KeyError(kind)


def _frame_of(blks):
    """one frame of independent blocks, block and content checksums on -> (image, rows)"""
    img, _ = S.lz4_frame([(b.plain, S.lz4_block(b.enc, stored=b.stored, bsum=True)) for b in blks], flg=0x74)
    return img, list(blks)


@functools.lru_cache(maxsize=None)
def _dependent_frame(seed):
    """a frame of four blocks that read the block before them (general kernel, one wave per chain) -> (image, rows)"""
    rnd = random.Random(0xDE9000 + seed)
    chunks = [rnd.randbytes(rnd.randint(40, 300)) * 3 for _ in range(4)]
    img, plain = S.lz4_dependent_frame(chunks)
    ref, res = O.lz4_stream_decode(img, len(plain) + 16)
    assert res.rc == 0 and ref.tobytes() == plain
    idx_plain, rows, prev = [], [], b""
    for i, c in enumerate(chunks):     # (what lz4_dependent_frame makes of each chunk)
        p = c if i == 0 or len(prev) < 8 else prev[:8] + c
        rows.append(Blk("dependent", b"", p))
        prev = p
    assert b"".join(r.plain for r in rows) == plain
    return img, rows


def _unit(kind, seed):
    """a frame that holds one block of `kind` (four for a dependent chain)"""
    return _dependent_frame(seed) if kind == "dependent" else _frame_of([_block(kind, seed)])


@functools.lru_cache(maxsize=None)
def _middle():
    """about 70 rows, every route side by side: frames of mixed independent blocks and two dependent chains"""
    units, seed = [], 100
    for rep in range(6):
        blks = []
        for kind in ("window", "stored", "bad_offset_zero", "window", "general", "window", "bad_offset_far", "stored", "window"):
            blks.append(_block(kind, seed))
            seed += 1
        if rep in (1, 4):
            blks.insert(3, _block("segmented", seed))
            blks.insert(6, _block("full", seed + 1))
            seed += 2
        units.append(_frame_of(blks))
        if rep in (2, 3):
            units.append(_dependent_frame(seed))
            seed += 1
    return units


def _batch(units):
    img = b"".join(u[0] for u in units)
    rows = [r for u in units for r in u[1]]
    return img, rows


# ---------------------------------------------------------------- decoding and checking

def _decode(ctx, img, opt):
    from libarchive_amd.lz4 import decode_image
    out, rc, msg, plan = decode_image(ctx, img, options=opt)
    out_len, dst_off, bst, fst = [a.copy() for a in plan.arrays()]
    slab = plan.d_dst[:int(dst_off[-1])].cpu().numpy().tobytes()
    return (out.tobytes(), rc, msg), out_len, dst_off, bst, slab, plan


def _check_words(ctx, plan, rows):
    """dependency words and literal plan of every window row against the rules"""
    for i, r in enumerate(rows):
        if not r.window:
            continue
        seq, deps = ctx.lz4_debug_deps(plan.batch, i, cap=4096)
        assert len(seq) > 0, i
        got, want = [int(w) for w in deps], rule_words(seq, len(r.plain))
        assert got == want, (i, r.kind, [(k, hex(g), hex(w)) for k, (g, w) in enumerate(zip(got, want)) if g != w][:8])
        lp = [int(x) for x in ctx.lz4_debug_literal_plan(plan.batch, i)]
        assert lp == R.rule_plan(seq, len(r.enc)), (i, r.kind)


def check_batch(ctx, units):
    """the batch four ways: each against the oracle and, row by row, against the generator; the words of the default run"""
    img, rows = _batch(units)
    ref, res = O.lz4_stream_decode(img, sum(len(r.plain) for r in rows) + 16)
    want = (ref.tobytes(), res.rc, res.errmsg.decode())
    first_bad = next((i for i, r in enumerate(rows) if r.fails), len(rows))
    assert want[0] == b"".join(r.plain for r in rows[:first_bad]), "the generator and the oracle disagree"
    assert want[1] == (0 if first_bad == len(rows) else -30)
    for opt in _options():
        got, out_len, dst_off, bst, slab, plan = _decode(ctx, img, opt)
        assert got == want, opt
        assert len(out_len) == len(rows)
        assert bst.tolist() == [ST_DECODE if r.fails else ST_OK for r in rows], opt
        assert out_len.tolist() == [len(r.plain) for r in rows], opt
        assert slab == b"".join(r.plain for r in rows), opt     # also the rows behind a failing one
        if opt == 0:
            _check_words(ctx, plan, rows)


# ---------------------------------------------------------------- the cases

@pytest.mark.parametrize("count", [1, 2])
def test_batch_of_one_and_of_two_window_blocks(gpu_ctx, count):
    check_batch(gpu_ctx, [_frame_of([_block("window", 10 + k) for k in range(count)])])


@pytest.mark.parametrize("kind", KINDS)
def test_every_route_side_by_side(gpu_ctx, kind):
    """about 70 rows of every kind, and one more of `kind` as the batch's first row and as its last"""
    units = [_unit(kind, 1)] + list(_middle()) + [_unit(kind, 2)]
    img, rows = _batch(units)
    assert 60 <= len(rows) <= 90 and rows[0].kind == rows[-1].kind == kind
    assert {r.kind for r in rows} == set(KINDS)
    check_batch(gpu_ctx, units)


def _run_rows(ctx, img, rows, options, slab_cap=None):
    """`img` through a hand-built block table: row i is block rows[i] of the image's own index, no frames.  slab_cap:
    the batch names a slab that ends there; the buffer behind it is longer and filled with GUARD.
    -> out_len, dst_off, block status, the whole buffer, the plan"""
    import torch
    from libarchive_amd import _native as N
    from libarchive_amd.lz4 import Lz4DevicePlan
    image = np.frombuffer(img, dtype=np.uint8)
    idx = N.lz4_index(image, at_eof=True)
    blocks = idx.blocks[np.asarray(rows)].copy()
    cap = int(blocks["dst_cap"].astype(np.uint64).sum())
    hand = N.Lz4Index(blocks, idx.frames[:0].copy(), idx.end_kind, idx.consumed, cap)
    plan = Lz4DevicePlan(ctx, torch.from_numpy(image.copy()).to("cuda:0"), hand)
    plan.d_dst.fill_(GUARD)
    if slab_cap is not None:
        assert slab_cap <= plan.dst_cap
        plan.batch.dst_cap = slab_cap
    plan.run(options)
    out_len, dst_off, bst, _ = [a.copy() for a in plan.arrays()]
    return out_len, dst_off, bst, plan.d_dst.cpu().numpy(), plan


def test_rows_without_a_table_slot(gpu_ctx):
    """A table whose rows name the same eight blocks over and over runs out of slots (tests/test_gpu_lz4_parse_stage.py):
    the rows behind the cut report 0xFFFFFFFF sequences and go to the general kernel.  Every kernel fetches their words
    like any other row's and must leave them to it; every row decodes, and the rows in front of the cut have the
    rules' words and plans."""
    rnd = random.Random(0xB10C01)
    counts = (2, 5, 9, 17, 33, 12, 4, 8)
    blocks = [block_of(rnd, n, lit=(2, 6)) for n in counts]
    img, plain = S.lz4_frame([(p, S.lz4_block(e, bsum=True)) for e, p in blocks], flg=0x74)
    ref, res = O.lz4_stream_decode(img, 1 << 20)
    assert res.rc == 0 and ref.tobytes() == plain
    n = 64 * 3
    rows = [i % 8 for i in range(n)]
    for opt in _options():
        out_len, dst_off, bst, buf, plan = _run_rows(gpu_ctx, img, rows, opt)
        assert not bst.any(), opt
        assert out_len.tolist() == [len(blocks[r][1]) for r in rows], opt
        assert buf[:int(dst_off[-1])].tobytes() == plain * (n // 8), opt
        if opt == 0:
            fits = [len(gpu_ctx.lz4_debug_deps(plan.batch, i, cap=64)[0]) > 0 for i in range(n)]
            assert fits[0] and not fits[-1], "the first row has a slot, the last has none"
            cut = fits.index(False)
            assert not any(fits[cut:])
            for i in list(range(min(cut, 16))) + list(range(max(cut - 8, 0), cut)):
                seq, deps = gpu_ctx.lz4_debug_deps(plan.batch, i, cap=64)
                assert [int(w) for w in deps] == rule_words(seq, len(blocks[rows[i]][1])), i
                lp = [int(x) for x in gpu_ctx.lz4_debug_literal_plan(plan.batch, i)]
                assert lp == R.rule_plan(seq, len(blocks[rows[i]][0])), i
            for i in (cut, n - 1):
                assert len(gpu_ctx.lz4_debug_literal_plan(plan.batch, i)) == 0, i


@pytest.mark.parametrize("last", ["window", "general", "stored"])
def test_slab_ends_in_front_of_the_last_block(gpu_ctx, last):
    """the batch's slab is one byte too short for its last row: nobody writes that row (la_lz4_route: never past the
    slab, whatever the tables say), every row in front of it decodes, and no byte from the row's offset on changes"""
    blks = [_block("window", 30), _block("stored", 31), _block("general", 32), _block("window", 33), _block(last, 34)]
    img, _ = _frame_of(blks)
    total = sum(len(b.plain) for b in blks)
    for opt in _options():
        out_len, dst_off, bst, buf, plan = _run_rows(gpu_ctx, img, list(range(len(blks))), opt, slab_cap=total - 1)
        assert out_len.tolist() == [len(b.plain) for b in blks], opt
        assert int(dst_off[-1]) == total and int(dst_off[-2]) == total - len(blks[-1].plain)
        assert buf[:int(dst_off[-2])].tobytes() == b"".join(b.plain for b in blks[:-1]), opt
        assert (buf[int(dst_off[-2]):] == GUARD).all(), opt


def test_empty_batches(gpu_ctx):
    """no image at all, and a frame without blocks"""
    for img in (b"", S.lz4_frame([], flg=0x64)[0]):
        ref, res = O.lz4_stream_decode(img, 64)
        for opt in _options():
            got, out_len, dst_off, bst, slab, plan = _decode(gpu_ctx, img, opt)
            assert got == (ref.tobytes(), res.rc, res.errmsg.decode()) and got[0] == b"", opt
            assert len(out_len) == 0 and slab == b""


def test_gzip_members_through_the_deflate_front_end(gpu_ctx):
    """a few small members by every inflate path, the two-phase ones (entropy decode, then the window kernel or the
    in-order kernel over the front end's tables, without dependency words) among them, against zlib"""
    rnd = random.Random(0xB10C02)
    words = [rnd.randbytes(rnd.randint(1, 12)) for _ in range(40)]
    datas = []
    for n in (1, 7, 100, 3000, 20000, 65536, 40000, 5):
        datas.append(b"".join(rnd.choice(words) for _ in range(n // 5 + 1))[:n])
    bodies = []
    for d in datas:
        co = zlib.compressobj(6, zlib.DEFLATED, -15)
        bodies.append(co.compress(d) + co.flush() + trailer(d))
    res, sm = gpu_inflate(gpu_ctx, bodies, [len(d) for d in datas])
    for (st, out, cons, crc), d, b in zip(res, datas, bodies):
        assert zlib.decompress(b[:-8], -15) == d
        assert (st, out, crc) == (GZ_OK, d, zlib.crc32(d) & 0xFFFFFFFF)
    assert int(sm["n_bad_units"]) == 0 and int(sm["total_out"]) == sum(len(d) for d in datas)
