"""GPU parity for the split last expand slice of the lz4 decode (la_lz4_slices.h, la_gpu_lz4_decode): the slice's blocks
are launched by their position in the frame, and the frames' content checksums advance between the launches through a
carry per frame, so that the step waits only for the chain over each frame's last few blocks.

Every image is decoded three times on one plan, the outputs overwritten in between: with LA_LZ4_OPT_SPLIT_SMALL (the
whole batch is the split slice), without it (a batch below 32 768 blocks takes the contiguous sequence, one at size
splits its last quarter), and with LA_LZ4_OPT_SEARCH_IN_EXPAND (always the contiguous sequence).  The three runs must
agree in out_len, dst_off, block status, frame status, summary and every byte of the slab, and with what the generator
meant: decoded lengths, statuses, bytes, and the outcome of the oracle.  Which sequence a run took is read from the
profile ranges: only the split one has lz4_frame_sums_tail."""
import random
import struct

import numpy as np
import pytest

import oracle_lib as O
import streams as S
from test_gpu_lz4_depchains import lz4_block_from_sequences

pytestmark = pytest.mark.gpu

ST_OK, ST_BAD_BLOCK_SUM, ST_DECODE, ST_BAD_HEADER, ST_BAD_CONTENT = 0, 1, 2, 3, 4
FILL = 0xA5
BAD_BLOCK = bytes([0x10]) + b"A" + b"\x00\x00" + bytes([0x50]) + b"12345"      # offset 0: fails in the parse


@pytest.fixture(scope="module")
def ctx(gpu_ctx):
    gpu_ctx.profile_enable(True)
    yield gpu_ctx
    gpu_ctx.profile_enable(False)


# ---------------------------------------------------------------- blocks and frames

def tiny(rnd, size):
    """a window block that decodes to exactly `size` bytes -> (encoded, decoded)"""
    if size < 13 or rnd.random() < 0.25:
        return lz4_block_from_sequences([], rnd.randbytes(size))
    lit = rnd.randint(1, size - 9)
    mlen = rnd.randint(4, size - lit - 5)
    return lz4_block_from_sequences([(rnd.randbytes(lit), rnd.randint(1, lit), mlen)], rnd.randbytes(size - lit - mlen))


def tiny_frame(rnd, nblocks, lo=1, hi=65, **kw):
    return dict(blocks=[tiny(rnd, rnd.randint(lo, hi)) for _ in range(nblocks)], **kw)


def flipped(rnd, size=48):
    """a block with one literal byte changed behind the generator's back: still valid, other bytes than the frame's
    content checksum was made for"""
    lit = rnd.randbytes(9)
    enc, dec = lz4_block_from_sequences([(lit, 3, 20)], rnd.randbytes(size - 29))
    at = 1 + 4          # token, then the literals
    enc2 = bytearray(enc)
    enc2[at] ^= 0x40
    out = bytearray(lit)                # what the changed block decodes to, by the format's rule
    out[4] ^= 0x40
    for _ in range(20):
        out.append(out[-3])
    out += dec[29:]
    return bytes(enc2), dec, dict(actual=bytes(out))


def build(frames):
    """frames: dicts of blocks=[(encoded, decoded[, dict(stored=, bad_sum=, actual=, fail=)])], flg=, bad_content=, bad_hc=
    -> image, and what the device must report: out_len, block status, frame status, the slab's bytes"""
    img, out_len, bst, fst, slab = b"", [], [], [], b""
    for fr in frames:
        flg = fr.get("flg", 0x74)
        entries, got = [], b""
        for b in fr["blocks"]:
            kw = dict(b[2]) if len(b) > 2 else {}
            actual, fail = kw.pop("actual", b[1]), kw.pop("fail", False)
            entries.append((b[1], S.lz4_block(b[0], bsum=bool(flg & 0x10), **kw)))
            out_len.append(0 if fail else len(actual))
            bst.append(ST_DECODE if fail else ST_BAD_BLOCK_SUM if kw.get("bad_sum") else ST_OK)
            got += b"" if fail else actual
        fimg, plain = S.lz4_frame(entries, flg=flg, bad_content=fr.get("bad_content", False), bad_hc=fr.get("bad_hc", False))
        img += fimg
        slab += got
        if fr.get("bad_hc"):
            fst.append(ST_BAD_HEADER)
        elif flg & 0x04:
            stored = O.xxh32(plain) ^ (1 if fr.get("bad_content") else 0)
            fst.append(ST_OK if O.xxh32(got) == stored else ST_BAD_CONTENT)
        else:
            fst.append(ST_OK)
    return img, dict(out_len=out_len, bst=bst, fst=fst, slab=slab)


# ---------------------------------------------------------------- the three runs

def _one(ctx, plan, opt, carry_out):
    import torch
    plan.d_dst.fill_(FILL)
    plan.d_out_len.fill_(0x5A5A5A5A)
    plan.d_dst_off.fill_(-1)
    plan.d_block_status.fill_(0x5A5A5A5A)
    plan.d_frame_status.fill_(0x5A5A5A5A)
    plan.d_summary.fill_(FILL)
    if carry_out is not None:
        carry_out.fill_(FILL)
    plan.run(opt)
    out_len, dst_off, bst, fst = [a.copy() for a in plan.arrays()]
    names = [n for n, _ in ctx.profile_read()]
    delivered, rc, msg = plan.resolve()
    r = dict(out_len=out_len, dst_off=dst_off, bst=bst, fst=fst, summary=plan.d_summary.cpu().numpy().copy(),
             slab=plan.d_dst[:plan.dst_cap].cpu().numpy().copy(), outcome=(delivered, rc, msg),
             split="lz4_frame_sums_tail" in names, names=names)
    if carry_out is not None:
        r["carry_out"] = carry_out.cpu().numpy().copy()
    torch.cuda.synchronize()
    return r


def three_runs(ctx, img, want=None, split=True, dst_cap=None, edit=None, carry_in=None, oracle=True):
    """-> the run with LA_LZ4_OPT_SPLIT_SMALL, after all three agreed with each other, with `want` and with the oracle"""
    import torch
    from libarchive_amd import _native as N
    from libarchive_amd.lz4 import Lz4DevicePlan
    image = np.frombuffer(bytes(img), dtype=np.uint8)
    idx = N.lz4_index(image, at_eof=True)
    if edit:
        edit(idx)
    plan = Lz4DevicePlan(ctx, torch.from_numpy(image.copy()).to("cuda:0"), idx, dst_cap=dst_cap)
    carry_out = None
    if carry_in is not None:
        d_in = torch.from_numpy(np.frombuffer(carry_in, dtype=np.uint8).copy()).to("cuda:0")
        carry_out = torch.zeros(64, dtype=torch.uint8, device="cuda:0")
        plan.batch.d_carry_in, plan.batch.d_carry_out = d_in.data_ptr(), carry_out.data_ptr()
    at_size = plan.n_blocks >= 4 * 8192
    runs = [_one(ctx, plan, opt, carry_out) for opt in (N.LA_LZ4_OPT_SPLIT_SMALL, 0, N.LA_LZ4_OPT_SEARCH_IN_EXPAND)]
    assert [r["split"] for r in runs] == [split, split and at_size, False], [r["names"] for r in runs]
    a = runs[0]
    for b in runs[1:]:
        for k in ("out_len", "dst_off", "bst", "fst", "summary", "slab"):
            assert np.array_equal(a[k], b[k]), k
        assert a["outcome"] == b["outcome"]
    if want is not None:
        assert a["out_len"].tolist() == want["out_len"]
        assert a["bst"].tolist() == want["bst"]
        assert a["fst"].tolist() == want["fst"]
        n = len(want["slab"])
        assert int(a["dst_off"][-1]) == n and a["slab"][:n].tobytes() == want["slab"]
        assert (a["slab"][n:] == FILL).all()
    if oracle:
        ref, res = O.lz4_stream_decode(bytes(img), plan.dst_cap + 16)
        delivered, rc, msg = a["outcome"]
        assert (a["slab"][:delivered].tobytes(), rc, msg) == (ref.tobytes(), res.rc, res.errmsg.decode())
    return a


# ---------------------------------------------------------------- frames on and off the period

def test_eight_frames_of_sixteen_blocks(ctx):
    rnd = random.Random(0x3201)
    img, want = build([tiny_frame(rnd, 16) for _ in range(8)])
    r = three_runs(ctx, img, want)
    assert r["outcome"][1:] == (0, "") and not r["fst"].any()


def test_frames_off_the_period(ctx):
    """1, 2, 3, 15, 16, 17 and 33 blocks and a frame of 41: 128 blocks in 8 frames, period 16, hardly a frame on it"""
    rnd = random.Random(0x3202)
    img, want = build([tiny_frame(rnd, n) for n in (1, 2, 3, 15, 16, 17, 33, 41)])
    r = three_runs(ctx, img, want)
    assert r["outcome"][1:] == (0, "") and not r["fst"].any()


def test_frames_without_blocks_and_without_checksums(ctx):
    """frames without a content checksum (with and without block checksums: only the header check is left) between
    frames that are streamed, and a frame without blocks (the stream ends behind one, so it is the last); 10 frames,
    40 blocks, period 4"""
    rnd = random.Random(0x3203)
    frames = [tiny_frame(rnd, 4), tiny_frame(rnd, 7, flg=0x60), tiny_frame(rnd, 4, flg=0x70), tiny_frame(rnd, 5),
              tiny_frame(rnd, 4, flg=0x64), tiny_frame(rnd, 8), tiny_frame(rnd, 3, flg=0x60), tiny_frame(rnd, 3),
              tiny_frame(rnd, 2, flg=0x70), dict(blocks=[])]
    img, want = build(frames)
    assert len(want["out_len"]) == 40
    r = three_runs(ctx, img, want)
    assert r["outcome"][1:] == (0, "") and not r["fst"].any()


def test_stripes_straddle_blocks_and_group_bounds(ctx):
    """blocks of 1 .. 65 bytes in order, then 63 .. 1: hardly a block ends on a 16-byte stripe, and every pass but a
    frame's first starts inside one (the carry's waiting bytes)"""
    rnd = random.Random(0x3204)
    sizes = list(range(1, 66)) + list(range(63, 0, -1))
    assert len(sizes) == 128 and max(sizes) == 65
    frames = [dict(blocks=[tiny(rnd, s) for s in sizes[k:k + 16]]) for k in range(0, 128, 16)]
    img, want = build(frames)
    r = three_runs(ctx, img, want)
    assert r["outcome"][1:] == (0, "") and not r["fst"].any()
    # and a frame of less than one stripe in all
    img, want = build([dict(blocks=[tiny(rnd, 1) for _ in range(4)]), dict(blocks=[tiny(rnd, 3) for _ in range(4)]),
                       dict(blocks=[tiny(rnd, 4) for _ in range(4)])])
    three_runs(ctx, img, want)


# ---------------------------------------------------------------- checksums that must fail

def test_wrong_stored_content_sum(ctx):
    rnd = random.Random(0x3205)
    frames = [tiny_frame(rnd, 16) for _ in range(8)]
    frames[5]["bad_content"] = True
    img, want = build(frames)
    r = three_runs(ctx, img, want)
    assert r["fst"].tolist() == [0, 0, 0, 0, 0, ST_BAD_CONTENT, 0, 0]
    assert r["outcome"][1:] == (-30, "lz4 stream checksum error")


@pytest.mark.parametrize("pos", [2, 10, 14], ids=["head_group", "middle_group", "tail_group"])
def test_one_changed_byte_in_each_group(ctx, pos):
    """positions 0 .. 7, 8 .. 12 and 13 .. 15 of a frame of sixteen are the three launches: a byte the checksum was not
    made for is found whichever pass hashes it"""
    rnd = random.Random(0x3206 + pos)
    frames = [tiny_frame(rnd, 16) for _ in range(8)]
    frames[3]["blocks"][pos] = flipped(rnd)
    img, want = build(frames)
    assert want["fst"][3] == ST_BAD_CONTENT and want["bst"] == [ST_OK] * 128
    r = three_runs(ctx, img, want)
    assert r["outcome"][1:] == (-30, "lz4 stream checksum error")


def test_wrong_header_check_byte(ctx):
    rnd = random.Random(0x3207)
    frames = [tiny_frame(rnd, 16) for _ in range(8)]
    frames[6]["bad_hc"] = True
    img, want = build(frames)
    r = three_runs(ctx, img, want)
    assert r["fst"].tolist() == [0, 0, 0, 0, 0, 0, ST_BAD_HEADER, 0]
    assert r["outcome"][1:] == (-30, "malformed lz4 data")


@pytest.mark.parametrize("pos", [1, 15], ids=["head_group", "tail_group"])
def test_block_that_fails_in_the_parse(ctx, pos):
    """out_len 0 in mid-frame: the frame's chain goes over the bytes that are there, as the contiguous form's does"""
    rnd = random.Random(0x3208 + pos)
    frames = [tiny_frame(rnd, 16) for _ in range(8)]
    frames[2]["blocks"][pos] = (BAD_BLOCK, b"", dict(fail=True))
    img, want = build(frames)
    assert want["out_len"][32 + pos] == 0 and want["bst"][32 + pos] == ST_DECODE
    r = three_runs(ctx, img, want)
    assert r["outcome"][1:] == (-30, "lz4 decompression failed")


# ---------------------------------------------------------------- blocks of the other expand launches

def test_stored_general_and_segmented_blocks_in_the_slice(ctx):
    """a stored block, a block of few long sequences (the general kernel takes it) and one of 4 097 sequences (the
    segmented launch): none of them is a window launch's, all of them are hashed by the passes"""
    rnd = random.Random(0x3209)
    raw = rnd.randbytes(333)
    long_seqs = lz4_block_from_sequences([(rnd.randbytes(8), 5, 2000)], rnd.randbytes(5))
    dense = lz4_block_from_sequences([(b"xyzw", 2, 4)] + [(b"", rnd.randint(1, 8), 4) for _ in range(4095)], rnd.randbytes(5))
    frames = [tiny_frame(rnd, 16) for _ in range(8)]
    frames[1]["blocks"][3] = (raw, raw, dict(stored=True))
    frames[1]["blocks"][14] = long_seqs
    frames[4]["blocks"][9] = dense
    frames[4]["blocks"][15] = (raw, raw, dict(stored=True))
    frames[6]["blocks"][0] = long_seqs
    img, want = build(frames)
    r = three_runs(ctx, img, want)
    assert r["outcome"][1:] == (0, "") and not r["fst"].any()


# ---------------------------------------------------------------- hash state across batches

P1, P2 = 2654435761, 2246822519


def _xxh_state(data):
    """XXH32 streaming state after `data` from seed 0, as the device's carry record (LA_XXH_CARRY_BYTES)"""
    v = [(P1 + P2) & 0xFFFFFFFF, P2, 0, (0 - P1) & 0xFFFFFFFF]
    full = len(data) // 16 * 16
    for at in range(0, full, 16):
        for j, x in enumerate(struct.unpack_from("<4I", data, at)):
            t = (v[j] + x * P2) & 0xFFFFFFFF
            v[j] = (((t << 13) | (t >> 19)) & 0xFFFFFFFF) * P1 & 0xFFFFFFFF
    mem = data[full:]
    return v, mem, len(data)


def _carry_record(data):
    v, mem, total = _xxh_state(data)
    return struct.pack("<4IIII", *v, len(mem), total & 0xFFFFFFFF, total >> 32) + mem.ljust(16, b"\0") + bytes(20)


def test_hash_state_comes_in_and_goes_out(ctx):
    """the first frame began in an earlier batch (its checksum continues from d_carry_in), the last goes on in the next
    (its state leaves through d_carry_out): neither is streamed, the last pass takes both whole"""
    from libarchive_amd import _native as N
    rnd = random.Random(0x320A)
    frames = [tiny_frame(rnd, 16) for _ in range(8)]
    img, want = build(frames)
    before = rnd.randbytes(1000 + 7)
    first_plain = b"".join(b[1] for b in frames[0]["blocks"])
    last_plain = b"".join(b[1] for b in frames[7]["blocks"])

    def edit(idx):
        f = idx.frames
        f["flags"][0] = N.LA_LZ4F_CONTENT_SUM | N.LA_LZ4F_CONT | N.LA_LZ4F_HASHED
        f["content_sum"][0] = O.xxh32(before + first_plain)
        f["flags"][7] = N.LA_LZ4F_OPEN | N.LA_LZ4F_HASHED | N.LA_LZ4F_HEADER_SUM

    r = three_runs(ctx, img, want, edit=edit, carry_in=_carry_record(before), oracle=False)
    assert not r["fst"].any()
    v, mem, total = _xxh_state(last_plain)
    got = r["carry_out"].tobytes()
    assert struct.unpack_from("<4IIII", got) == (*v, len(mem), total, 0) and got[28:28 + len(mem)] == mem
    # the state that came in counts: another one, and the first frame's checksum is wrong
    r = three_runs(ctx, img, dict(want, fst=[ST_BAD_CONTENT] + [0] * 7), edit=edit, carry_in=_carry_record(before[:-1] + bytes([before[-1] ^ 1])), oracle=False)
    assert r["fst"][0] == ST_BAD_CONTENT


# ---------------------------------------------------------------- the slab's end, and batches that do not split

def test_slab_one_byte_short_for_the_last_row(ctx):
    rnd = random.Random(0x320B)
    img, want = build([tiny_frame(rnd, 16, lo=20) for _ in range(8)])
    total = len(want["slab"])
    keep = total - want["out_len"][-1]
    short = dict(want, slab=want["slab"][:keep])
    r = three_runs(ctx, img, None, dst_cap=total - 1, oracle=False)
    assert r["out_len"].tolist() == want["out_len"]
    assert r["slab"][:keep].tobytes() == short["slab"] and (r["slab"][keep:] == FILL).all()


def test_blocks_not_a_multiple_of_frames(ctx):
    rnd = random.Random(0x320C)
    frames = [tiny_frame(rnd, 16) for _ in range(7)] + [tiny_frame(rnd, 17)]
    frames[7]["bad_content"] = True
    img, want = build(frames)
    r = three_runs(ctx, img, want, split=False)
    assert r["fst"].tolist() == [0] * 7 + [ST_BAD_CONTENT]


def test_periods_outside_4_to_64(ctx):
    rnd = random.Random(0x320D)
    img, want = build([tiny_frame(rnd, 3) for _ in range(8)])
    three_runs(ctx, img, want, split=False)
    img, want = build([tiny_frame(rnd, 65, hi=20)])
    three_runs(ctx, img, want, split=False)
    img, want = build([tiny_frame(rnd, 64, hi=20)])
    three_runs(ctx, img, want, split=True)


# ---------------------------------------------------------------- at size, without the option bit

_kit = None


def _frame_kit():
    """eight frames of sixteen tiny blocks and one of seventeen, built once: (image, expectation) each"""
    global _kit
    if _kit is None:
        rnd = random.Random(0x320E)
        kit = [build([tiny_frame(rnd, 16)]) for _ in range(8)]
        bad = build([tiny_frame(rnd, 16, bad_content=True)])
        seventeen = build([tiny_frame(rnd, 17)])
        _kit = (kit, bad, seventeen)
    return _kit


def _at_size(order):
    img = b"".join(p[0] for p in order)
    want = dict(out_len=[x for p in order for x in p[1]["out_len"]], bst=[x for p in order for x in p[1]["bst"]],
                fst=[x for p in order for x in p[1]["fst"]], slab=b"".join(p[1]["slab"] for p in order))
    return img, want


def test_the_threshold_without_the_option_bit(ctx):
    """2 048 frames of 16 blocks = 32 768 blocks: four slices, the last one (from block 24 576) split; wrong content
    sums in a frame of every slice"""
    kit, bad, _ = _frame_kit()
    order = [kit[i % 8] for i in range(2048)]
    for i in (5, 700, 1535, 1536, 1800, 2047):
        order[i] = bad
    img, want = _at_size(order)
    assert len(want["out_len"]) == 32768
    r = three_runs(ctx, img, want, dst_cap=len(want["slab"]) + 64)      # (the index allows 64 KiB per block: 2 GiB)
    assert np.flatnonzero(r["fst"]).tolist() == [5, 700, 1535, 1536, 1800, 2047]


def test_the_threshold_with_a_frame_of_seventeen(ctx):
    """the same with one frame of 17 blocks in the last quarter: 32 769 blocks in 2 048 frames, no period, no split"""
    kit, bad, seventeen = _frame_kit()
    order = [kit[i % 8] for i in range(2048)]
    order[1900] = seventeen
    order[2040] = bad
    img, want = _at_size(order)
    assert len(want["out_len"]) == 32769
    r = three_runs(ctx, img, want, split=False, dst_cap=len(want["slab"]) + 64)
    assert np.flatnonzero(r["fst"]).tolist() == [2040]


@pytest.mark.parametrize("fault", ["good", "wrong_sum", "changed_byte_below_first"])
@pytest.mark.parametrize("shape", [(17, 15), (15, 17)], ids=["one_block_in_the_slice", "one_block_below_the_slice"])
def test_a_frame_that_straddles_the_first_block_of_the_split_slice(ctx, shape, fault):
    """frames 1535 and 1536 of 17 and 15 blocks (or 15 and 17): still 32 768 blocks in 2 048 frames, period 16, the split
    slice from block 24 576 -- in the middle of a frame.  That frame ends in the split slice, so slice 3's hash launch
    leaves it alone and pass 0 takes its blocks below 24 576 with the first ones of the slice; its carry lies at its last
    block's place.  Once as it should be, once with a wrong stored sum, once with a byte changed in a block BELOW 24 576."""
    kit, _, _ = _frame_kit()
    rnd = random.Random(0x3210 + shape[0])
    straddler = 0 if shape[0] == 17 else 1          # which of the two crosses block 24 576
    pair = [tiny_frame(rnd, shape[0], lo=20), tiny_frame(rnd, shape[1], lo=20)]
    below = 3 if straddler == 0 else 0              # a block of the straddling frame in front of 24 576
    assert 1535 * 16 + (0 if straddler == 0 else shape[0]) + below < 24576 < 1535 * 16 + sum(shape[:straddler + 1])
    if fault == "wrong_sum":
        pair[straddler]["bad_content"] = True
    elif fault == "changed_byte_below_first":
        pair[straddler]["blocks"][below] = flipped(rnd)
    order = [kit[i % 8] for i in range(2048)]
    order[1535], order[1536] = build([pair[0]]), build([pair[1]])
    img, want = _at_size(order)
    assert len(want["out_len"]) == 32768 and len(want["fst"]) == 2048
    r = three_runs(ctx, img, want, dst_cap=len(want["slab"]) + 64)
    assert np.flatnonzero(r["fst"]).tolist() == ([] if fault == "good" else [1535 + straddler])
    assert not r["bst"].any()
