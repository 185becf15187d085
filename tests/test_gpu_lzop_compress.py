"""la_gpu_lzop_compress through the C ABI.  Every output, with the header in its gap and the closing word behind it, must
pass lzop_write_support.accept (the stream shape, the proven worst case, the reference's read loop over the Python
decoder) and must decode with this repository's device reader (la_gpu_lzop_decode: status OK, Adler-32 verified, the
input back).  The inputs are lzop_write_support.inputs(): the smallest that reach each border of the shape and each
instruction form the coder writes; what each is there for is asserted from the instruction list of its streams."""
import numpy as np
import pytest
import torch

import lzop_support as LS
import lzop_write_support as W
from libarchive_amd import lzop

pytestmark = pytest.mark.gpu

WANTED_FORMS = {"first_byte_short", "first_byte_long", "literals_short", "literals_long", "m2", "m3_short", "m3_long", "m4_short", "m4_long",
                "zero_bytes", "overlap", "trail_0", "trail_1", "trail_2", "trail_3", "end"}
CASES = [(name, W.BLOCK) for name in sorted(W.inputs())] + [(name, bs) for name in ("text_noise_text", "trails") for bs in (4096, 1)]
_seen = {}      # (name, block_size) -> forms of the case, for the union


def dev(data):
    if not data:
        return torch.zeros(0, dtype=torch.uint8, device="cuda")
    return torch.from_numpy(np.frombuffer(data, dtype=np.uint8).copy()).cuda()


def image(ctx, data, block_size=W.BLOCK, level=5):
    """the blocks behind a gap of 38 bytes, the header written into the gap as the filter does, the closing word"""
    out = lzop.compress_window(ctx, dev(data), block_size, lead_bytes=W.HEADER_BYTES).cpu().numpy().tobytes()
    assert len(out) <= W.HEADER_BYTES + lzop.compress_bound(len(data), block_size) == W.HEADER_BYTES + len(data) + 12 * -(-len(data) // block_size)
    assert out[:W.HEADER_BYTES] == bytes(W.HEADER_BYTES)        # the gap is counted and left untouched
    return W.header(level, 0x5F000000) + out[W.HEADER_BYTES:] + bytes(4)


def checked(ctx, name, block_size):
    """compress, run every reader; returns the image's blocks"""
    data = W.inputs()[name]
    forms = set()
    img = image(ctx, data, block_size)
    blocks = W.accept(img, data, 5, block_size, forms)
    _seen[(name, block_size)] = forms
    # our own device reader over the blocks of the image
    entries, dst = [], 0
    for b in blocks:
        entries.append({"src_off": b["off"] + 12, "src_len": b["csize"], "dst_off": dst, "dst_len": b["usize"], "flags": lzop.U_ADLER32, "sum_u": b["adler"]})
        dst += b["usize"]
    res, plan = lzop.decode_blocks(ctx, img, entries)
    assert not res["status"].any(), sorted(set(int(s) for s in res["status"]))
    assert all(int(r["sum_u"]) == b["adler"] for r, b in zip(res, blocks) if b["stream"] is not None)
    assert plan.slab() == data
    return blocks


def matches(blocks):
    return [i for b in blocks if b["stream"] is not None for i in W.instructions(b["stream"]) if i.distance]


@pytest.mark.parametrize("name,block_size", CASES)
def test_named_inputs(gpu_ctx, name, block_size):
    blocks = checked(gpu_ctx, name, block_size)
    data = W.inputs()[name]
    assert len(blocks) == -(-len(data) // block_size)
    ms = matches(blocks)
    assert all(1 <= m.distance <= W.MAX_DIST and m.length >= 4 for m in ms)
    if name in ("one_byte", "three_bytes", "four_bytes", "noise_2b5") or block_size == 1:
        assert all(b["stream"] is None for b in blocks)         # stored: the image is exactly n + 12 per block
    if name == "run_3b":
        assert all(b["stream"] is not None and b["csize"] <= 512 for b in blocks) and any(m.distance < m.length for m in ms)
    if name.startswith("pair_"):
        dist = int(name[5:])
        (b,) = blocks
        far = [m for m in ms if m.at == 100 + dist]
        if dist <= W.MAX_DIST:
            # the second marker is one M4 of the distance; 20000 and 40000 are the two values of its high distance bit
            assert [(m.form[:2], m.distance) for m in far] == [("m4", dist)] and far[0].length >= 64
        else:
            assert not far and all(W.literal_mask(b["stream"], W.BLOCK)[100 + dist:100 + dist + 64])     # the whole second marker
    if name == "short_far":
        assert [(m.form, m.distance, m.length) for m in ms if m.at == 20100] == [("m4_short", 20000, 6)]
    if name == "long_first":
        first = W.instructions(blocks[0]["stream"])[0]
        assert first.form == "literals_long" and first.length > 238
    if name == "period3":
        first, second = W.instructions(blocks[0]["stream"])[:2]
        assert (first.form, first.length) == ("first_byte_short", 3) and second.distance == 3 and second.length > 3


def test_union_of_forms(gpu_ctx):
    """every form the coder can write is written by some input (if one is missing, an input is reshaped, not the coder)"""
    for name, block_size in CASES:
        if (name, block_size) not in _seen:
            checked(gpu_ctx, name, block_size)
    union = set().union(*_seen.values())
    assert union == WANTED_FORMS, (sorted(WANTED_FORMS - union), sorted(union - WANTED_FORMS))


def test_no_input_writes_only_the_gap(gpu_ctx):
    for lead in (0, 38):
        d_out = torch.full((64,), 0xA5, dtype=torch.uint8, device="cuda")
        _, need = lzop.compress_window(gpu_ctx, dev(b""), W.BLOCK, lead_bytes=lead, out_cap=64, d_out=d_out)
        assert need == lead and d_out.cpu().numpy().tobytes() == b"\xa5" * 64


def test_lead_bytes_leave_the_gap_untouched_and_are_counted(gpu_ctx):
    data = W.inputs()["block_plus_1"]
    plain = lzop.compress_window(gpu_ctx, dev(data)).cpu().numpy().tobytes()
    d_out = torch.full((len(plain) + 38 + 64,), 0xA5, dtype=torch.uint8, device="cuda")
    _, need = lzop.compress_window(gpu_ctx, dev(data), W.BLOCK, lead_bytes=38, out_cap=len(plain) + 38, d_out=d_out)
    got = d_out.cpu().numpy().tobytes()
    assert need == len(plain) + 38 and got == b"\xa5" * 38 + plain + b"\xa5" * 64


@pytest.mark.parametrize("block_size", [W.BLOCK, 4096])
def test_short_output_buffer(gpu_ctx, block_size):
    """la_gpu_lzip_compress's way: *d_out_bytes is the size needed, nothing is written at or behind out_cap"""
    data = W.inputs()["text_noise_text"]
    img = lzop.compress_window(gpu_ctx, dev(data), block_size).cpu().numpy().tobytes()
    for cap in (0, 5, 11, 12, 25, len(img) - 1):
        d_out = torch.full((len(img) + 64,), 0xA5, dtype=torch.uint8, device="cuda")
        _, need = lzop.compress_window(gpu_ctx, dev(data), block_size, out_cap=cap, d_out=d_out)
        got = d_out.cpu().numpy().tobytes()
        assert need == len(img) > cap
        assert got[:cap] == img[:cap]
        assert got[cap:] == b"\xa5" * (len(got) - cap)


def test_bad_block_sizes_are_refused(gpu_ctx):
    assert lzop.compress_bound(100, 0) == 0
    for bs in (0, 65537):
        with pytest.raises(RuntimeError, match=r"la_gpu_lzop_compress failed \(-3\)"):     # LA_ERR_ARG
            lzop.compress_window(gpu_ctx, dev(b"abcdefgh"), bs, out_cap=64)
    assert len(lzop.compress_window(gpu_ctx, dev(b"abcdefgh"), 65536)) == 20
