"""Device zstd compression (la_gpu_zstd_compress through zstd.compress_to_frames): every image must decode to the input
with everything that reads the format -- the image's libzstd (the library the reference's filter calls), the oracle's
stream decoder and this repository's own device decoder -- and its frame and block headers must have the shape the
writer promises (single segment, exact content sizes, the checksum flag as asked, block sizes within the limits).
The compressed bytes themselves are not libzstd's (a zstd stream is not unique)."""
import ctypes as C
import random
import time

import numpy as np
import pytest

import zstd_support as Z

pytestmark = pytest.mark.gpu

CHECKSUM, RAW_LITERALS = 1, 2
SHAPES = [(131072, 1), (131072, 4), (65536, 2), (1024, 3)]


def _z():
    z = Z.libzstd()
    if z is None:
        pytest.fail("no libzstd.so.1 in this image")
    return z


def _text(rnd, n):
    words = [bytes(rnd.choice(b"abcdefghijklmnopqrstuvwxyz") for _ in range(rnd.randint(2, 9))) for _ in range(400)]
    out = bytearray()
    while len(out) < n:
        out += rnd.choice(words) + rnd.choice([b" ", b" ", b" ", b", ", b".\n"])
    return bytes(out[:n])


def _binary_high(rnd, n):
    """bytes above 128 with structure: records of a few fixed fields and a counter"""
    out = bytearray()
    i = 0
    while len(out) < n:
        out += bytes([0xF0 | (i & 15), 0xC3, 0xA9, 0x80 + (i % 64)]) + (i * 2654435761 & 0xFFFFFFFF).to_bytes(4, "little") + b"\xff\xfe"
        i += rnd.randint(1, 3)
    return bytes(out[:n])


def _inputs():
    rnd = random.Random(8878)
    text = _text(rnd, 700000)
    seqs = bytearray()          # a block with far more than 127 sequences: short repeats of 5..9 bytes between literals
    while len(seqs) < 300000:
        seqs += rnd.randbytes(rnd.randint(0, 3))
        k = rnd.randint(5, 9)
        seqs += bytes(seqs[-k - rnd.randint(1, 200):][:k]) if len(seqs) > 300 else rnd.randbytes(k)
    return [
        ("empty", b""), ("one", b"\x07"), ("three", b"abc"),
        ("zeros", bytes(3 * 131072)), ("random", rnd.randbytes(300000)), ("text", text),
        ("binary_high", _binary_high(rnd, 400000)), ("period3", b"xyz" * 100000),
        ("ragged", text[:131072 * 2 + 4097]),
        ("long_run", rnd.randbytes(100) + b"q" * 120000 + rnd.randbytes(100)),
        ("random_then_repeats", (lambda r: r + r[:60000] + r[5000:20000])(rnd.randbytes(70000))),
        ("many_sequences", bytes(seqs)),
    ]


INPUTS = _inputs()


def walk(img):
    """frame / block headers of an image: [{single, fcs, csum, blocks: [(type, size, literals type)]}]"""
    frames, p = [], 0
    while p < len(img):
        assert int.from_bytes(img[p:p + 4], "little") == 0xFD2FB528
        fhd = img[p + 4]
        single, csum, fcs_flag = (fhd >> 5) & 1, (fhd >> 2) & 1, fhd >> 6
        assert fhd & 0x0B == 0, fhd            # no dictionary id, reserved bit clear
        q = p + 5 + (0 if single else 1)
        fl = [1 if single else 0, 2, 4, 8][fcs_flag]
        fcs = int.from_bytes(img[q:q + fl], "little") + (256 if fl == 2 else 0)
        q += fl
        blocks = []
        while True:
            bh = int.from_bytes(img[q:q + 3], "little")
            q += 3
            bt, bs = (bh >> 1) & 3, bh >> 3
            blocks.append((bt, bs, img[q] & 3 if bt == 2 else None))
            q += 1 if bt == 1 else bs
            if bh & 1:
                break
        q += 4 if csum else 0
        frames.append({"single": single, "fcs": fcs, "csum": csum, "blocks": blocks})
        p = q
    assert p == len(img)
    return frames


def compress(gpu_ctx, data, bs, bpf, flags):
    import torch
    from libarchive_amd import zstd
    d = torch.from_numpy(np.frombuffer(data, dtype=np.uint8).copy()).cuda() if data else torch.empty(0, dtype=torch.uint8, device="cuda")
    return zstd.compress_to_frames(gpu_ctx, d, bs, bpf, flags).cpu().numpy().tobytes()


def device_decode(gpu_ctx, img, n):
    """the image through this repository's walker and device decoder; the walker's slots are the exact content sizes"""
    import torch
    from libarchive_amd import zstd
    frames, end_kind, consumed, dst_bytes = zstd.index_image(img)
    assert consumed == len(img) and int(frames["dst_cap"].sum()) == n
    d_src = torch.from_numpy(np.frombuffer(img, dtype=np.uint8).copy()).cuda()
    plan = zstd.ZstdDevicePlan(gpu_ctx, d_src, frames, dst_bytes)
    plan.run()
    res = plan.results()
    assert (res["status"] == 0).all(), res["status"]
    assert (res["out_len"] == frames["dst_cap"]).all()
    dst = plan.d_dst.cpu().numpy()
    return b"".join(dst[int(f["dst_off"]):int(f["dst_off"]) + int(f["dst_cap"])].tobytes() for f in frames)


def check_image(gpu_ctx, z, o, data, img, bs, bpf, flags, device=True):
    n = len(data)
    assert Z.zstd_decompress(z, img, n + 16) == data
    assert Z.oracle_decode(o, img, n + 16) == (0, data, "")
    if device:
        assert device_decode(gpu_ctx, img, n) == data
    frames = walk(img)
    per = bs * bpf
    assert len(frames) == max(1, -(-n // per))
    for i, fr in enumerate(frames):
        assert fr["single"] == 1 and fr["csum"] == (1 if flags & CHECKSUM else 0)
        assert fr["fcs"] == min(per, n - i * per) if n else fr["fcs"] == 0
        assert all(b[1] <= min(fr["fcs"], 131072) for b in fr["blocks"])
        assert len(fr["blocks"]) == max(1, -(-fr["fcs"] // bs))
    return frames


@pytest.mark.parametrize("name,data", INPUTS, ids=[n for n, _ in INPUTS])
def test_round_trip_every_shape_and_flag(gpu_ctx, name, data):
    z, o = _z(), Z.oracle_lib()
    for bs, bpf in SHAPES:
        for flags in (0, CHECKSUM, RAW_LITERALS, CHECKSUM | RAW_LITERALS):
            img = compress(gpu_ctx, data, bs, bpf, flags)
            check_image(gpu_ctx, z, o, data, img, bs, bpf, flags)


def test_block_types(gpu_ctx):
    z, o = _z(), Z.oracle_lib()
    zeros = bytes(4 * 131072)
    fr = check_image(gpu_ctx, z, o, zeros, compress(gpu_ctx, zeros, 131072, 1, CHECKSUM), 131072, 1, CHECKSUM)
    assert all(b[0] == 1 for f in fr for b in f["blocks"])                       # RLE blocks
    rnd = random.Random(3)
    rand = rnd.randbytes(1 << 20)
    img = compress(gpu_ctx, rand, 131072, 1, CHECKSUM)
    fr = check_image(gpu_ctx, z, o, rand, img, 131072, 1, CHECKSUM)
    assert all(b[0] == 0 for f in fr for b in f["blocks"])                       # raw blocks
    assert len(img) <= len(rand) + len(fr) * (6 + 4 + 4 + 3)                     # the documented per-frame overhead
    text = _text(rnd, 1 << 20)
    img_h = compress(gpu_ctx, text, 131072, 1, CHECKSUM)
    fr = check_image(gpu_ctx, z, o, text, img_h, 131072, 1, CHECKSUM)
    assert all(b[0] == 2 and b[2] == 2 for f in fr for b in f["blocks"])         # Compressed_Literals_Block
    img_r = compress(gpu_ctx, text, 131072, 1, CHECKSUM | RAW_LITERALS)
    fr = check_image(gpu_ctx, z, o, text, img_r, 131072, 1, CHECKSUM | RAW_LITERALS)
    assert all(b[0] == 2 and b[2] == 0 for f in fr for b in f["blocks"])         # Raw_Literals_Block
    assert len(img_h) < len(img_r)
    import torch
    from libarchive_amd import lz4
    d = torch.from_numpy(np.frombuffer(text, dtype=np.uint8).copy()).cuda()
    assert len(img_h) < int(lz4.compress_to_frames(gpu_ctx, d).numel())


def test_empty_input_is_one_frame(gpu_ctx):
    z = _z()
    img = compress(gpu_ctx, b"", 131072, 1, CHECKSUM)
    buf = C.create_string_buffer(16)
    assert z.ZSTD_decompress(buf, 16, img, len(img)) == 0
    fr = walk(img)
    assert len(fr) == 1 and fr[0]["fcs"] == 0 and fr[0]["blocks"] == [(0, 0, None)]
    assert img[-4:] == bytes.fromhex("99e9d851")                                 # XXH64 of nothing, low 32 bits


def test_out_cap_and_argument_checks(gpu_ctx):
    import torch
    from libarchive_amd import _native as N
    data = _text(random.Random(5), 500000)
    full = compress(gpu_ctx, data, 131072, 1, CHECKSUM)
    d = torch.from_numpy(np.frombuffer(data, dtype=np.uint8).copy()).cuda()
    cap = len(full) // 2
    d_out = torch.full((len(full) + 64,), 0xA5, dtype=torch.uint8, device="cuda")
    d_len = torch.zeros(1, dtype=torch.int64, device="cuda")
    b = N._ZstdcBatchC()
    b.d_src, b.src_bytes = d.data_ptr(), len(data)
    b.block_size, b.blocks_per_frame, b.flags = 131072, 1, CHECKSUM
    b.d_out, b.out_cap, b.d_out_bytes = d_out.data_ptr(), cap, d_len.data_ptr()
    gpu_ctx.zstd_compress(b)
    gpu_ctx.sync()
    assert int(d_len.cpu()[0]) == len(full)
    assert (d_out[cap:].cpu().numpy() == 0xA5).all()                             # nothing past out_cap
    lib = N.gpu_lib()
    for bad in (0, 131073):
        b.block_size = bad
        assert lib.la_gpu_zstd_compress(gpu_ctx._h, C.byref(b)) == -3         # LA_ERR_ARG
    b.block_size, b.blocks_per_frame = 131072, 0
    assert lib.la_gpu_zstd_compress(gpu_ctx._h, C.byref(b)) == -3


def test_randomized_sweep_through_libzstd(gpu_ctx):
    z = _z()
    rnd = random.Random(0x5A5A)
    t0 = time.time()
    for it in range(300):
        n = rnd.choice([0, 1, 7, 100, 1023, 1024, 1025, 5000, 65536, 70000, 131073, 250000])
        data = Z.gen(rnd, n, rnd.randint(0, 4)) if rnd.random() < 0.8 else _text(rnd, n)
        bs = rnd.choice([1024, 4096, 65536, 131072, rnd.randint(1, 131072)])
        bpf = rnd.choice([1, 2, 5])
        flags = rnd.choice([0, CHECKSUM, RAW_LITERALS, CHECKSUM | RAW_LITERALS])
        img = compress(gpu_ctx, data, bs, bpf, flags)
        assert Z.zstd_decompress(z, img, n + 16) == data, (it, n, bs, bpf, flags)
        assert len(walk(img)) == max(1, -(-n // (bs * bpf)))
        assert time.time() - t0 < 240
