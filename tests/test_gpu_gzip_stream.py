"""The device compressor's second framing and the gzip write filter's "single-member" option.

la_gzc_batch.framing = LA_GZC_FRAME_STREAM makes la_gpu_gzip_compress return a byte-aligned piece of ONE raw-deflate
stream instead of a gzip member per chunk: per chunk a non-final Huffman block followed by zlib's sync-flush shape (the
three bits of an empty stored block's header, padding to the byte, 00 00 FF FF), or a stored block 00 LEN NLEN data when
that is no larger.  No block is final; followed by the empty fixed block 03 00 the piece must inflate to the input.
The filter option frames such pieces as one gzip member: the reference's 10-byte header, the pieces, 03 00, CRC32 and
ISIZE of all the input."""
import gzip
import random
import struct
import time
import zlib

import numpy as np
import pytest

import la_api
import oracle_lib as O
from test_gpu_gzip_write_levels import _datas
from test_gpu_lz4_write import ARCHIVE_OK, write_lz4

pytestmark = pytest.mark.gpu

MODES = (0, 1, 2)       # LA_GZC_FIXED, LA_GZC_DYNAMIC, LA_GZC_STORED
CHUNK = 49152


def _word_text(seed, n):
    rnd = random.Random(seed)
    words = [rnd.randbytes(rnd.randint(2, 10)) for _ in range(150)]
    return b"".join(rnd.choice(words) for _ in range(n // 4 + 1))[:n]


def _dev(data):
    import torch
    return torch.from_numpy(np.frombuffer(data, dtype=np.uint8).copy()).cuda()


def _piece(ctx, d_plain, chunk, mode):
    from libarchive_amd.gzip import compress_to_stream
    return compress_to_stream(ctx, d_plain, chunk, options=mode).cpu().numpy().tobytes()


def _members(ctx, d_plain, chunk, mode):
    from libarchive_amd.gzip import compress_to_members
    return compress_to_members(ctx, d_plain, chunk, mtime=0, options=mode).cpu().numpy().tobytes()


def _inflate_ended(piece):
    """the piece, ended by the caller with an empty final fixed block, through zlib's raw inflate"""
    d = zlib.decompressobj(-15)
    out = d.decompress(piece + b"\x03\x00")
    assert d.eof and d.unused_data == b""
    return out


def _inputs():
    yield "empty", b"", CHUNK
    yield "one_byte", b"q", CHUNK
    # 9-bit literals of the fixed code after a short compressible run: the block's last bit lands on every position
    # within a byte, so every padding length of the tail is used
    for k in range(16):
        yield "tail_%d" % k, bytes(200) + bytes(range(144, 256))[:k], CHUNK
    text = _word_text(3, 3 * 257 + 1)
    yield "exact_chunk", text[:257], 257
    yield "one_byte_over", text[:258], 257
    yield "short_last_chunk", text, 257
    yield "random", random.Random(8).randbytes(100000), CHUNK
    for name, data in _datas():
        yield "levels_" + name, data, CHUNK


_INPUTS = list(_inputs())


@pytest.mark.parametrize("name,data,chunk", _INPUTS, ids=[i[0] for i in _INPUTS])
def test_piece_round_trips_and_is_bounded(gpu_ctx, name, data, chunk):
    d_plain = _dev(data)
    nc = (len(data) + chunk - 1) // chunk
    for mode in MODES:
        piece = _piece(gpu_ctx, d_plain, chunk, mode)
        assert _inflate_ended(piece) == data, (name, mode)
        if not data:
            assert piece == b""
        # derived, not measured: a Huffman chunk trades 26 bytes of member framing for at most 5 of tail, a stored one
        # for none; and no chunk takes more than its stored block
        assert len(piece) <= len(_members(gpu_ctx, d_plain, chunk, mode)) - 21 * nc, (name, mode)
        assert len(piece) <= len(data) + 5 * nc
        if name == "random":
            assert len(piece) == len(data) + 5 * nc         # stored wins in every mode


def test_fixed_tail_uses_every_padding_length(gpu_ctx):
    """The tail_k inputs, fixed mode: one literal more is nine bits more, so sixteen of them end the block on every bit
    of a byte; each piece is a Huffman block (BFINAL 0, BTYPE 01) ending in the sync marker."""
    sizes = []
    for k in range(16):
        piece = _piece(gpu_ctx, _dev(bytes(200) + bytes(range(144, 256))[:k]), CHUNK, 0)
        assert piece[0] & 7 == 2 and piece[-4:] == b"\x00\x00\xff\xff"
        sizes.append(len(piece))
    steps = [b - a for a, b in zip(sizes, sizes[1:])]
    assert set(steps) == {1, 2} and sum(steps) in (16, 17)      # nine bits a step: 135 bits over the fifteen steps


@pytest.mark.parametrize("chunk", [4099, CHUNK])
def test_chunks_are_independent_and_byte_aligned(gpu_ctx, chunk):
    data = _word_text(4, 5 * chunk)
    for mode in MODES:
        whole = _piece(gpu_ctx, _dev(data), chunk, mode)
        last = 0
        for k in range(1, 5):
            part = _piece(gpu_ctx, _dev(data[:k * chunk]), chunk, mode)
            assert last < len(part) < len(whole) and whole.startswith(part), (mode, k)
            # the prefix is a stream of its own: nothing of it leans on the chunk after it
            assert _inflate_ended(part) == data[:k * chunk]
            last = len(part)


def test_no_match_crosses_a_chunk_boundary(gpu_ctx):
    """The second chunk repeats the first: were matches allowed to reach back, it would shrink to a few bytes.  Both
    chunks cost the same, and the second chunk's bytes are those of the same data compressed alone."""
    half = _word_text(5, 4099)
    for mode in (0, 1):
        one = _piece(gpu_ctx, _dev(half), 4099, mode)
        two = _piece(gpu_ctx, _dev(half + half), 4099, mode)
        assert two == one + one, mode


@pytest.mark.parametrize("n,chunk", [(3 * 257 + 1, 257), (100000, CHUNK), (CHUNK, CHUNK), (1, CHUNK)])
def test_stored_only_mode(gpu_ctx, n, chunk):
    data = random.Random(n).randbytes(n)
    piece = _piece(gpu_ctx, _dev(data), chunk, 2)
    nc = (n + chunk - 1) // chunk
    assert len(piece) == n + 5 * nc
    for i in range(nc):
        o, m = i * (chunk + 5), min(chunk, n - i * chunk)
        assert piece[o] == 0 and struct.unpack_from("<HH", piece, o + 1) == (m, m ^ 0xFFFF)
        assert piece[o + 5:o + 5 + m] == data[i * chunk:i * chunk + m]


@pytest.mark.parametrize("framing", [2, 0xFFFFFFFF])
def test_unknown_framing_is_an_argument_error(gpu_ctx, framing):
    import torch
    from libarchive_amd import _native as N
    d_plain = torch.from_numpy(np.frombuffer(b"hello hello hello", dtype=np.uint8).copy()).cuda()
    d_out = torch.full((256,), 0xA5, dtype=torch.uint8, device="cuda")
    d_len = torch.full((1,), -7, dtype=torch.int64, device="cuda")
    for options in MODES + (3,):
        b = N._GzcBatchC()
        b.d_src, b.src_bytes, b.chunk_bytes, b.options = d_plain.data_ptr(), 17, 49152, options
        b.framing = framing
        b.d_out, b.out_cap, b.d_out_bytes = d_out.data_ptr(), 256, d_len.data_ptr()
        assert N.gpu_lib().la_gpu_gzip_compress(gpu_ctx._h, N.C.byref(b)) == -3      # LA_ERR_ARG
    b.framing = N.LA_GZC_FRAME_STREAM           # unknown options are refused in stream framing too
    assert N.gpu_lib().la_gpu_gzip_compress(gpu_ctx._h, N.C.byref(b)) == -3
    gpu_ctx.sync()
    assert int(d_len.cpu()[0]) == -7 and bool((d_out == 0xA5).all())     # nothing written


@pytest.mark.parametrize("name,data", _datas(), ids=[n for n, _ in _datas()])
def test_members_framing_is_the_zeroed_field(gpu_ctx, name, data):
    """LA_GZC_FRAME_MEMBERS, named, writes what a batch whose field was never touched writes"""
    import torch
    from libarchive_amd import _native as N
    d_plain = _dev(data)
    cap = int(N.gpu_lib().la_gpu_gzip_compress_bound(len(data), CHUNK))
    for mode in MODES:
        imgs = []
        for framing in (None, N.LA_GZC_FRAME_MEMBERS):
            d_out = torch.zeros(cap, dtype=torch.uint8, device="cuda")
            d_len = torch.zeros(1, dtype=torch.int64, device="cuda")
            b = N._GzcBatchC()
            b.d_src, b.src_bytes, b.chunk_bytes, b.options = d_plain.data_ptr(), len(data), CHUNK, mode
            b.d_out, b.out_cap, b.d_out_bytes = d_out.data_ptr(), cap, d_len.data_ptr()
            if framing is not None:
                b.framing = framing
            gpu_ctx.gzip_compress(b)
            gpu_ctx.sync()
            imgs.append(d_out[:int(d_len.cpu()[0])].cpu().numpy().tobytes())
        assert imgs[0] == imgs[1] and imgs[0][:4] == b"\x1f\x8b\x08\x04", (name, mode)
        assert gzip.decompress(imgs[0]) == data


def _check_single_member(img, data, xfl):
    assert img[:4] == b"\x1f\x8b\x08\x00" and img[8] == xfl and img[9] == 3
    assert gzip.decompress(img) == data
    d = zlib.decompressobj(31)
    assert d.decompress(img) == data and d.eof and d.unused_data == b""     # exactly one member
    assert struct.unpack("<II", img[-8:]) == (zlib.crc32(data), len(data) & 0xFFFFFFFF)
    assert img[-10:-8] == b"\x03\x00"
    out, res = O.gzip_stream_decode(img, len(data) + 64)
    assert (res.rc, res.errmsg) == (0, b"") and out.tobytes() == data


@pytest.mark.parametrize("name,data", [("empty", b"")] + _datas(), ids=["empty"] + [n for n, _ in _datas()])
def test_single_member_through_the_filter(gpu_ctx, name, data):
    levels = (("0", 0), ("1", 4), ("6", 0), (None, 0)) + ((("9", 2),) if len(data) <= 300000 else ())
    for level, xfl in levels:
        options = (("timestamp", None),) + ((("compression-level", level),) if level is not None else ())
        imgs = []
        for piece in (7, 65537):
            rc, img = write_lz4(data, options + (("single-member", "1"),), piece, codec="gzip")
            assert rc == ARCHIVE_OK, (name, level, piece, img)
            imgs.append(img)
        assert imgs[0] == imgs[1]       # the image does not depend on how the caller cut its writes
        img = imgs[0]
        _check_single_member(img, data, xfl)
        assert img[4:8] == bytes(4)     # "!timestamp"
        if level == "0":
            assert len(img) == 10 + len(data) + 5 * ((len(data) + CHUNK - 1) // CHUNK) + 10
        if len(data) <= 300000:         # (a lone member is one serial unit for the device reader)
            r = la_api.cat(img)
            assert r.data == data and (not data or r.filters[0] == (1, "gzip"))
    if name == "text":
        rc, many = write_lz4(data, (("timestamp", None),), None, codec="gzip")
        assert rc == ARCHIVE_OK and len(img) < len(many)       # 21 bytes a chunk or more


def test_single_member_header_carries_the_time(gpu_ctx):
    t0 = int(time.time())
    rc, img = write_lz4(b"stamped " * 50, (("single-member", "1"),), None, codec="gzip")
    assert rc == ARCHIVE_OK
    assert t0 <= struct.unpack_from("<I", img, 4)[0] <= int(time.time())
    _check_single_member(img, b"stamped " * 50, 0)


def test_single_member_over_several_windows(gpu_ctx, monkeypatch):
    """2.5 MiB through a 1 MiB window: three flushes, each continuing the CRC32 from the one before"""
    monkeypatch.setenv("LA_GPU_WRITE_WINDOW_MIB", "1")
    rnd = random.Random(77)
    data = _word_text(6, 900000) + rnd.randbytes(800000) + bytes(500000) + _word_text(7, (5 << 19) - 2200000)
    assert len(data) == 5 << 19
    for level in (None, "1", "0"):
        options = (("compression-level", level),) if level is not None else ()
        rc, img = write_lz4(data, options + (("single-member", "1"),), 65537, codec="gzip")
        assert rc == ARCHIVE_OK, img
        _check_single_member(img, data, 4 if level == "1" else 0)
        # a window boundary is a chunk boundary and nothing else: the member is the pieces of the three windows
        pieces = b"".join(_piece(gpu_ctx, _dev(data[o:o + (1 << 20)]), CHUNK, {None: 1, "1": 0, "0": 2}[level])
                          for o in range(0, len(data), 1 << 20))
        assert img[10:-10] == pieces


def test_option_off_again_gives_many_members(gpu_ctx):
    data = _word_text(9, 120000)
    rc, want = write_lz4(data, (("timestamp", None),), None, codec="gzip")
    rc2, img = write_lz4(data, (("timestamp", None), ("single-member", "1"), ("single-member", None)), None, codec="gzip")
    assert rc == rc2 == ARCHIVE_OK and img == want
    assert img[:4] == b"\x1f\x8b\x08\x04" and img[12:14] == b"BC"
