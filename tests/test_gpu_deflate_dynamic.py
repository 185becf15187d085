"""Device gzip compression with a block mode (la_gzc_batch.options): LA_GZC_FIXED writes what the compressor always
wrote, LA_GZC_DYNAMIC the smallest of a dynamic-Huffman, the fixed-Huffman and the stored block per chunk,
LA_GZC_STORED stored blocks only.  Every image must inflate to the input with zlib, the oracle's gzip filter, this
repository's read path and every kernel variant of the device decoder; the dynamic mode is never larger than the
fixed one, member by member; the fixed mode's bytes are the ones recorded before the dynamic kernel existed; and what
the dynamic mode saves is held against what zlib saves when it goes from Z_FIXED to built codes.

Measured on one MI355X (profiles/r05_deflate_dynamic.txt), chunk 49152:
    2 MiB word text    fixed 961142 B, dynamic 842612 B: s_dev 0.1233; zlib level 1 per chunk 871866 -> 743145 B: s_zlib 0.1476
    2 MiB skewed text  fixed 1868302 B, dynamic 1291426 B: s_dev 0.3088; zlib 1818600 -> 1289872 B: s_zlib 0.2907
On the word text the device keeps 0.835 of zlib's gain.  That is the token mix, not the code builder: on these
histograms its lengths cost 0.01-0.09 % more bits than an unconstrained Huffman code's; the words are random bytes, so
the literals the greedy matcher leaves over (more than zlib's) have a flat histogram that no code shortens."""
import gzip
import hashlib
import io
import random
import struct
import zlib

import numpy as np
import pytest

import la_api
import oracle_lib as O
import streams as S
from test_gpu_gzip import ST_OK, gpu_inflate

pytestmark = pytest.mark.gpu
FIXED, DYNAMIC, STORED = 0, 1, 2
MTIME = 1234567


def _word_text(seed, n_words, size):
    rnd = random.Random(seed)
    words = [rnd.randbytes(rnd.randint(2, 11)) for _ in range(300)]
    return b"".join(rnd.choice(words) for _ in range(n_words))[:size], rnd


def _skewed_text(size, seed=5):
    """letters drawn one by one with English-like weights: nothing to match, literals alone compress"""
    letters = b" etaoinshrdlcumwfgypbvkjxqz"
    weights = [18.0, 12.7, 9.1, 8.2, 7.5, 7.0, 6.7, 6.3, 6.1, 6.0, 4.3, 4.0, 2.8, 2.8, 2.4, 2.4, 2.2, 2.0, 2.0, 1.9,
               1.5, 1.0, 0.8, 0.15, 0.15, 0.1, 0.07]
    return bytes(random.Random(seed).choices(letters, weights, k=size))


def _de_bruijn(k, n):
    a, seq = [0] * (k * n), []

    def db(t, p):
        if t > n:
            if n % p == 0:
                seq.extend(a[1:p + 1])
        else:
            a[t] = a[t - p]
            db(t + 1, p)
            for j in range(a[t - p] + 1, k):
                a[t] = j
                db(t + 1, t)
    db(1, 1)
    return bytes(seq)


def _fibonacci_ladder():
    """17 symbols with Fibonacci counts (4180 bytes), shuffled: an unconstrained Huffman code for them is 16 deep"""
    fib = [1, 1]
    while len(fib) < 17:
        fib.append(fib[-1] + fib[-2])
    b = bytearray()
    for i, c in enumerate(fib):
        b += bytes([65 + i]) * c
    random.Random(17).shuffle(b)
    return bytes(b)


TEXT_2M = _word_text(2, 400000, 2 << 20)[0]         # the text of test_gpu_gzip_compress.test_ratio_and_stored_fallback
SKEWED_2M = _skewed_text(2 << 20)


def _inputs():
    # the inputs of test_gpu_gzip_compress._inputs(), restated
    rnd = random.Random(777)
    words = [rnd.randbytes(rnd.randint(2, 11)) for _ in range(300)]
    text = b"".join(rnd.choice(words) for _ in range(120000))
    yield "one_byte", b"q"
    yield "two", b"ab"
    yield "three_same", b"aaa"
    yield "zeros", bytes(200000)
    yield "random", rnd.randbytes(150000)
    yield "text", text
    yield "period3", b"xyz" * 40000
    yield "high_bytes", bytes(range(144, 256)) * 300
    yield "long_runs", b"".join(bytes([i & 255]) * (i * 7 % 700 + 1) for i in range(600))
    _, plain = S.synth_lz4_stream(5, 0, 2, blocks_per_frame=16, block_size=65536, nthreads=2)
    yield "c2_like", plain.tobytes()
    # what a built code has to get right
    yield "skewed_text", _skewed_text(300000, seed=6)
    yield "same_x1", b"k"
    yield "same_x2", b"kk"
    yield "same_x49152", b"k" * 49152
    yield "all_256_once", bytes(range(256))
    yield "fibonacci_ladder", _fibonacci_ladder()
    yield "one_distance_64", bytes(range(64)) * 700
    yield "one_distance_7", b"abcdefg" * 5000
    yield "no_match_de_bruijn", _de_bruijn(37, 3)[:49152]
    yield "no_match_increasing", struct.pack(">8000H", *range(0, 64000, 8))


def _mixes():
    """200 seeded mixes of runs, noise, words, skewed letters and repeats of earlier pieces"""
    for seed in range(200):
        rnd = random.Random(9000 + seed)
        words = [rnd.randbytes(rnd.randint(1, 9)) for _ in range(rnd.randint(2, 60))]
        parts, size = [], 0
        target = rnd.choice([1, 2, 3, 17, 257, 999, 1000, 1001, 4095, 4096, 4097, 20000, 49151, 49152, 49153, 70000])
        while size < target:
            kind = rnd.randrange(5)
            n = rnd.randint(1, 3000)
            p = (bytes([rnd.randrange(256)]) * n if kind == 0 else rnd.randbytes(n) if kind == 1 else
                 b"".join(rnd.choice(words) for _ in range(n // 4 + 1)) if kind == 2 else
                 _skewed_text(n, seed=rnd.randrange(1 << 30)) if kind == 3 else
                 (rnd.choice(parts) if parts else b"ab") * rnd.randint(1, 4))
            parts.append(p)
            size += len(p)
        yield "mix%03d" % seed, b"".join(parts)[:target]


def _compress(ctx, data, chunk, mode):
    import torch
    from libarchive_amd.gzip import compress_to_members
    d_plain = torch.from_numpy(np.frombuffer(data, dtype=np.uint8).copy()).cuda()
    return compress_to_members(ctx, d_plain, chunk, mtime=MTIME, options=mode).cpu().numpy().tobytes()


def _members(img):
    """[(member bytes, BTYPE of its one block)] by the BC size subfields"""
    pos, out = 0, []
    while pos < len(img):
        assert img[pos:pos + 4] == b"\x1f\x8b\x08\x04" and img[pos + 12:pos + 16] == b"BC\x02\x00"
        assert struct.unpack_from("<I", img, pos + 4)[0] == MTIME
        bsize = struct.unpack_from("<H", img, pos + 16)[0] + 1
        assert pos + bsize <= len(img)
        first = img[pos + 18]
        assert first & 1, "BFINAL must be set: one block per member"
        out.append((img[pos:pos + bsize], (first >> 1) & 3))
        pos += bsize
    return out


def _check_image(ctx, data, chunk, mode, img, device_variants):
    mem = _members(img)
    got = bytearray()
    for m, _ in mem:
        d = zlib.decompressobj(-15)
        body = d.decompress(m[18:])
        assert d.eof and len(d.unused_data) == 8
        crc, isize = struct.unpack("<II", d.unused_data)
        assert crc == zlib.crc32(body) and isize == len(body)
        got += body
    assert bytes(got) == data and len(mem) == (len(data) + chunk - 1) // chunk
    assert gzip.GzipFile(fileobj=io.BytesIO(img)).read() == data
    out, res = O.gzip_stream_decode(img, len(data) + 64)
    assert (res.rc, res.errmsg) == (0, b"") and out.tobytes() == data
    if chunk >= 4096:
        r = la_api.cat(img)
        assert r.filters[0] == (1, "gzip") and r.data == data
    if device_variants:
        # wave-per-member, lane-per-member and both two-phase kernels; gpu_inflate asserts that they agree
        res, sm = gpu_inflate(ctx, [m[18:] for m, _ in mem], [min(chunk, len(data) - i * chunk) for i in range(len(mem))])
        assert [st for st, _, _, _ in res] == [ST_OK] * len(mem) and b"".join(o for _, o, _, _ in res) == data
    return mem


def _check_all_modes(ctx, name, data, chunks):
    from libarchive_amd import _native as N
    for chunk in chunks:
        mem = {}
        for mode in (FIXED, DYNAMIC, STORED):
            img = _compress(ctx, data, chunk, mode)
            mem[mode] = _check_image(ctx, data, chunk, mode, img, device_variants=(mode == DYNAMIC and chunk > 1))
            assert len(img) <= N.gpu_lib().la_gpu_gzip_compress_bound(len(data), chunk)
        # block types
        assert all(bt == 0 for _, bt in mem[STORED]), (name, chunk)
        assert all(bt in (0, 1) for _, bt in mem[FIXED]), (name, chunk)
        assert all(bt in (0, 1, 2) for _, bt in mem[DYNAMIC]), (name, chunk)
        # never larger, member by member: the dynamic mode picks the smallest of the three exact sizes
        for i, ((md, _), (mf, _)) in enumerate(zip(mem[DYNAMIC], mem[FIXED])):
            n = min(chunk, len(data) - i * chunk)
            assert len(md) <= len(mf) <= n + 31, (name, chunk, i, len(md), len(mf), n)
        for i, (ms, _) in enumerate(mem[STORED]):
            assert len(ms) == min(chunk, len(data) - i * chunk) + 31
    return mem


@pytest.mark.parametrize("name,data", list(_inputs()), ids=[n for n, _ in _inputs()])
def test_round_trip_every_mode(gpu_ctx, name, data):
    mem = _check_all_modes(gpu_ctx, name, data, (49152, 4096, 1000) + ((1,) if len(data) <= 4096 else ()))
    if name in ("text", "skewed_text"):      # the last chunk size checked was 1000; the claim is about 49152
        img = _compress(gpu_ctx, data, 49152, DYNAMIC)
        assert any(bt == 2 for _, bt in _members(img)), "no dynamic-Huffman block on text at 48 KiB chunks"
    del mem


def test_round_trip_seeded_mixes(gpu_ctx):
    for name, data in _mixes():
        _check_all_modes(gpu_ctx, name, data, (49152, 4096, 1000) + ((1,) if len(data) <= 4096 else ()))


# SHA-256 of the images the compressor wrote before it had modes (chunk 49152, mtime 1234567), on one MI355X
_BEFORE = {
    "word_text_2m": (961142, "98835460d077b8f451cffd83021cc3a55f055de94bb55dac15c359a213a2065e"),
    "c2_like": (1384045, "160595c4be45983de3060a1efa27f0e6d8351fa022bb5d582f514c7b4f7d8960"),
    "noise_1m": (1049258, "73d2f2a0805ba56c972f18d9b153deb7069aa1ac2e3b77e67b40c1c6191871dc"),
}


def test_fixed_mode_writes_the_bytes_it_always_wrote(gpu_ctx):
    text, rnd = _word_text(2, 400000, 2 << 20)
    noise = rnd.randbytes(1 << 20)
    _, plain = S.synth_lz4_stream(5, 0, 2, blocks_per_frame=16, block_size=65536, nthreads=2)
    for name, data in (("word_text_2m", text), ("c2_like", plain.tobytes()), ("noise_1m", noise)):
        img = _compress(gpu_ctx, data, 49152, FIXED)
        assert (len(img), hashlib.sha256(img).hexdigest()) == _BEFORE[name], name


def _zlib_chunks(data, strategy, chunk=49152):
    total = 0
    for i in range(0, len(data), chunk):
        co = zlib.compressobj(1, zlib.DEFLATED, -15, 8, strategy)
        total += len(co.compress(data[i:i + chunk]) + co.flush())
    return total


# What the dynamic mode must keep of zlib's own gain from building codes, s_dev >= _F * s_zlib: the quotient measured
# on the MI355X lowered by one tenth (the sizes are deterministic; the margin is for a later matcher change that shifts
# the token mix).  Word text: 0.1233 / 0.1476 = 0.835.  Skewed text: 0.3088 / 0.2907 = 1.062.
_F = {"word_text": 0.75, "skewed_text": 0.95}
# total size against zlib.compress(level 1), as test_ratio_and_stored_fallback has it for the fixed mode with 1.6:
# measured 1.249 on the word text and 1.007 on the skewed text, rounded up to the next 0.05
_VS_ZLIB1 = {"word_text": 1.25, "skewed_text": 1.05}


@pytest.mark.parametrize("name", ["word_text", "skewed_text"])
def test_ratio_against_zlib(gpu_ctx, name):
    data = TEXT_2M if name == "word_text" else SKEWED_2M
    fixed = len(_compress(gpu_ctx, data, 49152, FIXED))
    dyn_img = _compress(gpu_ctx, data, 49152, DYNAMIC)
    dyn = len(dyn_img)
    z_fixed, z_default = _zlib_chunks(data, zlib.Z_FIXED), _zlib_chunks(data, zlib.Z_DEFAULT_STRATEGY)
    zlib1 = len(zlib.compress(data, 1))
    s_dev, s_zlib = 1 - dyn / fixed, 1 - z_default / z_fixed
    print("%s: fixed %d dynamic %d s_dev %.4f | zlib L1 per chunk Z_FIXED %d default %d s_zlib %.4f | quotient %.3f | "
          "dynamic / zlib.compress(1) = %d / %d = %.3f" % (name, fixed, dyn, s_dev, z_fixed, z_default, s_zlib,
                                                         s_dev / s_zlib, dyn, zlib1, dyn / zlib1))
    assert sum(bt == 2 for _, bt in _members(dyn_img)) == len(_members(dyn_img))
    assert dyn < fixed
    assert s_dev >= _F[name] * s_zlib, (s_dev, s_zlib)
    assert _VS_ZLIB1[name] < 1.6 and dyn < _VS_ZLIB1[name] * zlib1, (dyn, zlib1)


@pytest.mark.parametrize("options", [3, 0x100, 0xFFFFFFFF])
def test_unknown_mode_is_an_argument_error(gpu_ctx, options):
    import torch
    from libarchive_amd import _native as N
    d_plain = torch.from_numpy(np.frombuffer(b"hello hello hello", dtype=np.uint8).copy()).cuda()
    d_out = torch.full((256,), 0xA5, dtype=torch.uint8, device="cuda")
    d_len = torch.full((1,), -7, dtype=torch.int64, device="cuda")
    b = N._GzcBatchC()
    b.d_src, b.src_bytes, b.chunk_bytes, b.options = d_plain.data_ptr(), 17, 49152, options
    b.d_out, b.out_cap, b.d_out_bytes = d_out.data_ptr(), 256, d_len.data_ptr()
    assert N.gpu_lib().la_gpu_gzip_compress(gpu_ctx._h, N.C.byref(b)) == -3      # LA_ERR_ARG
    gpu_ctx.sync()
    assert int(d_len.cpu()[0]) == -7 and bool((d_out == 0xA5).all())     # nothing written
