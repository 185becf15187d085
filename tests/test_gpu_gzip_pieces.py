"""Pieces of ONE raw-deflate stream through la_gpu_gzip_decode with LA_GZ_OPT_PIECES, by all four forced paths
(wave per member, lane per member in place, two-phase, two-phase with the in-order expand), which must agree.

A piece is a span that claims to start on a byte-aligned block boundary.  It ends with LA_ST_OK (a final block ended),
LA_ST_GZ_PIECE_END (18: a non-final block ended with not one bit of the span unread), LA_ST_GZ_NEEDS_HISTORY (19: a match
reaches in front of the piece's first byte) or as any member does.  What is expected comes from Python's zlib:
decompressobj(-15) over a piece gives its plain bytes, eof == False and no unused data; for a refused piece the bytes in
front of the error are the CPU oracle's (tests/oracle_lib.py, held to zlib by tests/test_oracle*.py), of which what zlib
hands out when fed byte by byte must be a prefix.

Every piece has its own slot in a destination prefilled with a guard byte, 64 guard bytes between slots; nothing outside
the slots may change.  Sources sit at chosen offsets (src_off & 3 = 0..3, src_off & 127 near 0 and 127)."""
import json
import os
import random
import zlib

import numpy as np
import pytest

import deflate_build as B
import oracle_lib as O

pytestmark = pytest.mark.gpu

OPT_WAVE, OPT_LANE, OPT_TWO_PHASE, OPT_RAW, OPT_INORDER, OPT_PIECES = 2, 4, 8, 16, 32, 64
PATHS = ((OPT_WAVE, "wave per member"), (OPT_LANE, "lane per member, in place"), (OPT_TWO_PHASE, "two-phase"),
         (OPT_TWO_PHASE | OPT_INORDER, "two-phase, in-order expand"))
ST_OK, ST_DATA, ST_TRUNC, ST_FULL, ST_PIECE_END, ST_NEEDS_HISTORY = 0, 5, 6, 9, 18, 19
GUARD = 0xA5
MARKER = b"\x00\x00\xff\xff"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "deflate_handbuilt.json")
WORDS = [b"window", b"piece", b"flush", b"marker", b"deflate", b"stored", b"lane", b"wave", b"boundary", b"history", b"the", b"of"]


def word_text(n, seed=7):
    r = random.Random(seed)
    return b" ".join(r.choice(WORDS) for _ in range(n // 4))[:n]


def zlib_flushed(plain, step, flush, level=6):
    """raw deflate of `plain` in steps with a flush behind each; returns (body, [piece spans]) -- the body ends in the
    final block zlib's flush(Z_FINISH) writes behind the last marker (03 00)"""
    c = zlib.compressobj(level, zlib.DEFLATED, -15)
    pieces = []
    for i in range(0, len(plain), step) if step else [None] * 3:
        pieces.append((c.compress(plain[i:i + step]) if step else b"") + c.flush(flush))
    tail = c.flush()
    return b"".join(pieces) + tail, pieces, tail


def zlib_piece(span):
    d = zlib.decompressobj(-15)
    out = d.decompress(span)
    assert not d.eof and d.unused_data == b""
    return out


@pytest.fixture(scope="module")
def text():
    return word_text(240000)


@pytest.fixture(scope="module")
def full(text):
    return zlib_flushed(text, 20000, zlib.Z_FULL_FLUSH)


@pytest.fixture(scope="module")
def sync(text):
    return zlib_flushed(text, 20000, zlib.Z_SYNC_FLUSH)


def run_table(gpu_ctx, entries, options, lead=0, pack=False):
    """entries: [(source bytes, dst_cap)]; the first source sits at offset `lead`, the others follow back to back (pack)
    or at the next multiple of 128 plus their index (so that every src_off & 3 occurs).  Returns [(status, bytes,
    consumed, crc32)] and checks the guard."""
    import torch
    from libarchive_amd import _native as N
    n = len(entries)
    mem = np.zeros(n, dtype=N.GZ_MEMBER_DTYPE)
    src = bytearray(b"\x5a" * lead)
    do = 64
    for i, (img, cap) in enumerate(entries):
        if not pack and i:
            src += b"\x5a" * ((-len(src)) % 128 + (i % 131))
        mem[i] = (len(src), len(img), cap, do)
        src += img
        do += cap + 64
    d_src = torch.from_numpy(np.frombuffer(bytes(src) + bytes(64), dtype=np.uint8).copy()).cuda()
    d_mem = torch.from_numpy(mem.view(np.uint8).reshape(-1).copy()).cuda()
    d_dst = torch.full((do,), GUARD, dtype=torch.uint8, device="cuda")
    d_res = torch.zeros(n * 16, dtype=torch.uint8, device="cuda")
    d_sum = torch.zeros(32, dtype=torch.uint8, device="cuda")
    bt = N._GzBatchC()
    bt.d_src = d_src.data_ptr(); bt.src_bytes = len(src)
    bt.d_members = d_mem.data_ptr(); bt.n_members = n
    bt.d_dst = d_dst.data_ptr(); bt.dst_cap = do
    bt.d_results = d_res.data_ptr(); bt.d_summary = d_sum.data_ptr()
    bt.options = options
    gpu_ctx.gzip_decode(bt)
    gpu_ctx.sync()
    res = d_res.cpu().numpy().view(N.GZ_RESULT_DTYPE)
    dst = d_dst.cpu().numpy()
    sm = d_sum.cpu().numpy().view(N.SUMMARY_DTYPE)[0]
    untouched = np.ones(do, dtype=bool)
    out = []
    for i in range(n):
        st, ln, off, cap = int(res[i]["status"]), int(res[i]["out_len"]), int(mem[i]["dst_off"]), int(mem[i]["dst_cap"])
        assert ln <= cap, i
        untouched[off:off + cap] = False
        out.append((st, dst[off:off + ln].tobytes(), int(res[i]["consumed"]), int(res[i]["crc32"])))
    assert (dst[untouched] == GUARD).all(), "bytes outside the pieces' slots changed (options %d)" % options
    # a piece that ends where its stream goes on is not a bad unit
    assert int(sm["n_bad_units"]) == sum(1 for o in out if o[0] not in (ST_OK, ST_PIECE_END)), options
    return out


def by_all_paths(gpu_ctx, entries, extra=OPT_PIECES, **kw):
    norm = lambda rs: [(st, None, None, None) if st == ST_FULL else (st, out, cons if st in (ST_OK, ST_PIECE_END) else None,
                                                                     crc if st in (ST_OK, ST_PIECE_END) else None) for st, out, cons, crc in rs]
    first = None
    for opt, what in PATHS:
        got = run_table(gpu_ctx, entries, opt | extra, **kw)
        if first is None:
            first = got
        else:
            a, b = norm(first), norm(got)
            diff = [i for i in range(len(a)) if a[i] != b[i]]
            assert not diff, "wave-per-member and %s disagree at pieces %s: %r / %r" % (what, diff[:10], a[diff[0]][0], b[diff[0]][0])
    return first


def check_piece(name, got, status, plain, consumed=None):
    st, out, cons, crc = got
    assert st == status, (name, st, status)
    assert out == plain, (name, len(out), len(plain))
    if status in (ST_OK, ST_PIECE_END):
        assert crc == zlib.crc32(plain) & 0xFFFFFFFF, name
        assert cons == consumed, (name, cons, consumed)


@pytest.mark.parametrize("lead", [0, 1, 2, 3, 125, 126, 127, 128, 129])
def test_full_flush_pieces(gpu_ctx, text, full, lead):
    """the 12 pieces of the 240 KB stream, each alone, and the span behind the last marker (03 00)"""
    body, pieces, tail = full
    assert len(pieces) == 12 and body.count(MARKER) == 12 and tail == b"\x03\x00"
    entries = [(p, 20000 + 64) for p in pieces] + [(tail, 64), (pieces[-1] + tail, 20000)]
    got = by_all_paths(gpu_ctx, entries, lead=lead)
    for k, p in enumerate(pieces):
        assert p.endswith(MARKER) and zlib_piece(p) == text[k * 20000:(k + 1) * 20000]
        check_piece("piece %d" % k, got[k], ST_PIECE_END, text[k * 20000:(k + 1) * 20000], len(p))
    check_piece("last span", got[12], ST_OK, b"", 2)
    check_piece("piece 11 + last span", got[13], ST_OK, text[220000:], len(pieces[-1]) + 2)


def test_full_flush_tiny_and_empty_steps(gpu_ctx):
    """1-byte steps and 0-byte steps (a flush with nothing new writes nothing: three of them are one marker at most)"""
    plain = word_text(300, 3)
    body, pieces, tail = zlib_flushed(plain, 1, zlib.Z_FULL_FLUSH)
    ebody, epieces, etail = zlib_flushed(b"", 0, zlib.Z_FULL_FLUSH)
    spans = [p for p in pieces + epieces if p]
    entries = [(p, 64) for p in spans] + [(tail, 64), (ebody, 64)]
    got = by_all_paths(gpu_ctx, entries, pack=True)
    for k, p in enumerate(spans):
        check_piece("tiny %d" % k, got[k], ST_PIECE_END, zlib_piece(p), len(p))
    assert b"".join(g[1] for g in got[:len(pieces)]) == plain
    check_piece("tail", got[len(spans)], ST_OK, b"", len(tail))
    # the whole empty stream in one span: markers (if any), then the final block
    check_piece("empty stream", got[len(spans) + 1], ST_OK, b"", len(ebody))


def _aligned_block(kind, want_bits):
    """a non-final fixed / dynamic block of literals and matches whose last bit is bit `want_bits` (mod 8) of its byte"""
    for n in range(20, 400):
        # (bytes from 144 up are 9-bit literals in the fixed code: their number moves the end of the block by a bit each)
        ops = list(word_text(n, n)) + [B.M(7, 5), B.M(30, 12)] + [144 + n % 100] * (n % 9)
        blk = B.Fixed(ops, final=0) if kind == "fixed" else B._dyn_auto(ops, random.Random(n), final=0)
        image, plain, valid, _, info = B.build([blk])
        if valid and info["bits"] % 8 == want_bits:
            return image, plain
    raise AssertionError("no such block")


def _image(blocks):
    image, plain, valid, _, _ = B.build(blocks)
    assert valid
    return image, plain


def test_hand_built_piece_ends(gpu_ctx):
    data = bytes(range(256)) * 3
    cases = []      # (name, span, status, plain, consumed)
    for kind in ("fixed", "dynamic"):
        img, plain = _aligned_block(kind, 0)
        cases.append((kind + " block ends exactly on a byte, nothing behind", img, ST_PIECE_END, plain, len(img)))
        cases.append((kind + " on a byte, span one byte long", img + b"\x00", ST_TRUNC, plain, None))
        cases.append((kind + " on a byte, span one byte short", img[:-1], ST_TRUNC, None, None))
        img2, plain2 = _aligned_block(kind, 3)
        # five pad bits of zero behind the end-of-block code: a stored block's header whose LEN / NLEN are missing
        cases.append((kind + " block ends mid-byte at the end of the span", img2, ST_TRUNC, plain2, None))
    simg, splain = _image([B.Fixed(list(b"in front of the stored block "), final=0), B.Stored(data, final=0)])
    cases.append(("behind a stored block with data", simg, ST_PIECE_END, splain, len(simg)))
    eimg, eplain = _image([B.Fixed(list(b"sync flush"), final=0), B.Stored(b"", final=0)])
    assert eimg.endswith(MARKER)
    cases.append(("behind an empty stored block", eimg, ST_PIECE_END, eplain, len(eimg)))
    cases.append(("empty stored block, one byte short", eimg[:-1], ST_TRUNC, eplain, None))
    cases.append(("empty stored block, one byte long", eimg + b"\x00", ST_TRUNC, eplain, None))
    chunk = b"\x00" + len(data).to_bytes(2, "little") + (len(data) ^ 0xFFFF).to_bytes(2, "little") + data
    cases.append(("stored-only chunk (00 LEN NLEN data)", chunk, ST_PIECE_END, data, len(chunk)))
    cases.append(("stored-only chunk, one byte short", chunk[:-1], ST_TRUNC, data[:-1], None))
    cases.append(("two stored-only chunks", chunk + chunk, ST_PIECE_END, data + data, 2 * len(chunk)))
    cases.append(("marker alone", b"\x00" + MARKER, ST_PIECE_END, b"", 5))
    cases.append(("no block at all", b"", ST_TRUNC, b"", None))
    fimg, fplain = _image([B.Fixed(list(b"the stream ends here"), final=1)])
    cases.append(("a final block", fimg + b"trailing", ST_OK, fplain, len(fimg)))
    want = []
    for name, span, status, plain, cons in cases:
        # zlib's verdict on the same span: no end of stream for a piece end or a cut, the same bytes
        d = zlib.decompressobj(-15)
        out = d.decompress(span)
        assert d.eof == (status == ST_OK), name
        if plain is None:
            plain = out
        assert out == plain, name
        want.append((name, status, plain, cons))
    got = by_all_paths(gpu_ctx, [(c[1], len(c[3] or b"") + 512) for c in cases])
    for (name, status, plain, cons), g in zip(want, got):
        check_piece(name, g, status, plain, cons)


def test_sync_flush_pieces_need_history(gpu_ctx, text, sync):
    body, pieces, tail = sync
    assert len(pieces) == 12
    want = []
    for k, p in enumerate(pieces):
        if k == 0:
            want.append((ST_PIECE_END, zlib_piece(p)))
            continue
        with pytest.raises(zlib.error, match="invalid distance too far back"):
            zlib.decompressobj(-15).decompress(p)
        rc, cons, out = O.inflate_raw(p, 20000 + 64)
        assert rc == 2
        d, fed = zlib.decompressobj(-15), b""
        try:
            for i in range(len(p)):
                fed += d.decompress(p[i:i + 1])
        except zlib.error:
            pass
        out = bytes(out)
        assert out.startswith(fed)
        want.append((ST_NEEDS_HISTORY, out))
    entries = [(p, 20000 + 64) for p in pieces]
    got = by_all_paths(gpu_ctx, entries)
    for k, ((status, plain), g) in enumerate(zip(want, got)):
        check_piece("sync piece %d" % k, g, status, plain, len(pieces[k]))
        assert len(g[1]) == len(plain)
    # without the option the same spans are members of their own: zlib's "invalid distance too far back"
    got = by_all_paths(gpu_ctx, entries, extra=OPT_RAW)
    assert [g[0] for g in got] == [ST_TRUNC] + [ST_DATA] * 11
    assert [g[1] for g in got[1:]] == [w[1] for w in want[1:]]


@pytest.mark.parametrize("options", [0, 1], ids=["fixed", "dynamic"])
@pytest.mark.parametrize("chunk", [1, 4096, 49152])
def test_round_trip_of_the_stream_writer(gpu_ctx, options, chunk):
    """compress_to_stream -> piece index -> decode with LA_GZ_OPT_PIECES: the input again, and its CRC32 from the pieces'"""
    import torch
    from libarchive_amd import _native as N
    from libarchive_amd.gzip import compress_to_stream, decode_pieces, piece_index
    host = N.host_lib()
    host.la_crc32_combine.restype = N.C.c_uint32
    host.la_crc32_combine.argtypes = [N.C.c_uint32, N.C.c_uint32, N.C.c_uint64]
    size = 700 if chunk == 1 else 150001
    for what, plain in (("text", word_text(size, 11)), ("zeros", bytes(size)), ("random", random.Random(5).randbytes(size))):
        d_plain = torch.from_numpy(np.frombuffer(plain, dtype=np.uint8).copy()).cuda()
        body = compress_to_stream(gpu_ctx, d_plain, chunk, options).cpu().numpy().tobytes() + b"\x03\x00"
        assert zlib.decompress(body, -15) == plain
        idx = piece_index(body)
        assert idx.consumed == len(body) and idx.last_open
        d_src = torch.from_numpy(np.frombuffer(body + bytes(64), dtype=np.uint8).copy()).cuda()[:len(body)]
        for opt, path in PATHS + ((0, "default routing"),):
            plan, res = decode_pieces(gpu_ctx, d_src, idx, opt)
            dst = plan.d_dst.cpu().numpy()
            out, crc = [], 0
            for m, r in zip(idx.members, res):
                last = m is idx.members[-1] or int(m["src_off"]) + int(m["src_len"]) == len(body)
                assert int(r["status"]) == (ST_OK if last else ST_PIECE_END), (what, path, int(r["status"]))
                assert last or int(r["consumed"]) == int(m["src_len"])
                out.append(dst[int(m["dst_off"]):int(m["dst_off"]) + int(r["out_len"])].tobytes())
                crc = host.la_crc32_combine(crc, int(r["crc32"]), int(r["out_len"]))
            assert b"".join(out) == plain, (what, path)
            assert crc == zlib.crc32(plain) & 0xFFFFFFFF, (what, path)


def test_batch_size_routing(gpu_ctx):
    """8 192 tiny pieces and more go the two-phase way by default, 3 go the wave way: the per-phase profile names them"""
    spans = [zlib_flushed(word_text(40 + k % 7, k), 64, zlib.Z_FULL_FLUSH)[1][0] for k in range(64)]
    plains = [zlib_piece(s) for s in spans]
    for n, phases in ((8192 + 5, {"inflate_symbols", "inflate_expand"}), (3, {"inflate"})):
        gpu_ctx.profile_enable(True)
        got = run_table(gpu_ctx, [(spans[i % 64], 64) for i in range(n)], OPT_PIECES, pack=True)
        names = {name for name, ms in gpu_ctx.profile_read()}
        gpu_ctx.profile_enable(False)
        assert phases <= names and (n > 3 or "inflate_symbols" not in names), names
        for i, g in enumerate(got):
            check_piece("tiny piece %d of %d" % (i, n), g, ST_PIECE_END, plains[i % 64], len(spans[i % 64]))


def test_catalogue_without_the_option_is_unchanged(gpu_ctx):
    """the 439 hand-built streams as bare members WITHOUT LA_GZ_OPT_PIECES, through the template instances that replace
    the kernels of before: the statuses and bytes they had (tests/golden/deflate_handbuilt.json is zlib's word on them)"""
    import hashlib
    gold = {r["name"]: r for r in json.load(open(GOLDEN))}
    cases = [c for c in B.handbuilt_cases() if c.name in gold]
    assert len(cases) == 439
    got = by_all_paths(gpu_ctx, [(c.image, len(c.plain) if c.valid else 8192) for c in cases], extra=OPT_RAW, pack=True)
    for c, g in zip(cases, got):
        assert g[0] == c.status, c.name
        assert g[0] not in (ST_PIECE_END, ST_NEEDS_HISTORY)
        assert hashlib.sha256(g[1]).hexdigest() == gold[c.name]["plain_sha256"], c.name
