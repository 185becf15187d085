"""CPU-only: the host side of piece mode against libla_host -- the walker that cuts one member's body at its flush
markers (la_gz_pieces_build, la_gzip_index.c) and the bid rule behind LA_GZIP_FLUSH_POINTS=1 (la_bid_policy.c).

Checked here with zlib: 240 KB of word text through compressobj(6, DEFLATED, -15) in 20 000-byte steps gives, with
Z_FULL_FLUSH, 12 pieces that each end in 00 00 FF FF and decode alone to their slice (the body holds exactly 12 markers);
with Z_SYNC_FLUSH, pieces 1 to 11 each fail alone with "invalid distance too far back"."""
import ctypes as C
import os
import random
import subprocess
import zlib

import numpy as np
import pytest

import streams as S
from libarchive_amd import _native as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MARKER = b"\x00\x00\xff\xff"
WORDS = [b"window", b"piece", b"flush", b"marker", b"deflate", b"stored", b"lane", b"wave", b"boundary", b"history", b"the", b"of"]
LA_END_EOF, LA_END_NEED_MORE = 0, 5


def word_text(n, seed=7):
    r = random.Random(seed)
    return b" ".join(r.choice(WORDS) for _ in range(n // 4))[:n]


def flushed(plain, flush, step=20000):
    c = zlib.compressobj(6, zlib.DEFLATED, -15)
    pieces = [c.compress(plain[i:i + step]) + c.flush(flush) for i in range(0, len(plain), step)]
    return pieces, c.flush()


TEXT = word_text(240000)


def slot_rule(n):
    return min(n * 1032 + 64, max(65536, 8 * n))


def test_zlib_facts():
    pieces, tail = flushed(TEXT, zlib.Z_FULL_FLUSH)
    assert len(pieces) == 12 and b"".join(pieces).count(MARKER) == 12 and tail == b"\x03\x00"
    for k, p in enumerate(pieces):
        d = zlib.decompressobj(-15)
        assert p.endswith(MARKER) and d.decompress(p) == TEXT[k * 20000:(k + 1) * 20000] and not d.eof and d.unused_data == b""
    pieces, tail = flushed(TEXT, zlib.Z_SYNC_FLUSH)
    for p in pieces[1:]:
        with pytest.raises(zlib.error, match="invalid distance too far back"):
            zlib.decompressobj(-15).decompress(p)


@pytest.mark.parametrize("flush", [zlib.Z_FULL_FLUSH, zlib.Z_SYNC_FLUSH], ids=["full", "sync"])
def test_piece_table(flush):
    """the markers are the same bytes whatever the flush: the same table shape for both streams"""
    pieces, tail = flushed(TEXT, flush)
    header = b"\x1f\x8b\x08\x00\x00\x00\x00\x00\x00\x03"
    img = header + b"".join(pieces) + tail + bytes(8)
    # at end of input: 12 pieces and the last span (final block + trailer)
    x = N.gz_pieces(img, len(header), at_eof=True)
    assert len(x.members) == 13 and x.last_open and x.end_kind == LA_END_EOF and x.consumed == len(img)
    off, dst = len(header), 0
    for m, p in zip(x.members, pieces + [tail + bytes(8)]):
        assert (int(m["src_off"]), int(m["src_len"]), int(m["dst_cap"]), int(m["dst_off"])) == (off, len(p), slot_rule(len(p)), dst)
        off += len(p)
        dst += (slot_rule(len(p)) + 15) & ~15
    assert x.max_out == dst
    # more input may follow: the last span is held back, its bytes are the next window's
    x = N.gz_pieces(img, len(header), at_eof=False)
    assert len(x.members) == 12 and not x.last_open and x.end_kind == LA_END_NEED_MORE
    assert x.consumed == len(header) + sum(len(p) for p in pieces)
    # a window that ends exactly behind a marker, at end of input: no empty last span
    cut = img[:x.consumed]
    y = N.gz_pieces(cut, len(header), at_eof=True)
    assert len(y.members) == 12 and not y.last_open and y.end_kind == LA_END_EOF and y.consumed == len(cut)
    # budget: stop in front of the piece that would pass it, one piece at least
    for budget, want in ((1, 1), (65536, 1), (65537, 2), (5 * 65536, 5), (1 << 30, 13)):
        z = N.gz_pieces(img, len(header), at_eof=True, out_budget=budget)
        assert len(z.members) == want, budget
        assert z.end_kind == (LA_END_EOF if want == 13 else LA_END_NEED_MORE)
        assert z.consumed == len(header) + sum(len(p) for p in (pieces + [tail + bytes(8)])[:want])
    # a refuted first marker merges pieces 0 and 1; a larger minimum slot holds for every piece it can apply to
    z = N.gz_pieces(img, len(header), at_eof=True, first_skip=1, min_cap=200000)
    assert len(z.members) == 12 and int(z.members[0]["src_len"]) == len(pieces[0]) + len(pieces[1])
    assert int(z.members[0]["dst_cap"]) == 200000 and int(z.members[1]["dst_cap"]) == 200000
    assert int(z.members[-1]["dst_cap"]) == 10 * 1032 + 64      # (ten bytes cannot make more)
    # nothing behind `start`
    e = N.gz_pieces(img, len(img), at_eof=True)
    assert len(e.members) == 0 and e.end_kind == LA_END_EOF
    e = N.gz_pieces(img[:len(header) + 100], len(header), at_eof=False)
    assert len(e.members) == 0 and e.end_kind == LA_END_NEED_MORE and e.consumed == len(header)


def test_marker_inside_stored_data_is_one_more_candidate():
    noise = random.Random(1).randbytes(3000)
    c = zlib.compressobj(0, zlib.DEFLATED, -15)
    body = c.compress(noise[:1000] + MARKER + noise[1000:]) + c.flush(zlib.Z_FULL_FLUSH)
    assert body.count(MARKER) == 2
    x = N.gz_pieces(body + b"\x03\x00", 0, at_eof=True)
    assert len(x.members) == 3
    assert int(x.members[0]["src_len"]) == body.index(MARKER) + 4
    assert int(x.members[0]["src_len"]) + int(x.members[1]["src_len"]) == len(body)
    # overlapping and adjacent candidates, a marker at offset 0 and one cut by the end
    odd = MARKER + b"\x00" + MARKER + MARKER + b"\x00\x00\x00\xff\xff" + b"\x00\x00\xff"
    x = N.gz_pieces(odd, 0, at_eof=True)
    assert [int(m["src_len"]) for m in x.members] == [4, 5, 4, 5, 3]


def _bid(stream, hdr_len=10, lookahead=256 << 10):
    lib = N.host_lib()
    lib.la_bid_gzip_parallel.argtypes = [C.c_char_p, C.c_size_t, C.c_size_t, C.c_size_t]
    return lib.la_bid_gzip_parallel(stream, len(stream), hdr_len, lookahead)


def _stored_stream(gaps):
    """a header, then random bytes (which hold no marker) with a marker behind each gap, then filler up to the look-ahead"""
    rnd = random.Random(3)
    body = b""
    for g in gaps:
        chunk = rnd.randbytes(g).replace(b"\xff\xff", b"\xff\xfe").replace(b"\x1f\x8b", b"\x1f\x8c")
        body += chunk[:g] + MARKER
    fill = rnd.randbytes(300 << 10).replace(b"\xff\xff", b"\xff\xfe").replace(b"\x1f\x8b", b"\x1f\x8c")
    return b"\x1f\x8b\x08\x00\x00\x00\x00\x00\x00\x03" + body + fill


def test_bid_rule(monkeypatch):
    four = _stored_stream([40000, 40000, 40000, 40000])
    three = _stored_stream([40000, 40000, 40000])
    wide = _stored_stream([30000, 200 << 10, 30000, 30000])
    first_gap = _stored_stream([129 << 10, 1000, 1000, 1000])
    edge = _stored_stream([128 << 10, 1000, 1000, 1000])
    short = four[:100000]
    for s in (four, three, first_gap, edge):
        assert len(s) >= 256 << 10
    monkeypatch.delenv("LA_GZIP_FLUSH_POINTS", raising=False)
    assert [_bid(s[:256 << 10]) for s in (four, three, first_gap, edge)] == [0, 0, 0, 0]
    assert _bid(wide[:512 << 10], lookahead=512 << 10) == 0
    assert _bid(short) == 1          # shorter than the look-ahead: small, taken as always
    monkeypatch.setenv("LA_GZIP_FLUSH_POINTS", "0")
    assert _bid(four[:256 << 10]) == 0
    monkeypatch.setenv("LA_GZIP_FLUSH_POINTS", "1")
    assert _bid(four[:256 << 10]) == 1
    assert _bid(three[:256 << 10]) == 0
    assert _bid(wide[:512 << 10], lookahead=512 << 10) == 0      # four markers, one gap of 200 KiB
    assert _bid(first_gap[:256 << 10]) == 0 and _bid(edge[:256 << 10]) == 1
    assert _bid(short) == 1


def test_switch_off_changes_nothing(monkeypatch):
    """the member walker and the bid answers on the streams of tests/streams.py, with the switch unset, off and on:
    the member walker does not know the switch, and on these streams (many members, or shorter than the look-ahead,
    or without four markers) the bid is today's either way"""
    rnd = random.Random(9)
    plains = [rnd.randbytes(3000), b"abc" * 5000, b""]
    imgs = [b"".join(S.gz_member(p) for p in plains), S.gz_member(plains[0], name=b"one"), S.gz_member(rnd.randbytes(400000), level=1),
            b"".join(S.gz_member(p, extra=b"xx\x02\x00ab") for p in plains)]
    seen = []
    for value in (None, "0", "1"):
        if value is None:
            monkeypatch.delenv("LA_GZIP_FLUSH_POINTS", raising=False)
        else:
            monkeypatch.setenv("LA_GZIP_FLUSH_POINTS", value)
        row = []
        for img in imgs:
            x = N.gz_index(img)
            row.append((x.members.tobytes(), x.headers.tobytes(), x.end_kind, x.consumed, x.max_out, x.speculative,
                        _bid(img, lookahead=256 << 10), _bid(img, lookahead=1024)))
        seen.append(row)
    assert seen[0] == seen[1] == seen[2]


DRIVER = r"""
#include "la_host.h"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
int main(int argc, char **argv)
{
	FILE *f = fopen(argv[1], "rb");
	if (argc < 2 || !f) return 2;
	static uint8_t all[1 << 20];
	const size_t n = fread(all, 1, sizeof(all), f);
	fclose(f);
	unsigned long pieces = 0;
	for (size_t len = 0; len <= n; len++) {
		/* an exact-size heap copy per prefix: one byte read past the window is an error the sanitizer sees */
		uint8_t *w = malloc(len ? len : 1);
		memcpy(w, all, len);
		for (int eof = 0; eof < 2; eof++)
			for (uint32_t skip = 0; skip < 3; skip++) {
				la_gz_pieces x;
				const uint64_t from = len > 10 ? (skip ? len / 3 : 10) : 0;
				if (la_gz_pieces_build(w, len, from, eof, skip, skip * 70000u, skip == 2 ? 100000 : 0, LA_GZ_SPAN_LIMIT, &x) != 0)
					return 3;
				uint64_t at = from < len ? from : len;
				for (uint32_t i = 0; i < x.n; i++) {
					if (x.pieces[i].src_off != at || x.pieces[i].src_len == 0 || at + x.pieces[i].src_len > len)
						return 4;
					at += x.pieces[i].src_len;
				}
				if (at != x.consumed || (eof && skip != 2 && x.consumed != len))
					return 5;
				pieces += x.n;
				la_gz_pieces_free(&x);
			}
		if (la_gz_next_marker(w, len, len / 2) > len)
			return 6;
		free(w);
	}
	printf("%lu\n", pieces);
	return 0;
}
"""


def test_walker_over_every_prefix_under_sanitizers(tmp_path):
    """a stand-alone program with its own main, built with -fsanitize=address,undefined, drives the walker over every
    byte-prefix of one stream (header, full-flush pieces of text and of stored noise with markers inside, final block)"""
    noise = random.Random(2).randbytes(1500)
    c = zlib.compressobj(6, zlib.DEFLATED, -15)
    body = b"".join(c.compress(TEXT[i:i + 700]) + c.flush(zlib.Z_FULL_FLUSH) for i in range(0, 7000, 700))
    c0 = zlib.compressobj(0, zlib.DEFLATED, -15)
    body += c0.compress(noise[:500] + MARKER + noise[500:] + MARKER) + c0.flush(zlib.Z_FULL_FLUSH) + b"\x03\x00"
    stream = b"\x1f\x8b\x08\x00\x00\x00\x00\x00\x00\x03" + body + bytes(8)
    (tmp_path / "stream.bin").write_bytes(stream)
    (tmp_path / "driver.c").write_text(DRIVER)
    exe = str(tmp_path / "driver")
    subprocess.check_call(["gcc", "-O1", "-g", "-std=gnu11", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I" + os.path.join(ROOT, "include"), "-o", exe, str(tmp_path / "driver.c"),
                           os.path.join(ROOT, "libarchive_amd", "host", "la_gzip_index.c")])
    for env_extra in ({}, {"LA_NO_AVX2": "1"}):
        out = subprocess.run([exe, str(tmp_path / "stream.bin")], capture_output=True, text=True, env=dict(os.environ, **env_extra))
        assert out.returncode == 0, out.stderr[-2000:]
        assert int(out.stdout) > len(stream)
