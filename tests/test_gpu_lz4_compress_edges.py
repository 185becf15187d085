"""The device LZ4 compressor (la_lz4_comp.hip) at the block format's edges.  LZ4_decompress_safe is lenient about
the end-of-block rules, so they are checked here on the block as written, through the plain reader
streams.lz4_parse_block: in every compressed (not stored) block the last sequence is literals only and at least five
of them, the last match starts at least twelve bytes before the block's end, every offset reaches produced bytes,
and re-executing the sequences gives the input.  The inputs are every small length and every length up to a full
64 KiB block of texts in which an unrestricted match would run into the last bytes, and crafted blocks whose literal
and match lengths sit on the steps of the length extension (zstd_edge_inputs.py).  Each test ends with a census read
from the parsed blocks alone."""
import ctypes as C
import random

import numpy as np
import pytest

import oracle_lib as O
import streams as S
import zstd_edge_inputs as E
from test_gpu_lz4 import gpu_decode

pytestmark = pytest.mark.gpu

DEVICE_DECODER = True       # (False on the bench: a compressor broken on purpose is judged by the host-side readers alone)


def _liblz4():
    try:
        lz = C.CDLL("liblz4.so.1")
    except OSError:
        pytest.fail("no liblz4.so.1 in this image")
    lz.LZ4_decompress_safe.argtypes = [C.c_char_p, C.c_char_p, C.c_int, C.c_int]
    return lz


def compress_blocks(gpu_ctx, data, bs=65536, bpf=4, flags=3):
    """(image, [(input bytes of the block, payload, stored)])"""
    import torch
    from libarchive_amd import _native as N
    from libarchive_amd.lz4 import compress_to_frames
    d = torch.from_numpy(np.frombuffer(data, dtype=np.uint8).copy()).cuda() if data else torch.zeros(0, dtype=torch.uint8, device="cuda")
    img = compress_to_frames(gpu_ctx, d, bs, bpf, flags).cpu().numpy()
    if not data:
        return img, []
    idx, raw = N.lz4_index(img), img.tobytes()
    assert len(idx.blocks) == (len(data) + bs - 1) // bs
    return img, [(data[k * bs:(k + 1) * bs], raw[int(b["src_off"]):int(b["src_off"]) + int(b["src_len"])], bool(int(b["flags"]) & N.LA_LZ4B_STORED))
                 for k, b in enumerate(idx.blocks)]


def check_block(lz, want, payload, stored):
    """the rules on one block as written; returns (sequences, extensions, start of the last match, its end) or None"""
    if stored:
        assert payload == want
        return None
    buf = C.create_string_buffer(len(want) + 1)
    assert lz.LZ4_decompress_safe(payload, buf, len(payload), len(want)) == len(want) and buf.raw[:len(want)] == want
    seqs, exts = S.lz4_parse_block(payload)
    assert S.lz4_execute(seqs) == want, "re-executing the sequences does not give the input"
    n = len(want)
    assert seqs[-1][1:] == (0, 0) and len(seqs[-1][0]) >= 5, "last sequence: %d literals, match %s (block of %d)" % (len(seqs[-1][0]), seqs[-1][1:], n)
    pos, start, end = 0, None, None
    for lit, off, ml in seqs[:-1]:
        pos += len(lit)
        assert 1 <= off <= pos, "offset %d at %d" % (off, pos)
        start, pos = pos, pos + ml
        end = pos
    if start is not None:
        assert start <= n - 12, "the last match starts %d bytes before the end of a block of %d" % (n - start, n)
        assert end <= n - 5
    return seqs, exts, start, end


# ---------------------------------------------------------------- every length
def _sweep_texts():
    """name -> function of the length"""
    rnd = random.Random(0x1E4)
    base = bytearray()
    E.Fresh(rnd).extend(base, 65536)
    base = bytes(base)

    def tail_repeat(k):
        def make(n):
            if n < 2 * k + 2:
                return base[:n]
            s = 0 if n < k + 250 else n - k - 150       # a source the table still holds: near, or position 0
            head = bytearray(base[:n - k])
            if n >= 140:                                # an early repeat, so that the block compresses whatever its end does
                head[70:100] = head[1:31]
            if head[-1] == head[s - 1] and s > 0:
                head[-1] ^= 0x55
            return bytes(head) + bytes(head[s:s + k])
        return make
    return {"zeros": lambda n: bytes(n), "period2": lambda n: (b"ab" * n)[:n], "period5": lambda n: (b"abcde" * n)[:n],
            "tail16": tail_repeat(16), "tail12": tail_repeat(12), "tail11": tail_repeat(11)}


LENGTHS = list(range(0, 201)) + list(range(65524, 65537))


def test_end_of_block_rules_at_every_length(gpu_ctx):
    lz = _liblz4()
    seen = {"compressed": 0, "stored": 0, "last literals 5": 0, "last match ends 5 before the end": 0, "last match starts 12 before the end": 0,
            "11 repeated bytes before the end left as literals": 0}
    for name, make in sorted(_sweep_texts().items()):
        for n in LENGTHS:
            data = make(n)
            assert len(data) == n
            img, blocks = compress_blocks(gpu_ctx, data, 65536, 1, 3)
            out, res = O.lz4_stream_decode(img, n + 64)
            assert (res.rc, res.errmsg) == (0, b"") and out.tobytes() == data, (name, n)
            for want, payload, stored in blocks:
                try:
                    r = check_block(lz, want, payload, stored)
                except AssertionError as e:
                    raise AssertionError("%s, length %d: %s" % (name, n, e))
                seen["stored" if r is None else "compressed"] += 1
                if r is None or r[2] is None:
                    continue
                seqs, _, start, end = r
                seen["last literals 5"] += len(seqs[-1][0]) == 5
                seen["last match ends 5 before the end"] += end == n - 5
                seen["last match starts 12 before the end"] += start == n - 12
                seen["11 repeated bytes before the end left as literals"] += name == "tail11" and n - end >= 11
    missing = ["%s: never seen" % k for k, v in sorted(seen.items()) if not v]
    assert not missing, "census: " + "; ".join(missing)


# ---------------------------------------------------------------- length extensions
LIT_LENGTHS = [14, 15, 269, 270, 525, 16335]
MATCH_LENGTHS = [4 + 14, 4 + 15, 4 + 270, 4 + 15 + 255 * 65, 4 + 16400]


def _crafted():
    rnd = random.Random(0x124C)
    return E.pack_pairs(rnd, LIT_LENGTHS, MATCH_LENGTHS, 65536)


def extension_census(records):
    """records: [(literal bytes, match length, (literal extension), (match extension))]"""
    missing = []
    for what, k in (("literal", 2), ("match", 3)):
        ext = [r[k] for r in records]
        for n in (0, 1, 2):
            if not any(e[0] == n for e in ext):
                missing.append("%s length with %d extension bytes not seen" % (what, n))
        if not any(e[0] > 64 for e in ext):
            missing.append("%s length with more than 64 extension bytes not seen" % what)
        for n, label in ((1, "1"), (2, "2")):
            if not any(e[0] == n and e[1] == 0 for e in ext):
                missing.append("%s length with %s extension bytes, the last 0, not seen" % (what, label))
        if not any(e[0] > 64 and e[1] == 0 for e in ext):
            missing.append("%s length with more than 64 extension bytes, the last 0, not seen" % what)
    lits, mls = {len(r[0]) for r in records}, {r[1] - 4 for r in records}
    missing += ["literal length %d not seen" % v for v in LIT_LENGTHS if v not in lits]
    missing += ["match length 4 + %d not seen" % (v - 4) for v in MATCH_LENGTHS[:4] if v - 4 not in mls]
    if not any(v > 16335 for v in mls):
        missing.append("match length above 4 + 16335 not seen")
    return missing


def test_length_extension_steps(gpu_ctx):
    lz = _liblz4()
    blocks_in = _crafted()
    data = b"".join(blocks_in)
    records = []
    for bs, bpf, flags in ((65536, 16, 3), (65536, 1, 0)):
        img, blocks = compress_blocks(gpu_ctx, data, bs, bpf, flags)
        out, res = O.lz4_stream_decode(img, len(data) + 64)
        assert (res.rc, res.errmsg) == (0, b"") and out.tobytes() == data
        if DEVICE_DECODER:
            got, rc, msg = gpu_decode(gpu_ctx, img)
            assert (rc, msg) == (0, "") and got == data
        for want, payload, stored in blocks:
            assert not stored, "a crafted block did not compress"
            seqs, exts, _, _ = check_block(lz, want, payload, stored)
            records += [(lit, ml, le, me) for (lit, off, ml), (le, me) in zip(seqs, exts)]
    missing = extension_census(records)
    assert not missing, "census: " + "; ".join(missing)
