"""The device ABI of the xz kernels (la_xz.hip through la_gpu_xz_decode) against liblzma: Python's lzma for what a
block decodes to, the reference's read loop (xz_support.reference_read) for what is refused.  Blocks are handed over
with and without their sizes; the check field is verified in the same call."""
import hashlib
import lzma
import struct
import zlib

import numpy as np
import pytest

import xz_build as XB
import xz_support as XS

pytestmark = pytest.mark.gpu

OK, DATA, LZMA, TRUNCATED, SIZE, BAD_CHECK, PADDING, OUT_FULL = 0, 25, 26, 27, 28, 29, 30, 31


def one_block(gpu_ctx, raw, plain_len, cid=0, check=b"", sized=False, pad_byte=0, cap=None, dict_size=1 << 21, tail=b""):
    """raw + padding + check as the whole source; returns (status, bytes, consumed)"""
    from libarchive_amd import xz
    img = raw + bytes([pad_byte]) * (-len(raw) % 4) + check + tail
    e = {"src_off": 0, "dst_cap": plain_len if sized else (plain_len + 64 if cap is None else cap), "check_id": cid, "dict_size": dict_size}
    if sized:
        e.update(comp_size=len(raw), uncomp_size=plain_len, check_off=len(raw) + (-len(raw) % 4))
    res, plan = xz.decode_blocks(gpu_ctx, img, [e])
    r = res[0]
    assert int(r["valid"]) == int(r["out_len"])
    return int(r["status"]), plan.output(0), int(r["consumed"])


PROPS = [(0, 0, 0), (3, 0, 2), (4, 0, 0), (0, 4, 0), (0, 0, 4), (1, 3, 2)]


@pytest.mark.parametrize("props", PROPS, ids=["lc%d_lp%d_pb%d" % p for p in PROPS])
def test_properties(gpu_ctx, props):
    """streams of 1 .. 3000 bytes under every corner of lc / lp / pb, all in ONE call: one block each"""
    from libarchive_amd import xz
    lc, lp, pb = props
    sizes = [1, 2, 3, 7, 64, 65, 255, 1000, 2999, 3000]
    plains = [XS.text(n, n) if n % 2 else XS.noise(n, n, 6) for n in sizes]
    raws = [XB.lzma2(p, lc, lp, pb) for p in plains]
    src, entries, off, dst = b"", [], 0, 0
    for p, raw in zip(plains, raws):
        assert lzma.decompress(raw, format=lzma.FORMAT_RAW, filters=[{"id": lzma.FILTER_LZMA2}]) == p
        blob = raw + bytes(-len(raw) % 4) + struct.pack("<Q", XB.crc64(p))
        entries.append({"src_off": off, "comp_size": len(raw), "uncomp_size": len(p), "dst_off": dst, "dst_cap": len(p), "check_id": 4,
                        "check_off": off + len(raw) + (-len(raw) % 4)})
        src, off, dst = src + blob, off + len(blob), dst + len(p)
    res, plan = xz.decode_blocks(gpu_ctx, src, entries)
    assert [int(s) for s in res["status"]] == [OK] * len(sizes)
    assert [int(c) for c in res["consumed"]] == [len(r) for r in raws]
    assert plan.output() == b"".join(plains)


@pytest.mark.parametrize("name", sorted(XS.packet_cases()) + sorted(XS.chunk_plans()))
def test_hand_built(gpu_ctx, name):
    raw, plain = {**XS.packet_cases(), **XS.chunk_plans()}[name]
    for sized in (False, True):
        st, out, consumed = one_block(gpu_ctx, raw, len(plain), 1, struct.pack("<I", zlib.crc32(plain)), sized=sized)
        assert (st, consumed) == (OK, len(raw)), (name, sized)
        assert out == plain


@pytest.mark.parametrize("name", sorted(XS.beyond_cases()))
def test_distance_beyond_the_data(gpu_ctx, name):
    raw, valid, ok, dict_byte = XS.beyond_cases()[name]
    assert (XS.reference_read(XS.wrap(raw, valid if ok else b"", dict_byte=dict_byte))[1] == 0) == ok
    st, out, _ = one_block(gpu_ctx, raw, len(valid) + 300, dict_size=4096 if dict_byte == 0 else 1 << 21)
    assert st == (OK if ok else LZMA) and out == valid


@pytest.mark.parametrize("name", sorted(XS.refusals()))
def test_lzma2_refusals(gpu_ctx, name):
    raw, built_from = XS.refusals()[name]
    assert XS.reference_read(XS.wrap(raw)) == (b"", -30, XS.DATA_ERROR)
    st, out, _ = one_block(gpu_ctx, raw, 300)
    # a range decoder that asks for bytes behind the chunk's compressed size is refused inside the chunk, the rest at its ends
    assert st == (LZMA if name in ("compressed_size_one_less", "uncompressed_size_one_more") else DATA), st
    assert built_from[:len(out)] == out
    want = {"uncompressed_size_one_less": len(built_from) - 1, "compressed_size_one_more": len(built_from), "match_over_the_chunk_end": 21}
    assert len(out) == want.get(name, len(out))


def test_checks(gpu_ctx):
    p = XS.text(11, 70001)
    raw = XB.lzma2(p)
    good = {0: b"", 1: struct.pack("<I", zlib.crc32(p)), 4: struct.pack("<Q", XB.crc64(p)), 10: hashlib.sha256(p).digest(), 2: b"abcd", 15: bytes(64)}
    for cid, chk in good.items():
        for sized in (False, True):
            assert one_block(gpu_ctx, raw, len(p), cid, chk, sized=sized)[::2] == (OK, len(raw)), cid
    for cid in (1, 4, 10):
        bad = bytearray(good[cid])
        bad[-1] ^= 1
        st, out, _ = one_block(gpu_ctx, raw, len(p), cid, bytes(bad))
        assert st == BAD_CHECK and out == p
        assert one_block(gpu_ctx, raw, len(p), cid, good[cid][:-1])[0] == TRUNCATED
    for n in (0, 1, 63, 64, 65, 4095, 4097):     # CRC64 segments: fewer bytes than lanes, an uneven last segment
        q = p[:n]
        r = XB.lzma2(q) if n else b"\x00"
        assert one_block(gpu_ctx, r, n, 4, struct.pack("<Q", XB.crc64(q)))[0] == OK, n
        assert one_block(gpu_ctx, r, n, 10, hashlib.sha256(q).digest())[0] == OK, n
    raw3 = XB.lzma2(p[:70000])
    assert len(raw3) % 4
    assert one_block(gpu_ctx, raw3, 70000, 1, struct.pack("<I", zlib.crc32(p[:70000])), pad_byte=1)[0] == PADDING


def test_bounds_and_sizes(gpu_ctx):
    from libarchive_amd import xz
    p = XS.text(12, 5000)
    raw = XB.lzma2(p)
    st, out, _ = one_block(gpu_ctx, raw, len(p), cap=1234)
    assert st == OUT_FULL and out == p[:1234]
    for cut in (0, 1, 5, 6, 7, 100, len(raw) - 1):
        res, plan = xz.decode_blocks(gpu_ctx, raw[:cut], [{"src_off": 0, "dst_cap": 6000}])
        assert int(res[0]["status"]) == TRUNCATED and p.startswith(plan.output(0)), cut
    for field, delta in (("comp_size", -4), ("comp_size", 4), ("uncomp_size", -1), ("uncomp_size", 1)):
        e = {"src_off": 0, "comp_size": len(raw), "uncomp_size": len(p), "dst_cap": len(p) + 1}
        e[field] += delta
        res, _ = xz.decode_blocks(gpu_ctx, raw + bytes(8), [e])
        assert int(res[0]["status"]) == SIZE, (field, delta)
    # table entries that point outside the buffers are not decoded
    res, _ = xz.decode_blocks(gpu_ctx, raw, [{"src_off": len(raw) + 1, "dst_cap": 10}])
    assert int(res[0]["status"]) == SIZE
    plan = xz.XzDevicePlan(gpu_ctx, plan.d_src, xz.block_table([{"src_off": 0, "dst_off": 10, "dst_cap": 6000}]), dst_cap=100).run()
    assert int(plan.results()[0]["status"]) == SIZE


def test_many_blocks_in_one_call(gpu_ctx):
    """300 blocks of 1 .. 900 bytes, sized and size-less mixed, with the four checks, packed output"""
    from libarchive_amd import xz
    src, entries, want, dst = b"", [], [], 0
    for i in range(300):
        p = XS.text(i, 1 + (i * 37) % 900)
        raw = XB.lzma2(p)
        cid = (0, 1, 4, 10)[i % 4]
        blob = raw + bytes(-len(raw) % 4) + XB.check_value(cid, p)
        e = {"src_off": len(src), "dst_off": dst, "dst_cap": len(p), "check_id": cid}
        if i % 3:
            e.update(comp_size=len(raw), uncomp_size=len(p))
        entries.append(e)
        src, dst = src + blob, dst + len(p)
        want.append(p)
    res, plan = xz.decode_blocks(gpu_ctx, src, entries)
    assert (res["status"] == OK).all() and plan.output() == b"".join(want)
    assert np.array_equal(res["out_len"], np.array([len(p) for p in want], dtype=np.uint64))
