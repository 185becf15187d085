"""The device ABI of the lzip kernels (la_lzip.hip through la_gpu_lzip_scan / la_gpu_lzip_decode) against liblzma's raw
LZMA1 decoder (lzip_support.expected_stream_result), Python's lzma, and the CPU stand-in that compiles the same rules
headers (tests/mock_gpu/la_gpu_lzip_mock.c): status, bytes, consumed and CRC32 per member."""
import ctypes as C
import random
import zlib

import pytest

import lzip_support as LS
import mock_build

pytestmark = pytest.mark.gpu

TILE = 4096


@pytest.fixture(scope="module")
def mock():
    return C.CDLL(mock_build.rules("liblzip_rules.so"))


def host_scan(buf):
    return [i for i in range(len(buf) - 5) if LS.has_member(buf[i:i + 6])]


def plant(buf, at, shape=b"LZIP\x01\x14"):
    buf[at:at + len(shape)] = shape


def test_scan_positions(gpu_ctx):
    """shapes at offset 0, in the last six bytes, across every kind of edge (a thread's 16 bytes, a tile of 4096),
    overlapping, and shapes with a bad version or dictionary byte"""
    from libarchive_amd import lzip
    n = 3 * TILE + 1000 + 7
    buf = bytearray(LS.noise(1, n, 200))
    spots = [0, 11, 27, 100, TILE - 12, TILE - 5, TILE + 1, 2 * TILE - 1, 2 * TILE + 13, 3 * TILE - 3, 3 * TILE + 990, n - 6]
    for k, at in enumerate(spots):        # (11 and 27 straddle a thread's 16 bytes, TILE - 5, 2 * TILE - 1 and 3 * TILE - 3 a tile)
        plant(buf, at, b"LZIP" + bytes([k & 1, 12 + k % 18 + (k % 8) * 32]))
    plant(buf, 300, b"LZIPLZIP\x01\x0c")
    plant(buf, 400, b"LZIP\x02\x14")
    plant(buf, 420, b"LZIP\x01\x0b")
    plant(buf, 440, b"LZIP\x01\x1e")
    plant(buf, 460, b"LZIP\x00\x3d")
    want = host_scan(bytes(buf))
    assert set(spots) | {304, 460} <= set(want) and not {300, 400, 420, 440} & set(want)
    d = lzip.to_device(buf)
    offs, count = lzip.scan(gpu_ctx, d)
    assert count == len(want) and [int(o) for o in offs] == want
    for m in (0, 5, 6, 7, 16, 17, 33, TILE, TILE + 1, TILE + 6, TILE + 7, 2 * TILE + 4, 2 * TILE + 5, n - 1):      # every prefix as its own source
        offs, count = lzip.scan(gpu_ctx, d, n=m)
        assert [int(o) for o in offs] == host_scan(bytes(buf[:m])) and count == len(offs), m


def test_scan_more_candidates_than_the_table_holds(gpu_ctx):
    from libarchive_amd import lzip
    buf = b"LZIP\x01\x14" * 3000 + b"LZ"
    d = lzip.to_device(buf)
    offs, count = lzip.scan(gpu_ctx, d, cap=1000)
    assert count == 3000 and [int(o) for o in offs] == [6 * i for i in range(1000)]
    offs, count = lzip.scan(gpu_ctx, d, cap=0)
    assert count == 3000 and len(offs) == 0


def name_of(status):
    from libarchive_amd import lzip
    return lzip.STATUS[int(status)]


def against_the_mock(mock, src, entries, res, plan, dst_cap):
    from libarchive_amd import lzip
    tab = lzip.member_table(entries)
    members = [LS.Member(*[int(x) for x in row]) for row in tab]
    for i, (r, out) in enumerate(LS.mock_decode(mock, src, members, dst_cap)):
        assert (int(res[i]["status"]), int(res[i]["out_len"]), int(res[i]["valid"]), int(res[i]["crc32"])) == (r.status, r.out_len, r.valid, r.crc32), i
        if r.status == 0:
            assert int(res[i]["consumed"]) == r.consumed, i
        assert plan.output(i) == out, i


def test_hand_built_streams(gpu_ctx, mock):
    """every hand-built stream in ONE call, both ends unknown, at a roomy budget and at the exact one"""
    from libarchive_amd import lzip
    cases = sorted(LS.stream_cases().items())
    src, entries, expect, off, dst = b"", [], [], 0, 0
    for name, (raw, db) in cases:
        plain = LS.liblzma_raw(raw, db)[0]
        for cap in (len(plain) + 64, len(plain)):
            exp = LS.expected_stream_result(raw, db, cap)
            # the source ends with the stream: a cut stream has to run into the end of the source, not into the next stream
            entries.append({"src_off": off, "dst_off": dst, "dst_cap": cap, "dict_size": LS.dict_size(db), "src_end": off + len(raw)})
            expect.append((name, cap, exp, len(plain)))
            dst += cap
        src, off = src + raw, off + len(raw)
    res, plan = lzip.decode_members(gpu_ctx, src, entries)
    for i, (name, cap, exp, n) in enumerate(expect):
        st = name_of(res[i]["status"])
        want = {"TRUNCATED": "SRC_END"}.get(exp[0], exp[0])
        if exp[0] == "OK" and exp[2] != len(LS.stream_cases()[name][0]):
            want = "EARLY_END"      # (bytes behind the marker)
        if cap == n and exp[0] == "TRUNCATED":
            assert st in ("SRC_END", "OUT_FULL"), (name, cap, st)
        else:
            assert st == want, (name, cap, st, want)
        assert plan.output(i) == exp[1], (name, cap)
    against_the_mock(mock, src, entries, res, plan, dst)


def test_member_sizes_and_many_members_in_one_call(gpu_ctx, mock):
    """members of 0, 1 and 65537 bytes and 300 members of 1 .. 4 KiB, all with their trailers' end, size and CRC"""
    from libarchive_amd import lzip
    r = random.Random(5)
    plains = [b"", b"x", LS.text(3, 65537)] + [LS.text(100 + i, r.randrange(1024, 4097)) if i % 3 else LS.noise(100 + i, r.randrange(1024, 4097), 40)
                                               for i in range(300)]
    src, entries, dst = b"", [], 0
    for p in plains:
        m = LS.member(p, preset=1)
        entries.append({"src_off": len(src) + 6, "src_end": len(src) + len(m) - 20, "data_size": len(p), "dst_off": dst, "dst_cap": len(p),
                        "crc32": zlib.crc32(p)})
        src, dst = src + m, dst + len(p)
    res, plan = lzip.decode_members(gpu_ctx, src, entries)
    assert [name_of(s) for s in res["status"]] == ["OK"] * len(plains)
    assert plan.output() == b"".join(plains)
    assert [int(c) for c in res["crc32"]] == [zlib.crc32(p) for p in plains]
    against_the_mock(mock, src, entries, res, plan, dst)


def test_tentative_ends(gpu_ctx, mock):
    """a tentative end too short and too long, a tentative size too small and too large, both ends unknown, a wrong CRC,
    entries that point outside either buffer: all in one call"""
    from libarchive_amd import lzip
    p = LS.text(9, 5000)
    m = LS.member(p)
    end, crc = len(m) - 20, zlib.crc32(p)
    base = {"src_off": 6, "dst_cap": 6000}
    variants = [
        ("OK", {"src_end": end, "data_size": len(p), "crc32": crc, "dst_cap": len(p)}),
        ("SRC_END", {"src_end": end - 1}), ("EARLY_END", {"src_end": end + 1}), ("EARLY_END", {"src_end": len(m)}),
        ("SIZE_OVER", {"data_size": len(p) - 1}), ("BAD_SIZE", {"data_size": len(p) + 1}),
        ("OK", {}), ("OUT_FULL", {"dst_cap": len(p) - 1}), ("OK", {"dst_cap": len(p)}),
        ("BAD_CRC", {"crc32": crc ^ 0x80000000}), ("OK", {"crc32": crc}),
        ("REFUSED", {"src_off": len(m) + 1}), ("REFUSED", {"src_end": len(m) + 1}), ("REFUSED", {"src_off": 10, "src_end": 9}),
        ("REFUSED", {"dst_off": 1 << 40}), ("REFUSED", {"dst_cap": 1 << 40}), ("REFUSED", {"data_size": 6001}),
        ("TRUNCATED", {"src_off": len(m) - 3}),
    ]
    entries, dst = [], 0
    for _, kw in variants:
        e = dict(base, **kw)
        if "dst_off" not in kw:
            e["dst_off"] = dst
            dst += 6000
        entries.append(e)
    res, plan = lzip.decode_members(gpu_ctx, m, entries, dst_cap=dst)
    assert [name_of(s) for s in res["status"]] == [v[0] for v in variants]
    for i, (want, kw) in enumerate(variants):
        out = plan.output(i)
        if want in ("OK", "BAD_CRC", "BAD_SIZE", "EARLY_END"):
            assert out == p and int(res[i]["consumed"]) == end - 6 and int(res[i]["crc32"]) == crc, i
        elif want in ("SIZE_OVER", "OUT_FULL"):
            assert out == p[:len(p) - 1], i
        elif want == "REFUSED":
            assert int(res[i]["out_len"]) == 0
        else:
            assert p.startswith(out), i
    against_the_mock(mock, m, entries, res, plan, dst)
    assert int(lzip.N.gpu_lib().la_gpu_lzip_workspace_bytes(300)) >= 300 * 20
