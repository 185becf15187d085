"""The device ABI of xz filter chains (la_xz_filters.hip through la_gpu_xz_decode with LA_XZ_BATCH_CHAINS) against
liblzma's raw decoder: for a buffer X and a chain, the block holds LZMA2(X) and has to come out as liblzma's filter
decoders leave X, with the block check -- taken over those unfiltered bytes -- verified in the same call."""
import hashlib
import struct
import zlib

import pytest

import xz_build as XB
import xz_chains_support as XC

pytestmark = pytest.mark.gpu

OK, LZMA, SIZE, BAD_CHECK = 0, 26, 28, 29
DELTA, X86, ARM = XC.DELTA, XC.X86, XC.ARM


def check_bytes(cid, data):
    return {0: b"", 1: struct.pack("<I", zlib.crc32(data)), 4: struct.pack("<Q", XB.crc64(data)), 10: hashlib.sha256(data).digest()}[cid]


def decode(gpu_ctx, items, spoil_check=()):
    """items: (X, chain, check id, sized).  One call for all of them; returns (results, outputs, expected outputs)"""
    from libarchive_amd import xz
    src, entries, dst, want = b"", [], 0, []
    for i, (x, chain, cid, sized) in enumerate(items):
        raw = XB.lzma2(bytes(x), preset=0)
        out = XC.liblzma_unfilter(chain, x) if chain else bytes(x)
        chk = check_bytes(cid, out if i not in spoil_check else bytes(x))
        off = len(src)
        e = {"src_off": off, "dst_off": dst, "dst_cap": len(x) if sized else len(x) + 64, "check_id": cid}
        if sized:
            e.update(comp_size=len(raw), uncomp_size=len(x), check_off=off + len(raw) + (-len(raw) % 4))
        entries.append(e)
        src += raw + bytes(-len(raw) % 4) + chk + bytes(-len(chk) % 4)
        dst += e["dst_cap"]
        want.append(out)
    res, plan = xz.decode_blocks(gpu_ctx, src, entries, chains=[c for _, c, _, _ in items])
    return res, [plan.output(i) for i in range(len(items))], want


def test_every_filter_and_every_hard_buffer_in_one_batch(gpu_ctx):
    items = []
    for fid, prop in XC.ALONE:
        for n in (0, 1, 5, 17, 4099, 2 * XC.TILE + 19):
            items.append((XC.dense(fid, fid * 7 + n, n), [(fid, prop)]))
    for dist in (1, 2, 3, 4, 255, 256):         # tiles that dist does not divide, one tile +- 1, two tiles + 1
        for n in (dist - 1, dist, dist + 1, XC.TILE - 1, XC.TILE + 1, 2 * XC.TILE + 1):
            items.append((XC.dense(ARM, dist * 9 + n, n), [(DELTA, dist)]))
    for off in (0, 0x1000, 0xFFFFFFFB):
        for name, x in sorted(XC.x86_buffers().items()):
            if off == 0 or not name.startswith(("short_", "tail_")):
                items.append((x, [(X86, off)]))
    for chain in XC.CHAINS.values():
        items.append((XC.dense(X86, 5, 3 * XC.TILE + 7), chain))
        items.append((XC.real_code(50000), chain))
    items.append((XC.real_code(), []))           # no chain beside chains
    items.append((XC.dense(XC.ARMTHUMB, 3, 70000), [(XC.ARMTHUMB, 0), (DELTA, 2), (XC.SPARC, 8)]))
    items = [(x, chain, (1, 4, 10)[i % 3], i % 2 == 0) for i, (x, chain) in enumerate(items)]
    res, got, want = decode(gpu_ctx, items)
    bad = [(i, int(res[i]["status"]), items[i][1], len(items[i][0])) for i in range(len(items)) if int(res[i]["status"]) != OK or got[i] != want[i]]
    assert not bad, bad[:10]
    assert any(w != bytes(x) for w, (x, _, _, _) in zip(want, items))


def test_the_check_is_taken_over_the_unfiltered_bytes(gpu_ctx):
    """a check value over the FILTERED bytes is refused"""
    x = XC.dense(X86, 11, 20000)
    items = [(x, [(X86, 0)], cid, sized) for cid in (1, 4, 10) for sized in (True, False)]
    res, got, want = decode(gpu_ctx, items, spoil_check=range(len(items)))
    assert [int(s) for s in res["status"]] == [BAD_CHECK] * len(items)
    assert got == want and want[0] != x


@pytest.mark.parametrize("fid,prop", [(X86, 0), (DELTA, 4), (ARM, 0)])
def test_a_failed_block_is_unfiltered_up_to_its_valid_bytes(gpu_ctx, fid, prop):
    from libarchive_amd import xz
    f = XC.dense(fid, 90 + fid, 74000)
    w = XB.Lzma2Writer().raw_chunk(1, f[:65536]).raw_chunk(2, f[65536:])
    w.lzma_chunk(0xC0, XB.literals(b"abcdefgh") + [XB.Match(len(f) + 9, 4)] + XB.literals(b"zz"))
    good = XC.dense(fid, 5, 30000)
    raw_good = XB.lzma2(good, preset=0)
    first = w.image() + bytes(-len(w.image()) % 4)
    src = first + raw_good + bytes(-len(raw_good) % 4)       # (the block padding is part of a block)
    entries = [{"src_off": 0, "dst_off": 0, "dst_cap": 80000}, {"src_off": len(first), "dst_off": 80000, "dst_cap": 30064}]
    res, plan = xz.decode_blocks(gpu_ctx, src, entries, chains=[[(fid, prop)], [(fid, prop)]])
    assert [int(s) for s in res["status"]] == [LZMA, OK]
    valid = int(res[0]["valid"])
    assert valid == len(f) + 8 == int(res[0]["out_len"])
    want = XC.liblzma_unfilter([(fid, prop)], f + b"abcdefgh")
    assert plan.output(0)[:valid - 16] == want[:valid - 16] and want != f + b"abcdefgh"
    assert plan.output(1) == XC.liblzma_unfilter([(fid, prop)], good)


def test_bad_table_entries(gpu_ctx):
    from libarchive_amd import xz
    x = XC.dense(X86, 2, 5000)
    raw = XB.lzma2(x, preset=0)
    raw += bytes(-len(raw) % 4)
    bad = [[(0x0A, 0)], [(0x0B, 0)], [(0x21, 0)], [(2, 0)], [(X86, 0), (0, 0)], [(ARM, 2)], [(XC.ARMTHUMB, 1)], [(XC.IA64, 8)], [(DELTA, 0)], [(DELTA, 257)],
           [(DELTA, 1)] * 4]       # (the last: a count of four)
    chains = [[(X86, 0)]] + bad + [[(DELTA, 256), (XC.IA64, 16)]]
    entries = [{"src_off": 0, "dst_off": 5100 * i, "dst_cap": 5064} for i in range(len(chains))]
    res, plan = xz.decode_blocks(gpu_ctx, raw, entries, chains=chains)
    assert [int(s) for s in res["status"]] == [OK] + [SIZE] * len(bad) + [OK]
    assert all(int(res[i]["out_len"]) == 0 for i in range(1, 1 + len(bad)))
    assert plan.output(0) == XC.liblzma_unfilter(chains[0], x) and plan.output(len(chains) - 1) == XC.liblzma_unfilter(chains[-1], x)


def test_other_flag_bits_are_refused(gpu_ctx):
    from libarchive_amd import xz
    x = XC.dense(X86, 2, 500)
    raw = XB.lzma2(x, preset=0)
    res, plan = xz.decode_blocks(gpu_ctx, raw + bytes(-len(raw) % 4), [{"src_off": 0, "dst_cap": len(x) + 64}], chains=[[(X86, 0)]])
    assert int(res[0]["status"]) == OK
    for flags in (2, 3, 0x80000000):
        plan.batch.reserved = flags
        with pytest.raises(RuntimeError, match="la_gpu_xz_decode"):
            plan.run()
