"""The device ABI of the lzop kernels (la_lzo.hip through la_gpu_lzop_decode, la_hash.hip through la_gpu_adler32_many),
bit-exact against the Python oracle (lzop_support.decode, which the reference's fixtures pin) and zlib's sums: status,
bytes, consumed and both sums per block."""
import zlib

import numpy as np
import pytest

import lzop_support as L

pytestmark = pytest.mark.gpu

NAMES = {v: k for k, v in L.ST.items()}


def decode_table(gpu_ctx, streams, flags=None):
    """[(stream, dst_len)] packed into one table and decoded in one call: [(status name, bytes of the slot, consumed)]
    and the raw results"""
    from libarchive_amd import lzop
    src, blocks, total = L.pack_table(streams)
    entries = [{"src_off": b.src_off, "dst_off": b.dst_off, "src_len": b.src_len, "dst_len": b.dst_len} for b in blocks]
    for e, f in zip(entries, flags or []):
        e.update(f)
    res, plan = lzop.decode_blocks(gpu_ctx, src, entries, total)
    slab = plan.slab()
    return [(NAMES[int(r["status"])], slab[e["dst_off"]:e["dst_off"] + int(r["out_len"])], int(r["consumed"])) for r, e in zip(res, entries)], res


@pytest.fixture(scope="module")
def cases():
    """the rules cases the ABI decodes (it refuses a stream longer than its bytes, and one as long is a stored block), with
    the oracle's answer for each"""
    out = []
    for name, (stream, dst_len, verdict, plain) in L.rules_cases().items():
        if len(stream) < dst_len:
            ref = L.decode(stream, dst_len)
            assert ref[0] == verdict and ref[1] == plain
            out.append((name, stream, dst_len, ref))
    assert len(out) > 150 and {c[3][0] for c in out} == {"OK", "INPUT_OVERRUN", "OUTPUT_OVERRUN", "LOOKBEHIND", "NOT_CONSUMED", "SHORT_OUTPUT"}
    return out


@pytest.mark.parametrize("data", ["noise", "ff"])
def test_adler32_many(gpu_ctx, data):
    from libarchive_amd import lzop
    lens = [0, 1, 63, 64, 65, 5551, 5552, 5553, 65521, 1 << 20]
    n = sum(lens) + 3 * len(lens) + 8
    buf = L.randbytes(5, n) if data == "noise" else b"\xff" * n
    jobs = []
    at = 1
    for ln in lens:                 # (every range at an odd offset; a fresh sum, a running one, and the largest running value)
        for seed in (1, zlib.adler32(b"a running value in front of the range"), (65520 << 16) | 65520):
            jobs.append((at, ln, seed))
        at += ln + 3
    got = lzop.adler32_many(gpu_ctx, lzop.to_device(buf), jobs)
    for j, g in zip(jobs, got):
        assert int(g) == zlib.adler32(buf[j[0]:j[0] + j[1]], j[2]), j


def test_adler32_many_more_jobs_than_waves(gpu_ctx):
    from libarchive_amd import lzop
    buf = L.randbytes(6, 300000)
    jobs = [(i * 31 % 200000, 1 + i * 7 % 3000, 1) for i in range(9000)]
    got = lzop.adler32_many(gpu_ctx, lzop.to_device(buf), jobs)
    assert [int(g) for g in got] == [zlib.adler32(buf[o:o + n]) for o, n, _ in jobs]


@pytest.mark.parametrize("n_blocks", [1, 2, 65, 4097])
def test_rules_cases_in_tables(gpu_ctx, cases, n_blocks):
    """the rules cases of tests/test_lzo_rules.py, packed into tables of 1, 2, 65 and 4097 blocks: every case is in one of
    the tables of each size class but the first two, which take the longest case and its neighbour"""
    if n_blocks <= 2:
        order = sorted(cases, key=lambda c: -len(c[1]))[:n_blocks]
    else:
        order = [cases[i % len(cases)] for i in range(n_blocks)]
    got, _ = decode_table(gpu_ctx, [(c[1], c[2]) for c in order])
    for c, g in zip(order, got):
        assert g == c[3], c[0]


def test_every_status_with_the_bytes_in_front_valid(gpu_ctx, cases):
    by = {}
    for c in cases:
        by.setdefault(c[3][0], c)
    order = list(by.values())
    got, res = decode_table(gpu_ctx, [(c[1], c[2]) for c in order])
    for c, g, r in zip(order, got, res):
        assert g == c[3], c[0]
        assert int(r["out_len"]) == len(c[3][1])
    assert any(len(g[1]) > 0 and g[0] != "OK" for g in got)


@pytest.mark.parametrize("n", [1, 63, 64, 65])
def test_stored_blocks(gpu_ctx, n):
    p = L.noise(n, n)
    big = L.randbytes(n, 70000 + n)
    t = L.text(3, 2000)
    got, res = decode_table(gpu_ctx, [(p, n), (L.compress(t), len(t)), (big, len(big)), (p, n)],
                            [{"flags": L.C_ADLER32, "sum_c": zlib.adler32(p)}, {}, {"flags": L.C_CRC32 | L.U_CRC32, "sum_c": zlib.crc32(big), "sum_u": 1}, {}])
    assert [g[0] for g in got] == ["OK"] * 4 and [g[1] for g in got] == [p, t, big, p]
    assert [g[2] for g in got] == [n, len(L.compress(t)), len(big), n]
    assert int(res[2]["sum_u"]) == 0        # a stored block's second sum is not looked at


@pytest.mark.parametrize("n", [511, 512, 513])
def test_literals_and_matches_across_the_window_refill(gpu_ctx, cases, n):
    """literal runs and matches of 511, 512 and 513 bytes whose instructions stand 0, 1, 250, 255 and 256 bytes into the
    stream: the instruction behind each run is read from the payload window's second half, its refill or a reload"""
    mine = [c for c in cases if c[0].startswith("window_literals_%d_" % n)]
    assert len(mine) == 5
    got, _ = decode_table(gpu_ctx, [(c[1], c[2]) for c in mine])
    for c, g in zip(mine, got):
        assert g == c[3] and g[0] == "OK", c[0]


@pytest.mark.parametrize("kind", ["text", "noise"])
def test_a_block_of_256_kib(gpu_ctx, kind):
    p = L.text(11, 262144) if kind == "text" else L.noise(12, 262144, 16)
    s = L.compress(p)
    assert len(s) < len(p)
    got, res = decode_table(gpu_ctx, [(s, len(p))], [{"flags": L.C_ADLER32 | L.U_ADLER32, "sum_c": zlib.adler32(s), "sum_u": zlib.adler32(p)}])
    assert got[0] == ("OK", p, len(s))
    assert (int(res[0]["sum_c"]), int(res[0]["sum_u"])) == (zlib.adler32(s), zlib.adler32(p))


def test_checksum_flags(gpu_ctx):
    """all four flag choices per side, CRC32 winning over Adler-32; a wrong sum on either side; no flag, no compare"""
    p = L.text(9, 3000)
    s = L.compress(p)
    sums = {0: 0, L.C_ADLER32: zlib.adler32(s), L.C_CRC32: zlib.crc32(s), L.C_ADLER32 | L.C_CRC32: zlib.crc32(s)}
    sumu = {0: 0, L.U_ADLER32: zlib.adler32(p), L.U_CRC32: zlib.crc32(p), L.U_ADLER32 | L.U_CRC32: zlib.crc32(p)}
    flags, want = [], []
    for fc in sums:
        for fu in sumu:
            flags.append({"flags": fc | fu, "sum_c": sums[fc], "sum_u": sumu[fu]})
            want.append(("OK", sums[fc], sumu[fu], len(p)))
            flags.append({"flags": fc | fu, "sum_c": sums[fc] ^ 1, "sum_u": sumu[fu]})
            want.append(("BAD_SUM_C" if fc else "OK", sums[fc], 0 if fc else sumu[fu], 0 if fc else len(p)))
            flags.append({"flags": fc | fu, "sum_c": sums[fc], "sum_u": sumu[fu] ^ 0x80000000})
            want.append(("BAD_SUM_U" if fu else "OK", sums[fc], sumu[fu], len(p)))
    got, res = decode_table(gpu_ctx, [(s, len(p))] * len(flags), flags)
    for g, r, w, f in zip(got, res, want, flags):
        assert (g[0], int(r["sum_c"]), int(r["sum_u"]), int(r["out_len"])) == w, f
        assert g[1] == p[:w[3]]


def test_a_refused_entry_beside_good_ones(gpu_ctx):
    from libarchive_amd import lzop
    p = L.text(9, 3000)
    s = L.compress(p)
    src = s + s
    good = {"src_off": 0, "dst_off": 0, "src_len": len(s), "dst_len": len(p)}
    entries = [good, dict(good, src_off=len(src) - 5), dict(good, dst_off=4000), dict(good, src_len=len(p) + 1, src_off=0, dst_len=len(p)),
               dict(good, dst_len=(64 << 20) + 1), dict(good, src_off=1 << 40), dict(good, src_off=len(s), dst_off=3000)]
    res, plan = lzop.decode_blocks(gpu_ctx, src, entries, 6000)
    assert [NAMES[int(r["status"])] for r in res] == ["OK", "REFUSED", "REFUSED", "REFUSED", "REFUSED", "REFUSED", "OK"]
    slab = plan.slab()
    assert slab[:3000] == p and slab[3000:6000] == p
    assert all(int(r["out_len"]) == 0 for r in res[1:6])
    res, _ = lzop.decode_blocks(gpu_ctx, b"", [], 0)
    assert len(res) == 0
