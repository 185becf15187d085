"""The hand-built Zstandard frames of tests/zstd_build.py through la_gpu_zstd_decode, with a frame table made here
(the host walker is bypassed, so the device's status is seen per frame), by both kernels (options 0 and
LA_ZSTD_OPT_LANE_KERNEL), then through the filter path (la_api.cat).

Every frame has its own slot (dst_cap = the plain size for a valid frame) in a destination prefilled with a guard
byte: nothing outside [dst_off, dst_off + out_len) may change for an accepted frame, nothing outside its slot for a
refused one (a refused frame may have written blocks in front of its error).  Both kernels must answer the same
(status, out_len, bytes); a valid frame's bytes are the builder's, whose sha256 is libzstd's by
tests/golden/zstd_handbuilt.json, so a GPU machine without libzstd is still held to libzstd's answers.

Where the device and the oracle are deliberately stricter than ZSTD_decompressStream 1.4.8 (the golden file shows
libzstd's "ok" for these):

| case | RFC 8878 | libzstd 1.4.8 | here |
|---|---|---|---|
| bits left over at the end of the sequence bit stream | 3.1.1.3.2.1.2 ("the bitstream shall be entirely consumed, otherwise the bitstream is considered corrupted") | accepts | status 11 |
| repeat offset rep[0] - 1 == 0 | 3.1.1.5 (an offset of 0 is not a valid offset) | forces it to 1 | status 11 |
| zero sequences written in the two-byte count form, with a modes byte behind it (without it libzstd refuses too) | 3.1.1.3.2.1 (0 sequences is the single byte 0) | reads the tables, decodes nothing | status 11 |
"""
import hashlib
import json
import os

import numpy as np
import pytest

import la_api
import zstd_build as B
import zstd_support as Z

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "zstd_handbuilt.json")
OPT_NO_VERIFY, OPT_LANE = 1, 2
GUARD = 0xA5
REFUSED_CAP = 1 << 18


@pytest.fixture(scope="module")
def cases():
    return B.handbuilt_cases()


@pytest.fixture(scope="module")
def gold():
    return {r["name"]: r for r in json.load(open(GOLDEN))}


def _expected_status(o, c):
    if c.status is not None:
        return c.status
    rc, _, msg = Z.oracle_decode(o, c.image, REFUSED_CAP)       # truncation: 12 or 11, as the oracle says
    assert rc != 0, c.name
    return B.ST_TRUNCATED if msg == "Truncated zstd input" else B.ST_CORRUPT


def run_table(gpu_ctx, entries, options):
    """entries: [(image, dst_cap)].  One slot per frame, 64 guard bytes between slots.  Returns [(status, out_len,
    bytes of the slot)] and checks the guard."""
    import torch
    from libarchive_amd import zstd
    frames = np.zeros(len(entries), dtype=zstd.ZSTD_FRAME_DTYPE)
    src, so, do = [], 0, 64
    for i, (img, cap) in enumerate(entries):
        frames[i] = (so, len(img), do, cap)
        src.append(img)
        so += len(img)
        do += ((cap + 15) & ~15) + 64
    image = b"".join(src) + bytes(64)
    d_src = torch.from_numpy(np.frombuffer(image, dtype=np.uint8).copy()).cuda()
    plan = zstd.ZstdDevicePlan(gpu_ctx, d_src, frames, do)
    plan.d_dst.fill_(GUARD)
    plan.batch.src_bytes = so
    plan.run(options)
    res = plan.results()
    dst = plan.d_dst.cpu().numpy()[:do]
    untouched = np.ones(do, dtype=bool)
    out = []
    for i, (img, cap) in enumerate(entries):
        st, n, off = int(res["status"][i]), int(res["out_len"][i]), int(frames["dst_off"][i])
        assert n <= cap, i
        untouched[off:off + (n if st == 0 else cap)] = False
        out.append((st, n, dst[off:off + n].tobytes()))
    assert (dst[untouched] == GUARD).all(), "bytes outside the frames' slots changed"
    return out


def test_every_case_by_both_kernels(gpu_ctx, cases, gold):
    o = Z.oracle_lib()
    entries, want = [], []
    for c in cases:
        entries.append((c.image, len(c.plain) if c.valid else REFUSED_CAP))
        want.append((c.name, _expected_status(o, c), c.plain))
    # a skippable frame in the table; dst_cap one byte short with the last block raw / RLE / compressed with
    # sequences / literals only
    entries.append((B.skippable(b"skip me", 3), 16)); want.append(("skippable", B.ST_OK, b""))
    for name, blocks in (("raw", [B.Raw(B.HIST)]), ("rle", [B.Raw(b"ab"), B.Rle(5, 300)]),
                         ("sequences", [B.Raw(B.HIST), B.Comp(b"abcdef", [(2, 5, 3 + 7), (1, 6, 3 + 9)])]),
                         ("literals-only", [B.Raw(B.HIST), B.Comp(b"abcdef" * 9, [])])):
        img, plain = B.frame(blocks)
        entries.append((img, len(plain))); want.append(("fits-" + name, B.ST_OK, plain))
        entries.append((img, len(plain) - 1)); want.append(("one-byte-short-" + name, B.ST_OUT_FULL, None))
    got = {opt: run_table(gpu_ctx, entries, opt) for opt in (0, OPT_LANE)}
    seen = {0: set(), OPT_LANE: set()}
    for i, (name, status, plain) in enumerate(want):
        a, b = got[0][i], got[OPT_LANE][i]
        print(name, status, a[0], a[1], b[0], b[1])
        assert a == b, name
        assert a[0] == status, (name, a[0], status)
        for opt in seen:
            seen[opt].add(got[opt][i][0])
        if status == B.ST_OK:
            assert a[1] == len(plain) and a[2] == plain, name
            if name in gold:
                assert hashlib.sha256(a[2]).hexdigest() == gold[name]["plain_sha256"], name
        if name in gold:
            assert hashlib.sha256(entries[i][0]).hexdigest() == gold[name]["image_sha256"], name
    for opt in seen:
        assert seen[opt] >= {0, 11, 12, 13, 14, 15, 16, 17}, (opt, seen[opt])


def test_wrong_checksum_passes_without_verification(gpu_ctx, cases):
    c = next(x for x in cases if x.name == "bad-checksum")
    img, plain = B.frame([B.Raw(B.HIST), B.Comp(b"literals", [(4, 5, 3 + 10), (2, 3, 1)])], checksum=True)
    assert len(img) == len(c.image) and img[:-4] == c.image[:-4]
    for opt in (0, OPT_LANE):
        assert run_table(gpu_ctx, [(c.image, len(plain))], opt) == [(B.ST_BAD_CHECKSUM, 0, b"")]
        assert run_table(gpu_ctx, [(c.image, len(plain))], opt | OPT_NO_VERIFY) == [(B.ST_OK, len(plain), plain)]


def test_batches_beyond_both_kernels_stride(gpu_ctx, cases):
    """more than 4096 (waves) and more than 8192 (lanes) frames in one call: both stride loops wrap; refused frames
    scattered among valid ones leave their neighbours alone"""
    o = Z.oracle_lib()
    small = [c for c in cases if len(c.image) <= 400 and (not c.valid or len(c.plain) <= 4096)]
    assert sum(1 for c in small if not c.valid) > 50 and sum(1 for c in small if c.valid) > 200
    status = {c.name: _expected_status(o, c) for c in small}
    for total in (4100, 8300):
        pick = [small[(i * 7) % len(small)] for i in range(total)]
        entries = [(c.image, len(c.plain) if c.valid else 4096 + 64) for c in pick]
        for opt in (0, OPT_LANE):
            got = run_table(gpu_ctx, entries, opt)
            for c, g in zip(pick, got):
                assert g[0] == status[c.name], (total, opt, c.name, g[0])
                if c.valid:
                    assert g[2] == c.plain, (total, opt, c.name)


@pytest.mark.parametrize("lane_kernel", [0, 1], ids=["wave-per-frame", "lane-per-frame"])
def test_through_the_filter(gpu_ctx, monkeypatch, cases, gold, lane_kernel):
    """all valid frames in one stream; then one stream per refusal class: the frames in front of the damage are
    delivered, then ARCHIVE_FATAL with libzstd's error name as the golden file has it"""
    monkeypatch.setenv("LA_ZSTD_LANE_KERNEL", str(lane_kernel))
    valid = [c for c in cases if c.valid]
    res = la_api.cat(b"".join(c.image for c in valid))
    data, rc, msg = la_api.as_reference_tuple(res)
    assert (rc, msg) == (0, "")
    assert hashlib.sha256(data).hexdigest() == hashlib.sha256(b"".join(c.plain for c in valid)).hexdigest()
    front = [c for c in valid if len(c.plain) < 70000][:40]
    prefix, plain = b"".join(c.image for c in front), b"".join(c.plain for c in front)
    by_name = {c.name: c for c in cases}
    for name, text in (("bad-checksum", "Restored data doesn't match checksum"), ("bad-reserved-header-bit", "Unsupported frame parameter"),
                       ("bad-window-descriptor-2^28", "Frame requires too much memory for decoding"),
                       ("bad-dictionary-id-2-bytes", "Dictionary mismatch"), ("bad-block-type-3", "Corrupted block detected"),
                       ("bad-raw-block-larger-than-window", "Corrupted block detected")):
        assert gold[name]["libzstd"] == text, name
        res = la_api.cat(prefix + by_name[name].image + front[0].image)
        assert la_api.as_reference_tuple(res) == (plain, la_api.ARCHIVE_FATAL, "Zstd decompression failed: " + gold[name]["libzstd"]), name
