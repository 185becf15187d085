"""The hand-built deflate streams of tests/deflate_build.py through la_gpu_gzip_decode with a member table made here,
by all four paths (LA_GZ_OPT_WAVE_KERNEL, LA_GZ_OPT_LANE_KERNEL, LA_GZ_OPT_TWO_PHASE and the same with
LA_GZ_OPT_EXPAND_INORDER), as gzip members (body + trailer) and as bare streams (LA_GZ_OPT_RAW), then through the filter
(la_api.cat).

Every member has its own slot in a destination prefilled with a guard byte, 64 guard bytes between slots; dst_cap is
exactly the plain size for a valid member and a fixed cap for a refused one.  Nothing outside
[dst_off, dst_off + out_len) may change for an accepted member whose slot is its plain size, nothing outside the slot for
any member (the lane kernel's wild copies may write past a match, inside the slot).  Sources are packed without padding,
the last member ends exactly at src_bytes, and one more member claims a src_len that reaches past src_bytes.

What is expected comes from the builder's model, whose sha256 per case is zlib 1.2.11's by
tests/golden/deflate_handbuilt.json (tests/test_oracle_deflate_handbuilt.py keeps that file honest where zlib is at
hand), so a GPU machine is held to zlib's answers without needing zlib."""
import hashlib
import json
import os
import random
import zlib

import numpy as np
import pytest

import deflate_build as B
import la_api
import oracle_lib as O

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "deflate_handbuilt.json")
OPT_WAVE, OPT_LANE, OPT_TWO_PHASE, OPT_RAW, OPT_INORDER = 2, 4, 8, 16, 32
PATHS = ((OPT_WAVE, "wave per member"), (OPT_LANE, "lane per member, in place"), (OPT_TWO_PHASE, "two-phase"),
         (OPT_TWO_PHASE | OPT_INORDER, "two-phase, in-order expand"))
GUARD = 0xA5
REFUSED_CAP = 8192
ST_OK, ST_DATA, ST_TRUNC, ST_FULL = B.ST_OK, B.ST_DATA, B.ST_TRUNCATED, B.ST_OUT_FULL


@pytest.fixture(scope="module")
def cases():
    return B.handbuilt_cases()


@pytest.fixture(scope="module")
def gold():
    return {r["name"]: r for r in json.load(open(GOLDEN))}


def trailer(data):
    return (zlib.crc32(data) & 0xFFFFFFFF).to_bytes(4, "little") + (len(data) & 0xFFFFFFFF).to_bytes(4, "little")


def run_table(gpu_ctx, entries, options, extra_claim=0):
    """entries: [(source bytes, dst_cap)].  One slot per member, 64 guard bytes between slots, sources back to back.
    extra_claim > 0: one more member reads the LAST entry's source again and claims extra_claim bytes more than the
    source holds.  Returns [(status, bytes, consumed, crc32)] and checks the guard."""
    import torch
    from libarchive_amd import _native as N
    n = len(entries) + (1 if extra_claim else 0)
    mem = np.zeros(n, dtype=N.GZ_MEMBER_DTYPE)
    so, do = 0, 64
    for i, (img, cap) in enumerate(entries):
        mem[i] = (so, len(img), cap, do)
        so += len(img)
        do += cap + 64
    if extra_claim:
        img, cap = entries[-1]
        mem[n - 1] = (so - len(img), len(img) + extra_claim, cap, do)
        do += cap + 64
    src = b"".join(e[0] for e in entries)
    d_src = torch.from_numpy(np.frombuffer(src + bytes(64), dtype=np.uint8).copy()).cuda()
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
    untouched = np.ones(do, dtype=bool)
    out = []
    for i in range(n):
        st, ln, off, cap = int(res[i]["status"]), int(res[i]["out_len"]), int(mem[i]["dst_off"]), int(mem[i]["dst_cap"])
        assert ln <= cap, i
        untouched[off:off + cap] = False
        out.append((st, dst[off:off + ln].tobytes(), int(res[i]["consumed"]), int(res[i]["crc32"])))
    assert (dst[untouched] == GUARD).all(), "bytes outside the members' slots changed (options %d)" % options
    return out


def by_all_paths(gpu_ctx, entries, raw=False, extra_claim=0):
    """the table by the four paths: they must agree exactly (as tests/test_gpu_gzip.py: `consumed` means something when
    the deflate stream ended, and what a member that does not fit had produced is not part of the contract)"""
    norm = lambda rs: [(st, None, None, None) if st == ST_FULL else (st, out, cons if st == ST_OK else None, crc)
                       for st, out, cons, crc in rs]
    first = None
    for opt, what in PATHS:
        got = run_table(gpu_ctx, entries, opt | (OPT_RAW if raw else 0), extra_claim)
        if first is None:
            first = got
        else:
            a, b = norm(first), norm(got)
            diff = [i for i in range(len(a)) if a[i] != b[i]]
            assert not diff, "wave-per-member and %s disagree at members %s" % (what, diff[:10])
    return first


def _check(name, got, status, plain, consumed=None, gold_row=None):
    st, out, cons, crc = got
    assert st == status, (name, st, status)
    if status == ST_FULL:
        return
    assert out == plain, (name, len(out), len(plain))
    if gold_row is not None:
        assert hashlib.sha256(out).hexdigest() == gold_row["plain_sha256"], name
    if status == ST_OK:
        assert crc == zlib.crc32(plain) & 0xFFFFFFFF, name
        if consumed is not None:
            assert cons == consumed, (name, cons, consumed)


@pytest.mark.parametrize("raw", [False, True], ids=["gzip-members", "bare-streams"])
def test_member_table_by_every_path(gpu_ctx, cases, gold, raw):
    tail = B.cut_case("tail-cut", B.prefix_streams()[1][1], 200)
    table = list(cases) + [tail]
    entries = [(c.image + (trailer(c.plain) if c.valid and not raw else b""), len(c.plain) if c.valid else REFUSED_CAP) for c in table]
    got = by_all_paths(gpu_ctx, entries, raw, extra_claim=37)
    seen = set()
    for c, g in zip(table, got):
        row = gold.get(c.name)
        if row is not None:
            assert hashlib.sha256(c.image).hexdigest() == row["image_sha256"], c.name
        _check(c.name, g, c.status, c.plain, row["consumed"] if row and c.valid else None, row)
        seen.add(g[0])
    _check("claims-past-src_bytes", got[-1], ST_TRUNC, tail.plain)
    assert seen == {ST_OK, ST_DATA, ST_TRUNC}


def _last_op_members():
    lits = list(b"the slot is one byte short: ")
    for kind, mk in (("fixed", lambda ops: B.Fixed(ops)), ("dynamic", lambda ops: B._dyn_auto(ops, random.Random(6)))):
        yield kind + "-last-op-literal", [mk(lits)]
        yield kind + "-last-op-match", [mk(lits + [B.M(9, 11)])]
        yield kind + "-last-op-long-match", [mk(lits + [B.M(258, 3)])]
        yield kind + "-last-op-end-of-block", [mk(lits), B.Fixed([])]
    yield "last-op-stored-byte", [B.Fixed(lits), B.Stored(b"stored tail")]
    yield "stored-only", [B.Stored(bytes(range(200)))]


def test_slots_one_byte_short_and_copy_class_boundaries(gpu_ctx):
    """status 9 when the slot is one byte short, whatever the last op is; then the lane kernel's copy classes
    (dist >= 16 and 16 bytes of room behind the match, dist >= 8 and 8 bytes, bytewise): a final match of distance
    7 / 8 / 15 / 16 with 0 / 7 / 8 / 15 / 16 bytes of slot behind it"""
    entries, want = [], []
    for name, blocks in _last_op_members():
        image, plain, valid, _, _ = B.build(blocks)
        assert valid
        entries.append((image + trailer(plain), len(plain))); want.append((name, ST_OK, plain))
        entries.append((image + trailer(plain), len(plain) - 1)); want.append((name + "-short", ST_FULL, None))
    for dist in (7, 8, 15, 16):
        for length in (3, 8, 16, 17, 40):
            image, plain, valid, _, _ = B.build([B.Fixed(list(range(100, 130)) + [B.M(length, dist)])])
            assert valid
            for room in (0, 7, 8, 15, 16):
                entries.append((image + trailer(plain), len(plain) + room))
                want.append(("match-%d-dist-%d-room-%d" % (length, dist, room), ST_OK, plain))
            entries.append((image + trailer(plain), len(plain) - 1)); want.append(("match-%d-dist-%d-short" % (length, dist), ST_FULL, None))
    got = by_all_paths(gpu_ctx, entries)
    for (name, status, plain), g in zip(want, got):
        _check(name, g, status, plain)


def test_every_prefix_members(gpu_ctx):
    """the six streams of tests/test_oracle_deflate_handbuilt.py cut at every byte, as one batch of bare streams: status
    and bytes are the oracle's for each prefix"""
    entries, want = [], []
    for name, blocks in B.prefix_streams():
        image, plain, valid, _, _ = B.build(blocks)
        for n in range(len(image) + 1):
            rc, cons, out = O.inflate_raw(image[:n], REFUSED_CAP)
            entries.append((image[:n], REFUSED_CAP))
            want.append(("%s[:%d]" % (name, n), {0: ST_OK, 1: ST_TRUNC, 2: ST_DATA}[rc], out, cons))
    got = by_all_paths(gpu_ctx, entries, raw=True)
    for (name, status, out, cons), g in zip(want, got):
        _check(name, g, status, out, cons)


def test_neighbours_do_not_matter(gpu_ctx, cases):
    """the table in catalogue order and in a seeded shuffle that gives every wave of the lane kernel 64 different codes:
    per-member results are identical"""
    order = list(range(len(cases)))
    random.Random(64).shuffle(order)
    for w in range(0, len(order) - 63, 64):
        assert len({cases[i].image for i in order[w:w + 64]}) == 64
    entry = lambda c: (c.image, len(c.plain) if c.valid else REFUSED_CAP)
    for opt, what in PATHS:
        a = run_table(gpu_ctx, [entry(c) for c in cases], opt | OPT_RAW)
        b = run_table(gpu_ctx, [entry(cases[i]) for i in order], opt | OPT_RAW)
        for k, i in enumerate(order):
            assert a[i] == b[k], (what, cases[i].name)
            _check(cases[i].name, b[k], cases[i].status, cases[i].plain)


GZ_HEADER = b"\x1f\x8b\x08\x00\x00\x00\x00\x00\x00\x03"


def test_through_the_filter(gpu_ctx, cases):
    """all valid cases as gzip members of one stream; then one stream per refusal class: the bytes in front of the damage,
    then ARCHIVE_FATAL with the reference's text, as oracle/orc_filters.c derives them"""
    valid = [c for c in cases if c.valid]
    stream = b"".join(GZ_HEADER + c.image + trailer(c.plain) for c in valid)
    plain = b"".join(c.plain for c in valid)
    data, rc, msg = la_api.as_reference_tuple(la_api.cat(stream))
    assert (rc, msg) == (0, "")
    assert hashlib.sha256(data).hexdigest() == hashlib.sha256(plain).hexdigest()
    front, total = [], 0
    for c in valid:                 # (more than two of the filter's 64 KiB blocks in front of the damage)
        if len(c.plain) <= 20000 and total < 150000:
            front.append(c)
            total += len(c.plain)
    assert total >= 150000
    head = b"".join(GZ_HEADER + c.image + trailer(c.plain) for c in front)
    by_name = {c.name: c for c in cases}
    for name in ("block-type-3", "fixed-length-symbol-286", "fixed-distance-symbol-31", "distance-too-far-after-matches",
                 "stored-bad-nlen", "dynamic-hlit-287", "dynamic-hdist-32", "dynamic-16-at-index-0", "dynamic-18-runs-3-past-hlit-plus-hdist",
                 "dynamic-all-zero-code-length-code", "dynamic-code-length-code-over-subscribed", "dynamic-no-end-of-block-code",
                 "dynamic-lone-1-bit-distance-code-unassigned-sibling", "stored-short-body", "stored-cut-inside-len-nlen",
                 "dynamic-16-at-index-0-extra-bits-missing-is-truncated", "dynamic-all-zero-code-length-code-cut"):
        c = by_name[name]
        image = head + GZ_HEADER + c.image
        ref, res = O.gzip_stream_decode(image, len(head) * 40 + 65536)
        want = "gzip decompression failed" if c.status == ST_DATA else "truncated gzip input"
        assert (res.rc, res.errmsg.decode()) == (la_api.ARCHIVE_FATAL, want), name
        got = la_api.as_reference_tuple(la_api.cat(image))
        assert got == (ref.tobytes(), la_api.ARCHIVE_FATAL, want), (name, len(got[0]), got[1:], len(ref))
