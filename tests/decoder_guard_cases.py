"""TEST INFRASTRUCTURE: the case tables of the guard-band tests for la_gpu_bzip2_decode, la_gpu_xz_decode (with and
without filter chains), la_gpu_lzip_decode, la_gpu_lzop_decode and la_gpu_uu_decode, and the rules they are held to.
CPU only: tests/test_decoder_guard_cases.py runs the tables through the CPU stand-ins of tests/mock_gpu,
tests/test_gpu_decoder_guards.py through the device.

A Call is one call of a decoder: the source image, the table, the size of d_dst and one Unit per table entry (uu: one
Unit for the window).  A Unit holds what a reference says about the entry -- status and bytes -- and the unit's slot in
d_dst.  Every expectation comes from a reference, never from the code under test: Python's lzma and bz2,
xz_support.reference_read (liblzma's stream decoder), lzip_support.expected_stream_result (liblzma's raw decoder),
lzop_support.decode, uu_support.walk, xz_chains_support.liblzma_unfilter, and bzip2_build's model with the recorded
answers of libbz2 (tests/golden/bzip2_handbuilt.json).  Which status a bound gives (LA_ST_XZ_OUT_FULL for dst_cap,
LA_ST_XZ_SIZE for a header size, ...) is include/la_gpu.h's wording.

The rules (judge() below), checked against include/la_gpu.h:
  slot       nothing changes outside the unit's slot, whatever its status: xz and lzip [dst_off, dst_off + dst_cap)
             ("every block's [dst_off, dst_off + dst_cap) lies inside it"), lzop [dst_off, dst_off + dst_len), bzip2
             [dst_off, dst_off + out_len) of each emitted block, uu [0, out_len)
  untouched  the whole slot is unchanged: an xz entry refused with LA_ST_XZ_SIZE ("is not decoded"), lzip REFUSED, lzop
             REFUSED ("not touched") and BAD_SUM_C ("not decoded"), a bzip2 block behind n_emit or whose packed end lies
             outside dst_cap, a bzip2 entry that is refuted or was never confirmed
  exact      a unit with status OK changes nothing at or behind dst_off + out_len.  For xz, lzip and lzop this asks more
             than the header's words do; EXACT says per decoder whether it is asserted
  prefix     a failed unit's [dst_off, dst_off + out_len) is the reference's prefix; between out_len and the slot's end
             the bytes are free

The only numbers that are not the formats' own are the kernels' tile sizes: TILE (csrc/la_xz_filters.hip, through
xz_chains_support.TILE), UU_SRC_LDS and UU_LINES_PER_GROUP (csrc/la_uu.hip: UU_SRC_LDS, UU_LPB)."""
import base64
import functools
import json
import lzma
import os
import zlib

import numpy as np

import guard_support as G
import lzip_support as LS
import lzop_support as LO
import uu_support as U
import xz_build as XB
import xz_chains_support as XC
import xz_support as XS
from libarchive_amd import _native as N

TILE = XC.TILE                  # csrc/la_xz_filters.hip: the filters' tile
UU_SRC_LDS = 24576              # csrc/la_uu.hip: UU_SRC_LDS, the source bytes of a group of lines that fit in LDS
UU_LINES_PER_GROUP = 256        # csrc/la_uu.hip: UU_LPB
OK = 0

# status OK: is "nothing at or behind dst_off + out_len changes" asserted (True), or the slot rule alone (False)?
EXACT = {"xz": True, "xz_chains": True, "lzip": True, "lzop": True, "bzip2": True, "uu": True}


class Unit:
    """one table entry: `status` and `out` from the reference; `slot` (off, length) is what the slot rule allows to change;
    `untouched`: nothing of it may.  `expect_len`: "exact" -- the record's out_len is len(out); "prefix" -- it is at most
    that, and out[:out_len] is what must be there; "covers" -- it is at least that, and the reference pins only those
    first bytes (a failed block behind a BCJ filter, whose last bytes liblzma never hands out); None -- the record's
    out_len is not about d_dst (a bzip2 block that is measured and not emitted)"""

    def __init__(self, name, status, out, slot, untouched=False, expect_len="exact"):
        self.name, self.status, self.out, self.slot, self.untouched, self.expect_len = name, status, bytes(out), slot, untouched, expect_len


class Call:
    def __init__(self, decoder, name, src, table, dst_total, units, **opts):
        self.decoder, self.name, self.src, self.table, self.dst_total, self.units, self.opts = decoder, name, bytes(src), table, dst_total, units, opts
        for u in units:
            assert u.slot is None or (0 <= u.slot[0] and u.slot[0] + u.slot[1] <= dst_total), (name, u.name)

    def statuses(self):
        return {u.status for u in self.units}


def judge(call, pairs, buf):
    """`pairs` is [(status, out_len)] per unit as the decoder answered, `buf` the GuardedBuffer it wrote to.  Holds the
    answer to the references and the buffer to the rules; returns the defined bytes of every unit (for two_fills)."""
    assert len(pairs) == len(call.units), (call.name, len(pairs), len(call.units))
    slots, defined, labels = [], [], []
    for u, (status, out_len) in zip(call.units, pairs):
        what = (call.name, u.name)
        assert status == u.status, (what, "status", status, "expected", u.status)
        if u.expect_len is None:
            out_len = 0
        elif u.expect_len == "exact":
            assert out_len == len(u.out), (what, "out_len", out_len, "expected", len(u.out))
        elif u.expect_len == "prefix":
            assert out_len <= len(u.out), (what, "out_len", out_len, "at most", len(u.out))
        else:
            assert out_len >= len(u.out), (what, "out_len", out_len, "at least", len(u.out))
        if u.untouched:
            assert out_len == 0, (what, "out_len of a unit that is not decoded", out_len)
            defined.append(b"")
            continue
        off, room = u.slot
        assert out_len <= room, (what, "out_len", out_len, "above the slot's", room)
        pinned = min(out_len, len(u.out))
        got = buf.read(off, pinned)
        assert got == u.out[:pinned], (what, "the bytes differ from the reference's, first at %d of %d"
                                       % (next(i for i in range(pinned) if got[i] != u.out[i]), pinned))
        defined.append(got)
        slots.append((off, out_len) if status == OK and EXACT[call.decoder] and u.expect_len is not None else (off, room))
        labels.append("%s %s" % what)
    G.assert_only_slots_changed(buf, slots, labels)
    return defined


def run_guarded(call, backend, shift_dst=0, shift_src=0):
    """the call through `backend` (decode(call, src, dst) -> (records as plain tuples, [(status, out_len)]); `device` for
    the buffers) under two fills, judged after each"""
    def run(fill, junk):
        src = G.SourceBuffer(call.src, junk, shift_src, device=backend.device)
        dst = G.GuardedBuffer(call.dst_total, fill, shift_dst, device=backend.device)
        records, pairs = backend.decode(call, src, dst)
        return records, judge(call, pairs, dst)
    return G.two_fills(run)


def rows(a):
    """a structured array as a list of tuples of plain ints (nested fields as tuples)"""
    return [tuple(tuple(int(v) for v in x) if isinstance(x, np.ndarray) else int(x) for x in r) for r in a]


# ---- lzop ---------------------------------------------------------------------------------------------------------------

LZOP_STORED_LENGTHS = range(1, 49)


class _LzopTable:
    def __init__(self):
        self.src, self.entries, self.units, self.dst = bytearray(), [], [], 0

    def add(self, name, stream, dst_len, status, out, gap=0, untouched=False, src_off=None, dst_off=None, **fields):
        self.dst += gap                 # the gap in front of the slot is guard: nothing may change there
        off = self.dst if dst_off is None else dst_off
        e = {"src_off": len(self.src) if src_off is None else src_off, "dst_off": off, "src_len": len(stream), "dst_len": dst_len}
        e.update(fields)
        self.entries.append(e)
        self.src += stream
        in_dst = dst_off is None
        self.units.append(Unit(name, LO.ST[status], out, (off, dst_len) if in_dst else None, untouched=untouched))
        if in_dst:
            self.dst += dst_len


def _lzop_table(entries):
    t = np.zeros(len(entries), dtype=N.LZOP_BLOCK_DTYPE)
    for i, e in enumerate(entries):
        t[i] = (e["src_off"], e["dst_off"], e["src_len"], e["dst_len"], e.get("flags", 0), e.get("sum_c", 0), e.get("sum_u", 0), 0)
    return t


@functools.lru_cache(maxsize=None)
def lzop_call():
    """768 stored blocks -- every length 1 .. 48 at every residue 0 .. 15 of its address in d_dst, 0 to 15 bytes of guard
    in front of each -- then the failing streams, each packed directly in front of a good block, the refusals and the sums"""
    t = _LzopTable()
    seen = set()
    for residue in range(16):
        for n in LZOP_STORED_LENGTHS:
            gap = (residue - t.dst) % 16
            data = LO.noise(1000 + 16 * n + residue, n)
            t.add("stored_%d_at_%d" % (n, residue), data, n, "OK", data, gap=gap)
            seen.add((n, t.entries[-1]["dst_off"] % 16))
    assert seen == {(n, r) for n in LZOP_STORED_LENGTHS for r in range(16)} and len(t.entries) == 768
    rc = LO.rules_cases()
    good_stream, good_len, verdict, good_plain = rc["overlap_chain"]
    assert verdict == "OK" and LO.decode(good_stream, good_len)[:2] == ("OK", good_plain) and len(good_stream) < good_len

    def good(name):
        t.add("good_behind_" + name, good_stream, good_len, "OK", good_plain)

    def failing(name, stream, dst_len):
        verdict, out, _ = LO.decode(stream, dst_len)
        assert len(stream) < dst_len, name      # (the ABI refuses a stream longer than its bytes and copies one as long)
        t.add(name, stream, dst_len, verdict, out)
        good(name)
        return verdict

    for want in ("OUTPUT_OVERRUN", "LOOKBEHIND", "INPUT_OVERRUN", "SHORT_OUTPUT"):
        names = [k for k, c in sorted(rc.items()) if c[2] == want and len(c[0]) < c[1]]
        assert names, want
        for name in names:
            assert failing(name, rc[name][0], rc[name][1]) == want and LO.decode(rc[name][0], rc[name][1])[1] == rc[name][3]
    # hand-built: what crosses dst_len, and what ends exactly on it
    e = LO.Emitter().first_literals(LO.noise(1, 20)).m3(7, 200).literals(LO.noise(2, 30)).end()
    assert failing("literal_run_crosses_dst_len", e.stream(), 235) == "OUTPUT_OVERRUN"
    e = LO.Emitter().first_literals(LO.noise(3, 10)).m3(3, 100).end()
    assert failing("overlapping_match_crosses_dst_len", e.stream(), 60) == "OUTPUT_OVERRUN"
    e = LO.Emitter().first_literals(LO.noise(3, 10)).m3(3, 100).end()
    verdict, out, _ = LO.decode(e.stream(), 110)
    assert verdict == "OK" and out == bytes(e.plain) and len(out) == 110
    t.add("match_ends_on_dst_len", e.stream(), 110, "OK", out)
    good("match_ends_on_dst_len")
    # not decoded: a wrong sum over the compressed bytes; refused: outside the source, outside d_dst, longer than its bytes
    t.add("bad_sum_c", good_stream, good_len, "BAD_SUM_C", b"", untouched=True, flags=LO.C_ADLER32, sum_c=zlib.adler32(good_stream) ^ 1)
    good("bad_sum_c")
    t.add("bad_sum_c_crc32", good_stream, good_len, "BAD_SUM_C", b"", untouched=True, flags=LO.C_CRC32, sum_c=zlib.crc32(good_stream) ^ 0x80000000)
    t.add("refused_src_outside", b"", good_len, "REFUSED", b"", untouched=True, src_off=1 << 40, src_len=len(good_stream))
    t.add("refused_longer_than_its_bytes", good_stream, len(good_stream) - 1, "REFUSED", b"", untouched=True)
    good("refusals")
    # the sums over the decoded bytes: the finish kernel runs
    t.add("sum_u_adler32", good_stream, good_len, "OK", good_plain, flags=LO.U_ADLER32, sum_u=zlib.adler32(good_plain))
    t.add("sum_u_crc32", good_stream, good_len, "OK", good_plain, flags=LO.U_CRC32 | LO.C_ADLER32, sum_u=zlib.crc32(good_plain), sum_c=zlib.adler32(good_stream))
    t.add("bad_sum_u", good_stream, good_len, "BAD_SUM_U", good_plain, flags=LO.U_ADLER32, sum_u=zlib.adler32(good_plain) ^ 1)
    good("sums")
    total = t.dst
    t.add("refused_dst_outside", good_stream, good_len, "REFUSED", b"", untouched=True, dst_off=total - good_len + 1)
    t.add("refused_dst_far_outside", good_stream, good_len, "REFUSED", b"", untouched=True, dst_off=1 << 40)
    call = Call("lzop", "lzop", t.src, _lzop_table(t.entries), total, t.units)
    assert call.statuses() == {LO.ST[s] for s in ("OK", "OUTPUT_OVERRUN", "LOOKBEHIND", "INPUT_OVERRUN", "SHORT_OUTPUT", "BAD_SUM_C", "BAD_SUM_U", "REFUSED")}
    return call


# ---- uu -----------------------------------------------------------------------------------------------------------------

def residue_stream_lines():
    return U.residue_stream(b"\n", 5)


def uu_group_paths(stream, final=True):
    """which way uu_decode_kernel takes for each group of UU_LINES_PER_GROUP lines, by the group's source span from the
    16-byte grid in front of its first line (csrc/la_uu.hip: s1 - a0 > UU_SRC_LDS)"""
    lines = U.lines_of(stream, final)
    out = []
    for g in range(0, len(lines), UU_LINES_PER_GROUP):
        group = lines[g:g + UU_LINES_PER_GROUP]
        a0, s1 = group[0][0] & ~15, group[-1][0] + group[-1][1]
        out.append("global" if s1 - a0 > UU_SRC_LDS else "lds")
    return out


def _uu_call(name, stream, state=U.FIND_HEAD, decoded=False, final=True):
    w = U.walk(stream, state, decoded, final)
    unit = Unit("window", w.status, w.out, (0, len(w.out)))
    # dst_cap >= src_bytes "always suffices and is required"
    return Call("uu", name, stream, None, len(stream), [unit], state=state, decoded=decoded, final=final, walk=w)


@functools.lru_cache(maxsize=None)
def uu_calls():
    calls = []
    for total in range(0, 49):      # every decoded total 0 .. 48, so that the output ends at every residue
        data = U.randbytes(total, total)
        calls.append(_uu_call("uuencode_%d" % total, U.uu_section(data, per_line=45)))
        calls.append(_uu_call("base64_%d" % total, U.b64_section(data, per_line=57)))
        assert calls[-2].opts["walk"].out == data and calls[-1].opts["walk"].out == data
        assert calls[-2].opts["walk"].status == calls[-1].opts["walk"].status == U.ST_OK
    # every group of 256 lines starts its output at another residue
    s = residue_stream_lines()
    c = _uu_call("residues", s, U.READ_BASE64)
    lines = U.lines_of(s)
    starts, at = set(), 0
    for i, (a, n, nl) in enumerate(lines):
        if i % UU_LINES_PER_GROUP == 0:
            starts.add(at % 16)
        nxt, what = U.line_step(U.READ_BASE64, s[a:a + n - nl], nl)
        assert nxt == U.READ_BASE64
        at += len(what)
    assert at == len(c.opts["walk"].out) and len(starts) >= 3 and c.opts["walk"].status == U.ST_OK
    calls.append(c)
    # 300 base64 lines of 100 characters: the first group's source is above UU_SRC_LDS (global), the second's is not
    body = b"".join(base64.b64encode(U.randbytes(100 + i, 75)) + b"\n" for i in range(300))
    c = _uu_call("lines_of_100", body, U.READ_BASE64)
    assert uu_group_paths(body) == ["global", "lds"] and len(c.opts["walk"].out) == 300 * 75
    calls.append(c)
    # one line of 32 767 bytes (its line end included) between short ones
    long_line = base64.b64encode(U.randbytes(7, 24576))[:32766]
    s = b"begin-base64 644 long\n" + base64.b64encode(b"in front") + b"\n" + long_line + b"\n" + base64.b64encode(b"behind it") + b"\n====\n"
    c = _uu_call("line_of_32767", s)
    assert uu_group_paths(s) == ["global"] and c.opts["walk"].status == U.ST_OK and len(c.opts["walk"].out) > 24000
    calls.append(c)
    # the walk stops at line 300 of 600: the lines behind it hold decodable text and nothing of it may be written
    good = [base64.b64encode(U.randbytes(500 + i, 45)) + b"\n" for i in range(600)]
    s = b"".join(good[:300]) + b"QUJD*UJD\n" + b"".join(good[301:])
    c = _uu_call("stops_at_line_300", s, U.READ_BASE64)
    w = c.opts["walk"]
    assert w.status == U.ST_BAD_LINE and len(w.out) == 300 * 45 and w.stop_off == 300 * 61 and len(U.lines_of(s)) == 600
    calls.append(c)
    # a window that goes on, its last line still open
    s = U.b64_section(U.randbytes(9, 500), end=None) + b"QUJDRUZH"
    c = _uu_call("open_tail", s, final=False)
    w = c.opts["walk"]
    assert w.status == U.ST_OK and w.consumed == len(s) - 8 and len(w.out) == 500
    calls.append(c)
    s = U.uu_section(U.randbytes(10, 100), zero_line=None) + U.uu_line(b"no line end yet")[:-1]
    c = _uu_call("open_tail_uuencode", s, final=False)
    assert c.opts["walk"].status == U.ST_OK and len(c.opts["walk"].out) == 100 and c.opts["walk"].state == U.READ_UU
    calls.append(c)
    assert {c.opts["walk"].status for c in calls} == {U.ST_OK, U.ST_BAD_LINE}
    paths = {p for c in calls for p in uu_group_paths(c.src, c.opts["final"])}
    assert paths == {"lds", "global"}
    assert {len(c.opts["walk"].out) for c in calls} >= set(range(49))
    return calls


def uu_record_check(call, r):
    """the rest of the result record against the oracle (r: the record as a dict of ints)"""
    w = call.opts["walk"]
    got = (r["state"], r["decoded"], r["n_headers"], r["consumed"], r["stop_off"])
    assert got == (w.state, int(w.decoded), w.n_headers, w.consumed, w.stop_off), (call.name, got)
    if w.n_headers:
        assert (r["head_off"], r["head_len"]) == (w.head_off, w.head_len), call.name


# ---- the LZMA plan of the xz and lzip tables ----------------------------------------------------------------------------

PLAN_HEAD = b"8 bytes."
PLAN_PACKETS = XB.literals(PLAN_HEAD) + [XB.Match(1, 273), XB.Rep(0, 273)]
PLAN_TAIL = XS.noise(21, 300)
PLAN_TOTAL = 8 + 273 + 273 + 300
# the cut falls on a literal, inside the match, inside the rep and inside the 300 bytes behind them
PLAN_CUTS = (0, 1, 7, 8, 9, 280, 281, 282, 554, 555, PLAN_TOTAL - 1)


# ---- lzip ---------------------------------------------------------------------------------------------------------------

def _lzip_table(entries):
    t = np.zeros(len(entries), dtype=N.LZIP_MEMBER_DTYPE)
    for i, e in enumerate(entries):
        t[i] = (e["src_off"], e.get("src_end", N.LA_LZIP_UNKNOWN), e.get("data_size", N.LA_LZIP_UNKNOWN), e["dst_off"], e["dst_cap"],
                e.get("dict_size", 1 << 20), e.get("crc32", 0), N.LA_LZIP_HAS_CRC if "crc32" in e else 0, 0)
    return t


@functools.lru_cache(maxsize=None)
def lzip_call():
    src, entries, units = bytearray(), [], []
    dst = 0

    def add(name, raw, status, out, dst_cap, untouched=False, in_dst=True, **fields):
        nonlocal dst
        e = {"src_off": len(src), "dst_off": dst, "dst_cap": dst_cap}
        e.update(fields)
        entries.append(e)
        src.extend(raw)
        units.append(Unit(name, LS.ST[status], out, (e["dst_off"], dst_cap) if in_dst else None, untouched=untouched))
        if in_dst:
            dst += dst_cap

    # 48 members of 1 .. 48 bytes back to back, dst_cap == their length: with the trailer's end, size and CRC, and with
    # both ends unknown
    for known in (True, False):
        for n in range(1, 49):
            p = LS.noise(300 + n, n, 7 if n % 2 else 256)
            raw = LS.raw_lzma1(p)
            assert LS.expected_stream_result(raw, 20, n)[:2] == ("OK", p)
            at = len(src)
            kw = {"src_end": at + len(raw), "data_size": n, "crc32": zlib.crc32(p)} if known else {}
            add("member_%d_%s" % (n, "known" if known else "unknown"), raw, "OK", p, n, **kw)
    # the plan: dst_cap cuts it (OUT_FULL), a tentative size one short cuts it (SIZE_OVER)
    raw = LS.StreamWriter().put(PLAN_PACKETS + XB.literals(PLAN_TAIL) + [LS.Marker(2)]).raw()
    st, plain, _ = LS.expected_stream_result(raw, 20, PLAN_TOTAL)
    assert st == "OK" and len(plain) == PLAN_TOTAL and plain[:8] == PLAN_HEAD and plain[8:554] == b"." * 546
    for cap in PLAN_CUTS:
        st, out, _ = LS.expected_stream_result(raw, 20, cap)
        assert st == "OUT_FULL" and out == plain[:cap]
        add("plan_cap_%d" % cap, raw, "OUT_FULL", out, cap)
    add("plan_whole", raw, "OK", plain, PLAN_TOTAL)
    for size in (PLAN_TOTAL - 1, 281, 9):       # the tentative size is "bounded by data_size instead of dst_cap"
        add("plan_size_%d" % size, raw, "SIZE_OVER", plain[:size], PLAN_TOTAL, data_size=size)
    add("plan_behind_the_cuts", raw, "OK", plain, PLAN_TOTAL, data_size=PLAN_TOTAL, crc32=zlib.crc32(plain))
    # refused, and a wrong CRC: the bytes are all there
    add("refused_src_outside", b"", "REFUSED", b"", 64, untouched=True, src_off=1 << 40)
    add("refused_size_above_cap", raw, "REFUSED", b"", 64, untouched=True, data_size=65)
    add("bad_crc", raw, "BAD_CRC", plain, PLAN_TOTAL, crc32=zlib.crc32(plain) ^ 1)
    add("good_behind_bad_crc", raw, "OK", plain, PLAN_TOTAL, crc32=zlib.crc32(plain))
    total = dst
    add("refused_dst_outside", raw, "REFUSED", b"", PLAN_TOTAL, untouched=True, in_dst=False, dst_off=total - PLAN_TOTAL + 1)
    add("refused_dst_far_outside", raw, "REFUSED", b"", PLAN_TOTAL, untouched=True, in_dst=False, dst_off=1 << 40)
    call = Call("lzip", "lzip", src, _lzip_table(entries), total, units)
    assert call.statuses() == {LS.ST[s] for s in ("OK", "OUT_FULL", "SIZE_OVER", "REFUSED", "BAD_CRC")}
    return call


# ---- xz, no chains --------------------------------------------------------------------------------------------------------

XZ_ST = {"OK": 0, "DATA": N.LA_ST_XZ_DATA, "LZMA": N.LA_ST_XZ_LZMA, "TRUNCATED": N.LA_ST_XZ_TRUNCATED, "SIZE": N.LA_ST_XZ_SIZE,
         "BAD_CHECK": N.LA_ST_XZ_BAD_CHECK, "PADDING": N.LA_ST_XZ_PADDING, "OUT_FULL": N.LA_ST_XZ_OUT_FULL}


def _xz_table(entries):
    t = np.zeros(len(entries), dtype=N.XZ_BLOCK_DTYPE)
    for i, e in enumerate(entries):
        t[i] = (e["src_off"], e.get("comp_size", N.LA_XZ_UNKNOWN), e.get("uncomp_size", N.LA_XZ_UNKNOWN), e["dst_off"], e["dst_cap"],
                e.get("check_off", N.LA_XZ_UNKNOWN), e.get("dict_size", 1 << 23), e.get("check_id", 0))
    return t


def liblzma_bytes(image, **kw):
    """(every byte liblzma's decoder produces for `image` in front of its error or its end, ended well): Python's lzma
    asked for one byte at a time, so that nothing liblzma had produced is lost with the exception"""
    d = lzma.LZMADecompressor(**kw)
    out = bytearray()
    try:
        out += d.decompress(image, 1)
        while not d.eof:
            got = d.decompress(b"", 1)
            if not got and d.needs_input:
                break
            out += got
    except lzma.LZMAError:
        return bytes(out), False
    return bytes(out), d.eof


def liblzma_block(raw, n, **header):
    """what liblzma's stream decoder gives for raw LZMA2 data as the one block of a stream whose index says n bytes"""
    img = XB.stream([XB.block(raw, bytes(n), XB.CHECK_NONE, comp=False, uncomp="uncomp_value" in header, **header)], XB.CHECK_NONE)
    return liblzma_bytes(img, format=lzma.FORMAT_XZ)


class _XzTable:
    def __init__(self):
        self.src, self.entries, self.units, self.chains, self.dst = bytearray(), [], [], [], 0

    def add(self, name, raw, status, out, dst_cap, untouched=False, in_dst=True, chain=(), expect_len="exact", **fields):
        e = {"src_off": len(self.src), "dst_off": self.dst, "dst_cap": dst_cap}
        e.update(fields)
        self.entries.append(e)
        self.chains.append(list(chain))
        self.src += raw + bytes(-len(raw) % 4)      # the block padding; no check field (check_id 0)
        self.units.append(Unit(name, XZ_ST[status], out, (e["dst_off"], dst_cap) if in_dst else None, untouched=untouched, expect_len=expect_len))
        if in_dst:
            self.dst += dst_cap


@functools.lru_cache(maxsize=None)
def xz_call():
    t = _XzTable()
    # 48 sized blocks of 1 .. 48 bytes, dst_cap == their length; the same without a size at dst_cap = length, + 1, + 64 in turn
    for sized in (True, False):
        for n in range(1, 49):
            p = XS.noise(400 + n, n, 5 if n % 2 else 256)
            raw = XB.lzma2(p)
            assert liblzma_block(raw, n) == (p, True)
            if sized:
                t.add("sized_%d" % n, raw, "OK", p, n, uncomp_size=n, comp_size=len(raw))
            else:
                kw = {"comp_size": len(raw)} if n % 2 else {}
                t.add("sizeless_%d" % n, raw, "OK", p, n + (0, 1, 64)[n % 3], **kw)
    # the plan: eight literals, a match and a rep of 273, a stored chunk of 300
    w = XB.Lzma2Writer().lzma_chunk(0xE0, PLAN_PACKETS).raw_chunk(2, PLAN_TAIL)
    raw, plain = w.image(), w.plain()
    assert liblzma_block(raw, PLAN_TOTAL) == (plain, True) and len(plain) == PLAN_TOTAL and plain[8:554] == b"." * 546 and plain[554:] == PLAN_TAIL
    for cap in PLAN_CUTS:           # "one without an uncompressed size is bounded by dst_cap (LA_ST_XZ_OUT_FULL)"
        t.add("plan_cap_%d" % cap, raw, "OUT_FULL", plain[:cap], cap)
    t.add("plan_whole", raw, "OK", plain, PLAN_TOTAL)
    # sized, the header's size one less and one more: "the data disagrees with a size of the block header"; liblzma's
    # block decoder gives the header's bytes and then its data error.  With a size one more it reports the error in the call
    # that produced the last byte, and Python's lzma drops that call's output: there the reference pins a prefix, no count
    for size in (PLAN_TOTAL - 1, PLAN_TOTAL + 1):
        ref, ended = liblzma_block(raw, size, uncomp_value=size)
        assert not ended and ref == plain[:PLAN_TOTAL - 1]
        if size < PLAN_TOTAL:
            t.add("plan_sized_%d" % size, raw, "SIZE", ref, size, uncomp_size=size)
        else:
            t.add("plan_sized_%d" % size, raw, "SIZE", plain, size, uncomp_size=size, expect_len="prefix")
    t.add("plan_behind_the_sizes", raw, "OK", plain, PLAN_TOTAL, uncomp_size=PLAN_TOTAL, comp_size=len(raw))
    # a match beyond the data in mid-block
    w = XB.Lzma2Writer().raw_chunk(1, XS.noise(22, 40)).lzma_chunk(0xC0, XB.literals(b"0123456789") + [XB.Match(51, 4)] + XB.literals(b"zz"))
    ref, ended = liblzma_block(w.image(), 64)
    assert not ended and ref == w.plain()[:50]
    t.add("match_beyond_the_data", w.image(), "LZMA", ref, 64)
    t.add("good_behind_the_match", raw, "OK", plain, PLAN_TOTAL)
    # entries that point outside either buffer, or whose header size is above the budget: "is LA_ST_XZ_SIZE and is not decoded"
    t.add("src_outside", b"", "SIZE", b"", 64, untouched=True, src_off=1 << 40)
    t.add("size_above_cap", raw, "SIZE", b"", 64, untouched=True, uncomp_size=65)
    t.add("good_behind_the_refusals", raw, "OK", plain, PLAN_TOTAL + 64)
    total = t.dst
    t.add("dst_outside", raw, "SIZE", b"", PLAN_TOTAL, untouched=True, in_dst=False, dst_off=total - PLAN_TOTAL + 1)
    t.add("dst_far_outside", raw, "SIZE", b"", PLAN_TOTAL, untouched=True, in_dst=False, dst_off=1 << 40)
    call = Call("xz", "xz", t.src, _xz_table(t.entries), total, t.units)
    assert call.statuses() == {XZ_ST[s] for s in ("OK", "OUT_FULL", "SIZE", "LZMA")}
    return call


# ---- xz with filter chains ------------------------------------------------------------------------------------------------

BCJ_NEIGHBOURS = {
    # filter: [(how block A ends, how block B begins)]: A's last bytes open a unit of the filter that B's first bytes would
    # complete, were the two one buffer
    XC.X86: [(b"\xE8" + bytes(k), bytes(4 - k) + b"\xE8\x00\x00\x00\x00") for k in range(4)],
    XC.ARM: [(b"\x10\x20\x30\xEB"[:k], b"\x10\x20\x30\xEB"[k:] + b"\x00\x00\x00\xEB") for k in (1, 2, 3)],
    XC.ARMTHUMB: [(b"\x00\xF0\x00\xF8"[:k], b"\x00\xF0\x00\xF8"[k:] + b"\x01\xF0\x02\xF8") for k in (1, 2, 3)],
    XC.POWERPC: [(b"\x48\x00\x00\x01"[:k], b"\x48\x00\x00\x01"[k:] + b"\x4B\xFF\xFF\xFD") for k in (1, 2, 3)],
    XC.SPARC: [(b"\x40\x00\x00\x00"[:k], b"\x40\x00\x00\x00"[k:] + b"\x7F\xFF\xFF\xFF") for k in (1, 2, 3)],
}


def _ia64_bundles(n):
    d = XC.dense(XC.IA64, 64, 16 * n)
    assert XC.liblzma_unfilter([(XC.IA64, 0)], d) != d
    return d


@functools.lru_cache(maxsize=None)
def xz_chains_call():
    """every block with a chain is packed against a neighbour without one, sized, dst_cap == its length: a filter that
    steps over out_len lands in the neighbour's bytes"""
    from libarchive_amd.xz import chain_table
    t = _XzTable()

    def block(name, x, chain, sized=True):
        x = bytes(x)
        raw = XB.lzma2(x, preset=0)
        want = XC.liblzma_unfilter(chain, x) if chain else x
        kw = {"uncomp_size": len(x), "comp_size": len(raw)} if sized else {}
        t.add(name, raw, "OK", want, len(x), chain=chain, **kw)
        return want

    def plain_neighbour(name, x=None):
        block("plain_behind_" + name, XC.dense(XC.X86, len(t.entries), 24) if x is None else x, [])

    changed = set()
    for fid, prop in XC.ALONE:
        for n in (0, 1, 5, 17, TILE - 1, TILE + 1, 2 * TILE + 19):
            x = XC.dense(fid, fid * 7 + n, n)
            if block("alone_%02x_%d" % (fid, n), x, [(fid, prop)], sized=n % 2 == 1) != x:
                changed.add(fid)
            plain_neighbour("alone_%02x_%d" % (fid, n))
    assert changed == {fid for fid, _ in XC.ALONE}       # every filter finds work in its buffers
    # the adversarial neighbours: A ends inside a unit of its filter, B (no chain) begins with the rest of it
    for fid, pairs in sorted(BCJ_NEIGHBOURS.items()):
        lead = XC.dense(fid, 30 + fid, 64)
        for k, (tail, head) in enumerate(pairs):
            a, b = lead + tail, head + XS.noise(k, 12)
            whole = XC.liblzma_unfilter([(fid, 0)], a + b)
            assert whole[len(a):] != b or whole[:len(a)] != XC.liblzma_unfilter([(fid, 0)], a), (fid, k)     # one buffer would come out otherwise
            block("neighbours_%02x_%d_a" % (fid, k), a, [(fid, 0)])
            block("neighbours_%02x_%d_b" % (fid, k), b, [])
    d = _ia64_bundles(12)

    def ia64_shows(cut):        # would one buffer come out otherwise than the two parts?
        whole = XC.liblzma_unfilter([(XC.IA64, 0)], d)
        return whole[cut:] != d[cut:] or whole[:cut] != XC.liblzma_unfilter([(XC.IA64, 0)], d[:cut])
    cuts = [[16 * i + k for i in range(12) if ia64_shows(16 * i + k)][:2] for k in (15, 1)]      # a bundle cut at 15 (and at 1) of its 16 bytes
    assert len(cuts[0]) == 2 and len(cuts[1]) == 2
    for cut in cuts[0] + cuts[1]:
        block("neighbours_ia64_%d_a" % cut, d[:cut], [(XC.IA64, 0)])
        block("neighbours_ia64_%d_b" % cut, d[cut:], [])
    for dist, n in ((1, 37), (256, 300), (256, 255), (4, TILE + 2)):      # delta: the length is no multiple of the distance
        a, b = XC.dense(XC.DELTA, dist, n), XC.dense(XC.DELTA, dist + 1, 40)
        assert XC.liblzma_unfilter([(XC.DELTA, dist)], a + b)[n:] != b
        block("neighbours_delta_%d_%d_a" % (dist, n), a, [(XC.DELTA, dist)])
        block("neighbours_delta_%d_%d_b" % (dist, n), b, [])
    # a failed block with a chain in front of a good block: stored chunks, eight literals, then a match beyond the data.
    # The chain is undone over the valid bytes; liblzma's BCJ decoders hold the last bytes of a buffer back until more
    # arrive or the stream ends well, so the reference pins all but the filter's look-ahead (16 bytes at most)
    for fid, prop, hold in ((XC.X86, 0, 16), (XC.DELTA, 4, 0), (XC.ARM, 0, 16)):
        f = XC.dense(fid, 90 + fid, TILE + 3000)
        w = XB.Lzma2Writer().raw_chunk(1, f).lzma_chunk(0xC0, XB.literals(b"abcdefgh") + [XB.Match(len(f) + 9, 4)] + XB.literals(b"zz"))
        valid = f + b"abcdefgh"
        want = XC.liblzma_unfilter([(fid, prop)], valid)
        assert want != valid
        t.add("lzma_error_%02x" % fid, w.image(), "LZMA", want[:len(valid) - hold], len(valid) + 40, chain=[(fid, prop)], expect_len="covers" if hold else "exact")
        good = XC.dense(fid, 5, 3000)
        block("good_behind_lzma_error_%02x" % fid, good, [(fid, prop)])
    # a chain the ABI refuses: its block's slot is untouched
    x = XC.dense(XC.X86, 2, 500)
    for name, chain in (("delta_0", [(XC.DELTA, 0)]), ("arm_offset_2", [(XC.ARM, 2)]), ("unknown_id", [(0x0A, 0)])):
        t.add("refused_chain_" + name, XB.lzma2(x, preset=0), "SIZE", b"", len(x), untouched=True, chain=chain)
        plain_neighbour("refused_chain_" + name)
    call = Call("xz_chains", "xz_chains", t.src, _xz_table(t.entries), t.dst, t.units, chains=chain_table(t.chains), chain_lists=t.chains)
    assert call.statuses() == {XZ_ST[s] for s in ("OK", "LZMA", "SIZE")}
    return call


# ---- bzip2 ----------------------------------------------------------------------------------------------------------------

BZ2_ST = {"OK": 0, "DATA": N.LA_ST_BZ2_DATA, "TRUNCATED": N.LA_ST_BZ2_TRUNCATED, "BAD_CRC": N.LA_ST_BZ2_BAD_CRC, "REFUTED": N.LA_ST_BZ2_REFUTED}
BZ2_GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "bzip2_handbuilt.json")


def _bz2_call(name, built, dst_total, dst_cap=None, n_emit=None, fails=None, unconfirmed_from=None):
    """One MEASURE + EMIT over every magic of the image.  The blocks are packed by the prefix sum of their lengths; one is
    emitted when its index is below n_emit and its packed end lies inside dst_cap.  `fails`: (index among the stream's own
    units, status) of the block that fails behind its bytes; the blocks behind it may or may not be expanded (the
    header promises neither), so their slots are free.  `unconfirmed_from`: the walk ends in that unit (a data error in
    MEASURE); it and everything behind it produce nothing."""
    import bzip2_support as BS
    magics = BS.find_magics(built.image)
    cands = np.zeros(len(magics), dtype=N.BZ2_CAND_DTYPE)
    for i, (bit, kind) in enumerate(magics):
        cands[i] = (bit, kind, 0)
    n = len(magics)
    dst_cap = dst_total if dst_cap is None else dst_cap
    n_emit = n if n_emit is None else n_emit
    units, off, failed = [], 0, False
    for i, m in enumerate(magics):
        if m not in built.marks:
            units.append(Unit("planted_%d" % i, BZ2_ST["REFUTED"], b"", None, untouched=True))
            continue
        k = built.marks.index(m)
        if unconfirmed_from is not None and k >= unconfirmed_from:
            units.append(Unit("unit_%d" % k, BZ2_ST["DATA" if k == unconfirmed_from else "REFUTED"], b"", None, untouched=True))
            continue
        if m[1] == 1:
            units.append(Unit("end_%d" % k, BZ2_ST["OK"], b"", None, untouched=True))
            continue
        plain = built.plains[k]
        emitted = i < n_emit and off + len(plain) <= dst_cap
        if failed and emitted:
            units.append(Unit("block_%d" % k, BZ2_ST["OK"], b"", (off, len(plain)), expect_len=None))
        elif emitted:
            status = fails[1] if fails and fails[0] == k else "OK"
            units.append(Unit("block_%d" % k, BZ2_ST[status], plain, (off, len(plain))))
            failed = failed or status != "OK"
        else:
            units.append(Unit("block_%d" % k, BZ2_ST["OK"], b"", None, untouched=True, expect_len=None))
        off += len(plain)
    assert off <= dst_total or unconfirmed_from is not None
    return Call("bzip2", name, built.image, cands, dst_total, units, dst_cap=dst_cap, n_emit=n_emit)


@functools.lru_cache(maxsize=None)
def bzip2_calls():
    import bz2
    import hashlib
    import bzip2_build as B
    # one stream: 40 blocks of 1 .. 40 bytes, a block whose surplus selectors spell both magics (refuted candidates between
    # confirmed ones), a block that ends in a run of 4 + 255
    blocks = [B.Block(B.text(500 + n, n)) for n in range(1, 41)]
    blocks.insert(20, B.Block(B.text(70, 30), ntables=4, surplus=B._planted(0)))
    blocks.append(B.Block(B.text(71, 25) + b"Q" * 4 + b"\xff"))
    blocks.append(B.Block(B.text(72, 7)))
    s = B.build(blocks)
    plain = b"".join(s.plains)
    assert bz2.decompress(s.image) == plain and s.plains[-2].endswith(b"Q" * 259) and [len(p) for p in s.plains[:20]] == list(range(1, 21))
    total = len(plain)
    calls = [_bz2_call("all", s, total), _bz2_call("cap_one_short", s, total, dst_cap=total - 1), _bz2_call("cap_0", s, total, dst_cap=0),
             _bz2_call("cap_inside_the_long_run", s, total, dst_cap=total - 100)]
    n = len(calls[0].units)
    calls.append(_bz2_call("n_emit_n_minus_3", s, total, n_emit=n - 3))
    calls.append(_bz2_call("n_emit_0", s, total, n_emit=0))
    assert BZ2_ST["REFUTED"] in calls[0].statuses() and sum(1 for u in calls[1].units if u.expect_len is None) == 1
    assert sum(1 for u in calls[3].units if u.expect_len is None) == 2 and sum(1 for u in calls[4].units if u.expect_len is None) >= 1
    # four equal bytes without their count, in front of a good block: libbz2 makes a count up, writes the run and fails
    with open(BZ2_GOLDEN) as f:
        gold = {r["name"]: r for r in json.load(f)}["missing-count-one-block"]
    s = B.build([B.Block(B.text(66, 30) + b"Q" * 4), B.Block(B.text(67, 40))])
    assert hashlib.sha256(s.plains[0]).hexdigest() == gold["written_sha256"] and gold["libbz2"] == "data" and len(s.plains[0]) > 34
    calls.append(_bz2_call("missing_count", s, len(s.plains[0]) + 40 + 64, fails=(0, "DATA")))
    calls[-1].opts["stand_in_models_it"] = False     # (tests/mock_gpu/la_gpu_bzip2_mock.c takes the block's length from one libbz2 call: a byte short here)
    # a block MEASURE refuses: it, the block behind it and the end of stream produce nothing
    bad = B.Block(B.text(60, 30), ntables_field=0)
    bad.refused = True
    s = B.build([B.Block(B.text(73, 33)), bad, B.Block(B.text(74, 50))])
    calls.append(_bz2_call("unconfirmed", s, 33 + 50 + 64, unconfirmed_from=1))
    assert {st for c in calls for st in c.statuses()} == {BZ2_ST[k] for k in ("OK", "REFUTED", "DATA")}
    return calls
