"""la_gpu_uu_decode on the device (csrc/la_uu.hip) against the oracle (uu_support.walk): status, out_len, consumed,
state, stop offset, the accepted header and the bytes, for single lines at their edges, lines at every residue of the
kernels' tiles, one line per byte, random multi-section streams and windows that go on."""
import base64
import random

import numpy as np
import pytest

import uu_support as U

pytestmark = pytest.mark.gpu

TILE, LINES_PER_GROUP = 4096, 256      # csrc/la_uu.hip: UU_TILE, UU_LPB


class Device:
    """one context, buffers kept between the calls"""

    def __init__(self, ctx):
        import torch
        from libarchive_amd import uu
        self.torch, self.uu, self.ctx = torch, uu, ctx
        self.cap = 1 << 20
        self.d_src = torch.zeros(self.cap, dtype=torch.uint8, device="cuda")
        self.d_dst = torch.zeros(self.cap, dtype=torch.uint8, device="cuda")

    def run(self, window, state=U.FIND_HEAD, decoded=False, final=True):
        n = len(window)
        assert n <= self.cap
        if n:
            self.d_src[:n].copy_(self.torch.from_numpy(np.frombuffer(bytes(window), dtype=np.uint8).copy()))
            self.torch.cuda.synchronize()       # (the context runs on a stream of its own)
        plan = self.uu.UuDevicePlan(self.ctx, self.d_src[:n], self.d_dst).run(state, decoded, final)
        r = plan.result()
        return r, plan.output(r["out_len"])

    def check(self, window, state=U.FIND_HEAD, decoded=False, final=True):
        r, out = self.run(window, state, decoded, final)
        w = U.walk(window, state, decoded, final)
        got = (int(r["status"]), int(r["state"]), int(r["decoded"]), int(r["n_headers"]), int(r["out_len"]), int(r["consumed"]), int(r["stop_off"]))
        assert got == (w.status, w.state, int(w.decoded), w.n_headers, len(w.out), w.consumed, w.stop_off), (bytes(window[:80]), state, final)
        assert out == w.out
        if w.n_headers:
            assert (int(r["head_off"]), int(r["head_len"])) == (w.head_off, w.head_len)
        return w


@pytest.fixture(scope="module")
def dev(gpu_ctx):
    return Device(gpu_ctx)


def test_every_uuencode_length_character(dev):
    """0x20 .. 0x60 with a body of exactly, one fewer than and one more than the characters the count needs; a checksum
    and padding characters behind them; '`' and the blank as zero"""
    seen = set()
    for lc in range(0x20, 0x61):
        l = U.uudec(lc)
        need = 4 * (l // 3) + (l % 3 + 1 if l % 3 else 0)
        chars = U.uu_body(U.randbytes(lc, 63), zero=0x60 if lc & 1 else 0x20)
        for body in (chars[:need], chars[:max(need - 1, 0)], chars[:need] + b"A", chars[:need] + b"z", chars[:need] + b"Kzz~", chars[:l], chars[:max(l - 1, 0)]):
            w = dev.check(bytes([lc]) + body + b"\n" + (U.uu_line(b"abc") if l else b"end\n"), U.READ_UU)
            seen.add(w.status)
    assert seen == {U.ST_OK, U.ST_BAD_LINE}
    dev.check(b"`\nend\n", U.READ_UU)
    dev.check(b" \nend\n", U.READ_UU)
    dev.check(b"`\nend", U.READ_UU)
    dev.check(b"`\nEND\n", U.READ_UU)


def test_base64_bodies_of_0_to_80_characters(dev):
    """'=' and an invalid character at every position of the last group"""
    seen = set()
    for n in range(0, 81):
        body = base64.b64encode(U.randbytes(n, 60))[:n]
        cases = [body]
        for k in range(1, min(n, 4) + 1):
            cases += [body[:n - k] + b"=" + body[n - k + 1:], body[:n - k] + b"*" + body[n - k + 1:], body[:n - k] + b"=" * k]
        for c in cases:
            w = dev.check(c + b"\n" + base64.b64encode(b"tail of the window") + b"\n", U.READ_BASE64)
            seen.add(w.status)
    assert seen == {U.ST_OK, U.ST_BAD_LINE}
    for body in (b"===", b"====", b"===x", b"==", b"="):
        dev.check(body + b"\nbegin 644 next\n" + U.uu_line(b"xyz"), U.READ_BASE64)


def test_long_base64_lines(dev):
    head = b"begin-base64 644 long\n"
    for n in (4096, 32767, 32769):        # bytes of the line, its line end included
        body = base64.b64encode(U.randbytes(n, 24576))[:n - 1]
        w = dev.check(head + base64.b64encode(b"in front") + b"\n" + body + b"\n" + base64.b64encode(b"behind") + b"\n====\n")
        assert w.status == (U.ST_TOO_LONG if n > 32768 else U.ST_OK)
    # a line that fills whole tiles while looking for a head, clean and with a bad byte in a tile of its own
    for n in (131071, 131072):
        assert dev.check(b"j" * (n - 1) + b"\n" + U.uu_section(b"abc")).status == (U.ST_OK if n < 131072 else U.ST_TOO_LONG)
    assert dev.check(b"j" * 70000 + b"\x80" + b"j" * 70000 + b"\n").status == U.ST_BAD_BYTE_HEAD
    assert dev.check(b"j" * 70000 + b"\x80" + b"j" * 70000 + b"\n", decoded=True).status == U.ST_IGNORED


@pytest.mark.parametrize("style", [b"\n", b"\r\n", b"\r", b"mixed"])
def test_line_starts_at_every_residue(dev, style):
    s = U.residue_stream(style, 5)
    assert len(s) > 3 * TILE and len(U.lines_of(s)) > 3 * LINES_PER_GROUP
    w = dev.check(s, U.READ_BASE64)
    assert w.status == U.ST_OK and len(w.out) > 15000
    for lead in range(1, 17):       # the same lines at every offset inside the 16-byte loads
        dev.check(b"j" * (lead - 1) + b"\n" + b"begin-base64 644 r\n" + s[:3000], U.FIND_HEAD)


@pytest.mark.parametrize("state", [U.FIND_HEAD, U.READ_UU, U.UUEND, U.READ_BASE64])
def test_one_line_per_byte(dev, state):
    w = dev.check(b"\n" * 65536, state)
    assert w.status == {U.FIND_HEAD: U.ST_OK, U.READ_BASE64: U.ST_OK, U.READ_UU: U.ST_BAD_LINE, U.UUEND: U.ST_BAD_END}[state]
    assert w.consumed == (65536 if w.status == U.ST_OK else 0)
    dev.check(b"\r" * 4097, state, final=False)
    dev.check(b"\r\n" * 3000 + b"\r", state, final=False)


def random_stream(r, limit, edge_line=None):
    out = bytearray()

    def lines():
        return len(U.lines_of(bytes(out)))
    if edge_line is not None:       # junk up to the line in front of a group's first or last line, then a header there
        while lines() < edge_line:
            out.extend(U.junk(r.randrange(1 << 30), 1, nl=r.choice([b"\n", b"\r\n"])))
    while len(out) < limit:
        kind = r.randrange(10)
        nl = r.choice([b"\n", b"\n", b"\r\n", b"\r"])
        data = r.randbytes(r.choice([0, 1, 44, 45, 46, 57, 100, 700, 3000]))
        if kind < 3:
            out += U.uu_section(data, name=b"n%d" % r.randrange(100), mode=r.randrange(512), nl=nl, zero=r.choice([0x20, 0x60]),
                                zero_line=r.choice([b"`", b" ", b"`", None]))
        elif kind < 6:
            out += U.b64_section(data, name=b"n%d" % r.randrange(100), mode=r.randrange(512), nl=nl, end=r.choice([b"====", b"===", b"====", None]))
        elif kind < 8:
            out += U.junk(r.randrange(1 << 30), r.randrange(1, 12), nl=nl)
        elif kind == 8 and out:
            at = r.randrange(len(out))      # damage: a byte of any class
            out[at] = r.choice([0x00, 0x80, 0xFF, 0x7F, 0x2A, 0x3D, 0x60, 0x61, 0x0A, 0x0D, 0x20])
        else:
            out += r.choice([b"end\n", b"`\n", b"====\n", b"begin 644 \n", b"begin 644 ab\n", b"begin-base64 644 ab\r\n", b"\n", b"\r"])
    return bytes(out[:limit])


@pytest.mark.parametrize("part", range(3))
def test_300_random_streams(dev, part):
    """100 streams per case: eight with a section change on the first or the last line of a group of lines, two of
    64 KiB, the others short"""
    r = random.Random(300 + part)
    statuses = set()
    for i in range(100):
        if i < 8:
            s = random_stream(r, 16000, edge_line=LINES_PER_GROUP * (1 + i % 2) - (i // 2) % 2)
        else:
            s = random_stream(r, 65536 if i % 50 == 49 else r.randrange(1, 3000))
        w = dev.check(s, final=bool(i % 3))
        statuses.add(w.status)
    assert statuses >= {U.ST_OK, U.ST_BAD_BYTE_HEAD, U.ST_IGNORED, U.ST_BAD_BYTE, U.ST_BAD_LINE, U.ST_UNTERMINATED}


def test_windows_that_go_on(dev):
    """a tail without a line end, one that ends in '\\r', one that is a complete `end`: left to the next window, or judged
    when the window ends the stream"""
    body = U.uu_section(U.randbytes(8, 500))
    uu_head = body[:body.rindex(b"`\n")]
    b64_head = U.b64_section(U.randbytes(9, 500), end=None)
    cases = [(uu_head, U.uu_line(b"no line end")[:-1]), (uu_head, U.uu_line(b"a cr")[:-1] + b"\r"), (uu_head + b"`\n", b"end"),
             (uu_head + b"`\n", b"en"), (uu_head + b"`\n", b"end\r"), (U.junk(1, 5), b"begin 644 name"), (b64_head, b"QUJD"), (b64_head, b"QUJD\r")]
    for front, tail in cases:
        w = dev.check(front + tail, final=False)
        assert w.status == U.ST_OK and w.consumed == len(front)
        dev.check(tail, w.state, decoded=w.decoded, final=False)
        dev.check(front + tail, final=True)
        dev.check(tail, w.state, decoded=w.decoded, final=True)
    assert dev.check(body[:-1], final=True).state == U.FIND_HEAD       # a complete `end` ends a final window
    assert dev.check(body[:-1], final=False).state == U.UUEND
    assert dev.check(b"", final=True).status == U.ST_OK
    assert dev.check(b"x", final=False).consumed == 0
