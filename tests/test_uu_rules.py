"""The uu read filter's rules, twice: the oracle (tests/uu_support.py, the reference's state machine in Python) against
Python's own uuencode and base64 codecs on valid text, and the rules header the kernels compile
(libarchive_amd/csrc/la_uu_dev.h, called through the CPU stand-in's entry) against the oracle line by line."""
import base64
import binascii
import ctypes as C
import random

import pytest

import uu_mock_build as mock_build
import uu_support as U


@pytest.mark.parametrize("nl", [b"\n", b"\r\n"])
@pytest.mark.parametrize("backtick", [True, False])
def test_oracle_decodes_what_binascii_writes(nl, backtick):
    for n in range(0, 46):
        data = U.randbytes(100 + n, n)
        line = binascii.b2a_uu(data, backtick=backtick)[:-1] + nl
        nxt, out = U.line_step(U.READ_UU, line[:-len(nl)], len(nl))
        assert (nxt, out) == ((U.READ_UU, data) if n else (U.UUEND, b"")), n
    data = U.randbytes(7, 45 * 33 + 17)
    got = U.reference_read(U.b2a_uu_section(data, backtick, nl))
    assert got == (data, 0, "", b"py", 0o644)


@pytest.mark.parametrize("nl", [b"\n", b"\r\n"])
def test_oracle_decodes_what_base64_writes(nl):
    for n in (0, 1, 2, 3, 56, 57, 58, 1000, 5000):
        data = U.randbytes(200 + n, n)
        text = base64.encodebytes(data).replace(b"\n", nl)
        got = U.reference_read(b"begin-base64 600 b.bin" + nl + text + b"====" + nl)
        assert got == (data, 0, "", b"b.bin", 0o600), n


def rules_line():
    lib = mock_build.gpu_lib()
    f = lib.la_uu_rules_line
    f.restype = C.c_uint64
    f.argtypes = [C.c_char_p, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.c_char_p]
    return f


def header_says(f, line, nl, state, out):
    """(next state, bytes) or (STOP, status) as the oracle words it"""
    nxt, reason, nbytes = C.c_uint32(), C.c_uint32(), C.c_uint32()
    f(line, len(line), nl, state, C.byref(nxt), C.byref(reason), C.byref(nbytes), out)
    if nxt.value == U.STOP:
        assert 1 <= reason.value <= 6 and nbytes.value == 0
        return U.STOP, 49 + reason.value
    assert reason.value == 0
    return nxt.value, out.raw[:nbytes.value]


CLASSES = [bytes(range(0x20, 0x61)), U.B64_ALPHABET, b"abcdefghijklmnopqrstuvwxyz{|}~", b"=", b"`M ", bytes(range(0x20, 0x7F)),
           bytes([0, 1, 9, 0x1F, 0x7F, 0x80, 0xFF])]
STARTS = [b"", b"", b"", b"M", b"begin 644 ", b"begin-base64 600 ", b"begin 64", b"begin 648 n", b"end", b"===", b"=", b"`", b" "]


def test_header_and_oracle_agree_on_20000_random_lines():
    f = rules_line()
    out = C.create_string_buffer(256)
    r = random.Random(20240)
    seen = set()
    for i in range(20000):
        n = r.randrange(0, 91)
        weights = [6, 6, 2, 1, 1, 3, 0 if r.random() < 0.8 else 1]
        body = bytearray(r.choice(STARTS))
        while len(body) < n:
            cls = r.choices(CLASSES, weights)[0]
            body += bytes(r.choice(cls) for _ in range(r.randrange(1, 20)))
        body = bytes(body[:n])
        if r.random() < 0.3 and n:      # a line that is valid in one of the data states, cut or padded at random
            k = r.randrange(0, 46)
            body = (U.uu_line(U.randbytes(i, k), nl=b"") if r.random() < 0.5 else base64.b64encode(U.randbytes(i, k)))
            if r.random() < 0.5:
                body = body[:r.randrange(0, len(body) + 1)] + bytes(r.choice(CLASSES[5]) for _ in range(r.randrange(0, 3)))
        nl, end = r.choice([(1, b"\n"), (2, b"\r\n"), (1, b"\r"), (0, b"")])
        for state in (U.FIND_HEAD, U.READ_UU, U.UUEND, U.READ_BASE64):
            want = U.line_step(state, body, nl)
            got = header_says(f, body + end, nl, state, out)
            assert got == want, (state, body, nl)
            seen.add((state, want[0], want[1] if want[0] == U.STOP else None))
    # every transition and every reason was met
    assert {(s, n) for s, n, _ in seen if n != U.STOP} == {(0, 0), (0, 1), (0, 3), (1, 1), (1, 2), (2, 0), (3, 3), (3, 0)}
    assert {w for _, n, w in seen if n == U.STOP} == {U.ST_BAD_BYTE_HEAD, U.ST_BAD_BYTE, U.ST_BAD_LINE, U.ST_BAD_END, U.ST_UNTERMINATED}


def test_header_and_oracle_agree_at_the_length_limits():
    f = rules_line()
    out = C.create_string_buffer(32768)
    for n in (32766, 32767, 32768, 131070, 131071, 131072):
        for body in (b"j" * n, b"M" + b"A" * (n - 1), b"A" * n, b"A" * (n - 1) + b"\x80"):
            for nl, end in ((1, b"\n"), (2, b"\r\n")):
                for state in (U.FIND_HEAD, U.READ_UU, U.UUEND, U.READ_BASE64):
                    assert header_says(f, body + end, nl, state, out) == U.line_step(state, body, nl), (n, body[:2], nl, state)


def test_the_stand_ins_walk_is_the_oracles_walk():
    """la_gpu_uu_decode of the stand-in over every shape of the filter tests, whole and as a window that goes on, from
    every state"""
    lib = mock_build.gpu_lib()

    class State(C.Structure):
        _fields_ = [("state", C.c_uint32), ("decoded", C.c_uint32)]

    class Result(C.Structure):
        _fields_ = [("status", C.c_uint32), ("state", C.c_uint32), ("decoded", C.c_uint32), ("n_headers", C.c_uint32), ("out_len", C.c_uint64),
                    ("consumed", C.c_uint64), ("stop_off", C.c_uint64), ("head_off", C.c_uint64), ("head_len", C.c_uint32), ("reserved", C.c_uint32)]

    class Batch(C.Structure):
        _fields_ = [("d_src", C.c_char_p), ("src_bytes", C.c_uint64), ("final", C.c_uint32), ("reserved", C.c_uint32), ("state_in", State),
                    ("d_dst", C.c_char_p), ("dst_cap", C.c_uint64), ("d_result", C.POINTER(Result))]
    lib.la_gpu_uu_decode.argtypes = [C.c_void_p, C.POINTER(Batch)]
    for name, img in sorted(U.filter_shapes().items()):
        for final in (1, 0):
            for state in range(4):
                for decoded in (0, 1):
                    res = Result()
                    dst = C.create_string_buffer(len(img) + 1)
                    b = Batch(img, len(img), final, 0, State(state, decoded), C.cast(dst, C.c_char_p), len(img), C.pointer(res))
                    assert lib.la_gpu_uu_decode(None, C.byref(b)) == 0
                    w = U.walk(img, state, bool(decoded), bool(final))
                    got = (res.status, res.state, res.decoded, res.n_headers, res.out_len, res.consumed, res.stop_off)
                    assert got == (w.status, w.state, int(w.decoded), w.n_headers, len(w.out), w.consumed, w.stop_off), (name, final, state)
                    assert dst.raw[:res.out_len] == w.out, name
                    if w.n_headers:
                        assert (res.head_off, res.head_len) == (w.head_off, w.head_len), name
