"""TEST INFRASTRUCTURE for the uu read filter: the oracle, builders of streams, and the reference's answers.

The oracle is the reference's state machine (archive_read_support_filter_uu.c: get_line, the four states of
uudecode_filter_read, the bidder) walked over a WHOLE stream in Python, with the decisions DESIGN.md records where the
reference's own answer depends on how its input happens to be buffered:
  - every byte of the lines in front of a failing line is handed out, then the error;
  - a line of 128 KiB or more (line end included) while looking for a head, and a data line of more than 32 768 bytes,
    are "Invalid format data"; nothing else is limited;
  - "\\r\\n" is one line end wherever upstream's blocks happen to split it; `end` may be split anywhere.
It shares no code with libarchive_amd/csrc/la_uu_dev.h: the byte classes are the reference's tables, built here as sets.
"""
import base64
import binascii
import hashlib
import json
import os
import random

ARCHIVE_FILTER_UU = 7
ARCHIVE_FATAL = -30
FIND_HEAD, READ_UU, UUEND, READ_BASE64, STOP = 0, 1, 2, 3, 4
(ST_OK, ST_IGNORED, ST_BAD_BYTE_HEAD, ST_BAD_BYTE, ST_BAD_LINE, ST_BAD_END, ST_TOO_LONG, ST_UNTERMINATED) = 0, 49, 50, 51, 52, 53, 54, 55
E_INSUFFICIENT, E_MISSING, E_INVALID = "Insufficient compressed data", "Missing format data", "Invalid format data"
MESSAGE = {ST_BAD_BYTE_HEAD: E_INSUFFICIENT, ST_BAD_BYTE: E_INSUFFICIENT, ST_BAD_LINE: E_INSUFFICIENT, ST_BAD_END: E_INSUFFICIENT,
           ST_TOO_LONG: E_INVALID, ST_UNTERMINATED: E_MISSING}
MAX_HEAD_LINE, MAX_DATA_LINE, BID_MAX_READ = 131072, 32768, 128 * 1024

FIXTURE_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_fixtures", "uu")

# uu.c:101-175
ASCII = set(range(0x20, 0x7F))
UUCHAR = set(range(0x20, 0x61))
B64_ALPHABET = b"ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz0123456789+/"
BASE64 = set(B64_ALPHABET)
BASE64NUM = {c: i for i, c in enumerate(B64_ALPHABET)}


def uudec(c):
    return (c - 0x20) & 0x3F


def lines_of(stream, final=True):
    """(start, length, nl) of every line the walk may take: '\\n', '\\r\\n' and a lone '\\r' end a line; the last line of a
    final stream may lack its line end (nl = 0); in a stream that goes on, a tail without a line end, or whose only line
    end is a '\\r' in the last byte, is not a line yet"""
    n, pos, out = len(stream), 0, []
    while pos < n:
        e = pos
        while e < n and stream[e] not in (0x0A, 0x0D):
            e += 1
        if e == n:
            if final:
                out.append((pos, n - pos, 0))
            break
        if stream[e] == 0x0D:
            if e + 1 == n:
                if final:
                    out.append((pos, n - pos, 1))
                break
            nl = 2 if stream[e + 1] == 0x0A else 1
        else:
            nl = 1
        out.append((pos, e - pos + nl, nl))
        pos = e + nl
    return out


def header_kind(body):
    """uu.c:565-574: 6, 13 or 0"""
    if len(body) >= 11 and body[:6] == b"begin ":
        k = 6
    elif len(body) >= 18 and body[:13] == b"begin-base64 ":
        k = 13
    else:
        return 0
    if all(0x30 <= body[k + i] <= 0x37 for i in range(3)) and body[k + 3] == 0x20:
        return k
    return 0


def line_step(state, body, nl):
    """One line (its body, the length of its line end) in `state`: (next state, bytes) or (STOP, status-without-the-
    ignore-rule).  The order of the tests is the reference's: bad byte, missing line end, length, the state's rules."""
    length = len(body) + nl
    if any(c not in ASCII for c in body):
        return STOP, (ST_BAD_BYTE_HEAD if state == FIND_HEAD else ST_BAD_BYTE)
    if nl == 0 and state != UUEND:
        return STOP, ST_UNTERMINATED
    if state == FIND_HEAD:
        if length >= MAX_HEAD_LINE:
            return STOP, ST_TOO_LONG
        k = header_kind(body)
        return (READ_UU if k == 6 else READ_BASE64 if k == 13 else FIND_HEAD), b""
    if state == UUEND:
        return (FIND_HEAD, b"") if body == b"end" else (STOP, ST_BAD_END)
    if length > MAX_DATA_LINE:
        return STOP, ST_TOO_LONG
    out = bytearray()
    if state == READ_UU:
        if not body or body[0] not in UUCHAR:
            return STOP, ST_BAD_LINE
        l = uudec(body[0])
        b = body[1:]
        if l > len(b):
            return STOP, ST_BAD_LINE
        if l == 0:
            return UUEND, b""
        i = 0
        b = b + b"\n"      # what the reference reads behind a short body is the line end: never in uuchar[]
        while l > 0:
            if b[i] not in UUCHAR or b[i + 1] not in UUCHAR:
                break
            n = uudec(b[i]) << 18 | uudec(b[i + 1]) << 12
            i += 2
            out.append(n >> 16)
            l -= 1
            if l > 0:
                if b[i] not in UUCHAR:
                    break
                n |= uudec(b[i]) << 6
                i += 1
                out.append((n >> 8) & 0xFF)
                l -= 1
            if l > 0:
                if b[i] not in UUCHAR:
                    break
                n |= uudec(b[i])
                i += 1
                out.append(n & 0xFF)
                l -= 1
        if l:
            return STOP, ST_BAD_LINE
        return READ_UU, bytes(out)
    # READ_BASE64, uu.c:668-712
    if body[:3] == b"===":
        return FIND_HEAD, b""
    b = body + b"\n"
    l, i = len(body), 0
    while l > 0:
        if b[i] not in BASE64 or b[i + 1] not in BASE64:
            break
        n = BASE64NUM[b[i]] << 18 | BASE64NUM[b[i + 1]] << 12
        i += 2
        out.append(n >> 16)
        l -= 2
        if l > 0:
            if b[i] not in BASE64:
                break
            n |= BASE64NUM[b[i]] << 6
            i += 1
            out.append((n >> 8) & 0xFF)
            l -= 1
        if l > 0:
            if b[i] not in BASE64:
                break
            n |= BASE64NUM[b[i]]
            i += 1
            out.append(n & 0xFF)
            l -= 1
    if l and b[i] != 0x3D:
        return STOP, ST_BAD_LINE
    return READ_BASE64, bytes(out)


class Walk:
    """what la_gpu_uu_decode answers for one window, and the header the host would parse"""

    def __init__(self):
        self.status, self.state, self.decoded, self.n_headers = ST_OK, FIND_HEAD, False, 0
        self.out, self.consumed, self.stop_off, self.head_off, self.head_len = b"", 0, 0, 0, 0
        self.name, self.mode = None, None


def walk(stream, state=FIND_HEAD, decoded=False, final=True):
    stream = bytes(stream)
    w = Walk()
    out = bytearray()
    pos = 0
    for start, length, nl in lines_of(stream, final):
        body = stream[start:start + length - nl]
        nxt, what = line_step(state, body, nl)
        if nxt == STOP:
            if what == ST_BAD_BYTE_HEAD and (decoded or out):
                what = ST_IGNORED
            w.status, state = what, STOP
            break
        out += what
        if state == FIND_HEAD and nxt != FIND_HEAD:
            k = header_kind(body)
            w.n_headers += 1
            w.head_off, w.head_len = start, length
            w.mode = (body[k] - 0x30) * 64 + (body[k + 1] - 0x30) * 8 + (body[k + 2] - 0x30)
            if len(body) - 4 - k > 1:
                w.name = body[k + 4:]
        state = nxt
        pos = start + length
    w.state, w.out, w.decoded = state, bytes(out), bool(decoded or out)
    w.consumed = w.stop_off = pos
    return w


def bid(image):
    """uu.c:262-359 over an upstream that hands the whole image over as one block (or, for an image below 128 KiB or one
    whose first line is the header, any blocks at all: the answer is the same)"""
    image = bytes(image)
    if not image:
        return 0
    firstline = 20
    pos = 0
    while True:
        e = pos
        while e < len(image) and image[e] not in (0x0A, 0x0D):
            if image[e] not in ASCII:
                return 0
            e += 1
        if e == len(image):
            return 0
        nl = 2 if image[e] == 0x0D and image[e + 1:e + 2] == b"\n" else 1
        k = header_kind(image[pos:e])
        pos = e + nl
        if k:
            break
        firstline = 0
        if len(image) >= BID_MAX_READ:
            return 0
    if pos == len(image):
        return 0
    e = pos
    while e < len(image) and image[e] not in (0x0A, 0x0D):
        if image[e] not in ASCII:
            return 0
        e += 1
    if e == len(image):
        return 0
    nl = 2 if image[e] == 0x0D and image[e + 1:e + 2] == b"\n" else 1
    body = image[pos:e]
    rest = image[e + nl:]
    if k == 6:
        if not body or body[0] not in UUCHAR:
            return 0
        l = uudec(body[0])
        if l > 45 or l > len(body) - 1:
            return 0
        if any(c not in UUCHAR for c in body[1:1 + l]):
            return 0
        # the reference counts l CHARACTERS off, skips one checksum or padding character if exactly one is left, steps
        # over the line end and looks at what stands there: inside this line still, when more characters were left
        rem = len(body) - 1 - l
        skip = 1 if rem == 1 and (body[1 + l] in UUCHAR or 0x61 <= body[1 + l] <= 0x7A) else 0
        if rest and image[pos + 1 + l + skip + nl] in UUCHAR:
            return firstline + 30
        return 0
    if any(c not in BASE64 for c in body):
        return 0
    if rest[:5] == b"====\n" or rest[:6] == b"====\r\n":
        return firstline + 40
    if rest and rest[0] in BASE64:
        return firstline + 30
    return 0


def reference_read(image):
    """(bytes, rc, message, name, mode) of the filter over the whole stream"""
    w = walk(image)
    if w.status in (ST_OK, ST_IGNORED):
        return w.out, 0, "", w.name, w.mode
    return w.out, ARCHIVE_FATAL, MESSAGE[w.status], w.name, w.mode


def reference_cat(image, read_size=None):
    """(bytes, rc, message) of bsdcat over the image: a stream the bidder declines comes out as it is (the raw format)"""
    image = bytes(image)
    if read_size is not None:
        first = lines_of(image)[:1]
        assert len(image) < BID_MAX_READ or (first and header_kind(image[:first[0][1] - first[0][2]])), "the bid depends on the blocks"
    if bid(image) == 0:
        return image, 0, ""
    return reference_read(image)[:3]


# ---- builders ----

def randbytes(seed, n):
    return random.Random(seed).randbytes(n)


def text(seed, n):
    r = random.Random(seed)
    words = [b"archive", b"filter", b"stream", b"header", b"window", b"device", b"line", b"state", b"0123456789", b"uu", b"\n"]
    out = bytearray()
    while len(out) < n:
        out += r.choice(words) + b" "
    return bytes(out[:n])


def uu_char(v):
    """the character of a 6-bit value; 0 is '`' as modern encoders write it"""
    return 0x60 if v == 0 else 0x20 + v


def uu_body(data, zero=0x60):
    """the characters of `data` (at most 63 bytes), without the length character"""
    out = bytearray()
    for i in range(0, len(data), 3):
        g = data[i:i + 3] + bytes(3 - len(data[i:i + 3]))
        n = g[0] << 16 | g[1] << 8 | g[2]
        out += bytes((uu_char((n >> s) & 63) if (n >> s) & 63 else zero) for s in (18, 12, 6, 0))
    return bytes(out)


def uu_line(data, length_char=None, nl=b"\n", tail=b"", zero=0x60):
    """one uuencode line: the length character (chosen, or the one of len(data)), the groups, `tail`, the line end"""
    lc = length_char if length_char is not None else (zero if len(data) == 0 else 0x20 + len(data))
    return bytes([lc]) + uu_body(data, zero) + tail + nl


def uu_section(data, name=b"file.bin", mode=0o644, nl=b"\n", per_line=45, zero_line=b"`", end=b"end", zero=0x60):
    out = bytearray(b"begin %03o " % mode + name + nl)
    for i in range(0, len(data), per_line):
        out += uu_line(data[i:i + per_line], nl=nl, zero=zero)
    if zero_line is not None:
        out += zero_line + nl
        if end is not None:
            out += end + nl
    return bytes(out)


def b64_section(data, name=b"file.bin", mode=0o644, nl=b"\n", per_line=57, end=b"===="):
    out = bytearray(b"begin-base64 %03o " % mode + name + nl)
    for i in range(0, len(data), per_line):
        out += base64.b64encode(data[i:i + per_line]) + nl
    if end is not None:
        out += end + nl
    return bytes(out)


def residue_stream(style, seed):
    """base64 lines whose lengths (line end included) cycle through 1 .. 62: more than three tiles, more than three
    groups of lines; a body of 4k + 1 characters ends in '='"""
    r = random.Random(seed)
    out = bytearray()
    alphabet = B64_ALPHABET
    for i in range(1000):
        nl = style if style != b"mixed" else r.choice([b"\n", b"\r\n", b"\r"])
        length = 1 + i % 62
        n = max(length - len(nl), 0)
        body = bytes(r.choice(alphabet) for _ in range(n))
        if n % 4 == 1:
            body = body[:-1] + b"="
        out += body + nl
    return bytes(out)


def junk(seed, n_lines, nl=b"\n", width=72):
    """mail-style lines of printable characters; none of them is a header line"""
    r = random.Random(seed)
    out = bytearray()
    for i in range(n_lines):
        k = r.randrange(0, width)
        ln = bytes(r.randrange(0x20, 0x7F) for _ in range(k))
        if ln.startswith(b"begin"):
            ln = b"B" + ln[1:]
        out += ln + nl
    return bytes(out)


def preamble(n_bytes):
    """exactly n_bytes of mail-style lines (the last one padded)"""
    if n_bytes == 0:
        return b""
    out = bytearray()
    i = 0
    while len(out) < n_bytes:
        out += b"X-Header-%d: some words that a mail program wrote in front of the body\n" % i
        i += 1
    out = out[:n_bytes - 1]
    if out.endswith(b"\r"):
        out[-1] = 0x20
    return bytes(out) + b"\n"


def replace_line(image, index, new_line):
    ls = lines_of(image)
    s, n, _ = ls[index]
    return image[:s] + new_line + image[s + n:]


_SHAPES = None


def filter_shapes():
    """name -> image.  The first section of every image is taken by the bidder unless the name says `declined`."""
    global _SHAPES
    if _SHAPES is not None:
        return _SHAPES
    d45, d100, d7 = randbytes(1, 45 * 40), randbytes(2, 100), randbytes(3, 7)
    big = randbytes(4, 70000)
    uu = uu_section(d45)
    b64 = b64_section(d45)
    empty_uu = uu_section(b"")
    sh = {
        "uu": uu,
        "uu_crlf": uu_section(d45, nl=b"\r\n"),
        "uu_cr": uu_section(d45, nl=b"\r"),
        "uu_short_last_line": uu_section(d100),
        "uu_space_for_zero": uu_section(d100 + bytes(50), zero_line=b" ", zero=0x20),
        "uu_70000_bytes": uu_section(big),
        "declined_uu_lines_of_60": uu_section(d45, per_line=60),
        "uu_lines_of_60_behind_one_of_45": b"begin 644 x\n" + uu_line(d45[:45]) + uu_section(d45[45:], per_line=60)[19:],
        "uu_checksum_characters": b"begin 644 c\n" + b"".join(uu_line(d45[i:i + 45], tail=b"K") for i in range(0, 450, 45)) + b"`\nend\n",
        "uu_padding_ignored": b"begin 644 c\n" + uu_line(d7, tail=b"zz{|}~ padding of any printable kind") + uu_line(d7) + b"`\nend\n",
        "uu_no_end_line": uu_section(d100, end=None),
        "uu_no_zero_line": uu_section(d100, zero_line=None),
        "uu_end_without_line_end": uu[:-1],
        "uu_cut_inside_a_data_line": uu[:200],
        "uu_cut_inside_end": uu[:-3],
        "uu_cut_behind_a_cr": uu_section(d45, nl=b"\r\n")[:uu_section(d45, nl=b"\r\n").index(b"\r\n", 200) + 1],
        "uu_wrong_end": uu[:-4] + b"enx\n",
        "uu_end_with_a_blank": uu[:-1] + b" \n",
        "uu_length_character_above_the_body": replace_line(uu, 3, b"M" + uu_body(d45[:30]) + b"\n"),
        "uu_invalid_character": replace_line(uu, 5, uu_line(d45[:45])[:20] + b"a" + uu_line(d45[:45])[21:]),
        "uu_empty_line_in_data": replace_line(uu, 4, b"\n"),
        "uu_length_character_not_uuchar": replace_line(uu, 2, b"a" + uu_body(d45[:45]) + b"\n"),
        "uu_bad_byte_in_data": replace_line(uu, 7, uu_line(d45[:45])[:10] + b"\x01" + uu_line(d45[:45])[11:]),
        "uu_high_byte_in_end": uu[:-4] + b"en\xe4\n",
        "uu_tab_in_data": replace_line(uu, 9, b"\t" + uu_line(d45[:45])),
        "b64": b64,
        "b64_crlf": b64_section(d45, nl=b"\r\n"),
        "b64_cr": b64_section(d45, nl=b"\r"),
        "b64_padding_1": b64_section(d100),
        "b64_padding_2": b64_section(d100 + b"x"),
        "b64_no_terminator": b64_section(d100, end=None),
        "b64_three_equals": b64_section(d100, end=b"==="),
        "b64_lines_of_19_groups_and_two_characters": b64_section(d45[:57], end=None) + b64_section(d45[57:], per_line=58)[26:],
        "b64_empty_lines": replace_line(b64, 3, b"\n\n" + base64.b64encode(d45[:57]) + b"\n"),
        "b64_lone_character": replace_line(b64, 4, b"Q\n"),
        "b64_invalid_character": replace_line(b64, 4, base64.b64encode(d45[:57])[:30] + b"*" + base64.b64encode(d45[:57])[31:] + b"\n"),
        "b64_equals_inside": replace_line(b64, 4, base64.b64encode(d45[:57])[:32] + b"=" + base64.b64encode(d45[:57])[33:] + b"\n"),
        "b64_two_equals_line": replace_line(b64, 4, b"==\n"),
        "b64_cut_inside_a_line": b64[:300],
        "b64_bad_byte": replace_line(b64, 6, b"\x7f" + base64.b64encode(d45[:57]) + b"\n"),
        "b64_70000_bytes": b64_section(big),
        "two_sections": uu_section(d100, name=b"first") + b64_section(d7 * 30, name=b"second"),
        "three_sections_with_junk": uu + junk(5, 20) + b64 + junk(6, 3, nl=b"\r\n") + uu_section(d100, nl=b"\r\n"),
        "preamble_of_40_lines": junk(7, 40) + uu,
        "preamble_crlf": junk(8, 12, nl=b"\r\n") + b64,
        "declined_header_in_line_with_bad_mode": b"begin 6a4 x\n" + uu[12:],
        "declined_bad_byte_in_preamble": b"caf\xe9\n" + uu,
        "declined_first_data_line_too_long": b"begin 644 x\n" + b"N" + uu_body(bytes(46)) + b"\n`\nend\n",
        "name_of_one_character": uu_section(d100, name=b"x"),
        "binary_junk_behind_end": uu + randbytes(9, 3000),
        "binary_junk_behind_base64": b64 + b"\x00\x01\x02" + randbytes(10, 500),
        "declined_empty_uu_section": empty_uu + b"\xff\n",
        "declined_empty_base64_section": b64_section(b"") + junk(11, 3) + b"\x00",
        "bad_byte_behind_an_empty_base64_section": b"begin-base64 644 nothing\n\n====\n" + junk(11, 3) + b"\x00",
        "text_behind_end_without_line_end": uu + b"trailing words",
        "head_line_of_131071_bytes": uu + b"j" * 131070 + b"\n" + b64,
        "head_line_of_131072_bytes": uu + b"j" * 131071 + b"\n" + b64,
        "head_line_of_200000_bytes_with_a_bad_byte": uu + b"j" * 150000 + b"\x80" + b"j" * 50000 + b"\n" + b64,
        "uu_line_of_32768_bytes": b"begin 644 x\n" + b"M" + uu_body(d45[:45]) + b" " * (32768 - 62) + b"\n" + b"`\nend\n",
        "uu_line_of_32769_bytes": b"begin 644 x\n" + uu_line(d45[:45]) + b"M" + uu_body(d45[:45]) + b" " * (32769 - 62) + b"\n" + b"`\nend\n",
        "b64_line_of_32768_bytes": b"begin-base64 644 x\n" + base64.b64encode(d45[:57]) + b"\n" + base64.b64encode(randbytes(12, 24573)) + b"AAA\n====\n",
        "b64_line_of_32769_bytes": b"begin-base64 644 x\n" + base64.b64encode(d45[:57]) + b"\n" + base64.b64encode(randbytes(12, 24576)) + b"\n====\n",
        "end_line_of_40000_bytes": uu_section(d100, end=b"e" * 40000),
    }
    _SHAPES = sh
    return sh


def fixtures():
    """[(manifest entry, image)] of tests/golden/ref_fixtures/uu"""
    with open(os.path.join(FIXTURE_DIR, "manifest.json")) as f:
        man = json.load(f)
    out = []
    for m in man["files"]:
        with open(os.path.join(FIXTURE_DIR, m["file"]), "rb") as f:
            img = f.read()
        assert hashlib.sha256(img).hexdigest() == m["sha256"], m["file"]
        out.append((m, img))
    return out


def b2a_uu_section(data, backtick=True, nl=b"\n", name=b"py"):
    """a section written by Python's binascii (lines of 45 bytes)"""
    out = bytearray(b"begin 644 " + name + nl)
    for i in range(0, len(data), 45):
        out += binascii.b2a_uu(data[i:i + 45], backtick=backtick)[:-1] + nl
    out += (b"`" if backtick else b" ") + nl + b"end" + nl
    return bytes(out)
