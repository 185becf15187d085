"""A bzip2 stream WRITER in plain Python, from the format (no libbz2, no bz2 module): streams that no compressor emits,
for the device decoder (la_bzip2.hip) and the host filter.  A stream is a list of Blocks.  A Block is described either by
its post-RLE1 bytes `r` (the test chooses the count bytes itself; the rotations are sorted here, then MTF and RUNA/RUNB)
or by raw fields (used bytes, orig_ptr, symbol list), and every field of the block can be scripted: the stored CRC,
orig_ptr, the 16 + 16 x 16 map words, the table count, the declared selector count, the selectors and surplus selector
codes, the code lengths per table with the delta walk taken, and the image can stop at any bit.  The symbols' codes
are the canonical assignment over the lengths (codes ascending by length, then by symbol), which is what libbz2's
limit / base / perm tables decode, complete or not.

While it writes, a small model keeps the plain bytes: the inverse BWT as the format defines it (the vector chased from
orig_ptr), then the run-length expansion, with the run libbz2 makes up behind four equal bytes at a block's end.  The
model is never its own judge: tests/test_bzip2_handbuilt.py holds every case to libbz2 itself.

handbuilt_cases(census) returns the catalogue as Case(name, image, plain, valid, cls, ...): plain is the whole plain for
a valid case and the bytes in front of the error for a refused one, cls is ok / data / truncated / crc."""
import random
from collections import namedtuple

BLOCK_MAGIC, END_MAGIC = 0x314159265359, 0x177245385090
MAX_SEL = 18002
RUNA, RUNB = 0, 1

# level: the stream's; marks: [(bit, kind)] of the REAL block (0) and end-of-stream (1) magics; bad: index into marks of
# the unit that fails (None: none); end_run: the failure is the missing count behind four equal bytes
Case = namedtuple("Case", "name image plain valid cls level marks bad end_run")
Built = namedtuple("Built", "image plains marks blocks features")

CENSUS_KEYS = [
    "count_252_255", "count_at_thread_range_edge", "vector_of_many_cycles", "count_at_chunk_first", "count_at_chunk_last", "count_at_block_last", "count_run_straddles_chunk",
    "len_18", "len_19", "len_20", "minlen_1", "minlen_20", "walk_up_and_down", "walk_out_of_range",
    "tables_3_tiny", "tables_4_tiny", "tables_5_tiny", "tables_6_tiny", "table_unnamed", "selectors_surplus",
    "selectors_over_18002", "selectors_too_few", "selector_equals_table_count",
    "false_block_magic", "false_end_magic", "false_end_magic_with_crc",
    "nblock_at_level_bound", "nblock_over_level_bound", "orig_ptr_last", "orig_ptr_at_nblock", "orig_ptr_over_level_bound",
    "level_1_in_level_9_slot_second_look",
    "run_fills_slot", "run_overflows_slot", "run_22_symbols", "missing_count",
    "map_empty_word", "map_all_empty", "map_16_ranges_one_byte", "incomplete_code_pattern", "oversubscribed_lengths",
]


# ---------------------------------------------------------------- bits and CRC

class _Bits:
    """MSB-first bit writer"""
    def __init__(self):
        self.acc, self.k, self.out = 0, 0, bytearray()

    def put(self, v, nbits):
        self.acc = (self.acc << nbits) | (v & ((1 << nbits) - 1))
        self.k += nbits
        while self.k >= 8:
            self.k -= 8
            self.out.append((self.acc >> self.k) & 255)
        self.acc &= (1 << self.k) - 1

    def bits(self, s):
        for ch in s:
            self.put(1 if ch == "1" else 0, 1)

    def pos(self):
        return len(self.out) * 8 + self.k

    def done(self, cut_bit=None):
        out = bytearray(self.out)
        if self.k:
            out.append((self.acc << (8 - self.k)) & 255)
        if cut_bit is not None:
            out = out[:(cut_bit + 7) // 8]
            if cut_bit & 7:
                out[-1] &= (0xFF00 >> (cut_bit & 7)) & 0xFF
        return bytes(out)


def _crc_table():
    tab = []
    for i in range(256):
        c = i << 24
        for _ in range(8):
            c = ((c << 1) ^ 0x04C11DB7 if c & 0x80000000 else c << 1) & 0xFFFFFFFF
        tab.append(c)
    return tab


_TAB = _crc_table()


def crc(data):
    """the block CRC: polynomial 0x04C11DB7, MSB first, initial and final complement"""
    c = 0xFFFFFFFF
    for b in data:
        c = ((c << 8) & 0xFFFFFFFF) ^ _TAB[(c >> 24) ^ b]
    return c ^ 0xFFFFFFFF


def combine(comb, block_crc):
    """the stream's combined CRC behind one more block"""
    return (((comb << 1) | (comb >> 31)) & 0xFFFFFFFF) ^ block_crc


# ---------------------------------------------------------------- the transforms and their model

def bwt(r, window=None):
    """(last column, orig_ptr) of the sorted rotations of r.  window: compare that many bytes of each rotation only, for a
    long r whose windows of that size are all different (checked)"""
    n = len(r)
    rr = bytes(r) + bytes(r)
    w = window or n
    idx = sorted(range(n), key=lambda i: rr[i:i + w])
    assert w == n or len({rr[i:i + w] for i in range(n)}) == n
    return bytes(rr[i + n - 1] for i in idx), idx.index(0)


def unbwt(col, orig_ptr):
    """The block as the format's decoder reads it: the vector tt[cftab[col[i]]++] = i chased from tt[orig_ptr].  Returns
    (bytes, the byte the chain gives behind the block's last)."""
    n = len(col)
    if col.count(col[:1]) == n:     # one value: the vector is the identity
        return bytes(col), col[0]
    start, tot = [0] * 256, 0
    cnt = [0] * 256
    for b in col:
        cnt[b] += 1
    for v in range(256):
        start[v], tot = tot, tot + cnt[v]
    tt = [0] * n
    for i, b in enumerate(col):
        tt[start[b]] = i
        start[b] += 1
    out = bytearray(n)
    p = tt[orig_ptr]
    for k in range(n):
        out[k] = col[p]
        p = tt[p]
    return bytes(out), col[p]


def count_bytes(pre):
    """[(index, value)] of the count bytes of a pre-RLE block, and whether it ends on four equal bytes with none"""
    out, run, prev = [], 0, -1
    for i, b in enumerate(pre):
        if run == 4:
            out.append((i, b))
            run, prev = 0, -1
            continue
        run = run + 1 if b == prev else 1
        prev = b
    return out, run == 4


def unrle1(pre):
    """(plain bytes, True if the block ends on four equal bytes with no count behind them)"""
    out, run, prev = bytearray(), 0, -1
    for b in pre:
        if run == 4:
            out += bytes([prev]) * b
            run, prev = 0, -1
            continue
        out.append(b)
        run = run + 1 if b == prev else 1
        prev = b
    return bytes(out), run == 4


def run_symbols(n):
    """n >= 1 in RUNA / RUNB digits (bijective base 2, least significant first)"""
    out = []
    while n > 0:
        if n & 1:
            out.append(RUNA)
            n = (n - 1) >> 1
        else:
            out.append(RUNB)
            n = (n - 2) >> 1
    return out


def mtf_symbols(col, used):
    """the symbol list of a column over the sorted used bytes, end-of-block included"""
    yy = list(used)
    syms, run = [], 0
    for b in col:
        j = yy.index(b)
        if j == 0:
            run += 1
            continue
        syms += run_symbols(run)
        run = 0
        syms.append(j + 1)
        yy.insert(0, yy.pop(j))
    syms += run_symbols(run)
    syms.append(len(used) + 1)
    return syms


def symbols_to_column(used, syms):
    """the column a symbol list decodes to (up to the end-of-block symbol), None if an entry is no symbol"""
    yy = list(used)
    eob = len(used) + 1
    parts, es, n = [], 0, 1
    for s in syms:
        if not isinstance(s, int) or s < 0 or s > eob:
            return None
        if s <= RUNB:
            es += n if s == RUNA else 2 * n
            n *= 2
            continue
        if es:
            parts.append(bytes([yy[0]]) * es)
            es, n = 0, 1
        if s == eob:
            break
        yy.insert(0, yy.pop(s - 1))
        parts.append(bytes([yy[0]]))
    if es:
        parts.append(bytes([yy[0]]) * es)
    return b"".join(parts)


def flat_lengths(alpha):
    """a complete code over alpha >= 2 symbols with two neighbouring lengths"""
    k = alpha.bit_length() - 1
    longer = 2 * (alpha - (1 << k))
    return [k] * (alpha - longer) + [k + 1] * longer


def chain_lengths(maxlen):
    """the complete code 1, 2, ..., maxlen - 1, maxlen, maxlen over maxlen + 1 symbols"""
    return list(range(1, maxlen)) + [maxlen, maxlen]


def canon(lens):
    """symbol -> (code, length): codes ascending by (length, symbol); a symbol whose code does not fit its length (the
    lengths are over-subscribed) has none"""
    order = sorted(range(len(lens)), key=lambda i: (lens[i], i))
    out, code, prev = {}, 0, lens[order[0]]
    for i in order:
        code <<= lens[i] - prev
        prev = lens[i]
        if code < (1 << lens[i]):
            out[i] = (code, lens[i])
        code += 1
    return out


def bits_as_selectors(bitstring):
    """the selector codes (j ones and a zero each) whose unary coding spells bitstring; a zero is appended behind ones
    that end it"""
    codes, j = [], 0
    for ch in bitstring:
        if ch == "1":
            j += 1
        else:
            codes.append(j)
            j = 0
    if j:
        codes.append(j)
    return codes


def magic_bits(v, nbits=48):
    return format(v, "0%db" % nbits)


# ---------------------------------------------------------------- a block

class Block:
    """One block.  r: its post-RLE1 bytes (sorted here), or used / orig_ptr / syms given raw.  An entry of syms may be a
    string of '0' / '1': raw bits in a symbol's place.
    window: see bwt().  crc_xor: damage to the stored CRC.  map16 / map_words ({range: word}): the symbol map as written.  ntables: tables
    written; ntables_field: the 3-bit field if it is to differ.  selectors: table per group (default: table 0);
    sel_mtf: the selector codes as written, instead; surplus: more codes behind them; nsel_field: the declared count if
    it is to differ from the codes written.  lens: one list of lengths for all tables or one per table (an entry of
    0 or 21 ends the image's meaningful part there); start: {table: 5-bit start value}; via: {(table, symbol): [lengths
    the delta walk visits before it settles]}."""

    def __init__(self, r=None, *, window=None, used=None, orig_ptr=None, syms=None, crc_xor=0, map16=None, map_words=None, ntables=2,
                 ntables_field=None, nsel_field=None, selectors=None, sel_mtf=None, surplus=(), lens=None, start=None, via=None):
        if r is not None:
            col, op = bwt(r, window)
            self.used = sorted(set(r) | set(used or ()))
            self.syms = mtf_symbols(col, self.used)
            self.orig_ptr = op if orig_ptr is None else orig_ptr
            self.r, self.sorted_ptr = bytes(r), op
        else:
            self.used, self.syms, self.orig_ptr, self.r = sorted(used), list(syms), orig_ptr, None
        self.crc_xor, self.map16, self.map_words = crc_xor, map16, dict(map_words or {})
        self.ntables, self.ntables_field, self.nsel_field = ntables, ntables_field, nsel_field
        self.selectors, self.sel_mtf, self.surplus = selectors, sel_mtf, list(surplus)
        alpha = len(self.used) + 2
        if lens is None:
            lens = flat_lengths(alpha)
        self.lens = [list(lens)] * ntables if isinstance(lens[0], int) else [list(l) for l in lens]
        assert len(self.lens) == ntables and all(len(l) == alpha for l in self.lens)
        self.start, self.via = dict(start or {}), dict(via or {})
        self.pos = {}
        self.features = set()
        self.refused = False    # set for the block a decoder stops in: the model need not decode it

    def model(self):
        """(plain, missing count, pre-RLE bytes): what a decoder makes of the block if it takes it"""
        col = None if self.refused else symbols_to_column(self.used, self.syms)
        if not col or self.orig_ptr >= len(col):
            return b"", False, b""
        pre, beyond = unbwt(col, self.orig_ptr)
        if self.r is not None and self.orig_ptr == self.sorted_ptr:
            assert pre == self.r
        plain, missing = unrle1(pre)
        if missing:         # libbz2 reads a count all the same: the byte the chain gives there
            plain += pre[-1:] * beyond
        return plain, missing, pre

    def _codes(self):
        ngroups = (len(self.syms) + 49) // 50
        if self.sel_mtf is not None:
            codes = list(self.sel_mtf)
        else:
            tables = list(self.selectors) if self.selectors is not None else [0] * ngroups
            pos, codes = list(range(self.ntables)), []
            for t in tables:
                j = pos.index(t)
                codes.append(j)
                pos.insert(0, pos.pop(j))
        codes += self.surplus
        pos, tables = list(range(self.ntables)), []
        for j in codes[:MAX_SEL]:
            if j < self.ntables:
                pos.insert(0, pos.pop(j))
            tables.append(pos[0])
        return codes, tables, ngroups

    def write(self, w, stored_crc):
        """False if the block ends in a length out of range (nothing behind it can be read)"""
        f = self.features
        w.put(BLOCK_MAGIC, 48)
        w.put(stored_crc, 32)
        w.put(0, 1)
        w.put(self.orig_ptr, 24)
        words = [0] * 16
        for b in self.used:
            words[b >> 4] |= 0x8000 >> (b & 15)
        for i, v in self.map_words.items():
            words[i] = v
        m16 = self.map16 if self.map16 is not None else sum(0x8000 >> i for i in range(16) if words[i])
        w.put(m16, 16)
        for i in range(16):
            if m16 & (0x8000 >> i):
                w.put(words[i], 16)
                if words[i] == 0:
                    f.add("map_empty_word")
        w.put(self.ntables if self.ntables_field is None else self.ntables_field, 3)
        codes, tables, ngroups = self._codes()
        nsel = len(codes) if self.nsel_field is None else self.nsel_field
        w.put(nsel, 15)
        self.pos["selectors"] = w.pos()
        for j in codes:
            w.put(((1 << j) - 1) << 1, j + 1)
        if len(codes) > ngroups:
            f.add("selectors_surplus")
        if nsel > MAX_SEL:
            f.add("selectors_over_18002")
        named = set(tables[:ngroups])
        if len(named) < self.ntables:
            f.add("table_unnamed")
        if 3 <= self.ntables <= 6 and len(self.syms) < 50:
            f.add("tables_%d_tiny" % self.ntables)
        self.pos["tables"] = w.pos()
        for t in range(self.ntables):
            curr = self.start.get(t, self.lens[t][0])
            w.put(curr, 5)
            for i, target in enumerate(self.lens[t]):
                for wp in self.via.get((t, i), []) + [target]:
                    if self.via.get((t, i)):
                        f.add("walk_up_and_down")
                    while curr != wp and 1 <= curr <= 20:
                        w.put(2 if curr < wp else 3, 2)
                        curr += 1 if curr < wp else -1
                if not 1 <= curr <= 20:
                    return False
                w.put(0, 1)
        for t in named:
            if max(self.lens[t]) >= 18:
                f.add("len_%d" % max(self.lens[t]))
            if min(self.lens[t]) in (1, 20):
                f.add("minlen_%d" % min(self.lens[t]))
        self.pos["symbols"] = w.pos()
        table_codes = [canon(l) for l in self.lens]
        self.sym_pos = []
        for k, s in enumerate(self.syms):
            self.sym_pos.append(w.pos())
            if isinstance(s, str):
                w.bits(s)
                continue
            g = k // 50
            t = tables[g] if g < len(tables) else (tables[-1] if tables else 0)
            if s not in table_codes[t]:
                raise ValueError("symbol %d has no code in table %d" % (s, t))
            w.put(*table_codes[t][s])
        self.pos["end"] = w.pos()
        return True


def build(blocks, level=1, combined_xor=0, cut_bit=None, cut_byte=None):
    """The stream "BZh<level>" + blocks + end of stream.  cut_bit: the image stops at that bit (the last byte is filled
    with zeros); cut_byte: at that byte."""
    w = _Bits()
    for ch in b"BZh" + bytes([0x30 + level]):
        w.put(ch, 8)
    comb, marks, plains, feats, whole = 0, [], [], set(), True
    for b in blocks:
        plain, missing, pre = b.model()
        c = crc(plain)
        marks.append((w.pos(), 0))
        whole = b.write(w, c ^ b.crc_xor)
        plains.append(plain)
        comb = combine(comb, c)
        feats |= b.features
        counts, _ = count_bytes(pre)
        for i, v in counts:
            if v >= 252:
                feats.add("count_252_255")
            if i % 256 == 0:
                feats.add("count_at_chunk_first")
            if i % 256 == 255:
                feats.add("count_at_chunk_last")
            if i % 256 in (1, 2, 3) and i >= 256:
                feats.add("count_run_straddles_chunk")
            if i == len(pre) - 1:
                feats.add("count_at_block_last")
        if not whole:
            break
    if whole:
        marks.append((w.pos(), 1))
        w.put(END_MAGIC, 48)
        w.put(comb ^ combined_xor, 32)
    if cut_byte is not None:
        cut_bit = cut_byte * 8
    image = w.done(cut_bit)
    if cut_bit is not None:
        marks = [m for m in marks if m[0] + 48 <= len(image) * 8]
    return Built(image, plains, marks, blocks, feats)


# ---------------------------------------------------------------- the catalogue

def text(seed, n, k=12, base=97):
    """n bytes over k values, no two neighbours equal: no run the test did not write"""
    rnd, out = random.Random(seed), []
    while len(out) < n:
        b = base + rnd.randrange(k)
        if not out or out[-1] != b:
            out.append(b)
    return bytes(out)


def _two_values(seed, n):
    """n bytes over two values with no four equal in a row"""
    rnd, out = random.Random(seed), []
    while len(out) < n:
        b = 120 + rnd.randrange(2)
        if len(out) >= 3 and out[-1] == out[-2] == out[-3] == b:
            continue
        out.append(b)
    return bytes(out)


def _planted(lead, end_too=True, tail_bits=""):
    """surplus selector codes: `lead` one-bit selectors, then the block magic (and the end-of-stream magic and tail_bits)"""
    return [0] * lead + bits_as_selectors(magic_bits(BLOCK_MAGIC) + (magic_bits(END_MAGIC) + tail_bits if end_too else ""))


_CACHE = None


def _catalogue():
    out = []

    def add(name, blocks, cls="ok", bad=None, keys=(), end_run=False, level=1, **kw):
        out.append((name, blocks, cls, bad, tuple(keys), end_run, level, kw))

    q = b"Q" * 4
    # run counts behind four equal bytes
    for c in (0, 1, 251, 252, 254, 255):
        add("count-%d" % c, [Block(text(c, 40) + q + bytes([c]) + text(c + 1, 30))])
    # where the count byte lands among the chunks of 256 pre-RLE bytes
    for front in (251, 252, 253, 254, 255):
        add("count-byte-at-%d" % (front + 4), [Block(text(front, front) + q + b"\xff" + text(7, 20))])
    add("count-byte-at-the-block's-last-index", [Block(text(11, 100) + q + b"\xff")])
    add("count-byte-at-every-chunk's-last-index", [Block(b"".join(text(20 + i, 251) + q + b"\xfe" for i in range(5)) + text(9, 17))])
    add("count-byte-at-every-chunk's-first-index", [Block(text(5, 1) + b"".join(text(30 + i, 251) + q + b"\xfd" for i in range(5)) + text(8, 3))])
    add("bbbbaaaaa-with-count-255", [Block(b"XXXX" + b"\xff" * 6 + b"z")])
    # 70000 pre-RLE bytes are 274 chunks, two per thread of the measure kernel: counts at the last and first index of a
    # thread's range and around it, with every count value class
    big = bytearray(text(12, 70000))
    for k in range(1, 136):
        at = 512 * k + (-1, 0, 1, 2, 3, 255, 256)[k % 7]
        big[at - 4:at] = q
        big[at] = (0, 1, 4, 251, 252, 255, 97)[(k // 7) % 7]
    add("count-bytes-at-the-measure-threads'-range-edges", [Block(bytes(big), window=64)], keys=["count_at_thread_range_edge"])
    # a column that is no sorted text's: the vector has many cycles, the chase starts in the shortest and in the longest
    rnd = random.Random(13)
    col = bytes(rnd.choice(b"ABCDEFGH") for _ in range(3000))
    short, long_ = _cycle_starts(col)
    for what, at in (("shortest", short), ("longest", long_)):
        add("arbitrary-column-origin-in-its-%s-cycle" % what, [Block(used=sorted(set(col)), orig_ptr=at, syms=mtf_symbols(col, sorted(set(col))))],
            keys=["vector_of_many_cycles"])
    # code lengths
    flat = flat_lengths(14)
    r6 = text(14, 400)
    groups = (len(Block(r6).syms) + 49) // 50
    add("six-different-tables-all-named", [Block(r6, ntables=6, lens=[flat[3 * t:] + flat[:3 * t] for t in range(6)],
                                                 selectors=[(5 * g + g // 6) % 6 for g in range(groups)])])
    for m in (17, 18, 19, 20):
        r = bytes(random.Random(m).sample(list(range(65, 65 + m - 1)) * 4, 4 * (m - 1)))
        add("max-code-length-%d" % m, [Block(_no_runs(r), lens=chain_lengths(m))])
    add("minlen-1", [Block(text(41, 60, 3), lens=[1, 2, 3, 4, 4])])
    add("minlen-20-one-used-byte", [Block(b"AAA", lens=[20, 20, 20])])
    add("minlen-20-meets-pattern-1", [Block(used=[65], orig_ptr=0, syms=[RUNA, "1" * 24, 2], lens=[20, 20, 20])], "data", 0,
        ["incomplete_code_pattern"])
    add("incomplete-code-unused-pattern-met", [Block(used=[65], orig_ptr=0, syms=[RUNA, "1" * 24, 2], lens=[2, 2, 2])], "data", 0,
        ["incomplete_code_pattern"])
    r = text(42, 70)
    alpha = len(set(r)) + 2
    add("delta-walk-up-to-20-and-back", [Block(r, via={(0, 1): [20], (1, alpha - 1): [20]})])
    add("delta-walk-down-to-1-and-back", [Block(r, via={(0, 2): [1], (1, 0): [1, 20, 1]})])
    add("delta-walk-to-0", [Block(r, via={(1, 3): [0]})], "data", 0, ["walk_out_of_range"])
    add("delta-walk-to-21", [Block(r, via={(0, alpha - 1): [21]})], "data", 0, ["walk_out_of_range"])
    add("length-start-value-0", [Block(r, start={0: 0})], "data", 0, ["walk_out_of_range"])
    add("length-start-value-21", [Block(r, start={1: 21})], "data", 0, ["walk_out_of_range"])
    # table counts
    for n in (2, 3, 4, 5, 6):
        add("%d-tables-tiny-block" % n, [Block(text(50 + n, 30), ntables=n, selectors=[n - 1])])
    for n in (0, 1, 7):
        add("table-count-%d" % n, [Block(text(60, 30), ntables_field=n)], "data", 0)
    # selectors
    r120 = text(61, 120)
    add("selector-count-0", [Block(text(62, 30), sel_mtf=[], nsel_field=0)], "data", 0, ["selectors_too_few"])
    add("one-selector-fewer-than-groups", [Block(r120, selectors=[0] * ((len(Block(r120).syms) + 49) // 50 - 1))], "data", 0,
        ["selectors_too_few"])
    add("selectors-groups-plus-1", [Block(r120, ntables=3, selectors=[0, 1, 0][:(len(Block(r120).syms) + 49) // 50], surplus=[2])])
    for n in (18002, 18003, 32767):
        add("selectors-%d" % n, [Block(text(63, 30), ntables=3, surplus=[(i * 7 + i // 5) % 3 for i in range(n - 1)])])
    add("selector-code-equals-table-count", [Block(text(64, 30), ntables=3, sel_mtf=[3])], "data", 0, ["selector_equals_table_count"])
    # a real false magic: both magics spelt by surplus selectors of a valid block, at every bit phase
    for lead in range(8):
        add("false-magics-phase-%d-block-follows" % lead, [Block(text(70 + lead, 30), ntables=4, surplus=_planted(lead)), Block(text(90, 40))],
            keys=["false_block_magic", "false_end_magic"])
        add("false-magics-phase-%d-last-block" % lead, [Block(text(91, 40)), Block(text(70 + lead, 30), ntables=6, surplus=_planted(lead))],
            keys=["false_block_magic", "false_end_magic"])
    for k in range(64):     # a first block whose CRC the unary coding of 6 tables can spell
        first = Block(text(100 + k, 40))
        c0 = format(crc(first.model()[0]), "032b")
        if "111111" not in "0" + c0 + "0":
            break
    add("false-end-magic-followed-by-the-combined-crc", [first, Block(text(99, 30), ntables=6, surplus=[0, 0, 0] + bits_as_selectors(magic_bits(END_MAGIC) + c0))],
        keys=["false_end_magic_with_crc"])
    # the level's bounds
    one = lambda n: run_symbols(n) + [2]
    add("level-1-run-of-100000", [Block(used=[1], orig_ptr=0, syms=one(100000))], keys=["nblock_at_level_bound", "run_fills_slot"])
    add("level-1-run-of-100001", [Block(used=[1], orig_ptr=0, syms=one(100001))], "data", 0,
        ["nblock_over_level_bound", "run_overflows_slot", "level_1_in_level_9_slot_second_look"])
    add("level-1-nblock-100001-cut-before-end-of-block", [Block(used=[1, 2], orig_ptr=0, syms=run_symbols(100000) + [2, 3])], "data", 0,
        ["level_1_in_level_9_slot_second_look"], cut_at_symbol=-1)
    add("level-9-run-of-900000", [Block(used=[1], orig_ptr=0, syms=one(900000))], keys=["nblock_at_level_bound", "run_fills_slot"], level=9)
    add("level-9-run-of-900001", [Block(used=[1], orig_ptr=0, syms=one(900001))], "data", 0, ["nblock_over_level_bound", "run_overflows_slot"], level=9)
    add("22-runa-in-a-row", [Block(used=[1], orig_ptr=0, syms=[RUNA] * 22 + [2])], "data", 0, ["run_22_symbols"])
    add("21-runb-in-a-row", [Block(used=[1], orig_ptr=0, syms=[RUNB] * 21 + [2])], "data", 0, ["run_overflows_slot"], level=9)
    add("end-of-block-first", [Block(used=[65], orig_ptr=0, syms=[2])], "data", 0, ["orig_ptr_at_nblock"])
    r60 = text(65, 60)
    add("orig-ptr-nblock-minus-1", [Block(r60, orig_ptr=59)], keys=["orig_ptr_last"])
    add("orig-ptr-nblock", [Block(r60, orig_ptr=60)], "data", 0, ["orig_ptr_at_nblock"])
    add("orig-ptr-100010-level-1", [Block(r60, orig_ptr=100010)], "data", 0, ["orig_ptr_at_nblock"])
    add("orig-ptr-100011-level-1", [Block(r60, orig_ptr=100011)], "data", 0, ["orig_ptr_over_level_bound", "level_1_in_level_9_slot_second_look"])
    add("orig-ptr-100011-level-1-cut-behind-it", [Block(r60, orig_ptr=100011)], "data", 0,
        ["orig_ptr_over_level_bound", "level_1_in_level_9_slot_second_look"], cut_byte=4 + 14)
    add("orig-ptr-900011-level-9", [Block(r60, orig_ptr=900011)], "data", 0, ["orig_ptr_over_level_bound"], level=9)
    # four equal bytes at the block's end and no count
    add("missing-count-one-block", [Block(text(66, 30) + q)], "data", 0, ["missing_count"], end_run=True)
    add("missing-count-made-up-run-crosses-64k", [Block(used=[1], orig_ptr=0, syms=one(65520)), Block(b"abc" + b"XXXX")], "data", 1,
        ["missing_count"], end_run=True)
    add("missing-count-periodic-block", [Block(b"aaaa")], "data", 0, ["missing_count"], end_run=True)
    # the symbol map
    add("map-all-empty", [Block(text(67, 30), map16=0)], "data", 0, ["map_all_empty"])
    add("map-flagged-range-with-an-empty-word", [Block(text(68, 30), map16=0x0600 | 0x0002)])
    r16 = bytes(16 * i + (i * 5 + 3) % 16 for i in range(16))
    add("map-16-ranges-one-byte-each", [Block(_no_runs(r16 + r16[::-1] + r16[3:11]))], keys=["map_16_ranges_one_byte"])
    add("map-all-256-used", [Block(bytes(random.Random(69).sample(range(256), 256)) + bytes(range(255, -1, -3)))])
    # CRCs
    two = lambda: [Block(text(71, 50)), Block(text(72, 50))]
    b2 = two(); b2[0].crc_xor = 1
    add("wrong-block-crc-in-block-0-of-2", b2, "crc", 0)
    b2 = two(); b2[1].crc_xor = 0x80000000
    add("wrong-block-crc-in-block-1-of-2", b2, "crc", 1)
    add("wrong-combined-crc", two(), "crc", 2, combined_xor=0x00010000)
    # over-subscribed lengths: libbz2 builds its tables without a Kraft check; the codes that fit decode
    rx = _two_values(73, 150)
    groups = (len(Block(rx).syms) + 49) // 50
    assert groups >= 2
    add("oversubscribed-lengths-1-2-2-2", [Block(rx, lens=[[1, 2, 2, 2], [2, 2, 2, 2]], selectors=[0] * (groups - 1) + [1])],
        keys=["oversubscribed_lengths"])
    ry = _two_values(74, 150) + b"z"
    groups = (len(Block(ry).syms) + 49) // 50
    add("oversubscribed-lengths-five-of-2-bits", [Block(ry, lens=[[2, 2, 2, 2, 2], [2, 2, 2, 3, 3]], selectors=[0] * (groups - 1) + [1])],
        keys=["oversubscribed_lengths"])
    # cut streams
    rt = text(75, 120)
    for where, extra in (("selectors", 0), ("tables", 3), ("symbols", 9)):
        add("cut-inside-the-%s" % where, [Block(rt, ntables=3, surplus=[1, 2, 0, 1])], "truncated", 0, cut_in=(0, where, extra))
    add("cut-inside-the-stream-crc", [Block(rt)], "truncated", 1, cut_from_end=2)
    add("cut-behind-the-block-magic", [Block(rt)], "truncated", 0, cut_in=(0, "magic", 7))
    return out


def _cycle_starts(col):
    """orig_ptr values whose chase runs in the shortest and in the longest cycle of the column's vector"""
    n = len(col)
    order = sorted(range(n), key=lambda i: (col[i], i))      # tt
    seen, best = [False] * n, {}
    for s0 in range(n):
        if seen[s0]:
            continue
        p, length = s0, 0
        while not seen[p]:
            seen[p] = True
            p = order[p]
            length += 1
        best.setdefault(length, s0)
    return best[min(best)], best[max(best)]


def _no_runs(r):
    """r with no four equal bytes in a row (a sample may hold some)"""
    out = bytearray()
    for b in r:
        if len(out) >= 3 and out[-1] == out[-2] == out[-3] == b:
            continue
        out.append(b)
    return bytes(out)


def _make(entry):
    name, blocks, cls, bad, keys, end_run, level, kw = entry
    kw = dict(kw)
    cut_sym, cut_in, cut_end = kw.pop("cut_at_symbol", None), kw.pop("cut_in", None), kw.pop("cut_from_end", None)
    if cls in ("data", "truncated") and not end_run and bad < len(blocks):
        blocks[bad].refused = True
    s = build(blocks, level, **kw)
    if cut_sym is not None:
        s = build(blocks, level, cut_bit=blocks[bad].sym_pos[cut_sym], **kw)
    if cut_in is not None:
        k, where, extra = cut_in
        at = s.marks[k][0] + 48 if where == "magic" else blocks[k].pos[where]
        s = build(blocks, level, cut_byte=at // 8 + extra, **kw)
    if cut_end is not None:
        s = build(blocks, level, cut_byte=len(s.image) - cut_end, **kw)
    if cls == "ok":
        plain = b"".join(s.plains)
    else:
        plain = b"".join(s.plains[:bad]) + (s.plains[bad] if (cls == "crc" or end_run) and bad < len(s.plains) else b"")
    feats = set(keys) | (s.features if cls == "ok" else set())
    return Case(name, s.image, plain, cls == "ok", cls, level, s.marks, bad, end_run), feats


def handbuilt_cases(census=None):
    """The catalogue.  census (a dict) gets, per feature, how many cases took it: what the writer saw itself write in a
    VALID stream, and what a case states for itself."""
    global _CACHE
    if _CACHE is None:
        made = [_make(e) for e in _catalogue()]
        assert len({c.name for c, _ in made}) == len(made)
        _CACHE = made
    if census is not None:
        for _, feats in _CACHE:
            for k in feats:
                census[k] = census.get(k, 0) + 1
    return [c for c, _ in _CACHE]


def prefix_stream():
    """(image, the two blocks' plain bytes, marks) of one valid two-block stream of 250 .. 500 bytes for the cut-at-every-byte tests: 4 and 3
    tables, surplus selectors that spell the block magic, a count byte of 255"""
    a = Block(text(200, 120) + b"Q" * 4 + b"\xff" + text(201, 60), ntables=4, surplus=_planted(3, end_too=False))
    a.selectors = [0, 3, 1, 2, 0, 3][:(len(a.syms) + 49) // 50]
    b = Block(text(202, 150, 20), ntables=3)
    b.selectors = [2, 0, 1, 2, 0, 1][:(len(b.syms) + 49) // 50]
    s = build([a, b])
    assert 250 <= len(s.image) <= 500, len(s.image)
    return s.image, s.plains, s.marks
