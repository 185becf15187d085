"""A Zstandard frame WRITER in plain Python, from RFC 8878 (test infrastructure).

Not a compressor: it serialises an explicit script -- frame-header fields, then per block raw bytes, an RLE byte and
count, or a compressed block given as literal bytes plus (literal_length, match_length, offset_value) entries
(offset_value is the coded value: 1..3 are the repeat codes) with every header choice spelled out: literals type, size
format, stream count, Huffman weights and how they are sent, the mode / normalised counts / accuracy log of each of
the three sequence tables, the byte form of the sequence count.  It also EXECUTES the script with a minimal model and
returns the plain bytes; the tests never let that model judge itself (libzstd must return the same bytes).  Fields can
be forced to invalid values for the refusal cases.  No libzstd, nothing from any decoder in this repository.

Bit order (RFC 8878 4.1 / 4.2.2): a "backward" stream is written forward, least significant bit first, closed with a
single 1 bit; the decoder starts below that bit and reads downwards.  The writer therefore lists the decoder's reads
in DECODING order as (value, nbits) and packs the list reversed.
"""
import heapq
import sys

MAGIC = 0xFD2FB528
BLOCK_MAX = 128 * 1024

# RFC 8878 3.1.1.3.2.1.1: literal-length / match-length codes
LL_BASE = list(range(16)) + [16, 18, 20, 22, 24, 28, 32, 40, 48, 64, 128, 256, 512, 1024, 2048, 4096, 8192, 16384, 32768, 65536]
LL_BITS = [0] * 16 + [1, 1, 1, 1, 2, 2, 3, 3, 4, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16]
ML_BASE = list(range(3, 35)) + [35, 37, 39, 41, 43, 47, 51, 59, 67, 83, 99, 131, 259, 515, 1027, 2051, 4099, 8195, 16387, 32771, 65539]
ML_BITS = [0] * 32 + [1, 1, 1, 1, 2, 2, 3, 3, 4, 4, 5, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16]
# RFC 8878 3.1.1.3.2.2: default distributions
LL_DEF = [4, 3, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 1, 1, 1, 2, 2, 2, 2, 2, 2, 2, 2, 2, 3, 2, 1, 1, 1, 1, 1, -1, -1, -1, -1]
ML_DEF = [1, 4, 3, 2, 2, 2, 2, 2, 2] + [1] * 37 + [-1] * 7
OF_DEF = [1, 1, 1, 1, 1, 1, 2, 2, 2] + [1] * 15 + [-1] * 5
DEFAULTS = {"ll": (LL_DEF, 6), "of": (OF_DEF, 5), "ml": (ML_DEF, 6)}
MAX_AL = {"ll": 9, "of": 8, "ml": 9}
MAX_SYM = {"ll": 35, "of": 31, "ml": 52}
assert len(LL_DEF) == 36 and len(ML_DEF) == 53 and len(OF_DEF) == 29
assert all(sum(abs(c) for c in d) == 1 << al for d, al in DEFAULTS.values())


# ---------------------------------------------------------------- XXH64 (xxHash specification)
_P1, _P2, _P3, _P4, _P5 = 11400714785074694791, 14029467366897019727, 1609587929392839161, 9650029242287828579, 2870177450012600261
_M = (1 << 64) - 1


def _rotl(x, r):
    return ((x << r) | (x >> (64 - r))) & _M


def _round(acc, v):
    return (_rotl((acc + v * _P2) & _M, 31) * _P1) & _M


def _merge(h, v):
    return ((h ^ _round(0, v)) * _P1 + _P4) & _M


def xxh64(data, seed=0):
    data = bytes(data)
    n, p = len(data), 0
    if n >= 32:
        v = [(seed + _P1 + _P2) & _M, (seed + _P2) & _M, seed & _M, (seed - _P1) & _M]
        assert sys.byteorder == "little"
        words = memoryview(data)[:n - n % 32].cast("Q")
        for i in range(0, len(words), 4):
            v[0] = _round(v[0], words[i]); v[1] = _round(v[1], words[i + 1])
            v[2] = _round(v[2], words[i + 2]); v[3] = _round(v[3], words[i + 3])
        p = n - n % 32
        h = (_rotl(v[0], 1) + _rotl(v[1], 7) + _rotl(v[2], 12) + _rotl(v[3], 18)) & _M
        for x in v:
            h = _merge(h, x)
    else:
        h = (seed + _P5) & _M
    h = (h + n) & _M
    while p + 8 <= n:
        h = ((_rotl(h ^ _round(0, int.from_bytes(data[p:p + 8], "little")), 27)) * _P1 + _P4) & _M
        p += 8
    if p + 4 <= n:
        h = (_rotl(h ^ (int.from_bytes(data[p:p + 4], "little") * _P1) & _M, 23) * _P2 + _P3) & _M
        p += 4
    while p < n:
        h = (_rotl(h ^ (data[p] * _P5) & _M, 11) * _P1) & _M
        p += 1
    h ^= h >> 33; h = (h * _P2) & _M
    h ^= h >> 29; h = (h * _P3) & _M
    h ^= h >> 32
    return h


# ---------------------------------------------------------------- bit writers
class BitWriter:
    """forward writer, least significant bit first"""

    def __init__(self):
        self.out, self.acc, self.n = bytearray(), 0, 0

    def add(self, value, nbits):
        assert 0 <= value < (1 << nbits) or nbits == 0 and value == 0, (value, nbits)
        self.acc |= value << self.n
        self.n += nbits
        while self.n >= 8:
            self.out.append(self.acc & 0xFF)
            self.acc >>= 8
            self.n -= 8

    def finish(self):
        if self.n:
            self.out.append(self.acc & 0xFF)
            self.acc = self.n = 0
        return bytes(self.out)


def pack_backward(reads, marker=True):
    """reads = [(value, nbits)] in the order the decoder performs them"""
    w = BitWriter()
    for value, nbits in reversed(reads):
        w.add(value, nbits)
    if marker:
        w.add(1, 1)
    return w.finish()


# ---------------------------------------------------------------- FSE
def highbit(v):
    return v.bit_length() - 1


def write_ncount(norm, al, al_field=None):
    """RFC 8878 4.1.1: accuracy log, then the counts (value = count + 1; -1 is "less than 1"), a zero count followed
    by 2-bit repeat flags.  Symbols behind the one that completes the sum are not written."""
    w = BitWriter()
    w.add((al if al_field is None else al_field) - 5, 4)
    remaining, threshold, nbits = (1 << al) + 1, 1 << al, al + 1
    s = 0
    while remaining > 1 and s < len(norm):
        c = norm[s]
        mx = 2 * threshold - 1 - remaining
        v = c + 1
        if v < mx:
            w.add(v, nbits - 1)
        elif v < threshold:
            w.add(v, nbits)
        else:
            w.add(v + mx, nbits)
        remaining -= abs(c)
        s += 1
        if c == 0:
            z = 0
            while s + z < len(norm) and norm[s + z] == 0:
                z += 1
            s += z
            while z >= 3:
                w.add(3, 2)
                z -= 3
            w.add(z, 2)
        assert remaining >= 1, "counts exceed the table"
        while remaining < threshold:
            nbits -= 1
            threshold >>= 1
    return w.finish()


def fse_dtable(norm, al):
    """decoding table [(symbol, nbits, base)] (RFC 8878 4.1.1: spread with step size/2 + size/8 + 3, -1 symbols from
    the top)"""
    size = 1 << al
    sym = [None] * size
    high = size - 1
    nxt = {}
    for s, c in enumerate(norm):
        if c == -1:
            sym[high] = s
            high -= 1
            nxt[s] = 1
        else:
            nxt[s] = c
    step, mask, pos = (size >> 1) + (size >> 3) + 3, size - 1, 0
    for s, c in enumerate(norm):
        for _ in range(max(c, 0)):
            sym[pos] = s
            pos = (pos + step) & mask
            while pos > high:
                pos = (pos + step) & mask
    assert pos == 0 and None not in sym, "counts do not fill the table"
    tab = []
    for u in range(size):
        s = sym[u]
        nx = nxt[s]
        nxt[s] += 1
        nb = al - highbit(nx)
        tab.append((s, nb, (nx << nb) - size))
    return tab


def rle_dtable(symbol):
    return [(symbol, 0, 0)]


def fse_states(tab, symbols, last_pick=None):
    """the states a decoder walks through while it emits `symbols` from ONE state variable.  The last one is free
    (any state of that symbol: last_pick chooses, default the one with the most update bits)."""
    by_sym = {}
    for u, (s, nb, base) in enumerate(tab):
        by_sym.setdefault(s, []).append(u)
    n = len(symbols)
    states = [0] * n
    cands = by_sym[symbols[-1]]
    states[-1] = last_pick(cands) if last_pick else max(cands, key=lambda u: tab[u][1])
    for i in range(n - 2, -1, -1):
        target = states[i + 1]
        for u in by_sym[symbols[i]]:
            _, nb, base = tab[u]
            if base <= target < base + (1 << nb):
                states[i] = u
                break
        else:
            raise AssertionError("no state of symbol %d reaches %d" % (symbols[i], target))
    return states


def normalize(hist, al, minus_one=False):
    """counts summing to 1 << al for the symbols of hist (a list); rare symbols get 1, or -1 with minus_one"""
    size, total = 1 << al, sum(hist)
    norm = [0] * len(hist)
    for s, h in enumerate(hist):
        if h:
            norm[s] = max(1, h * size // total)
    big = max(range(len(hist)), key=lambda s: norm[s])
    norm[big] += size - sum(norm)
    assert norm[big] >= 1, "too many symbols for this accuracy log"
    if minus_one:
        norm = [-1 if c == 1 and s != big else c for s, c in enumerate(norm)]
    while norm and norm[-1] == 0:
        norm.pop()
    return norm


# ---------------------------------------------------------------- Huffman (RFC 8878 4.2)
def huf_weights_for(data, max_bits=11, extra_symbols=()):
    """complete prefix code for the bytes of data: weights[0..last symbol] (the last one is implied on the wire)"""
    hist = [0] * 256
    for b in data:
        hist[b] += 1
    for s in extra_symbols:
        hist[s] = max(hist[s], 1)
    if sum(1 for h in hist if h) < 2:
        hist[(max(range(256), key=lambda s: hist[s]) + 1) % 256] = 1
    floor = 0
    while True:
        heap = [(max(h, floor), s, (s,)) for s, h in enumerate(hist) if h]
        heapq.heapify(heap)
        length = [0] * 256
        while len(heap) > 1:
            a, b = heapq.heappop(heap), heapq.heappop(heap)
            for s in a[2] + b[2]:
                length[s] += 1
            heapq.heappush(heap, (a[0] + b[0], min(a[1], b[1]), a[2] + b[2]))
        mb = max(length)
        if mb <= max_bits:
            break
        floor = max(1, floor * 2, sum(hist) >> (max_bits + 2))
    last = max(s for s in range(256) if hist[s])
    return [mb + 1 - length[s] if length[s] else 0 for s in range(last + 1)]


def huf_codes(weights):
    """{symbol: (code, nbits)}; the code is the value the decoder sees in the nbits it consumes (first bit read = most
    significant).  Weights ascending, symbols ascending inside a weight, fill the table from index 0 (RFC 8878 4.2.1)."""
    total = sum(1 << (w - 1) for w in weights if w)
    mb = highbit(total)
    assert total == 1 << mb, "weights do not complete a power of two"
    codes, pos = {}, 0
    for wt in range(1, mb + 1):
        for s, w in enumerate(weights):
            if w == wt:
                codes[s] = (pos >> (wt - 1), mb + 1 - wt)
                pos += 1 << (wt - 1)
    return codes


def huf_stream(codes, data):
    return pack_backward([codes[b] for b in data])


def weights_direct(weights):
    """header byte 127 + number of sent weights, two 4-bit weights per byte, first in the high nibble"""
    sent = weights[:-1]
    assert 1 <= len(sent) <= 128
    out = bytearray([127 + len(sent)])
    for i in range(0, len(sent), 2):
        out.append((sent[i] << 4) | (sent[i + 1] if i + 1 < len(sent) else 0))
    return bytes(out)


def weights_fse(weights, al=6, norm=None, minus_one=False):
    """header byte = size of what follows: normalised counts, then the weights through two interleaved FSE states
    (the first state decodes the even positions).  The stream ends when the decoder's next update runs out of bits,
    so the last state of the chain that is asked for that update must need at least one bit."""
    sent = weights[:-1]
    assert len(sent) >= 2
    if norm is None:
        hist = [0] * (max(sent) + 1)
        for w in sent:
            hist[w] += 1
        norm = normalize(hist, al, minus_one)
    tab = fse_dtable(norm, al)
    chains = [sent[0::2], sent[1::2]]
    st = [fse_states(tab, c) for c in chains]
    reads = [(st[0][0], al), (st[1][0], al)]
    for i in range(len(sent) - 2):
        chain, k = i & 1, i >> 1
        _, nb, base = tab[st[chain][k]]
        reads.append((st[chain][k + 1] - base, nb))
    phantom = st[(len(sent) - 2) & 1][-1]
    assert tab[phantom][1] > 0, "the closing state would read no bits: the stream's end could not be seen"
    body = write_ncount(norm, al) + pack_backward(reads)
    assert len(body) < 128, "FSE-coded weights too long for the header byte"
    return bytes([len(body)]) + body


# ---------------------------------------------------------------- script objects
class Table:
    """one of the three sequence tables of a compressed block: mode 'predef' | 'rle' | 'fse' | 'repeat'"""

    def __init__(self, mode="predef", norm=None, al=None, minus_one=False, rle_symbol=None, al_field=None, raw=None):
        self.mode, self.norm, self.al, self.minus_one = mode, norm, al, minus_one
        self.rle_symbol, self.al_field, self.raw = rle_symbol, al_field, raw


class Lit:
    """literals section: type 'raw' | 'rle' | 'huf' | 'treeless'; sf = Size_Format (None: smallest that fits)"""

    def __init__(self, type="raw", sf=None, streams=None, weights=None, send="direct", al=6, norm=None, minus_one=False,
                 regen=None, comp=None, tree_bytes=None, jump=None, stream_fix=None):
        self.type, self.sf, self.streams, self.weights, self.send = type, sf, streams, weights, send
        self.al, self.norm, self.minus_one = al, norm, minus_one
        self.regen, self.comp, self.tree_bytes, self.jump, self.stream_fix = regen, comp, tree_bytes, jump, stream_fix


class Comp:
    def __init__(self, literals=b"", seqs=(), lit=None, ll=None, of=None, ml=None, nseq_form=None, nseq_value=None,
                 tail=b"", drop_bits=None, modes_low=0):
        self.literals, self.seqs = bytes(literals), list(seqs)
        self.lit = lit or Lit()
        self.tabs = {"ll": ll or Table(), "of": of or Table(), "ml": ml or Table()}
        self.nseq_form, self.nseq_value, self.tail, self.drop_bits, self.modes_low = nseq_form, nseq_value, tail, drop_bits, modes_low


def Raw(data, size=None):
    return ("raw", bytes(data), size)


def Rle(byte, count, size=None):
    return ("rle", byte, count, size)


def code_of(base, bits, v):
    c = max(i for i in range(len(base)) if base[i] <= v)
    assert v - base[c] < (1 << bits[c]) or (bits[c] == 0 and v == base[c]), v
    return c, v - base[c], bits[c]


class FrameState:
    """what a frame carries from block to block: the output so far, repeat offsets, the last tables and tree"""

    def __init__(self, strict=True):
        self.out = bytearray()
        self.rep = [1, 4, 8]
        self.tabs = {}
        self.weights = None
        self.strict = strict
        self.census = {}

    def count(self, key):
        self.census[key] = self.census.get(key, 0) + 1


def _literals_section(st, c):
    L, data = c.lit, c.literals
    regen = len(data) if L.regen is None else L.regen
    t = {"raw": 0, "rle": 1, "huf": 2, "treeless": 3}[L.type]
    if t < 2:
        if t == 1:
            assert L.regen is not None or len(set(data)) <= 1
        # Size_Format "?0" is ONE bit: in the one-byte header bit 3 is already the low bit of Regenerated_Size, so the
        # field reads 0 for an even size and 2 for an odd one
        sf = L.sf if L.sf is not None else ((regen & 1) * 2 if regen < 32 else 1 if regen < 4096 else 3)
        if sf in (0, 2):
            assert regen < 32 and sf == (regen & 1) * 2, "one-byte header: Size_Format's second bit is the size's low bit"
            head = bytes([t | (regen << 3)])
        elif sf == 1:
            assert regen < 4096
            head = ((t | (1 << 2) | (regen << 4)) & 0xFFFF).to_bytes(2, "little")
        else:
            assert regen < (1 << 20)
            head = (t | (3 << 2) | (regen << 4)).to_bytes(3, "little")
        st.count("lit_%s_sf%d" % (L.type, sf))
        body = data if t == 0 else (data[:1] if data else b"\0")
        return head + body
    # Huffman-coded
    tree = b""
    if t == 2:
        weights = L.weights if L.weights is not None else huf_weights_for(data)
        if L.tree_bytes is not None:
            tree = L.tree_bytes
        elif L.send == "direct":
            tree = weights_direct(weights)
            st.count("huf_direct")
        else:
            tree = weights_fse(weights, L.al, L.norm, L.minus_one)
            st.count("huf_fse")
        st.weights = weights
    else:
        weights = st.weights
        st.count("lit_treeless")
        if weights is None:
            weights = [1, 1]   # (invalid on purpose: no tree to repeat)
    codes = huf_codes(weights) if L.tree_bytes is None else huf_codes(L.weights)
    streams = L.streams or (1 if regen < 1024 and L.sf in (None, 0) else 4)
    if streams == 1:
        payload = huf_stream(codes, data)
        st.count("huf_1stream")
    else:
        q = (len(data) + 3) // 4
        parts = [huf_stream(codes, data[i * q:(i + 1) * q]) for i in range(3)] + [huf_stream(codes, data[3 * q:])]
        if L.stream_fix:
            parts = L.stream_fix(parts)
        jump = L.jump if L.jump is not None else b"".join(len(p).to_bytes(2, "little") for p in parts[:3])
        payload = jump + b"".join(parts)
        st.count("huf_4streams")
    if L.stream_fix and streams == 1:
        payload = L.stream_fix([payload])[0]
    comp = len(tree) + len(payload) if L.comp is None else L.comp
    if L.sf is not None:
        sf = L.sf
    elif streams == 1:
        sf = 0
    else:
        sf = 1 if regen < 1024 and comp < 1024 else 2 if regen < 16384 and comp < 16384 else 3
    assert (sf == 0) == (streams == 1)
    bits = {0: 10, 1: 10, 2: 14, 3: 18}[sf]
    assert regen < (1 << bits) and comp < (1 << bits), (regen, comp, sf)
    head = (t | (sf << 2) | (regen << 4) | (comp << (4 + bits))).to_bytes({10: 3, 14: 4, 18: 5}[bits], "little")
    st.count("lit_huf_sf%d" % sf)
    return head + tree + payload


def _table(st, kind, T, codes_used):
    """returns (mode bits, header bytes, decoding table, accuracy log)"""
    if T.mode == "predef":
        norm, al = DEFAULTS[kind]
        st.tabs[kind] = (fse_dtable(norm, al), al)
        st.count(kind + "_predef")
        return 0, b"", st.tabs[kind]
    if T.mode == "rle":
        st.tabs[kind] = (rle_dtable(codes_used[0]), 0)
        st.count(kind + "_rle")
        return 1, bytes([codes_used[0] if T.rle_symbol is None else T.rle_symbol]), st.tabs[kind]
    if T.mode == "fse":
        al = T.al or 6
        norm = T.norm
        if norm is None:
            hist = [0] * (max(codes_used) + 1)
            for c_ in codes_used:
                hist[c_] += 1
            if sum(1 for h in hist if h) < 2:     # a described table of one symbol is the RLE mode's business
                other = codes_used[0] - 1 if codes_used[0] else 1
                hist += [0] * (other + 1 - len(hist))
                hist[other] += 1
            norm = normalize(hist, al, T.minus_one)
        head = T.raw if T.raw is not None else write_ncount(norm, al, T.al_field)
        st.tabs[kind] = (fse_dtable(norm, al), al)
        st.count(kind + "_fse")
        return 2, head, st.tabs[kind]
    st.count(kind + "_repeat")
    if kind not in st.tabs:        # (invalid on purpose)
        norm, al = DEFAULTS[kind]
        return 3, b"", (fse_dtable(norm, al), al)
    return 3, b"", st.tabs[kind]


def _execute(st, c, block_start):
    """the model: literal runs and matches (RFC 8878 3.1.1.4 / 3.1.1.5)"""
    out, rep, lit, lp = st.out, st.rep, c.literals, 0
    for ll, ml, ofv in c.seqs:
        out += lit[lp:lp + ll]
        lp += ll
        if ofv > 3:
            off = ofv - 3
            rep[:] = [off, rep[0], rep[1]]
        else:
            idx = ofv - 1 + (1 if ll == 0 else 0)
            if idx == 0:
                off = rep[0]
            else:
                off = rep[0] - 1 if idx == 3 else rep[idx]
                if idx == 1:
                    rep[:] = [off, rep[0], rep[2]]
                else:
                    rep[:] = [off, rep[0], rep[1]]
        if st.strict:
            assert 0 < off <= len(out), ("offset beyond the output", off, len(out))
        if off <= 0 or off > len(out):
            out += bytes(ml)       # (an invalid script: the bytes do not matter)
            continue
        if off >= ml:
            out += out[len(out) - off:len(out) - off + ml]
        else:
            pat = bytes(out[len(out) - off:])
            out += (pat * (ml // off + 1))[:ml]
    out += lit[lp:]
    if st.strict:
        assert lp <= len(lit) and len(out) - block_start <= BLOCK_MAX


def compressed_block(st, c):
    """body bytes of one Compressed_Block; appends its plain bytes to st.out"""
    body = bytearray(_literals_section(st, c))
    n = len(c.seqs)
    nv = n if c.nseq_value is None else c.nseq_value
    form = c.nseq_form or (1 if nv < 128 else 2 if nv < 0x7F00 else 3)
    if form == 1:
        assert nv < 128
        body.append(nv)
    elif form == 2:
        assert nv < 0x7F00
        body += bytes([128 + (nv >> 8), nv & 0xFF])
    else:
        assert 0x7F00 <= nv <= 0x7F00 + 0xFFFF
        body += bytes([255]) + (nv - 0x7F00).to_bytes(2, "little")
    st.count("nseq_form%d" % form)
    start = len(st.out)
    if n:
        lc = [code_of(LL_BASE, LL_BITS, ll) for ll, _, _ in c.seqs]
        mc = [code_of(ML_BASE, ML_BITS, ml) for _, ml, _ in c.seqs]
        oc = [(highbit(o), o - (1 << highbit(o)), highbit(o)) for _, _, o in c.seqs]
        used = {"ll": [x[0] for x in lc], "of": [x[0] for x in oc], "ml": [x[0] for x in mc]}
        modes, heads, tabs = 0, b"", {}
        for kind, shift in (("ll", 6), ("of", 4), ("ml", 2)):
            m, h, tabs[kind] = _table(st, kind, c.tabs[kind], used[kind])
            modes |= m << shift
            heads += h
        body.append(modes | c.modes_low)
        body += heads
        states = {k: fse_states(tabs[k][0], used[k]) for k in ("ll", "of", "ml")}
        reads = [(states["ll"][0], tabs["ll"][1]), (states["of"][0], tabs["of"][1]), (states["ml"][0], tabs["ml"][1])]
        for i in range(n):
            reads.append((oc[i][1], oc[i][2]))
            reads.append((mc[i][1], mc[i][2]))
            reads.append((lc[i][1], lc[i][2]))
            if i + 1 < n:
                for k in ("ll", "ml", "of"):
                    _, nb, base = tabs[k][0][states[k][i]]
                    reads.append((states[k][i + 1] - base, nb))
        if c.drop_bits:
            reads = c.drop_bits(reads)
        body += pack_backward(reads)
    body += c.tail
    _execute(st, c, start)
    return bytes(body)


def frame(blocks, single=None, fcs_bytes=None, window=None, checksum=False, dict_id=None, reserved=False,
          fcs_value=None, checksum_xor=0, strict=True, census=None, last_flags=None):
    """(image, plain).  blocks: Raw(..) / Rle(..) / Comp(..) / ("type3", body).  fcs_bytes in (0, 1, 2, 4, 8);
    window = (exponent, mantissa) of the Window_Descriptor (single-segment frames have none); dict_id = (field bytes,
    value).  Defaults: single-segment with the smallest content-size field when every Block_Size fits the content
    size (Block_Maximum_Size is min(Window_Size, 128 KiB) and a single-segment frame's window IS its content size),
    otherwise a window descriptor that covers the frame."""
    st = FrameState(strict)
    body = bytearray()
    sizes = []
    for i, b in enumerate(blocks):
        last = (i == len(blocks) - 1) if last_flags is None else last_flags[i]
        before = len(st.out)
        if isinstance(b, Comp):
            data = compressed_block(st, b)
            btype, bsize = 2, len(data)
            st.count("block_compressed")
        elif b[0] == "raw":
            data, btype = b[1], 0
            bsize = len(data) if b[2] is None else b[2]
            st.out += data
            st.count("block_raw")
        elif b[0] == "rle":
            data, btype = bytes([b[1]]), 1
            bsize = b[2] if b[3] is None else b[3]
            st.out += bytes([b[1]]) * b[2]
            st.count("block_rle")
        else:
            data, btype, bsize = b[1], 3, len(b[1])
        sizes.append(max(bsize, len(st.out) - before, 1 if btype == 1 else 0))    # (an RLE block's one byte counts)
        body += ((1 if last else 0) | (btype << 1) | (bsize << 3)).to_bytes(3, "little") + data
    plain = bytes(st.out)
    n = len(plain) if fcs_value is None else fcs_value
    if single is None:
        single = window is None and max(sizes, default=0) <= n
    if window is None and not single:
        need = max(1024, len(plain), max(sizes, default=0))
        e = max(0, highbit(need - 1) + 1 - 10) if need > 1024 else 0
        window = (e, 0)
    if fcs_bytes is None:
        fcs_bytes = (1 if n < 256 else 2 if n < 65792 else 4 if n < (1 << 32) else 8) if single else 0
    flag = {0: 0, 1: 0, 2: 1, 4: 2, 8: 3}[fcs_bytes]
    assert not (fcs_bytes == 0 and single) and not (fcs_bytes == 1 and not single)
    did_flag = {0: 0, 1: 1, 2: 2, 4: 3}[dict_id[0] if dict_id else 0]
    head = bytearray(MAGIC.to_bytes(4, "little"))
    head.append((flag << 6) | ((1 if single else 0) << 5) | ((1 if reserved else 0) << 3) | ((1 if checksum else 0) << 2) | did_flag)
    if not single:
        head.append((window[0] << 3) | window[1])
        st.count("window_descriptor")
    else:
        st.count("single_segment")
    if dict_id:
        head += dict_id[1].to_bytes(dict_id[0], "little")
    if fcs_bytes:
        head += ((n - 256) & 0xFFFF if fcs_bytes == 2 else n).to_bytes(fcs_bytes, "little")
    st.count("fcs_%d_bytes" % fcs_bytes)
    img = bytes(head) + bytes(body)
    if checksum:
        img += (((xxh64(plain) & 0xFFFFFFFF) ^ checksum_xor)).to_bytes(4, "little")
        st.count("checksum")
    if census is not None:
        for k, v in st.census.items():
            census[k] = census.get(k, 0) + v
    return img, plain


def skippable(payload, nibble=0):
    return (0x184D2A50 + nibble).to_bytes(4, "little") + len(payload).to_bytes(4, "little") + bytes(payload)


# ---------------------------------------------------------------- the hand-built cases
# device statuses (include/la_gpu.h)
ST_OK, ST_CORRUPT, ST_TRUNCATED, ST_BAD_CHECKSUM, ST_OUT_FULL, ST_UNSUPPORTED, ST_WINDOW, ST_DICTIONARY = 0, 11, 12, 13, 14, 15, 16, 17


class Case:
    """status: what the device must answer (ST_OK: a valid frame; None: truncation, "12 or 11 as the oracle says")"""

    def __init__(self, name, image, plain, status):
        self.name, self.image, self.plain, self.status = name, image, plain, status
        self.valid = status == ST_OK


def _bytes(rnd, n, alphabet=256):
    return bytes(rnd.randrange(alphabet) for _ in range(n))


class Seqs:
    """sequence list with the output position tracked, so that a match source can be named by position"""

    def __init__(self, start):
        self.pos, self.seqs, self.nlit, self.ends = start, [], 0, []

    def add(self, ll, ml, src=None, off=None, ofv=None):
        """src: absolute position of the first source byte; off: distance; ofv: the coded value as is"""
        at = self.pos + ll
        if ofv is None:
            ofv = (at - src if off is None else off) + 3
        self.seqs.append((ll, ml, ofv))
        self.nlit += ll
        self.pos = at + ml
        self.ends.append(self.pos)
        return at


def _rep_offset(rep, ll, ofv):
    """the offset a coded value stands for, and the history after it (RFC 8878 3.1.1.5)"""
    if ofv > 3:
        return ofv - 3, [ofv - 3, rep[0], rep[1]]
    idx = ofv - 1 + (1 if ll == 0 else 0)
    if idx == 0:
        return rep[0], list(rep)
    off = rep[0] - 1 if idx == 3 else rep[idx]
    return off, ([off, rep[0], rep[2]] if idx == 1 else [off, rep[0], rep[1]])


def random_frame(rnd):
    """one frame drawing from everything above; every choice keeps the frame valid"""
    blocks, out_len, rep = [], 0, [1, 4, 8]
    avail, tree_syms = {}, None
    for _ in range(rnd.randint(1, 4)):
        kind = rnd.choice("rrlcccc")
        if kind == "r":
            d = _bytes(rnd, rnd.choice([0, 1, 7, 40, 300]), rnd.choice([2, 16, 256]))
            blocks.append(Raw(d)); out_len += len(d)
            continue
        if kind == "l":
            n = rnd.choice([0, 1, 5, 100, 5000])
            blocks.append(Rle(rnd.randrange(256), n)); out_len += n
            continue
        ltype = rnd.choice(["raw", "raw", "rle", "huf", "huf", "huf", "treeless"])
        if ltype == "treeless" and tree_syms is None:
            ltype = "huf"
        nlit = rnd.choice([0, 1, 3, 31, 32, 200, 1023, 1024, 3000]) if ltype in ("raw", "rle") else rnd.choice([20, 64, 300, 1023, 1024, 5000])
        if ltype == "rle":
            lits = bytes([rnd.randrange(256)]) * nlit
        elif ltype == "treeless":
            lits = bytes(rnd.choice(tree_syms) for _ in range(nlit))
        else:
            k = rnd.choice([2, 3, 17, 129, 256])
            lo = rnd.randrange(0, 257 - k)
            lits = bytes(lo + min(int(rnd.expovariate(6.0 / k)), k - 1) for _ in range(nlit))
        seqs, lp, pos = [], 0, out_len
        used = {"ll": set(), "of": set(), "ml": set()}
        want = rnd.choice([0, 1, 2, 5, 30, 63, 64, 65, 130]) if out_len + nlit > 0 else 0
        for i in range(want):
            left = want - i
            ll = min(rnd.choice([0, 0, 1, 2, 5, 17, 40]), (nlit - lp) // left if i else nlit - lp)
            if pos + ll == 0:
                ll = min(1, nlit - lp)
                if ll == 0:
                    break
            ml = rnd.choice([3, 3, 4, 7, 18, 35, 36, 70, 300])
            if pos + ll + ml - out_len > 60000:
                break
            ofv = rnd.choice([1, 2, 3]) if rnd.random() < 0.35 else rnd.randint(1, min(pos + ll, rnd.choice([8, 300, 1 << 20]))) + 3
            off, nrep = _rep_offset(rep, ll, ofv)
            if not 0 < off <= pos + ll:
                ofv = rnd.randint(1, pos + ll) + 3
                off, nrep = _rep_offset(rep, ll, ofv)
            rep = nrep
            seqs.append((ll, ml, ofv)); lp += ll; pos += ll + ml
            used["ll"].add(code_of(LL_BASE, LL_BITS, ll)[0]); used["ml"].add(code_of(ML_BASE, ML_BITS, ml)[0]); used["of"].add(highbit(ofv))
        tabs = {}
        for k in ("ll", "of", "ml"):
            modes = ["predef", "fse", "fse"]
            if len(used[k]) == 1:
                modes += ["rle", "rle"]
            if seqs and k in avail and used[k] <= avail[k]:
                modes += ["repeat", "repeat"]
            m = rnd.choice(modes)
            if m == "fse" and len(used[k]) > 24:
                m = "predef"
            tabs[k] = Table(m, al=rnd.choice([5, 6, 7, MAX_AL[k]]) if len(used[k]) < 30 else MAX_AL[k], minus_one=rnd.random() < 0.4)
            if seqs and m != "repeat":
                avail[k] = set(range(len(DEFAULTS[k][0]))) if m == "predef" else set(used[k])
                if m == "fse" and len(used[k]) == 1:
                    c0 = next(iter(used[k]))
                    avail[k].add(c0 - 1 if c0 else 1)
        if not seqs and nlit == 0:      # (a compressed block holds at least three bytes)
            blocks.append(Raw(b""))
            continue
        lit = Lit(ltype)
        if ltype in ("huf", "treeless"):
            lit.streams = 4 if nlit >= 1024 or rnd.random() < 0.5 else 1
            if ltype == "huf":
                w = huf_weights_for(lits)
                lit.weights = w
                lit.send = "fse" if (len(w) > 129 or (len(w) > 3 and rnd.random() < 0.5)) else "direct"
                lit.al = 6 if len(w) > 40 else rnd.choice([5, 6])
                tree_syms = [s for s, x in enumerate(w) if x]
        elif nlit < 32:
            lit.sf = rnd.choice([(nlit & 1) * 2, 1, 3])
        blocks.append(Comp(lits, seqs, lit=lit, ll=tabs["ll"], of=tabs["of"], ml=tabs["ml"],
                           nseq_form=rnd.choice([None, 2]) if 0 < len(seqs) < 128 else None))
        out_len = pos + (nlit - lp)
    kw = {"checksum": rnd.random() < 0.5}
    if rnd.random() < 0.5:
        e = max(0, highbit(max(out_len, 1024) - 1) + 1 - 10) + rnd.randint(0, 3)
        kw.update(window=(e, rnd.randrange(8)), single=False, fcs_bytes=rnd.choice([0, 0, 4, 8] + ([2] if 256 <= out_len < 65792 else [])))
    return blocks, kw


HIST = bytes((i * 37 + 11) & 0xFF for i in range(64))


def handbuilt_cases(census=None, big=True):
    """[Case].  big=False leaves out the frames whose plain bytes pass 1 MiB (quick experiments only)."""
    import random
    rnd = random.Random(0x5A57D)
    cases = []

    def ok(name, blocks, **kw):
        img, plain = frame(blocks, census=census, **kw)
        cases.append(Case(name, img, plain, ST_OK))
        return img, plain

    def bad(name, status, blocks, **kw):
        kw.setdefault("strict", False)
        img, plain = frame(blocks, **kw)
        cases.append(Case(name, img, None, status))
        return img

    # ---- frame headers
    for n in (0, 255, 256, 65791, 65792):
        data = _bytes(rnd, n)
        blocks = [Raw(data)] if n else [Raw(b"")]
        for fb in (0, 1, 2, 4, 8):
            if (fb == 1 and n > 255) or (fb == 2 and not 256 <= n < 65792):
                continue
            for cs in (False, True):
                if fb == 0:
                    ok("hdr-fcs0-n%d-cs%d" % (n, cs), blocks, single=False, fcs_bytes=0, checksum=cs)
                else:
                    ok("hdr-fcs%d-single-n%d-cs%d" % (fb, n, cs), blocks, single=True, fcs_bytes=fb, checksum=cs)
                    if fb != 1:
                        ok("hdr-fcs%d-window-n%d-cs%d" % (fb, n, cs), blocks, single=False, window=(7, 3), fcs_bytes=fb, checksum=cs)
    for e, m in ((0, 0), (0, 7), (1, 1), (5, 4), (10, 0), (16, 7), (17, 0)):
        ok("hdr-window-e%d-m%d" % (e, m), [Raw(HIST), Rle(9, 900)], window=(e, m), single=False)
    ok("hdr-empty-no-block-bytes", [Raw(b"")], single=True)
    ok("hdr-empty-rle0", [Rle(7, 0)], single=False, window=(0, 0), checksum=True)

    # ---- blocks
    big_raw = _bytes(rnd, BLOCK_MAX)
    ok("blk-mixed", [Raw(HIST), Rle(1, 77), Comp(b"xyz" * 5, [(3, 9, 3 + 70), (2, 4, 3 + 150)]), Raw(b""), Raw(b"q"), Rle(2, 1),
                     Comp(b"lit", [])], checksum=True)
    ok("blk-raw-128k", [Raw(big_raw)], checksum=True)
    ok("blk-rle-128k", [Rle(0xEE, BLOCK_MAX)])
    ok("blk-comp-regen-128k-literals-only", [Comp(b"z" * BLOCK_MAX, [], lit=Lit("rle"))], checksum=True)
    ok("blk-comp-regen-128k-one-match", [Raw(HIST), Comp(b"ab", [(2, BLOCK_MAX - 2, 3 + 66)])], window=(8, 0), single=False)
    s = Seqs(64 + 500 + 40)
    s.add(2, 20, src=10); s.add(1, 30, src=64 + 490); s.add(0, 12, src=64 + 500 + 5); s.add(3, 50, src=40)
    ok("blk-matches-into-raw-rle-comp", [Raw(HIST), Rle(3, 500), Comp(_bytes(rnd, 20), [(10, 10, 3 + 30), (10, 10, 3 + 520)]),
                                         Comp(_bytes(rnd, 6), s.seqs)], checksum=True)

    # ---- literals
    for t in ("raw", "rle"):
        for sf, n in ((0, 0), (0, 30), (2, 5), (2, 31), (1, 32), (1, 4095), (1, 7), (3, 4096), (3, 9), (3, 70000)):
            d = (_bytes(rnd, n) if t == "raw" else b"r" * n)
            ok("lit-%s-sf%d-n%d" % (t, sf, n), [Raw(HIST), Comp(d, [(0, 4, 3 + 9)] if n % 2 or n == 0 else [], lit=Lit(t, sf=sf))])
    ok("lit-rle-128k", [Comp(b"\x00" * BLOCK_MAX, [], lit=Lit("rle", sf=3))])
    text = bytes(97 + min(int(rnd.expovariate(0.4)), 25) for _ in range(20000))
    ok("lit-huf-1stream", [Comp(text[:900], [(5, 5, 3 + 3)], lit=Lit("huf", streams=1))])
    for sf, n in ((1, 1000), (2, 16000), (3, 20000), (3, 500), (2, 40)):
        ok("lit-huf-4streams-sf%d-n%d" % (sf, n), [Comp(text[:n], [(5, 5, 3 + 3)], lit=Lit("huf", streams=4, sf=sf))])
    for n in (6, 7, 8, 9, 10, 11, 12, 13):
        ok("lit-huf-4streams-n%d" % n, [Raw(HIST), Comp(text[:n], [], lit=Lit("huf", streams=4))])
    for nsent in (1, 2, 3, 4, 15, 16, 64, 127, 128):
        d = bytes(min(int(rnd.expovariate(3.0 / (nsent + 1))), nsent) for _ in range(40 * (nsent + 1))) + bytes(range(nsent + 1))
        w = huf_weights_for(d)
        assert len(w) == nsent + 1
        ok("lit-huf-direct-%dweights" % nsent, [Comp(d, [(1, 3, 3 + 1)], lit=Lit("huf", weights=w, send="direct", streams=4 if nsent & 1 or len(d) > 1000 else 1))])
    wide = bytes(range(256)) * 2 + bytes(int(rnd.triangular(0, 255, 60)) for _ in range(6000))
    for al in (5, 6):
        ok("lit-huf-fse-al%d-256symbols" % al, [Comp(wide, [(9, 9, 3 + 4)], lit=Lit("huf", send="fse", al=al, streams=4))])
        ok("lit-huf-fse-al%d-minus1" % al, [Comp(text[:3000] + bytes([255, 254, 200]), [(9, 9, 3 + 4)], lit=Lit("huf", send="fse", al=al, minus_one=True, streams=4))])
    ok("lit-huf-two-symbols", [Comp(b"\x00\x01\x01\x00\x00\x00\x01\x00" * 9, [], lit=Lit("huf", streams=1))])
    deep = b"".join(bytes([i]) * (1 if i == 0 else 1 << (i - 1)) for i in range(12))
    w = huf_weights_for(deep)
    assert sorted(w)[-1] == 11 and 1 in w
    ok("lit-huf-depth-11", [Comp(bytes(rnd.sample(list(deep), len(deep))), [(1, 3, 3 + 1)], lit=Lit("huf", weights=w, streams=4))])
    ok("lit-treeless-after-tree", [Comp(text[:700], [(5, 5, 3 + 3)], lit=Lit("huf", streams=1, weights=huf_weights_for(text))),
                                   Comp(text[700:2900], [(5, 5, 3 + 3)], lit=Lit("treeless", streams=4)),
                                   Comp(text[3000:3100], [], lit=Lit("treeless", streams=1))])
    ok("lit-treeless-after-raw-literal-blocks", [Comp(text[:700], [], lit=Lit("huf", streams=4, weights=huf_weights_for(text))), Comp(b"raw lits", [(1, 3, 3 + 2)]),
                                                 Raw(b"between"), Rle(5, 50), Comp(b"", [(0, 3, 3 + 5)]),
                                                 Comp(text[1000:1300], [(5, 5, 1)], lit=Lit("treeless", streams=1))], checksum=True)

    # ---- sequences: counts
    for n in (1, 63, 64, 65, 127, 128, 129, 0x7EFF, 0x7F00, 0x7F01):
        if n <= 129:
            ok("seq-count-%d" % n, [Raw(HIST), Comp(_bytes(rnd, n + 3), [(1, 4, 3 + 8 + (i % 50)) for i in range(n)])], checksum=True)
            if n < 128:
                ok("seq-count-%d-2byte-form" % n, [Raw(HIST), Comp(_bytes(rnd, n), [(1, 4, 3 + 8)] * n, nseq_form=2)])
        else:
            ok("seq-count-%d" % n, [Raw(HIST), Comp(_bytes(rnd, n // 16 + 1), [(1 if i % 16 == 0 else 0, 3, 3 + 1 + (i % 60)) for i in range(n)])], checksum=True)
    nmax = (BLOCK_MAX - 2) // 3
    ok("seq-count-largest-%d" % nmax, [Raw(b"ab"), Comp(b"", [(0, 3, 3 + 2)] * nmax, ll=Table("rle"), of=Table("rle"), ml=Table("rle"))],
       window=(8, 0), single=False)

    # ---- sequences: the 64 mode combinations, each followed by a block in repeat mode
    names = ("predef", "rle", "fse", "repeat")
    for combo in range(64):
        m = [names[(combo >> 4) & 3], names[(combo >> 2) & 3], names[combo & 3]]
        tabs = [Table(x, al=5 + (combo % 3)) for x in m]
        # a "repeat" needs something to repeat ("repeat" in a first block: see the refusals): a block of described tables
        lead = [Comp(_bytes(rnd, 12), [(2, 5, 3 + 7)] * 3 + [(1, 6, 3 + 9)], ll=Table("fse"), of=Table("fse"), ml=Table("fse"))] if "repeat" in m else []
        # sequences whose codes every mode can carry: one code per table (RLE), present in the lead block's tables
        seqs = [(2, 5, 3 + 7)] * 5
        ok("seq-modes-%s-%s-%s" % tuple(m), [Raw(HIST)] + lead + [Comp(_bytes(rnd, 10), seqs, ll=tabs[0], of=tabs[1], ml=tabs[2]),
           Comp(_bytes(rnd, 6), [(2, 5, 3 + 7)] * 3, ll=Table("repeat"), of=Table("repeat"), ml=Table("repeat"))])

    # ---- sequences: described tables
    many = [(i % 20, 3 + (i * 7) % 50, 3 + 1 + (i * 13) % 60) for i in range(200)]
    for al_ll, al_of, al_ml, m1 in ((5, 5, 5, False), (9, 8, 9, False), (6, 6, 7, True), (9, 8, 9, True)):
        few = many if al_ll > 5 else [(i % 4, 3 + i % 5, 3 + 1 + (i % 3) * 20) for i in range(50)]
        ok("seq-fse-al-%d-%d-%d-minus1-%d" % (al_ll, al_of, al_ml, m1), [Raw(HIST), Comp(_bytes(rnd, sum(x[0] for x in few)), few,
           ll=Table("fse", al=al_ll, minus_one=m1), of=Table("fse", al=al_of, minus_one=m1), ml=Table("fse", al=al_ml, minus_one=m1))])
    # zero runs: codes 0 and 30 (LL), 2 and 20 (OF), 0 and 45 (ML): runs of 29, 17 and 44 zero counts (chained flags)
    ok("seq-fse-chained-zero-runs", [Raw(HIST * 3)] + [Rle(4 + i, BLOCK_MAX) for i in range(8)] + [Comp(bytes(3000), [(0, 3, 3 + 1), (2048, 3 + 8195 - 3, (1 << 20) + 5), (0, 3, 3 + 1), (0, 3, 4)],
       ll=Table("fse", al=6), of=Table("fse", al=5), ml=Table("fse", al=6))], window=(11, 0), single=False)

    # ---- every literal-length and match-length code, extra bits all zero and all one ("max": the most the 128 KiB a
    # block may produce leave room for, which is all ones except for LL 35 and ML 52)
    ok("seq-ll-codes-0-15", [Raw(HIST), Comp(_bytes(rnd, 120), [(c, 3, 3 + 5) for c in range(16)])])
    ok("seq-ml-codes-0-31", [Raw(HIST), Comp(b"", [(0, 3 + c, 3 + 5) for c in range(32)])])
    for c in range(16, 36):
        for ones in (0, 1):
            ll = LL_BASE[c] + (min((1 << LL_BITS[c]) - 1, BLOCK_MAX - 3 - LL_BASE[c]) if ones else 0)
            ok("seq-ll-code-%d-extra-%s" % (c, "max" if ones else "zero"), [Raw(HIST), Comp(bytes([c]) * ll, [(ll, 3, 3 + 2)], lit=Lit("rle"))], window=(8, 0), single=False)
    for c in range(32, 53):
        for ones in (0, 1):
            ml = ML_BASE[c] + (min((1 << ML_BITS[c]) - 1, BLOCK_MAX - ML_BASE[c]) if ones else 0)
            ok("seq-ml-code-%d-extra-%s" % (c, "max" if ones else "zero"), [Raw(HIST), Comp(b"", [(0, ml, 3 + 7)])], window=(8, 0), single=False)
    ok("seq-31-extra-bits-ll35-ml51", [Raw(HIST), Comp(b"w" * (65536 + 0x3FFD), [(65536 + 0x3FFD, 32771 + 0x3FFF, 3 + 64)], lit=Lit("rle"))], window=(8, 0), single=False)
    ok("seq-31-extra-bits-ll34-ml52", [Raw(HIST), Comp(b"w" * (32768 + 0x3FFD), [(32768 + 0x3FFD, 65539 + 0x3FFF, 3 + 64)], lit=Lit("rle"))], window=(8, 0), single=False)

    # ---- every offset code up to 24: a frame of 17 MiB of RLE blocks, reached back to its start
    if big:
        nb = 136
        blocks = [Raw(big_raw)] + [Rle(i, BLOCK_MAX) for i in range(1, nb)]
        total = nb * BLOCK_MAX
        seqs = [(1, 8, (1 << c) + ((1 << c) - 1 if c < 24 else total + 1 - 8 + 3 - (1 << 24))) for c in range(2, 25)] + \
               [(0, 5, (1 << c)) for c in range(2, 25)]
        for pre, tab in (("predef", Table()), ("fse", Table("fse", al=8))):
            ok("seq-offset-codes-2-24-%s-17MiB" % pre, blocks + [Comp(_bytes(rnd, 30), seqs, of=tab)], window=(15, 0), single=False, checksum=True)

    # ---- repeat offsets
    reps = [(2, 4, 1), (0, 3, 1), (1, 3, 2), (0, 3, 2), (1, 3, 3), (0, 4, 3 + 20), (0, 3, 3), (3, 5, 3 + 33), (1, 3, 1), (0, 5, 2), (0, 3, 3), (2, 3, 3)]
    ok("seq-repeat-initial-1-4-8", [Raw(HIST[:8]), Comp(b"abcdef", [(1, 3, 3), (1, 3, 3), (1, 3, 3), (0, 3, 1), (0, 3, 2), (1, 3, 1)])])
    ok("seq-repeat-every-form", [Raw(HIST), Comp(_bytes(rnd, 12), reps)], checksum=True)
    ok("seq-repeat-carried-across-blocks", [Raw(HIST), Comp(_bytes(rnd, 12), reps), Comp(b"nosq", []), Comp(b"ab", [(1, 3, 1), (0, 3, 1)]),
                                            Raw(b"raw block"), Comp(b"cd", [(1, 3, 2), (0, 3, 3)]), Rle(8, 30), Comp(b"ef", [(1, 4, 3), (1, 3, 1)])], checksum=True)

    # ---- overlap matches
    for off in range(1, 9):
        ok("seq-overlap-offset-%d-ml-%d" % (off, 65540 + off * 11), [Comp(HIST[:8], [(8, 65540 + off * 11, 3 + off)])], window=(8, 0), single=False, checksum=True)
    for ml in (3, 8, 9, 64, 65, 1000):
        ok("seq-overlap-offset-eq-ml-%d" % ml, [Raw(HIST * 16), Comp(b"", [(0, ml, 3 + ml), (0, ml, 3 + ml - 1), (0, ml + 1, 3 + ml)])])

    # ---- the wave kernel's 64-sequence groups
    ok("grp-chain-through-all-lanes", [Raw(HIST[:8]), Comp(b"", [(0, 8, 3 + 8)] * 200)], checksum=True)
    ok("grp-chain-with-literals", [Raw(HIST[:8]), Comp(_bytes(rnd, 150), [(1, 9, 3 + 9)] * 150)], checksum=True)
    ok("grp-chain-overlapping", [Raw(HIST[:8]), Comp(b"", [(0, 11, 3 + 3)] * 140)], checksum=True)
    s = Seqs(64)
    for i in range(20):
        s.add(1, 3, src=i)
    s.add(0, 60, src=64 + 5)                       # spans fifteen lanes' outputs
    s.add(0, 30, src=s.ends[20] - 30)              # the whole of it inside the previous lane's match
    a = s.add(12, 3, src=0)                        # (a literal run to aim at)
    s.add(1, 10, src=a - 12 + 1)                   # lies only in that lane's literal run
    s.add(0, 12, src=a - 12)                       # exactly that literal run
    s.add(0, 7, src=s.ends[5] - 7)                 # ends exactly at lane 5's boundary
    s.add(0, 9, src=s.ends[5])                     # begins exactly at it
    s.add(2, 4, src=s.ends[-1] - 1)                # the predecessor's last byte, then own literals (overlap)
    for i in range(50):
        s.add(i % 3, 5 + i % 9, src=s.ends[max(0, len(s.ends) - 1 - i % 40)] - 4)
    ok("grp-sources-inside-the-group", [Raw(HIST), Comp(_bytes(rnd, s.nlit + 5), s.seqs)], checksum=True)

    # ---- seeded random scripts
    for i in range(320):
        blocks, kw = random_frame(rnd)
        ok("random-%03d" % i, blocks, **kw)

    # ================================================================ refusals
    good = [Raw(HIST), Comp(b"literals", [(4, 5, 3 + 10), (2, 3, 1)])]
    bad("bad-reserved-header-bit", ST_UNSUPPORTED, good, reserved=True)
    for n in (1, 2, 4):
        bad("bad-dictionary-id-%d-bytes" % n, ST_DICTIONARY, good, dict_id=(n, 0x5D if n == 1 else 0x1234 if n == 2 else 0x12345678))
    bad("bad-window-descriptor-2^28", ST_WINDOW, good, window=(18, 0), single=False)
    bad("bad-window-descriptor-2^27-plus", ST_WINDOW, good, window=(17, 1), single=False)
    bad("bad-window-single-segment-size", ST_WINDOW, good, single=True, fcs_bytes=8, fcs_value=(1 << 27) + 2)
    # ZSTD_decompressStream's default limit is (1 << 27) + 1: this size passes the window check and fails as a wrong content size
    bad("bad-content-size-at-the-window-limit", ST_CORRUPT, good, single=True, fcs_bytes=8, fcs_value=(1 << 27) + 1)
    bad("bad-checksum", ST_BAD_CHECKSUM, good, checksum=True, checksum_xor=0x00010000)
    c = ST_CORRUPT
    bad("bad-content-size-larger", c, good, single=False, window=(0, 0), fcs_bytes=4, fcs_value=64 + 19 + 1)
    bad("bad-content-size-smaller", c, good, single=False, window=(0, 0), fcs_bytes=4, fcs_value=64 + 19 - 1)
    bad("bad-block-type-3", c, [Raw(HIST), ("type3", b"abc")])
    bad("bad-block-above-128k", c, [Raw(bytes(BLOCK_MAX + 1))], window=(8, 0), single=False)
    bad("bad-rle-block-above-128k", c, [Rle(1, BLOCK_MAX + 1)], window=(8, 0), single=False)
    bad("bad-raw-block-larger-than-window", c, [Raw(bytes(2048))], window=(0, 0), single=False)
    bad("bad-raw-block-above-window-and-past-the-input", c, [Raw(HIST), Raw(bytes(100), size=2000)], window=(0, 0), single=False)
    bad("bad-rle-block-larger-than-window", c, [Rle(1, 2048)], window=(0, 0), single=False)
    bad("bad-rle-block-larger-than-window-mantissa", c, [Raw(HIST), Rle(1, 1024 + 128 * 3 + 1)], window=(0, 3), single=False)
    bad("bad-compressed-block-produces-more-than-window", c, [Raw(HIST), Comp(b"", [(0, 1100, 3 + 1)])], window=(0, 0), single=False)
    bad("bad-compressed-block-size-above-window", c, [Comp(_bytes(rnd, 1025), [])], window=(0, 0), single=False)
    bad("bad-single-segment-block-size-above-content-size", c, [Comp(b"abcab", [], lit=Lit("huf", streams=1))], single=True)
    bad("bad-compressed-block-of-2-bytes", c, [Raw(HIST), Comp(b"", [])], window=(0, 0), single=False)
    bad("bad-literals-regenerate-above-128k", c, [Comp(b"x", [], lit=Lit("rle", sf=3, regen=BLOCK_MAX + 1))], window=(8, 0), single=False)
    bad("bad-literals-compressed-size-past-block", c, [Comp(text[:500], [], lit=Lit("huf", streams=1, comp=900))], window=(0, 0), single=False)
    two = b"\x00\x01" * 40

    def tree(nibbles):      # direct weights as given
        return bytes([127 + len(nibbles)]) + bytes((nibbles[i] << 4) | (nibbles[i + 1] if i + 1 < len(nibbles) else 0) for i in range(0, len(nibbles), 2))
    bad("bad-weights-sum-not-completable", c, [Comp(two, [], lit=Lit("huf", streams=1, weights=[1, 1], tree_bytes=tree([3, 1])))], window=(0, 0), single=False)
    bad("bad-weight-above-11", c, [Comp(two, [], lit=Lit("huf", streams=1, weights=[1, 1], tree_bytes=tree([12, 1])))], window=(0, 0), single=False)
    bad("bad-tree-depth-above-11", c, [Comp(two, [], lit=Lit("huf", streams=1, weights=[1, 1], tree_bytes=tree([11, 11])))], window=(0, 0), single=False)
    bad("bad-huffman-stream-ends-off-zero", c, [Comp(text[:400], [], lit=Lit("huf", streams=1, regen=399))], window=(0, 0), single=False)
    bad("bad-huffman-stream-last-byte-zero", c, [Comp(text[:400], [], lit=Lit("huf", streams=1, stream_fix=lambda p: [p[0] + b"\0"]))], window=(0, 0), single=False)
    bad("bad-huffman-4streams-last-byte-zero", c, [Comp(text[:400], [], lit=Lit("huf", streams=4, stream_fix=lambda p: p[:2] + [p[2][:-1] + b"\0"] + p[3:]))], window=(0, 0), single=False)
    bad("bad-jump-table-past-section", c, [Comp(text[:400], [], lit=Lit("huf", streams=4, jump=b"\xff\xff" * 3))], window=(0, 0), single=False)
    bad("bad-treeless-without-tree", c, [Raw(HIST), Comp(two, [], lit=Lit("treeless", streams=1))], window=(0, 0), single=False)
    bad("bad-4streams-regen-5", c, [Raw(HIST), Comp(text[:5], [], lit=Lit("huf", streams=4))], window=(0, 0), single=False)
    sq = [(2, 5, 3 + 7), (1, 6, 3 + 9), (0, 4, 3 + 7)]
    for k, mx in (("ll", 9), ("of", 8), ("ml", 9)):
        tb = {k: Table("fse", al=6, al_field=mx + 1)}
        bad("bad-%s-accuracy-log-above-%d" % (k, mx), c, [Raw(HIST), Comp(b"abcdef", sq, **tb)], window=(0, 0), single=False)
        tb = {k: Table("fse", al=6, norm=[1] * (MAX_SYM[k] + 1) + [64 - MAX_SYM[k] - 2, 1], raw=write_ncount([1] * (MAX_SYM[k] + 1) + [64 - MAX_SYM[k] - 2, 1], 6))}
        bad("bad-%s-described-symbol-above-%d" % (k, MAX_SYM[k]), c, [Raw(HIST), Comp(b"abcdef", [(2, 5, 3 + 7)] * 3, **tb)], window=(0, 0), single=False)
        tb = {k: Table("rle", rle_symbol=MAX_SYM[k] + 1)}
        bad("bad-%s-rle-symbol-above-%d" % (k, MAX_SYM[k]), c, [Raw(HIST), Comp(b"abcdef", [(2, 5, 3 + 7)] * 3, **tb)], window=(0, 0), single=False)
        tb = {k: Table("repeat")}
        bad("bad-%s-repeat-without-table" % k, c, [Raw(HIST), Comp(b"abcdef", sq, **tb)], window=(0, 0), single=False)
    bad("bad-literal-length-past-literals", c, [Raw(HIST), Comp(b"abc", [(2, 5, 3 + 7), (2, 5, 3 + 7)])], window=(0, 0), single=False)
    bad("bad-offset-beyond-output", c, [Raw(HIST), Comp(b"abc", [(2, 5, 3 + 67)])], window=(0, 0), single=False)
    bad("bad-offset-beyond-output-first-byte", c, [Comp(b"abc", [(0, 5, 3 + 1)])], window=(0, 0), single=False)
    bad("bad-repeat-offset-1-minus-1", c, [Raw(HIST), Comp(b"abc", [(0, 3, 3)])], window=(0, 0), single=False)
    bad("bad-sequence-bits-run-out", c, [Raw(HIST), Comp(b"abcdef", sq + [(1, 40, 3 + 50)], drop_bits=lambda r: r[:-4])], window=(0, 0), single=False)
    bad("bad-sequence-bits-left-over", c, [Raw(HIST), Comp(b"abcdef", sq, drop_bits=lambda r: r + [(5, 3)])], window=(0, 0), single=False)
    bad("bad-block-produces-more-than-128k", c, [Raw(HIST), Comp(b"y" * 70000, [(70000, 65539, 3 + 2)], lit=Lit("rle"))], window=(8, 0), single=False)
    bad("bad-zero-sequences-in-2-byte-form", c, [Raw(HIST), Comp(b"abc", [], nseq_form=2)], window=(0, 0), single=False)
    bad("bad-zero-sequences-in-2-byte-form-with-modes-byte", c, [Raw(HIST), Comp(b"abc", [], nseq_form=2, tail=b"\x00")], window=(0, 0), single=False)
    bad("bad-rle-block-in-frame-of-content-size-0", c, [Rle(7, 0)], single=True)
    bad("bad-bytes-after-zero-sequences", c, [Raw(HIST), Comp(b"abc", [], tail=b"\x00")], window=(0, 0), single=False)
    bad("bad-sequence-count-without-modes-byte", c, [Raw(HIST), Comp(b"abc", [], nseq_value=2)], window=(0, 0), single=False)
    # truncation of a small frame at every byte: 12 or 11, as the oracle says
    img, _ = frame([Raw(b"tr"), Rle(1, 5), Comp(text[:40], [(5, 5, 3 + 3), (1, 5, 1)], lit=Lit("huf", streams=1), ll=Table("fse"), of=Table("fse"), ml=Table("rle"))],
                   checksum=True, single=False, window=(0, 0), fcs_bytes=4)
    for cut in range(1, len(img)):
        cases.append(Case("trunc-at-%03d-of-%d" % (cut, len(img)), img[:cut], None, None))
    assert len({x.name for x in cases}) == len(cases)
    return cases
