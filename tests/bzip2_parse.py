"""A plain Python reading of bzip2 blocks, written from the format, for the compressor's tests: the header fields, the
tables' code lengths, the selectors and (on request) the decoded MTF / RLE2 symbols with their zero-run lengths.  Plus
a model of the block transform (RLE1, rotation sort, MTF, RLE2) for inputs small enough to sort in Python, which says
how many symbols a block of given bytes has."""
import bzip2_support as BS

RUNA, RUNB = 0, 1


class Bits:
    """MSB-first bit reader over bytes; every read looks at eight bytes around the position, so it costs the same
    anywhere in a long image"""

    def __init__(self, data, bit=0):
        self.d, self.n, self.bit = bytes(data) + bytes(8), len(data) * 8, bit

    def get(self, n):
        assert n <= 56 and self.bit + n <= self.n, "ran off the image"
        i = self.bit >> 3
        r = (int.from_bytes(self.d[i:i + 8], "big") >> (64 - (self.bit & 7) - n)) & ((1 << n) - 1)
        self.bit += n
        return r


def parse_block(image, bit, symbols=False, bits=None):
    """The block whose 48-bit magic starts at `bit`.  With symbols=True also "symbols", "zero_runs" and "end_bit"."""
    b = bits or Bits(image)
    b.bit = bit
    assert b.get(48) == BS.BLOCK_MAGIC
    blk = {"crc": b.get(32), "randomised": b.get(1), "orig_ptr": b.get(24)}
    ranges = b.get(16)
    used = []
    for r in range(16):
        if ranges >> (15 - r) & 1:
            m = b.get(16)
            used += [16 * r + k for k in range(16) if m >> (15 - k) & 1]
    alpha = len(used) + 2
    blk["used"], blk["n_tables"], blk["n_selectors"] = used, b.get(3), b.get(15)
    order, sels = list(range(blk["n_tables"])), []
    for _ in range(blk["n_selectors"]):
        j = 0
        while b.get(1):
            j += 1
            assert j < blk["n_tables"]
        order.insert(0, order.pop(j))
        sels.append(order[0])
    blk["selectors"] = sels
    lengths = []
    for _ in range(blk["n_tables"]):
        cur, row = b.get(5), []
        for _ in range(alpha):
            while b.get(1):
                cur += -1 if b.get(1) else 1
            assert 1 <= cur <= 20
            row.append(cur)
        lengths.append(row)
    blk["lengths"] = lengths
    if not symbols:
        return blk
    decode = []
    for row in lengths:
        code, table = 0, {}
        for ln in range(1, max(row) + 1):
            for s, l in enumerate(row):
                if l == ln:
                    table[(ln, code)] = s
                    code += 1
            code <<= 1
        decode.append(table)
    syms, eob = [], alpha - 1
    data, pos, nbits = b.d, b.bit, b.n
    while True:
        assert len(syms) // 50 < len(sels), "more groups than selectors"
        table = decode[sels[len(syms) // 50]]
        i = pos >> 3
        window = (int.from_bytes(data[i:i + 4], "big") >> (12 - (pos & 7))) & 0xFFFFF      # the 20 bits ahead
        for ln in range(1, 21):
            s = table.get((ln, window >> (20 - ln)))
            if s is not None:
                break
        else:
            raise AssertionError("no code of 20 bits or fewer")
        pos += ln
        assert pos <= nbits, "ran off the image"
        syms.append(s)
        if s == eob:
            break
    b.bit = pos
    blk["symbols"], blk["end_bit"] = syms, b.bit
    runs, run, weight = [], 0, 1
    for s in syms:
        if s in (RUNA, RUNB):
            run += weight * (s + 1)
            weight *= 2
        elif run:
            runs.append(run)
            run, weight = 0, 1
    blk["zero_runs"] = runs
    return blk


def blocks(image, symbols=False):
    bits = Bits(image)
    return [parse_block(image, bit, symbols, bits) for bit, kind in BS.find_magics(image) if kind == 0]


def rle1(data):
    out, i = bytearray(), 0
    while i < len(data):
        j = i
        while j < len(data) and data[j] == data[i] and j - i < 255:
            j += 1
        n = j - i
        out += data[i:i + min(n, 4)]
        if n >= 4:
            out.append(n - 4)
        i = j
    return bytes(out)


def model_symbols(data):
    """MTF / RLE2 symbols (end-of-block included) of ONE block made of `data`; Python sort: small inputs only."""
    r = rle1(data)
    n = len(r)
    rows = sorted(range(n), key=lambda i: r[i:] + r[:i])
    last = bytes(r[(i - 1) % n] for i in rows)
    order = sorted(set(r))
    syms, run = [], 0

    def flush(run):
        while run:
            if run & 1:
                syms.append(RUNA)
                run = (run - 1) >> 1
            else:
                syms.append(RUNB)
                run = (run - 2) >> 1
    for c in last:
        p = order.index(c)
        if p == 0:
            run += 1
            continue
        flush(run)
        run = 0
        order.insert(0, order.pop(p))
        syms.append(p + 1)
    flush(run)
    syms.append(len(order) + 1)
    return syms


def table_counts(blk):
    """per table, the count of every symbol in the groups that select it (what the table was fitted to)"""
    alpha = len(blk["used"]) + 2
    counts = [[0] * alpha for _ in range(blk["n_tables"])]
    for i, s in enumerate(blk["symbols"]):
        counts[blk["selectors"][i // 50]][s] += 1
    return counts


def huffman_depth(counts):
    """depth of an UNLIMITED Huffman code for these counts, every symbol present (a count of 0 counts as 1, as in the
    format every symbol of the alphabet gets a length)"""
    import heapq
    heap = [(max(c, 1), 0) for c in counts]
    heapq.heapify(heap)
    while len(heap) > 1:
        a, b = heapq.heappop(heap), heapq.heappop(heap)
        heapq.heappush(heap, (a[0] + b[0], max(a[1], b[1]) + 1))
    return heap[0][1]
