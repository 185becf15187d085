"""Designed inputs for the device compressors' format edges (test infrastructure; see test_gpu_zstd_compress_edges.py
and test_gpu_lz4_compress_edges.py).

The builders here know how the block matcher looks for matches (lz77_match, la_comp_common.h): it walks the block in
windows of 64 positions, a position's candidate is what the 4096-slot table held for its four bytes' hash BEFORE the
window's own positions were written, an empty slot reads as position 0, and after a match that ends beyond the window
the next window starts at the match's end, so the positions the match covered behind the window are never inserted.
They use that only to AIM: what a test asserts is read from the image the device wrote, never from these builders.
"""


def slot(q):
    """the matcher's table slot of four bytes"""
    return ((int.from_bytes(bytes(q), "little") * 2654435761) & 0xFFFFFFFF) >> 20


# ---------------------------------------------------------------- the densest block of four-byte matches
def _unit_values():
    vals, used = [], set()
    for a in range(1, 256):
        s = {slot([a, 0, 0, 0]), slot([0, 0, 0, a]), slot([0, 0, a, 0]), slot([0, a, 0, 0])}
        if len(s) == 4 and not (s & used):
            vals.append(a)
            used |= s
            if len(vals) == 32:
                return vals
    raise AssertionError("no 32 unit values with 128 different slots")


def unit_stream(n):
    """n bytes of four-byte units [a, 0, 0, 0] over 32 values of a whose aligned and unaligned quads fall into 128
    different table slots; after its k-th occurrence unit u is followed by unit (u + 1 + k mod 31) mod 32, so no unit
    is followed by the same unit twice within reach and every match is exactly four bytes long"""
    vals = _unit_values()
    seen = [0] * 32
    out, u = bytearray(), 0
    while len(out) < n:
        out += bytes([vals[u], 0, 0, 0])
        k = seen[u]
        seen[u] += 1
        u = (u + 1 + k % 31) % 32
    return bytes(out[:n])


# ---------------------------------------------------------------- text without a repeated four-byte string
class Fresh:
    """bytes whose every four-byte string is new to everything emitted through (or shown to) this object"""

    def __init__(self, rnd, symbols=None, weights=None):
        self.rnd, self.grams = rnd, set()
        self.symbols = list(range(256)) if symbols is None else list(symbols)
        self.weights = weights

    def show(self, data):
        for i in range(len(data) - 3):
            self.grams.add(bytes(data[i:i + 4]))

    def extend(self, out, k, not_first=None, distinct_from=()):
        """append k fresh bytes to out (a bytearray whose four-byte strings are all known to this object)"""
        for i in range(k):
            tail = bytes(out[-3:])
            for _ in range(10000):
                b = self.rnd.choices(self.symbols, self.weights)[0] if self.weights else self.rnd.choice(self.symbols)
                if i == 0 and b == not_first:
                    continue
                if b in distinct_from:
                    continue
                if len(tail) < 3 or tail + bytes([b]) not in self.grams:
                    break
            else:
                raise AssertionError("alphabet exhausted: no fresh four-byte string left")
            out.append(b)
            if len(out) >= 4:
                self.grams.add(bytes(out[-4:]))


def no_repeat(rnd, n, symbols, weights=None):
    out = bytearray()
    Fresh(rnd, symbols, weights).extend(out, n)
    return bytes(out)


def exact_counts(rnd, counts):
    """a text with exactly counts[s] bytes s and no repeated four-byte string"""
    left = dict(counts)
    out, grams = bytearray(), set()
    for _ in range(sum(counts.values())):
        tail = bytes(out[-3:])
        syms = [s for s, c in left.items() if c and (len(tail) < 3 or tail + bytes([s]) not in grams)]
        assert syms, "stuck: every remaining symbol would repeat a four-byte string"
        b = rnd.choices(syms, [left[s] for s in syms])[0]
        left[b] -= 1
        out.append(b)
        if len(out) >= 4:
            grams.add(bytes(out[-4:]))
    return bytes(out)


def lit_block(lits, size):
    """a block whose literals are `lits` (no repeated four-byte string) and whose rest is one match: the text goes on
    periodically with its own last t bytes -- all of it while it is shorter than 100 bytes (the source is then
    position 0), else the last 100 or a few more.  None if another four-byte string between source and copy falls
    into the source's table slot, or one that straddles the copy's start occurred before, so that the matcher would
    not find the copy exactly where it starts."""
    n = len(lits)
    t = n if n < 100 else 100
    while t < n and lits[n - 1] == lits[n - t - 1]:
        t += 1
    data = (lits + lits[n - t:] * ((size - n) // t + 1))[:size]
    s0 = slot(data[n - t:n - t + 4])
    if len(data) < n + 4 or any(slot(data[q:q + 4]) == s0 for q in range(n - t + 1, n)):
        return None
    grams = {data[q:q + 4] for q in range(n - 3)}
    if any(data[q:q + 4] in grams for q in range(max(n - 3, 0), n)):        # a match would start before the copy does
        return None
    return data


def lit_case(rnd, n, size, symbols, weights=None):
    """lit_block of n fresh literals over `symbols`"""
    for _ in range(100):
        data = lit_block(no_repeat(rnd, n, symbols, weights), size)
        if data is not None:
            return data
    raise AssertionError("no block of %d literals" % n)


# ---------------------------------------------------------------- chosen (literal length, match length) pairs
class SeqBlock:
    """Builds a block sequence by sequence: fresh literals, then a copy whose source the matcher can see.  Tracks the
    matcher's windows so that every source lies in the last window processed before the one that holds the copy."""

    def __init__(self, rnd, symbols=None):
        self.rnd = rnd
        self.out = bytearray()
        self.fresh = Fresh(rnd, symbols)
        self.base, self.prev_w = 0, None
        self.cont = None            # the byte that would prolong the last match
        self.asked = []

    def _advance(self, p):
        while self.base + 64 <= p:
            self.prev_w, self.base = self.base, self.base + 64

    def literals(self, k):
        self.fresh.extend(self.out, k, not_first=self.cont)
        if k:
            self.cont = None

    def copy_from(self, s, ml):
        out, p = self.out, len(self.out)
        self._advance(p)
        for i in range(ml):
            out.append(out[s + i])
        self.fresh.show(out[max(0, p - 3):])
        self.cont = out[len(out) - (p - s)]
        if p + ml > self.base + 64:
            self.prev_w, self.base = self.base, p + ml
        return p - s

    def copy(self, ml):
        """a copy of ml bytes from a source in the last processed window; False if none fits"""
        out, p = self.out, len(self.out)
        self._advance(p)
        if self.prev_w is None:
            return False
        w = self.prev_w
        hi = min(w + 64, p - 3)
        slots = [slot(out[q:q + 4]) for q in range(w, hi)]
        cands = []
        for s in range(w, hi):
            if slots.count(slots[s - w]) != 1:
                continue
            if self.cont is not None and out[s] == self.cont:          # the match before must stop here
                continue
            if self.cont is None and s > 0 and out[s - 1] == out[p - 1]:   # and this one must not start a byte early
                continue
            cands.append(s)
        if not cands:
            return False
        far = [s for s in cands if p - s >= 64]     # (a copy longer than its distance is periodic: keep the period above a window)
        self.copy_from(self.rnd.choice(far or cands), ml)
        return True

    def add(self, ll, ml):
        self.literals(ll)
        if not self.copy(ml):
            self.literals(1)
            assert self.copy(ml), "no visible source"
        self.asked.append((ll, ml))

    def finish(self, size):
        """fill up to `size` with one last copy (a match may run to the block's end)"""
        assert len(self.out) + 4 <= size, (len(self.out), size)
        self.literals(1)
        assert self.copy(size - len(self.out))
        return bytes(self.out)


def pack_pairs(rnd, lls, mls, size):
    """blocks of `size` bytes that realise every literal length of lls and every match length of mls, the largest
    first, a literal length paired with a match length where both fit"""
    lls, mls = sorted(lls, reverse=True), sorted(mls, reverse=True)
    blocks = []
    while lls or mls:
        sb = SeqBlock(rnd)
        sb.literals(64)
        sb.add(3, 70)
        progress = False
        while True:
            room = size - len(sb.out) - 80
            ll = next((x for x in lls if x + 4 <= room), None)
            ml = next((x for x in mls if (ll if ll is not None else 2) + x <= room), None)
            if ll is None and ml is None:
                break
            if ll is not None:
                lls.remove(ll)
            if ml is not None:
                mls.remove(ml)
            sb.add(ll if ll is not None else rnd.randint(1, 15), ml if ml is not None else rnd.randint(4, 34))
            progress = True
        assert progress, "a target does not fit a block"
        blocks.append(sb.finish(size))
    return blocks


# ---------------------------------------------------------------- chosen offsets
def offset_gadgets(rnd, offsets, size):
    """blocks of `size` bytes with one match at each of `offsets` (each at least 68): 64 fresh bytes U, a run that
    repeats U[1:] with period 63 and is therefore covered by one match that never re-inserts U's first four bytes,
    then U again -- found at offset 64 + the run's length -- for 70 bytes, which also puts the next window at the
    next gadget's first byte"""
    blocks, out, fresh = [], bytearray(), Fresh(rnd)
    cont = last = None
    for off in sorted(offsets):
        need = off + 70
        assert off >= 68 and need + 8 <= size
        if len(out) + need + 8 > size:
            blocks.append(_close_gadgets(out, last, size))
            out, fresh, cont = bytearray(), Fresh(rnd), None
        g = len(out)
        for _ in range(100):
            u = bytearray()
            trial = Fresh(rnd)
            trial.grams = set(fresh.grams)
            tmp = bytearray(out[-3:])
            k = len(tmp)
            while len(tmp) - k < 64:
                trial.extend(tmp, 1, not_first=cont if len(tmp) == k else None, distinct_from=tmp[k:])
            u = tmp[k:]
            s0 = slot(u[:4])
            per = u[1:]
            if all(slot((per * 2)[i:i + 4]) != s0 for i in range(63)) and all(slot(u[i:i + 4]) != s0 for i in range(1, 61)):
                break
        else:
            raise AssertionError("no gadget head")
        fresh.grams = trial.grams
        out += u
        zl = off - 64
        out += (per * (zl // 63 + 2))[:zl]
        src = g
        for i in range(70):
            out.append(out[src + i])
        fresh.show(out[g:])
        cont, last = out[src + 70], off
    blocks.append(_close_gadgets(out, last, size))
    return blocks


def _close_gadgets(out, d, size):
    """prolong the last copy (at distance d) to the block's end"""
    out = bytearray(out)
    while len(out) < size:
        out.append(out[len(out) - d])
    return bytes(out)


def farthest_offset_block(rnd, size):
    """offset size - 4, the farthest a block can hold: its last four bytes repeat its first four, and everything
    between is one match of period 63 that never re-inserts them"""
    for _ in range(100):
        u = bytearray()
        Fresh(rnd).extend(u, 64, distinct_from=u)
        s0 = slot(u[:4])
        per = bytes(u[1:])
        if all(slot((per * 2)[i:i + 4]) != s0 for i in range(63)) and all(slot(u[i:i + 4]) != s0 for i in range(1, 61)):
            return bytes(u) + (per * (size // 63 + 2))[:size - 68] + bytes(u[:4])
    raise AssertionError("no head")


# ---------------------------------------------------------------- sequences that cost more than the bytes they save
def costly_block(rnd, size=131072, uses=800, ll=64):
    """A block whose compressed form outgrows it: `uses` four-byte matches at offsets of 2^16 and more (16 offset
    bits), each behind `ll` literals (literal-length code 25: 6 extra bits), cost about 36 bits where they save 32,
    and the literals -- bytes of every value, so they stay raw -- cost what they are.  The sources are four-byte
    strings near the block's start; every byte behind a source is chosen so that no four-byte string falls into that
    source's table slot before its copy is reached."""
    out, grams, reserved = bytearray(), set(), set()

    def ok(b, own=None):
        if len(out) < 3:
            return True
        g = bytes(out[-3:]) + bytes([b])
        return g == own or (g not in grams and slot(g) not in reserved)

    def put(b):
        out.append(b)
        if len(out) >= 4:
            grams.add(bytes(out[-4:]))

    def fresh(k, not_first=None):
        for i in range(k):
            while True:
                b = rnd.randrange(256)
                if ok(b) and not (i == 0 and b == not_first):
                    break
            put(b)

    def rollback(mark):
        for g in range(max(mark, 3), len(out)):
            grams.discard(bytes(out[g - 3:g + 1]))
        del out[mark:]

    def quad(q, own):
        mark = len(out)
        for j, b in enumerate(q):
            if not ok(b, own if j == 3 else None):
                rollback(mark)
                return False
            put(b)
        return True

    fresh(8)
    srcs = []
    while len(srcs) < uses:
        q = bytes(rnd.randrange(256) for _ in range(4))
        if slot(q) not in reserved and q not in grams and quad(q, None):
            reserved.add(slot(q))
            srcs.append((len(out) - 4, q))
            fresh(2)
    fresh(srcs[-1][0] + 65536 + 8 - ll - len(out))
    cont = None
    for pos, q in srcs:
        while True:
            mark = len(out)
            fresh(ll, not_first=cont)
            if out[-1] != out[pos - 1] and quad(q, q):
                break
            rollback(mark)
        reserved.discard(slot(q))
        cont = out[pos + 4]
    assert len(out) + 8 <= size
    fresh(size - len(out), not_first=cont)
    return bytes(out)
