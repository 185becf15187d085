"""A plain READER of the Zstandard images the device compressor writes (test infrastructure), from RFC 8878.

The counterpart of zstd_build.py, whose tables, fse_dtable and huf_codes it reuses.  parse(image) returns one record
per frame and, inside it, one per block: everything a census of the compressor's format decisions needs -- header
forms, stream sizes, the bit position of every Huffman stream's end mark, the weights as written, every sequence with
its three codes -- plus the bytes the frame regenerates, so that a test can compare this reader's own reconstruction
with the input.  It supports what la_zstd_comp.hip can write and raises ParseError on anything else: Huffman weights
are direct (no FSE-coded weights, no treeless literals), the three sequence tables are the predefined ones, no
sequence uses a repeat offset, no dictionary.

Frame record:  single, fcs_bytes, fcs (None without the field), checksum, blocks, plain (deep only).
Block record:  type (0 raw, 1 RLE, 2 compressed), size (the header's Block_Size), last; for type 2 also
    lit         type (0 raw, 1 RLE, 2 Huffman), hdr (header bytes), regen, comp, streams, stream_sizes, end_marks
                (bit position of each stream's end mark = payload bits of that stream), weights (as written: the last
                symbol's is implied), lengths ({symbol: code length}), max_bits, data (the literals)
    nseq, nseq_form (1, 2 or 3 header bytes)
    seqs        [(literal length, match length, offset value, LL code, ML code, OF code)]  (deep only)
deep=False stops after the literals section's and the sequence count's headers (no Huffman decoding, no sequences, no
execution): enough to pick the blocks worth the full walk.
"""
import zstd_build as B

LL_TAB = B.fse_dtable(B.LL_DEF, 6)
ML_TAB = B.fse_dtable(B.ML_DEF, 6)
OF_TAB = B.fse_dtable(B.OF_DEF, 5)


class ParseError(Exception):
    pass


def _need(cond, what):
    if not cond:
        raise ParseError(what)


class _Back:
    """a backward bit stream: the decoder starts below the end mark and reads downwards; bits below bit 0 read as 0"""

    def __init__(self, buf):
        _need(len(buf) > 0 and buf[-1] != 0, "a backward stream ends in a byte with the end mark")
        self.buf = bytes(buf)
        self.mark = (len(buf) - 1) * 8 + B.highbit(buf[-1])
        self.pos = self.mark

    def peek(self, n):
        lo = self.pos - n
        if lo >= 0:
            v = int.from_bytes(self.buf[lo >> 3:(lo >> 3) + 5], "little") >> (lo & 7)
        else:
            v = int.from_bytes(self.buf[:5], "little") << -lo
        return v & ((1 << n) - 1)

    def read(self, n):
        v = self.peek(n) if n else 0
        self.pos -= n
        return v


def full_weights(sent):
    """the weights with the implied last one (RFC 8878 4.2.1.1)"""
    total = sum(1 << (w - 1) for w in sent if w)
    _need(total > 0, "all weights zero")
    mb = B.highbit(total) + 1
    rest = (1 << mb) - total
    _need(rest & (rest - 1) == 0, "the weights leave no power of two for the last symbol")
    return list(sent) + [B.highbit(rest) + 1], mb


def _huf_table(weights, mb):
    tab = [None] * (1 << mb)
    for s, (code, nb) in B.huf_codes(weights).items():
        for k in range(1 << (mb - nb)):
            tab[(code << (mb - nb)) + k] = (s, nb)
    _need(None not in tab, "incomplete Huffman code")
    return tab


def _huf_decode(tab, mb, buf, count):
    r = _Back(buf)
    out = bytearray()
    for _ in range(count):
        s, nb = tab[r.peek(mb)]
        r.pos -= nb
        out.append(s)
    _need(r.pos == 0, "Huffman stream of %d symbols ends at bit %d, not 0" % (count, r.pos))
    return bytes(out), r.mark


def _literals(body, deep):
    b0 = body[0]
    t, sf = b0 & 3, (b0 >> 2) & 3
    _need(t != 3, "treeless literals")
    if t < 2:
        if sf in (0, 2):
            hl, regen = 1, b0 >> 3
        elif sf == 1:
            hl, regen = 2, int.from_bytes(body[:2], "little") >> 4
        else:
            hl, regen = 3, int.from_bytes(body[:3], "little") >> 4
        size = regen if t == 0 else 1
        _need(hl + size <= len(body), "literals past the block")
        data = bytes(body[hl:hl + regen]) if t == 0 else bytes(body[hl:hl + 1]) * regen
        return {"type": t, "hdr": hl, "regen": regen, "comp": size, "streams": 0, "stream_sizes": [], "end_marks": [],
                "weights": None, "lengths": None, "max_bits": None, "data": data}, hl + size
    hl, bits = {0: (3, 10), 1: (3, 10), 2: (4, 14), 3: (5, 18)}[sf]
    v = int.from_bytes(body[:hl], "little")
    regen, comp = (v >> 4) & ((1 << bits) - 1), v >> (4 + bits)
    streams = 1 if sf == 0 else 4
    _need(hl + comp <= len(body), "compressed literals past the block")
    sec = body[hl:hl + comp]
    hb = sec[0]
    _need(hb >= 128, "FSE-coded Huffman weights")
    nw = hb - 127
    tree = 1 + (nw + 1) // 2
    sent = []
    for k in range(nw):
        byte = sec[1 + k // 2]
        sent.append(byte >> 4 if k % 2 == 0 else byte & 15)
    if nw & 1:
        _need(sec[1 + nw // 2] & 15 == 0, "the unused low nibble behind an odd weight count is not zero")
    weights, mb = full_weights(sent)
    _need(mb <= 11, "code length above 11")
    lengths = {s: mb + 1 - w for s, w in enumerate(weights) if w}
    pay = sec[tree:]
    if streams == 1:
        parts, counts = [pay], [regen]
    else:
        _need(len(pay) >= 6, "no jump table")
        j = [int.from_bytes(pay[2 * k:2 * k + 2], "little") for k in range(3)]
        _need(6 + sum(j) < len(pay), "jump table past the section")
        q = (regen + 3) // 4
        _need(regen >= 3 * q, "four streams for %d literals" % regen)
        parts, p = [], 6
        for k in range(3):
            parts.append(pay[p:p + j[k]])
            p += j[k]
        parts.append(pay[p:])
        counts = [q, q, q, regen - 3 * q]
    lit = {"type": 2, "hdr": hl, "regen": regen, "comp": comp, "streams": streams, "stream_sizes": [len(x) for x in parts],
           "weights": sent, "lengths": lengths, "max_bits": mb, "data": None, "end_marks": None}
    for x in parts:
        _need(len(x) > 0 and x[-1] != 0, "a Huffman stream without its end mark")
    lit["end_marks"] = [(len(x) - 1) * 8 + B.highbit(x[-1]) for x in parts]
    if deep:
        tab = _huf_table(weights, mb)
        lit["data"] = b"".join(_huf_decode(tab, mb, x, c)[0] for x, c in zip(parts, counts))
    return lit, hl + comp


def _sequences(buf, nseq):
    r = _Back(buf)
    sl, so, sm = r.read(6), r.read(5), r.read(6)
    seqs = []
    for i in range(nseq):
        lc, _, _ = LL_TAB[sl]
        oc, _, _ = OF_TAB[so]
        mc, _, _ = ML_TAB[sm]
        ofv = (1 << oc) + r.read(oc)
        ml = B.ML_BASE[mc] + r.read(B.ML_BITS[mc])
        ll = B.LL_BASE[lc] + r.read(B.LL_BITS[lc])
        seqs.append((ll, ml, ofv, lc, mc, oc))
        if i + 1 < nseq:
            _, nb, base = LL_TAB[sl]
            sl = base + r.read(nb)
            _, nb, base = ML_TAB[sm]
            sm = base + r.read(nb)
            _, nb, base = OF_TAB[so]
            so = base + r.read(nb)
        _need(r.pos >= 0, "sequence bits run out at sequence %d" % i)
    _need(r.pos == 0, "%d sequence bits left over" % r.pos)
    return seqs


def _compressed(body, out, start, deep):
    _need(len(body) >= 3, "a compressed block of fewer than 3 bytes")
    lit, p = _literals(body, deep)
    _need(p < len(body), "no sequences section")
    b0 = body[p]
    if b0 < 128:
        nseq, form = b0, 1
    elif b0 < 255:
        nseq, form = ((b0 - 128) << 8) + body[p + 1], 2
    else:
        nseq, form = int.from_bytes(body[p + 1:p + 3], "little") + 0x7F00, 3
    p += form
    rec = {"lit": lit, "nseq": nseq, "nseq_form": form, "seqs": None}
    if nseq == 0:
        _need(p == len(body), "bytes behind a sequences section of no sequences")
    else:
        _need(body[p] == 0, "sequence tables not all predefined (modes byte %#x)" % body[p])
        p += 1
    if not deep:
        return rec
    rec["seqs"] = seqs = _sequences(body[p:], nseq) if nseq else []
    data, lp = lit["data"], 0
    for ll, ml, ofv, _, _, _ in seqs:
        _need(ofv > 3, "repeat offset (offset value %d)" % ofv)
        off = ofv - 3
        _need(lp + ll <= len(data), "literal length past the literals")
        out += data[lp:lp + ll]
        lp += ll
        _need(0 < off <= len(out) - start, "offset %d reaches before the frame (at %d)" % (off, len(out) - start))
        if off >= ml:
            out += out[len(out) - off:len(out) - off + ml]
        else:
            out += (bytes(out[len(out) - off:]) * (ml // off + 1))[:ml]
    out += data[lp:]
    return rec


def parse(img, deep=True):
    """[frame record] of every frame of img"""
    img = bytes(img)
    frames, p = [], 0
    while p < len(img):
        _need(int.from_bytes(img[p:p + 4], "little") == B.MAGIC, "no zstd magic at %d" % p)
        fhd = img[p + 4]
        _need(fhd & 0x0B == 0, "dictionary id or reserved bit in the frame header")
        single, csum, flag = (fhd >> 5) & 1, (fhd >> 2) & 1, fhd >> 6
        p += 5 + (0 if single else 1)
        fl = [1 if single else 0, 2, 4, 8][flag]
        fcs = int.from_bytes(img[p:p + fl], "little") + (256 if fl == 2 else 0) if fl else None
        p += fl
        out, blocks = bytearray(), []
        while True:
            _need(p + 3 <= len(img), "truncated block header")
            bh = int.from_bytes(img[p:p + 3], "little")
            p += 3
            last, bt, bs = bh & 1, (bh >> 1) & 3, bh >> 3
            _need(bt != 3, "reserved block type")
            rec = {"type": bt, "size": bs, "last": last}
            if bt == 0:
                _need(p + bs <= len(img), "truncated raw block")
                out += img[p:p + bs]
                p += bs
            elif bt == 1:
                out += img[p:p + 1] * bs
                p += 1
            else:
                _need(p + bs <= len(img), "truncated compressed block")
                before = len(out)
                rec.update(_compressed(img[p:p + bs], out, 0, deep))
                rec["regen"] = len(out) - before
                p += bs
            blocks.append(rec)
            if last:
                break
        p += 4 if csum else 0
        _need(p <= len(img), "truncated checksum")
        plain = bytes(out) if deep else None
        if deep and fcs is not None:
            _need(fcs == len(plain), "frame content size %d but %d bytes regenerated" % (fcs, len(plain)))
        frames.append({"single": single, "fcs_bytes": fl, "fcs": fcs, "checksum": csum, "blocks": blocks, "plain": plain})
    return frames


def plain_of(frames):
    return b"".join(f["plain"] for f in frames)
