"""A plain READER of Zstandard images that accepts every entropy form of a compressed block (test infrastructure), from
RFC 8878.

zstd_parse.py reads exactly what the flag-less device compressor writes and refuses the rest.  This reader goes on
where that one stops: Huffman weights in the FSE form (4.2.1.1), every Symbol_Compression_Modes byte -- Predefined,
RLE, FSE_Compressed and, because libzstd's many-block frames use them, Repeat and treeless literals, which take the
frame's previous table -- and sequences that name a repeat offset (3.1.1.5).  It is what the tests of
LA_ZSTDC_FULL_ALPHABET / LA_ZSTDC_FIT_TABLES read their census from, and test_zstd_parse_modes.py checks it against
libzstd's own output first.

parse(image) returns [frame record] like zstd_parse.parse (single, fcs_bytes, fcs, checksum, blocks, plain).  A block
record holds type, size, last and, for a compressed block:
    lit         type (0 raw, 1 RLE, 2 Huffman, 3 treeless), hdr, regen, comp, streams, stream_sizes, data and, for type 2,
                tree ("direct" or "fse"), tree_bytes (header byte included), weights (as sent: the last symbol's is
                implied), weight_norm / weight_al (the FSE form's normalised counts and accuracy log), lengths, max_bits
    nseq, nseq_form
    modes       {"ll" | "of" | "ml": 0 predefined, 1 RLE, 2 FSE_Compressed, 3 repeat}   (nseq > 0)
    als         the three accuracy logs (0 for an RLE table)
    norms       the normalised counts as described (None for RLE; the default distribution for predefined)
    seqs        [(literal length, match length, offset value, LL code, ML code, OF code)]
    regen       the bytes the block regenerates
"""
import zstd_build as B
from zstd_parse import ParseError, _Back, _huf_decode, _huf_table, _need, full_weights

MODE_NAMES = {0: "predefined", 1: "rle", 2: "fse", 3: "repeat"}


def read_ncount(buf, max_al, max_sym):
    """(normalised counts, accuracy log, bytes used) of an FSE table description (RFC 8878 4.1.1)"""
    _need(len(buf) > 0, "empty table description")
    bits = int.from_bytes(bytes(buf[:80]), "little")

    def get(p, n):
        return (bits >> p) & ((1 << n) - 1)

    al, bp = get(0, 4) + 5, 4
    _need(al <= max_al, "accuracy log %d above %d" % (al, max_al))
    remaining, threshold, nbits = (1 << al) + 1, 1 << al, al + 1
    norm = []
    while remaining > 1 and len(norm) <= max_sym:
        mx = 2 * threshold - 1 - remaining
        v = get(bp, nbits)
        if v & (threshold - 1) < mx:
            count = v & (threshold - 1)
            bp += nbits - 1
        else:
            count = v & (2 * threshold - 1)
            if count >= threshold:
                count -= mx
            bp += nbits
        count -= 1
        remaining -= abs(count)
        norm.append(count)
        if count == 0:
            while True:
                r = get(bp, 2)
                bp += 2
                norm += [0] * r
                if r != 3:
                    break
        _need(remaining >= 1, "counts exceed the table")
        while remaining < threshold:
            nbits -= 1
            threshold >>= 1
    _need(remaining == 1 and len(norm) <= max_sym + 1, "counts do not fill the table")
    used = (bp + 7) >> 3
    _need(used <= len(buf), "table description past its section")
    return norm, al, used


def _fse_weights(sec):
    """weights of an FSE-form tree description (the bytes behind its header byte): two interleaved states, the stream
    ends when a state update runs out of bits"""
    norm, al, c = read_ncount(sec, 6, 11)
    tab = B.fse_dtable(norm, al)
    r = _Back(sec[c:])
    s1, s2 = r.read(al), r.read(al)
    _need(r.pos >= 0, "weight stream shorter than its two states")
    w = []
    while True:
        _need(len(w) <= 253, "more than 255 weights")
        w.append(tab[s1][0])
        s1 = tab[s1][2] + r.read(tab[s1][1])
        if r.pos < 0:
            w.append(tab[s2][0])
            break
        _need(len(w) <= 253, "more than 255 weights")
        w.append(tab[s2][0])
        s2 = tab[s2][2] + r.read(tab[s2][1])
        if r.pos < 0:
            w.append(tab[s1][0])
            break
    return w, norm, al


def _literals(body, st):
    b0 = body[0]
    t, sf = b0 & 3, (b0 >> 2) & 3
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
        return {"type": t, "hdr": hl, "regen": regen, "comp": size, "streams": 0, "stream_sizes": [], "tree": None,
                "tree_bytes": 0, "weights": None, "weight_norm": None, "weight_al": None, "lengths": None,
                "max_bits": None, "data": data}, hl + size
    hl, bits = {0: (3, 10), 1: (3, 10), 2: (4, 14), 3: (5, 18)}[sf]
    v = int.from_bytes(body[:hl], "little")
    regen, comp = (v >> 4) & ((1 << bits) - 1), v >> (4 + bits)
    streams = 1 if sf == 0 else 4
    _need(hl + comp <= len(body), "compressed literals past the block")
    sec = body[hl:hl + comp]
    lit = {"type": t, "hdr": hl, "regen": regen, "comp": comp, "streams": streams, "tree": None, "tree_bytes": 0,
           "weights": None, "weight_norm": None, "weight_al": None}
    tree = 0
    if t == 2:
        _need(len(sec) > 0, "no tree description")
        hb = sec[0]
        if hb >= 128:
            nw = hb - 127
            tree = 1 + (nw + 1) // 2
            _need(tree <= len(sec), "direct weights past the section")
            sent = [sec[1 + k // 2] >> 4 if k % 2 == 0 else sec[1 + k // 2] & 15 for k in range(nw)]
            lit["tree"] = "direct"
        else:
            _need(hb > 0 and 1 + hb <= len(sec), "FSE-coded weights past the section")
            tree = 1 + hb
            sent, lit["weight_norm"], lit["weight_al"] = _fse_weights(sec[1:1 + hb])
            lit["tree"] = "fse"
        _need(all(w <= 11 for w in sent), "weight above 11")
        weights, mb = full_weights(sent)
        _need(mb <= 11, "code length above 11")
        lit["weights"], lit["tree_bytes"] = sent, tree
        st["huf"] = (weights, mb)
    else:
        _need("huf" in st, "treeless literals without an earlier tree")
        weights, mb = st["huf"]
    lit["lengths"] = {s: mb + 1 - w for s, w in enumerate(weights) if w}
    lit["max_bits"] = mb
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
    lit["stream_sizes"] = [len(x) for x in parts]
    tab = _huf_table(weights, mb)
    lit["data"] = b"".join(_huf_decode(tab, mb, x, c)[0] for x, c in zip(parts, counts))
    return lit, hl + comp


def _tables(body, p, st):
    """the Symbol_Compression_Modes byte at body[p] and the descriptions behind it"""
    mb = body[p]
    p += 1
    _need(mb & 3 == 0, "reserved bits of the modes byte set (%#x)" % mb)
    modes, als, norms, tabs = {}, {}, {}, {}
    for kind, shift in (("ll", 6), ("of", 4), ("ml", 2)):
        m = (mb >> shift) & 3
        if m == 0:
            norm, al = B.DEFAULTS[kind]
            tab = B.fse_dtable(norm, al)
        elif m == 1:
            _need(p < len(body), "no RLE symbol")
            _need(body[p] <= B.MAX_SYM[kind], "RLE symbol %d" % body[p])
            norm, al, tab = None, 0, [(body[p], 0, 0)]
            p += 1
        elif m == 2:
            norm, al, c = read_ncount(body[p:], B.MAX_AL[kind], B.MAX_SYM[kind])
            p += c
            tab = B.fse_dtable(norm, al)
        else:
            _need(kind in st, "Repeat_Mode without an earlier table")
            norm, al, tab = st[kind]
        st[kind] = (norm, al, tab)
        modes[kind], als[kind], norms[kind], tabs[kind] = m, al, norm, tab
    return modes, als, norms, tabs, p


def _sequences(buf, nseq, tabs, als):
    r = _Back(buf)
    sl, so, sm = r.read(als["ll"]), r.read(als["of"]), r.read(als["ml"])
    LL, OF, ML = tabs["ll"], tabs["of"], tabs["ml"]
    seqs = []
    for i in range(nseq):
        lc, oc, mc = LL[sl][0], OF[so][0], ML[sm][0]
        _need(lc <= 35 and mc <= 52 and oc <= 31, "code out of range")
        ofv = (1 << oc) + r.read(oc)
        ml = B.ML_BASE[mc] + r.read(B.ML_BITS[mc])
        ll = B.LL_BASE[lc] + r.read(B.LL_BITS[lc])
        seqs.append((ll, ml, ofv, lc, mc, oc))
        if i + 1 < nseq:
            sl = LL[sl][2] + r.read(LL[sl][1])
            sm = ML[sm][2] + r.read(ML[sm][1])
            so = OF[so][2] + r.read(OF[so][1])
        _need(r.pos >= 0, "sequence bits run out at sequence %d" % i)
    _need(r.pos == 0, "%d sequence bits left over" % r.pos)
    return seqs


def _compressed(body, out, st):
    _need(len(body) >= 3, "a compressed block of fewer than 3 bytes")
    lit, p = _literals(body, st)
    _need(p < len(body), "no sequences section")
    b0 = body[p]
    if b0 < 128:
        nseq, form = b0, 1
    elif b0 < 255:
        nseq, form = ((b0 - 128) << 8) + body[p + 1], 2
    else:
        nseq, form = int.from_bytes(body[p + 1:p + 3], "little") + 0x7F00, 3
    p += form
    rec = {"lit": lit, "nseq": nseq, "nseq_form": form, "seqs": [], "modes": None, "als": None, "norms": None}
    if nseq == 0:
        _need(p == len(body), "bytes behind a sequences section of no sequences")
    else:
        rec["modes"], rec["als"], rec["norms"], tabs, p = _tables(body, p, st)
        rec["seqs"] = _sequences(body[p:], nseq, tabs, rec["als"])
    data, lp, rep = lit["data"], 0, st["rep"]
    for ll, ml, ofv, _, _, _ in rec["seqs"]:
        off, rep = B._rep_offset(rep, ll, ofv)
        _need(lp + ll <= len(data), "literal length past the literals")
        out += data[lp:lp + ll]
        lp += ll
        _need(0 < off <= len(out), "offset %d reaches before the frame (at %d)" % (off, len(out)))
        if off >= ml:
            out += out[len(out) - off:len(out) - off + ml]
        else:
            out += (bytes(out[len(out) - off:]) * (ml // off + 1))[:ml]
    st["rep"] = rep
    out += data[lp:]
    return rec


def parse(img):
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
        out, blocks, st = bytearray(), [], {"rep": [1, 4, 8]}
        while True:
            _need(p + 3 <= len(img), "truncated block header")
            bh = int.from_bytes(img[p:p + 3], "little")
            p += 3
            last, bt, bs = bh & 1, (bh >> 1) & 3, bh >> 3
            _need(bt != 3, "reserved block type")
            rec = {"type": bt, "size": bs, "last": last}
            before = len(out)
            if bt == 0:
                _need(p + bs <= len(img), "truncated raw block")
                out += img[p:p + bs]
                p += bs
            elif bt == 1:
                out += img[p:p + 1] * bs
                p += 1
            else:
                _need(p + bs <= len(img), "truncated compressed block")
                rec.update(_compressed(img[p:p + bs], out, st))
                p += bs
            rec["regen"] = len(out) - before
            blocks.append(rec)
            if last:
                break
        p += 4 if csum else 0
        _need(p <= len(img), "truncated checksum")
        plain = bytes(out)
        if fcs is not None:
            _need(fcs == len(plain), "frame content size %d but %d bytes regenerated" % (fcs, len(plain)))
        frames.append({"single": single, "fcs_bytes": fl, "fcs": fcs, "checksum": csum, "blocks": blocks, "plain": plain})
    return frames


def plain_of(frames):
    return b"".join(f["plain"] for f in frames)


def compressed_blocks(frames):
    return [b for f in frames for b in f["blocks"] if b["type"] == 2]
