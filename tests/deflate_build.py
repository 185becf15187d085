"""A raw-deflate WRITER in plain Python, from RFC 1951 (no zlib): streams that no compressor emits, for the two inflate
kernels and the oracle.  A stream is a list of blocks -- Stored, Fixed, Dynamic, Reserved -- whose every field can be
scripted: LEN / NLEN, the pad bits in front of a stored block, HLIT / HDIST / HCLEN, the code-length code, the PLAN (the
code-length symbols with their extra values, so repeats and single lengths are chosen, not derived), and ops that may
name symbols the format does not have.

While it writes, a small model keeps the plain bytes; for a stream built to be refused it keeps the status class
(ST_DATA / ST_TRUNCATED) and the bytes in front of the error.  The model is never its own judge:
tests/test_oracle_deflate_handbuilt.py holds every case to zlib's inflate.

handbuilt_cases(census) returns the catalogue as Case(name, image, plain, valid, status) and counts, per feature, how
often a VALID stream took it (refused classes count under "refused_*")."""
import os
import random
import re
from collections import namedtuple

ST_OK, ST_DATA, ST_TRUNCATED, ST_OUT_FULL = 0, 5, 6, 9

Case = namedtuple("Case", "name image plain valid status")

CLC_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
_LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
_LEN_XB = [0] * 8 + [1] * 4 + [2] * 4 + [3] * 4 + [4] * 4 + [5] * 4 + [0]
_DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577]
_DIST_XB = [0, 0, 0, 0] + [i // 2 for i in range(2, 28)]
# the fixed code can express these and the format forbids them: the extra bits zlib's tables give them do not matter
_LEN_XB_ANY = _LEN_XB + [0, 0]
_DIST_XB_ANY = _DIST_XB + [0, 0]


def inflate_maxseq():
    """LA_INFLATE_MAXSEQ as the device code has it"""
    here = os.path.dirname(os.path.abspath(__file__))
    text = open(os.path.join(os.path.dirname(here), "libarchive_amd", "csrc", "la_dev.h")).read()
    return int(re.search(r"#define\s+LA_INFLATE_MAXSEQ\s+(\d+)u", text).group(1))


class _Bits:
    """LSB-first bit writer (RFC 1951 3.1.1); Huffman codes go in MSB-first."""
    def __init__(self):
        self.acc, self.n, self.out = 0, 0, bytearray()

    def put(self, v, nbits):
        self.acc |= (v & ((1 << nbits) - 1)) << self.n
        self.n += nbits
        while self.n >= 8:
            self.out.append(self.acc & 255)
            self.acc >>= 8
            self.n -= 8

    def code(self, c, nbits):
        self.put(int(format(c, "0%db" % nbits)[::-1], 2), nbits)

    def pos(self):
        return len(self.out) * 8 + self.n

    def done(self):
        if self.n:
            self.out.append(self.acc & 255)
        return bytes(self.out)


def _canon(lens):
    """symbol -> (code, length), canonical assignment of RFC 1951 3.2.2"""
    bl = [0] * 16
    for l in lens:
        bl[l] += 1 if l else 0
    nxt, c = [0] * 16, 0
    for b in range(1, 16):
        c = (c + bl[b - 1]) << 1
        nxt[b] = c
    out = {}
    for sy, l in enumerate(lens):
        if l:
            out[sy] = (nxt[l], l)
            nxt[l] += 1
    return out


def _dynamic_block(ll_lens, d_lens, ops, final=True):
    """One dynamic-Huffman block with the GIVEN code lengths (286 / 30 entries).  The lengths are sent one by one
    (no repeat codes) through a flat code-length code: sixteen 4-bit words for the lengths 0..15.
    ops: ints (literal bytes) or (length symbol index, extra value, distance symbol, extra value)."""
    w = _Bits()
    w.put(1 if final else 0, 1)
    w.put(2, 2)
    nlen, ndist = 286, 30
    w.put(nlen - 257, 5)
    w.put(ndist - 1, 5)
    w.put(19 - 4, 4)
    order = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
    cl_lens = [4 if s < 16 else 0 for s in range(19)]		# sixteen 4-bit codes: a complete code
    for s in order:
        w.put(cl_lens[s], 3)
    clc = _canon(cl_lens)
    for l in list(ll_lens) + list(d_lens):
        w.code(*clc[l])
    ll, dd = _canon(ll_lens), _canon(d_lens)
    for op in ops:
        if isinstance(op, int):
            w.code(*ll[op])
        else:
            ls, lx, ds, dx = op
            w.code(*ll[257 + ls])
            w.put(lx, _LEN_XB[ls])
            w.code(*dd[ds])
            w.put(dx, _DIST_XB[ds])
    w.code(*ll[256])
    return w


FIXED_LL = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_D = [5] * 32


# ---------------------------------------------------------------- scripts

class Raw:
    """n raw bits in the symbol stream; error = the status the decoder reaches while it reads them (None: none)"""
    def __init__(self, value, nbits, error=None):
        self.value, self.nbits, self.error = value, nbits, error


class Stored:
    def __init__(self, data, pad_bits=0, len_=None, nlen=None, final=None, refuse=None):
        self.data, self.pad_bits, self.len_, self.nlen, self.final, self.refuse = bytes(data), pad_bits, len_, nlen, final, refuse


class Fixed:
    def __init__(self, ops, final=None, eob=True):
        self.ops, self.final, self.eob = list(ops), final, eob


class Reserved:
    """block type 3"""
    def __init__(self, final=None):
        self.final = final


class Dynamic:
    """ll_lens / d_lens: the code lengths (lists of hlit / hdist entries; shorter lists are padded with zeros).  With a
    `plan` and no ll_lens the lengths are what the plan expands to.  plan: [(code-length symbol, extra value)] or
    Raw items.  clc_lens: the 19 code-length-code lengths.  refuse: the status the HEADER (or the built codes) earns."""
    def __init__(self, ll_lens, d_lens, ops, hlit=None, hdist=None, hclen=None, clc_lens=None, plan=None, final=None,
                 refuse=None, eob=True, plan_style="runs", rnd=None):
        self.ll_lens, self.d_lens, self.ops = ll_lens, d_lens, list(ops)
        self.hlit, self.hdist, self.hclen, self.clc_lens, self.plan = hlit, hdist, hclen, clc_lens, plan
        self.final, self.refuse, self.eob, self.plan_style, self.rnd = final, refuse, eob, plan_style, rnd


def M(length, dist, long258=False):
    """the op of a match: (length symbol, extra, distance symbol, extra)"""
    ls = max(i for i in range(29) if _LEN_BASE[i] <= length)
    if long258 and length == 258:
        ls = 27
    ds = max(i for i in range(30) if _DIST_BASE[i] <= dist)
    return (ls, length - _LEN_BASE[ls], ds, dist - _DIST_BASE[ds])


def kraft(n, maxbits, rnd=None):
    """n code lengths with Kraft sum exactly 1 (n == 1: the lone 1-bit word); rnd: random shape, else the flattest"""
    if n == 1:
        return [1]
    leaves = [0]
    while len(leaves) < n:
        cand = [i for i, l in enumerate(leaves) if l < maxbits]
        i = rnd.choice(cand) if rnd else min(cand, key=lambda k: leaves[k])
        l = leaves.pop(i)
        leaves += [l + 1, l + 1]
    if rnd:
        rnd.shuffle(leaves)
    return leaves


def expand_plan(plan):
    out = []
    for sym, extra in plan:
        if sym < 16:
            out.append(sym)
        elif sym == 16:
            out += [out[-1]] * (3 + extra)
        elif sym == 17:
            out += [0] * (3 + extra)
        else:
            out += [0] * (11 + extra)
    return out


def make_plan(lens, style="runs", rnd=None):
    """code-length symbols for `lens`: style "single" sends every length singly, "runs" uses the longest repeat that
    fits, "random" picks among what fits"""
    plan, i, n = [], 0, len(lens)
    while i < n:
        v = lens[i]
        run = 1
        while i + run < n and lens[i + run] == v:
            run += 1
        opts = [(v, 0, 1)]
        if style != "single":
            if v == 0 and run >= 3:
                opts.append((17, min(run, 10) - 3, min(run, 10)))
            if v == 0 and run >= 11:
                opts.append((18, min(run, 138) - 11, min(run, 138)))
            back = 0
            while i - back - 1 >= 0 and lens[i - back - 1] == v:
                back += 1
            if i > 0 and lens[i - 1] == v and run >= 3:
                opts.append((16, min(run, 6) - 3, min(run, 6)))
        if style == "random":
            sym, extra, adv = rnd.choice(opts)
            if sym >= 16 and rnd.random() < 0.5:       # a shorter repeat than the longest that fits
                lo = 11 if sym == 18 else 3
                adv = rnd.randint(lo, adv)
                extra = adv - lo
        else:
            sym, extra, adv = opts[-1]
        plan.append((sym, extra))
        i += adv
    return plan


class _Model:
    def __init__(self, census):
        self.out = bytearray()
        self.error = None            # (status, length of the prefix)
        self.marks = [(0, 0)]        # (bits read, bytes out) after every whole symbol / stored byte
        self.census = census if census is not None else {}
        self.local = {}
        self.nlit = 0
        self.run = 0

    def count(self, key, n=1):
        self.local[key] = self.local.get(key, 0) + n

    def fail(self, status):
        if self.error is None:
            self.error = (status, len(self.out))


def _write_ops(w, mo, ops, ll, dd, eob, dynamic):
    for op in ops:
        if isinstance(op, Raw):
            w.put(op.value, op.nbits)
            if op.error:
                mo.fail(op.error)
            continue
        if isinstance(op, int):
            if op not in ll:
                assert mo.error, "literal without a code in a stream that is not refused"
                continue
            w.code(*ll[op])
            if dynamic:
                mo.count("ll_codelen_%d" % ll[op][1])
            if mo.error is None:
                mo.out.append(op)
                mo.nlit += 1
                mo.run += 1
                mo.marks.append((w.pos(), len(mo.out)))
            continue
        ls, lx, ds, dx = op
        if 257 + ls not in ll or ds not in dd:
            assert mo.error, "match without a code in a stream that is not refused"
            continue
        w.code(*ll[257 + ls])
        if ls >= 29:
            mo.fail(ST_DATA)
        w.put(lx, _LEN_XB_ANY[ls])
        w.code(*dd[ds])
        if ds >= 30:
            mo.fail(ST_DATA)
        w.put(dx, _DIST_XB_ANY[ds])
        if mo.error is None:
            length, dist = _LEN_BASE[ls] + lx, _DIST_BASE[ds] + dx
            if dist > len(mo.out):
                mo.fail(ST_DATA)
                continue
            if dynamic:
                mo.count("ll_codelen_%d" % ll[257 + ls][1])
                mo.count("d_codelen_%d" % dd[ds][1])
            mo.count("len_sym_%d_%s" % (257 + ls, "min" if lx == 0 else "max" if lx == (1 << _LEN_XB[ls]) - 1 else "mid"))
            if _LEN_XB[ls] == 0:
                mo.count("len_sym_%d_max" % (257 + ls))
            mo.count("dist_sym_%d_%s" % (ds, "min" if dx == 0 else "max" if dx == (1 << _DIST_XB[ds]) - 1 else "mid"))
            if _DIST_XB[ds] == 0:
                mo.count("dist_sym_%d_max" % ds)
            if ls == 27 and lx == 31:
                mo.count("len258_as_284_31")
            if dist == len(mo.out):
                mo.count("dist_eq_op")
            if dist == 32768:
                mo.count("dist_32768")
            if dist < length:
                mo.count("overlap")
            if mo.run in (63, 64, 65):
                mo.count("lits_before_match_%d" % mo.run)
            if mo.stored_end and len(mo.out) - dist < mo.stored_end:
                mo.count("match_into_stored")
            if mo.block_start and len(mo.out) - dist < mo.block_start:
                mo.count("match_across_blocks")
            mo.run = 0
            mo.nseq += 1
            for _ in range(length):
                mo.out.append(mo.out[-dist])
            mo.marks.append((w.pos(), len(mo.out)))
    if eob:
        w.code(*ll[256])
        if dynamic:
            mo.count("ll_codelen_%d" % ll[256][1])


def build(blocks, census=None):
    """Returns (image, plain or prefix, valid, status, info).  info: marks [(bits read, bytes out)], total bits, and per
    dynamic block the bit position behind each plan entry's CODE (in front of its extra bits)."""
    w, mo = _Bits(), _Model(census)
    mo.stored_end, mo.block_start, mo.nseq = 0, 0, 0
    info = {"plan_code_end": [], "block_bits": []}
    for bi, b in enumerate(blocks):
        final = b.final if b.final is not None else (1 if bi == len(blocks) - 1 else 0)
        mo.block_start = len(mo.out)
        info["block_bits"].append(w.pos())
        w.put(final, 1)
        if isinstance(b, Reserved):
            w.put(3, 2)
            mo.fail(ST_DATA)
        elif isinstance(b, Stored):
            w.put(0, 2)
            mo.count("stored_phase_%d" % (w.pos() % 8))
            w.put(b.pad_bits, (8 - w.n) % 8)
            ln = len(b.data) if b.len_ is None else b.len_
            w.put(ln, 16)
            w.put((ln ^ 0xFFFF) if b.nlen is None else b.nlen, 16)
            if b.refuse:
                mo.fail(b.refuse)
            mo.count("stored_len_%d" % ln if ln in (0, 65535) else "stored_len_other")
            if mo.error is None:
                mo.marks.append((w.pos(), len(mo.out)))
            for k, by in enumerate(b.data):
                w.put(by, 8)
                if mo.error is None:
                    mo.out.append(by)
                    mo.nlit += 1
                    if len(b.data) <= 4096 or k == len(b.data) - 1:
                        mo.marks.append((w.pos(), len(mo.out)))
            if mo.error is None:
                mo.run += len(b.data)
                mo.stored_end = len(mo.out)
                if len(b.data) < ln:
                    mo.fail(ST_TRUNCATED)
        elif isinstance(b, Fixed):
            w.put(1, 2)
            mo.count("fixed_blocks")
            _write_ops(w, mo, b.ops, _canon(FIXED_LL), _canon(FIXED_D), b.eob, False)
        else:
            w.put(2, 2)
            plan = b.plan
            ll_lens, d_lens = b.ll_lens, b.d_lens
            if ll_lens is None:
                flat = expand_plan([p for p in plan if not isinstance(p, Raw)])
                hlit = b.hlit
                ll_lens, d_lens = flat[:hlit], flat[hlit:]
            hlit = b.hlit if b.hlit is not None else max(257, max((i + 1 for i, l in enumerate(ll_lens) if l), default=0))
            hdist = b.hdist if b.hdist is not None else max(1, max((i + 1 for i, l in enumerate(d_lens) if l), default=0))
            ll_lens = (list(ll_lens) + [0] * hlit)[:max(hlit, len(ll_lens))] if b.plan is None else list(ll_lens)
            d_lens = (list(d_lens) + [0] * hdist)[:max(hdist, len(d_lens))] if b.plan is None else list(d_lens)
            if plan is None:
                plan = make_plan(ll_lens[:hlit] + d_lens[:hdist], b.plan_style, b.rnd)
            used = sorted({p[0] for p in plan if not isinstance(p, Raw)})
            clc_lens = b.clc_lens
            if clc_lens is None:
                syms = list(used)
                if len(syms) == 1:                      # (the code-length code must be complete)
                    syms.append(next(s for s in CLC_ORDER if s not in syms))
                clc_lens = [0] * 19
                for s, l in zip(syms, kraft(len(syms), 7, b.rnd)):
                    clc_lens[s] = l
            hclen = b.hclen if b.hclen is not None else max(4, max((i + 1 for i, s in enumerate(CLC_ORDER) if clc_lens[s]), default=0))
            w.put(hlit - 257, 5)
            w.put(hdist - 1, 5)
            w.put(hclen - 4, 4)
            for s in CLC_ORDER[:hclen]:
                w.put(clc_lens[s], 3)
            clc = _canon([clc_lens[s] if s in CLC_ORDER[:hclen] else 0 for s in range(19)])
            ends, idx = [], 0
            for p in plan:
                if isinstance(p, Raw):
                    w.put(p.value, p.nbits)
                    ends.append(w.pos())
                    continue
                sym, extra = p
                w.code(*clc[sym])
                ends.append(w.pos())
                if not b.refuse and mo.error is None:
                    mo.count("clc_codelen_%d" % clc[sym][1])
                    if sym >= 16:
                        rep = (11 if sym == 18 else 3) + extra
                        mo.count("rep%d" % sym)
                        if rep > 64:
                            mo.count("rep_gt64")
                        if rep > 128:
                            mo.count("rep_gt128")
                        if sym == 16 and idx < hlit < idx + rep:
                            mo.count("rep16_cross_boundary")
                        if sym != 16 and idx < hlit < idx + rep:
                            mo.count("zero_run_cross_boundary")
                        idx += rep
                    else:
                        idx += 1
                if sym >= 16:
                    w.put(extra, {16: 2, 17: 3, 18: 7}[sym])
            info["plan_code_end"].append(ends)
            if b.refuse:
                mo.fail(b.refuse)
            if mo.error is None:
                mo.count("dynamic_blocks")
                mo.count("hlit_%d" % hlit if hlit in (257, 286) else "hlit_other")
                mo.count("hdist_%d" % hdist if hdist in (1, 30) else "hdist_other")
                mo.count("hclen_%d" % hclen)
                if not any(d_lens[:hdist]):
                    mo.count("empty_distance_code")
                if sum(1 for l in d_lens[:hdist] if l) == 1:
                    mo.count("lone_distance_code")
                mo.marks.append((w.pos(), len(mo.out)))
            _write_ops(w, mo, b.ops, _canon(ll_lens[:hlit]), _canon(d_lens[:hdist]), b.eob, True)
        if mo.error is None:
            mo.marks.append((w.pos(), len(mo.out)))
    info["bits"] = w.pos()
    info["marks"] = mo.marks
    info["nlit"], info["nseq"] = mo.nlit, mo.nseq
    image = w.done()
    if mo.error is None:
        mo.count("end_bit_%d" % ((w.pos() - 1) % 8))
        mo.count("nl_and_15_is_%d" % (mo.nlit & 15) if (mo.nlit & 15) in (0, 15) else "nl_and_15_other")
        for k, v in mo.local.items():
            mo.census[k] = mo.census.get(k, 0) + v
        return image, bytes(mo.out), True, ST_OK, info
    return image, bytes(mo.out[:mo.error[1]]), False, mo.error[0], info


def case(name, blocks, census=None):
    image, plain, valid, status, _ = build(blocks, census)
    return Case(name, image, plain, valid, status)


def cut_case(name, blocks, nbytes, census=None):
    """the stream of `blocks` (valid by the model) cut to nbytes: truncated, with the whole symbols in front of the cut"""
    image, plain, valid, status, info = build(blocks)
    assert valid and 0 <= nbytes < len(image), name
    # (the last byte of a valid stream may hold only pad bits: a cut that keeps every used bit is no truncation)
    assert nbytes * 8 < info["bits"], name
    n = max(o for bits, o in info["marks"] if bits <= nbytes * 8)
    if census is not None:
        census["refused_truncated"] = census.get("refused_truncated", 0) + 1
    return Case(name, image[:nbytes], plain[:n], False, ST_TRUNCATED)


# ---------------------------------------------------------------- the catalogue

def _lits(n, seed=0, lo=0, hi=255):
    r = random.Random(seed)
    return [r.randint(lo, hi) for _ in range(n)]


def _every_length_codes(rnd):
    """literal/length and distance codes with a word at EVERY length 1..15 (lengths 1..14, 15, 15: Kraft sum 1)"""
    pool_lit = rnd.sample(range(256), 9)
    pool_len = rnd.sample(range(29), 6)
    syms = pool_lit + [256] + [257 + i for i in pool_len]
    rnd.shuffle(syms)
    ll_lens = [0] * 286
    for sy, l in zip(syms, list(range(1, 15)) + [15, 15]):
        ll_lens[sy] = l
    dsyms = rnd.sample(range(30), 16)
    d_lens = [0] * 30
    for sy, l in zip(dsyms, list(range(1, 15)) + [15, 15]):
        d_lens[sy] = l
    return ll_lens, d_lens, pool_lit, pool_len, dsyms


def _random_ops(rnd, have, budget, lits, len_syms=None, dist_syms=None):
    """random literals and matches that fit: `have` bytes are out already, at most `budget` more"""
    ops, n = [], 0
    for _ in range(rnd.randint(0, 120)):
        if have + n and rnd.random() < 0.45:
            ls = rnd.choice(len_syms) if len_syms else rnd.randrange(29)
            lx = rnd.getrandbits(_LEN_XB[ls]) if _LEN_XB[ls] else 0
            cands = [d for d in (dist_syms if dist_syms else range(30)) if _DIST_BASE[d] <= have + n]
            if not cands or n + _LEN_BASE[ls] + lx > budget:
                continue
            ds = rnd.choice(cands)
            dx = rnd.getrandbits(_DIST_XB[ds]) if _DIST_XB[ds] else 0
            if _DIST_BASE[ds] + dx > have + n:
                dx = 0
            ops.append((ls, lx, ds, dx))
            n += _LEN_BASE[ls] + lx
        elif n < budget:
            ops.append(rnd.choice(lits))
            n += 1
    return ops, n


def random_script(seed):
    """a random block mix with random code shapes (Kraft sum 1) and a random header plan: valid by construction"""
    rnd = random.Random(seed)
    blocks, have = [], 0
    for _ in range(rnd.randint(1, 4)):
        kind = rnd.randrange(5)
        budget = min(4000 - have, rnd.choice([8, 60, 400, 1500]))
        if kind == 0:
            data = bytes(rnd.getrandbits(8) for _ in range(rnd.randint(0, min(budget, 300))))
            blocks.append(Stored(data, pad_bits=rnd.getrandbits(7)))
            have += len(data)
        elif kind == 1:
            ops, n = _random_ops(rnd, have, budget, list(range(256)))
            blocks.append(Fixed(ops))
            have += n
        else:
            lits = rnd.sample(range(256), rnd.randint(1, 40))
            len_syms = rnd.sample(range(29), rnd.randint(1, 10))
            dist_syms = rnd.sample(range(30), rnd.randint(1, 12))
            ops, n = _random_ops(rnd, have, budget, lits, len_syms, dist_syms)
            have += n
            ll_used = sorted(set(lits) | {256} | {257 + l for l in len_syms})
            ll_lens = [0] * 286
            for s, l in zip(ll_used, kraft(len(ll_used), 15, rnd)):
                ll_lens[s] = l
            d_lens = [0] * 30
            if any(not isinstance(o, int) for o in ops) or rnd.random() < 0.7:
                for s, l in zip(sorted(dist_syms), kraft(len(dist_syms), 15, rnd)):
                    d_lens[s] = l
            blocks.append(Dynamic(ll_lens, d_lens, ops, plan_style=rnd.choice(["single", "runs", "random", "random"]), rnd=rnd,
                                  hlit=rnd.choice([None, 286]), hdist=rnd.choice([None, 30])))
    return blocks


def overlap_streams():
    """distance 1..130 x lengths {3..20, 63, 64, 65, 127, 128, 129, 257, 258}, thirteen distances per stream"""
    lengths = list(range(3, 21)) + [63, 64, 65, 127, 128, 129, 257, 258]
    out = []
    for lo in range(1, 131, 13):
        ops = _lits(130, seed=lo)
        for d in range(lo, lo + 13):
            for n in lengths:
                ops.append(M(n, d))
            ops.append(d & 255)
        out.append(("overlap-matrix-d%03d-%03d" % (lo, lo + 12), [Fixed(ops) if lo % 2 else _dyn_auto(ops, random.Random(lo))]))
    return out


def _dyn_auto(ops, rnd=None, **kw):
    """a dynamic block whose codes cover exactly the symbols of `ops` (and the end-of-block code)"""
    ll_used = sorted({o for o in ops if isinstance(o, int)} | {256} | {257 + o[0] for o in ops if not isinstance(o, (int, Raw))})
    d_used = sorted({o[2] for o in ops if not isinstance(o, (int, Raw))})
    ll_lens = [0] * 286
    for s, l in zip(ll_used, kraft(len(ll_used), 15, rnd)):
        ll_lens[s] = l
    d_lens = [0] * 30
    for s, l in zip(d_used, kraft(len(d_used), 15, rnd)):
        d_lens[s] = l
    return Dynamic(ll_lens, d_lens, ops, rnd=rnd, **kw)


def prefix_streams():
    """the streams that tests cut at EVERY byte: about 400 bytes each, one of each block type and the header-heavy ones"""
    rnd = random.Random(4242)
    text = b"every prefix of this stream is a member of its own; " * 6
    ll_lens, d_lens, pool_lit, pool_len, dsyms = _every_length_codes(rnd)
    ops15, _ = _random_ops(random.Random(7), 0, 3000, pool_lit, pool_len, dsyms)
    mixed_ops, _ = _random_ops(random.Random(8), 40, 3000, list(range(97, 123)))
    return [
        ("prefix-stored", [Stored(text[:180], pad_bits=21), Stored(b"", pad_bits=3), Stored(text[:200])]),
        ("prefix-fixed", [Fixed(list(text[:150]) + [M(40, 52), M(258, 1), M(3, 150)] + _lits(160, 5))]),
        ("prefix-dynamic-every-code-length", [Dynamic(ll_lens, d_lens, ops15, plan_style="single")]),
        ("prefix-dynamic-run-coded-header", [_dyn_auto(list(text[:120]) + [M(9, 52), M(100, 104)] + _lits(150, 6), random.Random(3),
                                                         plan_style="runs")]),
        ("prefix-dynamic-random-plan-7-bit-clc", [_clc7_block(list(text[:100]) + [M(30, 52)] + _lits(200, 9, 0, 120))]),
        ("prefix-mixed-blocks", [Stored(text[:40], pad_bits=5), Fixed(mixed_ops[:60]), _dyn_auto(list(text[:90]) + [M(20, 40), M(5, 130)],
                                                                                                   random.Random(5)),
                                 Stored(text[:33]), Fixed([M(33, 33), M(10, 200)])]),
    ]


def _clc7_block(ops, **kw):
    """a dynamic block whose code-length code has 6- and 7-bit words that the header uses"""
    for seed in range(1000):
        rnd = random.Random(seed)
        b = _dyn_auto(ops, rnd, plan_style="random", **kw)
        _, _, valid, _, _ = build([b], c := {})
        if valid and c.get("clc_codelen_7") and c.get("clc_codelen_6"):
            return _dyn_auto(ops, random.Random(seed), plan_style="random", **kw)
    raise AssertionError("no 7-bit code-length code found")


def _aligned(make, want):
    """make(k) -> (blocks, info key function); the k in 0..7 leading 9-bit literals for which want(info) % 8 == 0"""
    for k in range(8):
        blocks = make(k)
        info = build(blocks)[4]
        if want(info) % 8 == 0:
            return blocks, info
    raise AssertionError("no phase aligns")


def handbuilt_cases(census=None):
    census = census if census is not None else {}
    cases = []

    def ok(name, blocks):
        c = case(name, blocks, census)
        assert c.valid, name
        cases.append(c)

    def bad(name, blocks, status, klass):
        c = case(name, blocks)
        assert not c.valid and c.status == status, (name, c.valid, c.status)
        census["refused_" + klass] = census.get("refused_" + klass, 0) + 1
        cases.append(c)

    hi = [200, 201, 250, 255, 144, 199, 222]     # 9-bit literals of the fixed code
    # ---- the smallest streams, `consumed` at both ends of a byte
    ok("fixed-empty", [Fixed([])])
    ok("fixed-6-nine-bit-literals-last-bit-is-bit-7", [Fixed(hi[:6])])
    ok("fixed-7-nine-bit-literals-last-bit-is-bit-0", [Fixed(hi[:7])])
    ok("stored-empty", [Stored(b"")])
    ok("fixed-5000-empty-blocks", [Fixed([]) for _ in range(5000)])
    bad("block-type-3", [Fixed(list(b"abc")), Reserved()], ST_DATA, "block_type_3")
    bad("block-type-3-first", [Reserved()], ST_DATA, "block_type_3")

    # ---- every length and distance symbol at its least and greatest extra value
    for which in ("min", "max"):
        ops = list(b"0123456789")
        for ls in range(29):
            ops.append((ls, 0 if which == "min" else (1 << _LEN_XB[ls]) - 1, 3, 0))
            ops.append(65 + ls)
        ok("fixed-every-length-symbol-%s" % which, [Fixed(ops)])
        ok("dynamic-every-length-symbol-%s" % which, [_dyn_auto(ops, random.Random(len(which)))])
    base = bytes((i * 7 + (i >> 8)) & 255 for i in range(32768))
    ops = []
    for ds in range(30):
        ops += [(0, 0, ds, 0), ds, (1, 0, ds, (1 << _DIST_XB[ds]) - 1)]
    ok("fixed-every-distance-symbol-min-max-32768", [Stored(base), Fixed(ops)])
    ok("dynamic-every-distance-symbol-min-max-32768", [Stored(base), _dyn_auto(ops, random.Random(30))])
    ok("length-258-as-symbol-284-extra-31", [Fixed(list(b"ab") + [(27, 31, 1, 0), M(258, 2), (27, 31, 0, 0)])])
    bad("fixed-length-symbol-286", [Fixed(list(b"abcd") + [(29, 0, 0, 0)])], ST_DATA, "length_symbol_286_287")
    bad("fixed-length-symbol-287", [Fixed(list(b"abcd") + [M(3, 2), (30, 0, 0, 0)])], ST_DATA, "length_symbol_286_287")
    bad("fixed-distance-symbol-30", [Fixed(list(b"abcd") + [(0, 0, 30, 0)])], ST_DATA, "distance_symbol_30_31")
    bad("fixed-distance-symbol-31", [Fixed(list(b"abcd") + [M(4, 4), (5, 0, 31, 0)])], ST_DATA, "distance_symbol_30_31")
    for n in (1, 5, 24, 300):
        ok("distance-equals-op-%d" % n, [Fixed(_lits(n, n) + [M(3 if n < 10 else 9, n)])])
        bad("distance-is-op-plus-1-at-%d" % n, [Fixed(_lits(n, n) + [M(3, n + 1)])], ST_DATA, "distance_too_far")
    bad("distance-with-nothing-out", [Fixed([M(3, 1)])], ST_DATA, "distance_too_far")
    bad("distance-too-far-behind-a-stored-block", [Stored(b"stored"), Fixed([M(3, 7)])], ST_DATA, "distance_too_far")
    bad("distance-too-far-after-matches", [Fixed(list(b"xy") + [M(100, 1), M(50, 102), M(4, 153)])], ST_DATA, "distance_too_far")

    # ---- stored blocks
    ok("stored-len-65535", [Stored(bytes((i * 13) & 255 for i in range(65535)))])
    ok("stored-len-0-between-blocks", [Fixed(list(b"ab")), Stored(b"", pad_bits=0x7F), Stored(b"", pad_bits=1), Fixed([M(4, 2)])])
    for k in range(8):       # k nine-bit literals in front: the stored header's first bit lands on every bit phase
        ok("stored-at-bit-phase-%d" % k, [Fixed(hi[:k] if k else []), Stored(b"phase %d" % k, pad_bits=0x55), Fixed([M(5, 7), M(3, 1)])])
    ok("match-reaches-into-stored-block", [Stored(b"The stored bytes a match copies. " * 3), Fixed([M(40, 99), M(99, 33), M(3, 238)])])
    bad("stored-bad-nlen", [Fixed(list(b"ab")), Stored(b"never delivered", nlen=0x1234, refuse=ST_DATA)], ST_DATA, "stored_len_nlen")
    bad("stored-nlen-equals-len", [Stored(b"x" * 5, nlen=5, refuse=ST_DATA)], ST_DATA, "stored_len_nlen")
    bad("stored-short-body", [Fixed(list(b"ab")), Stored(b"only these", len_=400)], ST_TRUNCATED, "stored_short")
    bad("stored-len-65535-short-body", [Stored(b"\x00" * 100, len_=65535)], ST_TRUNCATED, "stored_short")
    cases.append(cut_case("stored-cut-inside-len-nlen", [Fixed(list(b"ab")), Stored(b"abcdef")], 5, census))
    cases.append(cut_case("stored-cut-in-front-of-len", [Fixed(hi[:3]), Stored(b"abcdef")], 5, census))

    # ---- dynamic headers
    rnd = random.Random(15)
    for t in range(3):
        ll_lens, d_lens, pool_lit, pool_len, dsyms = _every_length_codes(rnd)
        ops, _ = _random_ops(rnd, 0, 3500, pool_lit, pool_len, dsyms)
        ok("dynamic-codes-of-every-length-%d" % t, [Dynamic(ll_lens, d_lens, ops + pool_lit + [M(_LEN_BASE[l], 1)[:2] + (d, 0) for l, d in
                                                                                                  zip(pool_len * 3, dsyms) if _DIST_BASE[d] <= 9],
                                                            plan_style=("single", "runs", "random")[t], rnd=rnd, hlit=286, hdist=30)])
    text = list(b"a dynamic block, hand made. ")
    ok("dynamic-hlit-257", [_dyn_auto(text, hlit=257)])
    ok("dynamic-hlit-286", [_dyn_auto(text + [M(3, 5)], hlit=286, hdist=30)])
    ok("dynamic-hdist-1-empty-distance-code-literals-only", [_dyn_auto(text, hdist=1)])
    ll2 = [0] * 286
    ll2[65], ll2[256], ll2[257] = 2, 2, 1
    rev = lambda cl: int(format(cl[0], "0%db" % cl[1])[::-1], 2)
    bad("dynamic-hdist-1-empty-distance-code-with-a-length-code",
        [Dynamic(ll2, [0], [65, Raw(rev(_canon(ll2)[257]), 1), Raw(0, 1, ST_DATA)])], ST_DATA, "empty_distance_code_used")
    ok("dynamic-lone-1-bit-distance-code", [Dynamic(ll2, [1], [65, (0, 0, 0, 0), 65, (0, 0, 0, 0)])])
    bad("dynamic-lone-1-bit-distance-code-unassigned-sibling",
        [Dynamic(ll2, [1], [65, (0, 0, 0, 0), Raw(rev(_canon(ll2)[257]), 1), Raw(1, 1, ST_DATA)])], ST_DATA, "unassigned_code")
    only_eob = [0] * 257
    only_eob[256] = 1
    ok("dynamic-end-of-block-code-alone-then-stored", [Dynamic(only_eob, [1], []), Stored(b"stored after an empty dynamic block")])
    bad("dynamic-end-of-block-code-alone-unassigned-sibling", [Dynamic(only_eob, [1], [Raw(1, 1, ST_DATA)])], ST_DATA, "unassigned_code")
    ll3 = [0] * 257
    ll3[65], ll3[66], ll3[256] = 1, 1, 1
    bad("dynamic-literal-code-over-subscribed", [Dynamic(ll3, [1], [], refuse=ST_DATA)], ST_DATA, "code_over_subscribed")
    ll4 = [0] * 257
    ll4[65], ll4[256] = 2, 2
    bad("dynamic-literal-code-incomplete", [Fixed(text), Dynamic(ll4, [1], [65], refuse=ST_DATA)], ST_DATA, "code_incomplete")
    ll5 = [0] * 258
    ll5[65], ll5[256], ll5[257] = 1, 2, 2
    bad("dynamic-distance-code-incomplete", [Dynamic(ll5, [2, 2, 2], [65], refuse=ST_DATA)], ST_DATA, "code_incomplete")
    bad("dynamic-distance-code-over-subscribed", [Dynamic(ll5, [1, 1, 1], [65], refuse=ST_DATA)], ST_DATA, "code_over_subscribed")
    no_eob = [0] * 257
    no_eob[65], no_eob[66] = 1, 1
    bad("dynamic-no-end-of-block-code", [Fixed(text), Dynamic(no_eob, [1], [65], refuse=ST_DATA, eob=False)], ST_DATA, "no_end_of_block")
    for hlit in (287, 288):
        bad("dynamic-hlit-%d" % hlit, [Fixed(text), Dynamic([8] * 144 + [9] * 112 + [7] * 24 + [8] * (hlit - 280), [5] * 30, [65], hlit=hlit,
                                                              hdist=30, refuse=ST_DATA)], ST_DATA, "hlit_287_288")
    for hdist in (31, 32):
        bad("dynamic-hdist-%d" % hdist, [Dynamic(FIXED_LL[:286], [5] * hdist, [65], hlit=286, hdist=hdist, refuse=ST_DATA)], ST_DATA,
            "hdist_31_32")

    # ---- the code-length code
    ok("dynamic-7-bit-code-length-code", [_clc7_block(text + [M(5, 3), M(70, 1)] + _lits(60, 1, 0, 90))])
    all8 = [8] * 255 + [0, 8]
    clc5 = [0] * 19
    clc5[8], clc5[16], clc5[0] = 1, 2, 2
    ok("dynamic-hclen-5-sixteens-only", [Dynamic(None, None, _lits(300, 2, 0, 254), hlit=257, hdist=1, hclen=5, clc_lens=clc5,
                                                   plan=[(8, 0)] + [(16, 3)] * 42 + [(8, 0), (8, 0), (0, 0), (8, 0), (0, 0)])])
    clc4 = [0] * 19
    clc4[0], clc4[18], clc4[17], clc4[16] = 1, 2, 3, 3
    bad("dynamic-hclen-4-zero-lengths-only", [Fixed(text), Dynamic(None, None, [], hlit=257, hdist=1, hclen=4, clc_lens=clc4,
                                                                     plan=[(18, 127), (17, 7), (0, 0), (16, 3), (18, 93)], refuse=ST_DATA, eob=False)],
        ST_DATA, "hclen_4")
    zero_bits = [Raw(i & 1, 1) for i in range(258)]
    bad("dynamic-all-zero-code-length-code", [Fixed(text), Dynamic([0] * 257, [0], [], hlit=257, hdist=1, hclen=19, clc_lens=[0] * 19,
                                                                     plan=zero_bits, refuse=ST_DATA, eob=False)], ST_DATA, "clc_all_zero")
    bad("dynamic-all-zero-code-length-code-hclen-4", [Dynamic([0] * 286, [0] * 30, [], hlit=286, hdist=30, hclen=4, clc_lens=[0] * 19,
                                                               plan=[Raw(1, 1)] * 316, refuse=ST_DATA, eob=False)], ST_DATA, "clc_all_zero")
    img = build([Fixed(text), Dynamic([0] * 257, [0], [], hlit=257, hdist=1, hclen=19, clc_lens=[0] * 19, plan=zero_bits, refuse=ST_DATA,
                                      eob=False)])[0]
    cases.append(Case("dynamic-all-zero-code-length-code-cut", img[:len(img) - 9], bytes(text), False, ST_TRUNCATED))
    census["refused_truncated"] = census.get("refused_truncated", 0) + 1
    inc = [0] * 19
    inc[0], inc[8] = 1, 2
    bad("dynamic-code-length-code-incomplete", [Dynamic([0] * 257, [0], [], clc_lens=inc, plan=[(0, 0)] * 258, refuse=ST_DATA, eob=False)],
        ST_DATA, "clc_incomplete")
    one = [0] * 19
    one[8] = 1
    bad("dynamic-code-length-code-of-one-word", [Dynamic(all8, [0], [], clc_lens=one, plan=[(8, 0)] * 258, refuse=ST_DATA, eob=False)],
        ST_DATA, "clc_incomplete")
    over = [0] * 19
    over[0], over[8], over[7] = 1, 1, 1
    bad("dynamic-code-length-code-over-subscribed", [Dynamic(all8, [0], [], clc_lens=over, plan=[(8, 0)] * 258, refuse=ST_DATA, eob=False)],
        ST_DATA, "clc_over_subscribed")
    inc2 = [0] * 19
    inc2[0], inc2[8], inc2[7] = 1, 2, 3
    bad("dynamic-code-length-code-unassigned-word", [Fixed(text), Dynamic(all8, [0], [], clc_lens=inc2, plan=[(8, 0)] * 258, refuse=ST_DATA,
                                                                            eob=False)], ST_DATA, "clc_incomplete")

    # ---- repeats: 16 across the literal/distance boundary, 16 first, overruns, TRUNCATED in front of DATA
    cross = [(18, 54), (1, 0), (18, 127), (18, 41), (2, 0), (3, 0), (4, 0), (4, 0), (16, 3), (16, 3), (16, 1)]
    ok("dynamic-16-carries-a-length-across-the-boundary",
       [Dynamic(None, None, [65] * 30 + [(0, 0, 5, 0), (2, 0, 0, 0), (1, 0, 9, 0), 65], hlit=260, hdist=16, plan=cross)])
    ok("dynamic-18-runs-across-the-boundary",
       [Dynamic(None, None, [65, 65], hlit=262, hdist=30,
                plan=[(18, 54), (1, 0), (18, 127), (18, 41), (2, 0), (3, 0), (3, 0), (18, 21), (1, 0)])])
    ok("dynamic-16-at-index-1", [Dynamic(None, None, [0, 1, 2, 3, 0], hlit=257, hdist=1,
                                         plan=[(3, 0), (16, 3), (18, 127), (18, 97), (17, 0), (3, 0), (0, 0)])])
    bad("dynamic-16-at-index-0", [Fixed(text), Dynamic([0] * 257, [0], [], hlit=257, hdist=1, clc_lens=[2 if s in (16, 3, 0, 18) else 0 for s in range(19)],
                                                         plan=[(16, 3), (3, 0)], refuse=ST_DATA, eob=False)], ST_DATA, "repeat_16_first")

    def first16(k):
        return [Fixed(hi[:k] if k else []), Dynamic([0] * 257, [0], [], hlit=257, hdist=1,
                                                    clc_lens=[2 if s in (16, 3, 0, 18) else 0 for s in range(19)], plan=[(16, 3), (3, 0)],
                                                    refuse=ST_DATA, eob=False)]
    blocks, info = _aligned(first16, lambda i: i["plan_code_end"][0][0])
    cases.append(Case("dynamic-16-at-index-0-extra-bits-missing-is-truncated", build(blocks)[0][:info["plan_code_end"][0][0] // 8],
                      build(blocks)[1], False, ST_TRUNCATED))
    census["refused_truncated_before_data"] = census.get("refused_truncated_before_data", 0) + 1
    three = [2 if s in (16, 17, 18, 8) else 0 for s in range(19)]
    for sym, extra, fill in ((16, 3, 254), (17, 7, 250), (18, 127, 200), (18, 0, 250), (16, 0, 256)):
        plan = [(8, 0)] * fill + [(sym, extra)]
        while len(expand_plan(plan)) < 258:
            plan.append((8, 0))
        over_by = len(expand_plan(plan)) - 258
        assert over_by > 0 or sym == 16 and fill == 256
        if over_by <= 0:
            continue
        bad("dynamic-%d-runs-%d-past-hlit-plus-hdist" % (sym, over_by), [Fixed(text), Dynamic(all8, [0], [], hlit=257, hdist=1, clc_lens=three,
                                                                                             plan=plan, refuse=ST_DATA, eob=False)], ST_DATA, "repeat_overrun")
    ok("dynamic-repeats-end-exactly-at-hlit-plus-hdist",
       [Dynamic(None, None, [0, 1, 2, 253, M(3, 2), M(3, 4)], hlit=258, hdist=4,
                plan=[(8, 0)] + [(16, 3)] * 42 + [(8, 0), (0, 0), (0, 0), (8, 0), (8, 0), (2, 0), (16, 0)])])

    # ---- copies: overlap matrix, chains, block boundaries
    for name, blocks in overlap_streams():
        ok(name, blocks)
    chain = list(b"abc")
    prev = 3
    for n in (3, 4, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 100, 3, 258, 258, 5):
        chain.append(M(n, prev))
        prev = n
    ok("fixed-chain-each-source-is-the-match-just-written", [Fixed(chain)])
    ok("dynamic-chain-each-source-is-the-match-just-written", [_dyn_auto(chain, random.Random(9))])
    t2 = b"blocks of all three kinds; "
    ok("mixed-blocks-matches-across-every-boundary",
       [Stored(t2), Fixed([M(10, 27), 33]), _dyn_auto([M(12, 38), 34, M(3, 1)], random.Random(1)), Stored(t2[:9], pad_bits=0x2A),
        _dyn_auto([M(9, 9), M(30, 60), 35], random.Random(2)), Fixed([M(258, 40), M(4, 300)]), Stored(b""), Fixed([M(3, 3)])])
    for n in (63, 64, 65, 127, 128, 129):
        ok("fixed-%d-literals-then-a-match" % n, [Fixed(_lits(n, n) + [M(70, n), 7] + _lits(n, n + 1) + [M(3, 2)])])
    for n in (15, 16, 31, 32):
        ok("fixed-%d-literals-in-all" % n, [Fixed(_lits(n - 8, n) + [M(20, 3)] + _lits(8, n + 1))])

    # ---- the two-phase path's limits (64 KiB slots)
    ok("fixed-65535-literals", [Fixed(_lits(65535, 11))])
    ok("fixed-65536-literals", [Fixed(_lits(65536, 12))])
    ok("fixed-65533-literals-then-a-match", [Fixed(_lits(65533, 13) + [M(3, 65533 - 40000)])])
    maxseq = inflate_maxseq()
    for d in (-1, 0, 1):
        for closing in (0, 5):
            ops = list(b"xyz") + [M(3, 1 + (i % 3)) for i in range(maxseq + d)] + _lits(closing, 14)
            ok("fixed-maxseq%+d-three-byte-matches-%s" % (d, "then-literals" if closing else "last"), [Fixed(ops)])

    # ---- 320 random scripts
    for s in range(320):
        ok("random-script-%03d" % s, random_script(1000 + s))
    assert len({c.name for c in cases}) == len(cases)
    return cases


CENSUS_KEYS = (["rep16", "rep17", "rep18", "rep_gt64", "rep_gt128", "rep16_cross_boundary", "zero_run_cross_boundary", "clc_codelen_6",
                "clc_codelen_7", "hclen_5", "hclen_19", "hlit_257", "hlit_286", "hdist_1", "hdist_30", "empty_distance_code",
                "lone_distance_code", "stored_len_0", "stored_len_65535", "len258_as_284_31", "dist_eq_op", "dist_32768", "overlap",
                "match_into_stored", "match_across_blocks", "lits_before_match_63", "lits_before_match_64", "lits_before_match_65",
                "nl_and_15_is_0", "nl_and_15_is_15", "end_bit_7", "end_bit_0", "fixed_blocks", "dynamic_blocks"]
               + ["stored_phase_%d" % k for k in range(8)]
               + ["len_sym_%d_%s" % (s, w) for s in range(257, 286) for w in ("min", "max")]
               + ["dist_sym_%d_%s" % (s, w) for s in range(30) for w in ("min", "max")]
               + ["ll_codelen_%d" % k for k in range(1, 16)] + ["d_codelen_%d" % k for k in range(1, 16)]
               + ["refused_" + k for k in ("block_type_3", "length_symbol_286_287", "distance_symbol_30_31", "distance_too_far",
                                           "stored_len_nlen", "stored_short", "truncated", "truncated_before_data", "empty_distance_code_used",
                                           "unassigned_code", "code_over_subscribed", "code_incomplete", "no_end_of_block", "hlit_287_288",
                                           "hdist_31_32", "hclen_4", "clc_all_zero", "clc_incomplete", "clc_over_subscribed", "repeat_16_first",
                                           "repeat_overrun")])
