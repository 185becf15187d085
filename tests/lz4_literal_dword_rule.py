"""Which dwords of a 32-byte payload chunk a literal run stores (la_lz4_lit_run_dwords, la_dev.h), restated in Python
over table entries, and the two ways the window kernel's phase L uses it: run by run (put(): every run walks the chunk's
dwords) and dword by dword (the six runs a chunk's thread fetches leave range masks, every dword picks its owner).
Both return the stores they issue as (window offset, payload dword) pairs.  Builds on lz4_literal_plan_rule.py."""
import lz4_literal_plan_rule as R

RUNS_AT_ONCE = 6        # table entries a chunk's thread fetches together


def run_dwords(ls, le, dst, c0):
    """None when the run [ls, le) has no byte in the chunk at c0, else (m0, mend, w0): it stores the chunk's dwords
    [m0, mend), dword m at window offset w0 + 4 m"""
    lo, hi = max(ls, c0), min(le, c0 + 32)
    if hi <= lo:
        return None
    return (lo - c0) >> 2, (hi - c0 + 3) >> 2, dst + c0 - ls


def _run(e, c0):
    ls, ll, dst, _ = R.fields(e)
    return ls, ls + ll, run_dwords(ls, ls + ll, dst, c0)


def stores_by_run(ent, k, c0, fin=False):
    """put() from sequence k on until a run reaches the chunk's end or starts behind it: [(window offset, payload
    dword)] in the order issued"""
    out = []
    while not fin and k < len(ent):
        ls, le, r = _run(ent[k], c0)
        if ls >= c0 + 32:
            break
        if r:
            out += [(r[2] + 4 * m, (c0 >> 2) + m) for m in range(r[0], r[1])]
        fin = le >= c0 + 32
        k += 1
    return out


def stores_by_dword(ent, k, c0):
    """the dword-wise form: sequences k .. k + 5 leave their window offset under the bits of their range mask (a dword
    already taken stays with its first owner), each dword with an owner is stored once; sequences behind the sixth go
    run by run.  Returns the stores and, per dword of the chunk, the runs whose range holds it."""
    owner, claims, any_, fin = [None] * 8, [0] * 8, 0, k + RUNS_AT_ONCE - 1 >= len(ent)
    for t in range(RUNS_AT_ONCE):
        if k + t >= len(ent):
            break       # (the kernel reads a zero entry here: no dwords)
        ls, le, r = _run(ent[k + t], c0)
        fin = fin or le >= c0 + 32
        if not r:
            continue
        mask = ((1 << (r[1] - r[0])) - 1) << r[0]
        for m in range(8):
            claims[m] += (mask >> m) & 1
        mask &= ~any_
        any_ |= mask
        for m in range(8):
            if (mask >> m) & 1:
                owner[m] = r[2]
    out = [(owner[m] + 4 * m, (c0 >> 2) + m) for m in range(8) if (any_ >> m) & 1]
    return out + stores_by_run(ent, k + RUNS_AT_ONCE, c0, fin), claims


def place(stores, payload, olen):
    """the window (16 bytes of headroom in front) behind those stores"""
    pay = bytes(payload) + bytes(64)
    win = bytearray(16 + olen + 16)
    for w, p in stores:
        assert w >= -3
        win[16 + w:16 + w + 4] = pay[4 * p:4 * p + 4]
    return win
