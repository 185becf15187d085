"""The literal plan of an lz4 window block (la_lz4_lit_chunk_edge, la_dev.h), restated in Python over table entries
(lit_src | lit_len << 16 | dst << 32 | off << 48), with a block parser that makes such entries from an encoded block and
an interpreter that places literals the way the window kernel's phase L does from the plan.  Shared by
test_lz4_literal_plan_rule.py (no GPU) and test_gpu_lz4_literal_plan.py."""

NONE = 0xFFFF


def chunk_edge(lit_end):
    """the payload chunks [0, edge) begin in front of lit_end"""
    return (lit_end + 31) >> 5


def plan_entries(src_len):
    return chunk_edge(src_len) + 1


def slot_entries(src_len):
    """table entries in the slot of a block with src_len payload bytes (lz4_table_caps_kernel)"""
    return (src_len // 3 + 8) & ~7


def fields(e):
    e = int(e)
    return e & 0xFFFF, (e >> 16) & 0xFFFF, (e >> 32) & 0xFFFF, e >> 48     # lit_src, lit_len, dst, off


def parse_block(enc):
    """table entries of one encoded lz4 block, the last (literal-only) sequence with offset 0, and the decoded length"""
    ent, ip, dst = [], 0, 0
    while ip < len(enc):
        tok = enc[ip]
        ip += 1
        ll = tok >> 4
        if ll == 15:
            while True:
                b = enc[ip]
                ip += 1
                ll += b
                if b != 255:
                    break
        ls = ip
        ip += ll
        if ip >= len(enc):
            ent.append(ls | ll << 16 | (dst & 0xFFFF) << 32)
            dst += ll
            break
        off = enc[ip] | enc[ip + 1] << 8
        ip += 2
        ml = tok & 15
        if ml == 15:
            while True:
                b = enc[ip]
                ip += 1
                ml += b
                if b != 255:
                    break
        ent.append(ls | ll << 16 | dst << 32 | off << 48)
        dst += ll + ml + 4
    return ent, dst


def rule_plan(ent, src_len):
    """entry c < ceil(src_len / 32): the first sequence whose literals end beyond payload offset 32 c, NONE when there
    is none; then the number of chunks that hold literals"""
    nchunks = chunk_edge(src_len)
    ends = [fields(e)[0] + fields(e)[1] for e in ent]
    plan, k = [], 0
    for c in range(nchunks):
        while k < len(ends) and ends[k] <= 32 * c:
            k += 1
        plan.append(k if k < len(ends) else NONE)
    plan.append(min(chunk_edge(ends[-1]) if ends else 0, nchunks))
    return plan


def place_literals(plan, ent, payload, olen):
    """Phase L from the plan: the thread of chunk c starts at sequence plan[c] and stores, for every sequence with
    literals inside the chunk, the chunk's dwords that meet the run -- whole dwords at window position
    dst + 4 P - lit_src, spilling up to three bytes over either end of the run.  Returns the window (16 bytes of headroom
    in front) and, per payload dword, how many runs stored it."""
    src_len = len(payload)
    pay = bytes(payload) + bytes(64)
    win = bytearray(16 + olen + 16)
    stored = [0] * (chunk_edge(src_len) * 8)
    for c in range(chunk_edge(src_len)):
        k = plan[c]
        if k == NONE:
            continue
        c0, c1 = 32 * c, 32 * c + 32
        while k < len(ent):
            ls, ll, dst, _ = fields(ent[k])
            le = ls + ll
            if ls >= c1:
                break
            lo, hi = max(ls, c0), min(le, c1)
            if hi > lo:
                for m in range((lo - c0) >> 2, (hi - c0 + 3) >> 2):
                    p = c0 + 4 * m
                    w = 16 + dst + p - ls
                    assert w >= 13
                    win[w:w + 4] = pay[p:p + 4]
                    stored[p >> 2] += 1
            if le >= c1:
                break
            k += 1
    return win, stored


def copy_matches(win, ent, olen):
    """the matches in order, byte by byte, behind the literals"""
    for k, e in enumerate(ent):
        _, ll, dst, off = fields(e)
        mdst = dst + ll
        end = fields(ent[k + 1])[2] if k + 1 < len(ent) else olen
        if end < mdst:
            end += 65536       # (positions are 16-bit: an end at 65536 reads 0)
        for i in range(mdst, end):
            win[16 + i] = win[16 + i - off]
    return bytes(win[16:16 + olen])
