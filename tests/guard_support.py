"""TEST INFRASTRUCTURE for the guard-band tests (tests/test_decoder_guard_cases.py, tests/test_gpu_decoder_guards.py):
a destination between two guards, the assert that nothing outside the allowed slots changed, and the two-fills run.

A byte-exact decoder can still write outside its unit's output range, let its output depend on what the destination
held, or let its verdict depend on bytes behind src_bytes.  A destination prefilled with a known byte, with guards on
both sides, shows the first; a second run over another fill and other bytes behind the source shows the other two, and
a stray store whose value happens to equal one guard byte.

No torch at import: GuardedBuffer and SourceBuffer sit over numpy for the CPU stand-ins (which take host pointers) and
over a torch CUDA tensor when a device is named."""
import numpy as np

GUARD = 4096        # a stray 16-byte (or 1 KiB) store next to a slot stays inside allocated memory
JUNK_BYTES = 64     # what stands in the source allocation behind src_bytes
FILLS = (0xA5, 0x5A)
# the bytes behind src_bytes: text that goes on as a decodable line and a line end, and binary that reads as LZO / LZMA /
# bzip2 input of some kind; neither may reach a verdict or a byte of output
JUNK = ((b"QUJDRA==\nM86%N9\"!T:&4@8G5N:P``\n`\nend\n" + b"QUJD" * 16)[:JUNK_BYTES],
        (bytes([0xFF, 0x00, 0xE8, 0x11, 0x00, 0x00, 0x31, 0x41, 0x59, 0x26, 0x53, 0x59, 0x0A, 0x80, 0x0D, 0x02]) * 4)[:JUNK_BYTES])


def _allocate(size, fill, device):
    """(whole allocation as a 1-D uint8 array / tensor whose first byte lies on the 16-byte grid, its address)"""
    if device is None:
        raw = np.full(size + 16, fill, dtype=np.uint8)
        lead = -raw.ctypes.data % 16
        whole = raw[lead:lead + size]
        return whole, whole.ctypes.data
    import torch
    whole = torch.full((size,), fill, dtype=torch.uint8, device=device)
    assert whole.data_ptr() % 16 == 0
    return whole, whole.data_ptr()


def _to_host(whole):
    return whole.copy() if isinstance(whole, np.ndarray) else whole.cpu().numpy()


class GuardedBuffer:
    """One allocation of guard + shift + total + guard bytes, all `fill`.  `data` is the view of the `total` bytes in the
    middle (a numpy array, or a tensor on `device`), `ptr` its address: `shift` (0 .. 15) moves it off the 16-byte grid."""

    def __init__(self, total, fill, shift=0, guard=GUARD, device=None):
        assert 0 <= shift <= 15 and 0 <= fill <= 255 and guard >= 0
        self.total, self.fill, self.shift, self.guard = int(total), fill, shift, guard
        self.lead = guard + shift
        self.whole, base = _allocate(self.lead + self.total + guard, fill, device)
        self.ptr = base + self.lead
        self.data = self.whole[self.lead:self.lead + self.total]
        assert self.ptr % 16 == shift

    def host(self):
        """the whole allocation, guards included, as a numpy array on the host"""
        return _to_host(self.whole)

    def read(self, off, n):
        """bytes [off, off + n) of the data"""
        return _to_host(self.whole[self.lead + off:self.lead + off + n]).tobytes()


class SourceBuffer:
    """`image` at an address `shift` bytes off the 16-byte grid, with `junk` behind it in the same allocation: the junk is
    never counted in src_bytes.  `data` is the view of the image alone, `ptr` its address, `n` its length."""

    def __init__(self, image, junk, shift=0, device=None):
        image = bytes(image)
        assert len(junk) == JUNK_BYTES and 0 <= shift <= 15
        self.n = len(image)
        host = np.frombuffer(bytes(shift) + image + bytes(junk), dtype=np.uint8)
        self.whole, base = _allocate(len(host), 0, device)
        if device is None:
            self.whole[:] = host
        else:
            import torch
            self.whole.copy_(torch.from_numpy(host.copy()))
        self.ptr = base + shift
        self.data = self.whole[shift:shift + self.n]


def assert_only_slots_changed(buf, slots, labels=None):
    """Every byte of `buf` outside `slots` [(off, length)] (offsets inside the data), both guards included, still equals
    the fill.  The failure names the first changed offset and the slot that ends nearest to it (by `labels`, one per
    slot, when given)."""
    h = buf.host()
    free = np.zeros(len(h), dtype=bool)
    for off, n in slots:
        assert 0 <= off and off + n <= buf.total, ("a slot outside the buffer", off, n, buf.total)
        free[buf.lead + off:buf.lead + off + n] = True
    changed = np.flatnonzero((h != buf.fill) & ~free)
    if len(changed) == 0:
        return
    at = int(changed[0]) - buf.lead
    where = "front guard" if at < 0 else "back guard" if at >= buf.total else "data"
    if slots:
        k = min(range(len(slots)), key=lambda i: abs(slots[i][0] + slots[i][1] - at))
        near = "slot %d%s [%d, %d) ends nearest, %+d bytes from its end" % (k, " (%s)" % labels[k] if labels else "", slots[k][0], slots[k][0] + slots[k][1],
                                                                             at - (slots[k][0] + slots[k][1]))
    else:
        near = "no slot may change"
    raise AssertionError("guard: offset %d (%s, address residue %d) changed from fill 0x%02X to 0x%02X, %d byte(s) changed outside the slots; %s"
                         % (at, where, (buf.ptr + at) % 16, buf.fill, int(h[changed[0]]), len(changed), near))


def two_fills(run):
    """run(fill, junk) for (0xA5, junk A) and (0x5A, junk B).  It returns (result records, [bytes of every allowed slot's
    defined part]); both must be the same under both fills.  (Inside a slot, only what the decoder reports as produced is
    defined: the rest of a failed unit's slot is free and may keep the fill.)  Returns the first run's answer."""
    first = run(FILLS[0], JUNK[0])
    second = run(FILLS[1], JUNK[1])
    assert first[0] == second[0], "the result records depend on the destination's fill or on bytes behind src_bytes"
    assert len(first[1]) == len(second[1])
    for i, (a, b) in enumerate(zip(first[1], second[1])):
        assert a == b, "the bytes of slot %d depend on the destination's fill or on bytes behind src_bytes" % i
    return first
