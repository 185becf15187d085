"""Device-resident lzip member scan, decode and compression through the C ABI (harness for tests / tools).  Plumbing
only: torch allocates the HBM buffers; the member table is the caller's (members are chained on the host,
host/la_filter_lzip.c), all work is la_gpu_lzip_scan(), la_gpu_lzip_decode() and la_gpu_lzip_compress()."""
import numpy as np

from . import _native as N

LZIP_MEMBER_DTYPE, LZIP_RESULT_DTYPE, LA_LZIP_UNKNOWN, LA_LZIP_HAS_CRC = N.LZIP_MEMBER_DTYPE, N.LZIP_RESULT_DTYPE, N.LA_LZIP_UNKNOWN, N.LA_LZIP_HAS_CRC
STATUS = {0: "OK", N.LA_ST_LZIP_DATA: "DATA", N.LA_ST_LZIP_SRC_END: "SRC_END", N.LA_ST_LZIP_TRUNCATED: "TRUNCATED",
          N.LA_ST_LZIP_EARLY_END: "EARLY_END", N.LA_ST_LZIP_SIZE_OVER: "SIZE_OVER", N.LA_ST_LZIP_OUT_FULL: "OUT_FULL",
          N.LA_ST_LZIP_BAD_SIZE: "BAD_SIZE", N.LA_ST_LZIP_BAD_CRC: "BAD_CRC", N.LA_ST_LZIP_REFUSED: "REFUSED"}


def dict_size(b):
    """the dictionary size a header's dictionary byte stands for"""
    size = 1 << (b & 0x1F)
    if (b & 0x1F) > 12:
        size -= (size // 16) * (b >> 5)
    return size


def member_bytes(level=6):
    """input bytes per member at `level` (0 above 9)"""
    return int(N.gpu_lib().la_gpu_lzip_compress_member_bytes(level))


def compress_bound(n, level=6):
    return int(N.gpu_lib().la_gpu_lzip_compress_bound(n, level))


def compress_window(ctx, d_plain, level=6, out_cap=None, d_out=None):
    """Device lzip compression of one window (la_gpu_lzip_compress): d_plain is a 1-D uint8 CUDA tensor; returns a uint8
    CUDA tensor holding the window's members back to back, a whole lzip stream.  With `out_cap` (and optionally `d_out`)
    the call gets that much room only and the needed size is returned beside the tensor."""
    import torch
    n = int(d_plain.numel())
    dev = d_plain.device
    cap = compress_bound(n, level) if out_cap is None else int(out_cap)
    if d_out is None:
        d_out = torch.empty(max(cap, 16), dtype=torch.uint8, device=dev)
    d_len = torch.zeros(1, dtype=torch.int64, device=dev)
    b = N._LzcBatchC()
    b.d_src, b.src_bytes = (d_plain.data_ptr() if n else None), n
    b.level, b.flags = level, 0
    b.d_out, b.out_cap, b.d_out_bytes = d_out.data_ptr(), cap, d_len.data_ptr()
    ctx.lzip_compress(b)
    ctx.sync()
    total = int(d_len.cpu()[0])
    if out_cap is not None:
        return d_out, total
    assert total <= cap, (total, cap)
    return d_out[:total]


def to_device(image):
    import torch
    buf = np.frombuffer(bytes(image), dtype=np.uint8)
    return torch.from_numpy(buf.copy()).cuda() if buf.size else torch.zeros(0, dtype=torch.uint8, device="cuda")


def scan(ctx, d_src, cap=1 << 16, n=None):
    """la_gpu_lzip_scan over the first n bytes (all) of a 1-D uint8 CUDA tensor: (offsets kept, number found)"""
    import torch
    n = int(d_src.numel()) if n is None else int(n)
    d_offs = torch.zeros(max(cap, 1), dtype=torch.int64, device=d_src.device)
    d_count = torch.zeros(1, dtype=torch.int32, device=d_src.device)
    ctx.lzip_scan(d_src.data_ptr() if n else None, n, d_offs.data_ptr() if cap else None, cap, d_count.data_ptr())
    ctx.sync()
    count = int(d_count.cpu().numpy().view(np.uint32)[0])
    return d_offs.cpu().numpy().view(np.uint64)[:min(count, cap)].copy(), count


def member_table(entries):
    """ndarray of LZIP_MEMBER_DTYPE from dicts; fields left out: both ends unknown, dictionary 1 MiB, no CRC."""
    t = np.zeros(len(entries), dtype=LZIP_MEMBER_DTYPE)
    for i, e in enumerate(entries):
        t[i] = (e["src_off"], e.get("src_end", LA_LZIP_UNKNOWN), e.get("data_size", LA_LZIP_UNKNOWN), e.get("dst_off", 0), e["dst_cap"],
                e.get("dict_size", 1 << 20), e.get("crc32", 0), LA_LZIP_HAS_CRC if "crc32" in e else 0, 0)
    return t


class LzipDevicePlan:
    """One call: run() decodes the table; results() / output(i) read back.  `d_dst` is the caller's destination (a 1-D
    uint8 tensor of at least dst_cap bytes, a view at any offset) instead of a zeroed one of the plan's own."""

    def __init__(self, ctx, d_src, members, dst_cap=None, d_dst=None):
        import torch
        dev = d_src.device
        self.ctx, self.n, self.d_src, self.members = ctx, len(members), d_src, members
        if dst_cap is None:
            dst_cap = max([int(m["dst_off"] + m["dst_cap"]) for m in members], default=0)
        self.dst_cap = int(dst_cap)
        table = np.ascontiguousarray(members).view(np.uint8).reshape(-1)
        self.d_members = torch.from_numpy(table.copy()).to(dev) if self.n else torch.zeros(16, dtype=torch.uint8, device=dev)
        self.d_results = torch.zeros(max(self.n, 1) * LZIP_RESULT_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        self.d_dst = d_dst if d_dst is not None else torch.zeros(max(self.dst_cap, 16), dtype=torch.uint8, device=dev)
        assert self.d_dst.numel() >= self.dst_cap
        b = N._LzipBatchC()
        b.d_src, b.src_bytes = (d_src.data_ptr() if d_src.numel() else None), d_src.numel()
        b.d_members, b.n = self.d_members.data_ptr(), self.n
        b.d_dst, b.dst_cap, b.d_results = self.d_dst.data_ptr(), self.dst_cap, self.d_results.data_ptr()
        b.reserved = 0
        self.batch = b

    def run(self):
        self.ctx.lzip_decode(self.batch)
        return self

    def results(self):
        self.ctx.sync()
        return self.d_results.cpu().numpy().view(LZIP_RESULT_DTYPE)[:self.n].copy()

    def output(self, i=None):
        res = self.results()
        if i is None:
            return b"".join(self.output(k) for k in range(self.n))
        off, n = int(self.members[i]["dst_off"]), int(res[i]["out_len"])
        return self.d_dst[off:off + n].cpu().numpy().tobytes()


def decode_members(ctx, image, entries, dst_cap=None):
    """Upload a host image and decode the members `entries` describe (see member_table).  Returns (results, plan)."""
    plan = LzipDevicePlan(ctx, to_device(image), member_table(entries), dst_cap).run()
    return plan.results(), plan
