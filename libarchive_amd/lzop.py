"""Device-resident lzop block decode, block compression and many-range Adler-32 through the C ABI (harness for tests /
tools).  Plumbing only: torch allocates the HBM buffers; the block table is the caller's (the host hops from block header
to block header, host/la_filter_lzop.c), all work is la_gpu_lzop_decode(), la_gpu_lzop_compress() and
la_gpu_adler32_many()."""
import numpy as np

from . import _native as N

LZOP_BLOCK_DTYPE, LZOP_RESULT_DTYPE = N.LZOP_BLOCK_DTYPE, N.LZOP_RESULT_DTYPE
C_ADLER32, C_CRC32, U_ADLER32, U_CRC32 = N.LA_LZOP_C_ADLER32, N.LA_LZOP_C_CRC32, N.LA_LZOP_U_ADLER32, N.LA_LZOP_U_CRC32
STATUS = {0: "OK", N.LA_ST_LZOP_BAD_SUM_C: "BAD_SUM_C", N.LA_ST_LZOP_INPUT_OVERRUN: "INPUT_OVERRUN", N.LA_ST_LZOP_OUTPUT_OVERRUN: "OUTPUT_OVERRUN",
          N.LA_ST_LZOP_LOOKBEHIND: "LOOKBEHIND", N.LA_ST_LZOP_NOT_CONSUMED: "NOT_CONSUMED", N.LA_ST_LZOP_SHORT_OUTPUT: "SHORT_OUTPUT",
          N.LA_ST_LZOP_BAD_SUM_U: "BAD_SUM_U", N.LA_ST_LZOP_REFUSED: "REFUSED"}


BLOCK_BYTES = N.LA_LZOPC_BLOCK_BYTES


def compress_bound(n, block_size=BLOCK_BYTES):
    """bytes the blocks of n input bytes can take (0 for block_size 0); a lead is the caller's to add"""
    return int(N.gpu_lib().la_gpu_lzop_compress_bound(n, block_size))


def compress_window(ctx, d_src, block_size=BLOCK_BYTES, lead_bytes=0, out_cap=None, d_out=None):
    """Device lzop compression of one window (la_gpu_lzop_compress): d_src is a 1-D uint8 CUDA tensor; returns a uint8
    CUDA tensor holding `lead_bytes` of untouched gap and the window's blocks back to back (no header, no closing word).
    With `out_cap` (and optionally `d_out`) the call gets that much room only and the needed size is returned beside the
    tensor."""
    import torch
    n = int(d_src.numel())
    dev = d_src.device
    cap = lead_bytes + compress_bound(n, block_size) if out_cap is None else int(out_cap)
    if d_out is None:
        d_out = torch.zeros(max(cap, 16), dtype=torch.uint8, device=dev)
    d_len = torch.zeros(1, dtype=torch.int64, device=dev)
    b = N._LzopcBatchC()
    b.d_src, b.src_bytes = (d_src.data_ptr() if n else None), n
    b.block_size, b.lead_bytes = block_size, lead_bytes
    b.d_out, b.out_cap, b.d_out_bytes = d_out.data_ptr(), cap, d_len.data_ptr()
    ctx.lzop_compress(b)
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


def adler32_many(ctx, d_base, jobs):
    """la_gpu_adler32_many over ranges of a 1-D uint8 CUDA tensor: jobs is [(off, len, seed)], a fresh sum starts from 1"""
    import torch
    n = len(jobs)
    t = np.zeros(max(n, 1), dtype=N.HASH_JOB_DTYPE)
    for i, j in enumerate(jobs):
        t[i] = j
    d_jobs = torch.from_numpy(t.view(np.uint8).reshape(-1).copy()).to(d_base.device)
    d_out = torch.zeros(max(n, 1), dtype=torch.int32, device=d_base.device)
    ctx.adler32_many(d_base.data_ptr(), d_jobs.data_ptr(), n, d_out.data_ptr())
    ctx.sync()
    return d_out.cpu().numpy().view(np.uint32)[:n].copy()


def block_table(entries):
    """ndarray of LZOP_BLOCK_DTYPE from dicts; fields left out: no sums"""
    t = np.zeros(len(entries), dtype=LZOP_BLOCK_DTYPE)
    for i, e in enumerate(entries):
        t[i] = (e["src_off"], e.get("dst_off", 0), e["src_len"], e["dst_len"], e.get("flags", 0), e.get("sum_c", 0), e.get("sum_u", 0), 0)
    return t


class LzopDevicePlan:
    """One call: run() decodes the table; results() / slab() read back.  `d_dst` is the caller's destination (a 1-D uint8
    tensor of at least dst_cap bytes, a view at any offset) instead of a zeroed one of the plan's own."""

    def __init__(self, ctx, d_src, blocks, dst_cap=None, d_dst=None):
        import torch
        dev = d_src.device
        self.ctx, self.n, self.d_src, self.blocks = ctx, len(blocks), d_src, blocks
        if dst_cap is None:
            dst_cap = max([int(b["dst_off"]) + int(b["dst_len"]) for b in blocks], default=0)
        self.dst_cap = int(dst_cap)
        table = np.ascontiguousarray(blocks).view(np.uint8).reshape(-1)
        self.d_blocks = torch.from_numpy(table.copy()).to(dev) if self.n else torch.zeros(16, dtype=torch.uint8, device=dev)
        self.d_results = torch.zeros(max(self.n, 1) * LZOP_RESULT_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        self.d_dst = d_dst if d_dst is not None else torch.zeros(max(self.dst_cap, 16), dtype=torch.uint8, device=dev)
        assert self.d_dst.numel() >= self.dst_cap
        b = N._LzopBatchC()
        b.d_src, b.src_bytes = (d_src.data_ptr() if d_src.numel() else None), d_src.numel()
        b.d_blocks, b.n = self.d_blocks.data_ptr(), self.n
        b.d_dst, b.dst_cap, b.d_results = self.d_dst.data_ptr(), self.dst_cap, self.d_results.data_ptr()
        b.reserved = 0
        self.batch = b

    def run(self):
        self.ctx.lzop_decode(self.batch)
        return self

    def results(self):
        self.ctx.sync()
        return self.d_results.cpu().numpy().view(LZOP_RESULT_DTYPE)[:self.n].copy()

    def slab(self):
        """the whole output buffer on the host"""
        self.ctx.sync()
        return self.d_dst[:self.dst_cap].cpu().numpy().tobytes()


def decode_blocks(ctx, image, entries, dst_cap=None):
    """Upload a host image and decode the blocks `entries` describe (see block_table).  Returns (results, plan)."""
    plan = LzopDevicePlan(ctx, to_device(image), block_table(entries), dst_cap).run()
    return plan.results(), plan
