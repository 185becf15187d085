"""Device-resident xz block decode and compression through the C ABI (harness for tests / tools).  Plumbing only: torch
allocates the HBM buffers; the block table is the caller's (the container is walked on the host, host/la_filter_xz.c),
all work is la_gpu_xz_decode() and la_gpu_xz_compress()."""
import numpy as np

from . import _native as N

XZ_BLOCK_DTYPE, XZ_RESULT_DTYPE, LA_XZ_UNKNOWN = N.XZ_BLOCK_DTYPE, N.XZ_RESULT_DTYPE, N.LA_XZ_UNKNOWN
XZ_CHAIN_DTYPE, LA_XZ_BATCH_CHAINS = N.XZ_CHAIN_DTYPE, N.LA_XZ_BATCH_CHAINS
LA_ST_XZ_DATA, LA_ST_XZ_LZMA, LA_ST_XZ_TRUNCATED, LA_ST_XZ_SIZE = N.LA_ST_XZ_DATA, N.LA_ST_XZ_LZMA, N.LA_ST_XZ_TRUNCATED, N.LA_ST_XZ_SIZE
LA_ST_XZ_BAD_CHECK, LA_ST_XZ_PADDING, LA_ST_XZ_OUT_FULL = N.LA_ST_XZ_BAD_CHECK, N.LA_ST_XZ_PADDING, N.LA_ST_XZ_OUT_FULL
LA_XZC_FIRST, LA_XZC_BLOCK_BYTES, LA_XZC_CHUNK_BYTES = N.LA_XZC_FIRST, N.LA_XZC_BLOCK_BYTES, N.LA_XZC_CHUNK_BYTES


def compress_bound(n, level=6):
    return int(N.gpu_lib().la_gpu_xz_compress_bound(n, level))


def compress_window(ctx, d_plain, level=6, flags=N.LA_XZC_FIRST, out_cap=None, d_out=None):
    """Device xz compression of one window (la_gpu_xz_compress): d_plain is a 1-D uint8 CUDA tensor; returns a uint8 CUDA
    tensor holding the window's blocks back to back, the stream header in front under LA_XZC_FIRST (index and footer are
    the write filter's).  With `out_cap` (and optionally `d_out`) the call gets that much room only and the needed size
    is returned beside the tensor."""
    import torch
    n = int(d_plain.numel())
    dev = d_plain.device
    cap = compress_bound(n, level) if out_cap is None else int(out_cap)
    if d_out is None:
        d_out = torch.empty(max(cap, 16), dtype=torch.uint8, device=dev)
    d_len = torch.zeros(1, dtype=torch.int64, device=dev)
    b = N._XzcBatchC()
    b.d_src, b.src_bytes = (d_plain.data_ptr() if n else None), n
    b.level, b.flags = level, flags
    b.d_out, b.out_cap, b.d_out_bytes = d_out.data_ptr(), cap, d_len.data_ptr()
    ctx.xz_compress(b)
    ctx.sync()
    total = int(d_len.cpu()[0])
    if out_cap is not None:
        return d_out, total
    assert total <= cap, (total, cap)
    return d_out[:total]


def block_table(entries):
    """ndarray of XZ_BLOCK_DTYPE from dicts; fields left out: sizes and check offset unknown, dictionary 8 MiB, no check."""
    t = np.zeros(len(entries), dtype=XZ_BLOCK_DTYPE)
    for i, e in enumerate(entries):
        t[i] = (e["src_off"], e.get("comp_size", LA_XZ_UNKNOWN), e.get("uncomp_size", LA_XZ_UNKNOWN), e.get("dst_off", 0), e["dst_cap"],
                e.get("check_off", LA_XZ_UNKNOWN), e.get("dict_size", 1 << 23), e.get("check_id", 0))
    return t


def chain_table(chains):
    """ndarray of XZ_CHAIN_DTYPE from one list per block of (filter id, property) pairs in chain order, LZMA2 left out:
    the property is delta's distance (1 .. 256) or a BCJ filter's start_offset.  (Nothing is checked here: the device
    call judges the entries.)"""
    t = np.zeros(len(chains), dtype=XZ_CHAIN_DTYPE)
    for i, ch in enumerate(chains):
        t[i]["count"] = len(ch)
        for k, (fid, prop) in enumerate(ch[:3]):
            t[i]["id"][k], t[i]["prop"][k] = fid, prop
    return t


class XzDevicePlan:
    """One call: run() decodes the table; results() / output(i) read back.  With `chains` (see chain_table) the chain
    table rides behind the blocks and the call is made with LA_XZ_BATCH_CHAINS.  `d_dst` is the caller's destination (a
    1-D uint8 tensor of at least dst_cap bytes, a view at any offset) instead of a zeroed one of the plan's own."""

    def __init__(self, ctx, d_src, blocks, dst_cap=None, chains=None, d_dst=None):
        import torch
        dev = d_src.device
        self.ctx, self.n, self.d_src, self.blocks = ctx, len(blocks), d_src, blocks
        if dst_cap is None:
            dst_cap = max([int(b["dst_off"] + b["dst_cap"]) for b in blocks], default=0)
        self.dst_cap = int(dst_cap)
        table = np.ascontiguousarray(blocks).view(np.uint8).reshape(-1)
        if chains is not None:
            assert len(chains) == self.n
            table = np.concatenate([table, np.ascontiguousarray(chain_table(chains)).view(np.uint8).reshape(-1)])
        self.d_blocks = torch.from_numpy(table.copy()).to(dev) if self.n else torch.zeros(16, dtype=torch.uint8, device=dev)
        self.d_results = torch.zeros(max(self.n, 1) * XZ_RESULT_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        self.d_dst = d_dst if d_dst is not None else torch.zeros(max(self.dst_cap, 16), dtype=torch.uint8, device=dev)
        assert self.d_dst.numel() >= self.dst_cap
        b = N._XzBatchC()
        b.d_src, b.src_bytes = (d_src.data_ptr() if d_src.numel() else None), d_src.numel()
        b.d_blocks, b.n = self.d_blocks.data_ptr(), self.n
        b.d_dst, b.dst_cap, b.d_results = self.d_dst.data_ptr(), self.dst_cap, self.d_results.data_ptr()
        b.reserved = LA_XZ_BATCH_CHAINS if chains is not None else 0
        self.batch = b

    def run(self):
        self.ctx.xz_decode(self.batch)
        return self

    def results(self):
        self.ctx.sync()
        return self.d_results.cpu().numpy().view(XZ_RESULT_DTYPE)[:self.n].copy()

    def output(self, i=None):
        res = self.results()
        if i is None:
            return b"".join(self.output(k) for k in range(self.n))
        off, n = int(self.blocks[i]["dst_off"]), int(res[i]["out_len"])
        return self.d_dst[off:off + n].cpu().numpy().tobytes()


def decode_blocks(ctx, image, entries, chains=None):
    """Upload a host image, decode the blocks `entries` describe (see block_table), with `chains` (see chain_table)
    their delta / BCJ filters undone.  Returns (results, plan)."""
    import torch
    buf = np.frombuffer(bytes(image), dtype=np.uint8)
    d_src = torch.from_numpy(buf.copy()).cuda() if buf.size else torch.zeros(0, dtype=torch.uint8, device="cuda")
    plan = XzDevicePlan(ctx, d_src, block_table(entries), chains=chains).run()
    return plan.results(), plan
