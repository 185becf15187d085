"""Device-resident gzip batch decode through the C ABI (harness for tests / bench.py).
Plumbing only: torch allocates the HBM buffers; all work is la_gpu_gzip_decode()."""
import numpy as np

from . import _native as N


class GzDevicePlan:
    def __init__(self, ctx, d_src, index, device=None):
        import torch
        dev = d_src.device if device is None else device
        self.ctx, self.index, self.d_src = ctx, index, d_src
        n = len(index.members)
        self.n = n
        self.dst_cap = int(index.max_out)
        self.d_members = torch.from_numpy(index.members.view(np.uint8).reshape(-1).copy()).to(dev)
        self.d_dst = torch.empty(max(self.dst_cap, 16), dtype=torch.uint8, device=dev)
        self.d_results = torch.zeros(max(n, 1) * N.GZ_RESULT_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        self.d_summary = torch.zeros(N.SUMMARY_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        b = N._GzBatchC()
        b.d_src = d_src.data_ptr(); b.src_bytes = d_src.numel()
        b.d_members = self.d_members.data_ptr(); b.n_members = n
        b.d_dst = self.d_dst.data_ptr(); b.dst_cap = self.dst_cap
        b.d_results = self.d_results.data_ptr(); b.d_summary = self.d_summary.data_ptr()
        self.batch = b

    def run(self, options=0):
        self.batch.options = options
        self.ctx.gzip_decode(self.batch)

    def summary(self):
        self.ctx.sync()
        return self.d_summary.cpu().numpy().view(N.SUMMARY_DTYPE)[0]

    def results(self):
        self.ctx.sync()
        return self.d_results.cpu().numpy().view(N.GZ_RESULT_DTYPE)[:self.n]


def piece_index(image, start=0, at_eof=True, **kw):
    """Piece table of ONE member's body (image[start:] starts on a byte-aligned deflate block boundary, e.g. behind the
    gzip header): one la_gz_member per span between flush markers, for GzDevicePlan + decode_pieces."""
    return N.gz_pieces(image, start, at_eof, **kw)


def decode_pieces(ctx, d_src, pieces, options=0):
    """la_gpu_gzip_decode with LA_GZ_OPT_PIECES over a piece table; returns (plan, results).  A piece is confirmed
    when it answers LA_ST_GZ_PIECE_END with consumed == src_len (or LA_ST_OK: its stream ends in it)."""
    plan = GzDevicePlan(ctx, d_src, pieces)
    plan.run(options | N.LA_GZ_OPT_PIECES)
    return plan, plan.results()


class BlockStartsRun:
    """what decode_block_starts returns: status, out_len, consumed_bits, crc32 of the confirmed chain; candidates found and
    pieces confirmed; boundary = the third result; out = the d_dst tensor (the packed bytes start at lead)"""


def decode_block_starts(ctx, d_src, src_off, src_len, dst_cap, start_bit=0, hist=b"", lead=32768 + 64, guard=0xA5, src_bytes=None,
                        options=None, expect_rc=0):
    """la_gpu_gzip_decode with LA_GZ_OPT_PIECES | LA_GZ_OPT_CHAIN | LA_GZ_OPT_BLOCK_STARTS over ONE span of d_src that starts
    on a true block boundary of a raw-deflate stream, at bit start_bit of its first byte.  hist: the stream's earlier output
    (at most 32 KiB), placed in front of the packed bytes.  The destination is lead + dst_cap + 64 bytes prefilled with
    `guard`.  Returns a BlockStartsRun, or None when the call was refused with expect_rc."""
    import ctypes as C
    import torch
    dev = d_src.device
    assert len(hist) <= lead
    mem = np.zeros(1, dtype=N.GZ_MEMBER_DTYPE)
    mem[0] = (src_off, src_len, min(dst_cap, 0xFFFFFFFF), lead)
    host_dst = np.full(lead + dst_cap + 64, guard, dtype=np.uint8)
    host_dst[lead - len(hist):lead] = np.frombuffer(hist, dtype=np.uint8)
    d_mem = torch.from_numpy(mem.view(np.uint8).reshape(-1).copy()).to(dev)
    d_dst = torch.from_numpy(host_dst).to(dev)
    d_res = torch.full((3 * N.GZ_RESULT_DTYPE.itemsize,), 0xEE, dtype=torch.uint8, device=dev)
    b = N._GzBatchC()
    b.d_src = d_src.data_ptr(); b.src_bytes = d_src.numel() if src_bytes is None else src_bytes
    b.d_members = d_mem.data_ptr(); b.n_members = 1
    b.d_dst = d_dst.data_ptr(); b.dst_cap = dst_cap
    b.d_results = d_res.data_ptr(); b.d_summary = None
    if options is None:
        options = N.LA_GZ_OPT_PIECES | N.LA_GZ_OPT_CHAIN | N.LA_GZ_OPT_BLOCK_STARTS
    b.options = options | (start_bit << N.LA_GZ_OPT_START_BIT_SHIFT)
    b.hist_len = len(hist)
    rc = N.gpu_lib().la_gpu_gzip_decode(ctx._h, C.byref(b))
    ctx.sync()
    assert rc == expect_rc, (rc, expect_rc)
    if rc != 0:
        assert bool((d_res == 0xEE).all()) and bool((d_dst.cpu() == torch.from_numpy(host_dst)).all()), "a refused call wrote something"
        return None
    res = d_res.cpu().numpy().view(N.GZ_RESULT_DTYPE)
    r = BlockStartsRun()
    r.status, r.out_len, r.consumed_bits, r.crc32 = (int(res[0][k]) for k in ("status", "out_len", "consumed", "crc32"))
    r.candidates, r.pieces = int(res[1]["out_len"]), int(res[1]["consumed"])
    # (status, out_len, consumed_bits, crc32) of the chain as far as it stands on a block boundary
    r.boundary = tuple(int(res[2][k]) for k in ("status", "out_len", "consumed", "crc32"))
    r.out, r.lead, r.dst_cap, r.hist, r.guard = d_dst, lead, dst_cap, hist, guard
    return r


def compress_to_members(ctx, d_plain, chunk_bytes=49152, mtime=0, options=0, framing=0):
    """Device gzip compression (la_gpu_gzip_compress): d_plain is a 1-D uint8 CUDA tensor; returns a uint8 CUDA
    tensor holding the concatenated gzip members (harness for the tests).  options: 0 fixed Huffman, 1 the smallest of
    dynamic Huffman, fixed Huffman and stored per chunk, 2 stored blocks only (LA_GZC_*).  framing: LA_GZC_FRAME_*
    (compress_to_stream asks for the other one)."""
    import torch
    n = int(d_plain.numel())
    cap = int(N.gpu_lib().la_gpu_gzip_compress_bound(n, chunk_bytes))
    d_out = torch.empty(max(cap, 16), dtype=torch.uint8, device=d_plain.device)
    d_len = torch.zeros(1, dtype=torch.int64, device=d_plain.device)
    b = N._GzcBatchC()
    b.d_src = d_plain.data_ptr() if n else None
    b.src_bytes = n
    b.chunk_bytes, b.mtime, b.options, b.framing = chunk_bytes, mtime, options, framing
    b.d_out, b.out_cap, b.d_out_bytes = d_out.data_ptr(), cap, d_len.data_ptr()
    ctx.gzip_compress(b)
    ctx.sync()
    total = int(d_len.cpu()[0])
    assert total <= cap, (total, cap)
    return d_out[:total]


def compress_to_stream(ctx, d_plain, chunk_bytes=49152, options=0):
    """The same call with LA_GZC_FRAME_STREAM: returns a uint8 CUDA tensor holding a byte-aligned piece of one
    raw-deflate stream, no block of it final (followed by 03 00 it inflates to d_plain)."""
    return compress_to_members(ctx, d_plain, chunk_bytes, 0, options, N.LA_GZC_FRAME_STREAM)
