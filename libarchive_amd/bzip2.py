"""Device-resident bzip2 decode and compression through the C ABI (harness for tests / tools).  Plumbing only: torch
allocates the HBM buffers; the candidate table comes from la_gpu_bzip2_scan, all work is la_gpu_bzip2_decode() in its two
phases and la_gpu_bzip2_compress()."""
import ctypes as C

import numpy as np

from . import _native as N

BZ2_CAND_DTYPE, BZ2_RESULT_DTYPE, BZ2_STATE_DTYPE = N.BZ2_CAND_DTYPE, N.BZ2_RESULT_DTYPE, N.BZ2_STATE_DTYPE
LA_BZ2_OPT_SERIAL_CHASE = N.LA_BZ2_OPT_SERIAL_CHASE
LA_ST_BZ2_DATA, LA_ST_BZ2_TRUNCATED, LA_ST_BZ2_BAD_CRC = N.LA_ST_BZ2_DATA, N.LA_ST_BZ2_TRUNCATED, N.LA_ST_BZ2_BAD_CRC
LA_ST_BZ2_REFUTED, LA_ST_BZ2_RANDOMISED = N.LA_ST_BZ2_REFUTED, N.LA_ST_BZ2_RANDOMISED
LA_BZ2C_FIRST, LA_BZ2C_LAST, BZ2C_STATE_DTYPE = N.LA_BZ2C_FIRST, N.LA_BZ2C_LAST, N.BZ2C_STATE_DTYPE


def compress_block_bytes(level):
    return int(N.gpu_lib().la_gpu_bzip2_compress_block_bytes(level))


def compress_bound(n, level):
    return int(N.gpu_lib().la_gpu_bzip2_compress_bound(n, level))


def compress_to_stream(ctx, d_plain, level=9, flags=N.LA_BZ2C_FIRST | N.LA_BZ2C_LAST, state=None, out_cap=None, d_out=None):
    """Device bzip2 compression (la_gpu_bzip2_compress): d_plain is a 1-D uint8 CUDA tensor; returns a uint8 CUDA tensor
    holding the stream, or the piece of it this call wrote.  `state` is the 16-byte device tensor (la_bz2c_state) a
    stream written in several calls carries from one to the next; without one the call uses its own.  With `out_cap`
    (and optionally `d_out`) the call gets that much room only and the needed size is returned beside the tensor."""
    import torch
    n = int(d_plain.numel())
    dev = d_plain.device
    cap = compress_bound(n, level) if out_cap is None else int(out_cap)
    if d_out is None:
        d_out = torch.empty(max(cap, 16), dtype=torch.uint8, device=dev)
    d_len = torch.zeros(1, dtype=torch.int64, device=dev)
    if state is None:
        state = torch.zeros(16, dtype=torch.uint8, device=dev)
    b = N._Bz2cBatchC()
    b.d_src = d_plain.data_ptr() if n else None
    b.src_bytes = n
    b.level, b.flags = level, flags
    b.d_state = state.data_ptr()
    b.d_out, b.out_cap, b.d_out_bytes = d_out.data_ptr(), cap, d_len.data_ptr()
    ctx.bzip2_compress(b)
    ctx.sync()
    total = int(d_len.cpu()[0])
    if out_cap is not None:
        return d_out, total
    assert total <= cap, (total, cap)
    return d_out[:total]


def max_blocks(slot_level):
    return int(N.gpu_lib().la_gpu_bzip2_max_blocks(slot_level))


def scan(ctx, d_src, cap=1 << 16):
    """Candidate table (ndarray of BZ2_CAND_DTYPE, ascending bit_off) of a 1-D uint8 device tensor."""
    import torch
    d_cands = torch.zeros(max(cap, 1) * BZ2_CAND_DTYPE.itemsize, dtype=torch.uint8, device=d_src.device)
    d_count = torch.zeros(1, dtype=torch.int32, device=d_src.device)
    ctx.bzip2_scan(d_src.data_ptr() if d_src.numel() else None, d_src.numel(), d_cands.data_ptr(), cap, d_count.data_ptr())
    ctx.sync()
    n = int(d_count.cpu()[0]) & 0xFFFFFFFF
    if n > cap:
        return scan(ctx, d_src, n)
    return d_cands.cpu().numpy().view(BZ2_CAND_DTYPE)[:n].copy()


class Bz2DevicePlan:
    """One window: measure(), then emit(); results() / state() read back what the last phase wrote."""

    def __init__(self, ctx, d_src, cands, slot_level=9, options=0, state=None):
        import torch
        dev = d_src.device
        self.ctx, self.n, self.d_src = ctx, len(cands), d_src
        self.d_cands = torch.from_numpy(np.ascontiguousarray(cands).view(np.uint8).reshape(-1).copy()).to(dev) if self.n else \
            torch.zeros(16, dtype=torch.uint8, device=dev)
        self.d_results = torch.zeros(max(self.n, 1) * BZ2_RESULT_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        self.d_state = torch.zeros(BZ2_STATE_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        self.d_dst = None
        self.state_in = N._Bz2StateC()
        if state is not None:
            self.state_in.open, self.state_in.level = int(state["open"]), int(state["level"])
            self.state_in.crc, self.state_in.start_bit = int(state["crc"]), int(state["start_bit"])
        b = N._Bz2BatchC()
        b.d_src, b.src_bytes = (d_src.data_ptr() if d_src.numel() else None), d_src.numel()
        b.d_cands, b.n = self.d_cands.data_ptr(), self.n
        b.d_results, b.d_state_out = self.d_results.data_ptr(), self.d_state.data_ptr()
        b.state_in = C.pointer(self.state_in)
        b.options, b.slot_level = options, slot_level
        self.batch = b

    def measure(self):
        self.batch.phase = N.LA_BZ2_MEASURE
        self.ctx.bzip2_decode(self.batch)
        return self.state()

    def emit(self, n_emit=None, dst_cap=None, d_dst=None):
        """`d_dst`: the caller's destination (a 1-D uint8 tensor of at least dst_cap bytes, a view at any offset) instead
        of one of the plan's own"""
        import torch
        st = self.state()
        if dst_cap is None:
            dst_cap = int(st["total_out"])
        self.d_dst = d_dst if d_dst is not None else torch.empty(max(int(dst_cap), 16), dtype=torch.uint8, device=self.d_src.device)
        assert self.d_dst.numel() >= int(dst_cap)
        self.batch.phase = N.LA_BZ2_EMIT
        self.batch.d_dst, self.batch.dst_cap = self.d_dst.data_ptr(), int(dst_cap)
        self.batch.n_emit = self.n if n_emit is None else n_emit
        self.ctx.bzip2_decode(self.batch)
        return self.state()

    def results(self):
        self.ctx.sync()
        return self.d_results.cpu().numpy().view(BZ2_RESULT_DTYPE)[:self.n].copy()

    def state(self):
        self.ctx.sync()
        return self.d_state.cpu().numpy().view(BZ2_STATE_DTYPE)[0].copy()

    def output(self):
        self.ctx.sync()
        n = int(self.state()["total_out"])
        return self.d_dst[:n].cpu().numpy().tobytes()


def decode_image(ctx, image, slot_level=9, options=0, cands=None):
    """Scan + measure + emit of a whole host image in one window.  Returns (bytes, results, state after emit, plan)."""
    import torch
    buf = np.frombuffer(bytes(image), dtype=np.uint8)
    d_src = torch.from_numpy(buf.copy()).cuda() if buf.size else torch.zeros(0, dtype=torch.uint8, device="cuda")
    if cands is None:
        cands = scan(ctx, d_src)
    plan = Bz2DevicePlan(ctx, d_src, cands, slot_level=slot_level, options=options)
    plan.measure()
    st = plan.emit()
    return plan.output(), plan.results(), st, plan
