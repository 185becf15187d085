"""Device-resident uuencode / base64 line decode through the C ABI (harness for tests / tools).  Plumbing only: torch
allocates the HBM buffers; all work is la_gpu_uu_decode(): one window of text in, the decoded bytes and one result
record out, the two-word state carried by the caller from window to window."""
import numpy as np

from . import _native as N

UU_RESULT_DTYPE = N.UU_RESULT_DTYPE
FIND_HEAD, READ_UU, UUEND, READ_BASE64, STOP = N.LA_UU_FIND_HEAD, N.LA_UU_READ_UU, N.LA_UU_UUEND, N.LA_UU_READ_BASE64, N.LA_UU_STOP
STATUS = {0: "OK", N.LA_ST_UU_IGNORED: "IGNORED", N.LA_ST_UU_BAD_BYTE_HEAD: "BAD_BYTE_HEAD", N.LA_ST_UU_BAD_BYTE: "BAD_BYTE",
          N.LA_ST_UU_BAD_LINE: "BAD_LINE", N.LA_ST_UU_BAD_END: "BAD_END", N.LA_ST_UU_TOO_LONG: "TOO_LONG",
          N.LA_ST_UU_UNTERMINATED: "UNTERMINATED"}


def workspace_bytes(n):
    return int(N.gpu_lib().la_gpu_uu_workspace_bytes(n))


def to_device(image):
    import torch
    buf = np.frombuffer(bytes(image), dtype=np.uint8)
    return torch.from_numpy(buf.copy()).cuda() if buf.size else torch.zeros(0, dtype=torch.uint8, device="cuda")


class UuDevicePlan:
    """One window on the device: run(state, decoded, final) decodes it; result() / output() read back.  The buffers are
    kept, so one plan serves many calls over the same text (tools/measure_uu.py)."""

    def __init__(self, ctx, d_src, d_dst=None):
        import torch
        self.ctx, self.d_src, self.n = ctx, d_src, int(d_src.numel())
        self.d_dst = d_dst if d_dst is not None else torch.zeros(max(self.n, 16), dtype=torch.uint8, device=d_src.device)
        self.d_result = torch.zeros(UU_RESULT_DTYPE.itemsize, dtype=torch.uint8, device=d_src.device)
        torch.cuda.synchronize(d_src.device)    # the context's stream does not wait for torch's

    def run(self, state=FIND_HEAD, decoded=False, final=True):
        b = N._UuBatchC()
        b.d_src, b.src_bytes = (self.d_src.data_ptr() if self.n else None), self.n
        b.final, b.reserved = 1 if final else 0, 0
        b.state_in.state, b.state_in.decoded = state, 1 if decoded else 0
        b.d_dst, b.dst_cap, b.d_result = self.d_dst.data_ptr(), int(self.d_dst.numel()), self.d_result.data_ptr()
        self.ctx.uu_decode(b)
        return self

    def result(self):
        self.ctx.sync()
        return self.d_result.cpu().numpy().view(UU_RESULT_DTYPE)[0].copy()

    def output(self, n):
        self.ctx.sync()
        return self.d_dst[:int(n)].cpu().numpy().tobytes()


def decode_window(ctx, image, state=FIND_HEAD, decoded=False, final=True):
    """Upload a host image and decode it as one window.  Returns (result record, decoded bytes)."""
    plan = UuDevicePlan(ctx, to_device(image)).run(state, decoded, final)
    r = plan.result()
    return r, plan.output(r["out_len"])
