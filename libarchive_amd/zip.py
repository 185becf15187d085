"""Device ZIP entry compression through the C ABI (harness for the tests and tools/measure_zip_write.py).
Plumbing only: torch allocates the HBM buffers; all work is la_gpu_zip_compress()."""
import numpy as np

from . import _native as N


def seg_table(segs):
    """[(offset, length, seed, (gap_before, gap_after), flags), ...] as an array of la_zipc_seg"""
    t = np.zeros(len(segs), dtype=N.ZIPC_SEG_DTYPE)
    for i, (off, length, seed, gaps, flags) in enumerate(segs):
        t[i] = (off, length, seed, gaps[0], gaps[1], flags, 0)
    return t


def compress_segments(ctx, d_src, segs, chunk_bytes=49152, options=0, out_cap=None, fill=0xA5, reserved=0, alloc=0):
    """la_gpu_zip_compress over d_src (a 1-D uint8 CUDA tensor).  `segs` is a list of (offset, length, seed, (gap_before,
    gap_after), flags) or an array of la_zipc_seg.  d_out is prefilled with `fill` and is out_cap long (default: the
    bound) inside a buffer of at least `alloc` bytes.  Returns (rc, out, results, total): rc LA_OK or LA_ERR_ARG, `out` the WHOLE d_out buffer as bytes (gaps and
    the bytes beyond `total` keep the fill), results an array of la_zipc_result (None unless LA_OK), total
    *d_out_bytes (likewise)."""
    import torch
    t = segs if isinstance(segs, np.ndarray) else seg_table(segs)
    n, dev = len(t), d_src.device
    gaps = int(t["gap_before"].astype(np.uint64).sum() + t["gap_after"].astype(np.uint64).sum())
    bound = int(N.gpu_lib().la_gpu_zip_compress_bound(int(d_src.numel()), n, chunk_bytes, gaps))
    cap = bound if out_cap is None else int(out_cap)
    d_out = torch.full((max(cap, alloc, 16),), fill, dtype=torch.uint8, device=dev)
    d_segs = torch.from_numpy(t.view(np.uint8).reshape(-1).copy()).to(dev) if n else None
    d_res = torch.zeros(max(n, 1) * N.ZIPC_RESULT_DTYPE.itemsize, dtype=torch.uint8, device=dev)
    d_len = torch.full((1,), -1, dtype=torch.int64, device=dev)
    b = N._ZipcBatchC()
    b.d_src = d_src.data_ptr() if d_src.numel() else None
    b.src_bytes = int(d_src.numel())
    b.d_segs = d_segs.data_ptr() if n else None
    b.n_segs, b.chunk_bytes, b.options, b.reserved = n, chunk_bytes, options, reserved
    b.d_out, b.out_cap, b.d_results, b.d_out_bytes = d_out.data_ptr(), cap, d_res.data_ptr(), d_len.data_ptr()
    rc = ctx.zip_compress(b)
    ctx.sync()
    out = d_out.cpu().numpy().tobytes()
    if rc != N.LA_OK:
        assert int(d_len.cpu()[0]) == -1, "an argument error left *d_out_bytes alone"
        return rc, out, None, None
    return rc, out, d_res.cpu().numpy().view(N.ZIPC_RESULT_DTYPE)[:n].copy(), int(d_len.cpu()[0])
