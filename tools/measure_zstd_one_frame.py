"""ONE Zstandard frame (what `zstd file` writes) through la_gpu_zstd_decode: by the frame kernel (options 0, the whole
frame on one wave) and by the block path (LA_ZSTD_OPT_BLOCK_PARALLEL), alternating in one process on the same frame,
with and without the content checksum's verification.  Prints both rates per shape; asserts that both paths give the
plain bytes and that the block path finished the frame (path == 1).

    python tools/measure_zstd_one_frame.py [--sizes 16,256] [--levels 3,19] [--cache DIR] [--only-blocks]

--cache DIR keeps the compressed images (level 19 of 256 MiB takes minutes on a host core)."""
import argparse
import os
import random
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import zstd_support as Z  # noqa: E402

OPT_NO_VERIFY, OPT_BLOCKS = 1, 4


def plain_bytes(mib):
    rnd = random.Random(2)
    unit = b"".join(Z.gen(rnd, 65536, 2 if i % 2 else 4) for i in range(64)) * 4      # 16 MiB: words and LZ-shaped copies
    return unit * (mib // 16) if mib >= 16 else unit[:mib << 20]


def image(z, d, mib, level, cache):
    """one frame with a content checksum (the zstd tool's default), by libzstd's streaming-free advanced API"""
    path = os.path.join(cache, "one_frame_%d_l%d.zst" % (mib, level)) if cache else None
    if path and os.path.exists(path):
        return open(path, "rb").read()
    import ctypes
    z.ZSTD_createCCtx.restype = ctypes.c_void_p
    z.ZSTD_CCtx_setParameter.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int]
    z.ZSTD_compress2.restype = ctypes.c_size_t
    z.ZSTD_compress2.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_char_p, ctypes.c_size_t]
    z.ZSTD_freeCCtx.argtypes = [ctypes.c_void_p]
    cctx = z.ZSTD_createCCtx()
    z.ZSTD_CCtx_setParameter(cctx, 100, level)      # ZSTD_c_compressionLevel
    z.ZSTD_CCtx_setParameter(cctx, 201, 1)          # ZSTD_c_checksumFlag
    cap = z.ZSTD_compressBound(len(d))
    buf = ctypes.create_string_buffer(cap)
    n = z.ZSTD_compress2(cctx, buf, cap, d, len(d))
    assert not z.ZSTD_isError(n)
    z.ZSTD_freeCCtx(cctx)
    img = buf.raw[:n]
    if path:
        os.makedirs(cache, exist_ok=True)
        open(path, "wb").write(img)
    return img


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="16,256")
    ap.add_argument("--levels", default="3,19")
    ap.add_argument("--cache", default=None)
    ap.add_argument("--compress-only", action="store_true", help="fill the cache and stop (needs no GPU)")
    ap.add_argument("--only-blocks", action="store_true", help="time the block path alone (for a profiler run)")
    a = ap.parse_args()
    z = Z.libzstd()
    assert z is not None, "libzstd.so.1 makes the frames"
    shapes = []
    for mib in (int(x) for x in a.sizes.split(",")):
        d = plain_bytes(mib)
        for level in (int(x) for x in a.levels.split(",")):
            t0 = time.time()
            img = image(z, d, mib, level, a.cache)
            print("# %d MiB level %d: %d bytes compressed (%.1f s)" % (mib, level, len(img), time.time() - t0), flush=True)
            shapes.append((mib, level, img))
        if a.compress_only:
            continue
        import torch
        import libarchive_amd as la
        from libarchive_amd import zstd as LZ
        ctx = la.GpuContext(0)
        want = torch.from_numpy(np.frombuffer(d, dtype=np.uint8).copy()).cuda()
        for mib_, level, img in [s for s in shapes if s[0] == mib]:
            frames, end_kind, consumed, dst_bytes = LZ.index_image(img)
            assert len(frames) == 1 and consumed == len(img)
            d_src = torch.from_numpy(np.frombuffer(img, dtype=np.uint8).copy()).cuda()
            plan = LZ.ZstdDevicePlan(ctx, d_src, frames, dst_bytes)

            def timed(opt, check_path):
                plan.d_dst.zero_()
                ctx.sync(); t0 = time.perf_counter(); plan.run(opt); ctx.sync(); dt = time.perf_counter() - t0
                res = plan.results()
                assert int(res["status"][0]) == 0 and int(res["out_len"][0]) == len(d), (opt, res)
                assert int(res["path"][0]) == check_path, (opt, res)
                assert torch.equal(plan.d_dst[:len(d)], want), opt
                return dt

            for nv in (0, OPT_NO_VERIFY):
                timed(OPT_BLOCKS | nv, 1)       # (first call: workspace allocation)
                t4, t0_ = [], []
                for rep in range(3):
                    t4.append(timed(OPT_BLOCKS | nv, 1))
                    if not a.only_blocks and (rep == 0 or mib <= 64):    # (the frame kernel takes seconds on the large frame)
                        t0_.append(timed(nv, 0))
                r4 = len(d) / min(t4) / 2**20
                line = "ONE zstd frame of %d MiB, level %d, %s: block path %.1f ms = %.1f MiB/s" % (
                    mib, level, "checksum not verified" if nv else "checksum verified", min(t4) * 1e3, r4)
                if t0_:
                    r0 = len(d) / min(t0_) / 2**20
                    line += "; frame kernel (one wave) %.1f ms = %.1f MiB/s; ratio %.1f" % (min(t0_) * 1e3, r0, r4 / r0)
                print(line, flush=True)
            del plan
        ctx.close()


if __name__ == "__main__":
    main()
