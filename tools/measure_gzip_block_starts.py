"""ONE ordinary gzip member (what `gzip -6 file` writes: no flush point, no second header) through la_gpu_gzip_decode with
LA_GZ_OPT_BLOCK_STARTS, resident in HBM and verified against the plain bytes, beside zlib on one host core for the same
stream -- that number is the bar -- and the wave kernel (one wave, the only device path there was) on a 4 MiB cut.

    python tools/measure_gzip_block_starts.py [--mib 64] [--no-profile] [--no-cat]

Inputs: word text and the bench stream's kind of data (tests/streams.synth_lz4_stream's plain bytes), --mib MiB each, zlib
level 6.  Reports MiB/s decoded, candidates found and pieces confirmed, the time per stage from one
`rocprofv3 --kernel-trace --stats` run of its own (a child process that decodes each stream once, under a time limit), and
la_cat, file to bytes, with LA_GZIP_BLOCK_STARTS=1."""
import argparse
import csv
import glob
import os
import subprocess
import sys
import tempfile
import time
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import deflate_find_support as F  # noqa: E402

OPT_WAVE, OPT_RAW, OPT_PIECES, OPT_CHAIN, OPT_BLOCK_STARTS = 2, 16, 64, 128, 256
STAGES = (("find", ("find_quick", "find_write", "find_full", "find_pack")), ("measure", ("ELi1ELb1E", "<true, 1, true>")), ("walk", ("gz_walk",)),
          ("emit", ("ELi2ELb1E", "<true, 2, true>")), ("resolve", ("chain_jump", "chain_gather", "chain_total")), ("CRC32", ("gz_blocks_crc", "gz_blocks_fold")),
          ("scans", ("scan_tile", "scan_write")))


def inputs(mib):
    import streams as S
    n = mib << 20
    text = F.word_text(n, seed=41)
    frames = max(1, n // (16 * 65536))
    synth = S.synth_lz4_stream(0x4C413335, 0, frames, blocks_per_frame=16, block_size=65536, nthreads=8)[1].tobytes()[:n]
    return (("word text", text), ("bench-stream data", synth))


def device_decode(ctx, body, plain, reps):
    """la_gpu_gzip_decode with the block-start option over the resident body: (best seconds, candidates, pieces)"""
    import ctypes as C
    import torch
    from libarchive_amd import _native as N
    lead = 32768
    d_src = torch.from_numpy(np.frombuffer(body, dtype=np.uint8).copy()).cuda()
    want = torch.from_numpy(np.frombuffer(plain, dtype=np.uint8).copy()).cuda()
    mem = np.zeros(1, dtype=N.GZ_MEMBER_DTYPE)
    mem[0] = (0, len(body), len(plain), lead)
    d_mem = torch.from_numpy(mem.view(np.uint8).reshape(-1).copy()).cuda()
    d_dst = torch.zeros(lead + len(plain) + 64, dtype=torch.uint8, device="cuda")
    d_res = torch.zeros(3 * 16, dtype=torch.uint8, device="cuda")
    b = N._GzBatchC()
    b.d_src = d_src.data_ptr(); b.src_bytes = len(body)
    b.d_members = d_mem.data_ptr(); b.n_members = 1
    b.d_dst = d_dst.data_ptr(); b.dst_cap = len(plain)
    b.d_results = d_res.data_ptr(); b.d_summary = None
    b.options = OPT_PIECES | OPT_CHAIN | OPT_BLOCK_STARTS
    b.hist_len = 0
    best = None
    for rep in range(reps + 1):        # (the first call allocates the workspace)
        d_dst.zero_()
        ctx.sync(); t0 = time.perf_counter()
        rc = N.gpu_lib().la_gpu_gzip_decode(ctx._h, C.byref(b))
        ctx.sync(); dt = time.perf_counter() - t0
        assert rc == 0, rc
        res = d_res.cpu().numpy().view(N.GZ_RESULT_DTYPE)
        assert int(res[0]["status"]) == 0 and int(res[0]["out_len"]) == len(plain), res
        assert int(res[0]["crc32"]) == zlib.crc32(plain) & 0xFFFFFFFF
        assert torch.equal(d_dst[lead:lead + len(plain)], want)
        if rep:
            best = dt if best is None else min(best, dt)
    return best, int(res[1]["out_len"]), int(res[1]["consumed"])


def wave_decode(ctx, plain):
    """the wave kernel on its own: one member, one wave"""
    import torch
    from libarchive_amd import _native as N
    body = F.raw_deflate(plain, 6)
    d_src = torch.from_numpy(np.frombuffer(body + bytes(64), dtype=np.uint8).copy()).cuda()
    mem = np.zeros(1, dtype=N.GZ_MEMBER_DTYPE)
    mem[0] = (0, len(body), len(plain), 0)
    d_mem = torch.from_numpy(mem.view(np.uint8).reshape(-1).copy()).cuda()
    d_dst = torch.zeros(len(plain) + 64, dtype=torch.uint8, device="cuda")
    d_res = torch.zeros(16, dtype=torch.uint8, device="cuda")
    b = N._GzBatchC()
    b.d_src = d_src.data_ptr(); b.src_bytes = len(body)
    b.d_members = d_mem.data_ptr(); b.n_members = 1
    b.d_dst = d_dst.data_ptr(); b.dst_cap = len(plain)
    b.d_results = d_res.data_ptr(); b.d_summary = None
    b.options = OPT_WAVE | OPT_RAW
    ctx.gzip_decode(b); ctx.sync()
    t0 = time.perf_counter(); ctx.gzip_decode(b); ctx.sync(); dt = time.perf_counter() - t0
    res = d_res.cpu().numpy().view(N.GZ_RESULT_DTYPE)
    assert int(res[0]["status"]) == 0 and int(res[0]["crc32"]) == zlib.crc32(plain) & 0xFFFFFFFF
    return dt


def stage_times(mib):
    """one rocprofv3 run of a child that decodes each stream once; kernel time per stage, ms"""
    out = tempfile.mkdtemp(prefix="r22_prof_")
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", out, "--", sys.executable, os.path.abspath(__file__), "--child", "--mib", str(mib)]
    run = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    if run.returncode != 0:
        return "rocprofv3 run failed (exit %d): %s" % (run.returncode, run.stderr[-300:])
    files = glob.glob(os.path.join(out, "**", "*kernel_stats.csv"), recursive=True)
    if not files:
        return "rocprofv3 wrote no kernel_stats.csv, only " + ", ".join(sorted(os.path.basename(f) for f in glob.glob(os.path.join(out, "**", "*"), recursive=True)))
    ms = {name: 0.0 for name, _ in STAGES}
    other = 0.0
    for row in csv.DictReader(open(files[0])):
        t = float(row.get("TotalDurationNs") or 0) / 1e6
        for name, keys in STAGES:
            if any(k in row["Name"] for k in keys):
                ms[name] += t
                break
        else:
            other += t
    return ", ".join("%s %.1f ms" % (k, v) for k, v in ms.items()) + ", everything else (fills, compares) %.1f ms" % other


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mib", type=int, default=64)
    ap.add_argument("--child", action="store_true", help="decode each stream once and leave (what the profiler runs)")
    ap.add_argument("--no-profile", action="store_true")
    ap.add_argument("--no-cat", action="store_true")
    a = ap.parse_args()
    import libarchive_amd as la
    ctx = la.GpuContext(0)
    for name, plain in inputs(a.mib):
        body = F.raw_deflate(plain, 6)
        if a.child:
            device_decode(ctx, body, plain, 0)
            continue
        t0 = time.perf_counter(); got = zlib.decompress(body, -15); host = time.perf_counter() - t0
        assert got == plain
        dt, cands, pieces = device_decode(ctx, body, plain, 3)
        mibs = len(plain) / 2**20
        print("%s, %d MiB, level 6, %d bytes compressed: device %.1f ms = %.0f MiB/s (candidates %d, pieces %d); zlib on one host core "
              "%.1f ms = %.0f MiB/s; device / host %.2f" % (name, a.mib, len(body), dt * 1e3, mibs / dt, cands, pieces, host * 1e3, mibs / host,
                                                            host / dt), flush=True)
        cut = plain[:4 << 20]
        wt = wave_decode(ctx, cut)
        print("  the wave kernel alone on the first 4 MiB: %.1f ms = %.1f MiB/s" % (wt * 1e3, len(cut) / 2**20 / wt), flush=True)
        if not a.no_cat:
            with tempfile.NamedTemporaryFile(suffix=".gz") as f:
                f.write(F.gz_member(body, plain)); f.flush()
                env = {k: v for k, v in os.environ.items() if k != "LA_GPU_BID"}
                env["LA_GZIP_BLOCK_STARTS"] = "1"
                t0 = time.perf_counter()
                run = subprocess.run([os.path.join(ROOT, "libarchive_amd", "host", "la_cat"), f.name], capture_output=True, env=env, timeout=300)
                ct = time.perf_counter() - t0
                assert run.returncode == 0 and run.stdout == plain, run.stderr[-300:]
                print("  la_cat, file to bytes, LA_GZIP_BLOCK_STARTS=1: %.0f ms = %.0f MiB/s (process start and device open included)"
                      % (ct * 1e3, mibs / ct), flush=True)
    ctx.close()
    if not a.child and not a.no_profile:
        print("kernel time per stage, both streams decoded once each (rocprofv3 --kernel-trace --stats): " + stage_times(a.mib), flush=True)


if __name__ == "__main__":
    main()
