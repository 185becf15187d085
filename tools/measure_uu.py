"""uu read side on the device: la_gpu_uu_decode over uuencode (`M` lines) and base64 (76-character lines) text resident in
HBM, the split per phase from la_gpu_profile_read, beside la_gpu_memcpy_d2d of the same source bytes in the same run
(the ceiling) and libarchive_amd/csrc/la_uu_dev.h walked line by line at -O2 on ONE host core (tests/mock_gpu/
uu_rules_bench; the project's own rules header, not the reference's filter).

    python tools/measure_uu.py [--mib 1024] [--window 256] [--reps 3] [--host-mib 64] [--out FILE]

`mib` MiB of decoded data per encoding: one section whose body is a unit of 1 MiB of random bytes, encoded once on the
host and tiled in HBM.  The entry takes at most LA_UU_MAX_SRC_BYTES per call and its line table is sized for a window of
line ends alone (12 bytes per source byte), so the text is handed over in windows of `window` MiB cut at line
boundaries, the two-word state carried from call to call as the filter does; the times of a pass are the sums over its
calls.  One warm-up pass, then `reps` passes timed with events on the context's stream: the median is reported.  The
first and the last unit of the output are compared with the plain bytes on the device."""
import argparse
import base64
import ctypes as C
import os
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

UNIT = 45 * 57 * 416     # bytes of a unit: whole lines in both encodings, a multiple of 16, about 1 MiB


def encodings(plain):
    import uu_support as U
    uu_lines = b"".join(U.uu_line(plain[i:i + 45]) for i in range(0, len(plain), 45))
    b64_lines = b"".join(base64.b64encode(plain[i:i + 57]) + b"\n" for i in range(0, len(plain), 57))
    return (("uuencode, M lines", b"begin 644 measure.bin\n", uu_lines, b"`\nend\n"),
            ("base64, 76-character lines", b"begin-base64 644 measure.bin\n", b64_lines, b"====\n"))


def host_baseline(tmp, image, reps):
    import uu_mock_build as mock_build
    exe = mock_build.program("uu_rules_bench")
    path = os.path.join(tmp, "text.uu")
    with open(path, "wb") as f:
        f.write(image)
    out = subprocess.check_output([exe, path, str(reps)], text=True).split()
    return int(out[0]), float(out[1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mib", type=int, default=1024)
    ap.add_argument("--window", type=int, default=256)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--host-mib", type=int, default=64)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    import torch
    import libarchive_amd as la
    from libarchive_amd import uu
    import uu_support as U
    say("# tools/measure_uu.py --mib %d --window %d --reps %d --host-mib %d" % (args.mib, args.window, args.reps, args.host_mib))
    tiles = max((args.mib << 20) // UNIT, 1)
    plain = U.randbytes(30, UNIT)
    tmp = tempfile.mkdtemp(prefix="measure_uu")
    lib = la.gpu_lib()
    lib.la_gpu_memcpy_d2d.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64]
    for name, head, unit, trailer in encodings(plain):
        host_tiles = max((args.host_mib << 20) // UNIT, 1)
        nbytes, secs = host_baseline(tmp, head + unit * host_tiles + trailer, 3)
        total_out = tiles * UNIT
        ctx = la.GpuContext(0)
        ctx.set_stream(torch.cuda.current_stream().cuda_stream)
        as_dev = lambda b: torch.from_numpy(np.frombuffer(b, dtype=np.uint8).copy()).cuda()      # noqa: E731
        d_src = torch.cat([as_dev(head), as_dev(unit).repeat(tiles), as_dev(trailer)])
        d_plain = as_dev(plain)
        n = int(d_src.numel())
        d_dst = torch.zeros(n + 64, dtype=torch.uint8, device="cuda")      # (a call wants as much room as it has text)
        per = max((args.window << 20) // len(unit), 1)      # units per window
        cuts = [0] + [len(head) + k * len(unit) for k in range(per, tiles, per)] + [n]
        say("%s: %d MiB decoded, %.1f MiB of text in %d lines, %d windows of at most %d MiB; la_uu_dev.h -O2 on one host core: "
            "%.0f MiB/s decoded (%d MiB)" % (name, total_out >> 20, n / 2 ** 20, tiles * unit.count(b"\n") + 3, len(cuts) - 1, args.window,
                                             nbytes / 2 ** 20 / secs, nbytes >> 20))
        ctx.profile_enable(True)
        torch.cuda.synchronize()
        times, phases = [], []
        for rep in range(args.reps + 1):    # the first pass warms the workspace and the code objects
            state, decoded, out_at, t_ms, ph = uu.FIND_HEAD, False, 0, 0.0, {}
            for a, b in zip(cuts[:-1], cuts[1:]):
                plan = uu.UuDevicePlan(ctx, d_src[a:b], d_dst[out_at:])
                ctx.timer_start()
                plan.run(state, decoded, final=(b == n))
                t_ms += ctx.timer_stop()
                for k, v in ctx.profile_read():
                    ph[k] = ph.get(k, 0.0) + v
                r = plan.result()
                assert int(r["status"]) == 0 and int(r["consumed"]) == b - a, (int(r["status"]), int(r["consumed"]), b - a)
                state, decoded, out_at = int(r["state"]), bool(r["decoded"]), out_at + int(r["out_len"])
            assert out_at == total_out and state == uu.FIND_HEAD, (out_at, total_out, state)
            if rep:
                times.append(t_ms)
                phases.append(ph)
        assert torch.equal(d_dst[:UNIT], d_plain) and torch.equal(d_dst[total_out - UNIT:total_out], d_plain)
        med = statistics.median(times)
        say("  la_gpu_uu_decode, text resident in HBM: median of %d passes %.2f ms (min %.2f, max %.2f) = %.1f GiB/s decoded, %.1f GiB/s of text"
            % (len(times), med, min(times), max(times), total_out / 2 ** 30 / (med / 1e3), n / 2 ** 30 / (med / 1e3)))
        say("  per phase (median): " + ", ".join("%s %.2f ms" % (k, statistics.median(p[k] for p in phases)) for k in phases[0]))
        d_copy = torch.zeros(n, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        times = []
        for rep in range(args.reps + 1):
            ctx.timer_start()
            assert lib.la_gpu_memcpy_d2d(ctx._h, d_copy.data_ptr(), d_src.data_ptr(), n) == 0
            t_ms = ctx.timer_stop()
            if rep:
                times.append(t_ms)
        cp = statistics.median(times)
        say("  la_gpu_memcpy_d2d of the same %.1f MiB of text: median %.2f ms = %.1f GiB/s read and as much written; the decode takes %.1f x as long"
            % (n / 2 ** 20, cp, n / 2 ** 30 / (cp / 1e3), med / cp))
        ctx.close()
        del d_src, d_dst, d_copy, d_plain
        torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
