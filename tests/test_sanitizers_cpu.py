"""ASan + UBSan over the CPU-side C code (sanitizers are CPU-only on this pool): the oracle and
the host walkers are rebuilt with -fsanitize=address,undefined and driven over the reference
fixtures, the behaviour-table streams and a batch of mutated streams in a child process."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

DRIVER = r'''
import ctypes as C, glob, os, random, sys
sys.path.insert(0, os.path.join(ROOT, "tests")); sys.path.insert(0, ROOT)
import numpy as np
orc = C.CDLL(os.path.join(ROOT, "oracle", "liblaoracle_asan.so"))
walk = C.CDLL(os.path.join(ROOT, "libarchive_amd", "host", "libla_walkers_asan.so"))
import oracle_lib as O
O._lib = None; O._LIB_PATH = os.path.join(ROOT, "oracle", "liblaoracle_asan.so")
import streams as S

class LzIdx(C.Structure):
    _fields_ = [("blocks", C.c_void_p), ("n_blocks", C.c_uint32), ("cap_blocks", C.c_uint32), ("frames", C.c_void_p),
                ("n_frames", C.c_uint32), ("cap_frames", C.c_uint32), ("end_kind", C.c_int), ("consumed", C.c_uint64), ("max_out", C.c_uint64)]
class GzIdx(C.Structure):
    _fields_ = [("members", C.c_void_p), ("headers", C.c_void_p), ("n", C.c_uint32), ("cap", C.c_uint32),
                ("end_kind", C.c_int), ("consumed", C.c_uint64), ("max_out", C.c_uint64), ("speculative", C.c_int)]
walk.la_lz4_index_build.argtypes = [C.c_char_p, C.c_uint64, C.c_int, C.POINTER(LzIdx)]
walk.la_gz_index_build.argtypes = [C.c_char_p, C.c_uint64, C.c_int, C.POINTER(GzIdx)]

def run(img):
    img = bytes(img)
    for at_eof in (0, 1):
        x = LzIdx(); walk.la_lz4_index_build(img, len(img), at_eof, C.byref(x)); walk.la_lz4_index_free(C.byref(x))
        g = GzIdx(); walk.la_gz_index_build(img, len(img), at_eof, C.byref(g)); walk.la_gz_index_free(C.byref(g))
    O.lz4_stream_decode(img, 1 << 23); O.gzip_stream_decode(img, 1 << 23)

n = 0
for f in [g for g in glob.glob(os.path.join(ROOT, "tests", "golden", "ref_fixtures", "*")) if os.path.isfile(g)]:
    if not f.endswith(".json"):
        run(open(f, "rb").read()); n += 1
for img, *_ in S.appendix_d_lz4_cases().values():
    run(img); n += 1
rnd = random.Random(1)
base, _ = S.synth_lz4_stream(9, 0, 2, blocks_per_frame=3, block_size=2048, nthreads=1)
gz = S.gz_member(os.urandom(2000) + b"abc" * 2000, name=b"n") + S.gz_member(b"x" * 5000)
for seed in (base.tobytes(), gz):
    for t in range(300):
        m = bytearray(seed)
        for _ in range(rnd.randint(1, 4)):
            m[rnd.randrange(len(m))] = rnd.getrandbits(8)
        if rnd.random() < 0.3:
            m = m[:rnd.randrange(1, len(m))]
        run(m); n += 1
print("sanitized runs:", n)
'''


def test_oracle_and_walkers_under_asan_ubsan(tmp_path):
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "oracle"), "liblaoracle_asan.so"])
    host = os.path.join(ROOT, "libarchive_amd", "host")
    subprocess.check_call(["gcc", "-O1", "-g", "-fPIC", "-std=gnu11", "-fsanitize=address,undefined", "-fno-omit-frame-pointer",
                           "-I" + os.path.join(ROOT, "include"), "-shared", "-o", os.path.join(host, "libla_walkers_asan.so"),
                           os.path.join(host, "la_lz4_index.c"), os.path.join(host, "la_gzip_index.c")])
    libasan = subprocess.check_output(["gcc", "-print-file-name=libasan.so"]).decode().strip()
    env = dict(os.environ, LD_PRELOAD=libasan, ASAN_OPTIONS="detect_leaks=0:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1")
    script = tmp_path / "drv.py"
    script.write_text("ROOT = %r\n" % ROOT + DRIVER)
    out = subprocess.run([sys.executable, str(script)], env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    assert "sanitized runs:" in out.stdout


FILTER_DRIVER = r'''
import ctypes as C, io, os, random, sys, tarfile
sys.path.insert(0, os.path.join(ROOT, "tests")); sys.path.insert(0, ROOT)
os.environ["LA_GPU_BATCH_MIB"] = "1"
import la_api
la_api.use_library(C.CDLL(os.path.join(ROOT, "tests", "mock_gpu", "libla_host_mock_asan.so")))
import streams as S
from test_gpu_filters import _dependent_frame
from test_gpu_tar import _make_tar, _gz_members, _lz4_frames

rnd = random.Random(77)
n = 0
def mutations(img, k):
    yield img
    for _ in range(k):
        m = bytearray(img)
        for _ in range(rnd.randint(1, 3)):
            m[rnd.randrange(len(m))] = rnd.getrandbits(8)
        if rnd.random() < 0.3:
            m = m[:rnd.randrange(1, len(m))]
        yield bytes(m)

tar, _ = _make_tar(random.Random(3), 25, sizes=[0, 1, 511, 513, 3000, 70000])
for img in (tar, _gz_members(tar), _lz4_frames(tar)):
    for m in mutations(img, 25):
        la_api.list_entries(m, read_size=rnd.choice([None, 512, 4096]), skip_every=rnd.choice([0, 2]))
        la_api.cat(m, read_size=rnd.choice([None, 1000]))
        n += 2
# lz4 write filter: windows, pieces, options, a client buffer that is too small
import test_gpu_lz4_write as W
W._lib = lambda _l=C.CDLL(os.path.join(ROOT, "tests", "mock_gpu", "libla_host_mock_asan.so")): W._lib_setup(_l)
os.environ["LA_GPU_WRITE_WINDOW_MIB"] = "1"
for size in (0, 1, 65535, 65536, 1 << 20, (1 << 20) + 1, 3 * (1 << 20) + 12345):
    data = bytes(rnd.getrandbits(8) for _ in range(min(size, 4096))) * (size // 4096 + 1)
    data = data[:size]
    for opts in ((), (("block-checksum", "1"),), (("stream-checksum", None),)):
        rc, img = W.write_lz4(data, opts, rnd.choice([None, 1000, 70000]))
        assert rc == 0
        r = la_api.cat(img)
        assert r.data == data, (size, opts)
        n += 1
    rc, err = W.write_lz4(data, (), None, cap=max(1, size // 2))
    n += 1
# zstd write filter on the same window: frame sizes, pieces, the empty stream
import test_gpu_zstd_write as ZW
for size in (0, 1, 131072, (1 << 20) + 1, 3 * (1 << 20) + 12345):
    data = bytes(rnd.getrandbits(8) for _ in range(min(size, 4096))) * (size // 4096 + 1)
    data = data[:size]
    for opts in ((), (("max-frame-in", "64k"),), (("max-frame-in", "1M"),)):
        rc, img = ZW.write_zstd(data, opts, rnd.choice([None, 1000, 70000]))
        assert rc == 0
        assert la_api.cat(img).data == data, (size, opts)
        n += 1
# zstd filter and frame walker: mutated / truncated multi-frame streams (frame headers, block headers, skippable frames)
import zstd_support as Z
zz = Z.libzstd()
if zz is not None:
    parts = []
    for i in range(40):
        parts.append(Z.zstd_compress(zz, Z.gen(rnd, rnd.choice([0, 10, 3000, 140000]), rnd.randint(1, 4)), rnd.choice([1, 3, 19])))
        if i % 7 == 3:
            parts.append(Z.skippable(b"k" * i, i % 16))
    zimg = b"".join(parts)
    for m in mutations(zimg, 400):
        la_api.cat(m, read_size=rnd.choice([None, 7, 1000])); n += 1
    for pos in range(0, 40):
        for v in (0, 1, 0x7f, 0x80, 0xff):
            m = bytearray(zimg); m[pos] = v
            la_api.cat(bytes(m)); n += 1
# ZIP reader: mutated archives (directory records, local headers, bodies, end record) must fail cleanly
from test_gpu_zip import _make_zip
import zipfile
zimg = _make_zip([("d/", b"", zipfile.ZIP_STORED, None)] +
                 [("d/f%d" % i, bytes(rnd.getrandbits(8) for _ in range(rnd.choice([0, 5, 900]))) * rnd.choice([1, 40]),
                   rnd.choice([zipfile.ZIP_STORED, zipfile.ZIP_DEFLATED]), 6) for i in range(12)])
for m in mutations(zimg, 300):
    la_api.list_entries(m, read_size=rnd.choice([None, 100, 4096]), skip_every=rnd.choice([0, 3])); n += 1
cdpos = zimg.find(b"PK\x01\x02")
for pos in list(range(cdpos, min(cdpos + 60, len(zimg)))) + list(range(len(zimg) - 22, len(zimg))):
    for v in (0, 1, 0x7f, 0xff):
        m = bytearray(zimg); m[pos] = v
        la_api.list_entries(bytes(m)); n += 1
# header-field fuzz on the plain tar: every byte of the first header in turn takes odd values
for pos in range(0, 512, 3):
    for v in (0, 0x20, 0x37, 0x38, 0x80, 0xff):
        m = bytearray(tar); m[pos] = v
        la_api.list_entries(bytes(m)); n += 1
# GNU 'L' and pax 'x' headers: mutated special headers and bodies
for pyfmt in (tarfile.GNU_FORMAT, tarfile.PAX_FORMAT):
    bio = io.BytesIO()
    with tarfile.open(fileobj=bio, mode="w", format=pyfmt) as t:
        for i in range(6):
            ti = tarfile.TarInfo(("long-name-%d/" % i) * rnd.randint(1, 60) + "leaf")
            ti.size = 700; ti.mtime = 1700000000.5
            t.addfile(ti, io.BytesIO(bytes(700)))
    sp = bio.getvalue()
    for m in mutations(sp, 150):
        la_api.list_entries(m, read_size=rnd.choice([None, 512])); n += 1
    for cut in range(0, min(len(sp), 6000), 97):
        la_api.list_entries(sp[:cut]); n += 1
words = [rnd.randbytes(rnd.randint(2, 11)) for _ in range(300)]
data = b"".join(rnd.choice(words) for _ in range(500000))[:3 << 20]
dep, _ = _dependent_frame(data, flg=0x54)
big, _ = S.synth_lz4_stream(5, 0, 40, blocks_per_frame=16, block_size=65536, nthreads=2)
gz = b"".join(S.gz_member(data[o:o + 50000], level=1) for o in range(0, len(data), 50000))
odd = bytearray(gz); odd[8], odd[9] = 9, 99
for img in (dep, big.tobytes(), gz, bytes(odd)):
    for m in mutations(img, 12):
        la_api.cat(m, read_size=rnd.choice([None, 65536, 1000])); n += 1
print("sanitized filter runs:", n)
'''


def test_filters_read_core_and_tar_walker_under_asan_ubsan(tmp_path):
    """The whole host side (read core, both filters with their window / carry / history arithmetic, the ustar
    walker) on top of the CPU mock of the device ABI, everything built with ASan + UBSan, over clean, mutated and
    truncated tar / tar.gz / tar.lz4 / multi-window lz4 and gzip streams."""
    host = os.path.join(ROOT, "libarchive_amd", "host")
    mock = os.path.join(ROOT, "tests", "mock_gpu")
    orc = os.path.join(ROOT, "oracle")
    srcs = [os.path.join(host, f) for f in ("la_lz4_index.c", "la_gzip_index.c", "la_read_core.c", "la_format_tar.c",
                                            "la_format_zip.c", "la_hash_dropin.c", "la_write_filters.c", "la_write_zstd.c", "la_filter_lz4.c", "la_filter_gzip.c", "la_filter_zstd.c", "la_bid_policy.c", "la_zstd_index.c")]
    srcs += [os.path.join(mock, "la_gpu_mock.c")] + [os.path.join(orc, f) for f in ("orc_hash.c", "orc_lz4.c", "orc_inflate.c", "orc_zstd.c")]
    subprocess.check_call(["gcc", "-O1", "-g", "-fPIC", "-std=gnu11", "-fsanitize=address,undefined", "-fno-omit-frame-pointer",
                           "-I" + os.path.join(ROOT, "include"), "-shared", "-o", os.path.join(mock, "libla_host_mock_asan.so")] + srcs)
    libasan = subprocess.check_output(["gcc", "-print-file-name=libasan.so"]).decode().strip()
    env = dict(os.environ, LD_PRELOAD=libasan, ASAN_OPTIONS="detect_leaks=0:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1")
    script = tmp_path / "drv_filters.py"
    script.write_text("ROOT = %r\n" % ROOT + FILTER_DRIVER)
    out = subprocess.run([sys.executable, str(script)], env=env, capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, (out.stdout[-1000:], out.stderr[-4000:])
    assert "sanitized filter runs:" in out.stdout
