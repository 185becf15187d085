"""The uu read filter's HOST side (la_filter_uu.c: the bidder restated, windows, the carried tail line, the two-word
state, verdicts, read_header) over a CPU stand-in for la_gpu_uu_decode (tests/mock_gpu/la_gpu_uu_mock.c: the kernels'
own rules header, walked line by line).  la_api.cat through the mock library must equal the oracle
(uu_support.reference_cat) on bytes, return code, error string and filter code / name."""
import ctypes as C
import gzip
import hashlib
import io
import os
import subprocess
import tarfile

import pytest

import la_api
import uu_mock_build as mock_build
import uu_support as U

UU = (U.ARCHIVE_FILTER_UU, "uu")
ARCHIVE_ERRNO_MISC, ARCHIVE_ERRNO_FILE_FORMAT = -1, 84


@pytest.fixture(scope="module")
def mock():
    lib = mock_build.host_lib()
    la_api.use_library(lib)
    yield lib
    la_api.use_library(None)


def same_as_reference(image, read_size=None):
    ref = U.reference_cat(image, read_size)
    res = la_api.cat(image, read_size=read_size)
    got = la_api.as_reference_tuple(res)
    assert (len(got[0]), got[1], got[2]) == (len(ref[0]), ref[1], ref[2])
    assert got[0] == ref[0]
    if res.filters:     # (an error in front of the first decoded byte ends archive_read_open, before the filters can be listed)
        assert (res.filters[0] == UU) == (U.bid(image) > 0)
    return res


@pytest.mark.parametrize("name", sorted(U.filter_shapes()))
@pytest.mark.parametrize("read_size", [None, 1000, 1])
def test_shapes(mock, name, read_size):
    same_as_reference(U.filter_shapes()[name], read_size)


def test_the_shapes_end_as_their_names_say():
    """the oracle's own verdicts on the shapes: the table the filter is held against above is not all one kind"""
    sh = U.filter_shapes()
    end = lambda n: U.reference_cat(sh[n])[1:]      # noqa: E731
    bad = (U.ARCHIVE_FATAL, U.E_INSUFFICIENT)
    for n in sh:
        assert (U.bid(sh[n]) == 0) == n.startswith("declined"), n
    for n in ("uu", "uu_crlf", "uu_cr", "uu_space_for_zero", "uu_checksum_characters", "uu_padding_ignored", "uu_no_end_line", "uu_no_zero_line",
              "uu_end_without_line_end", "b64", "b64_no_terminator", "b64_three_equals", "b64_empty_lines", "b64_equals_inside", "b64_two_equals_line",
              "two_sections", "three_sections_with_junk", "binary_junk_behind_end", "binary_junk_behind_base64", "head_line_of_131071_bytes",
              "uu_line_of_32768_bytes", "b64_line_of_32768_bytes", "uu_cut_behind_a_cr"):
        assert end(n) == (0, ""), n
    for n in ("uu_wrong_end", "uu_end_with_a_blank", "uu_length_character_above_the_body", "uu_invalid_character", "uu_empty_line_in_data",
              "uu_length_character_not_uuchar", "uu_bad_byte_in_data", "uu_high_byte_in_end", "uu_tab_in_data", "b64_lone_character",
              "b64_invalid_character", "b64_bad_byte", "bad_byte_behind_an_empty_base64_section", "uu_cut_inside_end",
              "end_line_of_40000_bytes"):
        assert end(n) == bad, n
    for n in ("uu_cut_inside_a_data_line", "b64_cut_inside_a_line", "text_behind_end_without_line_end"):
        assert end(n) == (U.ARCHIVE_FATAL, U.E_MISSING), n
    for n in ("head_line_of_131072_bytes", "uu_line_of_32769_bytes", "b64_line_of_32769_bytes"):
        assert end(n) == (U.ARCHIVE_FATAL, U.E_INVALID), n
    assert end("head_line_of_200000_bytes_with_a_bad_byte") == (0, "")      # ignored: bytes were decoded in front of it
    # every byte of the lines in front of a failing line is out
    assert len(U.reference_cat(sh["uu_bad_byte_in_data"])[0]) == 45 * 6 and len(U.reference_cat(sh["uu_line_of_32769_bytes"])[0]) == 45
    assert U.reference_cat(sh["two_sections"])[0] == U.randbytes(2, 100) + U.randbytes(3, 7) * 30


def entry_of(lib, image):
    """(filters, pathname, file type | permissions) of the first header, through the raw format"""
    lib.archive_read_new.restype = C.c_void_p
    a = C.c_void_p(lib.archive_read_new())
    try:
        for f in (lib.archive_read_support_filter_all, lib.archive_read_support_format_raw):
            f.argtypes = [C.c_void_p]
            f(a)
        buf = C.create_string_buffer(bytes(image), len(image))
        lib.archive_read_open_memory2.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t]
        assert lib.archive_read_open_memory2(a, buf, len(image), len(image)) == 0
        ent = C.c_void_p()
        lib.archive_read_next_header.argtypes = [C.c_void_p, C.POINTER(C.c_void_p)]
        assert lib.archive_read_next_header(a, C.byref(ent)) == 0
        for f, t in ((lib.archive_entry_pathname, C.c_char_p), (lib.archive_entry_filetype, C.c_uint), (lib.archive_entry_perm, C.c_uint)):
            f.argtypes, f.restype = [C.c_void_p], t
        return lib.archive_entry_pathname(ent).decode(), lib.archive_entry_filetype(ent) | lib.archive_entry_perm(ent)
    finally:
        lib.archive_read_free.argtypes = [C.c_void_p]
        lib.archive_read_free(a)


@pytest.mark.parametrize("read_size", [None, 1000, 1])
def test_fixtures(mock, read_size):
    for m, img in U.fixtures():
        res = same_as_reference(img, read_size)
        assert res.rc == la_api.ARCHIVE_EOF and res.filters == [UU, (0, "none")], m["file"]
        assert res.pathname == m["pathname"] and res.format_name == "raw"
        assert len(res.data) == m["decoded_size"] and hashlib.sha256(res.data).hexdigest() == m["decoded_sha256"]
        assert entry_of(mock, img) == (m["pathname"], 0o100000 | int(m["mode"], 8))


def test_read_header_names(mock):
    sh = U.filter_shapes()
    assert entry_of(mock, sh["name_of_one_character"]) == ("data", 0o100644)      # a name of one character is not taken (uu.c:585)
    assert entry_of(mock, sh["two_sections"])[0] in ("first", "second")
    assert entry_of(mock, U.uu_section(b"abc", name=b"a name with blanks.tar", mode=0o7))[0:2] == ("a name with blanks.tar", 0o100007)


def test_errno_classes(mock):
    sh = U.filter_shapes()
    lib = mock
    for name, want in (("uu_wrong_end", ARCHIVE_ERRNO_MISC), ("uu_cut_inside_a_data_line", ARCHIVE_ERRNO_FILE_FORMAT),
                       ("uu_line_of_32769_bytes", ARCHIVE_ERRNO_FILE_FORMAT)):
        img = sh[name]
        lib.archive_read_new.restype = C.c_void_p
        a = C.c_void_p(lib.archive_read_new())
        lib.archive_read_support_filter_all(a)
        lib.archive_read_support_format_raw(a)
        buf = C.create_string_buffer(img, len(img))
        lib.archive_read_open_memory2.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t]
        r = lib.archive_read_open_memory2(a, buf, len(img), len(img))
        ent = C.c_void_p()
        if r == 0:
            r = lib.archive_read_next_header(a, C.byref(ent))
        tmp = C.create_string_buffer(1 << 16)
        while r == 0:
            k = lib.archive_read_data(a, tmp, 1 << 16)
            r = 0 if k > 0 else (1 if k == 0 else int(k))
        assert r == la_api.ARCHIVE_FATAL and lib.archive_errno(a) == want, name
        lib.archive_read_free(a)


def tar_gz():
    buf = io.BytesIO()
    with tarfile.open(fileobj=buf, mode="w", format=tarfile.USTAR_FORMAT) as t:
        for i, name in enumerate(("dir/one.txt", "dir/two.bin", "three")):
            data = U.text(i, 3000) if i != 1 else U.randbytes(i, 2000)
            ti = tarfile.TarInfo(name)
            ti.size, ti.mtime = len(data), 86400
            t.addfile(ti, io.BytesIO(data))
    return gzip.compress(buf.getvalue(), mtime=0), ["dir/one.txt", "dir/two.bin", "three"]


@pytest.mark.parametrize("lead", [0, 1, 65536])
def test_tar_gz_behind_a_preamble(mock, monkeypatch, lead):
    monkeypatch.setenv("LA_GPU_BID", "all")
    tgz, names = tar_gz()
    for img in (U.uu_section(tgz, name=b"x.tar.gz"), U.b64_section(tgz, name=b"x.tar.gz")):
        res = la_api.list_entries(U.preamble(lead) + img)
        assert res.open_rc == 0 and res.rc == la_api.ARCHIVE_EOF, res.error
        assert res.filters == [(1, "gzip"), UU, (0, "none")]
        assert [e[0] for e in res.entries] == names and res.entries[1][5] == U.randbytes(1, 2000)


def test_512_kib_of_preamble_is_not_bid_for(mock):
    tgz, _ = tar_gz()
    img = U.preamble(512 << 10) + U.uu_section(tgz, name=b"x.tar.gz")
    assert U.bid(img) == 0
    res = la_api.list_entries(img)
    assert res.open_rc != 0 and not res.entries
    cat = la_api.cat(img)
    assert cat.filters == [(0, "none")] and cat.data == img


def test_look_ahead_over_another_filter(mock, monkeypatch):
    """Over another filter the bidder looks at what that filter has handed out and asks for no more.  A few lines of
    text out of an lz4 frame whose content checksum fails: reading on for the next line would make the open fail and
    lose the text.  A .uu inside a .gz: the gzip filter hands out a whole window, so a header behind 100 KiB of
    preamble -- inside the 128 KiB cap -- is still found."""
    import streams as S
    monkeypatch.setenv("LA_GPU_BID", "all")
    img, plain, rc, msg = S.appendix_d_lz4_cases()["bad_content_sum"]
    res = la_api.cat(img)
    assert la_api.as_reference_tuple(res) == (plain, rc, msg) and res.filters == [(13, "lz4"), (0, "none")]
    text = b"".join(b"line %d of a text that ends with its stream\n" % i for i in range(40))
    img, plain = S.lz4_frame([(text, S.lz4_block(text, stored=True))], bad_content=True)
    res = la_api.cat(img)
    assert la_api.as_reference_tuple(res) == (text, -30, "lz4 stream checksum error") and UU not in res.filters
    data = U.randbytes(5, 3000)
    for lead in (0, 1000, 100000):
        for read_size in (None, 512):
            res = la_api.cat(gzip.compress(U.preamble(lead) + U.uu_section(data), mtime=0), read_size=read_size)
            assert res.filters == [UU, (1, "gzip"), (0, "none")] and res.data == data and res.rc == la_api.ARCHIVE_EOF
    res = la_api.cat(gzip.compress(U.preamble(140000) + U.uu_section(data), mtime=0))      # beyond the cap: not bid for
    assert res.filters == [(1, "gzip"), (0, "none")]


def windows_stream():
    """3 MiB and a little: lines across the window edges at 1 MiB and 2 MiB, a '\\r' | '\\n' split on the first edge, a
    second header in the second window, base64 behind it"""
    first = U.randbytes(31, 45 * 18000)
    a = U.uu_section(first, name=b"one", nl=b"\r\n")
    assert len(a) > (1 << 20) + 1000
    edge = a.index(b"\r\n", (1 << 20) - 70)
    # a longer name moves that '\r' to the last byte of the first window (the header stays the stream's first line)
    a = U.uu_section(first, name=b"one" + b"x" * ((1 << 20) - 1 - edge), nl=b"\r\n")
    second = U.randbytes(32, 57 * 27000)
    img = a + U.junk(33, 50) + U.b64_section(second, name=b"two")
    assert img[(1 << 20) - 1:(1 << 20) + 1] == b"\r\n" and len(img) > 3 << 20
    assert img[1 << 21] not in b"\r\n" and img[(1 << 21) - 1] not in b"\r\n" and img[3 << 20] not in b"\r\n"
    return img, first + second


def test_window_edges(mock, monkeypatch):
    monkeypatch.setenv("LA_GPU_BATCH_MIB", "1")
    img, plain = windows_stream()
    res = same_as_reference(img)
    assert res.data == plain and res.rc == la_api.ARCHIVE_EOF
    # a damaged line in the third window: all bytes in front come out, then the message
    at = img.index(b"\n", (2 << 20) + 300000) + 1
    bad = img[:at + 5] + b"*" + img[at + 6:]
    res = same_as_reference(bad)
    assert res.rc == la_api.ARCHIVE_FATAL and res.error == U.E_INSUFFICIENT and 0 < len(res.data) < len(plain)
    assert res.data == plain[:len(res.data)] and len(res.data) > 45 * 18000 + 500000
    same_as_reference(img[:(1 << 20) + 1])
    same_as_reference(img[:1 << 20])
    same_as_reference(img[:2 << 20])
    same_as_reference(img, read_size=4099)


def test_a_line_larger_than_the_window_limit_is_refused_by_name(mock, monkeypatch):
    monkeypatch.setenv("LA_GPU_BATCH_MIB", "1")
    monkeypatch.setenv("LA_GPU_MAX_BATCH_MIB", "1")
    res = la_api.cat(U.uu_section(b"abc") + b"j" * 1200000 + b"\n")
    assert res.rc == la_api.ARCHIVE_FATAL and "uu line too large for the GPU data plane" in res.error, res.error


def fnv1a(data):
    h = 1469598103934665603
    for b in data:
        h = ((h ^ b) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return h


def test_sanitizer_program(mock, tmp_path):
    """the C filter and the stand-in as one ASan/UBSan program of their own (la_read_asan reads each image whole, 1000
    bytes and 1 byte at a time; the three must agree) over shapes, cuts and the fixtures"""
    out = str(tmp_path)
    exe = mock_build.program("la_read_asan")
    sh = U.filter_shapes()
    images = [img for name, img in sorted(sh.items()) if len(img) < 20000] + [img for _, img in U.fixtures()]
    two = sh["two_sections"]
    images += [two[:cut] for cut in range(30, len(two), 37)]
    assert len(images) > 40
    paths = []
    for i, img in enumerate(images):
        paths.append(os.path.join(out, "img%04d.uu" % i))
        with open(paths[-1], "wb") as f:
            f.write(img)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    run = subprocess.run([exe] + paths, env=env, capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, (run.stdout + run.stderr)[-3000:]
    assert "runtime error" not in run.stderr and "AddressSanitizer" not in run.stderr, run.stderr[-3000:]
    lines = run.stdout.splitlines()
    assert len(lines) == len(paths)
    for img, line in zip(images, lines):
        data, rc, msg = U.reference_cat(img)
        assert line == ("%d %d %016x %s" % (rc, len(data), fnv1a(data), msg)), (line, len(img))
