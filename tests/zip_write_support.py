"""Shared by the ZIP writer's tests (tests/test_gpu_zip_write.py on the device, tests/test_host_zip_write.py on the CPU
mock): a ctypes harness over archive_write_* with archive_write_set_format_zip, the archive shapes both suites write, a
struct-level parser of what comes out, and the field-by-field comparison with what the cited lines of
libarchive/archive_write_set_format_zip.c prescribe."""
import ctypes as C
import random
import struct
import time
import zlib

ARCHIVE_OK, ARCHIVE_WARN, ARCHIVE_FAILED, ARCHIVE_FATAL = 0, -20, -25, -30
AE_IFREG, AE_IFDIR, AE_IFLNK, AE_IFIFO = 0o100000, 0o040000, 0o120000, 0o010000
WINDOW = 1 << 20        # LA_GPU_WRITE_WINDOW_MIB=1


def setup(lib):
    if getattr(lib, "_zip_write_ready", False):
        return lib
    lib.archive_write_new.restype = C.c_void_p
    lib.archive_entry_new.restype = C.c_void_p
    for f in ("archive_write_set_format_zip", "archive_write_set_format_raw", "archive_write_add_filter_gzip", "archive_write_close",
              "archive_write_free", "archive_write_finish_entry", "archive_entry_free", "archive_entry_clear", "archive_entry_unset_size"):
        getattr(lib, f).argtypes = [C.c_void_p]
    lib.archive_entry_clear.restype = C.c_void_p
    lib.archive_entry_free.restype = None
    for f in ("archive_write_set_format_option", "archive_write_set_filter_option"):
        getattr(lib, f).argtypes = [C.c_void_p, C.c_char_p, C.c_char_p, C.c_char_p]
    lib.archive_write_open_memory.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]
    lib.archive_write_header.argtypes = [C.c_void_p, C.c_void_p]
    lib.archive_write_data.argtypes = [C.c_void_p, C.c_char_p, C.c_size_t]
    lib.archive_write_data.restype = C.c_ssize_t
    lib.archive_error_string.argtypes = [C.c_void_p]
    lib.archive_error_string.restype = C.c_char_p
    lib.archive_entry_set_pathname.argtypes = [C.c_void_p, C.c_char_p]
    lib.archive_entry_set_mtime.argtypes = [C.c_void_p, C.c_int64, C.c_long]
    lib.archive_entry_set_size.argtypes = [C.c_void_p, C.c_int64]
    lib.archive_entry_set_filetype.argtypes = [C.c_void_p, C.c_uint]
    lib.archive_entry_set_perm.argtypes = [C.c_void_p, C.c_uint]
    for f in ("archive_entry_set_pathname", "archive_entry_set_mtime", "archive_entry_set_size", "archive_entry_set_filetype",
              "archive_entry_set_perm", "archive_entry_unset_size"):
        getattr(lib, f).restype = None
    lib._zip_write_ready = True
    return lib


class Entry:
    """name (bytes), type, perm, mtime (None = not set), size (None = not set), data, piece (bytes per write call)"""

    def __init__(self, name, data=b"", type=AE_IFREG, perm=0o644, mtime=1700000000, size="len", piece=None):
        self.name = name if isinstance(name, bytes) else name.encode()
        self.data, self.type, self.perm, self.mtime, self.piece = data, type, perm, mtime, piece
        self.size = len(data) if size == "len" else size

    @property
    def stored_name(self):
        return self.name + (b"/" if self.type == AE_IFDIR and not self.name.endswith(b"/") else b"")

    @property
    def kept(self):
        """the bytes that belong in the archive: bytes written past a set size are ignored"""
        if self.type != AE_IFREG:
            return b""
        return self.data if self.size is None else self.data[:self.size]


def _error(lib, a):
    e = lib.archive_error_string(a)
    return e.decode() if e else None


def write_zip(lib, entries, options=(), cap=None, gzip_filter=False, finish_every=3):
    """-> (rc, archive bytes) or (rc, error string) where a call fails.  options: [(key, value)], applied with the module
    name "zip"."""
    lib = setup(lib)
    a = lib.archive_write_new()
    ent = lib.archive_entry_new()
    try:
        if gzip_filter:
            assert lib.archive_write_add_filter_gzip(a) == ARCHIVE_OK
        assert lib.archive_write_set_format_zip(a) == ARCHIVE_OK
        for k, v in options:
            rc = lib.archive_write_set_format_option(a, b"zip", k.encode(), None if v is None else v.encode())
            if rc != ARCHIVE_OK:
                return rc, _error(lib, a)
        if cap is None:
            cap = sum(len(e.data) + len(e.data) // 8 + 2 * len(e.name) + 300 for e in entries) + 65536
        buf = C.create_string_buffer(cap)
        used = C.c_size_t(0)
        rc = lib.archive_write_open_memory(a, buf, cap, C.byref(used))
        if rc != ARCHIVE_OK:
            return rc, _error(lib, a)
        for i, e in enumerate(entries):
            lib.archive_entry_clear(ent)
            lib.archive_entry_set_pathname(ent, e.name)
            lib.archive_entry_set_filetype(ent, e.type)
            lib.archive_entry_set_perm(ent, e.perm)
            if e.mtime is not None:
                lib.archive_entry_set_mtime(ent, e.mtime, 0)
            if e.size is not None:
                lib.archive_entry_set_size(ent, e.size)
            rc = lib.archive_write_header(a, ent)
            if rc != ARCHIVE_OK:
                return rc, _error(lib, a)
            step = e.piece or max(len(e.data), 1)
            for at in range(0, len(e.data), step):
                part = e.data[at:at + step]
                r = lib.archive_write_data(a, part, len(part))
                if r < 0:
                    return r, _error(lib, a)
                assert r == min(len(part), max(0, (len(e.data) if e.size is None else e.size) - at)), (e.name, at, r)
            if finish_every and i % finish_every == 0:      # explicit, or left to the next header / close
                rc = lib.archive_write_finish_entry(a)
                if rc != ARCHIVE_OK:
                    return rc, _error(lib, a)
        rc = lib.archive_write_close(a)
        if rc != ARCHIVE_OK:
            return rc, _error(lib, a)
        return rc, buf.raw[:used.value]
    finally:
        lib.archive_entry_free(ent)
        lib.archive_write_free(a)


def set_option(lib, key, value, module=b"zip"):
    """-> (rc, error string) of one archive_write_set_format_option on a fresh handle"""
    lib = setup(lib)
    a = lib.archive_write_new()
    try:
        assert lib.archive_write_set_format_zip(a) == ARCHIVE_OK
        rc = lib.archive_write_set_format_option(a, module, key.encode(), None if value is None else value.encode())
        return rc, _error(lib, a)
    finally:
        lib.archive_write_free(a)


def word_text(seed, n):
    rnd = random.Random(seed)
    words = [rnd.randbytes(rnd.randint(2, 10)) for _ in range(150)]
    return b"".join(rnd.choice(words) for _ in range(n // 4 + 1))[:n]


_MAIN = []


def main_entries():
    """the main archive of both suites (built once, never changed)"""
    if not _MAIN:
        text = word_text(5, 3 << 20)
        _MAIN.extend([
            Entry("empty.txt", b"", mtime=1600000000),
            Entry("a/dir", type=AE_IFDIR, perm=0o755, mtime=1650000001),
            Entry("a/dir/one", b"x", perm=0o600),
            Entry("a/dir/text", text, piece=65553, mtime=1710000123),
            Entry("random.bin", random.Random(6).randbytes(300000), perm=0o444),
            Entry("window", word_text(7, WINDOW)),
            Entry("no-size", word_text(8, 70001), size=None, piece=9999, mtime=None),
            Entry("past-size", word_text(9, 5000), size=3000, piece=1024),
            Entry("dir-with-slash/", type=AE_IFDIR, perm=0o700),
            Entry("last", b"the end\n"),
        ])
    return _MAIN


# ------------------------------------------------------------------ what was written, field by field

def dos_time(t):
    """archive_time.c:76-122 for a time inside the DOS range"""
    lt = time.localtime(t)
    return ((lt.tm_year - 1980) << 25) | (lt.tm_mon << 21) | (lt.tm_mday << 16) | (lt.tm_hour << 11) | (lt.tm_min << 5) | (lt.tm_sec >> 1)


def parse(img, desc_size=16):
    """-> (locals, central, end): every record of the archive as dicts of its fields, walked front to back (local
    headers and descriptors of `desc_size` bytes: a descriptor does not say how wide it is) and from the end record
    (central directory)"""
    end = {}
    eocd = img.rfind(b"PK\x05\x06")
    assert eocd == len(img) - 22, "end record is the last 22 bytes (no comment)"
    (end["disk"], end["cd_disk"], end["n_disk"], end["n"], end["cd_bytes"], end["cd_off"], end["comment"]) = struct.unpack_from("<HHHHIIH", img, eocd + 4)
    end["zip64"] = None
    if img[eocd - 20:eocd - 16] == b"PK\x06\x07":
        disk, off64, disks = struct.unpack_from("<IQI", img, eocd - 16)
        assert img[off64:off64 + 4] == b"PK\x06\x06" and off64 == eocd - 20 - 56
        size, made, need, d0, d1, n0, n1, cdb, cdo = struct.unpack_from("<QHHIIQQQQ", img, off64 + 4)
        end["zip64"] = dict(locator_disk=disk, locator_disks=disks, size=size, made=made, need=need, disk=d0, cd_disk=d1,
                            n_disk=n0, n=n1, cd_bytes=cdb, cd_off=cdo)
    cd_off = end["zip64"]["cd_off"] if end["zip64"] else end["cd_off"]
    n = end["zip64"]["n"] if end["zip64"] else end["n"]
    central, at = [], cd_off
    for _ in range(n):
        assert img[at:at + 4] == b"PK\x01\x02"
        (made, need, flags, method, dost, crc, comp, unc, nl, xl, cl, disk, iattr, xattr, off) = struct.unpack_from("<HHHHIIIIHHHHHII", img, at + 4)
        name = img[at + 46:at + 46 + nl]
        extra = img[at + 46 + nl:at + 46 + nl + xl]
        central.append(dict(made=made, need=need, flags=flags, method=method, dos=dost, crc=crc, comp=comp, unc=unc, name=name,
                            extra=extra, comment_len=cl, disk=disk, iattr=iattr, xattr=xattr, off=off))
        at += 46 + nl + xl + cl
    assert at == cd_off + (end["zip64"]["cd_bytes"] if end["zip64"] else end["cd_bytes"])
    locals_, at = [], 0
    for c in central:
        assert c["off"] == at, "entries lie back to back from offset 0"
        assert img[at:at + 4] == b"PK\x03\x04"
        need, flags, method, dost, crc, comp, unc, nl, xl = struct.unpack_from("<HHHIIIIHH", img, at + 4)
        name = img[at + 30:at + 30 + nl]
        extra = img[at + 30 + nl:at + 30 + nl + xl]
        data_at = at + 30 + nl + xl
        rec = dict(need=need, flags=flags, method=method, dos=dost, crc=crc, comp=comp, unc=unc, name=name, extra=extra,
                   data=img[data_at:data_at + c["comp"]], desc=None)
        at = data_at + c["comp"]
        if flags & 8:
            assert img[at:at + 4] == b"PK\x07\x08"
            dcrc, dcomp, dunc = struct.unpack_from("<IQQ" if desc_size == 24 else "<III", img, at + 4)
            rec["desc"] = dict(crc=dcrc, comp=dcomp, unc=dunc, size=desc_size)
            at += desc_size
        locals_.append(rec)
    assert at == cd_off, "the central directory follows the last entry"
    return locals_, central, end


def check_records(img, entries, method=8, level=6, force_zip64=False, fake_crc=False, utf8=False):
    """every field of every record against archive_write_set_format_zip.c (line numbers in the comments)"""
    locals_, central, end = parse(img, 24 if force_zip64 else 16)
    assert len(central) == len(entries)
    for e, l, c in zip(entries, locals_, central):
        reg = e.type == AE_IFREG
        m = method if reg else 0                                     # :950-955 a directory is stored
        need = 20 if not reg else (10 if m == 0 else 20)             # :955 MIN_VERSION_NEEDED(20), :969, :1006
        if reg and (force_zip64 or e.size is None):                  # :1044-1049 forced, :1063-1066 size unknown
            need = 45
        flags = 0
        if reg:
            flags |= 8                                               # :1051-1052, :1062 length at end
            if m == 8:
                flags |= {1: 6, 2: 6, 3: 4, 4: 4, 8: 2, 9: 2}.get(level, 0)   # :990-1005, :1085-1100
        if utf8 and any(b > 127 for b in e.name):
            flags |= 0x800                                           # :924-935
        body = e.kept
        crc = 0 if fake_crc else zlib.crc32(body)                    # :507-517 fakecrc32
        ut = b"" if e.mtime is None else b"UT\x05\x00\x01" + struct.pack("<I", e.mtime)   # :1229-1255, :2054-2071
        dos = dos_time(e.mtime) if e.mtime is not None else 0x00210000   # archive_time.c:118-120 clamps 1970 to DOS_MIN_TIME
        # local header :1119-1136, :1303-1304
        assert l["name"] == e.stored_name == c["name"]                # :2242-2307
        assert (l["need"], l["flags"], l["method"], l["dos"]) == (need, flags, m, dos), (e.name, l)
        assert (l["crc"], l["comp"], l["unc"]) == (0, 0, 0), e.name  # :1131-1135: not with length-at-end; a directory has none
        assert l["extra"] == ut, e.name                               # no "ux" (no ids), no Zip64 field below 4 GiB
        # data and descriptor :2025-2052
        if reg:
            d = l["desc"]
            assert d is not None and d["size"] == (24 if force_zip64 else 16), e.name
            assert (d["crc"], d["comp"], d["unc"]) == (crc, c["comp"], len(body)), e.name
            if m == 8:
                z = zlib.decompressobj(-15)
                assert z.decompress(l["data"]) == body and z.eof and z.unused_data == b"", e.name
            else:
                assert l["data"] == body, e.name
        else:
            assert l["desc"] is None and l["data"] == b""
        # central directory :1145-1168, :2073-2139
        assert c["made"] == 3 * 256 + need, e.name                   # :1152
        assert (c["need"], c["flags"], c["method"], c["dos"]) == (need, flags, m, dos), e.name
        assert (c["crc"], c["unc"]) == (crc, len(body)), e.name
        assert c["extra"] == ut and c["comment_len"] == 0 and c["disk"] == 0 and c["iattr"] == 0, e.name
        assert c["xattr"] == (e.type | e.perm) << 16, e.name         # :1163-1165
    # end records :2144-2214
    n = len(entries)
    cd_bytes = sum(46 + len(c["name"]) + len(c["extra"]) for c in central)
    cd_off = central[0]["off"] + sum(30 + len(l["name"]) + len(l["extra"]) + len(l["data"]) + (l["desc"]["size"] if l["desc"] else 0)
                                     for l in locals_) if n else 0
    assert (end["disk"], end["cd_disk"], end["comment"]) == (0, 0, 0)
    assert end["n_disk"] == end["n"] == min(n, 0xFFFF) and end["cd_bytes"] == cd_bytes and end["cd_off"] == cd_off
    if force_zip64 or n > 0xFFFF:                                    # :2165-2196
        z = end["zip64"]
        assert z == dict(locator_disk=0, locator_disks=1, size=44, made=45, need=45, disk=0, cd_disk=0, n_disk=n, n=n,
                         cd_bytes=cd_bytes, cd_off=cd_off)
    else:
        assert end["zip64"] is None
    return locals_, central, end


OPTION_TABLE = [
    # key, value, rc, error string (None: not compared)          archive_write_set_format_zip.c
    ("compression", "deflate", ARCHIVE_OK, None),                 # :354-357
    ("compression", "store", ARCHIVE_OK, None),                   # :362-364
    ("compression", None, ARCHIVE_FAILED, "zip: compression option needs a compression name"),   # :350-353
    ("compression", "bzip2", ARCHIVE_FAILED, "bzip2 compression not supported"),                 # :365-372
    ("compression", "lzma", ARCHIVE_FAILED, "lzma compression not supported"),
    ("compression", "xz", ARCHIVE_FAILED, "xz compression not supported"),
    ("compression", "zstd", ARCHIVE_FAILED, "zstd compression not supported"),
    ("compression", "rot13", ARCHIVE_FAILED, None),               # :398 ret stays ARCHIVE_FAILED
    ("compression-level", "0", ARCHIVE_OK, None), ("compression-level", "1", ARCHIVE_OK, None),
    ("compression-level", "9", ARCHIVE_OK, None),
    ("compression-level", "10", ARCHIVE_FAILED, "Undefined option: `zip:compression-level=10'"),  # :406-410 WARN, archive_options.c:65-70
    ("compression-level", "x", ARCHIVE_FAILED, "Undefined option: `zip:compression-level=x'"),
    ("compression-level", None, ARCHIVE_FAILED, "Undefined option: `!zip:compression-level'"),     # :402-403
    ("zip64", "1", ARCHIVE_OK, None), ("zip64", None, ARCHIVE_OK, None),                           # :535-549
    ("fakecrc32", "1", ARCHIVE_OK, None), ("fakecrc32", None, ARCHIVE_OK, None),                   # :507-517
    ("threads", "4", ARCHIVE_OK, None), ("threads", "0", ARCHIVE_OK, None),                        # :436-462
    ("threads", None, ARCHIVE_FAILED, None), ("threads", "4x", ARCHIVE_FAILED, "Illegal value `4x'"),
    ("encryption", None, ARCHIVE_OK, None),                                                         # :464-466
    ("encryption", "aes256", ARCHIVE_FAILED, "encryption not supported"),                          # :486-494
    ("encryption", "zipcrypt", ARCHIVE_FAILED, "encryption not supported"),
    ("encryption", "rot13", ARCHIVE_FAILED, "zip: unknown encryption 'rot13'"),                    # :495-498
    ("hdrcharset", "UTF-8", ARCHIVE_OK, None),
    ("hdrcharset", None, ARCHIVE_FAILED, "zip: hdrcharset option needs a character-set name"),     # :522-525
    ("hdrcharset", "KOI8-R", ARCHIVE_FATAL, None),                                                  # :531-532: no conversion to it
    ("no-such-option", "1", ARCHIVE_FAILED, "Undefined option: `zip:no-such-option=1'"),           # :552-555
]


def check_with_zipfile(img, entries, method=8):
    """Python's zipfile reads it: CRCs hold, and names, bytes, times, attributes, flags and methods are the entries'"""
    import io
    import zipfile
    with zipfile.ZipFile(io.BytesIO(img)) as z:
        assert z.testzip() is None
        infos = z.infolist()
        assert [i.filename.encode("utf-8" if i.flag_bits & 0x800 else "cp437") for i in infos] == [e.stored_name for e in entries]
        for e, i in zip(entries, infos):
            assert z.read(i) == e.kept, e.name
            lt = time.localtime(e.mtime) if e.mtime is not None else (1980, 1, 1, 0, 0, 0)
            assert i.date_time == (lt[0], lt[1], lt[2], lt[3], lt[4], lt[5] & ~1), e.name
            assert i.external_attr == (e.type | e.perm) << 16, e.name
            assert i.flag_bits & 8 == (8 if e.type == AE_IFREG else 0), e.name
            assert i.compress_type == (method if e.type == AE_IFREG else 0), e.name
            assert i.file_size == len(e.kept) and i.create_system == 3, e.name
