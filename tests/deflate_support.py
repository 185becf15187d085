"""The referee of the hand-built deflate streams: the image's libz.so.1 through ctypes, called the way the reference's
gzip filter calls it (inflateInit2(-15), then inflate(Z_NO_FLUSH) until it ends or refuses;
archive_read_support_filter_gzip.c:363, :479).  Python's zlib module cannot serve: it reports neither the bytes in front
of a data error nor total_in."""
import ctypes as C

Z_OK, Z_STREAM_END, Z_DATA_ERROR, Z_BUF_ERROR = 0, 1, -3, -5


class _ZStream(C.Structure):
    _fields_ = [("next_in", C.c_void_p), ("avail_in", C.c_uint), ("total_in", C.c_ulong),
                ("next_out", C.c_void_p), ("avail_out", C.c_uint), ("total_out", C.c_ulong),
                ("msg", C.c_char_p), ("state", C.c_void_p), ("zalloc", C.c_void_p), ("zfree", C.c_void_p),
                ("opaque", C.c_void_p), ("data_type", C.c_int), ("adler", C.c_ulong), ("reserved", C.c_ulong)]


_z = None


def libz():
    global _z
    if _z is None:
        z = C.CDLL("libz.so.1")
        z.zlibVersion.restype = C.c_char_p
        z.inflateInit2_.argtypes = [C.POINTER(_ZStream), C.c_int, C.c_char_p, C.c_int]
        z.inflate.argtypes = [C.POINTER(_ZStream), C.c_int]
        z.inflateEnd.argtypes = [C.POINTER(_ZStream)]
        _z = z
    return _z


def zlib_version():
    return libz().zlibVersion().decode()


def zlib_inflate(image, piece=None, out_piece=None):
    """(verdict, total_in, bytes, msg).  verdict: "ok" (Z_STREAM_END), "data" (Z_DATA_ERROR), "more" (Z_OK / Z_BUF_ERROR
    with the whole input given: the stream is not over).  piece: input bytes per call (None: all at once); out_piece:
    output bytes per buffer (None: one buffer larger than any case's output)."""
    z = libz()
    s = _ZStream()
    rc = z.inflateInit2_(C.byref(s), -15, z.zlibVersion(), C.sizeof(_ZStream))
    assert rc == Z_OK, rc
    src = C.create_string_buffer(bytes(image), max(len(image), 1))
    osz = out_piece or (1 << 20)
    obuf = C.create_string_buffer(osz)
    out, p, n = bytearray(), 0, len(image)
    step = piece or max(n, 1)
    try:
        s.next_out, s.avail_out = C.addressof(obuf), osz
        while True:
            if s.avail_in == 0 and p < n:
                k = min(step, n - p)
                s.next_in, s.avail_in = C.addressof(src) + p, k
                p += k
            rc = z.inflate(C.byref(s), 0)
            full = s.avail_out == 0
            out += obuf.raw[:osz - s.avail_out]
            s.next_out, s.avail_out = C.addressof(obuf), osz
            msg = s.msg.decode() if s.msg else ""
            if rc == Z_STREAM_END:
                return "ok", int(s.total_in), bytes(out), msg
            if rc == Z_DATA_ERROR:
                return "data", int(s.total_in), bytes(out), msg
            assert rc in (Z_OK, Z_BUF_ERROR), rc
            if s.avail_in == 0 and p == n and not full:
                return "more", int(s.total_in), bytes(out), msg
    finally:
        z.inflateEnd(C.byref(s))
