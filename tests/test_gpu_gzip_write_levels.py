"""The gzip write filter's compression levels on the device: "compression-level" 0 writes stored blocks (what the
reference's level 0 writes), 1 the fixed-Huffman blocks of the fast level, 2..9 and the default (6) the smallest of a
dynamic-Huffman, a fixed-Huffman and a stored block per chunk.  Inputs stay below one filter window, so the members
are the ones a single la_gpu_gzip_compress call over the same bytes writes, and the images must be equal."""
import gzip
import io
import random
import struct

import numpy as np
import pytest

import la_api
import oracle_lib as O
from test_gpu_lz4_write import ARCHIVE_OK, write_lz4

pytestmark = pytest.mark.gpu


def _datas():
    rnd = random.Random(52)
    words = [rnd.randbytes(rnd.randint(2, 10)) for _ in range(200)]
    text = b"".join(rnd.choice(words) for _ in range(200000))[:700001]
    return [("text", text), ("noise", rnd.randbytes(100000)), ("zeros", bytes(150000)), ("short", b"levels"),
            ("mixed", text[:60000] + rnd.randbytes(50000) + bytes(40000))]


def _abi(ctx, data, mode):
    import torch
    from libarchive_amd.gzip import compress_to_members
    d_plain = torch.from_numpy(np.frombuffer(data, dtype=np.uint8).copy()).cuda()
    return compress_to_members(ctx, d_plain, 49152, mtime=0, options=mode).cpu().numpy().tobytes()


def _block_types(img):
    pos, out = 0, []
    while pos < len(img):
        out.append((img[pos + 18] >> 1) & 3)
        pos += struct.unpack_from("<H", img, pos + 16)[0] + 1
    return out


@pytest.mark.parametrize("name,data", _datas(), ids=[n for n, _ in _datas()])
def test_levels_select_the_block_mode(gpu_ctx, name, data):
    want = {mode: _abi(gpu_ctx, data, mode) for mode in (0, 1, 2)}
    for level, mode in (("0", 2), ("1", 0), ("2", 1), ("6", 1), ("9", 1), (None, 1)):
        options = (("timestamp", None),) + ((("compression-level", level),) if level is not None else ())
        rc, img = write_lz4(data, options, None, codec="gzip")
        assert rc == ARCHIVE_OK and img == want[mode], (name, level)
        for piece in (1, 7, 65537):
            if piece == 1 and len(data) > 200000:
                continue        # (a call per byte: the shorter inputs cover it)
            rc, cut = write_lz4(data, options, piece, codec="gzip")
            assert rc == ARCHIVE_OK and cut == img, (name, level, piece)
        assert gzip.GzipFile(fileobj=io.BytesIO(img)).read() == data
        out, res = O.gzip_stream_decode(img, len(data) + 64)
        assert (res.rc, res.errmsg) == (0, b"") and out.tobytes() == data
        r = la_api.cat(img)
        assert r.filters[0] == (1, "gzip") and r.data == data
        if level == "0":
            assert set(_block_types(img)) == {0}
    if name == "text":
        assert 2 in _block_types(want[1]) and set(_block_types(want[0])) <= {0, 1}
        assert len(want[1]) < len(want[0]) < len(want[2])
