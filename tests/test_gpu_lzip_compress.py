"""la_gpu_lzip_compress through the C ABI.  Every output must pass lzip_write_support.accept (the reference's read loop
over liblzma, the member walk, each raw stream alone, the bound), must decode with this repository's device reader
(la_gpu_lzip_scan finds the members, la_gpu_lzip_decode returns them, status OK, CRC32 verified), and must be the bytes
recorded in tests/golden/lzip_write_digests.json from the CPU stand-in, which compiles the kernels' rules header: the
device has to write the same bytes.  The inputs are lzip_write_support.inputs(): the smallest that reach each border of
the shape (member, one-byte last member, the large member, expansion, runs, distance classes)."""
import numpy as np
import pytest
import torch

import lzip_write_support as W
from libarchive_amd import lzip

pytestmark = pytest.mark.gpu


def dev(data):
    if not data:
        return torch.zeros(0, dtype=torch.uint8, device="cuda")
    return torch.from_numpy(np.frombuffer(data, dtype=np.uint8).copy()).cuda()


def compress(ctx, data, level, **kw):
    return lzip.compress_window(ctx, dev(data), level, **kw).cpu().numpy().tobytes()


def decodes(ctx, name, level):
    """compress, run every reader, check the recorded digest; returns (members of the image, the image)"""
    data = W.inputs()[name]
    img = compress(ctx, data, level)
    assert len(img) <= lzip.compress_bound(len(data), level) == W.bound(len(data), level)
    ms = W.accept(img, data, level)
    # our own device reader: the scan finds every member, the decode returns its piece
    d_img = lzip.to_device(img)
    offs, count = lzip.scan(ctx, d_img)
    assert count >= len(ms) and {m["off"] for m in ms} <= {int(o) for o in offs}       # (a match is a candidate: there may be more)
    entries, dst = [], 0
    for m in ms:
        entries.append({"src_off": m["off"] + 6, "src_end": m["off"] + m["member_size"] - 20, "data_size": m["data_size"], "dst_off": dst,
                        "dst_cap": m["data_size"], "dict_size": lzip.dict_size(m["dict_byte"]), "crc32": m["crc"]})
        dst += m["data_size"]
    res, plan = lzip.decode_members(ctx, img, entries)
    assert [int(s) for s in res["status"]] == [0] * len(ms)
    assert [int(c) for c in res["crc32"]] == [m["crc"] for m in ms]
    assert plan.output() == data
    assert W.digest(img) == W.golden()["%s/%d" % (name, level)], "the device's bytes are not the stand-in's"
    return ms, img


@pytest.mark.parametrize("level", W.LEVELS)
@pytest.mark.parametrize("name", sorted(W.inputs()))
def test_named_inputs(gpu_ctx, name, level):
    ms, img = decodes(gpu_ctx, name, level)
    n, m = len(W.inputs()[name]), lzip.member_bytes(level)
    assert m == W.member_bytes(level) and len(ms) == max(1, -(-n // m))
    if n % m == 1:
        assert ms[-1]["data_size"] == 1         # a one-byte last member


def test_the_empty_member_comes_from_the_kernels(gpu_ctx):
    ms, img = decodes(gpu_ctx, "empty", 6)
    assert len(ms) == 1 and len(img) == 26 + len(ms[0]["stream"]) and ms[0]["crc"] == 0


def test_noise_expands_and_stays_under_the_bound(gpu_ctx):
    data = W.inputs()["noise_2m5"]
    for level in W.LEVELS:
        img = compress(gpu_ctx, data, level)
        assert len(data) < len(img) <= W.bound(len(data), level)


def test_the_large_member_reaches_the_far_pair(gpu_ctx):
    data = W.inputs()["far_pair"]
    assert len(compress(gpu_ctx, data, 9)) < len(compress(gpu_ctx, data, 6))


def test_levels_are_refused_above_9(gpu_ctx):
    assert lzip.member_bytes(10) == 0 and lzip.compress_bound(100, 10) == 0
    with pytest.raises(Exception):
        lzip.compress_window(gpu_ctx, dev(b"abc"), 10, out_cap=64)


@pytest.mark.parametrize("level", W.LEVELS)
def test_short_output_buffer(gpu_ctx, level):
    """la_gpu_xz_compress's way: *d_out_bytes is the size needed, nothing is written at or behind out_cap"""
    data = W.inputs()["text_noise_text"]
    img = compress(gpu_ctx, data, level)
    for cap in (0, 5, 6, 25, len(img) - 1):
        d_out = torch.full((len(img) + 64,), 0xA5, dtype=torch.uint8, device="cuda")
        _, need = lzip.compress_window(gpu_ctx, dev(data), level, out_cap=cap, d_out=d_out)
        got = d_out.cpu().numpy().tobytes()
        assert need == len(img) > cap
        assert got[:cap] == img[:cap]
        assert got[cap:] == b"\xa5" * (len(got) - cap)
