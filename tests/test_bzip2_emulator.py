"""tests/bzip2_support.reference_read -- the reference's bzip2 read loop restated over the real libbz2 -- against Python's
bz2 on valid streams and against the manifest of the reference's own fixtures (tests/golden/ref_fixtures/bzip2)."""
import bz2
import hashlib

import pytest

import bzip2_support as BS


def test_library_is_the_one_the_numbers_were_measured_with():
    assert BS.libbz2().BZ2_bzlibVersion().startswith(b"1.0.")


@pytest.mark.parametrize("name", sorted(BS.abi_cases()))
def test_valid_streams_decode_as_python_bz2_does(name):
    plain = BS.abi_cases()[name]
    for level in (1, 9):
        img = bz2.compress(plain, level)
        assert bz2.decompress(img) == plain
        for read_size in (None, 1000, 1):
            if read_size == 1 and len(img) > 4096:
                continue
            assert BS.reference_read(img, read_size) == (plain, 0, "")


def test_stream_shapes():
    img = BS.stream350k()
    plain = bz2.decompress(img)
    assert len(plain) == 350000 and len([1 for _, k in BS.find_magics(img) if k == 0]) == 4
    assert BS.reference_read(img + b"junk" * 9) == (plain, 0, "")
    assert BS.reference_read(img + bz2.compress(b"") + img, 1000) == (plain + plain, 0, "")
    for cut in (1, 4):
        assert BS.reference_read(img[:-cut]) == (plain[:5 * 65536], -30, "truncated bzip2 input")
    assert BS.reference_read(img[:len(img) // 2]) == (plain[:65536], -30, "truncated bzip2 input")


def test_single_bit_flips_are_refused_after_whole_blocks():
    import random
    img = BS.stream350k()
    r = random.Random(300)
    for _ in range(300):
        data, rc, msg = BS.reference_read(BS.flip(img, r.randrange(80, len(img) * 8)))
        assert (rc, msg) == (-30, "bzip decompression failed")
        assert len(data) % 65536 == 0 and len(data) <= 5 * 65536      # (whole blocks; the last may hold a damaged block's bytes)


def test_fixture_manifest():
    got = {}
    for m, img in BS.fixtures():
        assert len(img) == m["size"] and hashlib.sha256(img).hexdigest() == m["sha256"]
        data, rc, msg = BS.reference_read(img)
        assert (len(data), hashlib.sha256(data).hexdigest(), rc, msg) == (m["decoded_size"], m["decoded_sha256"], m["rc"], m["message"])
        got[m["file"]] = (len(data), hashlib.sha256(data).hexdigest()[:12], rc, msg)
    assert got["test_expand.bz2"][0] == 71
    assert got["test_compat_bzip2_1.tbz"][:3] == (7168, "7565705704f8", 0)
    assert got["test_compat_bzip2_2.tbz"][:3] == (7168, "7565705704f8", 0)
    assert got["test_extract.tar.bz2"][0] == 3072
    assert got["test_read_format_mtree_crash747.mtree.bz2"] == (131072, got["test_read_format_mtree_crash747.mtree.bz2"][1], -30, "bzip decompression failed")
