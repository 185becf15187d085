"""The zstd write filter's compression levels (host/la_write_zstd.c): 0 and below write raw literals, 1 and 2 are the
fast coder (Huffman literals only for alphabets up to byte 128, predefined sequence tables), 3 and above -- the default
among them -- set LA_ZSTDC_FULL_ALPHABET | LA_ZSTDC_FIT_TABLES.  Read from what archive_write_add_filter_zstd writes
for 1 MiB of a skewed 256-symbol source, whose literals the fast coder cannot Huffman-code; every level's stream must
read back through libzstd, the oracle and this repository's read path."""
import random

import pytest

import la_api
import zstd_entropy_inputs as I
import zstd_parse_modes as PM
import zstd_support as Z
from test_gpu_lz4_write import ARCHIVE_OK
from test_gpu_zstd_write import write_zstd

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def skewed():
    return I.skewed256(random.Random(0x1E7E1), 1 << 20)


@pytest.mark.parametrize("level", ["0", "1", "2", "3", None, "19"], ids=lambda v: "level-%s" % (v or "default"))
def test_levels_choose_the_coder(gpu_ctx, skewed, level):
    z, o = Z.libzstd(), Z.oracle_lib()
    assert z is not None
    rc, img = write_zstd(skewed, (("compression-level", level),) if level else (), 99991)
    assert rc == ARCHIVE_OK and isinstance(img, bytes), img
    assert Z.zstd_decompress(z, img, len(skewed) + 16) == skewed
    assert Z.oracle_decode(o, img, len(skewed) + 16) == (0, skewed, "")
    r = la_api.cat(img)
    assert r.filters[0] == (14, "zstd") and r.data == skewed, r.error
    frames = PM.parse(img)
    assert PM.plain_of(frames) == skewed and len(frames) == 8
    blocks = [b for f in frames for b in f["blocks"]]
    lit_types = {b["lit"]["type"] for b in blocks if b["type"] == 2}
    if level == "0":
        assert lit_types <= {0}                                    # raw literals (or whole raw blocks)
    elif level in ("1", "2"):
        assert lit_types <= {0, 1}                                 # bytes above 128: the fast coder leaves them raw
    else:
        assert all(b["type"] == 2 for b in blocks) and lit_types == {2}
        assert all(b["lit"]["tree"] == "fse" and len(b["lit"]["weights"]) == 255 for b in blocks)
        assert len(img) < len(skewed)
