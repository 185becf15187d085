"""The CPU stand-in of tests/mock_gpu/la_gpu_lzip_comp_mock.c reproduces tests/golden/lzip_write_digests.json (recorded from it by
tools/record_lzip_write_digests.py); tests/test_gpu_lzip_compress.py holds the device to the same file, which pins kernel
and stand-in to the same bytes."""
import pytest

import lzip_write_support as W


@pytest.fixture(scope="module")
def stand_in():
    return W.StandIn()


def test_every_input_is_recorded():
    assert sorted(W.golden()) == sorted("%s/%d" % (n, lv) for n in W.inputs() for lv in W.LEVELS)


@pytest.mark.parametrize("level", W.LEVELS)
@pytest.mark.parametrize("name", sorted(W.inputs()))
def test_stand_in_reproduces_the_golden(stand_in, name, level):
    data = W.inputs()[name]
    out = stand_in.compress(data, level)
    assert W.digest(out) == W.golden()["%s/%d" % (name, level)]
    assert len(out) <= stand_in.bound(len(data), level)
