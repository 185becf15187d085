"""The CPU stand-in of tests/mock_gpu/la_gpu_xz_comp_mock.c reproduces tests/golden/xz_write_digests.json (recorded from it by
tools/record_xz_write_digests.py); tests/test_gpu_xz_compress.py holds the device to the same file, which pins kernel
and stand-in to the same bytes.  Every recorded image also passes the checks of a written stream."""
import pytest

import xz_parse as XP
import xz_write_support as W


@pytest.fixture(scope="module")
def stand_in():
    return W.StandIn()


def test_every_input_is_recorded():
    assert sorted(W.golden()) == sorted("%s/%d" % (n, lv) for n in W.inputs() for lv in (0, 6))


@pytest.mark.parametrize("level", [0, 6])
@pytest.mark.parametrize("name", sorted(W.inputs()))
def test_stand_in_reproduces_the_golden(stand_in, name, level):
    data = W.inputs()[name]
    out = stand_in.compress(data, level)
    assert W.digest(out) == W.golden()["%s/%d" % (name, level)]
    assert len(out) <= stand_in.bound(len(data), level)
    W.accept(XP.frame(out), data)


def test_levels_share_bytes_up_to_the_warm_up(stand_in):
    """levels 0..3 are one coder, levels 4..9 another"""
    data = W.inputs()["border_marker"]
    outs = [stand_in.compress(data, lv) for lv in range(10)]
    assert len(set(outs[:4])) == 1 and len(set(outs[4:])) == 1 and outs[0] != outs[4]


def test_without_first_the_stream_header_is_left_out(stand_in):
    data = W.inputs()["chunk_plus_1"]
    assert stand_in.compress(data, 6, flags=0) == stand_in.compress(data, 6)[12:]


def test_a_match_across_the_chunk_border_is_taken_from_level_4_on(stand_in):
    """the event hook of the rules header: a candidate in front of the chunk's start, never at levels 0..3"""
    data = W.inputs()["border_marker"]
    for level, crossed in ((0, False), (3, False), (4, True), (6, True)):
        stand_in.events(reset=True)
        stand_in.compress(data, level)
        assert (stand_in.events()["across_chunks"] > 0) == crossed, level
