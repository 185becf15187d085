"""The lzip encoder's rules (libarchive_amd/csrc/la_lzip_enc_dev.h over la_xz_enc_dev.h) through the ABI entry of the CPU
stand-in, which compiles those headers: every named input at one level of each group and at level 0 passes the checks of
a written stream (liblzma as the reader), and over the whole set the headers' event hook must have seen every symbol
kind the encoder can write, the end marker among them."""
import pytest

import lzip_support as LS
import lzip_write_support as W


@pytest.fixture(scope="module")
def stand_in():
    return W.StandIn()


@pytest.fixture(scope="module")
def images(stand_in):
    """(name, level) -> image, coded once; the event counters then hold the whole set's"""
    stand_in.events(reset=True)
    return {(name, level): stand_in.compress(data, level) for name, data in sorted(W.inputs().items()) for level in (0, 6, 9)}


@pytest.mark.parametrize("level", [0, 6, 9])
@pytest.mark.parametrize("name", sorted(W.inputs()))
def test_named_inputs_are_accepted(images, name, level):
    W.accept(images[name, level], W.inputs()[name], level)


def test_the_set_reaches_every_rule(stand_in, images):
    ev = stand_in.events()
    print(ev)
    for name in W.EVENTS:
        if name in ("stored", "across_chunks"):     # LZMA2's own: lzip has no stored form and nothing in front of a member
            assert ev[name] == 0, name
        else:
            assert ev[name] > 0, name
    members = sum(len(W.walk(img)) for img in images.values())
    assert ev["marker"] == members


def test_the_empty_member(stand_in):
    img = stand_in.compress(b"", 6)
    (m,) = W.walk(img)
    assert m["data_size"] == 0 and m["crc"] == 0 and m["member_size"] == len(img) == 6 + len(m["stream"]) + 20
    assert img[:6] == b"LZIP\x01\x10"
    assert LS.liblzma_raw(m["stream"], 0x10, 64) == (b"", True, len(m["stream"]))
    assert LS.reference_read(img) == (b"", 0, "")


def test_bound_is_the_headers_arithmetic(stand_in):
    for level, m in ((0, W.M), (6, W.M), (7, W.BIG), (9, W.BIG)):
        assert stand_in.member_bytes(level) == m
        for n in (0, 1, W.M, W.M + 1, m, m + 1, 1 << 30):
            members = max(1, -(-n // m))
            assert stand_in.bound(n, level) == W.bound(n, level) == 7 * n + (64 + 26) * members, (n, level)
    assert stand_in.member_bytes(10) == 0 and stand_in.bound(5, 10) == 0


def test_levels_write_the_same_bytes_within_a_group(stand_in):
    data = W.inputs()["far_pair"]
    outs = [stand_in.compress(data, lv) for lv in range(10)]
    assert len(set(outs[:7])) == 1 and len(set(outs[7:])) == 1 and outs[0] != outs[7]


def test_the_large_member_reaches_the_far_pair(stand_in):
    """the second marker lies 200 000 bytes behind the first: a match at level 9, forty literals at level 6"""
    data = W.inputs()["far_pair"]
    assert len(stand_in.compress(data, 9)) < len(stand_in.compress(data, 6))


def test_refusals_and_short_buffers(stand_in):
    data = W.inputs()["text_noise_text"]
    assert stand_in.call(data, 10)[0] != 0 and stand_in.call(data, 6, flags=1)[0] != 0
    img = stand_in.compress(data, 6)
    for cap in (0, 5, 6, 25, len(img) - 1):
        rc, need, got = stand_in.call(data, 6, cap=cap)
        assert rc == 0 and need == len(img) and got == img[:cap]
