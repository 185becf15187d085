"""The xz test builders against the image's liblzma: what xz_build writes -- containers with every header option,
hand-built packets and chunk plans -- is accepted with the intended bytes, what it writes wrong on purpose is refused,
and the emulator (xz_support.reference_read) agrees with Python's lzma where both apply."""
import lzma

import pytest

import xz_build as XB
import xz_support as XS


def raw_decode(raw, dict_size=1 << 21):
    return lzma.decompress(raw, format=lzma.FORMAT_RAW, filters=[{"id": lzma.FILTER_LZMA2, "dict_size": dict_size}])


@pytest.mark.parametrize("family", ["packet_cases", "chunk_plans"])
def test_hand_built_data_is_what_it_stands_for(family):
    for name, (raw, plain) in getattr(XS, family)().items():
        assert raw_decode(raw) == plain, name
        assert XS.reference_read(XS.wrap(raw, plain, XB.CHECK_CRC64)) == (plain, 0, ""), name


def dist_slot(d0):
    return d0 if d0 < 4 else 2 * (d0.bit_length() - 1) + ((d0 >> (d0.bit_length() - 2)) & 1)


def test_the_packet_cases_hit_what_they_name():
    """derived from the packet lists themselves: every rep kind and short rep; lengths 2, 9, 10, 17, 18, 273; distances
    1, 4, 127, 128, one in slot 14 or above with nonzero align bits, one equal to the bytes produced so far"""
    XS.packet_cases()
    log = XS.PACKET_LOG
    reps = [pk for pk, _ in log["reps"]]
    assert {pk.index for pk in reps if isinstance(pk, XB.Rep)} == {0, 1, 2, 3}
    assert any(isinstance(pk, XB.ShortRep) for pk in reps)
    for name in ("reps", "lengths"):    # the three length ranges' edges, through the rep-length and the match-length coder
        kind = XB.Rep if name == "reps" else XB.Match
        assert {2, 9, 10, 17, 18, 273} <= {pk.len for pk, _ in log[name] if isinstance(pk, kind)}, name
    matches = [(pk, pos) for pk, pos in log["distances"] if isinstance(pk, XB.Match)]
    assert {1, 4, 127, 128} <= {pk.dist for pk, _ in matches}
    assert any(dist_slot(pk.dist - 1) >= 14 and (pk.dist - 1) & 15 for pk, _ in matches)
    assert any(dist_slot(pk.dist - 1) >= 14 and (pk.dist - 1) >> 4 and (pk.dist - 1) & 15 == 15 for pk, _ in matches)
    slots = {dist_slot(pk.dist - 1) for pk, _ in matches}     # slots 0..3, reverse trees, direct bits and align
    assert {0, 3} <= slots and any(4 <= k < 14 for k in slots) and {14, 15} <= slots and max(slots) >= 32
    assert any(pk.dist == pos and pos > 0 for pk, pos in matches)
    # the chunk plans: a chunk of 2 MiB, one of 65 536 compressed bytes, every control byte
    raw, plain = XS.chunk_plans()["chunk_2mib"]
    assert raw[0] == 0xE0 | 0x1F and raw[1:3] == b"\xff\xff" and len(plain) > 1 << 21
    raw, _ = XS.chunk_plans()["chunk_65536_compressed"]
    assert raw[3:5] == b"\xff\xff"
    raw, _ = XS.chunk_plans()["every_kind"]
    assert raw[0] == 1


def test_refusals_are_refused_by_liblzma():
    for name, (raw, _) in XS.refusals().items():
        assert XS.reference_read(XS.wrap(raw)) == (b"", -30, XS.DATA_ERROR), name
    for name, (raw, valid, ok, dict_byte) in XS.beyond_cases().items():
        got = XS.reference_read(XS.wrap(raw, valid if ok else b"", dict_byte=dict_byte))
        assert got == ((valid, 0, "") if ok else (b"", -30, XS.DATA_ERROR)), name


def test_container_shapes_against_python_lzma():
    shapes = XS.filter_shapes()
    for name, img in shapes.items():
        if any(w in name for w in ("padd", "garbage", "second_stream", "three_streams")):
            continue        # (Python's lzma walks the streams itself and stops at what it cannot open: not liblzma's verdict)
        data, rc, msg = XS.reference_read(img)
        try:
            want = lzma.decompress(img)
        except lzma.LZMAError:
            assert rc == -30, name
            continue
        assert (data, rc, msg) == (want, 0, ""), name
    # the verdicts the shapes are named after
    for name, msg in (("padding_of_three", XS.DATA_ERROR), ("trailing_garbage", XS.DATA_ERROR), ("trailing_garbage_short", XS.BUF_ERROR),
                      ("header_reserved_flag", XS.OPTIONS_ERROR), ("index_records_swapped_sums_equal", XS.DATA_ERROR),
                      ("wrong_sha256", XS.DATA_ERROR), ("header_comp_size_too_small", XS.DATA_ERROR)):
        assert XS.reference_read(shapes[name])[1:] == (-30, msg), name
    for name in ("check_unknown_id_2", "seventy_blocks_bare", "three_streams_padded", "empty_stream", "one_byte_blocks"):
        assert XS.reference_read(shapes[name])[1] == 0, name


def test_truncation_is_no_progress_not_truncated_input():
    img = XS.stream3000()
    for cut in (6, 11, 12, 13, 30, 1000, len(img) - 13, len(img) - 1):
        assert XS.reference_read(img[:cut])[1:] == (-30, XS.BUF_ERROR), cut
    assert XS.reference_read(img)[1] == 0
    assert len(XS.flip_cases()) > 2500
