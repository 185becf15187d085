"""la_gpu_bzip2_compress through the C ABI: every output must decode to the input by libbz2 1.0.8 (bz2.decompress, at
eof, nothing unused) and by this repository's device reader (libarchive_amd.bzip2.decode_image), and must hold exactly
ceil(n / block_bytes) blocks.  The inputs are the smallest that reach each rule of the format and of the kernels: RLE1
run lengths and cuts, the sort's tie rounds, the table-count thresholds, the 50-symbol group, the 17-bit length limit,
RUNA / RUNB run lengths, the output bound, the state carried between calls, a short output buffer.

(An incompressible level-9 block has at most 719 984 + 1 symbols under the fixed input cut, so 14 400 selectors; the
format's 18 001 are out of reach of any cut that must leave room for RLE1's worst case.)"""
import bz2
import random

import numpy as np
import pytest
import torch

import bzip2_parse as P
import bzip2_support as BS
from libarchive_amd import bzip2 as B

pytestmark = pytest.mark.gpu
FIRST, LAST = B.LA_BZ2C_FIRST, B.LA_BZ2C_LAST


def block_bytes(level):
    return 4 * ((100000 * level - 19) // 5)


def dev(data):
    if not data:
        return torch.zeros(0, dtype=torch.uint8, device="cuda")
    return torch.from_numpy(np.frombuffer(data, dtype=np.uint8).copy()).cuda()


def compress(ctx, data, level, **kw):
    return B.compress_to_stream(ctx, dev(data), level, **kw).cpu().numpy().tobytes()


def check(ctx, data, level):
    assert B.compress_block_bytes(level) == block_bytes(level)
    img = compress(ctx, data, level)
    assert len(img) <= B.compress_bound(len(data), level)
    assert img[:4] == b"BZh%d" % level
    dec = bz2.BZ2Decompressor()
    assert dec.decompress(img) == data and dec.eof and dec.unused_data == b""
    magics = BS.find_magics(img)
    assert [k for _, k in magics] == [0] * -(-len(data) // block_bytes(level)) + [1]
    out, results, st, _ = B.decode_image(ctx, img)
    assert out == data and all(int(r["status"]) == 0 for r in results)
    return img


BB1 = block_bytes(1)
SMALL = {
    "len0": b"", "len1": b"q", "len2": b"qr", "len3": b"qrs",
    **{"run%d" % n: b"z" * n for n in (3, 4, 5, 258, 259, 260, 263, 264, 600)},
    "ends_on_four": b"hello" + b"y" * 4,
    "ends_on_four_after_255": b"k" * 259,
    "all256": bytes(range(256)),
    "one_value": b"\x07" * 1000,
    "two_symbols": bytes(random.Random(3).choice(b"01") for _ in range(3000)),
}


@pytest.mark.parametrize("level", [1, 9])
@pytest.mark.parametrize("name", sorted(SMALL))
def test_small_inputs(gpu_ctx, name, level):
    img = check(gpu_ctx, SMALL[name], level)
    if name == "len0":
        assert len(img) == 14 and img == bz2.compress(b"", level)
    if name == "one_value":
        blk = P.blocks(img)[0]
        assert blk["n_tables"] >= 2 and blk["n_selectors"] >= 1     # libbz2's reader refuses fewer


@pytest.mark.parametrize("level", [1, 9])
def test_run_straddling_the_cut(gpu_ctx, level):
    """RLE1 restarts at the cut: a run of 10 across it is two runs, in two blocks"""
    bb = block_bytes(level)
    data = BS.letters(5, bb - 4, 7) + b"Q" * 10 + BS.letters(6, 500, 7)
    check(gpu_ctx, data, level)


@pytest.mark.parametrize("period", [1, 2, 5, 251])
def test_periodic_full_block(gpu_ctx, period):
    """rotations that stay tied through every doubling round; origPtr is one of several equal rows"""
    unit = bytes(random.Random(period).sample(range(256), period))
    data = (unit * (BB1 // period + 1))[:BB1]
    check(gpu_ctx, data, 1)


@pytest.mark.parametrize("level", [1, 5, 9])
def test_rle1_worst_expansion_fills_the_block(gpu_ctx, level):
    """aaaab: five RLE1 bytes per four of input, 100000 x level - 19 - 1 symbols at most in a block"""
    bb = block_bytes(level)
    src = b"aaaab" * (2 * bb // 5 + 1)
    for n in (bb, bb - 1, bb + 1, 2 * bb):
        check(gpu_ctx, src[:n], level)


def _input_with_symbols(target, seed):
    """bytes whose single block has exactly `target` MTF / RLE2 symbols (by the Python model)"""
    rnd = random.Random(seed)
    data = bytearray(rnd.randrange(200) for _ in range(max(target - 2, 1)))
    for _ in range(400):
        n = len(P.model_symbols(bytes(data)))
        if n == target:
            return bytes(data)
        if n < target:
            data.append(rnd.randrange(200))
        else:
            data.pop()
    raise AssertionError("no input with %d symbols found" % target)


@pytest.mark.parametrize("nsym", [49, 50, 51, 199, 200, 599, 600, 1199, 1200, 2399, 2400])
def test_table_count_thresholds_and_group_boundary(gpu_ctx, nsym):
    data = _input_with_symbols(nsym, nsym)
    for level in (1, 9):
        blk = P.blocks(check(gpu_ctx, data, level), symbols=True)[0]
        assert blk["symbols"] == P.model_symbols(data)      # the symbol stream is the format's, so libbz2's too
        assert blk["n_selectors"] == -(-nsym // 50)
        assert blk["n_tables"] == (2 if nsym < 200 else 3 if nsym < 600 else 4 if nsym < 1200 else 5 if nsym < 2400 else 6)
        assert all(1 <= l <= 17 for row in blk["lengths"] for l in row)


def test_geometric_frequencies_stay_within_17_bits(gpu_ctx):
    """24 values, each half as frequent as the one before, one level-9 block.  An unlimited Huffman code for the
    block's symbol counts is deeper than 17 (asserted from the parsed symbols: 19 for this input), so the source is as
    long as the rule asks; no written length may pass 17.  Whether a TABLE's own code had to be limited depends on the
    counts of the groups that chose it, about a sixth of the block each: their unlimited depths are printed (15 to 17
    for this input under libbz2's own choice of groups), and a table whose depth passes 17 must still be written
    with 17 at most."""
    n = block_bytes(9)
    parts = [np.full(max(n >> (k + 1), 1), 65 + k, dtype=np.uint8) for k in range(24)]
    a = np.concatenate(parts)[:n]
    a = np.concatenate([a, np.full(n - a.size, 65, dtype=np.uint8)])
    np.random.RandomState(24).shuffle(a)
    img = check(gpu_ctx, a.tobytes(), 9)
    blk = P.blocks(img, symbols=True)[0]
    assert blk["n_tables"] == 6
    per_table = P.table_counts(blk)
    whole = [sum(c) for c in zip(*per_table)]
    depths = [P.huffman_depth(c) for c in per_table]
    longest = [max(row) for row in blk["lengths"]]
    print("unlimited depth, whole block:", P.huffman_depth(whole), "per table:", depths, "longest written:", longest)
    assert P.huffman_depth(whole) > 17
    assert max(longest) <= 17 and min(l for row in blk["lengths"] for l in row) >= 1


@pytest.mark.parametrize("level", [1, 9])
def test_zero_run_lengths(gpu_ctx, level):
    """one repeated word: "ab" x (r + 1) sorts to b..ba..a, two zero runs of r; RUNA / RUNB digits for 1..17, 1023, 1024"""
    seen = set()
    for r in list(range(1, 18)) + [1023, 1024]:
        data = b"ab" * (r + 1)
        blk = P.blocks(check(gpu_ctx, data, level), symbols=True)[0]
        assert blk["symbols"] == P.model_symbols(data)
        assert r in blk["zero_runs"]
        seen.update(blk["zero_runs"])
    assert seen >= set(range(1, 18)) | {1023, 1024}


def test_incompressible_level9_block_fits_the_bound(gpu_ctx):
    n = block_bytes(9)
    data = np.random.RandomState(256).randint(0, 256, n, dtype=np.uint8).tobytes()
    img = check(gpu_ctx, data, 9)
    blk = P.blocks(img, symbols=True)[0]
    assert len(img) > n                                  # it did not compress
    assert len(img) <= B.compress_bound(n, 9)
    assert n - n // 64 < len(blk["symbols"]) <= n + 1    # about one symbol per byte
    assert blk["n_selectors"] == -(-len(blk["symbols"]) // 50) == 14400
    assert blk["n_tables"] == 6


def test_split_calls_write_the_same_bytes(gpu_ctx):
    """one FIRST | LAST call against FIRST, middle, LAST calls of one block each, the state carried on the device"""
    data = BS.letters(21, BB1, 9) + BS.noise(22, BB1, 17) + BS.letters(23, BB1 - 333, 5)
    whole = compress(gpu_ctx, data, 1)
    state = torch.zeros(16, dtype=torch.uint8, device="cuda")
    pieces, nbits = [], []
    for i, flags in enumerate((FIRST, 0, LAST)):
        pieces.append(compress(gpu_ctx, data[i * BB1:(i + 1) * BB1], 1, flags=flags, state=state))
        nbits.append(int(state.cpu().numpy().view(B.BZ2C_STATE_DTYPE)[0]["nbits"]))
    assert b"".join(pieces) == whole
    assert nbits[2] == 0 and (nbits[0] != 0 or nbits[1] != 0), nbits
    assert nbits[1] != 0, nbits         # the middle call left bits pending
    assert bz2.decompress(whole) == data
    # an empty LAST call writes the trailer alone behind the pending bits
    state.zero_()
    head = compress(gpu_ctx, data[:BB1], 1, flags=FIRST, state=state)
    tail = compress(gpu_ctx, b"", 1, flags=LAST, state=state)
    assert bz2.decompress(head + tail) == data[:BB1]


@pytest.mark.parametrize("level", [1, 9])
def test_short_output_buffer(gpu_ctx, level):
    data = BS.noise(31, 5000, 30)
    img = compress(gpu_ctx, data, level)
    for cap in (0, 1, 15, 16, 17, len(img) - 1):
        d_out = torch.full((len(img) + 64,), 0xA5, dtype=torch.uint8, device="cuda")
        _, need = B.compress_to_stream(gpu_ctx, dev(data), level, out_cap=cap, d_out=d_out)
        got = d_out.cpu().numpy().tobytes()
        assert need == len(img)                          # the size needed
        assert got[:cap] == img[:cap]
        assert got[cap:] == b"\xa5" * (len(got) - cap)    # nothing past the cap


def test_state_stays_when_the_piece_does_not_fit(gpu_ctx):
    """a middle piece into too small a buffer reports its size and leaves the state alone: the same call again, with
    room, writes what one call would have written"""
    data = BS.letters(41, 2 * BB1, 8)
    whole = compress(gpu_ctx, data, 1)
    state = torch.zeros(16, dtype=torch.uint8, device="cuda")
    head = compress(gpu_ctx, data[:BB1], 1, flags=FIRST, state=state)
    before = state.cpu().numpy().tobytes()
    assert before != bytes(16)                               # the combined CRC so far, at the least
    _, need = B.compress_to_stream(gpu_ctx, dev(data[BB1:]), 1, flags=LAST, state=state, out_cap=10)
    assert need > 10 and state.cpu().numpy().tobytes() == before
    tail = compress(gpu_ctx, data[BB1:], 1, flags=LAST, state=state)
    assert len(tail) == need and head + tail == whole
    assert state.cpu().numpy().tobytes() == bytes(16)       # LAST, fitted: the state is cleared
