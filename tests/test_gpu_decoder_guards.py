"""The guard-band case tables (tests/decoder_guard_cases.py) through the five device calls: la_gpu_lzop_decode,
la_gpu_lzip_decode, la_gpu_xz_decode with and without filter chains, la_gpu_bzip2_decode (MEASURE and EMIT, by the
parallel and the serial chase) and la_gpu_uu_decode.

Every call decodes into a destination prefilled with one byte, 4 KiB of guard on both sides
(guard_support.GuardedBuffer), and is judged by decoder_guard_cases.judge: status, out_len and bytes against the
references the tables were built from, nothing changed outside the slots the rules allow.  Every call runs twice
(guard_support.two_fills): over 0xA5 and over 0x5A, with other bytes in the source allocation behind src_bytes; the
result records and the bytes must not depend on either.  tests/test_decoder_guard_cases.py runs the same tables through
the CPU stand-ins.

include/la_gpu.h states no alignment for d_src or d_dst of any of the five calls, so both base addresses are moved off
the 16-byte grid: the destination by 0, 1 and 15 bytes, the source by 0 and 3."""
import pytest

import decoder_guard_cases as D

pytestmark = pytest.mark.gpu

SHIFTS = [(d, s) for d in (0, 1, 15) for s in (0, 3)]
IDS = ["dst%d_src%d" % p for p in SHIFTS]


class DeviceBackend:
    device = "cuda"

    def __init__(self, ctx, bz2_options=0):
        self.ctx, self.bz2_options = ctx, bz2_options

    def decode(self, call, src, dst):
        return getattr(self, call.decoder)(call, src, dst)

    @staticmethod
    def _answer(res):
        return D.rows(res), [(int(r["status"]), int(r["out_len"])) for r in res]

    def lzop(self, call, src, dst):
        from libarchive_amd import lzop
        return self._answer(lzop.LzopDevicePlan(self.ctx, src.data, call.table, dst_cap=dst.total, d_dst=dst.data).run().results())

    def lzip(self, call, src, dst):
        from libarchive_amd import lzip
        return self._answer(lzip.LzipDevicePlan(self.ctx, src.data, call.table, dst_cap=dst.total, d_dst=dst.data).run().results())

    def xz(self, call, src, dst):
        from libarchive_amd import xz
        return self._answer(xz.XzDevicePlan(self.ctx, src.data, call.table, dst_cap=dst.total, d_dst=dst.data).run().results())

    def xz_chains(self, call, src, dst):
        from libarchive_amd import xz
        plan = xz.XzDevicePlan(self.ctx, src.data, call.table, dst_cap=dst.total, chains=call.opts["chain_lists"], d_dst=dst.data)
        return self._answer(plan.run().results())

    def bzip2(self, call, src, dst):
        from libarchive_amd import bzip2
        plan = bzip2.Bz2DevicePlan(self.ctx, src.data, call.table, slot_level=1, options=self.bz2_options)
        plan.measure()
        state = plan.emit(n_emit=call.opts["n_emit"], dst_cap=call.opts["dst_cap"], d_dst=dst.data)
        res = plan.results()
        return D.rows(res) + [tuple(int(state[k]) for k in state.dtype.names)], [(int(r["status"]), int(r["out_len"])) for r in res]

    def uu(self, call, src, dst):
        from libarchive_amd import uu
        plan = uu.UuDevicePlan(self.ctx, src.data, dst.data).run(call.opts["state"], call.opts["decoded"], call.opts["final"])
        r = plan.result()
        D.uu_record_check(call, {k: int(r[k]) for k in r.dtype.names})
        return [tuple(int(r[k]) for k in r.dtype.names)], [(int(r["status"]), int(r["out_len"]))]


@pytest.fixture(scope="module")
def device(gpu_ctx):
    return DeviceBackend(gpu_ctx)


@pytest.mark.parametrize("shift", SHIFTS, ids=IDS)
def test_lzop(device, shift):
    """768 stored blocks at every (length 1 .. 48, address residue) pair with guard gaps between them, the failing streams
    each directly in front of a good block, refusals and sums: one call.  Status OK: the exact rule."""
    D.run_guarded(D.lzop_call(), device, *shift)


@pytest.mark.parametrize("shift", SHIFTS, ids=IDS)
def test_lzip(device, shift):
    """members of 1 .. 48 bytes back to back, the 273-byte match and rep cut by dst_cap and by data_size, refusals, a wrong
    CRC: one call.  Status OK: the exact rule."""
    D.run_guarded(D.lzip_call(), device, *shift)


@pytest.mark.parametrize("shift", SHIFTS, ids=IDS)
def test_xz(device, shift):
    """blocks of 1 .. 48 bytes back to back with and without sizes, the LZMA2 plan cut by dst_cap at every kind of symbol
    and by a header size, an LZMA error in mid-block, refusals: one call.  Status OK: the exact rule."""
    D.run_guarded(D.xz_call(), device, *shift)


@pytest.mark.parametrize("shift", SHIFTS, ids=IDS)
def test_xz_chains(device, shift):
    """every block with a chain packed against a neighbour without one: each filter at the sizes around its tile, blocks
    that end inside a unit of their filter whose rest opens the neighbour, delta with a length the distance does not
    divide, failed blocks with chains in front of good ones, chains the ABI refuses: one call.  Status OK: the exact rule."""
    D.run_guarded(D.xz_chains_call(), device, *shift)


@pytest.mark.parametrize("options", [0, 1], ids=["parallel_chase", "serial_chase"])      # LA_BZ2_OPT_SERIAL_CHASE
@pytest.mark.parametrize("shift", SHIFTS, ids=IDS)
def test_bzip2(gpu_ctx, shift, options):
    """MEASURE and EMIT of 43 blocks of 1 .. 40 bytes and more with dst_cap at, one short of and far below the total and
    at 0, n_emit short of the table, a run of 4 + 255, refuted candidates between confirmed ones, the block without its
    count in front of a good one, a block MEASURE refuses: [dst_off, dst_off + out_len) of each emitted block exactly."""
    backend = DeviceBackend(gpu_ctx, options)
    for call in D.bzip2_calls():
        D.run_guarded(call, backend, *shift)


@pytest.mark.parametrize("shift", SHIFTS, ids=IDS)
def test_uu(device, shift):
    """every decoded total 0 .. 48 in both encodings, groups of lines at every output residue, both ways through the
    decode kernel (LDS and global), a walk that stops in mid-window, open tails: one call each.  [0, out_len) exactly."""
    for call in D.uu_calls():
        D.run_guarded(call, device, *shift)
