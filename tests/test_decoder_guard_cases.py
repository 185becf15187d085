"""The guard-band case tables (tests/decoder_guard_cases.py) on the CPU: every table is built -- which checks every
expectation against its reference and that the table reaches the statuses, residues and paths it claims -- and run
through the CPU stand-ins of tests/mock_gpu over host memory, under the same GuardedBuffer, two_fills and rule asserts
as on the device (tests/test_gpu_decoder_guards.py).

The stand-ins of lzop, lzip, xz (with and without chains: la_gpu_xz_chains_mock.c decodes a batch without the chain
table as it stands, so plain xz is modelled too) and uu compile the kernels' own rules headers (la_lzo_dev.h,
la_xz_dev.h, la_lzip_dev.h, la_xz_filters_dev.h, la_uu_dev.h), so this pins those headers to the rules and shows that
the asserts pass on a correct implementation.  The bzip2 stand-in is libbz2 behind the ABI's walk: it pins no kernel
code, only the tables and the asserts; it does not model the block that ends on four equal bytes without their count
(it takes a block's length from one call of libbz2, which is a byte short there), so that one call runs on the device
only."""
import ctypes as C

import numpy as np
import pytest

import decoder_guard_cases as D
import guard_support as G
import mock_build
import uu_mock_build
from libarchive_amd import _native as N


class MockBackend:
    """the device ABI of a library that takes host pointers"""
    device = None

    def __init__(self):
        self.lib = mock_build.gpu_lib()
        self.uu_lib = None

    def _table_call(self, fn, batch_type, call, src, dst, result_dtype, flags=0, table=None):
        table = np.ascontiguousarray(call.table if table is None else table).view(np.uint8).reshape(-1).copy()
        n = len(call.units)
        res = np.zeros(max(n, 1), dtype=result_dtype)
        b = batch_type()
        b.d_src, b.src_bytes = src.ptr, src.n
        setattr(b, batch_type._fields_[2][0], table.ctypes.data)
        b.n, b.reserved = n, flags
        b.d_dst, b.dst_cap, b.d_results = dst.ptr, dst.total, res.ctypes.data
        fn.argtypes = [C.c_void_p, C.POINTER(batch_type)]
        assert fn(None, C.byref(b)) == 0
        res = res[:n]
        return D.rows(res), [(int(r["status"]), int(r["out_len"])) for r in res]

    def decode(self, call, src, dst):
        return getattr(self, call.decoder)(call, src, dst)

    def lzop(self, call, src, dst):
        return self._table_call(self.lib.la_gpu_lzop_decode, N._LzopBatchC, call, src, dst, N.LZOP_RESULT_DTYPE)

    def lzip(self, call, src, dst):
        return self._table_call(self.lib.la_gpu_lzip_decode, N._LzipBatchC, call, src, dst, N.LZIP_RESULT_DTYPE)

    def xz(self, call, src, dst):
        return self._table_call(self.lib.la_gpu_xz_decode, N._XzBatchC, call, src, dst, N.XZ_RESULT_DTYPE)

    def xz_chains(self, call, src, dst):
        table = np.concatenate([np.ascontiguousarray(call.table).view(np.uint8).reshape(-1),
                                np.ascontiguousarray(call.opts["chains"]).view(np.uint8).reshape(-1)])
        return self._table_call(self.lib.la_gpu_xz_decode, N._XzBatchC, call, src, dst, N.XZ_RESULT_DTYPE, N.LA_XZ_BATCH_CHAINS, table)

    def bzip2(self, call, src, dst):
        n = len(call.units)
        cands = np.ascontiguousarray(call.table).view(np.uint8).reshape(-1).copy()
        res, state = np.zeros(max(n, 1), dtype=N.BZ2_RESULT_DTYPE), np.zeros(1, dtype=N.BZ2_STATE_DTYPE)
        state_in = N._Bz2StateC()
        b = N._Bz2BatchC()
        b.d_src, b.src_bytes, b.d_cands, b.n = src.ptr, src.n, cands.ctypes.data, n
        b.d_results, b.d_state_out, b.state_in = res.ctypes.data, state.ctypes.data, C.pointer(state_in)
        b.options, b.slot_level = 0, 1
        fn = self.lib.la_gpu_bzip2_decode
        fn.argtypes = [C.c_void_p, C.POINTER(N._Bz2BatchC)]
        b.phase = N.LA_BZ2_MEASURE
        assert fn(None, C.byref(b)) == 0
        b.phase, b.d_dst, b.dst_cap, b.n_emit = N.LA_BZ2_EMIT, dst.ptr, call.opts["dst_cap"], call.opts["n_emit"]
        assert fn(None, C.byref(b)) == 0
        res = res[:n]
        return D.rows(res) + D.rows(state), [(int(r["status"]), int(r["out_len"])) for r in res]

    def uu(self, call, src, dst):
        if self.uu_lib is None:
            self.uu_lib = uu_mock_build.gpu_lib()
        res = np.zeros(1, dtype=N.UU_RESULT_DTYPE)
        b = N._UuBatchC()
        b.d_src, b.src_bytes = src.ptr, src.n
        b.final, b.reserved = 1 if call.opts["final"] else 0, 0
        b.state_in.state, b.state_in.decoded = call.opts["state"], 1 if call.opts["decoded"] else 0
        b.d_dst, b.dst_cap, b.d_result = dst.ptr, dst.total, res.ctypes.data
        fn = self.uu_lib.la_gpu_uu_decode
        fn.argtypes = [C.c_void_p, C.POINTER(N._UuBatchC)]
        assert fn(None, C.byref(b)) == 0
        D.uu_record_check(call, {k: int(res[0][k]) for k in res.dtype.names})
        return D.rows(res), [(int(res[0]["status"]), int(res[0]["out_len"]))]


@pytest.fixture(scope="module")
def mock():
    return MockBackend()


SHIFTS = [(0, 0), (1, 3), (15, 0)]      # (destination, source): the address residues of the two base pointers


def test_guarded_buffer_and_the_assert():
    """the tools themselves: the address residue, the guards, and a failure that names offset and slot"""
    for shift in (0, 1, 15):
        buf = G.GuardedBuffer(100, 0xA5, shift)
        assert buf.ptr % 16 == shift and len(buf.host()) == 2 * G.GUARD + shift + 100 and buf.data.ctypes.data == buf.ptr
        G.assert_only_slots_changed(buf, [])
        buf.data[10:20] = 7
        G.assert_only_slots_changed(buf, [(10, 10)])
        G.assert_only_slots_changed(buf, [(0, 30), (50, 5)])
        with pytest.raises(AssertionError, match=r"offset 19 \(data, address residue %d\) changed from fill 0xA5 to 0x07.*slot 1 \[10, 19\) ends nearest, \+0 bytes"
                           % ((shift + 19) % 16)):
            G.assert_only_slots_changed(buf, [(0, 3), (10, 9)])
        buf.whole[buf.lead - 1] = 1
        with pytest.raises(AssertionError, match=r"offset -1 \(front guard"):
            G.assert_only_slots_changed(buf, [(10, 10)])
        buf.whole[buf.lead - 1] = 0xA5
        buf.whole[buf.lead + 100] = 0
        with pytest.raises(AssertionError, match=r"offset 100 \(back guard"):
            G.assert_only_slots_changed(buf, [(10, 10)])
    src = G.SourceBuffer(b"abc", G.JUNK[0], 3)
    assert src.ptr % 16 == 3 and src.n == 3 and bytes(src.whole[3:]) == b"abc" + G.JUNK[0] and len(G.JUNK[1]) == G.JUNK_BYTES
    # two_fills: a stray value equal to one fill, and an answer that depends on the fill
    assert G.two_fills(lambda fill, junk: ([(0, 3)], [b"abc"])) == ([(0, 3)], [b"abc"])
    with pytest.raises(AssertionError, match="records depend"):
        G.two_fills(lambda fill, junk: ([(fill,)], [b""]))
    with pytest.raises(AssertionError, match="slot 0 depend"):
        G.two_fills(lambda fill, junk: ([(0,)], [junk[:2]]))


@pytest.mark.parametrize("shift", SHIFTS)
def test_lzop(mock, shift):
    D.run_guarded(D.lzop_call(), mock, *shift)


@pytest.mark.parametrize("shift", SHIFTS)
def test_lzip(mock, shift):
    D.run_guarded(D.lzip_call(), mock, *shift)


@pytest.mark.parametrize("shift", SHIFTS)
def test_xz(mock, shift):
    D.run_guarded(D.xz_call(), mock, *shift)


@pytest.mark.parametrize("shift", SHIFTS)
def test_xz_chains(mock, shift):
    D.run_guarded(D.xz_chains_call(), mock, *shift)


@pytest.mark.parametrize("shift", SHIFTS)
def test_bzip2(mock, shift):
    for call in D.bzip2_calls():
        if call.opts.get("stand_in_models_it", True):
            D.run_guarded(call, mock, *shift)


@pytest.mark.parametrize("shift", SHIFTS)
def test_uu(mock, shift):
    for call in D.uu_calls():
        D.run_guarded(call, mock, *shift)
