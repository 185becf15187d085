"""CPU-only: the gzip read filter's piece mode (LA_GZIP_FLUSH_POINTS=1) END TO END against tests/mock_gpu, whose
LA_GZ_OPT_PIECES answers come from zlib -- the test functions of tests/test_gpu_filter_flush_points.py, as
tests/test_host_filters_mock.py runs those of the other filter tests.  (test_own_writer_single_member_over_several_windows
stays with the device: the mock's gzip writer stores one member per chunk and cannot write a flush-pointed member.)"""

import pytest

import la_api
import mock_build


@pytest.fixture(scope="module")
def gpu_ctx():
    """Same name as the GPU fixture on purpose: the imported tests ask for it."""
    la_api.use_library(mock_build.host_lib())
    yield None
    la_api.use_library(None)


# the fixtures and the test functions themselves (their module-level `gpu` mark stays behind in that module)
from test_gpu_filter_flush_points import (  # noqa: E402,F401
    plain, full_member, piece_mode,
    test_zlib_full_flush_with_name_and_mtime,
    test_false_marker_in_stored_data_merges_the_pieces,
    test_sync_flush_stream_falls_back,
    test_member_that_turns_dependent_is_refused_by_name,
    test_damage_cut_and_trailer,
    test_what_follows_the_trailer,
    test_slots_grow_until_the_piece_fits,
    test_slot_limit_refuses_the_piece_that_cannot_fit,
    test_span_limit_refuses_the_piece_that_is_too_long,
    test_no_flush_point_within_the_widest_window,
    test_pieces_right_behind_members_that_asked_for_a_retry,
)
