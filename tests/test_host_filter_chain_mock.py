"""CPU-only: the gzip read filter's chain mode (LA_GZIP_FLUSH_POINTS=chain) END TO END against tests/mock_gpu, whose
LA_GZ_OPT_PIECES | LA_GZ_OPT_CHAIN answers come from zlib -- the test functions of tests/test_gpu_filter_chain.py, as
tests/test_host_filters_mock.py runs those of the other filter tests."""

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
from test_gpu_filter_chain import (  # noqa: E402,F401
    plain, sync_member, chain_mode,
    test_sync_flush_member_with_name_and_mtime_across_windows,
    test_member_that_turns_dependent,
    test_damage_in_the_fourth_window,
    test_cut_behind_a_flush_point,
    test_trailer_mismatch,
    test_second_member_behind_the_trailer,
    test_slots_grow_until_the_piece_fits,
    test_slot_limit_refuses_the_piece_that_cannot_fit,
    test_no_flush_point_within_the_widest_window,
    test_pieces_right_behind_members_that_asked_for_a_retry,
)
