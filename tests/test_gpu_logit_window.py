"""In-graph logit processors through the engine on the GPU: decode windows
replay the processed graph variant (ModelRunner._ensure_processed_graph)."""

import pytest

from tests import logit_window_common as lw

pytestmark = pytest.mark.gpu


def test_windows_are_used():
    lw.check_windows_are_used("cuda")


def test_no_repeats_under_a_huge_presence_penalty():
    lw.check_no_repeats("cuda")


def test_device_path_equals_host_path():
    lw.check_device_path_equals_host_path("cuda")


def test_count_invariant_and_slot_reuse():
    lw.check_count_invariant_and_slot_reuse("cuda")


def test_min_p_rides_windows():
    lw.check_min_p_rides_windows("cuda")
