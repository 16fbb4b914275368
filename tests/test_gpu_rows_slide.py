"""Sliding-window normalisation of feature rows and frame selection on the GPU (-m gpu): SlidingCMVN.run (lw_slide_rows / k_slide)
against the numpy model of its contract and against torch's cumulative sums in float64, SelectFrames.run (lw_select_rows /
k_select) against numpy's boolean indexing, and the chain from samples to frame-major model input against the models composed.

The cases are in tests/rows_slide_gpu_cases.py and run ONCE, with pytest, in a process of their own that imports torch first
(tests/test_gpu_rows.py says why).  Each test below stands for one group of cases of that run (a function of the cases file with
all its parameters): every case of the group must have passed, and at least one must exist.  No case may skip."""
import pytest

import gpu_child

pytestmark = pytest.mark.gpu

CASES = "rows_slide_gpu_cases.py"
GROUPS = ["test_k_slide_is_the_model", "test_tile_seams", "test_special_values", "test_rows_and_channels_do_not_leak",
          "test_calls_queued_back_to_back_on_one_stream_and_on_a_side_stream", "test_refusals_are_value_errors",
          "test_against_torchs_cumulative_sums_in_float64", "test_k_select_is_the_model", "test_select_rows_do_not_leak_and_refusals",
          "test_fbank_to_sliding_cmvn_to_selected_frames_to_model_input_is_the_models_composed"]


@pytest.fixture(scope="module")
def child(tmp_path_factory):
    return gpu_child.run_cases(tmp_path_factory, CASES, "rows_slide_gpu")


def test_every_group_of_the_cases_file_is_listed(child):
    assert sorted(child) == sorted(GROUPS)


@pytest.mark.parametrize("group", GROUPS)
def test_rows_slide(child, group):
    gpu_child.check_group(child, group)
