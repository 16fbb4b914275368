"""SpecAugment masks over feature rows on the GPU (-m gpu): SpecAugment.run (lw_specaug_rows / k_specaug) against the integer and numpy
model of its contract, and the chain from samples through fbank, CMVN and the masks to frame-major model input against the five
models composed.

The cases are in tests/rows_specaug_gpu_cases.py and run ONCE, with pytest, in a process of their own that imports torch first
(tests/test_gpu_rows.py says why).  Each test below stands for one group of cases of that run (a function of the cases file with
all its parameters): every case of the group must have passed, and at least one must exist.  No case may skip."""
import pytest

import gpu_child

pytestmark = pytest.mark.gpu

CASES = "rows_specaug_gpu_cases.py"
GROUPS = ["test_k_specaug_is_the_model", "test_masks_at_the_ends_at_a_seam_empty_overlapping_and_whole_rows", "test_fill_bits_and_special_sources",
          "test_masks_depend_on_seed_and_id_alone", "test_per_channel", "test_spans_are_the_plan_are_the_model",
          "test_calls_queued_back_to_back_on_one_stream_and_on_a_side_stream", "test_refusals_are_value_errors",
          "test_fbank_to_cmvn_to_specaug_to_lfr_input_is_the_models_composed"]


@pytest.fixture(scope="module")
def child(tmp_path_factory):
    return gpu_child.run_cases(tmp_path_factory, CASES, "rows_specaug_gpu")


def test_every_group_of_the_cases_file_is_listed(child):
    assert sorted(child) == sorted(GROUPS)


@pytest.mark.parametrize("group", GROUPS)
def test_rows_specaug(child, group):
    gpu_child.check_group(child, group)
