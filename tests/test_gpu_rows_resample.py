"""The row resampler on the GPU (-m gpu): Resampler.run (lw_resample_rows / k_resample), decode_streams and decode_ogg_files
with sample_rate=.

The cases are in tests/rows_resample_gpu_cases.py and run ONCE, with pytest, in a process of their own that imports torch first
(tests/test_gpu_rows.py says why).  Each test below stands for one group of cases of that run (a function of the cases file with
all its parameters): every case of the group must have passed, and at least one must exist.  No case may skip."""
import pytest

import gpu_child

pytestmark = pytest.mark.gpu

CASES = "rows_resample_gpu_cases.py"
GROUPS = ["test_run_is_the_fold_bit_for_bit", "test_a_table_too_large_for_lds_goes_the_global_taps_route",
          "test_a_span_too_large_for_lds_goes_the_all_global_route", "test_equal_rates_copy_bits",
          "test_out_none_allocates_zeros_and_identity_rows", "test_calls_queued_back_to_back_each_give_their_own_result",
          "test_refusals_on_the_gpu_write_nothing", "test_decode_streams_sample_rate", "test_decode_ogg_files_of_three_rates_to_16k_mono"]


@pytest.fixture(scope="module")
def child(tmp_path_factory):
    return gpu_child.run_cases(tmp_path_factory, CASES, "rows_resample_gpu")


def test_every_group_of_the_cases_file_is_listed(child):
    assert sorted(child) == sorted(GROUPS)


@pytest.mark.parametrize("group", GROUPS)
def test_rows_resample(child, group):
    gpu_child.check_group(child, group)
