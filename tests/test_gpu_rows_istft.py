"""Inverse spectral frames of rows and the complex output of the spectral frames on the GPU (-m gpu): InverseSpectrogram.run
(lw_istft_rows / k_istft) and Spectrogram(output="complex") (k_spec_complex), both routes against the bit models.

The cases are in tests/rows_istft_gpu_cases.py and run ONCE, with pytest, in a process of their own that imports torch first
(tests/test_gpu_rows.py says why).  Each test below stands for one group of cases of that run (a function of the cases file with
all its parameters): every case of the group must have passed, and at least one must exist.  No case may skip."""
import pytest

import gpu_child

pytestmark = pytest.mark.gpu

CASES = "rows_istft_gpu_cases.py"
GROUPS = ["test_route_0_is_route_1_is_the_model", "test_two_tile_sizes_give_the_same_bits",
          "test_special_values_reach_exactly_the_samples_the_model_says", "test_a_dst_row_permutation_with_a_gap",
          "test_two_objects_queued_back_to_back_on_a_side_stream", "test_refusals_on_the_gpu_write_nothing",
          "test_complex_spec_route_0_is_route_1_is_the_model", "test_round_trip_through_the_public_classes"]


@pytest.fixture(scope="module")
def child(tmp_path_factory):
    return gpu_child.run_cases(tmp_path_factory, CASES, "rows_istft_gpu")


def test_every_group_of_the_cases_file_is_listed(child):
    assert sorted(child) == sorted(GROUPS)


@pytest.mark.parametrize("group", GROUPS)
def test_rows_istft(child, group):
    gpu_child.check_group(child, group)
