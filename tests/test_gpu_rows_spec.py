"""Spectral frames of rows on the GPU (-m gpu): Spectrogram.run (lw_spec_rows / k_spec), both routes against the fmaf-chain model.

The cases are in tests/rows_spec_gpu_cases.py and run ONCE, with pytest, in a process of their own that imports torch first
(tests/test_gpu_rows.py says why).  Each test below stands for one group of cases of that run (a function of the cases file with
all its parameters): every case of the group must have passed, and at least one must exist.  No case may skip."""
import pytest

import gpu_child

pytestmark = pytest.mark.gpu

CASES = "rows_spec_gpu_cases.py"
GROUPS = ["test_route_0_is_route_1_is_the_model", "test_a_dst_row_permutation_with_a_gap",
          "test_two_objects_queued_back_to_back_on_one_stream", "test_out_none_allocates_zeros",
          "test_log_is_torchs_own_at_the_written_positions_and_leaves_the_rest", "test_refusals_on_the_gpu_write_nothing"]


@pytest.fixture(scope="module")
def child(tmp_path_factory):
    return gpu_child.run_cases(tmp_path_factory, CASES, "rows_spec_gpu")


def test_every_group_of_the_cases_file_is_listed(child):
    assert sorted(child) == sorted(GROUPS)


@pytest.mark.parametrize("group", GROUPS)
def test_rows_spec(child, group):
    gpu_child.check_group(child, group)
