"""Normalising rows on the GPU (-m gpu): Normalize.run (lw_norm_rows / k_norm_sum, k_norm_fold, k_norm_apply) against the numpy
model of its contract, the device's scalars on a million scopes, and normalize= of decode_ogg_files.

The cases are in tests/rows_norm_gpu_cases.py and run ONCE, with pytest, in a process of their own that imports torch first
(tests/test_gpu_rows.py says why).  Each test below stands for one group of cases of that run (a function of the cases file with
all its parameters): every case of the group must have passed, and at least one must exist.  No case may skip."""
import pytest

import gpu_child

pytestmark = pytest.mark.gpu

CASES = "rows_norm_gpu_cases.py"
GROUPS = ["test_k_norm_is_the_model_on_the_base_shape", "test_list_level_boundaries_of_one_line",
          "test_a_row_scope_whose_list_crosses_lines_mid_group", "test_special_values",
          "test_the_devices_scalars_are_the_models_on_a_million_scopes", "test_rows_do_not_leak_and_both_fold_plans_agree_with_the_model",
          "test_one_launch_for_copy_and_fill_and_the_host_scalars", "test_calls_queued_back_to_back_on_one_stream",
          "test_decode_ogg_files_normalize_is_the_model_over_the_plain_call", "test_rows_to_cmvn_features_is_the_models_composed"]


@pytest.fixture(scope="module")
def child(tmp_path_factory):
    return gpu_child.run_cases(tmp_path_factory, CASES, "rows_norm_gpu", extra_args=("-s",))


def test_every_group_of_the_cases_file_is_listed(child):
    assert sorted(child) == sorted(GROUPS)


@pytest.mark.parametrize("group", GROUPS)
def test_rows_norm(child, group):
    gpu_child.check_group(child, group)
