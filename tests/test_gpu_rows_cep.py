"""Cepstra and deltas of feature rows on the GPU (-m gpu): Cepstrum.run (lw_cep_rows / k_cep) against the numpy model of its
contract, the chain from samples to MFCCs with deltas against the three models composed, and against torch in float64.

The cases are in tests/rows_cep_gpu_cases.py and run ONCE, with pytest, in a process of their own that imports torch first
(tests/test_gpu_rows.py says why).  Each test below stands for one group of cases of that run (a function of the cases file with
all its parameters): every case of the group must have passed, and at least one must exist.  No case may skip."""
import pytest

import gpu_child

pytestmark = pytest.mark.gpu

CASES = "rows_cep_gpu_cases.py"
GROUPS = ["test_k_cep_is_the_model_on_the_base_shape", "test_the_widest_window", "test_output_groups", "test_tile_seams",
          "test_special_values", "test_rows_and_channels_do_not_leak", "test_calls_queued_back_to_back_on_one_stream",
          "test_rows_to_mfcc_with_deltas_is_the_three_models_composed", "test_against_torchs_matmul_and_conv1d_in_float64"]


@pytest.fixture(scope="module")
def child(tmp_path_factory):
    return gpu_child.run_cases(tmp_path_factory, CASES, "rows_cep_gpu")


def test_every_group_of_the_cases_file_is_listed(child):
    assert sorted(child) == sorted(GROUPS)


@pytest.mark.parametrize("group", GROUPS)
def test_rows_cep(child, group):
    gpu_child.check_group(child, group)
