"""Finishing feature rows and reflect-padded frames on the GPU (-m gpu): LogCompress.run (lw_feat_rows / k_feat) against the numpy
model of its contract, Spectrogram(pad_mode="reflect") on both routes against the fmaf-chain model, and the two chained.

The cases are in tests/rows_feat_gpu_cases.py and run ONCE, with pytest, in a process of their own that imports torch first
(tests/test_gpu_rows.py says why).  Each test below stands for one group of cases of that run (a function of the cases file with
all its parameters): every case of the group must have passed, and at least one must exist.  No case may skip."""
import pytest

import gpu_child

pytestmark = pytest.mark.gpu

CASES = "rows_feat_gpu_cases.py"
GROUPS = ["test_k_feat_is_the_model_on_the_base_shape", "test_one_long_scope_over_several_tiles",
          "test_the_devices_log_is_the_models_on_a_million_bit_patterns", "test_rows_and_channels_do_not_leak",
          "test_no_maximum_no_second_launch_and_the_host_log", "test_calls_queued_back_to_back_on_one_stream",
          "test_reflect_route_0_is_route_1_is_the_model", "test_reflect_is_the_uncentred_transform_of_torchs_padded_rows",
          "test_rows_to_whisper_features_is_the_two_models_composed"]


@pytest.fixture(scope="module")
def child(tmp_path_factory):
    return gpu_child.run_cases(tmp_path_factory, CASES, "rows_feat_gpu")


def test_every_group_of_the_cases_file_is_listed(child):
    assert sorted(child) == sorted(GROUPS)


@pytest.mark.parametrize("group", GROUPS)
def test_rows_feat(child, group):
    gpu_child.check_group(child, group)
