"""Frame-major model input on the GPU (-m gpu): FramePack.run (lw_pack_rows / k_pack) against the numpy model of its contract, the
conversions over all 2^32 float32 bit patterns, and the chain from samples to a FunASR-style LFR input against the models composed
and against torch.

The cases are in tests/rows_pack_gpu_cases.py and run ONCE, with pytest, in a process of their own that imports torch first
(tests/test_gpu_rows.py says why).  Each test below stands for one group of cases of that run (a function of the cases file with
all its parameters): every case of the group must have passed, and at least one must exist.  No case may skip."""
import pytest

import gpu_child

pytestmark = pytest.mark.gpu

CASES = "rows_pack_gpu_cases.py"
GROUPS = ["test_k_pack_is_the_model_on_the_base_shape", "test_tile_seams", "test_line_groups", "test_special_values", "test_every_f32_bit_pattern",
          "test_rows_and_channels_do_not_leak", "test_mask_and_counts", "test_calls_queued_back_to_back_on_one_stream",
          "test_samples_to_lfr_input_is_the_models_composed", "test_65540_rows"]


@pytest.fixture(scope="module")
def child(tmp_path_factory):
    return gpu_child.run_cases(tmp_path_factory, CASES, "rows_pack_gpu", extra_args=("--durations=8",))


def test_every_group_of_the_cases_file_is_listed(child):
    assert sorted(child) == sorted(GROUPS)


@pytest.mark.parametrize("group", GROUPS)
def test_rows_pack(child, group):
    gpu_child.check_group(child, group)
