"""Energy voice-activity decisions of feature rows on the GPU (-m gpu): EnergyVad.run (lw_vad_rows / k_vad, k_vad_sum, k_vad_fold,
k_vad_decide) against the numpy model of its contract and against Kaldi's own order of operations restated, and the chain from
samples through the VAD's mask to frame-major model input against the six models composed.

The cases are in tests/rows_vad_gpu_cases.py and run ONCE, with pytest, in a process of their own that imports torch first
(tests/test_gpu_rows.py says why).  Each test below stands for one group of cases of that run (a function of the cases file with
all its parameters): every case of the group must have passed, and at least one must exist.  No case may skip."""
import pytest

import gpu_child

pytestmark = pytest.mark.gpu

CASES = "rows_vad_gpu_cases.py"
GROUPS = ["test_k_vad_is_the_model", "test_lengths_where_the_tree_changes_shape", "test_fused_is_split_is_the_model_on_one_input",
          "test_special_values", "test_rows_and_channels_do_not_leak", "test_without_a_mean_and_calls_with_nothing_to_write",
          "test_calls_queued_back_to_back_on_one_stream_and_on_a_side_stream", "test_refusals_are_value_errors",
          "test_kaldi_restatement_on_exact_inputs",
          "test_fbank_to_energy_vad_to_sliding_cmvn_to_selected_frames_to_model_input_is_the_models_composed"]


@pytest.fixture(scope="module")
def child(tmp_path_factory):
    return gpu_child.run_cases(tmp_path_factory, CASES, "rows_vad_gpu")


def test_every_group_of_the_cases_file_is_listed(child):
    assert sorted(child) == sorted(GROUPS)


@pytest.mark.parametrize("group", GROUPS)
def test_rows_vad(child, group):
    gpu_child.check_group(child, group)
