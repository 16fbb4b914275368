"""Stream-major rows through a channel matrix on the GPU (-m gpu): lw_rows_synth_mix / k_rows_mix (Rows.synth(mix=)),
decode_streams and decode_ogg_files with channels=.

The cases are in tests/rows_mix_gpu_cases.py and run ONCE, with pytest, in a process of their own that imports torch first
(tests/test_gpu_rows.py says why).  Each test below stands for one group of cases of that run (a function of the cases file with
all its parameters): every case of the group must have passed, and at least one must exist.  No case may skip."""
import pytest

import gpu_child

pytestmark = pytest.mark.gpu

CASES = "rows_mix_gpu_cases.py"
GROUPS = ["test_matrices_and_formats", "test_subnormal_products_are_kept", "test_alignment_cases", "test_two_matrices_back_to_back",
          "test_same_call_twice_is_idempotent", "test_plain_synth_between_two_mix_calls", "test_refusals_on_the_gpu_write_nothing",
          "test_decode_streams_channels", "test_decode_ogg_files_stereo_and_mono_to_mono",
          "test_decode_ogg_files_channels_dict_and_callable", "test_decode_ogg_files_wav_order_of_a_51_file",
          "test_decode_ogg_files_channels_refusals"]


@pytest.fixture(scope="module")
def child(tmp_path_factory):
    return gpu_child.run_cases(tmp_path_factory, CASES, "rows_mix_gpu")


def test_every_group_of_the_cases_file_is_listed(child):
    assert sorted(child) == sorted(GROUPS)


@pytest.mark.parametrize("group", GROUPS)
def test_rows_mix(child, group):
    gpu_child.check_group(child, group)
