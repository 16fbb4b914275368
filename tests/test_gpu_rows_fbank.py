"""The Kaldi-compatible front end on the GPU (-m gpu): Spectrogram(framing="kaldi", ...) and KaldiFbank (lw_spec_create_ex / k_spec
with its per-frame prologue), both routes against the bit model, and the whole chain against the three models composed and the
float64 yardstick.

The cases are in tests/rows_fbank_gpu_cases.py and run ONCE, with pytest, in a process of their own that imports torch first
(tests/test_gpu_rows.py says why).  Each test below stands for one group of cases of that run (a function of the cases file with
all its parameters): every case of the group must have passed, and at least one must exist.  No case may skip."""
import pytest

import gpu_child

pytestmark = pytest.mark.gpu

CASES = "rows_fbank_gpu_cases.py"
GROUPS = ["test_route_0_is_route_1_is_the_model", "test_stft_framing_takes_the_new_options_too", "test_a_constant_row_with_remove_dc",
          "test_special_values", "test_the_shortest_row_kaldi_edges_accepts_and_one_sample_below",
          "test_a_dst_row_permutation_with_a_gap_and_two_objects_back_to_back_on_a_side_stream",
          "test_kaldi_fbank_is_the_three_models_composed_and_within_the_bound_of_the_yardstick", "test_kaldi_fbank_refuses_what_it_does_not_offer"]


@pytest.fixture(scope="module")
def child(tmp_path_factory):
    return gpu_child.run_cases(tmp_path_factory, CASES, "rows_fbank_gpu")


def test_every_group_of_the_cases_file_is_listed(child):
    assert sorted(child) == sorted(GROUPS)


@pytest.mark.parametrize("group", GROUPS)
def test_rows_fbank(child, group):
    gpu_child.check_group(child, group)
