"""The rows chain past element 2^32 of a tensor and past 65535 rows of a call on the GPU (-m gpu): k_rows_mix, k_resample, k_spec,
k_spec_complex, k_istft, k_feat, k_norm, k_cep, k_slide and k_select at offsets no other test reaches, and the second launch
(row0 != 0) of lw_resample_rows, lw_spec_rows (power, mel and complex), lw_istft_rows, lw_feat_rows, lw_norm_rows, lw_cep_rows,
lw_slide_rows and lw_select_rows.

The cases are in tests/rows_large_gpu_cases.py and run ONCE, with pytest, in a process of their own that imports torch first
(tests/test_gpu_rows.py says why); that process allocates its 38.7 GB of device memory once (43.2 GB at the peak, with the
byte mask of a k_select case beside it).  The child run takes 5.9 s for its 106 cases on an MI355X, 3.4 s of it behind the allocation
(5.9 s for 70 cases before k_spec_complex, k_istft, k_slide and k_select had theirs: a new case takes 0.01 to 0.4 s).  Each test below stands for one group
of cases of that run (a function of the cases file with all its parameters): every case of the group must have passed, and at
least one must exist.  No case may skip: too little free device memory is a failure here."""
import pytest

import gpu_child

pytestmark = pytest.mark.gpu

CASES = "rows_large_gpu_cases.py"
GROUPS = ["test_k_cep_past_2_to_the_32", "test_k_norm_past_2_to_the_32", "test_k_feat_past_2_to_the_32", "test_k_spec_past_2_to_the_32",
          "test_k_resample_past_2_to_the_32", "test_k_rows_mix_past_2_to_the_32", "test_resample_65540_rows", "test_spec_65540_rows",
          "test_feat_65540_rows", "test_norm_65540_rows", "test_norm_65540_rows_workgroup_fold", "test_cep_65540_rows",
          "test_k_slide_past_2_to_the_32", "test_k_select_past_2_to_the_32", "test_k_istft_past_2_to_the_32",
          "test_k_spec_complex_past_2_to_the_32", "test_slide_65540_rows", "test_select_65540_rows", "test_istft_65540_rows",
          "test_spec_complex_65540_rows"]


@pytest.fixture(scope="module")
def child(tmp_path_factory):
    return gpu_child.run_cases(tmp_path_factory, CASES, "rows_large_gpu", extra_args=("-s", "--durations=8"))


def test_every_group_of_the_cases_file_is_listed(child):
    assert sorted(child) == sorted(GROUPS)


@pytest.mark.parametrize("group", GROUPS)
def test_rows_large(child, group):
    gpu_child.check_group(child, group)
