"""The rows chain past element 2^32 INSIDE a row on the GPU (-m gpu): k_resample, k_spec, k_spec_complex, k_istft, k_feat, k_norm,
k_slide, k_select and k_pack on one row of 2^32 + 2^20 + 5 elements, positions no other test reaches, and row lengths above 2^32 as counts in the kernels.

The cases are in tests/rows_long_row_gpu_cases.py and run ONCE, with pytest, in a process of their own that imports torch first
(tests/test_gpu_rows.py says why); that process allocates its 51.8 GB of device memory once (56.1 GB at the peak, with k_select's
byte mask beside it).  Each test below stands for one group
of cases of that run (a function of the cases file with all its parameters): every case of the group must have passed, and at
least one must exist.  No case may skip: too little free device memory is a failure here, as in tests/test_gpu_rows_large.py.

Durations of the child run on an MI355X (--durations=0): 21 cases in 11.2 s, 8.8 s of it behind the allocation;
tests/rows_large_gpu_cases.py took 5.9 s for its 70 cases on the same visit.  Per case, seconds: k_spec 32_hop1_mel1_zero 2.34
(route 0 alone: 1.85 in the kernel for 2^32 frames; route 1 took 5.6 and is left out there), kaldi_512_400_160_dc_energy 2.19,
400_160_mel1_reflect 1.45, 400_160_mel1_zero 1.44 (both routes each; most of it is the model's fmaf emulation on the host);
k_feat two_launches 0.25, the other four 0.02 to 0.03; k_pack 0.20 and 0.14; k_norm 0.08 to 0.12; k_resample 0.02 to 0.09.  A
kernel's pass over the 17 GB row is 10 to 80 ms.

With the cases of k_slide, k_select, k_spec_complex and k_istft (same box, a later visit): 32 cases in 23.8 s, 21.2 s of it behind
the allocation; tests/rows_large_gpu_cases.py took 5.9 s for its 106 cases.  Per new case, seconds: k_select keep_most and
drop_middle 3.08 each (3.07 in k_select: every workgroup adds up all 2^21 + 513 tile counts of the row; the cases take
the largest tile, 2048, for that reason), k_istft istft_256_128_tile_frames_1 2.09 (route 0 alone: 1.82 in the kernel, 2^25 + 2^13 + 2
tiles that compute 32 frames each for one frame's samples), istft_256_128_interleaved 1.02 and istft_256_128_planar 0.77 (both routes: 0.11 and 0.38 in the
kernel), k_spec_complex complex_256_128_reflect 1.60 (route 0 0.10, route 1 0.57) and complex_256_128_zero 0.70 (route 0 alone: the index arithmetic of the routes
is the same code, and reflect runs both), k_slide 0.05 to 0.13, its refusal 0.01.  The older cases took what they took before."""
import pytest

import gpu_child

pytestmark = pytest.mark.gpu

CASES = "rows_long_row_gpu_cases.py"
GROUPS = ["test_k_resample_inside_a_row_past_2_to_the_32", "test_k_spec_inside_a_row_past_2_to_the_32", "test_k_feat_inside_a_row_past_2_to_the_32",
          "test_k_norm_inside_a_row_past_2_to_the_32", "test_k_pack_inside_a_row_past_2_to_the_32", "test_k_slide_inside_a_row_past_2_to_the_32",
          "test_k_slide_refuses_more_tiles_than_a_grid_counts", "test_k_select_inside_a_row_past_2_to_the_32",
          "test_k_spec_complex_inside_a_row_past_2_to_the_32", "test_k_istft_inside_a_row_past_2_to_the_32"]


@pytest.fixture(scope="module")
def child(tmp_path_factory):
    return gpu_child.run_cases(tmp_path_factory, CASES, "rows_long_row_gpu", extra_args=("-s", "--durations=0"))


def test_every_group_of_the_cases_file_is_listed(child):
    assert sorted(child) == sorted(GROUPS)


@pytest.mark.parametrize("group", GROUPS)
def test_rows_long_row(child, group):
    gpu_child.check_group(child, group)
