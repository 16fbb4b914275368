"""SpecAugment masks past 65535 rows of a call, past element 2^32 of a tensor and past frame 2^32 of one row on the GPU (-m gpu): the
second launch (row0 != 0) of k_specaug, ids that are row indices of the call, and offsets and frame numbers no other test reaches.

The cases are in tests/rows_specaug_large_gpu_cases.py and run ONCE, with pytest, in a process of their own that imports torch first
(tests/test_gpu_rows.py says why); that process allocates 25.8 GB of device memory once.  Each test below stands for one group of
cases of that run (a function of the cases file with all its parameters): every case of the group must have passed, and at least
one must exist.  No case may skip: too little free device memory is a failure here."""
import pytest

import gpu_child

pytestmark = pytest.mark.gpu

CASES = "rows_specaug_large_gpu_cases.py"
GROUPS = ["test_specaug_65540_rows", "test_line_past_element_2_to_the_32_in_place", "test_one_row_past_frame_2_to_the_32_in_place"]


@pytest.fixture(scope="module")
def child(tmp_path_factory):
    return gpu_child.run_cases(tmp_path_factory, CASES, "rows_specaug_large_gpu", extra_args=("-s", "--durations=8"))


def test_every_group_of_the_cases_file_is_listed(child):
    assert sorted(child) == sorted(GROUPS)


@pytest.mark.parametrize("group", GROUPS)
def test_rows_specaug_large(child, group):
    gpu_child.check_group(child, group)
