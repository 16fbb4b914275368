"""Segments and segment rows past 65535 rows, past frame 2^32 of one mask line and past byte 2^32 of a source, on the GPU (-m gpu):
k_segment_count, k_segment and k_cut against the models.

The cases are in tests/rows_segment_large_gpu_cases.py, which says what they cover and what they cost, and run ONCE, with pytest,
in a process of their own that imports torch first (tests/test_gpu_rows.py says why).  Each test below stands for one group of
cases of that run (a function of the cases file with all its parameters): every case of the group must have passed, and at least one
must exist.  Part B needs 8.6 GB of device memory and skips, with the reason, on a device that has less free."""
import pytest

import gpu_child

pytestmark = pytest.mark.gpu

CASES = "rows_segment_large_gpu_cases.py"
GROUPS = ["test_segments_65540_rows", "test_cut_65540_jobs", "test_one_mask_line_past_frame_2_to_the_32", "test_cut_job_past_byte_2_to_the_32"]
PART_B = GROUPS[2:]


@pytest.fixture(scope="module")
def child(tmp_path_factory):
    return gpu_child.run_cases(tmp_path_factory, CASES, "rows_segment_large_gpu", extra_args=("-s",))


def test_every_group_of_the_cases_file_is_listed(child):
    assert sorted(child) == sorted(GROUPS)


@pytest.mark.parametrize("group", GROUPS)
def test_rows_segment_large(child, group):
    gpu_child.check_group(child, group, may_skip=group if group in PART_B else None)
