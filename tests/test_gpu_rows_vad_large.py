"""The energy VAD past 65535 rows of a call, past byte 2^32 of a mask and element 2^32 of a source, and past frame 2^32 of one row
on the GPU (-m gpu): the second launch (row0 != 0) of k_vad and of k_vad_sum, k_vad_fold and k_vad_decide, offsets no other test
reaches, and a chunk list of five fold levels.

The cases are in tests/rows_vad_large_gpu_cases.py and run ONCE, with pytest, in a process of their own that imports torch first
(tests/test_gpu_rows.py says why); that process allocates its 22.8 GB of device memory once (23.9 GB at the peak) and takes 4.2 s for its 7 cases on an
MI355X.  Each test below stands for one group of
cases of that run (a function of the cases file with all its parameters): every case of the group must have passed, and at least
one must exist.  No case may skip: too little free device memory is a failure here."""
import pytest

import gpu_child

pytestmark = pytest.mark.gpu

CASES = "rows_vad_large_gpu_cases.py"
GROUPS = ["test_vad_65540_rows", "test_k_vad_past_2_to_the_32", "test_one_row_past_frame_2_to_the_32"]


@pytest.fixture(scope="module")
def child(tmp_path_factory):
    return gpu_child.run_cases(tmp_path_factory, CASES, "rows_vad_large_gpu", extra_args=("-s", "--durations=8"))


def test_every_group_of_the_cases_file_is_listed(child):
    assert sorted(child) == sorted(GROUPS)


@pytest.mark.parametrize("group", GROUPS)
def test_rows_vad_large(child, group):
    gpu_child.check_group(child, group)
