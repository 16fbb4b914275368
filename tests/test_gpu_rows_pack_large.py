"""k_pack past element 2^32 of its source and of its destination on the GPU (-m gpu): offsets no other test of FramePack reaches,
through the row (one case per dtype), the channel and the line index.

The cases are in tests/rows_pack_large_gpu_cases.py and run ONCE, with pytest, in a process of their own that imports torch first
(tests/test_gpu_rows.py says why); that process holds up to 51.6 GB of device memory.  Each test below stands for one group of
cases of that run: every case of the group must have passed, and at least one must exist.  No case may skip: too little free
device memory is a failure here, as in tests/test_gpu_rows_large.py."""
import pytest

import gpu_child

pytestmark = pytest.mark.gpu

CASES = "rows_pack_large_gpu_cases.py"
GROUPS = ["test_k_pack_past_2_to_the_32", "test_k_pack_channel_and_line_past_2_to_the_32"]


@pytest.fixture(scope="module")
def child(tmp_path_factory):
    return gpu_child.run_cases(tmp_path_factory, CASES, "rows_pack_large_gpu", extra_args=("-s", "--durations=8"))


def test_every_group_of_the_cases_file_is_listed(child):
    assert sorted(child) == sorted(GROUPS)


@pytest.mark.parametrize("group", GROUPS)
def test_rows_pack_large(child, group):
    gpu_child.check_group(child, group)
