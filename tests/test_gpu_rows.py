"""Stream-major rows on the GPU (-m gpu): lw_rows_synth / k_rows (lewton_amd.rows.Rows), decode_streams, decode_ogg_files.

The cases are in tests/rows_gpu_cases.py and run ONCE, with pytest, in a process of their own: torch brings its own copy of the
HIP runtime, and a process that hands torch tensors and streams to the library has to load torch before the library
(lewton_amd/rows.py says why) -- in this process the test modules collected earlier have loaded the library already.  Each test
below stands for one group of cases of that run (a function of the cases file with all its parameters): every case of the group
must have passed, and at least one must exist.  A case that skipped there (only the test beyond 2^32 elements may, on a device
with less than 16 GB free) skips here."""
import pytest

import gpu_child

pytestmark = pytest.mark.gpu

CASES = "rows_gpu_cases.py"
GROUPS = ["test_rows_equal_packet_major_and_oracle", "test_rows_single_launch_patterns", "test_rows_device_entropy",
          "test_rows_damaged_packets", "test_alignment_cases", "test_back_to_back_on_a_side_stream",
          "test_same_call_twice_is_idempotent", "test_refusals_on_the_gpu_write_nothing", "test_handle_lifecycle",
          "test_size_256_streams_of_64_packets",
          "test_destination_beyond_2_to_the_32_elements", "test_decode_streams", "test_decode_ogg_files_golden_three_times",
          "test_decode_ogg_files_two_setups", "test_decode_ogg_files_refuses_chained_and_mixed"]


@pytest.fixture(scope="module")
def child(tmp_path_factory):
    return gpu_child.run_cases(tmp_path_factory, CASES, "rows_gpu", timeout=1500)


def test_every_group_of_the_cases_file_is_listed(child):
    assert sorted(child) == sorted(GROUPS)


@pytest.mark.parametrize("group", GROUPS)
def test_rows(child, group):
    gpu_child.check_group(child, group, may_skip="test_destination_beyond_2_to_the_32_elements")
