"""Stream-major rows on the GPU (-m gpu): lw_rows_synth / k_rows (lewton_amd.rows.Rows), decode_streams, decode_ogg_files.

The cases are in tests/rows_gpu_cases.py and run ONCE, with pytest, in a process of their own: torch brings its own copy of the
HIP runtime, and a process that hands torch tensors and streams to the library has to load torch before the library
(lewton_amd/rows.py says why) -- in this process the test modules collected earlier have loaded the library already.  Each test
below stands for one group of cases of that run (a function of the cases file with all its parameters): every case of the group
must have passed, and at least one must exist.  A case that skipped there (only the test beyond 2^32 elements may, on a device
with less than 16 GB free) skips here."""
import os
import subprocess
import sys
import xml.etree.ElementTree as ET

import pytest

from common import ROOT

pytestmark = pytest.mark.gpu

CASES = os.path.join(ROOT, "tests", "rows_gpu_cases.py")
GROUPS = ["test_rows_equal_packet_major_and_oracle", "test_rows_single_launch_patterns", "test_rows_device_entropy",
          "test_rows_damaged_packets", "test_alignment_cases", "test_back_to_back_on_a_side_stream",
          "test_same_call_twice_is_idempotent", "test_refusals_on_the_gpu_write_nothing", "test_size_256_streams_of_64_packets",
          "test_destination_beyond_2_to_the_32_elements", "test_decode_streams", "test_decode_ogg_files_golden_three_times",
          "test_decode_ogg_files_two_setups", "test_decode_ogg_files_refuses_chained_and_mixed"]


@pytest.fixture(scope="module")
def child(tmp_path_factory):
    xml = str(tmp_path_factory.mktemp("rows_gpu") / "cases.xml")
    r = subprocess.run([sys.executable, "-m", "pytest", CASES, "-m", "gpu", "-q", "-rs", "-p", "no:cacheprovider", "--junitxml", xml],
                       cwd=ROOT, capture_output=True, text=True, timeout=1500)
    print(r.stdout[-6000:])
    assert os.path.exists(xml), (r.returncode, r.stdout[-3000:], r.stderr[-3000:])
    groups = {}
    for tc in ET.parse(xml).getroot().iter("testcase"):
        name = tc.get("name")
        bad = [(e.tag, (e.get("message") or "")[:300], (e.text or "")[-3000:]) for e in tc if e.tag in ("failure", "error", "skipped")]
        groups.setdefault(name.split("[")[0], []).append((name, bad))
    return groups


def test_every_group_of_the_cases_file_is_listed(child):
    assert sorted(child) == sorted(GROUPS)


@pytest.mark.parametrize("group", GROUPS)
def test_rows(child, group):
    cases = child.get(group, [])
    assert cases, "no case of %s ran" % group
    failed = [(name, bad) for name, bad in cases if any(tag != "skipped" for tag, _, _ in bad)]
    assert not failed, "\n".join("%s: %s\n%s" % (name, bad[0][1], bad[0][2]) for name, bad in failed)
    skipped = [(name, bad) for name, bad in cases if bad]
    if skipped:
        assert group == "test_destination_beyond_2_to_the_32_elements", skipped
        pytest.skip(skipped[0][1][0][1])
