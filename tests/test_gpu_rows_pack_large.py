"""k_pack past element 2^32 of its source and of its destination on the GPU (-m gpu): offsets no other test of FramePack reaches,
through the row (one case per dtype), the channel and the line index.

The cases are in tests/rows_pack_large_gpu_cases.py and run ONCE, with pytest, in a process of their own that imports torch first
(tests/test_gpu_rows.py says why); that process holds up to 51.6 GB of device memory.  Each test below stands for one group of
cases of that run: every case of the group must have passed, and at least one must exist.  No case may skip: too little free
device memory is a failure here, as in tests/test_gpu_rows_large.py."""
import os
import subprocess
import sys
import xml.etree.ElementTree as ET

import pytest

from common import ROOT

pytestmark = pytest.mark.gpu

CASES = os.path.join(ROOT, "tests", "rows_pack_large_gpu_cases.py")
GROUPS = ["test_k_pack_past_2_to_the_32", "test_k_pack_channel_and_line_past_2_to_the_32"]


@pytest.fixture(scope="module")
def child(tmp_path_factory):
    xml = str(tmp_path_factory.mktemp("rows_pack_large_gpu") / "cases.xml")
    r = subprocess.run([sys.executable, "-m", "pytest", CASES, "-m", "gpu", "-q", "-rs", "-s", "-p", "no:cacheprovider", "--durations=8",
                        "--junitxml", xml], cwd=ROOT, capture_output=True, text=True, timeout=900)
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
def test_rows_pack_large(child, group):
    cases = child.get(group, [])
    assert cases, "no case of %s ran" % group
    failed = [(name, bad) for name, bad in cases if bad]               # a skip counts as a failure here
    assert not failed, "\n".join("%s: %s\n%s" % (name, bad[0][1], bad[0][2]) for name, bad in failed)
