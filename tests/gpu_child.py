"""The GPU cases files (tests/*_gpu_cases.py) run once each, with pytest, in a process of their own that imports torch first
(tests/test_gpu_rows.py says why).  run_cases starts that process and reads its junit XML; check_group is what one test of a
tests/test_gpu_rows*.py file asserts about one group of cases (a function of the cases file with all its parameters)."""
import os
import subprocess
import sys
import xml.etree.ElementTree as ET

import pytest

from common import ROOT


def run_cases(tmp_path_factory, cases_file, tag, extra_args=(), timeout=900):
    """{group: [(case name, [(tag, message, text) of every failure, error and skip])]} of one run of tests/<cases_file>"""
    xml = str(tmp_path_factory.mktemp(tag) / "cases.xml")
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.join(ROOT, "tests", cases_file), "-m", "gpu", "-q", "-rs", "-p", "no:cacheprovider",
                        *extra_args, "--junitxml", xml], cwd=ROOT, capture_output=True, text=True, timeout=timeout)
    print(r.stdout[-8000:])
    assert os.path.exists(xml), (r.returncode, r.stdout[-3000:], r.stderr[-3000:])
    groups = {}
    for tc in ET.parse(xml).getroot().iter("testcase"):
        name = tc.get("name")
        bad = [(e.tag, (e.get("message") or "")[:300], (e.text or "")[-3000:]) for e in tc if e.tag in ("failure", "error", "skipped")]
        groups.setdefault(name.split("[")[0], []).append((name, bad))
    return groups


def check_group(groups, group, may_skip=None):
    """at least one case of the group ran and none failed; a skip counts as a failure, except in the group `may_skip`, whose skip
    skips the calling test with the child's message"""
    cases = groups.get(group, [])
    assert cases, "no case of %s ran" % group
    failed = [(name, bad) for name, bad in cases if any(tag != "skipped" or group != may_skip for tag, _, _ in bad)]
    assert not failed, "\n".join("%s: %s\n%s" % (name, bad[0][1], bad[0][2]) for name, bad in failed)
    skipped = [bad for _, bad in cases if bad]
    if skipped:
        pytest.skip(skipped[0][0][1])
