"""Normalising rows on the GPU (-m gpu): Normalize.run (lw_norm_rows / k_norm_sum, k_norm_fold, k_norm_apply) against the numpy
model of its contract, the device's scalars on a million scopes, and normalize= of decode_ogg_files.

The cases are in tests/rows_norm_gpu_cases.py and run ONCE, with pytest, in a process of their own that imports torch first
(tests/test_gpu_rows.py says why).  Each test below stands for one group of cases of that run (a function of the cases file with
all its parameters): every case of the group must have passed, and at least one must exist.  No case may skip."""
import os
import subprocess
import sys
import xml.etree.ElementTree as ET

import pytest

from common import ROOT

pytestmark = pytest.mark.gpu

CASES = os.path.join(ROOT, "tests", "rows_norm_gpu_cases.py")
GROUPS = ["test_k_norm_is_the_model_on_the_base_shape", "test_list_level_boundaries_of_one_line",
          "test_a_row_scope_whose_list_crosses_lines_mid_group", "test_special_values",
          "test_the_devices_scalars_are_the_models_on_a_million_scopes", "test_rows_do_not_leak_and_both_fold_plans_agree_with_the_model",
          "test_one_launch_for_copy_and_fill_and_the_host_scalars", "test_calls_queued_back_to_back_on_one_stream",
          "test_decode_ogg_files_normalize_is_the_model_over_the_plain_call", "test_rows_to_cmvn_features_is_the_models_composed"]


@pytest.fixture(scope="module")
def child(tmp_path_factory):
    xml = str(tmp_path_factory.mktemp("rows_norm_gpu") / "cases.xml")
    r = subprocess.run([sys.executable, "-m", "pytest", CASES, "-m", "gpu", "-q", "-rs", "-s", "-p", "no:cacheprovider", "--junitxml", xml],
                       cwd=ROOT, capture_output=True, text=True, timeout=900)
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
def test_rows_norm(child, group):
    cases = child.get(group, [])
    assert cases, "no case of %s ran" % group
    failed = [(name, bad) for name, bad in cases if bad]               # a skip counts as a failure here
    assert not failed, "\n".join("%s: %s\n%s" % (name, bad[0][1], bad[0][2]) for name, bad in failed)
