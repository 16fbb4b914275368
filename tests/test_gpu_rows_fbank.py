"""The Kaldi-compatible front end on the GPU (-m gpu): Spectrogram(framing="kaldi", ...) and KaldiFbank (lw_spec_create_ex / k_spec
with its per-frame prologue), both routes against the bit model, and the whole chain against the three models composed and the
float64 yardstick.

The cases are in tests/rows_fbank_gpu_cases.py and run ONCE, with pytest, in a process of their own that imports torch first
(tests/test_gpu_rows.py says why).  Each test below stands for one group of cases of that run (a function of the cases file with
all its parameters): every case of the group must have passed, and at least one must exist.  No case may skip."""
import os
import subprocess
import sys
import xml.etree.ElementTree as ET

import pytest

from common import ROOT

pytestmark = pytest.mark.gpu

CASES = os.path.join(ROOT, "tests", "rows_fbank_gpu_cases.py")
GROUPS = ["test_route_0_is_route_1_is_the_model", "test_stft_framing_takes_the_new_options_too", "test_a_constant_row_with_remove_dc",
          "test_special_values", "test_the_shortest_row_kaldi_edges_accepts_and_one_sample_below",
          "test_a_dst_row_permutation_with_a_gap_and_two_objects_back_to_back_on_a_side_stream",
          "test_kaldi_fbank_is_the_three_models_composed_and_within_the_bound_of_the_yardstick", "test_kaldi_fbank_refuses_what_it_does_not_offer"]


@pytest.fixture(scope="module")
def child(tmp_path_factory):
    xml = str(tmp_path_factory.mktemp("rows_fbank_gpu") / "cases.xml")
    r = subprocess.run([sys.executable, "-m", "pytest", CASES, "-m", "gpu", "-q", "-rs", "-p", "no:cacheprovider", "--junitxml", xml],
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
def test_rows_fbank(child, group):
    cases = child.get(group, [])
    assert cases, "no case of %s ran" % group
    failed = [(name, bad) for name, bad in cases if bad]               # a skip counts as a failure here
    assert not failed, "\n".join("%s: %s\n%s" % (name, bad[0][1], bad[0][2]) for name, bad in failed)
