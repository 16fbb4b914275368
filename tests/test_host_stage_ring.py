"""The staged records of the row-chain entry points (lewton_amd/csrc/lw_stage.hpp) in the CPU suite: tests/san/stage_host.cpp
links lw_resample.cpp, lw_spec.cpp, lw_feat.cpp, lw_norm.cpp and lw_cep.cpp under ASan / UBSan against HIP stand-ins of its own,
which keep a model of what is in flight: an upload into a slot that queued work may still read, or freeing such a slot, ends the
harness with a message.  It drives the public entry points only.  The failure paths it covers cannot be reached on a GPU without
provoking a fault, so this is where they are tested."""
import os

import pytest

import host_harness as H
from common import ROOT
from host_harness import CS

SRC = [os.path.join(ROOT, "tests", "san", "stage_host.cpp")] + [
    os.path.join(CS, n) for n in ("lw_resample.cpp", "lw_spec.cpp", "lw_feat.cpp", "lw_norm.cpp", "lw_cep.cpp")]
ENTRIES = ["resample", "spec", "feat", "norm", "cep"]


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return H.build(tmp_path_factory, "stage_host", SRC)


def _run(exe, entry, case):
    assert H.run(exe, entry, case, timeout=300) == ["OK"]


@pytest.mark.parametrize("entry", ENTRIES)
def test_four_calls_back_to_back_rotate_three_slots_and_wait_once(harness, entry):
    """slots 0, 1, 2, 0; the only hipEventSynchronize is the fourth call's, before its upload, on the first call's event"""
    _run(harness, entry, "rotate")


@pytest.mark.parametrize("entry", ENTRIES)
def test_a_failed_launch_leaves_the_slot_marked_and_the_object_usable(harness, entry):
    """the last launch of a call fails (lw_feat_rows, lw_norm_rows: the second pass's, behind launches that were queued): the call
    returns LW_ERR_DEVICE; the calls of 1, 65, 66, 67 and 68 rows behind it return LW_OK, and none of their uploads or of the
    frees of their regrown slots touches memory that queued work may still read"""
    _run(harness, entry, "fail")


@pytest.mark.parametrize("entry", ENTRIES)
def test_65536_rows_are_two_launches_per_pass(harness, entry):
    """rows 0 .. 65534, then row 65535"""
    _run(harness, entry, "many")


@pytest.mark.parametrize("entry", ENTRIES)
def test_an_event_that_cannot_be_recorded_synchronises_the_stream(harness, entry):
    """LW_ERR_DEVICE, one hipStreamSynchronize, nothing left in flight, and the next calls are accepted"""
    _run(harness, entry, "norecord")
