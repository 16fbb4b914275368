"""The shared test plumbing, tested once (CPU only): the guarded buffer of tests/san/kernel_host.hpp -- what makes "ASan sees every
load and store the kernel makes" true at the FRONT of a buffer in the kernel host programs -- through
tests/san/kernel_host_selftest.cpp, which makes one deliberate access of host memory per run; and the status codes of
tests/host_harness.py against the enum of include/lewton_amd.h, read as text (lewton_amd._native loads the library at import)."""
import os
import re
import subprocess

import pytest

import host_harness as H
from common import ROOT


@pytest.fixture(scope="module")
def selftest(tmp_path_factory):
    return H.build(tmp_path_factory, "kernel_host_selftest", [os.path.join(H.SAN, "kernel_host_selftest.cpp")])


@pytest.mark.parametrize("off", [0, 3, 4, 15])
def test_writing_every_byte_of_a_guarded_buffer_is_clean(selftest, off):
    assert H.run(selftest, "ok", off) == ["INTACT 1"]


def test_a_store_into_the_unpoisoned_remainder_of_the_front_is_found_by_guard_intact(selftest):
    """OFF = 3: a front of 35 bytes, of which 32 are poisoned; at[-1] is the last of the three that are not"""
    assert H.run(selftest, "slack", 3) == ["INTACT 0"]


@pytest.mark.parametrize("mode,off", [("front", 0), ("front", 3), ("past", 0), ("past", 3), ("slack", 0), ("slack", 8)])
def test_an_access_in_front_of_or_beyond_a_guarded_buffer_is_an_asan_report(selftest, mode, off):
    """the first byte of the front (poisoned by hand), the byte behind the buffer (the allocation's end), and at[-1] where the
    front is whole granules"""
    r = subprocess.run([selftest, mode, str(off)], capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and "AddressSanitizer" in r.stderr, (r.returncode, r.stdout[-500:], r.stderr[-2000:])
    assert ("use-after-poison" if mode != "past" else "heap-buffer-overflow") in r.stderr, r.stderr[-2000:]
    assert "INTACT" not in r.stdout


def test_status_codes_are_those_of_the_header():
    text = open(os.path.join(ROOT, "include", "lewton_amd.h")).read()
    enum = {name: int(value) for name, value in re.findall(r"^\s*(LW_OK|LW_ERR_[A-Z_]+)\s*=\s*(\d+)\s*,?", text, re.M)}
    mine = {"LW_OK": H.OK, "LW_ERR_NULL_ARG": H.NULL_ARG, "LW_ERR_DEVICE": H.DEVICE, "LW_ERR_CAPACITY": H.CAPACITY,
            "LW_ERR_STATE_MISMATCH": H.STATE_MISMATCH, "LW_ERR_UNSUPPORTED": H.UNSUPPORTED}
    assert {name: enum.get(name) for name in mine} == mine
    assert sorted(n for n in enum if n.startswith("LW_ERR_")) == sorted(n for n in mine if n != "LW_OK")   # every LW_ERR_* is held
