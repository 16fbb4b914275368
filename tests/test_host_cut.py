"""Cutting rows into segment rows (lw_cut_*, lw_cut_rows, k_cut) in the CPU suite: tests/san/cut_host.cpp links lw_cut.cpp against the
HIP stand-ins (tests/san/hip_standins.inc) under ASan / UBSan and compiles the kernel source itself, lw_kernels_cut.hip, for the
host, where its stand-in launcher runs it workgroup by workgroup over exact-size buffers, the source poisoned outside the jobs'
parts of their lines.

The model is the rule of include/lewton_amd.h ("cutting rows into segment rows") in numpy (tests/cut_model.py).  Every comparison is
over every element of a sentinel-filled exact-size destination, as bit patterns.  What the kernel makes of real device memory is
checked on the GPU (tests/test_gpu_rows_segment.py)."""
import os

import numpy as np
import pytest

import cut_model as M
import host_harness as H
from common import ROOT
from host_harness import CAPACITY, CS, NULL_ARG, UNSUPPORTED

SRC = [os.path.join(ROOT, "tests", "san", "cut_host.cpp"), os.path.join(CS, "lw_cut.cpp")]
U64 = np.uint64


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return H.build(tmp_path_factory, "cut_host", SRC)


_run = H.run

REFUSALS = [("null_c", NULL_ARG), ("null_n", NULL_ARG), ("null_jobs", NULL_ARG), ("null_src", NULL_ARG), ("null_dst", NULL_ARG),
            ("null_dst_fill_only", NULL_ARG), ("elem1", UNSUPPORTED), ("elem3", UNSUPPORTED), ("elem8", UNSUPPORTED), ("row_over", CAPACITY),
            ("start_after_end", CAPACITY), ("end_over", CAPACITY), ("len_over", CAPACITY), ("fill_over", CAPACITY), ("n_over", CAPACITY),
            ("ch0", CAPACITY), ("ch256", CAPACITY), ("f0", CAPACITY), ("f65536", CAPACITY), ("too_large", CAPACITY), ("too_large_out", CAPACITY),
            ("too_many_tiles", CAPACITY)]


@pytest.mark.parametrize("case,code", REFUSALS)
def test_refusals_queue_nothing_and_leave_the_destination_untouched(harness, case, code):
    assert _run(harness, "refuse", case) == ["RC %d" % code, "LAUNCHES 0", "LAST -1", "OUT 1"]


def test_accepted_calls_and_their_launches(harness):
    """one launch per 65535 jobs, none where nothing is to be written"""
    for case, n in (("ok", 1), ("ok_i16", 1), ("ok_most_tiles", 1), ("ok_no_jobs", 0), ("ok_no_rows_no_jobs", 0), ("ok_empty_jobs", 0),
                    ("ok_fill_only", 1), ("ok_jobs65536", 2)):
        assert _run(harness, "refuse", case) == ["RC 0", "LAUNCHES %d" % n, "LAST %d" % n, "OUT 1"], case


def test_two_calls_back_to_back_each_reach_their_own_records(harness):
    """the second call's records do not replace the first's, which its kernel reads later; the caller's arrays are free at once"""
    assert _run(harness, "two") == ["RC 0 LAST 1", "RC 0 LAST 1", "ROWS 10/40/64 600/40/40 90/10/11", "ROWS 605/1/1", "LAUNCHES 2"]


def _check(harness, tmp_path, x, n, jobs, fill_to, outcap, elem, offs=(0, 0)):
    R, C, F, cap = x.shape
    jobs = np.asarray(jobs, U64).reshape(-1, 3)
    src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(src, "wb") as f:
        f.write(np.asarray(n, U64).tobytes())
        f.write(jobs.tobytes())
        f.write(np.asarray(fill_to if fill_to is not None else [0] * len(jobs), U64).tobytes())
        f.write(np.ascontiguousarray(x).tobytes())
    out = _run(harness, "run", elem, C, F, R, cap, len(jobs), outcap, int(fill_to is not None), offs[0], offs[1], src, dst)
    span = max([int(b - a) for _, a, b in jobs.tolist()] + ([int(v) for v in fill_to] if fill_to is not None else []), default=0)
    assert out == ["RC 0", "LAUNCHES %d" % (1 if span else 0)], out
    got = np.fromfile(dst, M.UINT[elem]).reshape(len(jobs), C, F, outcap)
    want = M.rows(x, jobs, fill_to, np.full((len(jobs), C, F, outcap), M.SENT[elem], M.UINT[elem]))
    M.same(got, want)
    return want


@pytest.mark.parametrize("elem", [2, 4])
@pytest.mark.parametrize("F", [1, 3])
def test_every_source_residue_against_16_bytes_times_every_length(harness, tmp_path, elem, F):
    """[2][2][F][157] elements of 2 and 4 bytes: a job for every start in 16 bytes' worth of elements (an i16 source at an odd start
    among them) times every length in 0 .. 40, into rows of 43 elements whose odd pitch takes the destination lines over every
    residue too; without fill_to, filled to the row's end, and filled a few elements past each length; both buffers moved against
    16 bytes.  Jobs overlap in the source and name both rows many times"""
    n = [157, 90]
    x = M.source(n, 2, F, 157, elem, 5 + elem + F)
    jobs = [(k % 2, 37 + s, 37 + s + ln) for k, (s, ln) in enumerate((s, ln) for s in range(16 // elem) for ln in range(41))]
    for i, fill in enumerate((None, [43] * len(jobs), [min(43, (ln * 3) % 47) for _, a, b in jobs for ln in [b - a]])):
        _check(harness, tmp_path, x, n, jobs, fill, 43, elem, offs=(elem * (i + 1), elem * (2 * i + 1) % 16))
    _check(harness, tmp_path, x, n, jobs, None, 48, elem)                       # a pitch of whole groups: aligned lines


@pytest.mark.parametrize("elem", [2, 4])
def test_long_jobs_over_several_tiles_repeated_and_overlapping(harness, tmp_path, elem):
    """lines longer than a workgroup's 16384 bytes (three tiles for f32, two for i16, the last one short), starts of every residue, the
    same stretch twice, one job inside another, whole rows, empty jobs, and the ends of both rows"""
    n = [10007, 9001]
    x = M.source(n, 1, 2, 10007, elem, 9 + elem)
    jobs = [(0, 0, 10007), (1, 0, 9001), (0, 1, 10007), (0, 3, 9000), (0, 3, 9000), (1, 4097, 9001), (0, 5000, 5000), (1, 9001, 9001), (0, 5, 4101),
            (1, 7, 8200), (0, 10006, 10007)]
    want = _check(harness, tmp_path, x, n, jobs, [0, 10008, 3, 10001, 0, 0, 5, 0, 4100, 9000, 10009], 10009, elem, offs=(elem, 16 - elem))
    assert np.array_equal(want[3, :, :, :8997], want[4, :, :, :8997]) and np.array_equal(want[0, :, :, 1:10007], want[2, :, :, :10006])
    _check(harness, tmp_path, x, n, jobs, None, 10008, elem)


def test_empty_calls(harness, tmp_path):
    x = M.source([50], 1, 1, 50, 4, 3)
    _check(harness, tmp_path, x, [50], [], None, 8, 4)
    _check(harness, tmp_path, x, [50], [(0, 5, 5), (0, 50, 50)], None, 8, 4)
    _check(harness, tmp_path, x, [50], [(0, 5, 5), (0, 50, 50)], [3, 0], 8, 4)


@pytest.mark.parametrize("elem", [2, 4])
def test_a_job_past_element_2_to_the_32(harness, tmp_path, elem):
    """one line of 2^32 + 4099 + 9000 elements of which only the last 9000 exist, the source pointer moved in front of them: the
    job's offset into the line is beyond 32 bits"""
    base, keep = (1 << 32) + 4099, 9000
    x = M.source([keep], 1, 1, keep, elem, 21)[0, 0, 0]
    src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    x.tofile(src)
    assert _run(harness, "far", elem, base, keep, 13, 8990, 9000, src, dst) == ["RC 0", "LAUNCHES 1"]
    got = np.fromfile(dst, M.UINT[elem])
    assert np.array_equal(got[:8977], x[13:8990]) and (got[8977:].view(np.uint8) == 0x7E).all()
