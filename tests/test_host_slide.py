"""Sliding-window normalisation (lw_slide_*, lw_slide_rows, k_slide) in the CPU suite: tests/san/slide_host.cpp links lw_slide.cpp
against the HIP stand-ins (tests/san/hip_standins.inc) under ASan / UBSan and compiles the kernel source itself,
lw_kernels_slide.hip, for the host, where its stand-in launcher runs it workgroup by workgroup and phase by phase over exact-size
buffers and an exact-size LDS image.

The model is the rule of include/lewton_amd.h ("sliding-window normalisation of feature rows") in numpy (tests/slide_model.py).
What the kernel makes of real device memory, LDS and the barriers is checked on the GPU (tests/test_gpu_rows_slide.py)."""
import os

import numpy as np
import pytest

import slide_model as M
import host_harness as H
from common import ROOT
from host_harness import CAPACITY, CS, DEVICE, NULL_ARG, OK, UNSUPPORTED

SRC = [os.path.join(ROOT, "tests", "san", "slide_host.cpp"), os.path.join(CS, "lw_slide.cpp")]
F32 = np.float32
TILES = [1024, 48]                                                     # the default, and one that divides no length used here


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return H.build(tmp_path_factory, "slide_host", SRC)


_run = H.run


# ---- refusals, and what is queued

# (W, min, center, norm_vars)
CREATE = [((0, 0, 0, 0), UNSUPPORTED), ((4, 0, 0, 0), UNSUPPORTED), ((4, 5, 0, 0), UNSUPPORTED), ((2049, 1, 0, 0), UNSUPPORTED),
          ((4, 2, 2, 0), UNSUPPORTED), ((4, 2, -1, 0), UNSUPPORTED), ((4, 2, 0, 2), UNSUPPORTED), ((4, 2, 0, -1), UNSUPPORTED),
          ((1, 1, 0, 0), OK), ((2048, 2048, 1, 1), OK), ((2048, 1, 0, 1), OK), ((600, 100, 0, 0), OK), ((300, 100, 1, 1), OK)]


def test_create_refusals(harness):
    for args, code in CREATE:
        assert _run(harness, "create", *args) == ["RC %d" % code], args
    for device, code in ((0, OK), (1, DEVICE), (-1, DEVICE), (1 << 20, DEVICE)):              # the stand-ins have one device
        assert _run(harness, "create", 300, 100, 1, 0, device) == ["RC %d" % code], device
    assert _run(harness, "create", 4, 5, 0, 0, 1) == ["RC %d" % UNSUPPORTED]                   # parameters are judged first


ROW_REFUSALS = [("null_sl", NULL_ARG), ("null_n", NULL_ARG), ("null_src", NULL_ARG), ("null_dst", NULL_ARG), ("null_dst_fill_only", NULL_ARG),
                ("n_over", CAPACITY), ("fill_over", CAPACITY), ("ch0", CAPACITY), ("ch256", CAPACITY), ("f0", CAPACITY), ("f65536", CAPACITY),
                ("too_large", CAPACITY), ("too_many_tiles", CAPACITY), ("too_many_groups", CAPACITY)]


@pytest.mark.parametrize("case,code", ROW_REFUSALS)
def test_refusals_queue_nothing(harness, case, code):
    assert _run(harness, "refuse", case) == ["RC %d" % code, "LAUNCHES 0", "LAST -1"]


def test_accepted_calls_and_their_launches(harness):
    """one launch per call; none without rows or with nothing to write; one for a fill alone; 2^24 - 1 tiles is the most a launch is
    given"""
    for case, n in (("ok", 1), ("ok_no_rows", 0), ("ok_nothing", 0), ("ok_fill_only", 1), ("ok_most_tiles", 1)):
        assert _run(harness, "refuse", case) == ["RC 0", "LAUNCHES %d" % n, "LAST %d" % n], case


def test_two_calls_back_to_back_each_reach_their_own_records(harness):
    """the second call's records do not replace the first's, which its kernel reads later; the caller's arrays are free at once"""
    assert _run(harness, "two") == ["RC 0 LAST 1", "RC 0 LAST 1", "ROWS 700/700 0/3 4/4", "ROWS 1/1 257/257 13/13", "LAUNCHES 2"]


def test_tile_hook(harness):
    for tile, code in ((16, OK), (48, OK), (4096, OK), (1024, OK), (0, UNSUPPORTED), (8, UNSUPPORTED), (24, UNSUPPORTED), (4112, UNSUPPORTED)):
        assert _run(harness, "tile", 600, tile) == ["RC %d TILE %d" % (code, tile if code == OK else 1024)]


def test_tile_plan_fits_its_budget(harness):
    """the image holds the longest span a tile's windows can cover (tile + W, and up to 15 frames of alignment), two lines at
    least, in at most 64 KiB; the doubles in front of the floats keep the floats on a 16-byte boundary"""
    for F in (1, 5, 80):
        for W in (1, 4, 300, 600, 2048):
            for tile in (16, 48, 1024, 4096):
                out = _run(harness, "plan", F, W, tile)[0].split()
                t, cols, pitch, nb, lines, lds = (int(v) for v in out[1::2])
                assert t == tile and cols >= tile + W + 15 and cols % 16 == 0 and nb == cols // 16 and pitch >= cols + (cols - 1) // 32 + 1
                most = min(16, 65536 // (4 * pitch + 16 * nb))
                most = most & ~3 if most >= 4 else most                                        # four lines side by side in the apply phase
                assert lines == min(F, most) and lines >= min(F, 2) and lds == lines * (4 * pitch + 16 * nb) <= 65536
    assert _run(harness, "plan", 5, 600, 20) == ["REFUSED"]


@pytest.mark.parametrize("W,mn,center", [(4, 2, 1), (4, 3, 0), (600, 100, 0), (600, 100, 1), (300, 100, 1), (2048, 1, 0), (33, 33, 0), (16, 1, 1)])
def test_lw_slide_window_is_the_model(harness, W, mn, center):
    for T in (1, 2, 10, 99, 100, 101, 700):
        out = _run(harness, "window", W, mn, center, T)
        assert out[-1] == "RC %d" % CAPACITY                                                   # t == T
        assert [tuple(int(v) for v in ln.split()) for ln in out[:-1]] == [M.window(t, T, W, mn, bool(center)) for t in range(T)]


# ---- the kernel source on the host

def _kernel(harness, tmp_path, x, n, fill_to, cfg, tile, offs=(0, 0)):
    R, C, F, cap = x.shape
    src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(src, "wb") as f:
        f.write(np.asarray(n, np.uint64).tobytes())
        f.write(np.asarray(fill_to if fill_to is not None else [0] * R, np.uint64).tobytes())
        f.write(np.ascontiguousarray(x, F32).tobytes())
    out = _run(harness, "run", *cfg, tile, C, F, R, cap, int(fill_to is not None), offs[0], offs[1], src, dst)
    assert out[0] == "RC 0" and out[2] == "TILE %d" % tile, out
    return np.fromfile(dst, F32).reshape(x.shape), int(out[1].split()[1])


def _check(harness, tmp_path, x, n, fill_to, cfg, tile, offs=(0, 0), want=None):
    got, launches = _kernel(harness, tmp_path, x, n, fill_to, cfg, tile, offs)
    if want is None:
        want = M.rows(x, n, fill_to, np.full(x.shape, M.SENT_F, F32), cfg[0], cfg[1], bool(cfg[2]), bool(cfg[3]))
    M.same_bits(got, want, M.SENT)
    assert launches == int(max(max(n), max(fill_to) if fill_to is not None else 0) > 0)
    return want


FILLS = [lambda n, cap: None, lambda n, cap: [cap] * len(n), lambda n, cap: [max(0, v - 2) for v in n],
         lambda n, cap: [min(cap, (v * 7 + 3) % (cap + 1)) for v in n]]


@pytest.mark.parametrize("part", ["small", "mid", "big"])
def test_kernel_on_the_host_is_the_model_at_every_shape_of_the_gpu_suite(harness, tmp_path, part):
    """[3][2][5][longest + 3] with one empty row, every (window, length) pair of the GPU suite, at the default tile and at one of 48
    frames; the kind of fill_to and the residue of the buffers against 16 bytes taken in rotation"""
    cfgs, calls = {"small": M.SMALL, "mid": M.MID, "big": M.BIG}[part]
    i = 0
    for cfg in cfgs:
        for n in calls:
            i += 1
            cap = max(n) + 3
            x = M.source(n, M.CH, M.LINES, cap, 1000 + i)
            fill = FILLS[i % 4](n, cap)
            want = None
            for tile in TILES:
                want = _check(harness, tmp_path, x, n, fill, cfg, tile, offs=(4 * (i % 4), 4 * ((i // 2) % 4)), want=want)


def test_line_groups_on_the_host(harness, tmp_path):
    """more lines than a workgroup stages at a time: 20 lines are two groups at W = 4, 80 lines ten at W = 300; 7 lines are a group of 4 + 2 + 1"""
    for F, cfg, n in ((20, (4, 2, 1, 1), [70, 33]), (80, (300, 100, 1, 0), [310, 0]), (7, (8, 3, 0, 1), [70, 33])):
        x = M.source(n, 1, F, max(n) + 1, 7 + F)
        _check(harness, tmp_path, x, n, [max(n) + 1] * 2, cfg, 1024)


def test_special_values_on_the_host(harness, tmp_path):
    """NaN, +-inf, +-0, subnormals and FLT_MAX in the data and a constant line (its variance at the floor): every bit that is not a
    NaN is the model's, the sign of a zero included"""
    n = [70] * 9
    x = M.source(n, 1, 4, 71, 31, special=True)
    for cfg in ((8, 3, 0, 1), (16, 1, 1, 1), (8, 3, 0, 0), (33, 33, 0, 1)):
        for tile in (1024, 16):
            want = _check(harness, tmp_path, x, n, None, cfg, tile)
    assert np.isnan(want[..., :70]).any() and not np.isnan(want[0, ..., :70]).any()
    assert (want[:, 0, 0, :70].view(np.uint32) == 0).all()              # the constant line: (x - mu) = +0.0 times the floor's gain


def test_rows_do_not_leak(harness, tmp_path):
    """rows of different lengths and an empty row between them give the bits each gives alone"""
    n = [300, 0, 650, 17]
    x = M.source(n, 2, 3, 650, 41)
    cfg = (300, 100, 1, 1)
    together = _check(harness, tmp_path, x, n, [650, 5, 0, 20], cfg, 1024)
    assert (together[1, :, :, :5].view(np.uint32) == 0).all() and (together[1, :, :, 5:].view(np.uint32) == M.SENT).all()
    for r in range(4):
        alone = _check(harness, tmp_path, x[r:r + 1], n[r:r + 1], None, cfg, 48)
        M.same_bits(alone[0, :, :, :n[r]], together[r, :, :, :n[r]])


@pytest.mark.parametrize("cfg", [(8, 3, 0, 1), (300, 100, 1, 0)])
def test_a_tile_far_up_a_row_past_frame_2_to_the_32(harness, tmp_path, cfg):
    """one row of 2^32 + 4096 + 14000 frames of which only the last 14000 exist, in tiles of 4096 (a million of them: a smaller tile
    would be more than a grid counts): the tiles that lie wholly behind the first 2 W + tile existing frames are run with the source
    and destination pointers moved 2^32 + 4096 frames in front of the data, and give the model's bits of a row that is those
    frames alone (the windows of frames beyond W of its start, and the blocks -- the base is a multiple of 16 -- are the same);
    every offset of the kernel is therefore 64-bit"""
    W, mn, center, nv = cfg
    base, keep, tile, F = (1 << 32) + 4096, 14000, 4096, 2
    x = M.source([keep], 1, F, keep, 77)[0, 0]
    src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    x.tofile(src)
    out = _run(harness, "far", W, mn, center, nv, tile, F, base, keep, src, dst)
    assert out[:2] == ["RC 0", "LAUNCHES %d" % F], out
    lo = int(out[2].split()[1])
    assert 2 * W + tile <= lo < 2 * W + 2 * tile
    got = np.fromfile(dst, F32).reshape(F, keep)
    want = M.lines(x, W, mn, bool(center), bool(nv))
    M.same_bits(got[:, lo:], want[:, lo:])
    assert (got[:, :lo].view(np.uint32) == M.SENT).all()


# ---- Python

def test_python_parameter_errors_need_no_gpu():
    from lewton_amd.rows import SlidingCMVN
    for kw in [dict(cmn_window=0), dict(cmn_window=2049), dict(cmn_window=600.0), dict(cmn_window=True), dict(min_cmn_window=0),
               dict(cmn_window=50), dict(min_cmn_window=601), dict(min_cmn_window=1.5), dict(center=2), dict(center="yes"), dict(norm_vars=-1),
               dict(norm_vars=None)]:
        with pytest.raises(ValueError):
            SlidingCMVN(**kw)
