"""Frame selection (lw_select_*, lw_select_rows, k_select_count, k_select) in the CPU suite: tests/san/select_host.cpp links
lw_select.cpp against the HIP stand-ins (tests/san/hip_standins.inc) under ASan / UBSan and compiles the kernel source itself,
lw_kernels_select.hip, for the host, where its stand-in launchers run it workgroup by workgroup and phase by phase over exact-size
buffers.

The model is the rule of include/lewton_amd.h ("frame decisions and frame selection") in numpy (tests/select_model.py).  What the
kernels make of real device memory, LDS and the barriers is checked on the GPU (tests/test_gpu_rows_slide.py)."""
import os

import numpy as np
import pytest

import select_model as M
import host_harness as H
from common import ROOT
from host_harness import CAPACITY, CS, DEVICE, NULL_ARG, OK, UNSUPPORTED

SRC = [os.path.join(ROOT, "tests", "san", "select_host.cpp"), os.path.join(CS, "lw_select.cpp")]
F32 = np.float32
SENT_COUNT = 0xEEEEEEEEEEEEEEEE
N, CAP = [1100, 0, 257, 600], 1103                                      # two seams of the default tile's quarter, one of the default


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return H.build(tmp_path_factory, "select_host", SRC)


_run = H.run


# ---- refusals, and what is queued

def test_create_and_the_tile_hook(harness):
    for device, code in ((0, OK), (1, DEVICE), (-1, DEVICE), (1 << 20, DEVICE)):              # the stand-ins have one device
        assert _run(harness, "create", device) == ["RC %d" % code], device
    for tile, code in ((256, OK), (512, OK), (2048, OK), (1024, OK), (0, UNSUPPORTED), (128, UNSUPPORTED), (300, UNSUPPORTED), (2304, UNSUPPORTED)):
        assert _run(harness, "tile", tile) == ["RC %d TILE %d" % (code, tile if code == OK else 1024)]


ROW_REFUSALS = [("null_se", NULL_ARG), ("null_n", NULL_ARG), ("null_src", NULL_ARG), ("null_mask", NULL_ARG), ("null_dst", NULL_ARG),
                ("null_dst_fill_only", NULL_ARG), ("n_over", CAPACITY), ("fill_over", CAPACITY), ("ch0", CAPACITY), ("ch256", CAPACITY), ("f0", CAPACITY),
                ("f65536", CAPACITY), ("too_large", CAPACITY), ("too_many_tiles", CAPACITY)]
UNTOUCHED = "COUNTS" + " 77" * 6


@pytest.mark.parametrize("case,code", ROW_REFUSALS)
def test_refusals_queue_nothing(harness, case, code):
    assert _run(harness, "refuse", case) == ["RC %d" % code, "LAUNCHES 0", "LAST -1", UNTOUCHED]


def test_accepted_calls_and_their_launches(harness):
    """two launches per call (the counts of the tiles, then the selection); one where no row has a frame (nothing to count, the
    fill alone); none without rows or with nothing to write -- the counts are then zeroed by a memset, all of them 0"""
    for case, n in (("ok", 2), ("ok_no_rows", 0), ("ok_nothing", 0), ("ok_fill_only", 1), ("ok_most_tiles", 1)):
        out = _run(harness, "refuse", case)
        assert out[:3] == ["RC 0", "LAUNCHES %d" % n, "LAST %d" % n], case
        if case == "ok_nothing":
            assert out[3] == "COUNTS" + " 0" * 6


def test_two_calls_back_to_back_each_reach_their_own_records(harness):
    """the second call's records do not replace the first's, which its kernels read later; the caller's arrays are free at once"""
    assert _run(harness, "two") == ["RC 0 LAST 2", "RC 0 LAST 2", "ROWS 3000/3000 0/3 4/4", "ROWS 1/1 257/257 13/13", "LAUNCHES 4"]


# ---- the kernel source on the host

def _kernel(harness, tmp_path, x, mask, n, fill_to, tile, counts=True, offs=(0, 0)):
    R, C, F, cap = x.shape
    src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(src, "wb") as f:
        f.write(np.asarray(n, np.uint64).tobytes())
        f.write(np.asarray(fill_to if fill_to is not None else [0] * R, np.uint64).tobytes())
        f.write(np.ascontiguousarray(mask, np.uint8).tobytes())
        f.write(np.ascontiguousarray(x, F32).tobytes())
    out = _run(harness, "run", tile, C, F, R, cap, int(fill_to is not None), int(counts), offs[0], offs[1], src, dst)
    assert out[0] == "RC 0" and out[2] == "TILE %d" % tile, out
    raw = np.fromfile(dst, np.uint8)
    return raw[:x.nbytes].view(F32).reshape(x.shape), raw[x.nbytes:].view(np.uint64).reshape(R, C), int(out[1].split()[1])


def _check(harness, tmp_path, x, mask, n, fill_to, tile, counts=True, offs=(0, 0)):
    got, gk, launches = _kernel(harness, tmp_path, x, mask, n, fill_to, tile, counts, offs)
    want, k = M.rows(x, mask, n, fill_to, np.full(x.shape, M.SENT_F, F32))
    M.same_bits(got, want)
    assert np.array_equal(gk, k.astype(np.uint64) if counts else np.full(k.shape, SENT_COUNT, np.uint64))
    span = max(max(n), max(fill_to) if fill_to is not None else 0)
    assert launches == (0 if span == 0 else 2 if max(n) else 1)
    return want, k


FILLS = [lambda n, cap: None, lambda n, cap: [cap] * len(n), lambda n, cap: [max(0, v - 2) for v in n],
         lambda n, cap: [min(cap, (v * 7 + 3) % (cap + 1)) for v in n]]


@pytest.mark.parametrize("F", [1, 3, 81])
def test_kernel_on_the_host_is_the_model_at_every_shape_of_the_gpu_suite(harness, tmp_path, F):
    """[4][2][F][1103] with lengths 1100, 0, 257 and 600, every kind of mask, tiles of 256 (five in the longest row) and 1024 (two);
    the kind of fill_to, whether the counts are wanted and the residue of the buffers against 16 bytes in rotation"""
    x = M.source(N, 2, F, CAP, 50 + F)
    for i, kind in enumerate(M.KINDS):
        mask = M.mask(kind, N, 2, CAP, 9 + i)
        for tile in (256, 1024):
            _, k = _check(harness, tmp_path, x, mask, N, FILLS[(i + tile // 1024) % 4](N, CAP), tile, counts=bool((i + tile // 256) % 3),
                          offs=(4 * (i % 4), 4 * ((i + 1) % 4)))
        if kind in ("zero", "one", "last"):
            assert k[:, 0].tolist() == [{"zero": 0, "one": T, "last": min(T, 1)}[kind] for T in N]


def test_rows_do_not_leak_and_empty_calls(harness, tmp_path):
    """every row alone gives the bits it gives among the others; a call whose rows are all empty writes zero counts and nothing
    else; rows that only fill need no mask"""
    x = M.source(N, 2, 3, CAP, 41)
    mask = M.mask("random", N, 2, CAP, 3)
    together, k = _check(harness, tmp_path, x, mask, N, [CAP, 5, 0, 700], 256)
    assert (together[1, :, :, :5].view(np.uint32) == 0).all() and (together[1, :, :, 5:].view(np.uint32) == M.SENT).all()
    for r in range(4):
        alone, ka = _check(harness, tmp_path, x[r:r + 1], mask[r:r + 1], N[r:r + 1], None, 1024)
        M.same_bits(alone[0, :, :, :N[r]], together[r, :, :, :N[r]])
        assert np.array_equal(ka[0], k[r])
    _check(harness, tmp_path, x, mask, [0] * 4, None, 1024)
    _check(harness, tmp_path, x, mask, [0] * 4, [3, 0, CAP, 1], 1024)


def test_a_tile_far_up_a_row_past_frame_2_to_the_32(harness, tmp_path):
    """one row of 2^32 + 4096 + 5000 frames in tiles of 2048 of which only the last 5000 exist; the tiles in front of them are not run
    and count as kept whole, so the kept frames land from position 2^32 + 4096 on: the offsets of the mask, of the gather and of
    the destination, the sum of two million tile counts and K are all 64-bit"""
    base, keep, F = (1 << 32) + 4096, 5000, 2
    x = M.source([keep], 1, F, keep, 77)[0, 0]
    mask = M.mask("random", [keep], 1, keep, 5)[0, 0]
    src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(src, "wb") as f:
        f.write(mask.tobytes())
        f.write(x.tobytes())
    out = _run(harness, "far", 2048, F, base, keep, src, dst)
    assert out == ["RC 0", "LAUNCHES %d" % (2 * F)], out
    raw = np.fromfile(dst, np.uint8)
    got, K = raw[:x.nbytes].view(F32).reshape(F, keep), int(raw[x.nbytes:].view(np.uint64)[0])
    want, k = M.rows(x[None, None], mask[None, None], [keep], None, np.full((1, 1, F, keep), M.SENT_F, F32))
    assert K == int(k[0, 0]) and 2000 < K < 3000
    M.same_bits(got, want[0, 0])


# ---- Python

def test_python_parameter_errors_need_no_gpu():
    from lewton_amd.rows import SelectFrames
    for kw in [dict(device=-1), dict(device=1.5), dict(device="0"), dict(device=True)]:
        with pytest.raises(ValueError):
            SelectFrames(**kw)
