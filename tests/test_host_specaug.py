"""SpecAugment (lw_specaug_*, lw_specaug_rows, k_specaug, lw_rng.hpp) in the CPU suite: tests/san/specaug_host.cpp links
lw_specaug.cpp against the HIP stand-ins (tests/san/hip_standins.inc) under ASan / UBSan and compiles the kernel source itself,
lw_kernels_specaug.hip, for the host, where its stand-in launcher runs it workgroup by workgroup and phase by phase over exact-size
guarded buffers (out of place the source is poisoned at and beyond every line's T).

The model is the rule of include/lewton_amd.h ("masking feature rows") in Python integers and numpy (tests/specaug_model.py).  What
the kernel makes of real device memory, LDS and the barrier is checked on the GPU (tests/test_gpu_rows_specaug.py)."""
import os

import numpy as np
import pytest

import specaug_model as M
import host_harness as H
from common import ROOT
from host_harness import CAPACITY, CS, DEVICE, NULL_ARG, OK, UNSUPPORTED

SRC = [os.path.join(ROOT, "tests", "san", "specaug_host.cpp"), os.path.join(CS, "lw_specaug.cpp")]
U32 = np.uint32
N, CAP = [1100, 0, 1, 3, 255, 256, 257, 1023, 1024, 1025], 1103                 # the GPU suite's lengths and capacity
LONG = (1 << 32) + (1 << 20) + 5
SENT_SPAN = -0x5A5A5A5A5A5A5A5A


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return H.build(tmp_path_factory, "specaug_host", SRC)


_run = H.run


def _p(P, reserved=0):
    """the twelve numbers of lw_specaug_params"""
    return [P.seed, P.num_t, P.min_t, P.max_t, P.ratio_num, P.ratio_den, P.num_f, P.min_f, P.max_f, int(P.per_channel), P.fill_bits, reserved]


# ---- the generator

def test_philox_and_the_bounded_draws_on_the_host(harness, tmp_path):
    assert _run(harness, "philox", 0, 0, 0, 0, 0, 0) == ["X 6627e8d5 e169c58d bc57ac4c 9b00dbd8"]
    assert _run(harness, "philox", *([0xFFFFFFFF] * 6)) == ["X 408f276d 41c83b0e a20bc7c6 6d5451fd"]
    assert _run(harness, "philox", 0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344, 0xA4093822, 0x299F31D0) == ["X d16cfe09 94fdcceb 5001e420 24126ea1"]
    rng = np.random.default_rng(5)
    q = rng.integers(0, 1 << 64, (300, 2), dtype=np.uint64)
    q[:8] = [[0, 0], [(1 << 64) - 1, (1 << 64) - 1], [(1 << 64) - 1, 1], [1 << 63, 3001], [(1 << 32) - 1, 51], [12345, 0], [(1 << 64) - 1, 1 << 63], [7, 65536]]
    src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(src, "wb") as f:
        f.write(np.uint64(len(q)).tobytes())
        f.write(q.tobytes())
    _run(harness, "below", src, dst)
    got = np.fromfile(dst, np.uint64).reshape(-1, 2)
    for (x, n), (g32, g64) in zip(q.tolist(), got.tolist()):
        assert g32 == M.below32(x & M.M32, n & M.M32) and g64 == M.below64(x, n), (x, n)


# ---- refusals, and what is queued

def test_create_and_the_hooks(harness):
    ok = M.Params(seed=1)
    for device, code in ((0, OK), (1, DEVICE), (-1, DEVICE), (1 << 20, DEVICE)):              # the stand-ins have one device
        assert _run(harness, "create", device, *_p(ok)) == ["RC %d" % code], device
    cases = [(dict(min_t=51, max_t=50), UNSUPPORTED), (dict(min_f=11, max_f=10), UNSUPPORTED), (dict(num_t=33), UNSUPPORTED), (dict(num_f=33), UNSUPPORTED),
             (dict(max_t=65536), UNSUPPORTED), (dict(max_f=65536), UNSUPPORTED), (dict(ratio=(2, 1)), UNSUPPORTED), (dict(ratio=(1, 65536)), UNSUPPORTED),
             (dict(ratio=(65536, 65536)), UNSUPPORTED), (dict(num_t=32, num_f=32, min_t=65535, max_t=65535, min_f=65535, max_f=65535, ratio=(65535, 65535)), OK),
             (dict(num_t=0, num_f=0, max_t=0, max_f=0), OK), (dict(ratio=(0, 1)), OK), (dict(seed=(1 << 64) - 1, fill_bits=0x7FC12345), OK)]
    for kw, code in cases:
        assert _run(harness, "create", 0, *_p(M.Params(**kw))) == ["RC %d" % code], kw
    for pos, v in ((9, 2), (9, 0xFFFFFFFF), (11, 1)):                                          # per_channel not 0 or 1; reserved != 0
        q = _p(ok)
        q[pos] = v
        assert _run(harness, "create", 0, *q) == ["RC %d" % UNSUPPORTED], (pos, v)
    q = _p(ok)
    q[4], q[5] = 1, 0                                                                         # a ratio without a denominator
    assert _run(harness, "create", 0, *q) == ["RC %d" % UNSUPPORTED]
    for tile, code in ((256, OK), (512, OK), (2048, OK), (1024, OK), (768, OK), (0, UNSUPPORTED), (128, UNSUPPORTED), (300, UNSUPPORTED), (2304, UNSUPPORTED)):
        assert _run(harness, "tile", tile) == ["RC %d TILE %d" % (code, tile if code == OK else 2048)]


ROW_REFUSALS = [("null_sa", NULL_ARG), ("null_n", NULL_ARG), ("null_src", NULL_ARG), ("null_dst", NULL_ARG), ("null_dst_fill_only", NULL_ARG),
                ("n_over", CAPACITY), ("fill_over", CAPACITY), ("ch0", CAPACITY), ("ch256", CAPACITY), ("f0", CAPACITY), ("f65536", CAPACITY),
                ("too_large", CAPACITY), ("too_many_tiles", CAPACITY), ("too_many_tiles_by_lines", CAPACITY)]
UNTOUCHED = ["DST untouched", "SPANS untouched"]


@pytest.mark.parametrize("case,code", ROW_REFUSALS)
def test_refusals_queue_nothing(harness, case, code):
    assert _run(harness, "refuse", case) == ["RC %d" % code, "LAUNCHES 0", "LAST -1"] + UNTOUCHED


def test_accepted_calls_and_their_launches(harness):
    """one launch per 65535 rows; none without rows or when nothing can be written: out of place no position below any fill_end, in
    place no masks configured (or no frame to mask) and no fill span -- unless spans are owed, which rows without frames have too"""
    for case, n in (("ok", 1), ("ok_in_place", 1), ("ok_no_rows", 0), ("ok_no_masks_in_place", 0), ("ok_no_masks_in_place_fill", 1),
                    ("ok_no_masks_out_of_place", 1), ("ok_nothing", 0), ("ok_nothing_but_spans", 1), ("ok_in_place_no_frames", 0), ("ok_fill_only", 1),
                    ("ok_most_tiles", 1), ("ok_rows65535", 1), ("ok_rows65536", 2)):
        assert _run(harness, "refuse", case) == ["RC 0", "LAUNCHES %d" % n, "LAST %d" % n] + UNTOUCHED, case


def test_two_calls_back_to_back_each_reach_their_own_records(harness):
    """the second call's records do not replace the first's, which its kernel reads later; the caller's arrays are free at once;
    without ids a row's id is its index"""
    assert _run(harness, "two") == ["RC 0 LAST 1", "RC 0 LAST 1", "ROWS 3000/3000/7 0/3/%d 4/4/0" % (1 << 40), "ROWS 1/1/0 257/257/1 13/13/2", "LAUNCHES 2"]


# ---- lw_specaug_plan

def _plans(harness, tmp_path, P, queries):
    src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(src, "wb") as f:
        f.write(np.uint64(len(queries)).tobytes())
        f.write(np.asarray(queries, np.uint64).tobytes())
    _run(harness, "plans", *_p(P), src, dst)
    return np.fromfile(dst, np.int64).reshape(len(queries), 1 + 2 * P.masks)


def test_plan_on_the_host_is_the_model(harness, tmp_path):
    for P in (M.Params(seed=2024, num_t=32, max_t=65535, num_f=3, max_f=27), M.Params(seed=(1 << 64) - 3, min_t=5, ratio=(1, 5), min_f=2, per_channel=True),
              M.Params(seed=5, num_t=0, num_f=0)):
        q = [(id_, g, T, F) for id_ in (0, 7, 6099, (1 << 40) + 1, (1 << 64) - 1) for g in (0, 3, 65535) for T, F in
             ((3000, 80), (0, 0), (3, 1), (100, 65535), (LONG, 80), ((1 << 32) - 1, 5), ((1 << 63) - 1, 2))]
        got = _plans(harness, tmp_path, P, q)
        for (id_, g, T, F), row in zip(q, got.tolist()):
            assert row[0] == OK and row[1:] == [v for s in M.plan(P, id_, g, T, F) for v in s], (id_, g, T, F)
    P = M.Params(seed=2024, num_t=32, max_t=65535, num_f=0)
    assert tuple(_plans(harness, tmp_path, P, [(6099, 0, LONG, 1)])[0, 1 + 2 * 18:3 + 2 * 18]) == (4294953827, 4294968123)
    got = _plans(harness, tmp_path, P, [(0, 65536, 10, 1), (0, 0, 10, 65536), (0, 0, 1 << 63, 1)])
    assert (got[:, 0] == CAPACITY).all() and (got[:, 1:] == SENT_SPAN).all()


# ---- the kernel source on the host

def _kernel(harness, tmp_path, P, x, n, fill_to, ids, tile, in_place, want_spans=True, offs=(0, 0)):
    R, C, F, cap = x.shape
    src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(src, "wb") as f:
        f.write(np.asarray(n, np.uint64).tobytes())
        f.write(np.asarray(fill_to if fill_to is not None else [0] * R, np.uint64).tobytes())
        f.write(np.asarray(ids if ids is not None else [0] * R, np.uint64).tobytes())
        f.write(np.ascontiguousarray(x, U32).tobytes())
    out = _run(harness, "run", tile, C, F, R, cap, int(fill_to is not None), int(ids is not None), int(in_place), int(want_spans), offs[0], offs[1], *_p(P),
               src, dst)
    assert out[0] == "RC 0" and out[2] == "TILE %d" % tile, out
    raw = np.fromfile(dst, np.uint8)
    ne = R * C * F * cap
    return raw[:4 * ne].view(U32).reshape(x.shape), raw[4 * ne:].view(np.int64).reshape(R, C if P.per_channel else 1, P.masks, 2), int(out[1].split()[1])


def _launches(P, n, fill_to, in_place, want_spans):
    R = len(n)
    span = max([max(n)] + (list(fill_to) if fill_to is not None else [])) if R else 0
    fills = fill_to is not None and any(f > v for f, v in zip(fill_to, n))
    writes = (fills or (P.masks and max(n) > 0)) if in_place else span > 0
    return int(bool(R and (writes or (want_spans and P.masks))))


def _check(harness, tmp_path, P, x, n, fill_to, ids, tile, in_place, want_spans=True, offs=(0, 0)):
    got, spans, launches = _kernel(harness, tmp_path, P, x, n, fill_to, ids, tile, in_place, want_spans, offs)
    want, wspans = M.rows(P, x, n, fill_to, ids, x if in_place else np.full(x.shape, M.SENT_DST, U32))
    M.same_bits(got, want)
    if want_spans:
        assert np.array_equal(spans, wspans)
    else:
        assert (spans == SENT_SPAN).all()
    assert launches == _launches(P, n, fill_to, in_place, want_spans)
    return want, wspans


FILLS = [lambda n, cap: None, lambda n, cap: [cap] * len(n), lambda n, cap: [max(0, v - 2) for v in n],
         lambda n, cap: [min(cap, (v * 7 + 3) % (cap + 1)) for v in n]]
IDS = [3 * i + 1 for i in range(len(N))]


@pytest.mark.parametrize("F,ch", [(1, 2), (3, 1), (80, 1), (3, 2)])
def test_kernel_on_the_host_is_the_model_at_every_shape_of_the_gpu_suite(harness, tmp_path, F, ch):
    """[10][ch][F][1103] with lengths 1100, 0, 1, 3, 255, 256, 257, 1023, 1024 and 1025, tiles of 256, 1024 and 2048, in place and out
    of place, the four kinds of fill_to, with and without ids and spans, per_channel on and off, and the buffers at every residue
    of the line against 16 bytes, in rotation; the WeNet preset's widths and one with wide masks that meet tile seams and row ends"""
    x = M.source(N, ch, F, CAP, 60 + F + ch, special=True)
    i = 0
    for P in (M.Params(seed=2024, min_t=1, max_t=50, min_f=1, max_f=min(10, F), per_channel=ch > 1, fill_bits=0x7FC12345),
              M.Params(seed=11, num_t=5, min_t=0, max_t=700, num_f=1, max_f=min(2, F), fill_bits=0x80000000)):
        for tile in (256, 1024, 2048):
            for in_place in (False, True):
                i += 1
                _check(harness, tmp_path, P, x, N, FILLS[i % 4](N, CAP), IDS if i % 3 else None, tile, in_place, want_spans=bool(i % 2),
                       offs=(4 * (i % 4), 4 * ((i // 2) % 4)))


def test_every_residue_of_source_and_destination_against_sixteen_bytes(harness, tmp_path):
    """the 16-byte loads and stores and the dwords at the ragged head and tail of every tile's share: all sixteen pairs of residues"""
    n = [1100, 257, 5, 0]
    x = M.source(n, 1, 2, CAP, 77)
    P = M.Params(seed=3, num_t=3, max_t=300, num_f=0, fill_bits=M.bits_of(-np.inf))
    for a in range(4):
        for b in range(4):
            _check(harness, tmp_path, P, x, n, FILLS[(a + b) % 4](n, CAP), None, 256 if a % 2 else 1024, False, offs=(4 * a, 4 * b))
        _check(harness, tmp_path, P, x, n, FILLS[a](n, CAP), None, 512, True, offs=(4 * a, 0))


def test_masks_at_the_ends_at_a_seam_empty_overlapping_and_whole_rows(harness, tmp_path):
    """ids picked WITH the model: a mask that starts at 0, one that ends at T, one that crosses the seam of two tiles of 256, an empty
    one, two that overlap, and one that covers the whole of a row of 3 frames"""
    P = M.Params(seed=2024, num_t=2, min_t=0, max_t=50, num_f=0)
    T = 600
    found = {}
    for id_ in range(20000):
        (a0, b0), (a1, b1) = M.plan(P, id_, 0, T, 1)
        for what, hit in (("starts at 0", a0 == 0 and b0 > 0), ("ends at T", b0 == T and a0 < T), ("crosses a seam", a0 < 256 < b0 or a0 < 512 < b0),
                          ("empty", a0 == b0), ("overlap", a0 < b1 and a1 < b0 and a0 != a1)):
            if hit:
                found.setdefault(what, id_)
        if len(found) == 5:
            break
    assert len(found) == 5, found
    ids = [found[w] for w in ("starts at 0", "ends at T", "crosses a seam", "empty", "overlap")]
    x = M.source([T] * 5, 1, 1, T + 3, 8)
    for in_place in (False, True):
        _check(harness, tmp_path, P, x, [T] * 5, None, ids, 256, in_place)
    Q = M.Params(seed=2024, num_t=1, min_t=5, max_t=50, num_f=0)
    assert M.plan(Q, 7, 0, 3, 1) == [(0, 3)]
    x = M.source([3, 3], 2, 1, 7, 9)
    want, _ = _check(harness, tmp_path, Q, x, [3, 3], [5, 0], [7, 7], 256, False)
    assert (want[:, :, 0, :3] == 0).all() and (want[0, :, 0, 3:5] == 0).all() and (want[0, :, 0, 5:] == M.SENT_DST).all()


def test_fill_bits_special_sources_and_calls_with_nothing_to_write(harness, tmp_path):
    n = [300, 0, 40]
    x = M.source(n, 2, 3, 301, 12, special=True)
    for bits in (0x00000000, 0x80000000, 0x7FC12345, M.bits_of(-np.inf)):
        P = M.Params(seed=4, num_t=2, max_t=80, num_f=1, min_f=1, max_f=2, fill_bits=bits)
        for in_place in (False, True):
            want, _ = _check(harness, tmp_path, P, x, n, [301, 2, 0], None, 256, in_place)
            assert (want[0, :, :, :300] == bits).any()
    P0 = M.Params(seed=4, num_t=0, num_f=0)
    _check(harness, tmp_path, P0, x, n, None, None, 1024, True)                          # nothing can be written: no launch
    _check(harness, tmp_path, P0, x, n, [301, 2, 0], None, 1024, True)                   # the fill spans alone
    _check(harness, tmp_path, P0, x, n, None, None, 1024, False)                         # a copy
    _check(harness, tmp_path, M.Params(seed=4), x, [0, 0, 0], None, None, 1024, False, want_spans=False)
    _check(harness, tmp_path, M.Params(seed=4), x, [0, 0, 0], None, None, 1024, False, want_spans=True)   # rows without frames have spans


# ---- Python

def test_python_parameter_errors_need_no_gpu():
    from lewton_amd.rows import SpecAugment
    for kw in [dict(device=-1), dict(device=1.5), dict(device=True), dict(num_time_masks=33), dict(num_freq_masks=-1), dict(num_time_masks=1.0),
               dict(time_mask_param=65536), dict(freq_mask_param=65536), dict(min_time=51), dict(min_freq=11), dict(min_time=-1), dict(p=1.5), dict(p=-0.1),
               dict(p=float("nan")), dict(p="1"), dict(per_channel=2), dict(per_channel=None), dict(fill="0"), dict(fill=None), dict(seed=-1), dict(seed=1 << 64),
               dict(seed=1.0)]:
        with pytest.raises(ValueError):
            SpecAugment(**kw)
    with pytest.raises(ValueError):
        SpecAugment.paper("LX")
