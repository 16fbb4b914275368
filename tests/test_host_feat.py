"""Finishing feature rows (lw_feat_*, lw_feat_rows, k_feat) in the CPU suite: tests/san/feat_host.cpp links lw_feat.cpp against the
HIP stand-ins (tests/san/hip_standins.inc) under ASan / UBSan and compiles the kernel source itself, lw_kernels_feat.hip, for the
host, where its stand-in launchers run it workgroup by workgroup and lane by lane over exact-size buffers.

The model is the rule of include/lewton_amd.h ("finishing feature rows") in numpy (tests/feat_model.py).  What the kernels make
of real device memory, the shuffles included, is checked on the GPU (tests/test_gpu_rows_feat.py)."""
import itertools
import os

import numpy as np
import pytest

import feat_model as M
import host_harness as H
from common import ROOT
from host_harness import CAPACITY, CS, DEVICE, NULL_ARG, OK, UNSUPPORTED

SRC = [os.path.join(ROOT, "tests", "san", "feat_host.cpp"), os.path.join(CS, "lw_feat.cpp")]
F32 = np.float32


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return H.build(tmp_path_factory, "feat_host", SRC)


_run = H.run


# ---- LOG

@pytest.fixture(scope="module")
def log_inputs():
    rng = np.random.default_rng(7)
    one = np.array(1.0, F32).view(np.uint32)
    bits = np.concatenate([
        rng.integers(1, 0x7F800000, 1 << 20, dtype=np.uint32),                       # positive finite f32, subnormals included
        np.arange(int(one) - (1 << 20), int(one) + (1 << 20) + 1, dtype=np.uint32),  # the 2^20 values either side of 1.0
        np.array([1, 0x00800000, 0x7F7FFFFF, 0x7F800000], np.uint32),                # smallest subnormal, FLT_MIN, FLT_MAX, +inf
        (np.arange(1, 255, dtype=np.uint32) << 23),                                  # the powers of two
        (np.arange(1, 255, dtype=np.uint32) << 23) - 1, (np.arange(1, 255, dtype=np.uint32) << 23) + 1])
    v = bits.astype(np.uint32).view(F32)
    assert len(v) >= 3_000_000 and (v > 0).all()
    return v


@pytest.mark.parametrize("kind", [M.NONE, M.LN, M.LOG10, M.DB])
def test_lw_feat_log_is_the_model_bit_for_bit(harness, tmp_path, log_inputs, kind):
    src, dst = str(tmp_path / "v.bin"), str(tmp_path / "l.bin")
    log_inputs.tofile(src)
    _run(harness, "log", kind, src, dst)
    got, want = np.fromfile(dst, F32), M.log(kind, log_inputs)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert not np.isnan(want).any() and want[log_inputs == np.inf][0] == np.inf


def test_lw_feat_log_outside_step_ones_range_is_nan(harness, tmp_path):
    src, dst = str(tmp_path / "v.bin"), str(tmp_path / "l.bin")
    np.array([0.0, -0.0, -1.0, np.nan, -np.inf], F32).tofile(src)
    _run(harness, "log", M.LOG10, src, dst)
    assert np.isnan(np.fromfile(dst, F32)).all()
    _run(harness, "log", M.NONE, src, dst)
    assert np.fromfile(dst, F32).tolist()[:3] == [0.0, 0.0, -1.0]


@pytest.mark.parametrize("kind,fn,scale", [(M.LN, np.log, 1.0), (M.LOG10, np.log10, 1.0), (M.DB, np.log10, 10.0)])
def test_the_model_is_within_one_ulp_of_the_rounded_float64_logarithm(log_inputs, kind, fn, scale):
    """the series leaves about 2e-17 relative, numpy's float64 log less than 1e-16, the constants half a float64 ulp each and
    (DB) the product by 10 another: all far below half a float32 ulp (6e-8 relative), so the two roundings to float32 can
    differ only where the value lies at a rounding boundary -- by one ulp.  The margin is that bound, not a measurement."""
    v = log_inputs[np.isfinite(log_inputs)]
    want = (fn(v.astype(np.float64)) * scale).astype(F32)
    got = M.log(kind, v)
    off = np.abs(got.view(np.int32).astype(np.int64) - want.view(np.int32).astype(np.int64))
    zero = (got == 0) & (want == 0)
    print("differ on %d of %d" % (int((off > 0).sum()), len(v)))
    assert (off[~zero] <= 1).all()


# ---- refusals, and what is queued

CREATE = [(("null", 0, 1e-10, 8, 4, 0.25), NULL_ARG), ((4, 0, 1e-10, 8, 4, 0.25), UNSUPPORTED), ((-1, 0, 1e-10, 8, 4, 0.25), UNSUPPORTED),
          ((2, 2, 1e-10, 8, 4, 0.25), UNSUPPORTED), ((2, 0, 0, 8, 4, 0.25), UNSUPPORTED), ((1, 0, -1, 8, 4, 0.25), UNSUPPORTED),
          ((3, 0, "inf", 8, 4, 0.25), UNSUPPORTED), ((2, 0, "nan", 8, 4, 0.25), UNSUPPORTED), ((0, 0, "nan", 8, 4, 0.25), UNSUPPORTED),
          ((2, 0, 1e-10, "nan", 4, 0.25), UNSUPPORTED), ((2, 0, 1e-10, -0.5, 4, 0.25), UNSUPPORTED),
          ((2, 0, 1e-10, 8, "nan", 0.25), UNSUPPORTED), ((2, 0, 1e-10, 8, 4, "nan"), UNSUPPORTED),
          ((2, 0, 1e-10, 8, 4, 0.25), OK), ((2, 1, 1e-45, "inf", "inf", 0), OK), ((0, 0, -5, 0, 0, -1), OK), ((0, 1, "-inf", 8, 4, 0.25), OK)]


def test_create_refusals(harness):
    for args, code in CREATE:
        assert _run(harness, "create", *args) == ["RC %d" % code], args
    ok = (2, 0, 1e-10, 8, 4, 0.25)
    for device, code in ((0, OK), (1, DEVICE), (-1, DEVICE), (1 << 20, DEVICE)):              # the stand-ins have one device
        assert _run(harness, "create", *ok, device) == ["RC %d" % code], device
    assert _run(harness, "create", 4, 0, 1e-10, 8, 4, 0.25, 1) == ["RC %d" % UNSUPPORTED]      # parameters are judged first


ROW_REFUSALS = [("null_ft", NULL_ARG), ("null_frames", NULL_ARG), ("null_src", NULL_ARG), ("null_dst", NULL_ARG),
                ("null_dst_fill_only", NULL_ARG), ("frames_over", CAPACITY), ("fill_over", CAPACITY), ("ch0", CAPACITY),
                ("ch256", CAPACITY), ("f0", CAPACITY), ("f65536", CAPACITY), ("too_large", CAPACITY), ("too_many_runs", CAPACITY)]


@pytest.mark.parametrize("case,code", ROW_REFUSALS)
def test_refusals_queue_nothing(harness, case, code):
    assert _run(harness, "refuse", case) == ["RC %d" % code, "LAUNCHES 0", "LAST -1"]


def test_accepted_calls_and_their_launches(harness):
    for case, n in (("ok", 2), ("ok_max", 2), ("ok_nothing", 0), ("ok_no_rows", 0), ("ok_max_of_nothing", 2)):
        assert _run(harness, "refuse", case) == ["RC 0", "LAUNCHES %d" % n, "LAST %d" % n], case


def test_two_calls_back_to_back_each_reach_their_own_records(harness):
    """the second call's records do not replace the first's, which its kernels read later; the caller's arrays are free at once"""
    out = _run(harness, "two")
    assert out == ["RC 0 LAST 2", "RC 0 LAST 2", "ROWS 9/9 0/3 4/4", "ROWS 9/9 0/3 4/4", "ROWS 1/1 2/2 3/3", "ROWS 1/1 2/2 3/3", "LAUNCHES 4"]


# ---- the kernel source on the host

def _kernel(harness, tmp_path, x, n_frames, fill_to, kind, scope, floor, top, add, mul, inplace, want_max, shifts=(0, 0)):
    R, C, F, cap = x.shape
    src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(src, "wb") as f:
        f.write(np.asarray(n_frames, np.uint64).tobytes())
        f.write(np.asarray(fill_to if fill_to is not None else [0] * R, np.uint64).tobytes())
        f.write(np.ascontiguousarray(x, F32).tobytes())
    out = _run(harness, "run", kind, scope, floor, top, add, mul, C, F, R, cap, int(inplace), int(want_max), int(fill_to is not None),
               shifts[0], shifts[1], src, dst)
    assert out[0] == "RC 0"
    raw = np.fromfile(dst, F32)
    return raw[:x.size].reshape(x.shape), raw[x.size:], int(out[1].split()[1])


def _check(harness, tmp_path, x, n_frames, fill_to, kind, scope, floor, top, add=4.0, mul=0.25, inplace=False, want_max=True, shifts=(0, 0)):
    got, mx, launches = _kernel(harness, tmp_path, x, n_frames, fill_to, kind, scope, floor, top, add, mul, inplace, want_max, shifts)
    before = x if inplace else np.full(x.shape, M.SENT_F, F32)
    want, Ms = M.rows(x, n_frames, fill_to, before, kind, scope, floor, top, add, mul)
    M.same_bits(got, want, M.SENT)
    if want_max:
        M.same_bits(mx, Ms.ravel(), M.SENT)
    else:
        assert (mx.view(np.uint32) == M.SENT).all()
    assert launches == (1 if np.isposinf(F32(top)) and not want_max else 2)


FILLS = {"none": lambda n, cap: None, "frames": lambda n, cap: list(n), "capacity": lambda n, cap: [cap] * len(n),
         "below": lambda n, cap: [max(0, v - 2) for v in n], "mixed": lambda n, cap: [min(cap, (v * 7 + 3) % (cap + 1)) for v in n]}


@pytest.mark.parametrize("kind,floor", [(M.NONE, -1.0), (M.LN, 1e-10), (M.LOG10, 1e-10), (M.DB, 1e-42)])
def test_kernel_on_the_host_is_the_model_on_the_base_shape(harness, tmp_path, kind, floor):
    """F = 3, capacity 37, n_frames 0 .. 37 over the rows of one call, one and two channels, both scopes, top 8 / 0 / inf, in place
    and not, every kind of fill_to, d_max asked for or not, source and destination lines at every residue against 16 bytes:
    every element of a sentinel-filled exact-size destination, NaN in the source beyond n_frames"""
    n = M.BASE_FRAMES
    combos = list(itertools.product((1, 2), (M.ROW, M.CHANNEL), (8.0, 0.0, "inf"), (False, True), sorted(FILLS)))
    for i, (ch, scope, top, inplace, fill) in enumerate(combos):
        x = M.source(n, ch, 3, 37, floor, 100 + i, inf_row=4 if i % 3 == 0 else None)
        shifts = ((i // 5) % 4, (i // 5 + i) % 4)
        _check(harness, tmp_path, x, n, FILLS[fill](n, 37), kind, scope, floor, top, inplace=inplace, want_max=i % 2 == 0, shifts=shifts)


@pytest.mark.parametrize("where", ["first", "last", "tile_end", "tile_start"])
def test_one_long_scope_over_several_tiles_and_misaligned_lines(harness, tmp_path, where):
    """F = 5, 5000 frames in a capacity of 5003, four channels: 20 runs a line, 100 a channel, 25 tiles of one run a wave, lines
    at every residue against 16 bytes; the row's maximum at the first element, the last, the last of a tile and the first of the
    next.  A tile's runs end at 16-byte boundaries of the destination line: the first tile of a line that starts sd elements
    behind one ends with frame 1023 - sd"""
    n, cap, F, ch = 5000, 5003, 5, 4
    base = M.source([n, 17], ch, F, cap, 1e-10, 5)
    base[0, :, :, :n] = np.minimum(base[0, :, :, :n], F32(100.0))
    for scope, inplace, shifts in ((M.ROW, False, (2, 3)), (M.CHANNEL, True, (1, 1))):
        sd = shifts[1]
        at = {"first": (0, 0, 0), "last": (ch - 1, F - 1, n - 1), "tile_end": (0, 0, 1023 - sd), "tile_start": (0, 0, 1024 - sd)}[where]
        x = base.copy()
        x[0][at] = 1e6
        _check(harness, tmp_path, x, [n, 17], [cap, 0], M.LOG10, scope, 1e-10, 8.0, inplace=inplace, shifts=shifts)


def test_rows_and_channels_do_not_leak(harness, tmp_path):
    """four rows with different maxima, the largest of each in channel 1 only: the two scopes differ exactly as the model does"""
    n = [30, 37, 5, 33]
    x = M.source(n, 2, 3, 37, 1e-10, 9)
    for r in range(4):
        x[r, :, :, :n[r]] = np.minimum(x[r, :, :, :n[r]], F32(1.0))
        x[r, 1, 2, n[r] - 1] = 10.0 ** (3 + 2 * r)
    outs = []
    for scope in (M.ROW, M.CHANNEL):
        _check(harness, tmp_path, x, n, [37] * 4, M.LOG10, scope, 1e-10, 8.0)
        outs.append(M.rows(x, n, [37] * 4, np.zeros_like(x), M.LOG10, scope, 1e-10, 8.0)[0])
    assert not np.array_equal(outs[0][:, 0], outs[1][:, 0]) and np.array_equal(outs[0][:, 1], outs[1][:, 1])


def test_python_parameter_errors_need_no_gpu():
    from lewton_amd.rows import LogCompress, Spectrogram
    for kw in [dict(log="log2"), dict(scope="batch"), dict(floor=0.0), dict(floor=-1.0), dict(floor=float("inf")), dict(floor=float("nan"), log=None),
               dict(top=-1.0), dict(top=float("nan")), dict(add=float("nan")), dict(mul=float("nan")), dict(floor="low")]:
        with pytest.raises(ValueError):
            LogCompress(**kw)
    for kw in [dict(pad_mode="edge"), dict(pad_mode="reflect", center=False), dict(pad_mode=None)]:
        with pytest.raises(ValueError):
            Spectrogram(**kw)
    assert LogCompress.WHISPER == dict(log="log10", floor=1e-10, top=8.0, add=4.0, mul=0.25, scope="row")
