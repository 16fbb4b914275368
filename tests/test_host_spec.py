"""Spectral frames of rows (lw_spec_*, lw_spec_rows, k_spec) in the CPU suite: tests/san/spec_host.cpp links lw_spec.cpp against
the HIP stand-ins (tests/san/hip_standins.inc) under ASan / UBSan and compiles the kernel source itself, lw_kernels_spec.hip, for
the host (its route with per-lane fmaf chains), where its stand-in launcher runs it workgroup by workgroup and lane by lane.

The model is the rule of include/lewton_amd.h ("spectral frames of rows"): the tables in numpy float64, the indices in Python
integers, the chains in tests/spec_model.py.  What the kernel makes of real device memory, and whether the matrix instruction
gives the same bits, is checked on the GPU (tests/test_gpu_rows_spec.py)."""
import ctypes
import math
import os

import numpy as np
import pytest

import spec_model as M
import host_harness as H
from common import ROOT
from host_harness import CAPACITY, CS, NULL_ARG, UNSUPPORTED

SRC = [os.path.join(ROOT, "tests", "san", "spec_host.cpp"), os.path.join(CS, "lw_spec.cpp")]
HANN, RECT = 0, 1
SHAPES = [(400, 400, 160, HANN, 1), (512, 400, 160, HANN, 1), (16, 16, 4, RECT, 0), (25, 25, 7, HANN, 1), (64, 64, 100, HANN, 1),
          (32, 32, 1, HANN, 1), (2048, 2048, 512, HANN, 1), (2048, 1001, 65535, RECT, 0), (2, 1, 1, HANN, 0)]


# ---- the fmaf emulation both suites rest on

def _libm_fmaf():
    lib = ctypes.CDLL("libm.so.6")
    lib.fmaf.restype = ctypes.c_float
    lib.fmaf.argtypes = [ctypes.c_float] * 3
    return lambda a, b, c: np.array([lib.fmaf(float(x), float(y), float(z)) for x, y, z in zip(a, b, c)], np.float32)


def test_fmaf_emulation_is_glibc_fmaf_on_random_inputs():
    ref = _libm_fmaf()
    rng = np.random.default_rng(1)
    n = 20000
    a = rng.uniform(-2, 2, n).astype(np.float32)
    b = rng.uniform(-2, 2, n).astype(np.float32)
    c = (rng.uniform(-2, 2, n) * 10.0 ** rng.integers(-8, 3, n)).astype(np.float32)
    c[::5] = (-a[::5].astype(np.float64) * b[::5]).astype(np.float32)          # cancellation: the result is the product's tail
    a[1::97] *= np.float32(1e-30)                                               # ... and results among the subnormals
    b[1::97] *= np.float32(1e-12)
    c[1::97] *= np.float32(1e-42)
    got, want = M.fmaf(a, b, c), ref(a, b, c)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


def test_fmaf_emulation_is_glibc_fmaf_on_the_ties_the_naive_form_gets_wrong():
    """a * b = (2^46 + 1) 2^-60 = 2^-14 + 2^-60 exactly; c = M 2^-13 has ulp 2^-13, so a * b + c lies 2^-60 beside a float32 tie,
    which the float64 sum no longer holds: rounding that sum again goes to even, right for one parity of M only"""
    ref = _libm_fmaf()
    m = np.concatenate([np.arange(1 << 23, (1 << 23) + 2000), np.arange((1 << 24) - 2000, 1 << 24)]).astype(np.float64)
    assert (m % 2 == 1).sum() == (m % 2 == 0).sum()
    c = np.concatenate([m, -m]) * 2.0 ** -13
    a = np.full(len(c), 8392705 * 2.0 ** -30)
    b = np.full(len(c), 8384513 * 2.0 ** -30)
    for v in (a, b, c):
        assert np.array_equal(v.astype(np.float32).astype(np.float64), v)     # all three are float32 values
    assert 8392705 * 8384513 == (1 << 46) + 1
    a, b, c = (v.astype(np.float32) for v in (a, b, c))
    want = ref(a, b, c)
    naive_wrong = int((M.naive_fmaf(a, b, c).view(np.uint32) != want.view(np.uint32)).sum())
    wrong = int((M.fmaf(a, b, c).view(np.uint32) != want.view(np.uint32)).sum())
    print("ties: naive form wrong on %d of %d, emulation on %d" % (naive_wrong, len(c), wrong))
    assert wrong == 0 and 0.4 * len(c) <= naive_wrong <= 0.6 * len(c)


# ---- the host program

@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return H.build(tmp_path_factory, "spec_host", SRC)


_run = H.run


def _model_basis(n_fft, win, window):
    B, o = n_fft // 2 + 1, (n_fft - win) // 2
    i = np.arange(win, dtype=np.int64)
    w = 0.5 - 0.5 * np.cos(2 * np.pi * i / win) if window == HANN else np.ones(win)
    a = 2 * np.pi * (((i + o)[:, None] * np.arange(B, dtype=np.int64)[None, :]) % n_fft) / n_fft
    return np.stack([w[:, None] * np.cos(a), -w[:, None] * np.sin(a)])


@pytest.mark.parametrize("shape", SHAPES)
def test_basis_is_the_formula_rounded_once(harness, tmp_path, shape):
    n_fft, win, hop, window, center = shape
    path = str(tmp_path / "basis.bin")
    out = _run(harness, "basis", n_fft, win, hop, window, center, path)
    B = n_fft // 2 + 1
    assert out[0] == "G %d %d %d" % (B, B, (n_fft - win) // 2)
    got = np.fromfile(path, np.float32).reshape(2, win, B)
    want = _model_basis(n_fft, win, window)
    # two double evaluations differ by a few 1e-16; after the one rounding to f32 that is at most one f32 ulp.  Zeros of either
    # sign are equal (the comparison is on values)
    tol = np.spacing(np.abs(want).astype(np.float32)).astype(np.float64) + 1e-15
    err = np.abs(got.astype(np.float64) - want)
    assert (err <= tol).all(), (float(err.max()), np.argwhere(err > tol)[:4].tolist())
    if window == RECT:
        assert (got[0, :, 0] == 1).all() and (got[1, :, 0] == 0).all()
    elif win > 2:
        assert got[0, 0, 0] == 0 and np.count_nonzero(got[0]) > 0.5 * got[0].size


def test_frame_counts_and_first_indices_in_64_bits(harness):
    lens = [0, 1, 2, 15, 16, 17, 159, 160, 399, 400, 401, (1 << 31) - 1, 1 << 31, (1 << 32) + 5, (1 << 40) - 3, 1 << 40]
    for n_fft, win, hop, window, center in SHAPES:
        out = _run(harness, "frames", n_fft, win, hop, window, center, *lens)
        got = [tuple(int(x) for x in ln.split()[1:]) for ln in out if ln.startswith("L ")]
        want = [(n, M.n_frames(n, n_fft, hop, center)) for n in lens]
        assert got == want
        # the first input index of a frame by the kernel's own index functions (a tile's 64-bit start plus a 32-bit offset)
        frames = sorted({0, 1, 31, 32, 33, 1000} | {f - 1 for _, f in want if 0 < f < 1 << 37})
        out = _run(harness, "index", n_fft, win, hop, window, center, *frames)
        got = [tuple(int(x) for x in ln.split()[1:]) for ln in out if ln.startswith("I ")]
        assert got == [(f, f * hop - (n_fft // 2 if center else 0)) for f in frames]


CREATE_REFUSALS = [((1, 1, 1, HANN, 1, 0, 0), UNSUPPORTED), ((2049, 400, 160, HANN, 1, 0, 0), UNSUPPORTED), ((400, 0, 160, HANN, 1, 0, 0), UNSUPPORTED),
                   ((400, 401, 160, HANN, 1, 0, 0), UNSUPPORTED), ((400, 400, 0, HANN, 1, 0, 0), UNSUPPORTED),
                   ((400, 400, 65536, HANN, 1, 0, 0), UNSUPPORTED), ((400, 400, 160, 2, 1, 0, 0), UNSUPPORTED),
                   ((400, 400, 160, -1, 1, 0, 0), UNSUPPORTED), ((400, 400, 160, HANN, 1, 257, 1), UNSUPPORTED),
                   ((400, 400, 160, HANN, 1, 80, 0), NULL_ARG)]


def test_create_refusals_and_the_limits(harness):
    for args, code in CREATE_REFUSALS:
        assert _run(harness, "create", *args) == ["RC %d" % code], args
    for args in [(2, 1, 1, HANN, 0, 0, 0), (2048, 2048, 65535, RECT, 1, 256, 1), (400, 400, 160, HANN, 1, 80, 1), (400, 400, 160, HANN, 1, 0, 1)]:
        assert _run(harness, "create", *args) == ["RC 0"], args


ROW_REFUSALS = [("null_sp", NULL_ARG), ("null_len", NULL_ARG), ("null_src", NULL_ARG), ("null_dst", NULL_ARG),
                ("i16", UNSUPPORTED), ("i16_interleaved", UNSUPPORTED), ("bad_fmt", UNSUPPORTED),
                ("ch0", CAPACITY), ("ch256", CAPACITY), ("len_over", CAPACITY), ("frames_over", CAPACITY), ("row_over", CAPACITY),
                ("row_over_identity", CAPACITY), ("row_twice", CAPACITY), ("row_twice_empty", CAPACITY), ("bad_route", UNSUPPORTED)]


@pytest.mark.parametrize("case,code", ROW_REFUSALS)
def test_refusals_launch_nothing(harness, case, code):
    assert _run(harness, "refuse", case) == ["RC %d" % code, "LAUNCHES 0"]


def test_exactly_full_is_accepted_on_both_routes(harness):
    for case in ("ok", "ok_exact", "ok_route1"):                          # ok_exact: len == src_capacity, n_frames == frame_capacity
        assert _run(harness, "refuse", case) == ["RC 0", "LAUNCHES 1"]


def test_a_row_of_more_tiles_than_a_launch_holds_takes_several(harness):
    """2^30 + 1 frames are 2^25 + 1 tiles of 32; a grid dimension holds fewer than 2^32 lanes, 2^24 - 1 workgroups of 256 (a launch
    past that is accepted, and workgroups of it never run: tests/rows_long_row_gpu_cases.py found frames left unwritten under
    LW_OK).  The tiles go out in launches of at most 2^24 - 1, each with its tile0, and cover the row exactly once"""
    out = _run(harness, "refuse", "ok_many_tiles")
    assert out[:2] == ["RC 0", "LAUNCHES 3"]
    tiles = [tuple(int(v) for v in line.split()[1:]) for line in out[2:]]
    assert tiles == [(0, 0xFFFFFF), (0xFFFFFF, 0xFFFFFF), (2 * 0xFFFFFF, 3)]
    assert sum(n for _, n in tiles) == -(-((1 << 30) + 1) // 32) and all(n * 256 < 1 << 32 for _, n in tiles)


def test_two_calls_back_to_back_each_reach_their_own_lengths(harness):
    """the second call's records do not replace the first's, which its kernel reads later; the caller's array is free at once"""
    out = _run(harness, "two")
    assert out == ["RC 0", "RC 0", "ROWS 1000/7/2 0/0/0 441/3/3", "ROWS 7/1/0 8/1/1 159/1/2", "LAUNCHES 2"]


@pytest.mark.parametrize("seed", [1, 2])
def test_kernel_on_the_host_is_bit_identical_to_the_scalar_chain(harness, seed):
    """the kernel source (route 1) lane by lane under ASan against scalar fmaf chains over the library's own tables: the listed
    shapes first -- (400, 400, 160) with the ten lengths over two channels, (512, 400, 160), (16, 16, 4) rect not centred,
    (25, 25, 7), (64, 64, 100), (32, 32, 1), (2048, 2048, 512) on one short row, 0 / 1 / 80 / 128 mel bands, a row of exactly a
    tile of frames and one of a frame more -- then random ones; both formats, 1-3 channels, odd exact-size capacities, NaN between
    len and the capacity, a sentinel in the destination, reversed destination rows with a gap"""
    out = _run(harness, "kernel", seed, 40)
    assert out[-1] == "OK 40", out[-3:]
    cases = [ln.split() for ln in out if ln.startswith("CASE ")]
    assert {c[c.index("route") + 1] for c in cases} == {"1", "-1"}           # (-1: a case without a frame queues nothing)
    assert {c[7] for c in cases} >= {"mels0", "mels1", "mels80", "mels128"} and {c[8] for c in cases} == {"fmt2", "fmt3"}
    assert {(c[2], c[3], c[4]) for c in cases} >= {("fft%d" % a, "win%d" % b, "hop%d" % h) for a, b, h, _, _ in SHAPES[:7]}


def _power(harness, tmp_path, shape, x):
    n_fft, win, hop, window, center = shape
    src, dst = str(tmp_path / "x.bin"), str(tmp_path / "p.bin")
    np.asarray(x, np.float32).tofile(src)
    out = _run(harness, "run", n_fft, win, hop, window, center, src, dst)
    assert out[0] == "RC 0"
    B, T = [int(v) for v in out[1].split()[1:]]
    assert (B, T) == (n_fft // 2 + 1, M.n_frames(len(x), n_fft, hop, center))
    return np.fromfile(dst, np.float32).reshape(B, T)


def test_dc_through_a_rectangular_window_is_exact(harness, tmp_path):
    """every product is x and every partial sum a multiple of x below 2^24 x: nothing rounds, P[0] = (win_length x)^2"""
    P = _power(harness, tmp_path, (16, 16, 4, RECT, 0), np.full(64, 0.25, np.float32))
    assert P.shape == (9, 13) and (P[0] == 16 * 16 * 0.25 * 0.25).all()
    assert (P[1:] < 1e-10).all()
    P = _power(harness, tmp_path, (64, 40, 8, RECT, 0), np.full(200, 0.5, np.float32))
    assert (P[0] == 40 * 40 * 0.25).all()


def test_a_sine_on_a_bin_centre_peaks_at_that_bin(harness, tmp_path):
    for shape, j in (((64, 64, 16, RECT, 0), 5), ((400, 400, 160, HANN, 1), 50), ((512, 400, 160, HANN, 0), 100)):
        n_fft = shape[0]
        x = np.sin(2 * np.pi * j * np.arange(2000) / n_fft).astype(np.float32)
        P = _power(harness, tmp_path, shape, x)
        inner = P[:, 2:-3]                                                # frames that lie wholly inside the row
        assert inner.shape[1] > 3 and (inner.argmax(0) == j).all()
        # ... and the chains of the model give these very bits
        basis = np.fromfile(_basis_file(harness, tmp_path, shape), np.float32).reshape(2, shape[1], n_fft // 2 + 1)
        want = M.features(basis, None, M.frame_matrix(x, n_fft, shape[1], shape[2], shape[4]))
        M.same_bits(P.T, want)


def _basis_file(harness, tmp_path, shape):
    path = str(tmp_path / "b.bin")
    _run(harness, "basis", *shape, path)
    return path


# ---- the mel matrix

def _mel(f, scale):
    if scale == "htk":
        return 2595.0 * math.log10(1.0 + f / 700.0)
    return f / (200.0 / 3) if f < 1000.0 else 15.0 + math.log(f / 1000.0) / (math.log(6.4) / 27.0)


def _hz(m, scale):
    if scale == "htk":
        return 700.0 * (10.0 ** (m / 2595.0) - 1.0)
    return m * (200.0 / 3) if m < 15.0 else 1000.0 * math.exp((m - 15.0) * (math.log(6.4) / 27.0))


def _points(sample_rate, n_mels, fmin, fmax, scale):
    lo, hi = _mel(fmin, scale), _mel(fmax, scale)
    return [_hz(lo + (hi - lo) * i / (n_mels + 1), scale) for i in range(n_mels + 2)]


@pytest.mark.parametrize("scale,norm", [("htk", None), ("slaney", None), ("slaney", "slaney"), ("htk", "slaney")])
@pytest.mark.parametrize("cfg", [(16000, 400, 80, 0.0, None), (16000, 2048, 40, 20.0, 7600.0), (44100, 1024, 128, 0.0, None)])
def test_mel_filterbank_is_the_stated_rule(cfg, scale, norm):
    from lewton_amd.rows import mel_filterbank
    sr, n_fft, n_mels, fmin, fmax = cfg
    fb = mel_filterbank(sr, n_fft, n_mels, fmin=fmin, fmax=fmax, scale=scale, norm=norm)
    B = n_fft // 2 + 1
    assert fb.shape == (n_mels, B) and fb.dtype == np.float32 and (fb >= 0).all()
    p = _points(sr, n_mels, fmin, sr / 2 if fmax is None else fmax, scale)
    want = np.zeros((n_mels, B))
    for q in range(n_mels):
        for j in range(B):
            f = j * sr / n_fft
            w = max(0.0, min((f - p[q]) / (p[q + 1] - p[q]), (p[q + 2] - f) / (p[q + 2] - p[q + 1])))
            want[q, j] = w * (2.0 / (p[q + 2] - p[q]) if norm else 1.0)
    # two float64 evaluations of the points (numpy's and math's log / pow) differ by a few ulp of a frequency of up to 22 kHz,
    # 1e-11 Hz, over a slope of at least a hundredth of a hertz: 1e-9 on a weight, plus the one rounding to float32
    assert np.abs(fb.astype(np.float64) - want).max() <= 1e-8 + 2.0 ** -24 * want.max()
    df = sr / n_fft
    for q in range(n_mels):
        apex = p[q + 1] / df
        if fb[q].max() == 0:                                            # a triangle narrower than a bin can fall between two
            assert p[q + 2] - p[q] < 2 * df
            continue
        peak = int(fb[q].argmax())
        if p[q + 1] - p[q] >= df and p[q + 2] - p[q + 1] >= df:
            # the peak is one of the two bins around the apex; it is the nearer one unless the apex lies close to half way, where the
            # gentler falling slope can favour the farther bin (the slopes of neighbours differ by less than 1.5 here)
            assert peak in (math.floor(apex), math.ceil(apex)), (q, peak, apex)
            if abs(apex - math.floor(apex) - 0.5) > 0.1:
                assert peak == round(apex), (q, peak, apex)
    if norm:
        plain = mel_filterbank(sr, n_fft, n_mels, fmin=fmin, fmax=fmax, scale=scale)
        for q in range(n_mels):
            on = plain[q] > 1e-3
            ratio = fb[q][on].astype(np.float64) / plain[q][on]
            assert np.abs(ratio * (p[q + 2] - p[q]) / 2 - 1).max(initial=0) <= 1e-4          # each row times 2 / (p[q+2] - p[q])
        wide = [q for q in range(n_mels) if p[q + 2] - p[q] >= 20 * df]
        if cfg[1] == 2048:
            assert wide
        for q in wide:                                                  # ... which gives a triangle sampled that finely unit area
            assert abs(fb[q].astype(np.float64).sum() * df - 1) <= 0.01


def test_htk_and_slaney_differ_and_bad_parameters_are_refused_without_a_gpu():
    from lewton_amd import rows as R
    a, b = R.mel_filterbank(16000, 400, 80), R.mel_filterbank(16000, 400, 80, scale="slaney")
    assert np.abs(a - b).max() > 0.1
    assert not np.array_equal(R.mel_filterbank(16000, 400, 80, norm="slaney"), a)
    for kw in [dict(scale="bark"), dict(norm="l1"), dict(n_mels=0), dict(n_mels=257), dict(n_fft=1), dict(fmin=9000.0), dict(fmax=0.0)]:
        args = dict(sample_rate=16000, n_fft=400, n_mels=80)
        args.update(kw)
        with pytest.raises(ValueError):
            R.mel_filterbank(**args)
    for kw in [dict(n_fft=1), dict(n_fft=2049), dict(n_fft=400.0), dict(hop=0), dict(hop=65536), dict(win_length=0), dict(win_length=401),
               dict(window="blackman"), dict(mel=np.zeros((80, 200), np.float32)), dict(mel=np.zeros((257, 201), np.float32)),
               dict(mel=np.zeros(201, np.float32)), dict(n_fft=True)]:
        with pytest.raises(ValueError):
            R.Spectrogram(**kw)
