"""Reflect padding of the spectral frames (LW_SPEC_PAD_REFLECT) in the CPU suite: tests/san/spec_reflect_host.cpp links lw_spec.cpp
against the HIP stand-ins under ASan / UBSan and runs the kernel source itself, lw_kernels_spec.hip (its route with per-lane fmaf
chains), lane by lane over an exact-size row, so a reflected index outside [0, len) is a sanitizer report.

The model: the frames of tests/spec_model.py, uncentred, over the row padded by numpy (tests/spec_reflect_model.py); the reflected
indices in Python integers.  Route 0 and real device memory are checked on the GPU (tests/test_gpu_rows_feat.py)."""
import os

import numpy as np
import pytest

import spec_model as M
import spec_reflect_model as RM
import host_harness as H
from common import ROOT
from host_harness import CAPACITY, CS, NULL_ARG, UNSUPPORTED

SRC = [os.path.join(ROOT, "tests", "san", "spec_reflect_host.cpp"), os.path.join(CS, "lw_spec.cpp")]
HANN, RECT = 0, 1
ZERO, REFLECT = 0, 1


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return H.build(tmp_path_factory, "spec_reflect_host", SRC)


_run = H.run


@pytest.mark.parametrize("n_fft", [400, 25, 16, 32, 2048, 2])
def test_reflected_indices_are_python_integers(harness, n_fft):
    """every index a support sample can have, from -(n_fft / 2) to len - n_fft / 2 + n_fft - 1, lands inside the row after one
    reflection -- at the shortest row that is accepted, one sample more, and 2^40 samples (64-bit indices)"""
    pad, L = n_fft // 2, RM.min_len(n_fft)
    for n in (L, L + 1, 1 << 40):
        top = n - pad + n_fft - 1
        want = sorted(i for i in {-pad, -pad + 1, -1, 0, 1, n // 2, n - 2, n - 1, n, n + 1, top - 1, top} if -pad <= i <= top)
        out = _run(harness, "index", n, *want)
        assert out == ["X %d %d" % (i, RM.index(i, n)) for i in want]
    assert RM.index(-pad, L) == pad and RM.index(L - pad + n_fft - 1, L) in (0, 1)      # the limit leaves no sample to spare


def test_set_pad_mode_refusals(harness):
    assert _run(harness, "mode", 1, REFLECT) == ["RC 0 MODE 1"]
    assert _run(harness, "mode", 1, ZERO) == ["RC 0 MODE 0"]
    assert _run(harness, "mode", 0, ZERO) == ["RC 0 MODE 0"]
    assert _run(harness, "mode", 0, REFLECT) == ["RC %d MODE 0" % UNSUPPORTED]            # not centred
    assert _run(harness, "mode", 1, 2) == ["RC %d MODE 0" % UNSUPPORTED]
    assert _run(harness, "mode", 1, -1) == ["RC %d MODE 0" % UNSUPPORTED]
    assert _run(harness, "mode", "null", REFLECT) == ["RC %d MODE -1" % NULL_ARG]


@pytest.mark.parametrize("shape", [(400, 400, 160), (25, 25, 7), (16, 16, 4), (32, 32, 1), (512, 400, 160), (2, 1, 1)])
def test_a_row_one_sample_short_is_refused_before_anything_is_queued(harness, shape):
    L = RM.min_len(shape[0])
    assert _run(harness, "refuse", *shape, L - 1) == ["RC %d" % CAPACITY, "LAUNCHES 0"]
    if L > 2:
        assert _run(harness, "refuse", *shape, 1) == ["RC %d" % CAPACITY, "LAUNCHES 0"]
    assert _run(harness, "refuse", *shape, L) == ["RC 0", "LAUNCHES 1"]
    assert _run(harness, "refuse", *shape, 0) == ["RC 0", "LAUNCHES 1"]                   # an empty row yields no frames


def _power(harness, tmp_path, shape, x, modes):
    n_fft, win, hop, window = shape
    src, dst = str(tmp_path / "x.bin"), str(tmp_path / "p.bin")
    np.asarray(x, np.float32).tofile(src)
    out = _run(harness, "run", n_fft, win, hop, window, modes, src, dst)
    assert out[0] == "RC 0"
    B, T = [int(v) for v in out[1].split()[1:]]
    assert (B, T) == (n_fft // 2 + 1, M.n_frames(len(x), n_fft, hop, True))
    return np.fromfile(dst, np.float32).reshape(B, T)


def _basis(harness, tmp_path, shape):
    path = str(tmp_path / "b.bin")
    _run(harness, "basis", *shape, path)
    return np.fromfile(path, np.float32).reshape(2, shape[1], shape[0] // 2 + 1)


SHAPES = {(400, 400, 160, HANN): [201, 202, 1600, 1601], (16, 16, 4, RECT): [9, 10, 64, 67], (25, 25, 7, HANN): [14, 21, 70, 71],
          (32, 32, 1, HANN): [17, 18, 100]}


@pytest.mark.parametrize("shape", list(SHAPES))
def test_kernel_on_the_host_under_reflect_is_the_model_on_the_padded_row(harness, tmp_path, shape):
    """the kernel source (route 1) bit-identical to the uncentred model on numpy.pad(x, mode="reflect"): from the shortest row,
    lengths the hop divides ((25, 25, 7): the frame at len / hop, which torch's padding does not reach) and does not"""
    basis = _basis(harness, tmp_path, shape)
    rng = np.random.default_rng(shape[0])
    for n in SHAPES[shape]:
        x = rng.uniform(-1, 1, n).astype(np.float32)
        P = _power(harness, tmp_path, shape, x, "1")
        want = M.features(basis, None, RM.frame_matrix(x, shape[0], shape[1], shape[2]))
        M.same_bits(P.T, want)
        zero = M.features(basis, None, M.frame_matrix(x, shape[0], shape[1], shape[2], True))
        assert not np.array_equal(zero[0], want[0]) and not np.array_equal(zero[-1], want[-1])


def test_zero_mode_after_a_switch_back_is_a_fresh_objects(harness, tmp_path):
    shape = (400, 400, 160, HANN)
    x = np.random.default_rng(5).uniform(-1, 1, 1000).astype(np.float32)
    fresh, back = _power(harness, tmp_path, shape, x, "0"), _power(harness, tmp_path, shape, x, "10")
    assert np.array_equal(fresh.view(np.uint32), back.view(np.uint32))
    again = _power(harness, tmp_path, shape, x, "101")
    assert np.array_equal(again.view(np.uint32), _power(harness, tmp_path, shape, x, "1").view(np.uint32))
    assert not np.array_equal(fresh[:, 0], again[:, 0]) and np.array_equal(fresh[:, 2:-3].view(np.uint32), again[:, 2:-3].view(np.uint32))
    basis = _basis(harness, tmp_path, shape)
    M.same_bits(fresh.T, M.features(basis, None, M.frame_matrix(x, 400, 400, 160, True)))


def _front_end(seed):
    """(the models' features, the float64 formula's) [80][101] of one second of a chirp with noise 40 dB below it"""
    from lewton_amd.rows import LogCompress, mel_filterbank
    import feat_model as FM
    rng = np.random.default_rng(seed)
    t = np.arange(16000) / 16000.0
    x = (0.5 * np.sin(2 * np.pi * (100.0 * t + 0.5 * 7000.0 * t * t)) + 0.005 * rng.standard_normal(16000)).astype(np.float32)
    fb = mel_filterbank(16000, 400, 80, scale="slaney", norm="slaney")
    w = LogCompress.WHISPER
    # the formula in float64
    xp = np.pad(x.astype(np.float64), 200, "reflect")
    win = 0.5 - 0.5 * np.cos(2 * np.pi * np.arange(400) / 400)
    frames = np.stack([xp[i * 160:i * 160 + 400] * win for i in range(101)])
    mel = fb.astype(np.float64) @ (np.abs(np.fft.rfft(frames, axis=1)) ** 2).T
    l = np.log10(np.maximum(mel, np.float64(np.float32(w["floor"]))))
    ref = (np.maximum(l, l.max() - w["top"]) + w["add"]) * w["mul"]
    return x, fb, w, FM, ref


def test_the_whole_front_end_against_the_formula_in_float64(harness, tmp_path):
    """reflect frames (400, 160), 80 Slaney bands, LogCompress.whisper(), through the models (whose bits are the GPU's, by
    tests/test_gpu_rows_feat.py) against numpy.fft.rfft on the reflect-padded signal and a float64 logarithm.  Measured once on
    this signal (seed 1): the largest absolute difference of a feature is 1.045e-5 (MEASURED_MAX, rounded); four times that is
    asserted, the factor for other seeds, not for other algorithms.  (Features span [-0.58, 1.42] here.  1e-5 of a feature is 4e-5
    of a decade, 1e-4 relative on a band's power: the size to expect in a quiet band, whose bins hold the rounding noise that the
    loud chirp leaves in the 400-term f32 chains)"""
    MEASURED_MAX = 1.05e-5
    shape = (400, 400, 160, HANN)
    basis = _basis(harness, tmp_path, shape)
    for seed in (1, 2, 3):
        x, fb, w, FM, ref = _front_end(seed)
        lin = M.features(basis, fb, RM.frame_matrix(x, 400, 400, 160)).T[None, None]          # [1][1][80][101]
        got, _ = FM.rows(lin, [101], None, lin, FM.LOGS[w["log"]], FM.ROW, w["floor"], w["top"], w["add"], w["mul"])
        err = float(np.abs(got[0, 0].astype(np.float64) - ref).max())
        print("seed %d: largest absolute difference %.3e, features in [%.3f, %.3f]" % (seed, err, ref.min(), ref.max()))
        assert err <= 4 * MEASURED_MAX
