"""The complex output of the spectral frames (lw_spec_params.output = LW_SPEC_OUT_COMPLEX, k_spec_complex) in the CPU suite:
tests/san/spec_complex_host.cpp links lw_spec.cpp against the HIP stand-ins under ASan / UBSan and runs the kernel source's own
phases for both outputs lane by lane (tests/test_host_spec.py says how).  The complex lines are the two chains of the contract
themselves; the power of the twin object is fmaf(im, im, re * re) of them; and a params struct with output = 0 is the object
lw_spec_create makes, byte for byte."""
import os

import numpy as np
import pytest

import spec_model as M
import spec_reflect_model as R
import host_harness as H
from common import ROOT
from host_harness import CS, UNSUPPORTED

SRC = [os.path.join(ROOT, "tests", "san", "spec_complex_host.cpp"), os.path.join(CS, "lw_spec.cpp")]
HANN, RECT = 0, 1
SENT = 0x7FC00ABC
# (n_fft, win_length, hop, window, center, pad mode, samples)
CASES = [(16, 16, 4, HANN, 1, 0, 150), (16, 16, 4, RECT, 0, 0, 150), (25, 25, 7, HANN, 1, 1, 333), (512, 400, 160, HANN, 1, 1, 1999),
         (512, 400, 160, HANN, 1, 0, 32 * 160), (1024, 1024, 256, HANN, 0, 0, 1024 + 256)]


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return H.build(tmp_path_factory, "spec_complex_host", SRC)


_run = H.run


def _spec(harness, tmp_path, case, x, output):
    """(raw destination bytes, basis bytes, the written lines [F][T])"""
    n_fft, win, hop, window, center, pad, _ = case
    src, dst, bas = (str(tmp_path / n) for n in ("x.bin", "y.bin", "b.bin"))
    np.asarray(x, np.float32).tofile(src)
    out = _run(harness, "run", n_fft, win, hop, window, center, pad, output, src, dst, bas)
    assert out[0] == "RC 0"
    F, T = [int(v) for v in out[1].split()[1:]]
    B = n_fft // 2 + 1
    assert (F, T) == (2 * B if output == 1 else B, M.n_frames(len(x), n_fft, hop, center))
    raw = np.fromfile(dst, np.float32).reshape(F, T + 1)
    assert (raw[:, T].view(np.uint32) == SENT).all()                      # nothing beyond the frames is written
    return open(dst, "rb").read(), open(bas, "rb").read(), raw[:, :T]


def chains(basis, X):
    """re and im of the contract, float32 [T][B] each: k ascending, one fmaf a step (spec_model.features without the power)"""
    re, im = (np.zeros((X.shape[0], basis.shape[2]), np.float32) for _ in range(2))
    for k in range(basis.shape[1]):
        re, im = M.fmaf(X[:, k:k + 1], basis[0][k][None, :], re), M.fmaf(X[:, k:k + 1], basis[1][k][None, :], im)
    return re, im


@pytest.mark.parametrize("case", CASES)
def test_complex_lines_are_the_chains_and_the_twins_power_is_their_fmaf(harness, tmp_path, case):
    n_fft, win, hop, window, center, pad, n = case
    B = n_fft // 2 + 1
    rng = np.random.default_rng(n_fft + n)
    x = rng.uniform(-1, 1, n).astype(np.float32)
    x[::9] *= np.float32(1e-22)                                           # squares among the subnormals
    _, bas_c, Z = _spec(harness, tmp_path, case, x, 1)
    _, bas_p, P = _spec(harness, tmp_path, case, x, 0)
    assert bas_c == bas_p                                                 # the table does not know the output
    basis = np.frombuffer(bas_c, np.float32).reshape(2, win, B)
    X = R.frame_matrix(x, n_fft, win, hop) if pad == 1 else M.frame_matrix(x, n_fft, win, hop, center)
    re, im = chains(basis, X)
    M.same_bits(Z[:B], re.T)
    M.same_bits(Z[B:], im.T)
    sq = Z[:B] * Z[:B]
    assert sq.dtype == np.float32
    M.same_bits(M.fmaf(Z[B:], Z[B:], sq), P)


@pytest.mark.parametrize("case", CASES[:3])
def test_output_zero_is_the_object_without_the_field_byte_for_byte(harness, tmp_path, case):
    x = np.random.default_rng(5).uniform(-1, 1, case[6]).astype(np.float32)
    new, old = _spec(harness, tmp_path, case, x, 0), _spec(harness, tmp_path, case, x, -1)
    assert new[0] == old[0] and new[1] == old[1]


def test_create_refusals(harness):
    # (n_fft, win, hop, window, center, n_mels, remove_dc, energy, output)
    for args in [(400, 400, 160, HANN, 1, 0, 0, 0, 2), (400, 400, 160, HANN, 1, 0, 0, 0, -1), (400, 400, 160, HANN, 1, 80, 0, 0, 1),
                 (400, 400, 160, HANN, 1, 0, 1, 0, 1), (400, 400, 160, HANN, 1, 0, 0, 1, 1)]:
        assert _run(harness, "create", *args) == ["RC %d" % UNSUPPORTED, "F 0"], args
    assert _run(harness, "create", 400, 400, 160, HANN, 1, 0, 0, 0, 1) == ["RC 0", "F 402"]
    assert _run(harness, "create", 400, 400, 160, 2, 0, 0, 0, 0, 1) == ["RC 0", "F 402"]                 # any window
    assert _run(harness, "create", 400, 400, 160, HANN, 1, 0, 0, 0, 0) == ["RC 0", "F 201"]
    assert _run(harness, "create", 400, 400, 160, HANN, 1, 80, 0, 1, 0) == ["RC 0", "F 81"]
