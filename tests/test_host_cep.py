"""Cepstra and deltas of feature rows (lw_cep_*, lw_cep_rows, k_cep) in the CPU suite: tests/san/cep_host.cpp links lw_cep.cpp
against the HIP stand-ins (tests/san/hip_standins.inc) under ASan / UBSan and compiles the kernel source itself,
lw_kernels_cep.hip, for the host, where its stand-in launcher runs it workgroup by workgroup and phase by phase over exact-size
buffers.

The model is the rule of include/lewton_amd.h ("cepstra and deltas of feature rows") in numpy (tests/cep_model.py).  What the
kernel makes of real device memory, LDS and the barriers is checked on the GPU (tests/test_gpu_rows_cep.py)."""
import itertools
import os

import numpy as np
import pytest

import cep_model as M
import host_harness as H
from common import ROOT
from host_harness import CAPACITY, CS, DEVICE, NULL_ARG, OK, UNSUPPORTED

SRC = [os.path.join(ROOT, "tests", "san", "cep_host.cpp"), os.path.join(CS, "lw_cep.cpp")]
F32, F64 = np.float32, np.float64


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return H.build(tmp_path_factory, "cep_host", SRC)


_run = H.run


# ---- refusals, and what is queued

# (n_in, n_out, matrix, order, width)
CREATE = [((0, 5, "ones", 0, 0), UNSUPPORTED), ((257, 5, "ones", 0, 0), UNSUPPORTED), ((7, 0, "ones", 0, 0), UNSUPPORTED),
          ((7, 257, "ones", 0, 0), UNSUPPORTED), ((7, 5, "ones", 3, 2), UNSUPPORTED), ((7, 5, "ones", 1, 0), UNSUPPORTED),
          ((7, 5, "ones", 2, 17), UNSUPPORTED), ((7, 5, "ones", 0, 2), UNSUPPORTED), ((7, 5, "null", 0, 0), NULL_ARG),
          ((7, 5, "null", 2, 2), NULL_ARG), ((7, 5, "ones", 0, 0), OK), ((7, 7, "null", 0, 0), OK), ((256, 256, "ones", 2, 16), OK),
          ((1, 1, "null", 1, 1), OK), ((256, 256, "null", 2, 16), OK)]


def test_create_refusals(harness):
    for args, code in CREATE:
        assert _run(harness, "create", *args) == ["RC %d" % code], args
    ok = (7, 5, "ones", 2, 2)
    for device, code in ((0, OK), (1, DEVICE), (-1, DEVICE), (1 << 20, DEVICE)):              # the stand-ins have one device
        assert _run(harness, "create", *ok, device) == ["RC %d" % code], device
    assert _run(harness, "create", 7, 5, "ones", 3, 2, 1) == ["RC %d" % UNSUPPORTED]           # parameters are judged first


ROW_REFUSALS = [("null_cp", NULL_ARG), ("null_n", NULL_ARG), ("null_src", NULL_ARG), ("null_dst", NULL_ARG),
                ("null_dst_fill_only", NULL_ARG), ("n_over", CAPACITY), ("fill_over", CAPACITY), ("ch0", CAPACITY), ("ch256", CAPACITY),
                ("too_large", CAPACITY), ("too_many_tiles", CAPACITY)]


@pytest.mark.parametrize("case,code", ROW_REFUSALS)
def test_refusals_queue_nothing(harness, case, code):
    assert _run(harness, "refuse", case) == ["RC %d" % code, "LAUNCHES 0", "LAST -1"]


def test_accepted_calls_and_their_launches(harness):
    """one launch whatever the order; none without rows, with all rows empty and nothing to fill; one for a fill alone"""
    for case, n in (("ok", 1), ("ok_no_rows", 0), ("ok_nothing", 0), ("ok_fill_only", 1), ("ok_order0", 1), ("ok_order1", 1),
                    ("ok_most_tiles", 1)):                                   # 2^24 - 1 tiles: the most a launch is given
        assert _run(harness, "refuse", case) == ["RC 0", "LAUNCHES %d" % n, "LAST %d" % n], case


def test_two_calls_back_to_back_each_reach_their_own_records(harness):
    """the second call's records do not replace the first's, which its kernel reads later; the caller's arrays are free at once"""
    out = _run(harness, "two")
    assert out == ["RC 0 LAST 1", "RC 0 LAST 1", "ROWS 300/300 0/3 4/4", "ROWS 1/1 257/257 3/3", "LAUNCHES 2"]


def test_delta_weights_are_one_division_rounded_once(harness):
    for N in range(1, 17):
        out = _run(harness, "weights", N)
        D = 2 * sum(n * n for n in range(1, N + 1))
        want = [F32(F64(n) / F64(D)) for n in range(1, N + 1)]
        assert out == ["W " + " ".join("%08x" % int(np.array(w, F32).view(np.uint32)) for w in want), "N %d" % N]
        assert np.array_equal(M.delta_weights(N).view(np.uint32), np.array(want, F32).view(np.uint32))
    assert _run(harness, "weights", 0) == ["W", "N 0"]


# ---- the kernel source on the host

def _kernel(harness, tmp_path, x, n, fill_to, matrix, n_out, order, N, shifts=(0, 0)):
    R, C, n_in, cap = x.shape
    src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(src, "wb") as f:
        f.write(np.asarray(n, np.uint64).tobytes())
        f.write(np.asarray(fill_to if fill_to is not None else [0] * R, np.uint64).tobytes())
        f.write(np.ascontiguousarray(matrix if matrix is not None else np.zeros((n_out, n_in)), F32).tobytes())
        f.write(np.ascontiguousarray(x, F32).tobytes())
    out = _run(harness, "run", n_in, n_out, int(matrix is None), order, N if order else 0, C, R, cap, int(fill_to is not None), shifts[0], shifts[1],
               src, dst)
    assert out[0] == "RC 0" and out[2] == "TILE %d" % (256 - 2 * order * N if order else 256)
    return np.fromfile(dst, F32).reshape(R, C, n_out * (1 + order), cap), int(out[1].split()[1])


def _check(harness, tmp_path, x, n, fill_to, matrix, order, N, shifts=(0, 0)):
    n_out = x.shape[2] if matrix is None else matrix.shape[0]
    got, launches = _kernel(harness, tmp_path, x, n, fill_to, matrix, n_out, order, N, shifts)
    want = M.rows(x, n, fill_to, np.full(got.shape, M.SENT_F, F32), matrix, order, N)
    M.same_bits(got, want, M.SENT)
    assert launches == int(max(max(n), max(fill_to) if fill_to is not None else 0) > 0)
    return want


FILLS = {"none": lambda n, cap: None, "n": lambda n, cap: list(n), "capacity": lambda n, cap: [cap] * len(n),
         "below": lambda n, cap: [max(0, v - 2) for v in n], "mixed": lambda n, cap: [min(cap, (v * 7 + 3) % (cap + 1)) for v in n]}
BASE_N = [0, 1, 2, 3, 4, 5, 8, 9, 255, 256, 257, 1031]


@pytest.mark.parametrize("order", [0, 1, 2])
def test_kernel_on_the_host_is_the_model_on_the_base_shape(harness, tmp_path, order):
    """[12][2][7][1031] -> 5 cepstra (or the 7 lines themselves) with n_frames = 0, 1, 2, 3, 4, 5, 8, 9, 255, 256, 257, 1031 over the
    rows of one call -- rows shorter than N, than 2N and than 4N, where the two clamps overlap, and rows of several tiles: N = 1
    and 2, a matrix and the identity, every kind of fill_to, source and destination lines at every residue against 16 bytes (1031
    is odd; the buffers' own starts are shifted as well): every element of a sentinel-filled exact-size destination, the sentinel
    NaN in the source at and beyond n_frames"""
    combos = list(itertools.product((1, 2) if order else (0,), (False, True)))
    for i, (N, identity) in enumerate(combos):
        for k, fill in enumerate(sorted(FILLS)):
            x = M.source(BASE_N, 2, 7, 1031, 100 + 10 * i + k)
            _check(harness, tmp_path, x, BASE_N, FILLS[fill](BASE_N, 1031), None if identity else M.matrix(5, 7, 7 + i), order, N,
                   shifts=((i + k) % 4, (i // 2 + 2 * k + 1) % 4))


def test_wide_windows_and_output_groups_on_the_host(harness, tmp_path):
    """N = 16 over rows shorter than the window and of two tiles; 33 outputs cross an accumulator group, 80 -> 13 is the headline"""
    n = [1, 16, 17, 32, 33, 64, 65, 300]
    x = M.source(n, 1, 7, 301, 3)
    _check(harness, tmp_path, x, n, None, M.matrix(5, 7, 1), 2, 16, shifts=(1, 3))
    _check(harness, tmp_path, x, n, [301] * 8, None, 1, 16, shifts=(2, 0))
    n = [40, 3]
    _check(harness, tmp_path, M.source(n, 1, 9, 41, 4), n, [0, 41], M.matrix(33, 9, 2), 2, 2)
    _check(harness, tmp_path, M.source(n, 1, 80, 41, 5), n, None, M.matrix(13, 80, 3), 2, 2)
    _check(harness, tmp_path, M.source(n, 1, 33, 41, 6), n, None, None, 2, 3)


def test_special_values_on_the_host(harness, tmp_path):
    """NaN, +-inf, +-0, subnormals and FLT_MAX in the data: every bit that is not a NaN is the model's, the sign of a zero
    included; the identity's static lines are a bit copy, NaN payloads too"""
    n = [300] * 9
    x = M.source(n, 1, 7, 301, 31, special=True)
    _check(harness, tmp_path, x, n, None, M.matrix(5, 7, 9), 2, 2)
    want = _check(harness, tmp_path, x, n, None, None, 2, 2)
    assert np.array_equal(want[:, :, :7, :300].view(np.uint32), x[:, :, :, :300].view(np.uint32))
    got, _ = _kernel(harness, tmp_path, x, n, None, None, 7, 2, 2)
    assert np.array_equal(got[:, :, :7, :300].view(np.uint32), x[:, :, :, :300].view(np.uint32))


def test_rows_do_not_leak(harness, tmp_path):
    """rows of different lengths and an empty row between them give the bits each gives alone"""
    n = [300, 0, 1000, 17]
    x = M.source(n, 2, 7, 1000, 41)
    m = M.matrix(5, 7, 4)
    want = _check(harness, tmp_path, x, n, [1000, 5, 0, 20], m, 2, 2)
    assert (want[1, :, :, :5] == 0).all() and (want[1, :, :, 5:].view(np.uint32) == M.SENT).all()
    together, _ = _kernel(harness, tmp_path, x, n, [1000, 5, 0, 20], m, 5, 2, 2)
    for r in range(4):                                                       # ... each row alone through the kernel source
        alone, _ = _kernel(harness, tmp_path, x[r:r + 1], n[r:r + 1], None, m, 5, 2, 2)
        M.same_bits(alone[:, :, :, :n[r]], together[r:r + 1, :, :, :n[r]])
        assert (alone[:, :, :, n[r]:].view(np.uint32) == M.SENT).all()


# ---- dct_matrix

def test_dct_matrix_properties():
    from lewton_amd.rows import dct_matrix
    for n_out, n_in, norm, lifter in ((13, 80, "ortho", 0), (13, 40, "ortho", 22), (40, 40, "ortho", 0), (20, 128, None, 0), (5, 7, None, 22),
                                      (256, 256, "ortho", 0), (1, 1, "ortho", 0)):
        m = dct_matrix(n_out, n_in, norm, lifter)
        assert m.dtype == F32 and m.shape == (n_out, n_in)
        assert np.array_equal(m.view(np.uint32), M.dct_reference(n_out, n_in, norm, lifter).view(np.uint32)), (n_out, n_in, norm, lifter)
        assert (m[0] == m[0, 0]).all()                                                  # row 0 is constant
    for n in (7, 40, 80, 256):
        m = dct_matrix(n, n, "ortho").astype(F64)
        assert np.abs(m @ m.T - np.eye(n)).max() < 1e-6
    plain, lift = dct_matrix(13, 40).astype(F64), dct_matrix(13, 40, lifter=22).astype(F64)
    factor = 1.0 + 11.0 * np.sin(np.pi * np.arange(13) / 22.0)
    assert np.abs(lift - plain * factor[:, None]).max() <= 2.0 ** -23 * np.abs(lift).max()
    assert np.array_equal(dct_matrix(13, 40, None).astype(F64)[0], np.full(40, 2.0))


# ---- the model's accuracy, by a bound that is derived, not measured

@pytest.mark.parametrize("n_in,n_out", [(7, 5), (80, 13), (128, 40), (256, 128)])
def test_the_models_static_lines_are_within_their_bound_of_the_exact_sums(n_in, n_out):
    """|chain - exact| <= (n_in + 1) * 2^-24 * sum_f |x_f| |M_qf|: the chain makes n_in roundings, each at most half an ulp (2^-24
    relative) of a partial sum that is at most the sum of the magnitudes, and the float32 matrix is within 2^-24 relative of the
    float64 one that `exact` uses.  dB-like data, 20 sigma - 40"""
    from lewton_amd.rows import dct_matrix
    rng = np.random.default_rng(n_in)
    x = (20.0 * rng.standard_normal((n_in, 200)) - 40.0).astype(F32)
    m32 = dct_matrix(n_out, n_in)
    q, f = np.arange(n_out, dtype=F64)[:, None], np.arange(n_in, dtype=F64)[None, :]
    m64 = np.cos(np.pi * q * (2.0 * f + 1.0) / (2.0 * n_in)) * np.where(q == 0, np.sqrt(1.0 / n_in), np.sqrt(2.0 / n_in))
    got = M.static(x, m32).astype(F64)
    exact = m64 @ x.astype(F64)
    bound = (n_in + 1) * 2.0 ** -24 * (np.abs(m64) @ np.abs(x.astype(F64)))
    ratio = float((np.abs(got - exact) / bound).max())
    print("largest error %.3g of its bound" % ratio)
    assert ratio <= 1.0


# ---- Python

def test_python_parameter_errors_need_no_gpu():
    from lewton_amd.rows import Cepstrum, dct_matrix
    for kw in [dict(n_in=0), dict(n_in=257), dict(n_in=7.0), dict(n_in=True), dict(n_in=7, delta_order=3), dict(n_in=7, delta_order=-1),
               dict(n_in=7, delta_order=1, delta_width=0), dict(n_in=7, delta_order=2, delta_width=17), dict(n_in=7, delta_order=1, delta_width=2.5),
               dict(n_in=7, matrix=np.zeros((5, 8))), dict(n_in=7, matrix=np.zeros((257, 7))), dict(n_in=7, matrix=np.zeros(7)),
               dict(n_in=7, matrix=np.zeros((0, 7))), dict(n_in=7, matrix="dct")]:
        with pytest.raises(ValueError):
            Cepstrum(**kw)
    for args in [(0, 40), (13, 0), (257, 40), (13, 257), (13, 40, "slaney"), (13, 40, "ortho", -1), (13, 40, "ortho", float("nan")), (13.5, 40)]:
        with pytest.raises(ValueError):
            dct_matrix(*args)
    for kw in [dict(n_mels=40, n_mfcc=0), dict(n_mels=0), dict(n_mels=40, norm="x"), dict(n_mels=40, delta_order=3)]:
        with pytest.raises(ValueError):
            Cepstrum.mfcc(**kw)
    with pytest.raises(ValueError):
        Cepstrum.deltas(7, order=2, width=0)
