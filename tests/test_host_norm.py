"""Normalising rows (lw_norm_*, lw_norm_rows, k_norm) in the CPU suite: tests/san/norm_host.cpp links lw_norm.cpp against the HIP
stand-ins (tests/san/hip_standins.inc) under ASan / UBSan and compiles the kernel source itself, lw_kernels_norm.hip, for the host,
where its stand-in launchers run it workgroup by workgroup and wave by wave over exact-size buffers.

The model is the rule of include/lewton_amd.h ("normalising rows") in numpy (tests/norm_model.py).  What the kernels make of real
device memory, the shuffles and the device's sqrt included, is checked on the GPU (tests/test_gpu_rows_norm.py)."""
import itertools
import math
import os
from fractions import Fraction

import numpy as np
import pytest

import norm_model as M
import host_harness as H
from common import ROOT
from host_harness import CAPACITY, CS, DEVICE, NULL_ARG, OK, UNSUPPORTED

SRC = [os.path.join(ROOT, "tests", "san", "norm_host.cpp"), os.path.join(CS, "lw_norm.cpp")]
F32, F64 = np.float32, np.float64


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return H.build(tmp_path_factory, "norm_host", SRC)


_run = H.run


# ---- the scalars

@pytest.fixture(scope="module")
def quadruples():
    """(S1, S2, P, N) as the sums of plausible data have them: N up to 2^26 elements of a mean of either sign and a deviation over
    many decades, S2 a few ulps either side of N (sigma^2 + mean^2) so that v = q - mu^2 cancels, and for a share of them a
    deviation of 0, where the difference comes out negative as often as not and is clamped; P = 0, NaN and inf statistics and
    N = 1 strewn in"""
    rng = np.random.default_rng(19)
    K = 1 << 20
    N = np.exp2(rng.uniform(0, 26, K)).astype(np.uint64)
    mean = rng.standard_normal(K) * 10.0 ** rng.uniform(-6, 2, K)
    sigma = 10.0 ** rng.uniform(-6, 1, K)
    sigma[rng.random(K) < 0.25] = 0.0
    Nf = N.astype(F64)
    S1 = mean * Nf
    S2 = (sigma * sigma + mean * mean) * Nf * (1.0 + rng.integers(-4, 5, K) * 2.0 ** -52)
    P = (np.abs(mean) + 4 * sigma).astype(F32)
    P[rng.random(K) < 0.01] = 0.0
    odd = np.array([np.nan, np.inf, -np.inf, 0.0, -0.0], F64)
    for v in (S1, S2):
        pick = rng.random(K) < 0.002
        v[pick] = odd[rng.integers(0, len(odd), int(pick.sum()))]
    pick = rng.random(K) < 0.002
    P[pick] = np.array([np.nan, np.inf], F32)[rng.integers(0, 2, int(pick.sum()))]
    N[rng.random(K) < 0.01] = 1
    with np.errstate(all="ignore"):
        mu, q = S1 / N.astype(F64), S2 / N.astype(F64)
        assert 1000 < int((q - mu * mu < 0).sum()) and 1000 < int((P == 0).sum()) and K >= 1_000_000
    return S1, S2, P, N


@pytest.mark.parametrize("center,scale,eps,target", [(1, M.NONE, 0.0, 1.0), (0, M.NONE, 0.0, 1.0), (1, M.STD, 1e-7, 1.0), (1, M.STD, 0.0, 1.0),
                                                     (0, M.RMS, 1e-20, 0.1), (1, M.RMS, 0.0, 3.0), (0, M.PEAK, 0.0, 1.0), (1, M.PEAK, 0.0, 0.891)])
def test_lw_norm_scalars_is_the_model_bit_for_bit(harness, tmp_path, quadruples, center, scale, eps, target):
    S1, S2, P, N = quadruples
    src, dst = str(tmp_path / "q.bin"), str(tmp_path / "mg.bin")
    with open(src, "wb") as f:
        f.write(np.array([len(N)], np.uint64).tobytes() + S1.tobytes() + S2.tobytes() + N.tobytes() + P.tobytes())
    _run(harness, "scalars", center, scale, repr(eps), repr(target), src, dst)
    got = np.fromfile(dst, F64).reshape(2, -1)
    m, g = M.scalars(center, scale, eps, target, S1, S2, P, N)
    M.same_bits(got[0], m)
    M.same_bits(got[1], g)
    if scale == M.STD and eps == 0.0:
        assert np.isposinf(g).sum() > 1000                                  # v clamped to 0, and nothing under the root but it


# ---- the model's accuracy, by bounds that are derived, not measured

@pytest.fixture(scope="module")
def long_line():
    rng = np.random.default_rng(23)
    return (rng.standard_normal(1_048_577) * 0.1 + 0.05).astype(F32)


def test_the_models_mean_is_within_its_bound_of_the_exact_mean(long_line):
    """1 048 577 samples are 4097 chunks and three list levels.  Every element passes through at most 26 additions (2 in its lane,
    6 in its chunk's tree, 6 per list level, three levels), each with a relative error of at most 2^-53 of a partial sum that is
    at most the sum of the magnitudes, and one division: |mu - exact| <= 27 * 2^-53 * mean|x| to first order.  exact is
    math.fsum's correctly rounded sum over N, in rational arithmetic"""
    x, n = long_line, len(long_line)
    a, b, pk = M.chunk_triples(x[None], n)
    assert a.shape == (1, 4097)
    S1, S2, P = M.fold(a[0], b[0], pk[0])
    mu = S1 / F64(n)
    exact = Fraction(math.fsum(x.astype(F64))) / n
    bound = 27 * Fraction(1, 2 ** 53) * Fraction(math.fsum(np.abs(x).astype(F64))) / n
    err = abs(Fraction(float(mu)) - exact)
    print("error %.3g of the bound" % float(err / bound))
    assert err <= bound
    assert P == np.abs(x).max()


@pytest.mark.parametrize("offset", [0.0, 1.0, -37.5, 510.0])
def test_the_models_wav2vec2_output_is_within_an_ulp_of_the_exactly_centred_formula(offset):
    """z = (x - m) / sqrt(v + 1e-7) with the exact mean and the centred variance (math.fsum over float64), against the model's
    float32 z, for a DC offset of up to 512 deviations: one f32 ulp of rounding, 2^-23 |z|, plus the cancellation in
    v = q - mu^2, whose relative error 2^-50 mu^2 / v moves g by half of that and z by about 2^-50 |m| / sigma <= 2^-41 times a few
    deviations, and the error of m itself, 27 * 2^-53 |m| / sigma: 2^-38 covers both"""
    rng = np.random.default_rng(29)
    n = 100_003
    x = (rng.standard_normal(n) + offset).astype(F32)[None, None, None]
    out, stats = M.rows(x, [n], None, x, 1, M.STD, M.CHANNEL, 1e-7)
    d = x.ravel().astype(F64)
    mean = math.fsum(d) / n
    var = math.fsum((d - mean) ** 2) / n
    want = (d - mean) / math.sqrt(var + 1e-7)
    assert abs(mean) <= 512 * math.sqrt(var)
    err = np.abs(out.ravel().astype(F64) - want)
    bound = 2.0 ** -23 * np.abs(want) + 2.0 ** -38
    print("largest error %.3g of its bound" % float((err / bound).max()))
    assert (err <= bound).all()


# ---- refusals, and what is queued

# (center, scale, scope, reserved, eps, target)
CREATE = [(("null", 1, 0, 0, 1e-7, 1), NULL_ARG), ((1, 4, 0, 0, 1e-7, 1), UNSUPPORTED), ((1, -1, 0, 0, 1e-7, 1), UNSUPPORTED),
          ((1, 1, 3, 0, 1e-7, 1), UNSUPPORTED), ((1, 1, -1, 0, 1e-7, 1), UNSUPPORTED), ((2, 1, 0, 0, 1e-7, 1), UNSUPPORTED),
          ((-1, 1, 0, 0, 1e-7, 1), UNSUPPORTED), ((1, 1, 0, 1, 1e-7, 1), UNSUPPORTED), ((1, 1, 0, 0, "nan", 1), UNSUPPORTED),
          ((1, 1, 0, 0, -1e-30, 1), UNSUPPORTED), ((1, 1, 0, 0, "inf", 1), UNSUPPORTED), ((0, 2, 0, 0, 0, 0), UNSUPPORTED),
          ((0, 2, 0, 0, 0, -1), UNSUPPORTED), ((0, 3, 0, 0, 0, "inf"), UNSUPPORTED), ((0, 3, 0, 0, 0, "nan"), UNSUPPORTED),
          ((1, 1, 0, 0, 1e-7, 1), OK), ((1, 1, 2, 0, 0, "nan"), OK), ((0, 0, 1, 0, 0, -5), OK), ((0, 3, 0, 0, 0, 1e-300), OK),
          ((1, 2, 2, 0, 1e300, 0.1), OK)]


def test_create_refusals(harness):
    for args, code in CREATE:
        assert _run(harness, "create", *args) == ["RC %d" % code], args
    ok = (1, 1, 1, 0, 1e-7, 1)
    for device, code in ((0, OK), (1, DEVICE), (-1, DEVICE), (1 << 20, DEVICE)):              # the stand-ins have one device
        assert _run(harness, "create", *ok, device) == ["RC %d" % code], device
    assert _run(harness, "create", 1, 4, 0, 0, 1e-7, 1, 1) == ["RC %d" % UNSUPPORTED]          # parameters are judged first


ROW_REFUSALS = [("null_nm", NULL_ARG), ("null_n", NULL_ARG), ("null_src", NULL_ARG), ("null_dst", NULL_ARG),
                ("null_dst_fill_only", NULL_ARG), ("n_over", CAPACITY), ("fill_over", CAPACITY), ("ch0", CAPACITY),
                ("ch256", CAPACITY), ("f0", CAPACITY), ("f65536", CAPACITY), ("too_large", CAPACITY), ("too_many_chunks", CAPACITY),
                ("too_many_runs", CAPACITY)]


@pytest.mark.parametrize("case,code", ROW_REFUSALS)
def test_refusals_queue_nothing(harness, case, code):
    assert _run(harness, "refuse", case) == ["RC %d" % code, "LAUNCHES 0", "LAST -1"]


def test_accepted_calls_and_their_launches(harness):
    """sums, fold, apply; no sums where no row has an element, no apply where nothing is written, apply alone without center and
    scale (the fold before it where the stats are owed)"""
    for case, n in (("ok", 3), ("ok_stats", 3), ("ok_nothing", 0), ("ok_no_rows", 0), ("ok_stats_of_nothing", 1), ("ok_fill_only", 2),
                    ("ok_plain", 1), ("ok_plain_stats", 2)):
        assert _run(harness, "refuse", case) == ["RC 0", "LAUNCHES %d" % n, "LAST %d" % n], case


def test_two_calls_back_to_back_each_reach_their_own_records(harness):
    """the second call's records do not replace the first's, which its kernels read later; the caller's arrays are free at once"""
    out = _run(harness, "two")
    assert out == ["RC 0 LAST 3", "RC 0 LAST 3"] + ["ROWS 300/300/2 0/3/0 4/4/1"] * 3 + ["ROWS 1/1/1 257/257/2 3/3/1"] * 3 + ["LAUNCHES 6"]


# ---- the kernel source on the host

def _kernel(harness, tmp_path, x, n, fill_to, center, scale, scope, eps, target, inplace, want_stats, shifts=(0, 0)):
    R, C, F, cap = x.shape
    src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(src, "wb") as f:
        f.write(np.asarray(n, np.uint64).tobytes())
        f.write(np.asarray(fill_to if fill_to is not None else [0] * R, np.uint64).tobytes())
        f.write(np.ascontiguousarray(x, F32).tobytes())
    out = _run(harness, "run", center, scale, scope, repr(eps), repr(target), C, F, R, cap, int(inplace), int(want_stats), int(fill_to is not None),
               shifts[0], shifts[1], src, dst)
    assert out[0] == "RC 0"
    raw = np.fromfile(dst, np.uint8)
    return raw[:x.size * 4].view(F32).reshape(x.shape), raw[x.size * 4:].view(F64), int(out[1].split()[1])


def _check(harness, tmp_path, x, n, fill_to, center, scale, scope, eps=1e-7, target=1.0, inplace=False, want_stats=True, shifts=(0, 0)):
    got, st, launches = _kernel(harness, tmp_path, x, n, fill_to, center, scale, scope, eps, target, inplace, want_stats, shifts)
    before = x if inplace else np.full(x.shape, M.SENT_F, F32)
    want, stats = M.rows(x, n, fill_to, before, center, scale, scope, eps, target)
    M.same_bits(got, want, M.SENT)
    if want_stats:
        M.same_bits(st, stats.ravel())
    else:
        assert (st.view(np.uint64) == 0xEEEEEEEEEEEEEEEE).all()
    plain = not center and scale == M.NONE
    span = max(max(n), max(fill_to) if fill_to is not None else 0)
    assert launches == (0 if plain else int(max(n) > 0) + 1) + int(plain and want_stats) + int(span > 0)
    return want, stats


FILLS = {"none": lambda n, cap: None, "n": lambda n, cap: list(n), "capacity": lambda n, cap: [cap] * len(n),
         "below": lambda n, cap: [max(0, v - 2) for v in n], "mixed": lambda n, cap: [min(cap, (v * 7 + 3) % (cap + 1)) for v in n]}
BASE_N = [0, 1, 3, 4, 5, 255, 256, 257, 1031]


@pytest.mark.parametrize("scale", [M.NONE, M.STD, M.RMS, M.PEAK])
def test_kernel_on_the_host_is_the_model_on_the_base_shape(harness, tmp_path, scale):
    """[9][2][3][1031] with n = 0, 1, 3, 4, 5, 255, 256, 257, 1031 over the rows of one call: the three scopes, centred or not, in
    place and not, every kind of fill_to, the stats asked for or not, source and destination lines at every residue against 16
    bytes (1031 is odd, so the lines take all four in turn; the buffers' own starts are shifted as well): every element of a
    sentinel-filled exact-size destination, the sentinel NaN in the source at and beyond n"""
    combos = list(itertools.product((M.ROW, M.CHANNEL, M.LINE), (1, 0), (False, True)))
    for i, (scope, center, inplace) in enumerate(combos):
        fill = sorted(FILLS)[i % len(FILLS)]
        x = M.source(BASE_N, 2, 3, 1031, 100 + i, offset=0.3 * (i % 3))
        _check(harness, tmp_path, x, BASE_N, FILLS[fill](BASE_N, 1031), center, scale, scope, 1e-7 if i % 2 else 0.0, 0.5, inplace=inplace,
               want_stats=i % 3 != 1, shifts=(i % 4, (i // 4 + i) % 4))


@pytest.mark.parametrize("case", ["63", "64", "65", "three_levels", "row_scope"])
def test_list_level_boundaries_on_the_host(harness, tmp_path, case):
    """one line of 64 chunks - 1, 64 and 64 + 1 (the wave fold's last length and the workgroup fold's first), of 4097 chunks (three
    levels), and a ROW scope of six lines of 22 chunks whose list of 132 crosses lines in the middle of a group"""
    if case == "row_scope":
        x = M.source([5500, 300], 2, 3, 5501, 5, offset=0.1)
        _check(harness, tmp_path, x, [5500, 300], [5501, 0], 1, M.STD, M.ROW, shifts=(1, 2))
        return
    n = {"63": 16383 - 256, "64": 16384, "65": 16385, "three_levels": 1_048_577}[case]
    x = M.source([n], 1, 1, n + 2, 7, offset=-0.2)
    _check(harness, tmp_path, x, [n], [n + 1], 1, M.STD, M.LINE, inplace=case == "65", shifts=(3, 3))


def test_special_values_on_the_host(harness, tmp_path):
    """NaN, +-inf, +-0, subnormals and FLT_MAX in the data: every bit that is not a NaN is the model's; a NaN makes the peak NaN"""
    n = [700] * 9
    x = M.source(n, 1, 2, 701, 31, special=True)
    for scale, center in ((M.NONE, 0), (M.PEAK, 0), (M.STD, 1), (M.RMS, 0)):
        want, stats = _check(harness, tmp_path, x, n, None, center, scale, M.CHANNEL)
        if scale == M.PEAK:
            assert np.isnan(stats[8, 0, 1]) and stats[5, 0, 1] == 1.0 / float(np.finfo(F32).max) and stats[6, 0, 1] == 0.0
        if scale == M.NONE:
            keep = ~np.isnan(x[:, :, :, :700])
            assert np.array_equal(want[:, :, :, :700].view(np.uint32)[keep], x[:, :, :, :700].view(np.uint32)[keep])     # a bit copy


def test_rows_do_not_leak(harness, tmp_path):
    """rows of different lengths and levels and an empty row between them: every scope's stats are its own"""
    n = [300, 0, 1000, 17]
    x = M.source(n, 2, 2, 1000, 41)
    for scope in (M.ROW, M.CHANNEL, M.LINE):
        want, stats = _check(harness, tmp_path, x, n, [1000, 5, 0, 20], 1, M.STD, scope)
        assert (stats[1].reshape(-1, 2) == [0.0, 1.0]).all()
        for r in range(4):                                                   # ... as if the row were alone in its call
            alone = M.rows(x[r:r + 1], n[r:r + 1], None, x[r:r + 1], 1, M.STD, scope)[1]
            M.same_bits(stats[r:r + 1], alone)


def test_python_parameter_errors_need_no_gpu():
    from lewton_amd.rows import Normalize, _normalizer
    for kw in [dict(scale="l2"), dict(scope="batch"), dict(center=2), dict(center="yes"), dict(eps=-1e-9), dict(eps=float("nan")),
               dict(eps=float("inf")), dict(eps="small"), dict(scale="rms", target=0.0), dict(scale="peak", target=float("inf")),
               dict(scale="peak", target=-1.0), dict(scale="rms", target=float("nan"))]:
        with pytest.raises(ValueError):
            Normalize(**kw)
    for fmt in ("i16", "f32_interleaved", "i16_interleaved"):
        with pytest.raises(ValueError):
            _normalizer("wav2vec2", fmt, 0)
    with pytest.raises(ValueError):
        _normalizer("cmvn", "f32", 0)
