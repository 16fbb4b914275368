"""The row resampler (lw_resampler_*, lw_resample_rows, k_resample) in the CPU suite: tests/san/resample_host.cpp links
lw_resample.cpp against the HIP stand-ins (tests/san/hip_standins.inc) under ASan / UBSan and compiles the kernel source itself,
lw_kernels_resample.hip, for the host, where its stand-in launcher runs it workgroup by workgroup and lane by lane.

The model is the rule of include/lewton_amd.h ("resampling rows") evaluated here in numpy float64 and Python integers.  What the
kernel makes of real device memory is checked on the GPU (tests/test_gpu_rows_resample.py)."""
import math
import os

import numpy as np
import pytest

import host_harness as H
from common import ROOT, SETUPS
from host_harness import CAPACITY, CS, NULL_ARG, UNSUPPORTED

SRC = [os.path.join(ROOT, "tests", "san", "resample_host.cpp"), os.path.join(CS, "lw_resample.cpp")]
PAIRS = [(44100, 16000), (48000, 16000), (44100, 48000), (16000, 44100), (22050, 44100), (48000, 44100)]
KAISER_BETA = 14.769656459379492
FILTERS = {"hann": (6, 0.99, 0, 0.0), "kaiser": (16, 0.99, 1, KAISER_BETA)}          # zeros, rolloff, window, beta
HALF_WIDTHS = {"hann": [17, 19, 7, 7, 7, 7], "kaiser": [45, 49, 17, 17, 17, 18]}


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return H.build(tmp_path_factory, "resample_host", SRC)


def _run(exe, *args, **kw):
    return H.run(exe, *args, timeout=300, **kw)


def _geometry(in_rate, out_rate, zeros, rolloff):
    g = math.gcd(in_rate, out_rate)
    orig, new = in_rate // g, out_rate // g
    s = rolloff * min(1.0, new / orig)
    w = math.ceil(zeros / s)
    return orig, new, s, w, 2 * w + 2


def _i0(x):
    """I0 by its power series, elementwise in float64, until a term no longer changes any sum"""
    q = x * x / 4
    total, term, m = np.ones_like(x), np.ones_like(x), 1
    while True:
        term = term * q / (m * m)
        nxt = total + term
        if np.array_equal(nxt, total):
            return total
        total, m = nxt, m + 1


def _model_taps(in_rate, out_rate, zeros, rolloff, window, beta):
    orig, new, s, w, K = _geometry(in_rate, out_rate, zeros, rolloff)
    k = np.arange(K, dtype=np.float64)[None, :]
    ph = np.arange(new, dtype=np.float64)[:, None]
    u = s * ((k - w) - ph / new)
    pu = np.pi * u
    with np.errstate(invalid="ignore", divide="ignore"):
        sinc = np.where(u == 0, 1.0, np.sin(pu) / pu)
    inside = np.abs(u) < zeros
    if window == 0:
        win = np.cos(pu / (2 * zeros)) ** 2
    else:
        win = _i0(beta * np.sqrt(np.where(inside, 1 - (u / zeros) ** 2, 0.0))) / _i0(np.float64(beta))
    return np.where(inside, s * sinc * win, 0.0)


_TAPS = {}


def _taps(harness, tmp_path_factory, pair, name):
    """(orig, new, W, K, the library's taps [new][K] float32): read once per (pair, filter), never written to"""
    if (pair, name) not in _TAPS:
        zeros, rolloff, window, beta = FILTERS[name]
        path = str(tmp_path_factory.mktemp("taps") / "taps.bin")
        out = _run(harness, "taps", pair[0], pair[1], zeros, rolloff, window, beta, path)
        orig, new, w, K = [int(x) for x in out[0].split()[1:]]
        h = np.fromfile(path, np.float32).reshape(new, K)
        h.setflags(write=False)
        _TAPS[(pair, name)] = (orig, new, w, K, h)
    return _TAPS[(pair, name)]


@pytest.mark.parametrize("name", list(FILTERS))
@pytest.mark.parametrize("pair", PAIRS)
def test_taps_are_the_formula_rounded_once(harness, tmp_path_factory, pair, name):
    zeros, rolloff, window, beta = FILTERS[name]
    orig, new, w, K, h = _taps(harness, tmp_path_factory, pair, name)
    mo, mn, _, mw, mK = _geometry(pair[0], pair[1], zeros, rolloff)
    assert (orig, new, w, K) == (mo, mn, mw, mK) and K == 2 * w + 2
    assert w == HALF_WIDTHS[name][PAIRS.index(pair)]
    want = _model_taps(pair[0], pair[1], zeros, rolloff, window, beta)
    # two double evaluations differ by about 1e-15; after the one rounding to f32 that is at most one f32 ulp
    tol = np.spacing(np.abs(want).astype(np.float32)).astype(np.float64) + 1e-12
    err = np.abs(h.astype(np.float64) - want)
    assert (err <= tol).all(), (float(err.max()), np.argwhere(err > tol)[:4].tolist())
    assert np.count_nonzero(h) > 0.5 * h.size
    # each phase's taps sum to 1
    sums = h.astype(np.float64).sum(1)
    assert np.abs(sums - 1).max() <= (1e-3 if name == "hann" else 1e-7), float(np.abs(sums - 1).max())


def test_out_len_base_and_phase_in_64_bits(harness):
    lens = [0, 1, 2, 440, 441, 442, (1 << 31) - 1, 1 << 31, (1 << 32) + 5, (1 << 40) - 3, (1 << 40) + 12345]
    ns = [0, 1, 159, 160, 161, (1 << 31) - 1, 1 << 31, (1 << 31) + 1, (1 << 32) + 5, (1 << 40) + 77]
    for pair in PAIRS:
        for name in FILTERS:
            zeros, rolloff, window, beta = FILTERS[name]
            orig, new, _, w, K = _geometry(pair[0], pair[1], zeros, rolloff)
            out = _run(harness, "outlen", pair[0], pair[1], zeros, rolloff, window, beta, *lens)
            got = [tuple(int(x) for x in ln.split()[1:]) for ln in out if ln.startswith("L ")]
            assert got == [(n, -(-n * new // orig)) for n in lens]
            # base and n mod new by the kernel's own index arithmetic, on every route it has
            out = _run(harness, "index", pair[0], pair[1], zeros, rolloff, window, beta, *ns)
            rows = [tuple(int(x) for x in ln.split()[1:]) for ln in out if ln.startswith("I ")]
            assert len(rows) == 3 * len(ns) and {r[3] for r in rows} == {0, 1, 2}
            for n, base, i, route in rows:
                assert base == n * orig // new and i == n % new and (i * orig) % new == (n * orig) % new, (n, route)


def _fold64(h, orig, new, w, x, n_out):
    """the rule with the library's taps and a float64 fold"""
    n = np.arange(n_out, dtype=np.int64)
    base, ph = n * orig // new, n * orig % new
    idx = base[:, None] - w + np.arange(h.shape[1])[None, :]
    xs = np.where((idx >= 0) & (idx < len(x)), x[np.clip(idx, 0, len(x) - 1)], 0.0)
    return (h.astype(np.float64)[ph] * xs).sum(1), base


def _tone_error(h, orig, new, w, in_rate, out_rate, f, against_tone):
    n_in = in_rate // 10                                                # 0.1 s
    x = 0.5 * np.sin(2 * np.pi * f * np.arange(n_in) / in_rate)
    n_out = -(-n_in * new // orig)
    y, base = _fold64(h, orig, new, w, x, n_out)
    inner = (base >= 2 * w) & (base < n_in - 2 * w)                      # away from the 2 W edge samples
    assert inner.sum() > 0.8 * n_out
    want = 0.5 * np.sin(2 * np.pi * f * np.arange(n_out) / out_rate) if against_tone else 0.0
    return float(np.abs(y - want)[inner].max())


@pytest.mark.parametrize("name", list(FILTERS))
@pytest.mark.parametrize("pair", PAIRS)
def test_filter_quality(harness, tmp_path_factory, pair, name):
    """the formula itself: a pass-band tone at 0.2 * min(rates) comes through, a tone at 0.65 * out_rate is suppressed when
    down-sampling.  The limits are the issue's (2-3x its numpy model: 1.8e-4 / 5.6e-8 in the pass band, 2.8e-3 / 4.1e-8 in the
    stop band).  The stop-band tone exists as an input only where 0.65 * out_rate is below the INPUT's Nyquist frequency:
    at 48000 -> 44100 it would be 28 665 Hz, which sampled at 48 kHz IS a 19 335 Hz tone, inside the pass band."""
    orig, new, w, K, h = _taps(harness, tmp_path_factory, pair, name)
    err = _tone_error(h, orig, new, w, pair[0], pair[1], 0.2 * min(pair), True)
    print("pass band", pair, name, err)
    assert err <= (5e-4 if name == "hann" else 2e-7)
    if pair[1] < pair[0] and 0.65 * pair[1] < pair[0] / 2:
        err = _tone_error(h, orig, new, w, pair[0], pair[1], 0.65 * pair[1], False)
        print("stop band", pair, name, err)
        assert err <= (8e-3 if name == "hann" else 2e-7)


CREATE_REFUSALS = [(0, 16000, 6, 0.99, 0, 0.0), (44100, 0, 6, 0.99, 0, 0.0), (44100, 16000, 0, 0.99, 0, 0.0),
                   (44100, 16000, 6, 0.0, 0, 0.0), (44100, 16000, 6, 1.5, 0, 0.0), (44100, 16000, 6, -0.5, 0, 0.0),
                   (44100, 16000, 6, float("nan"), 0, 0.0), (44100, 16000, 6, 0.99, 2, 0.0), (44100, 16000, 6, 0.99, -1, 0.0),
                   (44100, 16000, 6, 0.99, 1, float("nan")), (44100, 16000, 6, 0.99, 1, -1.0),
                   (44100, 44101, 6, 0.99, 0, 0.0),                      # 44 101 phases of 16 taps
                   (192000, 7, 6, 0.99, 0, 0.0),                         # 7 phases of 332 k taps
                   (8000, 44100, 1000, 0.99, 0, 0.0)]                    # 441 phases of 2 024 taps


def test_create_refusals_and_the_standard_rates(harness):
    for args in CREATE_REFUSALS:
        assert _run(harness, "create", *args) == ["RC %d" % UNSUPPORTED], args
    for args in [(44100, 16000, 6, 1.0, 0, 0.0), (16000, 16000, 6, 0.99, 1, 0.0), (1, 1, 1, 0.5, 0, 0.0)]:
        assert _run(harness, "create", *args) == ["RC 0"], args
    # the standard rates against the cap of 65 536 taps: with the defaults every pair fits; with kaiser / 16 every pair but
    # 11 025 <-> 192 000 Hz (2 560 phases of 36 taps, 640 of 130), which the library refuses like any other table of that size
    rates = [8000, 11025, 12000, 16000, 22050, 24000, 32000, 44100, 48000, 88200, 96000, 176400, 192000]
    size = {(a, b, zeros): _geometry(a, b, zeros, 0.99)[1] * _geometry(a, b, zeros, 0.99)[4] for a in rates for b in rates for zeros in (6, 16)}
    over = sorted(k for k, v in size.items() if v > 65536)
    assert over == [(11025, 192000, 16), (192000, 11025, 16)]
    assert _run(harness, "create", 11025, 192000, 16, 0.99, 1, KAISER_BETA) == ["RC %d" % UNSUPPORTED]
    a, b, zeros = max((k for k in size if k not in over), key=size.get)
    assert size[(a, b, zeros)] == 46080 and _run(harness, "create", a, b, zeros, 0.99, 1, KAISER_BETA) == ["RC 0"]


ROW_REFUSALS = [("null_rs", NULL_ARG), ("null_len", NULL_ARG), ("null_src", NULL_ARG), ("null_dst", NULL_ARG),
                ("i16", UNSUPPORTED), ("i16_interleaved", UNSUPPORTED), ("bad_fmt", UNSUPPORTED),
                ("ch0", CAPACITY), ("ch256", CAPACITY), ("len_over", CAPACITY), ("out_over", CAPACITY), ("row_over", CAPACITY),
                ("row_over_identity", CAPACITY), ("row_twice", CAPACITY), ("row_twice_empty", CAPACITY)]


@pytest.mark.parametrize("case,code", ROW_REFUSALS)
def test_refusals_launch_nothing(harness, case, code):
    assert _run(harness, "refuse", case) == ["RC %d" % code, "LAUNCHES 0"]


def test_exactly_full_is_accepted(harness):
    assert _run(harness, "refuse", "ok") == ["RC 0", "LAUNCHES 1"]
    assert _run(harness, "refuse", "ok_exact") == ["RC 0", "LAUNCHES 1"]    # len == src_capacity, out_len == dst_capacity


def test_a_row_of_more_tiles_than_a_launch_holds_takes_several(harness):
    """a grid dimension holds fewer than 2^32 lanes, 2^23 - 1 workgroups of 512 (a launch past that is accepted, and workgroups of
    it never run: k_spec left rows unwritten under LW_OK that way, tests/test_host_spec.py).  The tiles of a row of nearly
    2^37 outputs go out in launches of at most 2^23 - 1, each with its tile0, and cover the row exactly once"""
    out = _run(harness, "refuse", "ok_many_tiles")
    assert out[0] == "RC 0"
    launches, tile = int(out[1].split()[1]), int(out[2].split()[1])
    tiles = [tuple(int(v) for v in line.split()[1:]) for line in out[3:]]
    outputs = (1 << 37) // 160 * 160                                      # out_len of (2^37 // 160) * 441 samples at 441 -> 160
    most = (1 << 23) - 1
    want = -(-outputs // tile)
    assert launches == len(tiles) == -(-want // most) > 1 and tile % 160 == 0
    assert tiles == [(t0, min(most, want - t0)) for t0 in range(0, want, most)] and all(n * 512 < 1 << 32 for _, n in tiles)


def test_two_calls_back_to_back_each_reach_their_own_lengths(harness):
    """the second call's records do not replace the first's, which its kernel reads later; the caller's array is free at once"""
    out = _run(harness, "two")
    assert out == ["RC 0", "RC 0", "ROWS 1000/363/2 0/0/0 441/160/3", "ROWS 7/3/0 8/3/1 9/4/2", "LAUNCHES 2"]


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_kernel_on_the_host_is_bit_identical_to_the_scalar_fold(harness, seed):
    """the kernel source lane by lane under ASan against a scalar fold: both formats, 1-6 channels, the six pairs (and the
    all-global route and the copy), both filters, lengths 0..3000, odd capacities, NaN between len and the capacity, a sentinel
    in the destination, permuted destination rows, the global-taps route forced for half the cases"""
    out = _run(harness, "kernel", seed, 64)
    assert out[-1] == "OK 64", out[-3:]
    cases = [ln.split() for ln in out if ln.startswith("CASE ")]
    routes = {int(c[c.index("route") + 1]) for c in cases}
    assert routes - {-1} == {0, 1, 2, 3}                                # (-1: a case whose rows are all empty queues nothing)
    assert {c[2] for c in cases} >= {"%d->%d" % p for p in PAIRS}
    assert {c[4] for c in cases} == {"fmt2", "fmt3"} and {c[5] for c in cases} == {"ch%d" % k for k in range(1, 7)}


def test_python_parameter_validation_needs_no_gpu():
    from lewton_amd import rows as R
    for kw in [dict(in_rate=0), dict(out_rate=0), dict(in_rate=44100.5), dict(zeros=0), dict(rolloff=0), dict(rolloff=1.01),
               dict(window="blackman"), dict(window="kaiser", beta=-1), dict(out_rate=44101), dict(in_rate=True)]:
        args = dict(in_rate=44100, out_rate=16000)
        args.update(kw)
        with pytest.raises(ValueError):
            R.Resampler(**args)
    for pair, (name, ws) in [(p, f) for p in PAIRS for f in HALF_WIDTHS.items()]:
        zeros = FILTERS[name][0]
        g = math.gcd(*pair)
        w = ws[PAIRS.index(pair)]
        assert R.resample_geometry(pair[0], pair[1], zeros) == (pair[0] // g, pair[1] // g, w, 2 * w + 2)
    assert R.KAISER_BETA == KAISER_BETA


def test_i16_at_another_rate_is_refused_before_anything_is_decoded():
    from lewton_amd import header
    from lewton_amd.rows import decode_ogg_files, decode_streams
    from test_ogg import _vorbis_stream
    setup = SETUPS["stereo"]()
    idp, _, stp = setup.headers()
    ident = header.read_header_ident(idp)
    st = header.read_header_setup(stp, ident.audio_channels, (ident.blocksize_0, ident.blocksize_1))
    assert ident.audio_sample_rate == 44100
    for fmt in ("i16", "i16_interleaved"):
        with pytest.raises(ValueError, match="f32"):
            decode_streams(ident, st, [[]], fmt, sample_rate=16000)
    with pytest.raises(ValueError, match="resample="):
        decode_streams(ident, st, [[]], "f32", sample_rate=16000, resample={"taps": 3})
    with pytest.raises(ValueError):
        decode_streams(ident, st, [[]], "f32", sample_rate=16000, resample={"window": "blackman"})
    a = _vorbis_stream("stereo", "LLSL", 9, serial=0x11)[2].bytes()
    with pytest.raises(ValueError, match="source 0.*f32"):
        decode_ogg_files([a], "i16", sample_rate=16000)
    with pytest.raises(ValueError):
        decode_ogg_files([a], "f32", sample_rate=0)
