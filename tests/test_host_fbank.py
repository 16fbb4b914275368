"""The Kaldi-compatible front end of lw_spec in the CPU suite (lw_spec_create_ex: Kaldi framing, symmetric padding, folded
pre-emphasis / window / scale, DC removal, energy): tests/san/fbank_host.cpp links lw_spec.cpp against the HIP stand-ins under
ASan / UBSan -- a stand-alone program, never loaded into python -- and runs the kernel source itself, lw_kernels_spec.hip (its route
with per-lane fmaf chains, and the prologue's four phases), lane by lane over exact-size buffers.

The models are in tests/kaldi_model.py: the bit model (the contract in numpy, sums as sequential float64 loops), the float64
yardstick (Kaldi's published algorithm restated) and the derived bound between the two.  Route 0 and real device memory are checked
on the GPU (tests/test_gpu_rows_fbank.py)."""
import os

import numpy as np
import pytest

import kaldi_model as K
import spec_model as M
import host_harness as H
from common import ROOT
from host_harness import CAPACITY, CS, UNSUPPORTED

SRC = [os.path.join(ROOT, "tests", "san", "fbank_host.cpp"), os.path.join(CS, "lw_spec.cpp")]
SENT = 0x7FC0DEAD
SENT_F = np.array(SENT, np.uint32).view(np.float32)


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return H.build(tmp_path_factory, "fbank_host", SRC)


_run = H.run


def _p(n_fft, win, hop, window=K.POVEY, center=0, framing=K.SNIP, dc=0, energy=0, reserved=0, c=0.0, scale=1.0):
    return [n_fft, win, hop, window, center, framing, dc, energy, reserved, repr(float(c)), repr(float(scale))]


def _basis(harness, tmp_path, p):
    path = str(tmp_path / "b.bin")
    out = _run(harness, "basis", *p, path)
    return np.fromfile(path, np.float32).reshape(2, p[1], p[0] // 2 + 1), [int(v) for v in out[0].split()[1:]]


# ---- the tables
@pytest.mark.parametrize("shape", [(400, 400, 160, 0, 1), (512, 400, 160, 0, 1), (16, 16, 4, 1, 0), (25, 25, 7, 0, 1), (64, 64, 100, 0, 1),
                                   (32, 32, 1, 0, 1), (2048, 2048, 512, 0, 1), (2, 1, 1, 1, 0)])
def test_create_ex_with_the_defaults_is_create_byte_for_byte(harness, shape):
    """the shapes of tests/test_host_spec.py: the same table bytes, the same frame counts, pad mode zero"""
    assert _run(harness, "legacy", *shape) == ["SAME %d" % (2 * shape[1] * (shape[0] // 2 + 1))]


def _ulps(got, want64):
    """got float32 against float64 values rounded once: the distance in float32 places"""
    w = want64.astype(np.float32)
    return np.abs(got.astype(np.float64) - w.astype(np.float64)) / np.maximum(np.spacing(np.abs(w)).astype(np.float64), 2.0 ** -149)


@pytest.mark.parametrize("window", sorted(K.WINDOWS.values()))
def test_every_table_element_is_the_formula_rounded_once(harness, tmp_path, window):
    """numpy's cos / sin / pow and libm's may differ in the last places of the DOUBLE; two values rounded once from such doubles
    cannot differ by more than one float32 place"""
    for n_fft, win, hop, framing, c, scale in ((512, 400, 160, K.SNIP, 0.97, 1.0), (512, 400, 160, K.EDGES, 0.0, 32768.0), (32, 25, 10, K.SNIP, 0.97, 32768.0),
                                               (512, 400, 160, K.STFT, 0.97, 1.0), (256, 200, 80, K.EDGES, 1.0, 0.5), (2, 2, 1, K.SNIP, 0.5, 1.0)):
        got, (bins, features, pad) = _basis(harness, tmp_path, _p(n_fft, win, hop, window, framing=framing, c=c, scale=scale))
        assert (bins, features, pad) == (n_fft // 2 + 1, n_fft // 2 + 1, 2 if framing == K.EDGES else 0)
        want = K.table(n_fft, win, window, (n_fft - win) // 2 if framing == K.STFT else 0, c, scale)
        d = _ulps(got, want)
        assert d.max() <= 1.0, (float(d.max()), np.argwhere(d > 1)[:4].tolist())
        assert (d == 0).mean() > 0.5                                        # (and nearly all of them are the same bits)


def test_features_counts_the_energy_line(harness, tmp_path):
    assert _basis(harness, tmp_path, _p(512, 400, 160, energy=1))[1] == [257, 258, 0]
    assert _basis(harness, tmp_path, _p(512, 400, 160, framing=K.EDGES, energy=1, dc=1))[1] == [257, 258, 2]


# ---- framing
FRAMINGS = [(32, 25, 10), (512, 400, 160), (8, 7, 7), (16, 16, 1)]


@pytest.mark.parametrize("shape", FRAMINGS)
@pytest.mark.parametrize("framing", [K.SNIP, K.EDGES])
def test_frame_counts_and_first_and_last_index(harness, shape, framing):
    """every len <= 2 W: lw_spec_frames, and the kernel's own index functions at frame 0 and at the last frame"""
    n_fft, W, hop = shape
    snip = framing == K.SNIP
    out = _run(harness, "frames", *_p(n_fft, W, hop, framing=framing), 0, 2 * W)
    want = []
    for n in range(2 * W + 1):
        ft = K.touched(n, W, hop, snip) or (0, 0)
        want.append("L %d %d %d %d" % (n, K.n_frames(n, W, hop, snip), ft[0], ft[1]))
    assert out == want
    if snip:
        assert all(K.accepted(n, W, hop, True) and (K.touched(n, W, hop, True) or (0, 0))[1] < max(n, 1) for n in range(2 * W + 1))


@pytest.mark.parametrize("shape", FRAMINGS)
def test_the_symmetric_refusal_at_its_exact_boundary(harness, shape):
    """LW_SPEC_FRAMES_KALDI_EDGES: every len <= 2 W at which the model's answer (first >= -len and last <= 2 len - 1, from the two
    indices) changes, on either side; a refused row launches nothing although a long row stands in front of it"""
    n_fft, W, hop = shape
    ok = [K.accepted(n, W, hop, False) for n in range(2 * W + 1)]
    edges = [n for n in range(1, 2 * W + 1) if ok[n] != ok[n - 1]]
    assert edges or all(ok)
    if W >= 2 * hop:
        assert edges and not all(ok)                                        # (short rows with a frame are refused there)
    for n in sorted(set([0, 1, 2 * W] + edges + [e - 1 for e in edges])):
        want = ["RC 0", "LAUNCHES 1"] if ok[n] else ["RC %d" % CAPACITY, "LAUNCHES 0"]
        assert _run(harness, "accept", *_p(n_fft, W, hop, framing=K.EDGES, dc=1, energy=1), n) == want, n


def test_snip_never_refuses_and_never_pads(harness):
    for n in (0, 1, 24, 25, 26):
        assert _run(harness, "accept", *_p(32, 25, 10, framing=K.SNIP), n) == ["RC 0", "LAUNCHES 1"]


# ---- refusals
def test_every_create_refusal(harness):
    good = dict(n_fft=512, win=400, hop=160)
    assert _run(harness, "create", *_p(**good)) == ["RC 0"]
    assert _run(harness, "create", *_p(**good, framing=K.EDGES, dc=1, energy=1, c=1.0, scale=32768.0, window=K.BLACKMAN)) == ["RC 0"]
    assert _run(harness, "create", *_p(**good, framing=K.STFT, center=1, dc=1, energy=1, c=0.97)) == ["RC 0"]   # orthogonal to the framing
    bad = [dict(window=6), dict(window=-1), dict(framing=3), dict(framing=-1), dict(framing=K.SNIP, center=1), dict(framing=K.EDGES, center=1),
           dict(c=-0.01), dict(c=1.01), dict(c=float("nan")), dict(scale=0.0), dict(scale=-1.0), dict(scale=float("inf")), dict(scale=float("nan")),
           dict(reserved=1), dict(dc=2), dict(dc=-1), dict(energy=2), dict(hop=0), dict(n_fft=4096), dict(win=513)]
    for kw in bad:
        args = dict(good)
        args.update(kw)
        assert _run(harness, "create", *_p(**args)) == ["RC %d" % UNSUPPORTED], kw
    for window in (K.POVEY, K.HAMMING, K.HANN_SYM, K.BLACKMAN):
        assert _run(harness, "create", *_p(2, 1, 1, window=window)) == ["RC %d" % UNSUPPORTED]      # a / (W - 1)
        assert _run(harness, "create", *_p(2, 2, 1, window=window)) == ["RC 0"]
    assert _run(harness, "create", *_p(2, 1, 1, window=K.RECT)) == ["RC 0"]


def test_set_pad_mode_on_a_kaldi_framed_object_is_unsupported(harness):
    for framing, mode in ((K.SNIP, 0), (K.EDGES, 2)):
        for m in (0, 1, 2):
            assert _run(harness, "padmode", *_p(512, 400, 160, framing=framing), m) == ["RC %d MODE %d" % (UNSUPPORTED, mode)]
    assert _run(harness, "padmode", *_p(512, 400, 160, framing=K.STFT, center=1), 1) == ["RC 0 MODE 1"]
    assert _run(harness, "padmode", *_p(512, 400, 160, framing=K.STFT, center=1), 2) == ["RC %d MODE 0" % UNSUPPORTED]


# ---- the kernel source against the bit model
def _lengths(W, hop, snip):
    tile = [W + (T - 1) * hop if snip else T * hop - hop // 2 for T in (32, 33, 65)]
    assert [K.n_frames(n, W, hop, snip) for n in tile] == [32, 33, 65]
    return [0, W - 1, W, W + hop - 1, W + hop] + tile


def _source(lengths, ch, seed, offset=0.25):
    """host [row][ch][cap] float32, cap = the longest + 3, NaN poison beyond each length"""
    rng = np.random.default_rng(seed)
    x = np.full((len(lengths), ch, max(lengths) + 3), SENT_F, np.float32)
    for r, n in enumerate(lengths):
        x[r, :, :n] = (rng.uniform(-1, 1, (ch, n)) + offset * (r % 3)).astype(np.float32)
    return x


def _kernel(harness, tmp_path, p, fb, x, lengths, itl):
    src, dst, fbp = str(tmp_path / "x.bin"), str(tmp_path / "y.bin"), str(tmp_path / "fb.bin")
    x.tofile(src)
    if fb is not None:
        np.ascontiguousarray(fb, np.float32).tofile(fbp)
    out = _run(harness, "run", *p, 0 if fb is None else len(fb), fbp if fb is not None else "-", x.shape[1], int(itl), src, dst, *lengths)
    assert out[0] == "RC 0", out
    F, fcap = [int(v) for v in out[1].split()[1:]]
    return np.fromfile(dst, np.float32).reshape(len(lengths) + 1, x.shape[1], F, fcap)


def _expected(basis, fb, x, lengths, W, hop, snip, dc, energy, scale, shape):
    want = np.full(shape, SENT_F, np.float32)
    for r, n in enumerate(lengths):
        T = K.n_frames(n, W, hop, snip)
        for c in range(x.shape[1]):
            if T:
                want[r, c, :, :T] = K.features(basis, fb, K.frame_matrix(x[r, c, :n], W, hop, snip), dc, energy, scale).T
    return want


CONFIGS = [(0, 0, 0.97), (1, 1, 0.97), (1, 0, 0.0), (0, 1, 0.0)]


@pytest.mark.parametrize("config", range(len(CONFIGS)))
@pytest.mark.parametrize("framing", [K.SNIP, K.EDGES])
@pytest.mark.parametrize("shape", [(32, 25, 10, 5), (512, 400, 160, 80)])
def test_kernel_on_the_host_is_the_bit_model(harness, tmp_path, shape, framing, config):
    """every element of a sentinel-filled destination with a row more than needed: two channels, planar or interleaved, NaN between
    len and the capacity, the lengths around the window and at the tile seams (32, 33, 65 frames)"""
    from lewton_amd.rows import kaldi_mel_banks
    n_fft, W, hop, n_mels = shape
    dc, energy, c = CONFIGS[config]
    snip = framing == K.SNIP
    scale = 32768.0 if config & 1 else 1.0
    p = _p(n_fft, W, hop, K.POVEY, framing=framing, dc=dc, energy=energy, c=c, scale=scale)
    fb = kaldi_mel_banks(16000, n_fft, n_mels)
    basis, _ = _basis(harness, tmp_path, p)
    lengths = _lengths(W, hop, snip)
    x = _source(lengths, 2, 7 * config + framing)
    got = _kernel(harness, tmp_path, p, fb, x, lengths, itl=(config + framing) & 1)
    assert got.shape[2] == n_mels + energy
    want = _expected(basis, fb, x, lengths, W, hop, snip, dc, energy, scale, got.shape)
    assert (want.view(np.uint32) != SENT).any()
    K.same_bits(got, want, SENT)
    assert ((got.view(np.uint32) == SENT) == (want.view(np.uint32) == SENT)).all()


@pytest.mark.parametrize("framing", [K.STFT, K.EDGES])
def test_the_power_spectrum_behind_the_energy_line_and_a_span_that_does_not_fit_lds(harness, tmp_path, framing):
    """n_mels = 0 with energy: line 0, then the B power lines.  hop = 300 with W = 64: the tile's span of 9364 samples does not fit
    the P region, so the prologue's chains read the row itself -- the same bits"""
    for n_fft, W, hop, lengths in ((32, 25, 10, [0, 24, 25, 26, 330]), (64, 64, 300, [64, 70, 9400])):
        center = int(framing == K.STFT)
        p = _p(n_fft, W, hop, K.HAMMING, center=center, framing=framing, dc=1, energy=1, c=0.5)
        basis, _ = _basis(harness, tmp_path, p)
        x = _source(lengths, 2, 3)
        got = _kernel(harness, tmp_path, p, None, x, lengths, itl=False)
        want = np.full(got.shape, SENT_F, np.float32)
        for r, n in enumerate(lengths):
            for ch in range(2):
                X = M.frame_matrix(x[r, ch, :n], n_fft, W, hop, True) if center else K.frame_matrix(x[r, ch, :n], W, hop, False)
                if len(X):
                    want[r, ch, :, :len(X)] = K.features(basis, None, X, True, True, 1.0).T
        K.same_bits(got, want, SENT)


def test_a_constant_row_with_remove_dc_is_zero_in_every_line(harness, tmp_path):
    """mu is the constant itself (a float64 sum of W equal float32 values, divided by W, is exact for these W), so x' = +0, every
    power +0, and Ed = S2 - S1^2 / W = 0"""
    from lewton_amd.rows import kaldi_mel_banks
    p = _p(512, 400, 160, K.POVEY, framing=K.EDGES, dc=1, energy=1, c=0.97, scale=32768.0)
    x = np.full((1, 1, 2003), np.float32(0.3), np.float32)
    got = _kernel(harness, tmp_path, p, kaldi_mel_banks(16000, 512, 80), x, [2000], itl=False)
    T = K.n_frames(2000, 400, 160, False)
    assert T == 13 and not got[0, 0, :, :T].view(np.uint32).any()


# ---- the mel banks
def test_kaldi_mel_banks_element_by_element():
    from lewton_amd.rows import kaldi_mel_banks
    import math
    for sr, n_fft, n_mels, low, high in ((16000, 512, 80, 20.0, 0.0), (16000, 512, 23, 20.0, -400.0), (8000, 256, 40, 0.0, 3800.0), (16000, 32, 5, 20.0, 0.0)):
        fb = kaldi_mel_banks(sr, n_fft, n_mels, low, high)
        assert fb.dtype == np.float32 and fb.shape == (n_mels, n_fft // 2 + 1)
        mel = lambda f: 1127.0 * math.log(1.0 + f / 700.0)
        hi = high if high > 0 else sr / 2 + high
        lo_m, hi_m = mel(low), mel(hi)
        delta = (hi_m - lo_m) / (n_mels + 1)
        want = np.zeros((n_mels, n_fft // 2 + 1))
        for q in range(n_mels):
            left, centre, right = lo_m + q * delta, lo_m + (q + 1) * delta, lo_m + (q + 2) * delta
            for i in range(n_fft // 2):
                m = mel(i * sr / n_fft)
                if left < m < right:
                    want[q, i] = (m - left) / (centre - left) if m <= centre else (right - m) / (right - centre)
        assert np.abs(fb.astype(np.float64) - want).max() <= 2.0 ** -24         # one rounding of a value in [0, 1]
        assert not fb[:, -1].any() and (fb >= 0).all()
        m_bins = np.array([mel(i * sr / n_fft) for i in range(n_fft // 2)])
        inner = (m_bins >= lo_m + delta) & (m_bins <= lo_m + n_mels * delta)   # between the first and the last centre
        assert inner.any() and np.abs(want[:, :-1][:, inner].sum(axis=0) - 1.0).max() < 1e-12
        assert np.abs(fb[:, :-1][:, inner].astype(np.float64).sum(axis=0) - 1.0).max() <= 2 * 2.0 ** -24
    for bad in (dict(n_fft=511), dict(n_mels=0), dict(n_mels=257), dict(low_freq=-1.0), dict(high_freq=9000.0), dict(low_freq=8000.0), dict(sample_rate=0)):
        args = dict(sample_rate=16000, n_fft=512, n_mels=80)
        args.update(bad)
        with pytest.raises(ValueError):
            kaldi_mel_banks(**args)


# ---- accuracy: the bit model within the derived bound of the float64 yardstick
def _signals():
    rng = np.random.default_rng(11)
    t = np.arange(16000) / 16000.0
    walk = np.cumsum(rng.standard_normal(16000))
    walk = walk - np.linspace(walk[0], walk[-1], 16000)
    return {"white noise": 0.3 * rng.standard_normal(16000),
            "speech-like": 0.4 * walk / np.abs(walk).max() + 0.1 * np.sin(2 * np.pi * 150.0 * t),
            "60 Hz tone + DC": 0.25 + 0.5 * np.sin(2 * np.pi * 60.0 * t)}


@pytest.mark.parametrize("snip", [True, False])
def test_the_bit_model_is_within_the_derived_bound_of_the_float64_yardstick(harness, tmp_path, snip):
    """(512, 400, 160) povey, 80 bands, pre-emphasis 0.97, DC removal, energy: kaldi_model.bound says how the bound is built.
    The observed share of the bound is printed per signal"""
    from lewton_amd.rows import kaldi_mel_banks
    import feat_model as FM
    fb = kaldi_mel_banks(16000, 512, 80)
    for scale in (1.0, 32768.0):
        p = _p(512, 400, 160, K.POVEY, framing=K.SNIP if snip else K.EDGES, dc=1, energy=1, c=0.97, scale=scale)
        basis, _ = _basis(harness, tmp_path, p)
        for name, sig in _signals().items():
            x = sig.astype(np.float32)
            X = K.frame_matrix(x, 400, 160, snip)
            lin = K.features(basis, fb, X, True, True, scale)
            got = FM.log(FM.LN, np.maximum(lin, K.EPS)).astype(np.float64)         # the contract's LOG of lw_feat_rows
            ref, re, im, ref_lin = K.yardstick(x, 512, 400, 160, snip, K.POVEY, fb, 0.97, True, True, scale, parts=True)
            Xp, _ = K.prologue(X, True, scale)
            mu = (X.astype(np.float64).mean(axis=1))
            b = K.bound(basis, fb, Xp, mu, re, im, ref_lin, True, scale)
            err = np.abs(got - ref)
            share = err / b
            print("%s, scale %g: largest difference %.3e (median %.3e), largest share of the bound %.3f" % (name, scale, err.max(), np.median(err), share.max()))
            assert (err <= b).all(), (name, float(share.max()), np.argwhere(err > b)[:4].tolist())
