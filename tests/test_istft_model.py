"""The bit model of the inverse spectral frames (tests/istft_model.py) against its float64 yardstick -- numpy.fft.irfft, window,
overlap-add, envelope division: torch.istft's published algorithm -- within the bound the model module derives, and the round
trip through the forward model within the composed bound.  No GPU and no library: this pins the MODEL the other suites compare
the kernel with.  The share of the bound each signal reaches is printed (DESIGN.md 3.23 quotes it), not asserted as a constant."""
import numpy as np
import pytest

import istft_model as IM
import spec_model as M
import spec_reflect_model as R

SHAPES = [(16, 16, 4, "hann", 1), (25, 25, 7, "hann", 1), (32, 20, 5, "hann", 1), (64, 64, 64, "rect", 0), (32, 32, 2, "hann", 1),
          (16, 16, 4, "hann", 0), (512, 400, 160, "hann", 1)]


def signals(n, rate=16000):
    rng = np.random.default_rng(n)
    walk = np.cumsum(rng.normal(0, 1, n))
    walk = (walk - walk.mean()) / (np.abs(walk - walk.mean()).max() + 1e-9)
    return {"white noise": rng.uniform(-1, 1, n), "speech-like random walk": 0.8 * walk,
            "60 Hz tone with DC": 0.3 + 0.5 * np.sin(2 * np.pi * 60.0 * np.arange(n) / rate)}


def stft64(x, n_fft, win_length, hop, name, center):
    """complex128 [B][T]: the exact forward transform the yardstick inverts (reflect padding when centred)"""
    x = np.asarray(x, np.float64)
    if center:
        x = np.pad(x, n_fft // 2, mode="reflect")
    T = 1 + (len(x) - n_fft) // hop
    o = (n_fft - win_length) // 2
    w = np.zeros(n_fft)
    w[o:o + win_length] = IM.window(name, win_length)
    return np.stack([np.fft.rfft(x[t * hop:t * hop + n_fft] * w) for t in range(T)], axis=1)


@pytest.mark.parametrize("shape", SHAPES)
def test_the_model_stays_within_its_bound_of_the_yardstick(shape):
    n_fft, win, hop, name, center = shape
    n = 40 * hop + n_fft
    G, w2 = IM.table_f32(n_fft, win, name), IM.window2(name, win)
    for what, x in signals(n).items():
        Xc = stft64(x, n_fft, win, hop, name, center)
        X = np.concatenate([Xc.real, Xc.imag]).astype(np.float32)
        Xr = X.astype(np.float64)
        B = n_fft // 2 + 1
        got = IM.istft(G, w2, X, n_fft, hop, center).astype(np.float64)
        want = IM.yardstick(Xr[:B] + 1j * Xr[B:], name, n_fft, win, hop, center)
        lim = IM.bound(G, w2, X, n_fft, hop, center)
        ok = np.isfinite(want)
        assert ok.sum() >= len(want) - 2 * n_fft and (np.isfinite(lim) == ok).all() and (got[~ok] == 0).all()
        err = np.abs(got - want)[ok]
        share = float((err / lim[ok]).max())
        print("%s %s: max error %.3g, at most %.3g of the bound" % (shape, what, float(err.max()), share))
        assert (err <= lim[ok]).all(), (what, share)
        # ... and from the unrounded transform the yardstick gives the signal back where the frames cover it: the float64
        # formulas are a round trip (a few ulp of 1 over an envelope that is not small: away from the first and last window)
        back = np.abs(IM.yardstick(Xc, name, n_fft, win, hop, center) - x[:len(want)])[win:-win]
        assert back.max() <= 1e-13, float(back.max())


def test_the_round_trip_of_the_two_bit_models_stays_within_the_composed_bound():
    """x -> the forward chains (float32) -> the inverse model, against x: the forward bound travels through the exact inverse
    (dX of istft_model.bound) and the inverse's own bound is added; no constant"""
    n_fft, win, hop, name = 64, 48, 12, "hann"
    B = n_fft // 2 + 1
    x = signals(40 * hop + n_fft)["white noise"].astype(np.float32)
    w = IM.window(name, win)
    o = (n_fft - win) // 2
    k, j = np.arange(win)[:, None] + o, np.arange(B)[None, :]
    a = 2 * np.pi * ((k * j) % n_fft) / n_fft
    basis = np.stack([w[:, None] * np.cos(a), -w[:, None] * np.sin(a)]).astype(np.float32)
    Xf = R.frame_matrix(x, n_fft, win, hop)
    re, im = np.zeros((len(Xf), B), np.float32), np.zeros((len(Xf), B), np.float32)
    for kk in range(win):
        re, im = M.fmaf(Xf[:, kk:kk + 1], basis[0][kk][None, :], re), M.fmaf(Xf[:, kk:kk + 1], basis[1][kk][None, :], im)
    X = np.concatenate([re.T, im.T])
    G, w2 = IM.table_f32(n_fft, win, name), IM.window2(name, win)
    got = IM.istft(G, w2, X, n_fft, hop, True, len(x)).astype(np.float64)
    lim = IM.bound(G, w2, X, n_fft, hop, True, len(x), dX=IM.stft_bound(basis, Xf))
    err = np.abs(got - x.astype(np.float64))
    assert np.isfinite(lim).all() and (err <= lim).all(), float((err / lim).max())
    print("round trip: max error %.3g, at most %.3g of the composed bound" % (float(err.max()), float((err / lim).max())))
    assert err.max() > 0                                                   # float32 chains do round
