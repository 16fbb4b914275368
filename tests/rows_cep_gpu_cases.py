"""Cepstra and deltas of feature rows on the GPU: Cepstrum.run (lw_cep_rows / k_cep).  The cases of tests/test_gpu_rows_cep.py,
which runs this file with pytest in a process of its own, torch imported first (tests/rows_gpu_cases.py says why).

The rule of include/lewton_amd.h ("cepstra and deltas of feature rows") is a contract on BITS.  The model is tests/cep_model.py
(numpy, the exact one-rounding fmaf of tests/spec_model.py, the clamp in Python integers).  Every comparison with it is over EVERY
element of a sentinel-filled exact-size destination, with no tolerance; the source holds a NaN at and beyond each length."""
import torch  # noqa: F401  (first: see above)

import itertools

import numpy as np
import pytest

import cep_model as M
import feat_model as FM
import rows_feat_gpu_cases as FC
import rows_spec_gpu_cases as S

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to("cuda:0")


def _check(cp, x, n, fill_to, matrix):
    """one call against the model: the whole destination; the source is only read"""
    R, C, _, cap = x.shape
    src = _dev(x)
    dst = S._filled((R, C, cp.features, cap))
    out = cp.run(src, n, out=dst, fill_to=fill_to)
    torch.cuda.synchronize()
    assert out is dst
    want = M.rows(x, n, fill_to, np.full(tuple(dst.shape), M.SENT_F, F32), matrix, cp.delta_order, cp.delta_width)
    M.same_bits(dst.cpu().numpy(), want, M.SENT)
    assert np.array_equal(src.cpu().numpy().view(np.uint32).ravel(), x.view(np.uint32).ravel())
    assert cp.last_launches() == int(max(max(n), max(fill_to) if fill_to is not None else 0) > 0)
    return want


BASE_N = [0, 1, 2, 3, 4, 5, 8, 9, 255, 256, 257, 1031]
FILLS = {"none": lambda n, cap: None, "n": lambda n, cap: list(n), "capacity": lambda n, cap: [cap] * len(n),
         "below": lambda n, cap: [max(0, v - 2) for v in n], "mixed": lambda n, cap: [min(cap, (v * 7 + 3) % (cap + 1)) for v in n]}


@pytest.mark.parametrize("order", [0, 1, 2])
def test_k_cep_is_the_model_on_the_base_shape(order):
    """[12][2][7][1031] -> 5 cepstra (or the 7 lines themselves), n_frames = 0, 1, 2, 3, 4, 5, 8, 9, 255, 256, 257, 1031 over the rows
    of one call (rows shorter than N, 2N and 4N, and rows of several tiles), N = 1 and 2, a matrix and the identity, every kind of
    fill_to; 1031 is odd, so the lines take every residue against 16 bytes"""
    from lewton_amd.rows import Cepstrum
    for i, (N, identity) in enumerate(itertools.product((1, 2) if order else (2,), (False, True))):
        m = None if identity else M.matrix(5, 7, 7 + i)
        cp = Cepstrum(7, m, order, N)
        try:
            assert cp.features == (7 if identity else 5) * (1 + order) and cp.tile_frames == 256 - 2 * order * N
            assert (cp.matrix() is None) if identity else np.array_equal(cp.matrix().view(np.uint32), m.view(np.uint32))
            assert np.array_equal(cp.delta_weights().view(np.uint32), M.delta_weights(N if order else 0).view(np.uint32))
            for k, fill in enumerate(sorted(FILLS)):
                x = M.source(BASE_N, 2, 7, 1031, 100 + 10 * i + k)
                _check(cp, x, BASE_N, FILLS[fill](BASE_N, 1031), m)
        finally:
            cp.close()


def test_the_widest_window():
    """N = 16 with n_frames 1, 16, 17, 32, 33, 64, 65, 300: rows inside one window, inside two, and of two tiles of 192"""
    from lewton_amd.rows import Cepstrum
    n = [1, 16, 17, 32, 33, 64, 65, 300]
    x = M.source(n, 2, 7, 301, 3)
    for order, identity in ((2, False), (1, True), (2, True)):
        m = None if identity else M.matrix(5, 7, 1)
        cp = Cepstrum(7, m, order, 16)
        try:
            assert cp.tile_frames == 256 - 32 * order
            _check(cp, x, n, [301, 0, 20, 0, 301, 0, 70, 300], m)
        finally:
            cp.close()


# the kernel's accumulator groups are 8, 16, 24 and 32 wide, by what is left of n_out: each size, and one either side of it
N_OUTS = [1, 7, 8, 9, 15, 16, 17, 23, 24, 25, 31, 32, 33, 41, 57, 256]


@pytest.mark.parametrize("n_in", [1, 80, 256])
def test_output_groups(n_in):
    """n_out across every accumulator-group boundary, with n_in = 1, 80 and 256 (the eight-line steps of the fold and its tail);
    delta-deltas of width 2; a row of two tiles and a short one"""
    from lewton_amd.rows import Cepstrum
    n = [300, 5]
    x = M.source(n, 1, n_in, 301, 50 + n_in)
    for n_out in N_OUTS:
        m = M.matrix(n_out, n_in, n_out)
        cp = Cepstrum(n_in, m, 2, 2)
        try:
            _check(cp, x, n, [0, 9], m)
        finally:
            cp.close()
    if n_in > 1:                                                       # the identity's groups: n_in lines copied, 32 at a time
        cp = Cepstrum.deltas(n_in, 2, 2)
        try:
            _check(cp, x, n, None, None)
        finally:
            cp.close()


@pytest.mark.parametrize("N", [16, 1])
def test_tile_seams(N):
    """one row of 3 tiles + 1 frames and one of a tile - 1, order 2: every frame against the model, those within 2N of a seam and
    of either end among them -- where a halo computed at the wrong index shows"""
    from lewton_amd.rows import Cepstrum
    for identity in (False, True):
        m = None if identity else M.matrix(5, 7, 11)
        cp = Cepstrum(7, m, 2, N)
        try:
            T = cp.tile_frames
            assert T == 256 - 4 * N
            n = [3 * T + 1, T - 1]
            x = M.source(n, 2, 7, 3 * T + 2, 60 + N)
            want = _check(cp, x, n, [3 * T + 2, T], m)
            assert not want[0, :, :, 3 * T + 1].any() and not want[1, :, :, T - 1].any()
        finally:
            cp.close()


def test_special_values():
    """NaN, +-inf, +-0, subnormals and FLT_MAX in the data, one kind more per row: every bit that is not a NaN is the model's, the
    sign of a zero and subnormal results included; the identity's static lines are a bit copy, NaN payloads too"""
    from lewton_amd.rows import Cepstrum
    n = [300] * 9
    x = M.source(n, 1, 7, 301, 31, special=True)
    m = M.matrix(5, 7, 9)
    for matrix in (m, None):
        cp = Cepstrum(7, matrix, 2, 2)
        try:
            _check(cp, x, n, None, matrix)
            if matrix is None:
                got = cp.run(_dev(x), n).cpu().numpy()
                assert np.array_equal(got[:, :, :7, :300].view(np.uint32), x[:, :, :, :300].view(np.uint32))
        finally:
            cp.close()


def test_rows_and_channels_do_not_leak():
    """rows of 300, 0, 1000 and 17 frames in one call give the bits each gives alone in a call; the empty row's destination is
    untouched apart from its fill"""
    from lewton_amd.rows import Cepstrum
    n = [300, 0, 1000, 17]
    x = M.source(n, 2, 7, 1000, 41)
    m = M.matrix(5, 7, 4)
    cp = Cepstrum(7, m, 2, 2)
    try:
        want = _check(cp, x, n, [1000, 5, 0, 20], m)
        assert (want[1, :, :, :5].view(np.uint32) == 0).all() and (want[1, :, :, 5:].view(np.uint32) == M.SENT).all()
        for r in range(4):
            alone = S._filled((1, 2, 15, 1000))
            cp.run(_dev(x[r:r + 1]), n[r:r + 1], out=alone)
            torch.cuda.synchronize()
            M.same_bits(alone.cpu().numpy()[..., :n[r]], want[r:r + 1, :, :, :n[r]])
        with pytest.raises(ValueError):
            cp.run(_dev(x), [300, 0, 1001, 17])
        with pytest.raises(ValueError):
            cp.run(_dev(x), n, fill_to=1001)
        with pytest.raises(ValueError):
            cp.run(_dev(x), n[:3])
        with pytest.raises(ValueError):
            cp.run(_dev(x), n, out=S._filled((4, 2, 15, 999)))
        with pytest.raises(ValueError):
            cp.run(_dev(x[:, :, :6]), n)
    finally:
        cp.close()


def test_calls_queued_back_to_back_on_one_stream():
    """five calls of one object (more than it has record slots), different lengths each, on a side stream, nothing synchronised
    until the end"""
    from lewton_amd.rows import Cepstrum
    m = M.matrix(5, 7, 21)
    cp = Cepstrum(7, m, 2, 2)
    try:
        assert cp.last_launches() == -1
        x = M.source([700] * 3, 2, 7, 701, 21)
        src = _dev(x)
        calls = []
        st = torch.cuda.Stream(device=0)
        torch.cuda.synchronize()
        with torch.cuda.stream(st):
            for k in range(5):
                n = [700 - 130 * k, 3 * k, 257 + k]
                dst = S._filled((3, 2, 15, 701))
                cp.run(src, n, out=dst, fill_to=[k, 701, 0])
                calls.append((n, [k, 701, 0], dst))
        st.synchronize()
        for n, fill, dst in calls:
            want = M.rows(x, n, fill, np.full((3, 2, 15, 701), M.SENT_F, F32), m, 2, 2)
            M.same_bits(dst.cpu().numpy(), want, M.SENT)
    finally:
        cp.close()


# ---- the chain

def test_rows_to_mfcc_with_deltas_is_the_three_models_composed():
    """[3][1][4000] with lengths 4000, 1601 and 0 through Spectrogram(400, 160, 40 mel bands), LogCompress(log="db", top=80) and
    Cepstrum.mfcc(40, 13, delta_order=2): bit for bit the three models composed, the empty row included"""
    from lewton_amd.rows import Cepstrum, LogCompress, Spectrogram, mel_filterbank
    mel = mel_filterbank(16000, 400, 40)
    sp, lc, cp = Spectrogram(400, 160, mel=mel), LogCompress(log="db", top=80), Cepstrum.mfcc(40, 13, delta_order=2)
    try:
        lengths = [4000, 1601, 0]
        x = S._source(lengths, 1, 4000, 77)
        fcap = 29
        feats = S._filled((3, 1, 40, fcap))
        out, frames = sp.run(S._device(x, False), lengths, out=feats)
        assert frames.tolist() == [26, 11, 0]
        lc.run(out, frames)
        dst = S._filled((3, 1, 39, fcap))
        res = cp.run(out, frames, out=dst, fill_to=[fcap, 20, fcap])
        torch.cuda.synchronize()
        assert res is dst and cp.features == 39
        lin = S._expected(sp, mel, x, lengths, [0, 1, 2], 3, fcap)
        logs, _ = FM.rows(lin, frames.tolist(), None, lin, FM.DB, FM.ROW, 1e-10, 80.0, 4.0, 0.25)
        FM.same_bits(feats.cpu().numpy(), logs, FM.SENT)
        want = M.rows(logs, frames.tolist(), [fcap, 20, fcap], np.full((3, 1, 39, fcap), M.SENT_F, F32), cp.matrix(), 2, 2)
        M.same_bits(dst.cpu().numpy(), want, M.SENT)
        assert not want[2].any() and (want[1, 0, :, 20:].view(np.uint32) == M.SENT).all()
    finally:
        sp.close()
        lc.close()
        cp.close()


# ---- against torch

def _torch_delta(s, w):
    """float64 [lines][T] -> the regression filter by conv1d over replicate-padded lines"""
    N = len(w)
    k = torch.zeros(2 * N + 1, dtype=torch.float64)
    for n in range(1, N + 1):
        k[N + n], k[N - n] = float(w[n - 1]), -float(w[n - 1])
    p = torch.nn.functional.pad(s[:, None, :], (N, N), mode="replicate")
    return torch.nn.functional.conv1d(p, k[None, None, :])[:, 0, :]


def _delta_bound(s, w):
    """(N + 2) * 2^-24 * sum_n w_n (|s[c(t + n)]| + |s[c(t - n)]|): each of the N steps rounds its difference and its partial sum,
    both at most the sum of the magnitudes so far, and w_n is within 2^-24 relative of n / D"""
    N, T = len(w), s.shape[1]
    a = np.abs(s)
    tot = np.zeros(s.shape, F64)
    for n in range(1, N + 1):
        tot += float(w[n - 1]) * (a[:, np.minimum(np.arange(T) + n, T - 1)] + a[:, np.maximum(np.arange(T) - n, 0)])
    return (N + 2) * 2.0 ** -24 * tot


@pytest.mark.parametrize("N", [2, 9])
def test_against_torchs_matmul_and_conv1d_in_float64(N):
    """80 dB-like lines -> 13 cepstra with deltas and delta-deltas: the static lines within (n_in + 1) * 2^-24 * sum |x| |M| of
    torch.matmul with the float64 DCT; each delta level within its bound of torch's conv1d, in float64 over replicate-padded lines,
    of the KERNEL'S OWN previous level -- the filter itself, not an accumulated error"""
    from lewton_amd.rows import Cepstrum
    n_in, n_out, n = 80, 13, [500, 300]
    rng = np.random.default_rng(5)
    x = (20.0 * rng.standard_normal((2, 1, n_in, 500)) - 40.0).astype(F32)
    cp = Cepstrum.mfcc(n_in, n_out, delta_order=2, delta_width=N)
    try:
        got = cp.run(_dev(x), n).cpu().numpy().astype(F64)
        w = cp.delta_weights()
    finally:
        cp.close()
    q, f = np.arange(n_out, dtype=F64)[:, None], np.arange(n_in, dtype=F64)[None, :]
    m64 = np.cos(np.pi * q * (2.0 * f + 1.0) / (2.0 * n_in)) * np.where(q == 0, np.sqrt(1.0 / n_in), np.sqrt(2.0 / n_in))
    for r, T in enumerate(n):
        xr = x[r, 0, :, :T].astype(F64)
        exact = torch.matmul(torch.from_numpy(m64), torch.from_numpy(xr)).numpy()
        bound = (n_in + 1) * 2.0 ** -24 * (np.abs(m64) @ np.abs(xr))
        ratio = np.abs(got[r, 0, :n_out, :T] - exact) / bound
        print("row %d static: largest error %.3g of its bound" % (r, ratio.max()))
        assert (ratio <= 1.0).all()
        for level in (1, 2):
            prev = got[r, 0, (level - 1) * n_out:level * n_out, :T]
            want = _torch_delta(torch.from_numpy(prev), w).numpy()
            ratio = np.abs(got[r, 0, level * n_out:(level + 1) * n_out, :T] - want) / _delta_bound(prev, w)
            print("row %d level %d: largest error %.3g of its bound" % (r, level, ratio.max()))
            assert (ratio <= 1.0).all()
        assert not got[r, 0, :, T:].any()                                # out=None is a zeroed tensor
