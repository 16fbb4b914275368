"""The window forms of the models (tests/*_model.py: window(), frame_matrix_window(), resample_model.fold_window()) against the
whole-array models, on short rows that are +0.0 outside three windows (tests/sparse_rows.py), at every window position: the start
of the row, its interior, across the length and the fill into the untouched capacity, and the whole row.  Bits, no tolerance.
tests/rows_long_row_gpu_cases.py relies on these forms for rows of more than 2^32 elements, where no whole array fits."""
import numpy as np
import pytest

import cep_model as CM
import feat_model as FM
import kaldi_model as K
import norm_model as NM
import pack_model as PM
import resample_model as RM
import spec_model as SM
import spec_reflect_model as XM
from sparse_rows import SparseRow

F32 = np.float32
T, CAP = 301, 330
RANGES = [(0, 37), (118, 171), (T - 29, T)]                       # the windows of the source: start, interior, end
SENT_F = FM.SENT_F


def _dense(lines, seed, quantum=None, n=T):
    """[lines][n]: random inside RANGES (clipped to n), +0.0 outside; quantum: integers / quantum"""
    rng = np.random.default_rng(seed)
    x = np.zeros((lines, n), F32)
    for lo, hi in RANGES:
        hi = min(hi, n)
        if hi > lo:
            v = rng.uniform(-1, 1, (lines, hi - lo))
            x[:, lo:hi] = np.rint(v * quantum) / quantum if quantum else v
    return x


def _positions(n, end, cap):
    """[a, b) of the destination: at the start, inside a window, across two windows and the zeros between, across n and the fill
    end into the capacity, one element, nothing, everything"""
    return [(0, 50), (125, 160), (30, 180), (max(0, n - 45), cap), (max(0, n - 1), n), (7, 7), (0, cap), (max(0, min(n, end) - 3), min(cap, end + 3))]


def _ranges(n):
    return [(lo, min(hi, n)) for lo, hi in RANGES if lo < n]


def test_sparse_row_is_the_dense_row():
    x = _dense(3, 1)
    row = SparseRow.of_dense(x, RANGES)
    assert row.covered() == sum(hi - lo for lo, hi in RANGES) and row.lines == 3
    assert np.array_equal(row.take(0, T).view(np.uint32), x.view(np.uint32))
    idx = np.array([[0, 36, 37], [300, 118, 170]], np.int64)
    assert np.array_equal(row.gather(idx), x[:, idx])
    assert np.array_equal(row.clipped(130).take(0, 130), x[:, :130]) and row.clipped(130).covered() == 37 + 12
    with pytest.raises(AssertionError):
        SparseRow.of_dense(np.ones((1, T), F32), RANGES)


@pytest.mark.parametrize("n, end", [(T, T), (T, T + 20), (140, 200), (100, 100), (0, 9)])
@pytest.mark.parametrize("scope, top", [(FM.ROW, 8.0), (FM.CHANNEL, 2.0), (FM.ROW, float("inf"))])
def test_feat_window_is_the_whole_model(scope, top, n, end):
    C, F = 2, 3
    x = np.abs(_dense(C * F, 2)) * F32(1e3)
    x[1, 130] = 7e4                                                 # one line's maximum in the interior window
    row = SparseRow.of_dense(x, RANGES)
    full = np.full((1, C, F, CAP), SENT_F, F32)
    full[0, :, :, :T] = x.reshape(C, F, T)
    before = np.full((1, C, F, CAP), SENT_F, F32)
    want, Ms = FM.rows(full, [n], [end], before, FM.LOG10, scope, 1e-10, top, 4.0, 0.25)
    for a, b in _positions(n, end, CAP):
        got, M = FM.window(row, C, F, a, b, n, end, before[0, :, :, a:b], FM.LOG10, scope, 1e-10, top, 4.0, 0.25)
        FM.same_bits(got, want[0, :, :, a:b], FM.SENT)
        FM.same_bits(M, Ms[0])


@pytest.mark.parametrize("n, end", [(T, T), (T, T + 20), (140, 200), (0, 9)])
@pytest.mark.parametrize("center, scale, scope", [(1, NM.STD, NM.CHANNEL), (1, NM.STD, NM.LINE), (0, NM.PEAK, NM.ROW), (1, NM.RMS, NM.ROW),
                                                  (1, NM.NONE, NM.LINE)])
def test_norm_window_is_the_whole_model(center, scale, scope, n, end):
    """values that are integers / 1024: the whole model's trees and the window form's integer sums give the same S1 and S2"""
    C, F = 2, 2
    x = _dense(C * F, 3, quantum=1024)
    row = SparseRow.of_dense(x, RANGES)
    full = np.full((1, C, F, CAP), SENT_F, F32)
    full[0, :, :, :T] = x.reshape(C, F, T)
    before = np.full((1, C, F, CAP), SENT_F, F32)
    want, stats = NM.rows(full, [n], [end], before, center, scale, scope, 1e-7, 0.5)
    for a, b in _positions(n, end, CAP):
        got, st = NM.window(row, C, F, a, b, n, end, before[0, :, :, a:b], center, scale, scope, 1e-7, 0.5)
        NM.same_bits(got, want[0, :, :, a:b], NM.SENT)
        NM.same_bits(st, stats[0])


def test_norm_exact_sums_refuses_other_values():
    with pytest.raises(AssertionError):
        NM.exact_sums(np.array([0.3], F32))
    assert NM.exact_sums(np.array([0.5, -0.25, 0.0], F32)) == (0.25, 0.3125, F32(0.5))


@pytest.mark.parametrize("n, end", [(T, T), (T, T + 20), (140, 200), (1, 1), (0, 9)])
@pytest.mark.parametrize("n_in, n_out, order, N", [(1, None, 1, 2), (1, 2, 0, 0), (3, 4, 2, 3), (2, None, 2, 16)])
def test_cep_window_is_the_whole_model(n_in, n_out, order, N, n, end):
    x = _dense(n_in, 4) * F32(30.0)
    row = SparseRow.of_dense(x, RANGES)
    m = None if n_out is None else CM.matrix(n_out, n_in, 5) if n_in > 1 else np.full((n_out, 1), 0.75, F32)
    lines = (n_out or n_in) * (1 + order)
    full = np.full((1, 1, n_in, CAP), SENT_F, F32)
    full[0, 0, :, :T] = x
    before = np.full((1, 1, lines, CAP), SENT_F, F32)
    want = CM.rows(full, [n], [end], before, m, order, N)
    for a, b in _positions(n, end, CAP):
        CM.same_bits(CM.window(row, a, b, n, end, before[0, 0, :, a:b], m, order, N), want[0, 0, :, a:b], CM.SENT)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("left, right, stride, edge", [(7, 8, 1, PM.REPLICATE), (2, 1, 3, PM.REPLICATE), (0, 6, 6, PM.VALID), (0, 0, 1, PM.VALID)])
@pytest.mark.parametrize("n", [T, 140, 3, 0])
def test_pack_window_is_the_whole_model(left, right, stride, edge, dtype, n):
    Fl = 5
    x = _dense(Fl, 6) * F32(30.0)
    row = SparseRow.of_dense(x, RANGES)
    D = (left + right + 1) * Fl
    k = PM.out_frames(n, left, right, stride, edge)
    end, ocap = k + 11, k + 17
    full = np.full((1, 1, Fl, CAP), SENT_F, F32)
    full[0, 0, :, :T] = x
    before = np.full((1, 1, ocap, D), PM.sentinel(dtype), PM.OUT_DTYPE[dtype])
    mb = np.full((1, ocap), PM.SENT_MASK, np.uint8)
    shift, scale = PM.vector(D, 1), PM.vector(D, 2, True)
    want, wmask, t_out = PM.rows(full, [n], [end], before, mb, left, right, stride, edge, dtype, shift, scale, -1.0)
    assert t_out == [k]
    for a, b in _positions(k, end, ocap):
        a, b = min(a, ocap), min(b, ocap)
        got, gm = PM.window(row, a, b, n, end, before[0, 0, a:b], mb[0, a:b], left, right, stride, edge, dtype, shift, scale, -1.0)
        PM.same_bits(got, want[0, 0, a:b], dtype, PM.sentinel(dtype))
        assert np.array_equal(gm, wmask[0, a:b])


@pytest.mark.parametrize("n", [T, 140, 30])
@pytest.mark.parametrize("n_fft, win, hop, center", [(32, 32, 1, True), (40, 40, 16, True), (64, 50, 16, True), (16, 16, 4, False), (25, 25, 7, True)])
def test_spec_frame_windows_are_the_whole_frame_matrices(n_fft, win, hop, center, n):
    x = _dense(1, 7, n=n)
    row = SparseRow.of_dense(x, _ranges(n))
    whole = SM.frame_matrix(x[0], n_fft, win, hop, center)
    frames = len(whole)
    for a, b in [(0, min(frames, 9)), (frames // 3, frames // 3 + min(5, frames - frames // 3)), (max(0, frames - 7), frames), (0, frames), (2, 2)]:
        if a <= b <= frames:
            assert np.array_equal(SM.frame_matrix_window(row, a, b, n_fft, win, hop, center).view(np.uint32), whole[a:b].view(np.uint32))
    if center and n >= XM.min_len(n_fft):
        whole = XM.frame_matrix(x[0], n_fft, win, hop)
        frames = len(whole)
        for a, b in [(0, min(frames, 9)), (frames // 3, min(frames, frames // 3 + 5)), (max(0, frames - 7), frames), (0, frames)]:
            assert np.array_equal(XM.frame_matrix_window(row, a, b, n_fft, win, hop).view(np.uint32), whole[a:b].view(np.uint32))


@pytest.mark.parametrize("n", [T, 140, 64])
@pytest.mark.parametrize("W, hop, snip", [(25, 10, True), (25, 10, False), (40, 16, False), (50, 7, True)])
def test_kaldi_frame_windows_are_the_whole_frame_matrix(W, hop, snip, n):
    x = _dense(1, 8, n=n)
    row = SparseRow.of_dense(x, _ranges(n))
    whole = K.frame_matrix(x[0], W, hop, snip)
    frames = len(whole)
    assert frames == K.n_frames(n, W, hop, snip) and frames >= 3
    for a, b in [(0, 3), (frames // 2, frames // 2 + 2), (frames - 3, frames), (0, frames)]:
        assert np.array_equal(K.frame_matrix_window(row, a, b, W, hop, snip).view(np.uint32), whole[a:b].view(np.uint32))


@pytest.mark.parametrize("n", [T, 140, 5])
@pytest.mark.parametrize("orig, new, w", [(3, 1, 19), (1, 3, 7), (441, 160, 18), (160, 147, 8)])
def test_resample_fold_window_is_the_whole_fold(orig, new, w, n):
    x = _dense(1, 9, n=n)
    row = SparseRow.of_dense(x, _ranges(n))
    K_ = 2 * w + 2
    h = np.random.default_rng(10).standard_normal((new, K_)).astype(F32)
    out = RM.out_len(n, orig, new)
    whole = RM.fold(h, orig, new, w, x[0], out)
    assert len(whole) == out
    for a, b in [(0, min(out, 11)), (out // 3, out // 3 + min(9, out - out // 3)), (max(0, out - 13), out), (0, out), (1, 1)]:
        assert np.array_equal(RM.fold_window(h, orig, new, w, row, a, b).view(np.uint32), whole[a:b].view(np.uint32))
    for k in (0, 1, out - 1, (1 << 32) + 5, (1 << 40) + 77):
        assert RM.base_phase(k, orig, new) == (k * orig // new, k * orig - (k * orig // new) * new)


def test_resample_fold_is_the_fold_of_the_gpu_cases_file():
    """resample_model.fold restates rows_resample_gpu_cases._model (which imports torch first, so it is not imported here): pinned
    by one hand-computed output"""
    h = np.array([[0.5, 0.25, -1.0, 2.0]], F32)                       # new = 1, K = 4, w = 1
    x = np.array([1.0, 2.0, 3.0, 4.0, 5.0, 6.0], F32)
    got = RM.fold(h, 3, 1, 1, x, 2)                                  # output 1: base 3, x[2..5] = 3, 4, 5, 6
    assert got.tolist() == [0.25 * 1 - 2 + 6, 1.5 + 1 - 5 + 12]


@pytest.mark.parametrize("n, end", [(T, T), (T, T + 20), (140, 200), (123, 123), (17, 17), (1, 1), (0, 9)])
@pytest.mark.parametrize("cfg", [(8, 3, 0, 0), (8, 3, 0, 1), (60, 20, 1, 1), (33, 33, 0, 0), (16, 1, 1, 1), (600, 100, 1, 0)])
def test_slide_window_rows_is_the_whole_model(cfg, n, end):
    """the term lists at absolute frames: windows that start off the multiples of 16 (125, 30, 7, n - 45), that touch both ends of
    the row, rows whose T is no multiple of 16, and a window of the rule wider than the row"""
    import slide_model as SL
    C, F = 2, 3
    x = _dense(C * F, 11) * F32(4.0) - F32(12.0) * (_dense(C * F, 11) != 0)
    row = SparseRow.of_dense(x, RANGES)
    full = np.full((1, C, F, CAP), SENT_F, F32)
    full[0, :, :, :T] = x.reshape(C, F, T)
    before = np.full((1, C, F, CAP), SENT_F, F32)
    want = SL.rows(full, [n], [end], before, cfg[0], cfg[1], bool(cfg[2]), bool(cfg[3]))
    for a, b in _positions(n, end, CAP) + [(16, 48), (33, 47)]:
        got = SL.window_rows(row, a, b, n, end, before[0, :, :, a:b].reshape(C * F, b - a), cfg[0], cfg[1], bool(cfg[2]), bool(cfg[3]))
        SL.same_bits(got.reshape(C, F, b - a), want[0, :, :, a:b], SL.SENT)


@pytest.mark.parametrize("n, end", [(T, T), (T, T + 20), (140, 200), (1, 1), (0, 9)])
@pytest.mark.parametrize("kind", ["keep_most", "drop_middle", "bytes", "zero", "one"])
def test_select_window_rows_is_the_whole_model(kind, n, end):
    """the places from the mask's stretches: a mask that is 1 outside random windows, one that is 0 between the first and the last
    window, random bytes everywhere, nothing kept, everything kept"""
    import select_model as SE
    from sparse_rows import SparseMask
    Fl = 3
    x = _dense(Fl, 12)
    x.view(np.uint32)[1, 130] = 0x7FC00001                           # NaNs of two payloads and a -0 travel as they are
    x.view(np.uint32)[2, 5] = 0xFFC12345
    x.view(np.uint32)[0, 299] = 0x80000000
    row = SparseRow.of_dense(x, RANGES)
    rng = np.random.default_rng(13)
    m = np.ones(T, np.uint8)
    if kind == "keep_most":
        for lo, hi in RANGES:
            m[lo:hi] = rng.integers(0, 256, hi - lo) * (rng.random(hi - lo) < 0.6)
    elif kind == "drop_middle":
        m[RANGES[0][1]:RANGES[2][0]] = 0
        m[:RANGES[0][1]] = rng.random(RANGES[0][1]) < 0.5
    elif kind == "bytes":
        m[:] = rng.integers(0, 256, T) * (rng.random(T) < 0.7)
    elif kind == "zero":
        m[:] = 0
    sm = SparseMask.of_dense(m, [(0, T)] if kind == "bytes" else RANGES)
    assert sm.count() == int(np.count_nonzero(m)) and sm.clipped(130).count() == int(np.count_nonzero(m[:130]))
    full = np.full((1, 1, Fl, CAP), SENT_F, F32)
    full[0, 0, :, :T] = x
    fm = np.full((1, 1, CAP), SE.SENT_MASK, np.uint8)
    fm[0, 0, :T] = m
    before = np.full((1, 1, Fl, CAP), SENT_F, F32)
    want, k = SE.rows(full, fm, [n], [end], before)
    for a, b in _positions(n, end, CAP) + [(int(k[0, 0]) // 2, min(CAP, int(k[0, 0]) + 5))]:
        got, K = SE.window_rows(row, sm, a, b, n, end, before[0, 0, :, a:b])
        SE.same_bits(got, want[0, 0, :, a:b])
        assert K == int(k[0, 0])


@pytest.mark.parametrize("frames, extra", [(T, 0), (T, 37), (T, -50), (140, 9), (3, 0), (1, 5), (0, 9)])
@pytest.mark.parametrize("n_fft, win, hop, name, center", [(16, 16, 4, "hann", True), (16, 16, 4, "hann", False), (16, 16, 16, "rect", False),
                                                           (32, 20, 5, "hann", True), (25, 25, 7, "hann", True), (64, 64, 32, "hann", True)])
def test_istft_window_rows_is_the_whole_model(n_fft, win, hop, name, center, frames, extra):
    """frames and envelope for a sample range: at the row's start (where the envelope may be 0), in its interior, across the natural
    length into the zeros behind it and across `length` into the untouched capacity; lengths shorter and longer than natural"""
    import istft_model as IM
    B = n_fft // 2 + 1
    X = _dense(2 * B, 14)
    row = SparseRow.of_dense(X, RANGES)
    G, w2 = IM.table_f32(n_fft, win, name), IM.window2(name, win)
    natural = IM.geometry(n_fft, win, hop, center, frames)[4]
    length = max(0, natural + extra)
    cap = length + 11
    whole = np.full(cap, SENT_F, F32)
    whole[:length] = IM.istft(G, w2, X[:, :frames], n_fft, hop, center, length)
    for a, b in [(0, min(cap, 50)), (min(cap, 125 * hop + 3), min(cap, 160 * hop)), (min(cap, 30 * hop + 1), min(cap, 180 * hop + 7)),
                 (max(0, natural - 45), cap), (max(0, length - 1), length), (7, 7), (0, cap), (max(0, length - 3), min(cap, length + 3))]:
        if a <= b:
            got = IM.window_rows(G, w2, row, a, b, frames, n_fft, hop, center, length, np.full(b - a, SENT_F, F32))
            assert np.array_equal(got.view(np.uint32), whole[a:b].view(np.uint32)), (a, b)
