"""The model of the sliding-window normalisation (tests/slide_model.py; include/lewton_amd.h, "sliding-window normalisation of
feature rows") in the CPU suite: the window rule on its pinned examples and its containment property, and the model against a
float64 yardstick that sums every window directly with math.fsum, within the bound the model file derives from the fold's depth
and the cancellations."""
import numpy as np
import pytest

import slide_model as M

F32, F64 = np.float32, np.float64


def test_pinned_windows():
    assert [M.window(t, 10, 4, 2, True) for t in (0, 1, 2, 3, 8, 9)] == [(0, 4), (0, 4), (0, 4), (1, 5), (6, 10), (6, 10)]
    assert [M.window(t, 10, 4, 3, False) for t in (0, 1, 2, 3, 5, 9)] == [(0, 3), (0, 3), (0, 3), (0, 4), (1, 6), (5, 10)]


CONFIGS = [(600, 100, False), (600, 100, True), (4, 2, True), (8, 3, False), (2048, 1, False)]


@pytest.mark.parametrize("W,mn,center", CONFIGS)
def test_every_window_contains_its_frame_and_lies_in_the_halo(W, mn, center):
    """... and s and e never decrease with t, s by at most one a frame: what lets a tile stage [s(first), e(last)) alone"""
    for T in (1, 2, 99, 100, 101, 700):
        prev = None
        for t in range(T):
            s, e = M.window(t, T, W, mn, center)
            assert s <= t < e and max(t - W, 0) <= s and e <= min(t + W, T - 1) + 1, (T, t, s, e)
            assert e - s <= W + 1
            if prev:
                assert 0 <= s - prev[0] <= 1 and e >= prev[1]
            prev = (s, e)


def test_terms_are_the_window_in_blocks():
    """rule 3's list: whole blocks wherever the window covers them, loose elements at most 15 either side, every frame once"""
    T = 300
    for s, e in [(0, 300), (1, 299), (15, 17), (16, 32), (17, 47), (5, 6), (31, 300), (160, 176), (3, 18)]:
        got = M.terms(s, e, T)
        frames = []
        for i in got:
            frames += [i] if i < T else list(range(16 * (i - T), 16 * (i - T) + 16))
        assert frames == list(range(s, e))
        blocks = [i for i in got if i >= T]
        assert len(got) - len(blocks) <= 30 and (not blocks or got.index(blocks[0]) <= 15)
    assert M.depth(600) == 84 and M.depth(2048) == 175


SHAPES = [(1, 4, 2, True), (17, 4, 2, True), (70, 8, 3, False), (101, 600, 100, False), (99, 33, 33, False), (700, 600, 100, True),
          (700, 600, 100, False), (650, 300, 100, True), (2100, 2048, 1, False), (300, 16, 1, True)]


@pytest.mark.parametrize("norm_vars", [False, True])
def test_model_is_within_its_bound_of_the_fsum_yardstick(norm_vars):
    """N(-12, 3) lines at ten shapes: |model - exact| <= bound on every frame; the largest fraction of the bound is printed"""
    worst, worst_ulp = 0.0, 0.0
    for k, (T, W, mn, center) in enumerate(SHAPES):
        x = (np.random.default_rng(100 + k).standard_normal(T) * 3.0 - 12.0).astype(F32)
        got = M.lines(x[None, :], W, mn, center, norm_vars)[0].astype(F64)
        want, _, _ = M.exact(x, W, mn, center, norm_vars)
        err = np.abs(got - want)
        b = M.bound(x, W, mn, center, norm_vars)
        assert (err <= b).all(), (T, W, mn, center, float((err / b).max()))
        worst = max(worst, float((err / b).max()))
        ulp = np.spacing(np.abs(want).astype(F32)).astype(F64)
        worst_ulp = max(worst_ulp, float((err / ulp).max()))
    print("norm_vars=%d: largest error %.3f of the bound, %.3f f32 ulp" % (norm_vars, worst, worst_ulp))


def test_model_blocks_do_not_depend_on_how_the_line_is_processed():
    """the model of a line equals the model of the same line among others (the fold is per line), and rows() places and fills"""
    n = [70, 0, 33]
    x = M.source(n, 2, 3, 80, 7)
    out = M.rows(x, n, [75, 4, 0], np.full(x.shape, M.SENT_F, F32), 8, 3, False, True)
    one = M.lines(x[0, 1, 2:3, :70], 8, 3, False, True)
    M.same_bits(out[0, 1, 2, :70], one[0])
    assert not out[0, :, :, 70:75].any() and (out[0, :, :, 75:].view(np.uint32) == M.SENT).all()
    assert not out[1, :, :, :4].any() and (out[1, :, :, 4:].view(np.uint32) == M.SENT).all()
    assert (out[2, :, :, 33:].view(np.uint32) == M.SENT).all()
