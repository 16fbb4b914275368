"""The model of lw_specaug_rows (tests/specaug_model.py) against the known answers of include/lewton_amd.h ("masking feature rows"):
Random123's Philox4x32-10 vectors, the pinned spans, the bounds every span keeps, which words of the counter and the key an id, a
seed, a group and a kind reach, and the uniformity of widths and starts over 100 000 utterances with fixed inputs (so the outcome
is a number, not a chance).  No GPU, no library."""
import numpy as np
import pytest

import specaug_model as M

LONG = (1 << 32) + (1 << 20) + 5


def _hex(x):
    return " ".join("%08x" % v for v in x)


def test_philox_known_answers():
    assert _hex(M.philox((0, 0, 0, 0), (0, 0))) == "6627e8d5 e169c58d bc57ac4c 9b00dbd8"
    assert _hex(M.philox((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2)) == "408f276d 41c83b0e a20bc7c6 6d5451fd"
    assert _hex(M.philox((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0))) == "d16cfe09 94fdcceb 5001e420 24126ea1"


def test_philox_on_arrays_is_philox_on_integers():
    rng = np.random.default_rng(1)
    w = rng.integers(0, 1 << 32, (6, 200), dtype=np.uint64)
    w[:, 0], w[:, 1] = 0, 0xFFFFFFFF
    got = np.stack(M.philox_np(*w))
    for i in range(200):
        assert tuple(int(v) for v in got[:, i]) == M.philox([int(v) for v in w[:4, i]], [int(v) for v in w[4:, i]])


P50 = dict(seed=2024, min_t=0, max_t=50, min_f=0, max_f=50)
SPAN_ANSWERS = [
    (M.Params(**P50), 0, M.TIME, 0, 3000, (797, 827)),
    (M.Params(**P50), 1, M.TIME, 0, 3000, (1300, 1317)),
    (M.Params(seed=2024, max_f=10), 0, M.FREQ, 0, 80, (40, 40)),                               # an empty mask
    (M.Params(seed=2024, max_t=50, ratio=(1, 5)), 7, M.TIME, 0, 100, (78, 84)),
    (M.Params(seed=2024, min_t=5, max_t=50), 7, M.TIME, 0, 3, (0, 3)),
    (M.Params(**P50), 7, M.TIME, 0, 0, (0, 0)),
    (M.Params(**P50), 0, M.TIME, 0, LONG, (1153752137, 1153752167)),
    (M.Params(seed=2024, num_t=32, max_t=65535), 6099, M.TIME, 18, LONG, (4294953827, 4294968123)),   # straddles frame 2^32
]


@pytest.mark.parametrize("i", range(len(SPAN_ANSWERS)))
def test_span_known_answers(i):
    P, id_, d, k, n, want = SPAN_ANSWERS[i]
    assert M.span(P, id_, 0, d, k, n) == want
    assert i != 7 or want[0] < 1 << 32 < want[1]


def test_bounded_draws():
    for n in (0, 1, 2, 51, 65536, (1 << 32) - 1):
        assert M.below32(0, n) == 0 and M.below32((1 << 32) - 1, n) == max(n - 1, 0)
    for n in (0, 1, 3000, 1 << 32, (1 << 63) + 1, (1 << 64) - 1):
        assert M.below64(0, n) == 0 and M.below64((1 << 64) - 1, n) == max(n - 1, 0)
    assert M.below32(1 << 31, 51) == 25 and M.below64(1 << 63, 3001) == 1500


@pytest.mark.parametrize("mn,mx,ratio", [(0, 50, None), (5, 50, None), (50, 50, None), (0, 65535, None), (3, 40, (1, 5)), (10, 10, (1, 3)), (0, 0, None),
                                         (7, 65535, (65534, 65535)), (2, 9, (0, 1))])
def test_every_span_lies_inside_the_row_and_every_width_inside_its_limits(mn, mx, ratio):
    P = M.Params(seed=77, num_t=3, min_t=mn, max_t=mx, ratio=ratio, num_f=3, min_f=mn, max_f=mx)
    for n in sorted({0, 1, 2, max(mn - 1, 0), mn, mx, mx + 1, 3000, (1 << 32) - 1, 1 << 32, (1 << 32) + 1, 1 << 63}):
        for d in (M.TIME, M.FREQ):
            lo, W = M.widths(P, d, n)
            assert 0 <= lo <= W <= min(mx, n) and (lo == min(mn, W))
            if d == M.TIME and ratio:
                assert W <= n * ratio[0] // ratio[1]
            for id_ in (0, 1, 12345, (1 << 64) - 1):
                for k in range(3):
                    a, b = M.span(P, id_, 2, d, k, n)
                    assert 0 <= a <= b <= n and lo <= b - a <= W, (n, d, id_, k, a, b)


def test_id_and_seed_above_2_to_the_32_reach_the_high_words():
    P = M.Params(seed=2024, max_t=50)
    a = M.span(P, 5, 0, M.TIME, 0, 3000)
    assert M.span(P, 5 + (1 << 32), 0, M.TIME, 0, 3000) != a and M.span(M.Params(seed=2024 + (1 << 32), max_t=50), 5, 0, M.TIME, 0, 3000) != a
    x = M.philox((5, 1, 0, 0), (2024, 1))                                                  # what the high halves are: counter word 1, key word 1
    Q = M.Params(seed=2024 + (1 << 32), max_t=50)
    w = M.below32(x[0], 51)
    assert M.span(Q, 5 + (1 << 32), 0, M.TIME, 0, 3000) == (M.below64(x[1] << 32 | x[2], 3000 - w + 1), M.below64(x[1] << 32 | x[2], 3000 - w + 1) + w)
    # the mask's number and the group share counter word 2, the kind is word 3: all four change the draw
    spans = {M.span(P, 5, g, d, k, 3000) for g in (0, 1) for d in (0, 1) for k in (0, 1)}
    assert len(spans) == 8
    x = M.philox((5, 0, 3 | 2 << 16, 1), (2024, 0))
    w = M.below32(x[0], 51)
    assert M.span(M.Params(seed=2024, max_f=50), 5, 2, M.FREQ, 3, 3000)[1] - M.span(M.Params(seed=2024, max_f=50), 5, 2, M.FREQ, 3, 3000)[0] == w


def test_groups_differ_only_under_per_channel():
    x = M.source([300, 40], 3, 8, 301, 3)
    for per_channel in (False, True):
        P = M.Params(seed=9, num_t=2, max_t=60, num_f=1, max_f=4, per_channel=per_channel, fill_bits=0x7FC12345)
        out, spans = M.rows(P, x, [300, 40], None, [11, 12], np.full(x.shape, M.SENT, np.uint32))
        filled = out == 0x7FC12345
        assert spans.shape == (2, 3 if per_channel else 1, 3, 2) and filled[0].any()
        same = all(np.array_equal(filled[r, 0], filled[r, c]) for r in range(2) for c in range(3))
        assert same != per_channel
        if per_channel:
            assert len({spans[0, g].tobytes() for g in range(3)}) == 3


def test_the_model_masks_what_its_spans_say():
    P = M.Params(seed=2024, num_t=2, max_t=50, num_f=2, max_f=3, fill_bits=0x80000000)
    x = M.source([1000, 0, 3], 2, 5, 1003, 4, special=True)
    out, spans = M.rows(P, x, [1000, 0, 3], [1003, 2, 0], None, np.full(x.shape, M.SENT, np.uint32))
    for r, T, end in ((0, 1000, 1003), (1, 0, 2), (2, 3, 3)):
        want = np.array(x[r], copy=True)
        for k, (a, b) in enumerate(spans[r, 0]):
            if k < 2:
                want[:, :, a:b] = 0x80000000
            else:
                want[:, a:b, :] = 0x80000000
        assert np.array_equal(out[r, :, :, :T], want[:, :, :T]) and (out[r, :, :, T:end] == 0).all() and (out[r, :, :, end:] == M.SENT).all()
        assert spans[r].tolist() == [[list(s) for s in M.plan(P, r, 0, T, 5)]]


def _chi2(values, bins):
    cnt = np.bincount(values, minlength=bins)
    e = len(values) / bins
    return float(((cnt - e) ** 2 / e).sum())


def test_widths_and_starts_are_uniform():
    """seed 2024, ids 0 .. 99 999, T = 3000.  Widths: min 0 / max 50, k = 0, chi-square over the 51 widths below the 99.9 % quantile
    for 50 degrees of freedom (86.7).  Starts: min = max = 10, k = 1, the first 2976 of the 2991 positions in 32 bins of 93, below
    the 99.9 % quantile for 31 degrees of freedom (61.1).  From the rule: 40.6 and 38.3."""
    ids = np.arange(100000, dtype=np.uint64)
    x = M.philox_np(ids, 0, 0, M.TIME, 2024, 0)
    w = ((x[0] * np.uint64(51)) >> np.uint64(32)).astype(np.int64)
    for i in (0, 1, 999, 99999):
        a, b = M.span(M.Params(seed=2024, max_t=50), i, 0, M.TIME, 0, 3000)
        assert b - a == w[i]
    c_w = _chi2(w, 51)
    P = M.Params(seed=2024, min_t=10, max_t=10)
    starts = np.array([M.span(P, i, 0, M.TIME, 1, 3000)[0] for i in range(100000)], np.int64)
    assert starts.min() >= 0 and starts.max() <= 2990
    c_s = _chi2(starts[starts < 2976] // 93, 32)
    print("chi-square: widths %.1f, starts %.1f" % (c_w, c_s))
    assert c_w < 86.7 and c_s < 61.1
    assert abs(c_w - 40.6) < 0.05 and abs(c_s - 38.3) < 0.05


def test_ratio_of():
    assert M.ratio_of(1.0) == (0, 0) and M.ratio_of(0.2) == (1, 5) and M.ratio_of(0.0) == (0, 1) and M.ratio_of(0.05) == (1, 20)
    n, d = M.ratio_of(1.0 / 3.0)
    assert (n, d) == (1, 3)
