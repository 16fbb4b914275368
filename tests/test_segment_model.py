"""The two statements of the segment rule (tests/segment_model.py) against each other and against the worked examples that
include/lewton_amd.h quotes ("segments of a frame mask").  No GPU, no library."""
import numpy as np

import segment_model as M


def _line(s):
    return np.array([c == "x" for c in s], np.uint8)


def _text(o):
    return "".join("x" if v else "." for v in o)


def _both(s, *params):
    """O of a line written with x and ., by the pointwise rule; the sequential restatement and the literal one must agree"""
    m = _line(s)
    o = M.pointwise(m, *params)
    assert M.runs(o) == M.sequential(m, *params), (s, params)
    assert np.array_equal(o, M.literal(m, *params)), (s, params)
    return _text(o)


def test_pointwise_and_sequential_agree_on_random_masks():
    """2400 masks of random lengths up to 700 frames, bursts of random sizes, every parameter random in a range of its own, H > T
    included; a tenth of the parameters are drawn up to the limit of 1024"""
    rng = np.random.default_rng(2026)
    longer, changed = 0, 0
    for i in range(2400):
        T = int(rng.integers(0, 701))
        hi = 1025 if i % 10 == 0 else int(rng.choice([2, 6, 20, 80]))
        params = tuple(int(v) for v in rng.integers(0, hi, 4))
        m = M.source([T], 1, T, 1000 + i, burst=int(rng.choice([2, 5, 12, 40])))[0, 0]
        if i % 7 == 0:
            m[:] = m * (rng.random(T) < 0.5)                                    # salt-and-pepper
        o = M.pointwise(m, *params)
        assert M.runs(o) == M.sequential(m, *params), (i, T, params)
        longer += max(params[0], params[1]) + params[2] + params[3] > T
        changed += not np.array_equal(o, m != 0)
    assert longer > 200 and changed > 1500


def test_literal_rule_on_short_random_masks():
    """the rule word for word, with loops, on 400 lines of at most 40 frames"""
    rng = np.random.default_rng(7)
    for i in range(400):
        T = int(rng.integers(0, 41))
        params = tuple(int(v) for v in rng.integers(0, 7, 4))
        m = (rng.random(T) < rng.choice([0.2, 0.5, 0.8])).astype(np.uint8) * 255
        assert np.array_equal(M.pointwise(m, *params), M.literal(m, *params)), (i, m.tolist(), params)


def test_worked_examples_of_the_header():
    # a gap of min_off - 1 frames is filled, one of min_off frames stays
    assert _both("x..x", 0, 0, 3, 0) == "xxxx"
    assert _both("x...x", 0, 0, 3, 0) == "x...x"
    # a run of min_on - 1 frames goes, one of min_on frames stays; the line's ends are not exempt
    assert _both(".xx.", 0, 0, 0, 3) == "...."
    assert _both(".xxx.", 0, 0, 0, 3) == ".xxx."
    assert _both("xx..xxx", 0, 0, 0, 3) == "....xxx"
    # pads clamped at 0 and at T
    assert _both(".....x", 2, 1, 0, 0) == "...xxx"
    assert _both("x.....", 2, 1, 0, 0) == "xx...."
    # pads that merge neighbours
    assert _both(".x..x.", 1, 1, 0, 0) == "xxxxxx"
    assert M.sequential(_line(".x..x."), 1, 1, 0, 0) == [(0, 6)]
    # a short gap at a line's end stays open, at either end
    assert _both("x..", 0, 0, 3, 0) == "x.."
    assert _both("..x", 0, 0, 3, 0) == "..x"
    # a hangover is pad_offset alone
    assert _both(".x....x..", 0, 2, 0, 0) == ".xxx..xxx"
    # the order: pad, then fill, then drop -- the pad makes the gap short enough, the fill makes the run long enough
    assert _both("x....x", 0, 1, 4, 6) == "xxxxxx"
    assert _both("x....x", 0, 0, 4, 6) == "......"


def test_trivial_lines():
    for params in ((0, 0, 0, 0), (3, 7, 5, 4), (1024, 1024, 1024, 1024)):
        assert M.sequential(np.zeros(0, np.uint8), *params) == [] and len(M.pointwise(np.zeros(0, np.uint8), *params)) == 0
        assert M.sequential(np.zeros(50, np.uint8), *params) == []
    assert _both("x", 0, 0, 0, 0) == "x" and _both("x", 0, 0, 0, 1) == "x" and _both("x", 5, 5, 5, 2) == "."
    assert _both(".", 3, 3, 3, 0) == "."
    for T in (1, 2, 7, 64, 65):
        assert M.sequential(np.ones(T, np.uint8), 0, 0, 0, 0) == [(0, T)]
        assert M.sequential(np.ones(T, np.uint8), 9, 9, 9, T) == [(0, T)] and M.sequential(np.ones(T, np.uint8), 0, 0, 0, T + 1) == []
        alt = np.arange(T) % 2 == 0                                               # 1010...: K = ceil(T / 2)
        assert len(M.sequential(alt, 0, 0, 0, 0)) == -(-T // 2) == len(M.runs(M.pointwise(alt, 0, 0, 0, 0)))
        assert len(M.sequential(alt, 0, 0, 2, 0)) == 1


def test_bytes_2_and_255_count_as_set_and_rows_writes_what_the_header_says():
    mask = np.full((2, 1, 12), M.SENT_MASK, np.uint8)
    mask[0, 0, :10] = [0, 2, 0, 0, 255, 1, 0, 0, 0, 7]
    spans = np.full((2, 1, 2, 2), M.SENT_SPAN, np.uint64)
    counts = np.full((2, 1), M.SENT_SPAN, np.uint64)
    smooth = np.full((2, 1, 12), M.SENT_MASK, np.uint8)
    s, k, o = M.rows(mask, [10, 0], [11, 3], (0, 0, 0, 0), spans, counts, smooth)
    assert k.tolist() == [[3], [0]] and s[0, 0].tolist() == [[1, 2], [4, 6]] and (s[1] == M.SENT_SPAN).all()      # K > seg_capacity: the true count
    assert o[0, 0].tolist() == [0, 1, 0, 0, 1, 1, 0, 0, 0, 1, 0, M.SENT_MASK] and o[1, 0].tolist() == [0] * 3 + [M.SENT_MASK] * 9
