"""The model of the energy VAD (tests/vad_model.py) held against itself and against Kaldi's own order of operations, on the CPU:
the pinned f32 products of rule 3 and the header's worked example, the threshold at the lengths where the summation tree changes
shape, the windows at both edges, special values, and the restatement of voice-activity-detection.cc.  What the kernels make of
the rule is in tests/test_host_vad.py (the kernel source on the host) and tests/test_gpu_rows_vad.py (the GPU)."""
import numpy as np
import pytest

import vad_model as M

F32, F64 = np.float32, np.float64


def test_the_pinned_products_and_the_headers_worked_example():
    """(den, num) = (5, 3) and (10, 6) are voiced at 0.6f because the ONE rounded f32 multiply gives 3.0 and 6.0; under an exact
    product neither is.  The counts of differing pairs are the ones the contract quotes"""
    assert F32(5) * F32(0.6) == F32(3.0) and F32(10) * F32(0.6) == F32(6.0)
    assert M.voiced(3, 5, 0.6) and M.voiced(6, 10, 0.6) and not M.voiced(2, 5, 0.6) and not M.voiced(5, 10, 0.6)
    assert 5 * float(F32(0.6)) > 3.0 and 10 * float(F32(0.6)) > 6.0     # the exact products: 3.00000012, 6.00000024

    def differing(p):
        return sum(M.voiced(num, den, p) != (num >= den * float(F32(p))) for den in range(1, 514) for num in range(den + 1))
    assert [differing(p) for p in (0.6, 0.3, 0.12, 0.5, 0.9)] == [63, 33, 0, 0, 0]
    d = np.array([1, 0, 0, 1, 1, 0, 1])
    e = np.where(d, 10.0, 0.0).astype(F32)
    assert [M.window(t, 7, 2) for t in range(7)] == [(0, 3), (0, 4), (0, 5), (1, 6), (2, 7), (3, 7), (4, 7)]
    assert M.decide(e, 7, 5.0, 2, 0.6).tolist() == [0, 0, 1, 0, 1, 1, 1] == M.decide_plain(e, 7, 5.0, 2, 0.6).tolist()
    assert [float(F32(n) * F32(0.6)) for n in (3, 4, 5)] == [float(F32(1.8000001)), float(F32(2.4)), 3.0]


@pytest.mark.parametrize("T", [1, 255, 256, 257, 16384, 16385])
def test_the_threshold_against_the_plain_restatement_of_the_tree(T):
    """one chunk, a short chunk, a whole one, two, 64 (ONE tree over the list) and 65 (two levels)"""
    e = M.source([T], 1, 1, T, 7 + T)[0, 0, 0]
    S, S2 = M.line_sum(e, T), M.tree_sum(e, T)
    assert S.tobytes() == S2.tobytes()
    thr = M.threshold(S, T, 5.5, 0.5)
    assert thr.dtype == F32 and abs(float(thr) - (5.5 + 0.5 * float(e.astype(F64).sum()) / T)) < 1e-5
    mask, thr2 = M.line(e, T, M.SRE)
    assert thr2.tobytes() == thr.tobytes() and np.array_equal(mask, M.decide(e, T, thr, 2, 0.12))
    assert M.threshold(S, T, 5.5, 0.0) == F32(5.5) and M.threshold(np.nan, 0, 5.5, 0.5) == F32(5.5)


@pytest.mark.parametrize("ctx", [0, 1, 2, 256])
@pytest.mark.parametrize("T", [1, 2, 5, 600])
def test_windows_at_both_edges(ctx, T):
    for t in {0, 1, T // 2, T - 2, T - 1} & set(range(T)):
        lo, hi = M.window(t, T, ctx)
        assert 0 <= lo <= t < hi <= T and hi - lo == min(T, t + ctx + 1) - max(0, t - ctx) and hi - lo <= 2 * ctx + 1
        assert (lo == 0 or lo == t - ctx) and (hi == T or hi == t + ctx + 1)
    e = M.source([T], 1, 1, T, 100 * ctx + T)[0, 0, 0]
    for prop in (0.6, 0.12):
        assert np.array_equal(M.decide(e, T, 12.0, ctx, prop), M.decide_plain(e, T, 12.0, ctx, prop))
    if ctx == 0:
        assert np.array_equal(M.decide(e, T, 12.0, 0, 0.6), e > 12.0)


def test_special_values_in_the_line():
    """a NaN frame is unvoiced on its own; a NaN in the line with a mean unvoices the row, without a mean it does not; +inf is
    above every finite threshold and makes the mean's threshold +inf, -inf makes it -inf (everything finite voiced); +-0 compare as 0"""
    e = np.array([10.0, np.nan, 10.0, 0.0, -0.0, 10.0], F32)
    mask, thr = M.line(e, 6, (5.0, 0.0, 0, 0.6))
    assert mask.tolist() == [1, 0, 1, 0, 0, 1] and thr == F32(5.0)
    mask, thr = M.line(e, 6, (5.0, 0.5, 0, 0.6))
    assert not mask.any() and np.isnan(thr)
    mask, thr = M.line(e, 6, (-0.0, 0.0, 0, 0.6))
    assert mask.tolist() == [1, 0, 1, 0, 0, 1]                                                    # 0 > -0 is false
    pinf = np.array([10.0, np.inf, 3.0], F32)
    mask, thr = M.line(pinf, 3, (5.0, 0.5, 0, 0.6))
    assert thr == F32(np.inf) and not mask.any()
    assert M.line(pinf, 3, (5.0, 0.0, 0, 0.6))[0].tolist() == [1, 1, 0]
    ninf = np.array([10.0, -np.inf, 3.0], F32)
    mask, thr = M.line(ninf, 3, (5.0, 0.5, 0, 0.6))
    assert thr == F32(-np.inf) and mask.tolist() == [1, 0, 1]
    both = np.array([np.inf, -np.inf, 3.0], F32)
    assert np.isnan(M.line(both, 3, (5.0, 0.5, 0, 0.6))[1])
    for cfg in ((5.0, 0.5, 2, 0.6), (5.0, 0.0, 1, 0.12)):
        x = M.source([300] * 6, 1, 1, 300, 3, special=True)
        for r in range(6):
            got, thr = M.line(x[r, 0, 0], 300, cfg)
            want, kthr = M.kaldi(x[r, 0, 0], 300, cfg)
            if np.isnan(thr) or thr.tobytes() == kthr.tobytes():
                assert np.array_equal(got, want), (cfg, r)


# ---- against Kaldi's order of operations

@pytest.mark.parametrize("T", [256, 1024, 4096])
def test_kaldi_restatement_is_identical_on_exact_inputs(T):
    """energies that are multiples of 2^-6 in [-8, 24) under (5.5, 0.5, 2, 0.6): the sum is exact in double in Kaldi's sequential order
    and in the tree's, T <= 4096 keeps the threshold inside 24 bits, so thresholds and masks must be IDENTICAL"""
    cfg = (5.5, 0.5, 2, 0.6)
    e = M.exact_line(T, 11 + T)
    assert float(M.line_sum(e, T)) == float(e.astype(F64).sum())
    got, thr = M.line(e, T, cfg)
    want, kthr = M.kaldi(e, T, cfg)
    assert thr.tobytes() == kthr.tobytes() and np.array_equal(got, want)
    assert 0.2 < got.mean() < 0.8


KALDI_SEEDS = list(range(40))                                        # every one qualifies: test below asserts it


@pytest.mark.parametrize("seed", KALDI_SEEDS)
def test_kaldi_restatement_gives_the_same_mask_where_the_thresholds_agree(seed):
    """N(12, 3) lines of random T < 3000: the two sums differ by a few 2^-53 at the most, which the conversion to float32 absorbs for
    every seed listed (asserted, so nothing is excluded at run time); the masks are then identical"""
    rng = np.random.default_rng(1000 + seed)
    T = int(rng.integers(1, 3000))
    e = (rng.standard_normal(T) * 3.0 + 12.0).astype(F32)
    cfg = [(5.5, 0.5, 2, 0.6), M.SRE, M.DEFAULT, (5.0, 0.5, 256, 0.3)][seed % 4]
    got, thr = M.line(e, T, cfg)
    want, kthr = M.kaldi(e, T, cfg)
    assert thr.tobytes() == kthr.tobytes()
    assert np.array_equal(got, want)
