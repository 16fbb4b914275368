"""The model of lw_cep_rows (include/lewton_amd.h, "cepstra and deltas of feature rows") for the CPU and the GPU suite, independent
of the kernel source: the static chains with spec_model.fmaf (the exact one-rounding fma), f ascending from +0.0, over all frames
at once; the delta weights as one float64 division rounded once; the deltas as n ascending from +0.0 over gathers at indices
clamped in Python integers, the subtraction a float32 operation of its own; the delta-deltas as the same of the delta lines."""
import numpy as np

from spec_model import fmaf

F32, F64 = np.float32, np.float64

SENT = 0x7FC0DEAD                     # a NaN: the destination's sentinel, and what the source holds at and beyond n
SENT_F = np.array(SENT, np.uint32).view(F32)


def delta_weights(N):
    """w_1 .. w_N as float32: (float)(n / D), D = 2 (1 + 4 + .. + N^2) an integer"""
    D = 2 * sum(n * n for n in range(1, N + 1))
    return np.array([F32(F64(n) / F64(D)) for n in range(1, N + 1)], F32)


def static(x, matrix):
    """x float32 [n_in][T], matrix float32 [n_out][n_in] or None (the identity: a bit copy) -> float32 [n_out][T]"""
    x = np.asarray(x, F32)
    if matrix is None:
        return x.copy()
    matrix = np.asarray(matrix, F32)
    acc = np.zeros((matrix.shape[0], x.shape[1]), F32)
    for f in range(x.shape[0]):
        acc = fmaf(x[f][None, :], matrix[:, f][:, None], acc)
    return acc


def delta(s, N):
    """s float32 [lines][T] (T >= 1) -> the regression delta of every line, the index clamped into [0, T - 1]"""
    s = np.asarray(s, F32)
    T = s.shape[1]
    w = delta_weights(N)
    acc = np.zeros(s.shape, F32)
    for n in range(1, N + 1):
        after = [min(max(t + n, 0), T - 1) for t in range(T)]
        before = [min(max(t - n, 0), T - 1) for t in range(T)]
        with np.errstate(over="ignore", invalid="ignore"):
            d = s[:, after] - s[:, before]
        assert d.dtype == F32
        acc = fmaf(w[n - 1], d, acc)
    return acc


def lines(x, matrix, order, N):
    """x float32 [n_in][T] -> float32 [n_out * (1 + order)][T]: statics, deltas, delta-deltas"""
    out = [static(x, matrix)]
    for _ in range(order):
        out.append(delta(out[-1], N))
    return np.concatenate(out, axis=0)


def rows(x, n, fill_to, dst, matrix, order, N):
    """x float32 [rows][ch][n_in][cap]; dst: the destination before the call, [rows][ch][n_out * (1 + order)][cap].  Returns the
    destination after the call"""
    x = np.asarray(x, F32)
    out = np.array(dst, F32, copy=True)
    R, C = x.shape[:2]
    for r in range(R):
        k = int(n[r])
        end = max(k, int(fill_to[r]) if fill_to is not None else 0)
        for c in range(C):
            if k:
                out[r, c, :, :k] = lines(x[r, c, :, :k], matrix, order, N)
            out[r, c, :, k:end] = 0.0
    return out


def same_bits(got, want, sentinel=None):
    """bits; a NaN result equals any NaN (which NaN it is, is outside the contract) except the destination's sentinel, which marks
    what must not have been written"""
    g, w = (np.ascontiguousarray(v, F32) for v in (got, want))
    assert g.shape == w.shape, (g.shape, w.shape)
    gb, wb = g.view(np.uint32), w.view(np.uint32)
    nan = np.isnan(g) & np.isnan(w)
    if sentinel is not None:
        nan &= (gb != sentinel) & (wb != sentinel)
    same = (gb == wb) | nan
    assert same.all(), (int((~same).sum()), np.argwhere(~same)[:4].tolist(), g[~same][:4].tolist(), w[~same][:4].tolist())


def source(n, ch, F, cap, seed, special=False):
    """float32 [rows][ch][F][cap]: dB-like noise of differing level per line; special: NaN, +-inf, +-0, subnormals and FLT_MAX strewn
    in per row (row 0 none, then one kind more per row, cyclically); the sentinel NaN at and beyond each n"""
    rng = np.random.default_rng(seed)
    x = np.full((len(n), ch, F, cap), SENT_F, F32)
    odd = np.array([0.0, -0.0, 1e-42, -1.4e-45, 3.4028234663852886e38, np.inf, -np.inf, np.nan], F32)
    for r, k in enumerate(n):
        v = (rng.standard_normal((ch, F, k)) * rng.uniform(2.0, 20.0, (ch, F, 1)) - 40.0).astype(F32)
        if special and r % (len(odd) + 1):
            pick = rng.random((ch, F, k)) < 0.2
            v[pick] = odd[rng.integers(0, r % (len(odd) + 1), int(pick.sum()))]
        x[r, :, :, :k] = v
    return x


def matrix(n_out, n_in, seed):
    """a dense float32 test matrix with a zero, a negative zero and a subnormal among its weights"""
    rng = np.random.default_rng(seed)
    m = (rng.standard_normal((n_out, n_in)) / np.sqrt(n_in)).astype(F32)
    flat = m.ravel()
    flat[::7] = 0.0
    flat[3::11] = -0.0
    flat[5::13] = 1e-41
    return m


def dct_reference(n_out, n_in, norm, lifter):
    """the DCT-II matrix written out element by element in float64 (independent of lewton_amd.rows.dct_matrix), rounded once"""
    m = np.zeros((n_out, n_in), F64)
    for q in range(n_out):
        for f in range(n_in):
            v = np.cos(np.pi * q * (2 * f + 1) / (2.0 * n_in))
            if norm == "ortho":
                v *= np.sqrt(1.0 / n_in) if q == 0 else np.sqrt(2.0 / n_in)
            else:
                v *= 2.0
            if lifter:
                v *= 1.0 + (lifter / 2.0) * np.sin(np.pi * q / lifter)
            m[q, f] = v
    return m.astype(F32)


def _delta_of(s, s_lo, lo, hi, T, N):
    """the delta at frames [lo, hi) of lines s that hold frames [s_lo, s_lo + s.shape[1]) of a row of T frames"""
    w = delta_weights(N)
    acc = np.zeros((s.shape[0], hi - lo), F32)
    for n in range(1, N + 1):
        after = np.array([min(max(t + n, 0), T - 1) - s_lo for t in range(lo, hi)], np.int64)
        before = np.array([min(max(t - n, 0), T - 1) - s_lo for t in range(lo, hi)], np.int64)
        assert hi == lo or (min(after.min(), before.min()) >= 0 and max(after.max(), before.max()) < s.shape[1])
        with np.errstate(over="ignore", invalid="ignore"):
            d = s[:, after] - s[:, before]
        assert d.dtype == F32
        acc = fmaf(w[n - 1], d, acc)
    return acc


def window(row, a, b, T, fill_end, before, matrix, order, N):
    """The window form of rows() for ONE row and channel that is +0.0 outside a few windows (tests/sparse_rows.py: row has n_in
    lines of at least T frames): frames [a, b) of every destination line after the call, from `before` float32
    [n_out * (1 + order)][b - a].  Each delta level is computed over the frames the next one refers to, the indices clamped into
    [0, T - 1] in Python integers -- at the row's true ends, wherever the window lies"""
    assert 0 <= a <= b and T <= fill_end
    out = np.array(before, F32, copy=True)
    lo, hi = min(a, T), min(b, T)
    if hi > lo:
        spans = [(lo, hi)]                                           # the frames level `order`, .., 0 must cover
        for _ in range(order):
            spans.append((max(0, spans[-1][0] - N), min(T, spans[-1][1] + N)))
        spans.reverse()
        s_lo, s_hi = spans[0]
        level = static(row.clipped(T).take(s_lo, s_hi), matrix)
        n_out = level.shape[0]
        out[:n_out, lo - a:hi - a] = level[:, lo - s_lo:hi - s_lo]
        for k in range(1, order + 1):
            level, (s_lo, s_hi) = _delta_of(level, s_lo, spans[k][0], spans[k][1], T, N), spans[k]
            out[k * n_out:(k + 1) * n_out, lo - a:hi - a] = level[:, lo - s_lo:hi - s_lo]
    f0, f1 = min(max(a, T), fill_end), min(b, fill_end)
    if f1 > f0:
        out[:, f0 - a:f1 - a] = 0.0
    return out
