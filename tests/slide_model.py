"""The model of lw_slide_rows (include/lewton_amd.h, "sliding-window normalisation of feature rows") for the CPU and the GPU suite,
independent of the kernel source: rule 1 in Python integers; the block sums as sixteen float64 additions from +0.0; the window sum
as ONE float64 accumulator per frame over the list of terms rule 3 names (head elements, block sums, tail elements), the lists
written out per frame in Python integers and folded for all lines and frames of a row at once, one numpy addition per position of
the list; rule 4 in float64 with one rounding to float32.  numpy's float64 + - * / and sqrt are single IEEE operations."""
import math

import numpy as np

F32, F64 = np.float32, np.float64
U = 2.0 ** -53                          # the unit roundoff of a double
BLOCK = 16
MAX_WINDOW = 2048

SENT = 0x7FC0DEAD                     # a NaN: the destination's sentinel, and what the source holds at and beyond n
SENT_F = np.array(SENT, np.uint32).view(F32)


def window(t, T, W, min_window, center):
    """rule 1: (s, e) of frame t of a line of T frames"""
    assert 0 <= t < T
    if center:
        s = t - W // 2
        e = s + W
    else:
        s = t - W
        e = t + 1
    if s < 0:
        e -= s
        s = 0
    if not center and e > t:
        e = max(t + 1, min_window)
    if e > T:
        s -= e - T
        e = T
        if s < 0:
            s = 0
    return s, e


def terms(s, e, T):
    """rule 3: the terms of the window [s, e) in the accumulator's order, as indices into [the T elements | the T // 16 block sums]"""
    b0, b1 = -(-s // BLOCK), e // BLOCK
    if b0 >= b1:
        return list(range(s, e))
    return list(range(s, BLOCK * b0)) + [T + b for b in range(b0, b1)] + list(range(BLOCK * b1, e))


def depth(W):
    """the most additions an element passes through on its way into S: 16 in its block, then at most every term of rule 3"""
    return BLOCK + (BLOCK - 1) + (W + 1) // BLOCK + 1 + (BLOCK - 1)


def _block_sums(v):
    """rule 2 of float64 [L][T] values: [L][T // 16], i ascending from +0.0"""
    nb = v.shape[1] // BLOCK
    acc = np.zeros((v.shape[0], nb), F64)
    for i in range(BLOCK):
        acc = acc + v[:, i:BLOCK * nb:BLOCK]
    return acc


def sums(x, W, min_window, center):
    """x float32 [L][T] (T >= 1) -> (S, Q, n), float64 [L][T] twice and int64 [T]: rules 1 - 3 for every frame of every line"""
    x = np.asarray(x, F32)
    L, T = x.shape
    wins = [window(t, T, W, min_window, center) for t in range(T)]
    lists = [terms(s, e, T) for s, e in wins]
    K = max(len(v) for v in lists)
    idx = np.zeros((T, K), np.int64)
    cnt = np.array([len(v) for v in lists], np.int64)
    for t, v in enumerate(lists):
        idx[t, :len(v)] = v
    with np.errstate(over="ignore", invalid="ignore"):
        d = x.astype(F64)
        out = []
        for v in (d, d * d):                                           # (the squares of floats are exact in double)
            pool = np.concatenate([v, _block_sums(v)], axis=1)
            acc = np.zeros((L, T), F64)
            for k in range(K):
                acc = np.where((k < cnt)[None, :], acc + pool[:, idx[:, k]], acc)
            out.append(acc)
    return out[0], out[1], np.array([e - s for s, e in wins], np.int64)


def value(x, S, Q, n, norm_vars):
    """rule 4: x float32 [L][T], S and Q float64 [L][T], n int64 [T] -> float32 [L][T]"""
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        dn = n.astype(F64)[None, :]
        mu = S / dn
        c = x.astype(F64) - mu
        if not norm_vars:
            return c.astype(F32)
        v = Q / dn - mu * mu
        v = np.where(v > 1e-10, v, 1e-10)
        g = 1.0 / np.sqrt(v)
        z = (c * g).astype(F32)
        return np.where((n == 1)[None, :], F32(0.0), z)


def lines(x, W, min_window, center, norm_vars):
    """x float32 [L][T] -> float32 [L][T]"""
    x = np.asarray(x, F32)
    if x.shape[1] == 0:
        return x.copy()
    S, Q, n = sums(x, W, min_window, center)
    return value(x, S, Q, n, norm_vars)


def rows(x, n, fill_to, dst, W, min_window, center, norm_vars):
    """x float32 [rows][ch][F][cap]; dst: the destination before the call, of x's shape.  Returns the destination after the call"""
    x = np.asarray(x, F32)
    out = np.array(dst, F32, copy=True)
    R, C, F, _ = x.shape
    for r in range(R):
        k = int(n[r])
        end = max(k, int(fill_to[r]) if fill_to is not None else 0)
        if k:
            out[r, :, :, :k] = lines(x[r, :, :, :k].reshape(C * F, k), W, min_window, center, norm_vars).reshape(C, F, k)
        out[r, :, :, k:end] = 0.0
    return out


def window_rows(row, a, b, T, fill_end, before, W, min_window, center, norm_vars):
    """The window form of rows() for ONE row that is +0.0 outside a few windows (tests/sparse_rows.py: row has the row's lines, all
    channels, of at least T frames): frames [a, b) of every destination line after the call, from `before` float32 [lines][b - a].
    Rules 1 and 3 are evaluated at the ABSOLUTE frames: the windows against the row's true T, the block sums on multiples of 16
    of the ROW wherever [a, b) lies.  Only the frames the windows of [a, b) reach are ever held: they start at a block boundary,
    so the local blocks are the row's"""
    assert 0 <= a <= b and T <= fill_end
    out = np.array(before, F32, copy=True)
    lo, hi = min(a, T), min(b, T)
    if hi > lo:
        wins = [window(t, T, W, min_window, center) for t in range(lo, hi)]
        s0 = min(s for s, _ in wins) // BLOCK * BLOCK
        e1 = max(e for _, e in wins)
        x = row.clipped(T).take(s0, e1)
        n_el = e1 - s0
        lists = [[i - s0 if i < T else n_el + (i - T) - s0 // BLOCK for i in terms(s, e, T)] for s, e in wins]
        K = max(len(v) for v in lists)
        idx = np.zeros((hi - lo, K), np.int64)
        cnt = np.array([len(v) for v in lists], np.int64)
        for t, v in enumerate(lists):
            idx[t, :len(v)] = v
        assert int(idx.min()) >= 0 and int(idx.max()) < n_el + n_el // BLOCK
        with np.errstate(over="ignore", invalid="ignore"):
            d = x.astype(F64)
            acc = []
            for v in (d, d * d):
                pool = np.concatenate([v, _block_sums(v)], axis=1)
                s = np.zeros((x.shape[0], hi - lo), F64)
                for k in range(K):
                    s = np.where((k < cnt)[None, :], s + pool[:, idx[:, k]], s)
                acc.append(s)
        n = np.array([e - s for s, e in wins], np.int64)
        out[:, lo - a:hi - a] = value(x[:, lo - s0:hi - s0], acc[0], acc[1], n, norm_vars)
    f0, f1 = min(max(a, T), fill_end), min(b, fill_end)
    if f1 > f0:
        out[:, f0 - a:f1 - a] = 0.0
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
    """float32 [rows][ch][F][cap]: log-mel-like noise N(-12, 3) of differing level per line; special: NaN, +-inf, +-0, subnormals and
    FLT_MAX strewn in per row (row 0 none, then one kind more per row, cyclically) and line 0 of every channel a constant (its
    variance is at the floor); the sentinel NaN at and beyond each n"""
    rng = np.random.default_rng(seed)
    x = np.full((len(n), ch, F, cap), SENT_F, F32)
    odd = np.array([0.0, -0.0, 1e-42, -1.4e-45, 3.4028234663852886e38, np.inf, -np.inf, np.nan], F32)
    for r, k in enumerate(n):
        v = (rng.standard_normal((ch, F, k)) * rng.uniform(1.0, 4.0, (ch, F, 1)) - 12.0).astype(F32)
        if special:
            if r % (len(odd) + 1):
                pick = rng.random((ch, F, k)) < 0.05
                v[pick] = odd[rng.integers(0, r % (len(odd) + 1), int(pick.sum()))]
            v[:, 0, :] = F32(-7.25)
        x[r, :, :, :k] = v
    return x


# ---- the shapes both suites run: (W, min, center, norm_vars) and the lengths of a call's three rows, one of them empty

def _calls(ts):
    ts = [t for t in ts if t]
    return [[ts[i], 0, ts[(i + 1) % len(ts)]] for i in range(0, len(ts), 2)]


SMALL = ([(4, 2, 1, nv) for nv in (0, 1)] + [(8, 3, 0, nv) for nv in (0, 1)] + [(33, 33, 0, 0), (16, 1, 1, 1)],
         _calls([0, 1, 2, 15, 16, 17, 31, 33, 64, 70]))
MID = ([(600, 100, 0, 0), (600, 100, 1, 1)], _calls([99, 100, 101, 599, 600, 601, 700]))
BIG = ([(2048, 1, 0, 1)], _calls([300, 2047, 2049, 2100]))
SHAPES = [(cfg, n) for cfgs, calls in (SMALL, MID, BIG) for cfg in cfgs for n in calls]
CH, LINES = 2, 5


# ---- the yardstick and the bound

def exact(x, W, min_window, center, norm_vars):
    """ONE line x (float32 [T]) -> (z, mu, v) as float64 [T] from window sums by math.fsum (exactly rounded, no block rule): the
    value rule 4 aims at, left unrounded"""
    T = len(x)
    d = [float(v) for v in x]
    q = [v * v for v in d]
    z, mus, vs = np.zeros(T, F64), np.zeros(T, F64), np.zeros(T, F64)
    for t in range(T):
        s, e = window(t, T, W, min_window, center)
        n = e - s
        mu = math.fsum(d[s:e]) / n
        v = math.fsum(q[s:e]) / n - mu * mu
        mus[t], vs[t] = mu, v
        if not norm_vars:
            z[t] = d[t] - mu
        elif n == 1:
            z[t] = 0.0
        else:
            z[t] = (d[t] - mu) / math.sqrt(max(v, 1e-10))
    return z, mus, vs


def bound(x, W, min_window, center, norm_vars, extra_S=0.0, extra_Q=0.0):
    """|model - exact| per frame of ONE line is at most this (float64 [T]), for windows whose exact variance is clear of the floor.
    With d = depth(W), u = 2^-53, a = the window's sum of |x| and q = its sum of squares:
      S, Q   every element passes through at most d additions:  |dS| <= d u a,  |dQ| <= d u q
      mu     one division more:                                 |dmu| <= (d + 1) u a / n
      c      = x - mu, one subtraction:                         |dc| <= |dmu| + u |c|
      v      = Q / n - mu^2:  |dv| <= u ((d + 1) q / n + 2 |mu| (d + 1) a / n + mu^2 + |v|)   (the cancellation: q / n and mu^2 are
             both about mu^2 + v)
      g      = 1 / sqrt(v):   |dg| / g <= |dv| / (2 v) + 2 u
      z      = c g:           |dz| <= g |dc| + |c| g (|dg| / g + u)
    all first order; the double terms carry a factor 1.001 for the orders left out.  The rounding to float32 adds half an ulp of
    the result: 2^-24 |z|, or 2^-150 for a subnormal.  extra_S and extra_Q (absolute) are added to |dS| and |dQ|: what the window
    sums of a SECOND witness, which is no exact yardstick, may be off by themselves; its few roundings behind the sums are of the
    kind counted above, so the double terms are then taken twice."""
    T = len(x)
    d = depth(W)
    a64 = np.abs(np.asarray(x, F64))
    z, mu, v = exact(x, W, min_window, center, norm_vars)
    out = np.zeros(T, F64)
    for t in range(T):
        s, e = window(t, T, W, min_window, center)
        n = e - s
        a, q = a64[s:e].sum(), (a64[s:e] ** 2).sum()
        dmu = ((d + 1) * U * a + extra_S) / n
        c = abs(float(x[t]) - mu[t])
        dc = dmu + U * c
        if not norm_vars:
            dz = dc
        elif n == 1:
            dz = 0.0
        else:
            assert v[t] > 4e-10, "the bound is for windows clear of the variance floor"
            dv = ((d + 1) * U * q + extra_Q) / n + 2 * abs(mu[t]) * dmu + U * (mu[t] ** 2 + abs(v[t]))
            g = 1.0 / math.sqrt(v[t])
            dz = g * dc + c * g * (dv / (2 * v[t]) + 3 * U)
        out[t] = (2.002 if extra_S or extra_Q else 1.001) * dz + max(2.0 ** -24 * abs(z[t]) * (1 + 2.0 ** -23), 2.0 ** -150)
    return out
