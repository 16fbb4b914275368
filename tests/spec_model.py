"""The model of the spectral frames (include/lewton_amd.h, "spectral frames of rows") for the CPU and the GPU suite: fmaf chains
in numpy with the library's own table bits, independent of the kernel source.

numpy has no fmaf, and float32(float64(a) * b + c) rounds twice.  fmaf() below is exact: the product of two float32 is exact in
float64, the sum's rounding error e is recovered (two-sum), and where the float64 sum lies exactly half way between two float32
values (the only place where the second rounding can go wrong) e decides the direction.  tests/test_host_spec.py pins it to
glibc's fmaf."""
import numpy as np


def fmaf(a, b, c):
    """float32 fma(a, b, c) with ONE rounding, elementwise"""
    a, b, c = (np.asarray(v, np.float32).astype(np.float64) for v in (a, b, c))
    with np.errstate(over="ignore", invalid="ignore"):
        p = a * b                                               # exact
        s = p + c
        bb = s - p
        e = (p - (s - bb)) + (c - bb)                           # s + e = p + c exactly
        r = s.astype(np.float32)
        d = s - r.astype(np.float64)
        n = np.nextafter(r, np.where(d > 0, np.float32(np.inf), np.float32(-np.inf)).astype(np.float32))
        fix = (d != 0) & (n.astype(np.float64) - s == d) & (e != 0) & (np.sign(e) == np.sign(d))
    return np.where(fix, n, r).astype(np.float32)


def naive_fmaf(a, b, c):
    """the form that rounds twice (what the emulation is there to avoid)"""
    return (np.asarray(a, np.float32).astype(np.float64) * np.asarray(b, np.float32).astype(np.float64)
            + np.asarray(c, np.float32).astype(np.float64)).astype(np.float32)


def n_frames(n, n_fft, hop, center):
    if n == 0:
        return 0
    if center:
        return 1 + n // hop
    return 0 if n < n_fft else 1 + (n - n_fft) // hop


def frame_matrix(x, n_fft, win_length, hop, center):
    """float32 [frames][win_length]: the support samples of every frame of one row and channel x (its len samples), +0.0 outside"""
    x = np.asarray(x, np.float32)
    L, T = len(x), n_frames(len(x), n_fft, hop, center)
    o, pad = (n_fft - win_length) // 2, (n_fft // 2 if center else 0)
    idx = np.arange(T, dtype=np.int64)[:, None] * hop - pad + o + np.arange(win_length, dtype=np.int64)[None, :]
    xp = np.concatenate([x, np.zeros(1, np.float32)])
    return xp[np.where((idx >= 0) & (idx < L), idx, L)]


def features(basis, fb, X):
    """basis [2][win_length][B] (lw_spec_basis), fb [n_mels][B] or None, X [T][win_length] -> float32 [T][F]: the chains of the
    contract, k and j ascending, every step one fmaf over all frames at once"""
    C, S = basis[0], basis[1]
    T, B = X.shape[0], C.shape[1]
    re, im = np.zeros((T, B), np.float32), np.zeros((T, B), np.float32)
    for k in range(C.shape[0]):
        xk = X[:, k:k + 1]
        re, im = fmaf(xk, C[k][None, :], re), fmaf(xk, S[k][None, :], im)
    sq = re * re
    assert sq.dtype == np.float32
    P = fmaf(im, im, sq)
    if fb is None:
        return P
    fb = np.asarray(fb, np.float32)
    m = np.zeros((T, fb.shape[0]), np.float32)
    for j in range(B):
        m = fmaf(P[:, j:j + 1], fb[:, j][None, :], m)
    return m


def same_bits(got, want):
    """-0 counts as +0 (the sign of a zero is outside the contract), then bits"""
    g, w = (np.ascontiguousarray(v, np.float32).view(np.uint32).copy() for v in (got, want))
    g[g == 0x80000000] = 0
    w[w == 0x80000000] = 0
    same = g == w
    assert same.all(), (int((~same).sum()), np.argwhere(~same)[:4].tolist())


def frame_matrix_window(row, a, b, n_fft, win_length, hop, center):
    """The window form of frame_matrix for a row that is +0.0 outside a few windows (tests/sparse_rows.py: one line, row.n its
    len): frames [a, b), float32 [b - a][win_length], +0.0 outside [0, len) at the row's true ends"""
    L = row.n
    assert 0 <= a <= b <= n_frames(L, n_fft, hop, center)
    o, pad = (n_fft - win_length) // 2, (n_fft // 2 if center else 0)
    idx = np.arange(a, b, dtype=np.int64)[:, None] * hop - pad + o + np.arange(win_length, dtype=np.int64)[None, :]
    inside = (idx >= 0) & (idx < L)
    return np.where(inside, row.gather(np.where(inside, idx, 0))[0], np.float32(0.0)).astype(np.float32)
