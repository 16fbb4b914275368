"""The models of the Kaldi-compatible front end (include/lewton_amd.h, "spectral frames of rows": framing, folded, per frame) for the
CPU and the GPU suite, independent of the kernel source.

BIT MODEL.  The frame matrix per framing with the symmetric reflection in Python integers; S1 / S2 as sequential float64 loops
over k (never np.sum, whose pairwise order is not the contract's); mu, x' and E by the contract's roundings; then
spec_model.features over x' with the library's own table bits, the energy line in front.

FLOAT64 YARDSTICK.  Kaldi's published algorithm restated directly (frame, mean, energy, pre-emphasis, window, rfft, banks, log):
what torchaudio.compliance.kaldi.fbank and kaldi-native-fbank compute, in float64 throughout.

BOUND.  How far the bit model may be from the yardstick, derived (bound() below), not observed."""
import numpy as np

import spec_model as M

F32, F64 = np.float32, np.float64
EPS = F32(np.finfo(np.float32).eps)                      # Kaldi's floor under the logarithm
HANN, RECT, POVEY, HAMMING, HANN_SYM, BLACKMAN = range(6)
WINDOWS = {"hann": HANN, "rect": RECT, "povey": POVEY, "hamming_sym": HAMMING, "hann_sym": HANN_SYM, "blackman_sym": BLACKMAN}
STFT, SNIP, EDGES = 0, 1, 2
U = 2.0 ** -24                                           # the unit roundoff of float32


# ---- framing, in Python integers
def n_frames(n, W, hop, snip):
    if snip:
        return 0 if n < W else 1 + (n - W) // hop
    return (n + hop // 2) // hop


def first_index(t, W, hop, snip):
    """the input index of support sample 0 of frame t"""
    return t * hop if snip else t * hop + hop // 2 - W // 2


def touched(n, W, hop, snip):
    """(first, last) index any frame of a row of n samples touches, or None without frames"""
    T = n_frames(n, W, hop, snip)
    return None if T == 0 else (first_index(0, W, hop, snip), first_index(T - 1, W, hop, snip) + W - 1)


def accepted(n, W, hop, snip):
    """one reflection reaches every index: first >= -n and last <= 2 n - 1"""
    ft = touched(n, W, hop, snip)
    return ft is None or (ft[0] >= -n and ft[1] <= 2 * n - 1)


def sym_index(i, n):
    """x[i] = x[-i - 1] below 0, x[2 n - 1 - i] from n on"""
    i = int(i)
    if i < 0:
        i = -i - 1
    if i >= n:
        i = 2 * n - 1 - i
    assert 0 <= i < n
    return i


def frame_matrix(x, W, hop, snip):
    """float32 [frames][W]: the support samples of every frame of one row and channel x (its len samples), after padding"""
    x = np.asarray(x, F32)
    n = len(x)
    T = n_frames(n, W, hop, snip)
    assert accepted(n, W, hop, snip)
    idx = np.array([[sym_index(first_index(t, W, hop, snip) + k, n) for k in range(W)] for t in range(T)], np.int64).reshape(T, W)
    return x[idx]


# ---- the per-frame part
def sums(X):
    """S1, S2 float64 [frames]: sequential folds over k ascending from +0.0"""
    X = np.asarray(X, F32).astype(F64)
    S1, S2 = np.zeros(X.shape[0], F64), np.zeros(X.shape[0], F64)
    with np.errstate(all="ignore"):
        for k in range(X.shape[1]):
            S1 = S1 + X[:, k]
            S2 = S2 + X[:, k] * X[:, k]
    return S1, S2


def prologue(X, remove_dc, scale):
    """(x' float32 [frames][W], E float32 [frames])"""
    X = np.asarray(X, F32)
    W = F64(X.shape[1])
    S1, S2 = sums(X)
    with np.errstate(all="ignore"):
        mu = (S1 / W).astype(F32)
        Xp = (X - mu[:, None]).astype(F32) if remove_dc else X
        Ed = S2 - (S1 * S1) / W if remove_dc else S2
        Ed = np.where(Ed > 0, Ed, 0.0)
        E = (Ed * (F64(scale) * F64(scale))).astype(F32)
    return Xp, E


def features(basis, fb, X, remove_dc=False, energy=False, scale=1.0):
    """float32 [frames][F]: the energy line (when asked for) in front of spec_model.features over x'"""
    if not (remove_dc or energy):
        return M.features(basis, fb, X)
    Xp, E = prologue(X, remove_dc, scale)
    Y = M.features(basis, fb, Xp)
    return np.concatenate([E[:, None], Y], axis=1) if energy else Y


def same_bits(got, want, sentinel=None):
    """bits, -0 as +0; a NaN equals any NaN but the sentinel"""
    g, w = (np.ascontiguousarray(v, F32).view(np.uint32).copy() for v in (got, want))
    assert g.shape == w.shape, (g.shape, w.shape)
    g[g == 0x80000000] = 0
    w[w == 0x80000000] = 0
    nan = np.isnan(g.view(F32)) & np.isnan(w.view(F32))
    if sentinel is not None:
        nan &= (g != sentinel) & (w != sentinel)
    same = (g == w) | nan
    assert same.all(), (int((~same).sum()), np.argwhere(~same)[:4].tolist(), g[~same][:4].tolist(), w[~same][:4].tolist())


# ---- the tables, by the formula in float64
def window(kind, W):
    i = np.arange(W, dtype=F64)
    if kind == RECT:
        return np.ones(W, F64)
    if kind == HANN:
        return 0.5 - 0.5 * np.cos(2 * np.pi * i / W)
    a = 2 * np.pi * i / (W - 1)
    if kind == HAMMING:
        return 0.54 - 0.46 * np.cos(a)
    if kind == HANN_SYM:
        return 0.5 - 0.5 * np.cos(a)
    if kind == POVEY:
        return (0.5 - 0.5 * np.cos(a)) ** 0.85
    return 0.42 - 0.5 * np.cos(a) + 0.08 * np.cos(2 * a)


def table(n_fft, W, kind, offset, c=0.0, scale=1.0):
    """float64 [2][W][B], the folded basis BEFORE its one rounding to float32"""
    B = n_fft // 2 + 1
    w = window(kind, W)
    kj = ((np.arange(W, dtype=np.int64)[:, None] + offset) * np.arange(B, dtype=np.int64)[None, :]) % n_fft
    ang = 2 * np.pi * kj.astype(F64) / n_fft
    out = np.zeros((2, W, B), F64)
    for s, g in enumerate((w[:, None] * np.cos(ang), -w[:, None] * np.sin(ang))):
        nxt = np.concatenate([g[1:], np.zeros((1, B))])
        lead = np.ones((W, 1))
        lead[0] = 1.0 - c
        out[s] = scale * (lead * g - c * nxt)
    return out


# ---- the yardstick
def yardstick(x, n_fft, W, hop, snip, kind, fb, c=0.97, remove_dc=True, energy=False, scale=1.0, parts=False):
    """float64 [frames][F]: ln(max(., eps)) of Kaldi's fbank of one row x, the log energy in front when asked for.  parts: also
    (re, im) float64 [frames][B] and the linear values"""
    X = frame_matrix(x, W, hop, snip).astype(F64) * scale
    if remove_dc:
        X = X - X.mean(axis=1, keepdims=True)
    E = (X * X).sum(axis=1)
    Y = X.copy()
    Y[:, 1:] = X[:, 1:] - c * X[:, :-1]
    Y[:, 0] = X[:, 0] - c * X[:, 0]
    spec = np.fft.rfft(Y * window(kind, W)[None, :], n=n_fft, axis=1)
    P = spec.real ** 2 + spec.imag ** 2
    lin = P if fb is None else P @ np.asarray(fb, F32).astype(F64).T
    if energy:
        lin = np.concatenate([E[:, None], lin], axis=1)
    out = np.log(np.maximum(lin, F64(EPS)))
    return (out, spec.real, spec.imag, lin) if parts else out


def bound(basis, fb, Xp, mu, re, im, lin, energy, scale=1.0):
    """How far ln(max(m, eps)) of the bit model may lie from the yardstick's, float64 [frames][F]; Xp the model's x' (float32),
    mu its means (zeros without remove_dc), re / im / lin the yardstick's exact values.

    amplitude  re_j is a chain of W fmaf over x'_k C[k][j]: W roundings of partial sums, none above A_j = sum_k |x'_k| |C[k][j]|;
               C is the exact table rounded once (U relative), x'_k = x_k - mu one rounded subtraction (U relative): (W + 2) U A_j.
               mu itself is a float64 quotient rounded to float32, off by U |mu| in EVERY sample of the frame alike: U |mu|
               sum_k |C[k][j]| more.  (S1 is a float64 fold: 2^-53 W, nothing at this scale.)
    power      P = re^2 + im^2 with two rounded operations: 2 |re| e + e^2 per part, and 2 U P.
    band       m_q a chain of B fmaf over P_j fb[q][j], the same float32 banks on both sides: sum_j dP_j fb[q][j] and B U m_q.
    logarithm  ln is 1 / v-Lipschitz and the floor a clamp: dm / max(m - dm, eps); the contract's LOG is the correctly rounded
               float32 logarithm but for its last place: 2 U max(|l|, 1).
    energy     E = S2 - S1^2 / W in float64 from exact squares, rounded once to float32: U E for that rounding, and the
               cancellation's share, a few float64 roundings of S2 on either side (W + 3 of them, 2^-53 each, of at most
               scale^2 sum_k (|x'_k| + |mu|)^2): taken as 2^-40 of that sum for every W up to 2048."""
    C, S = np.abs(basis[0].astype(F64)), np.abs(basis[1].astype(F64))
    W = C.shape[0]
    ax = np.abs(Xp.astype(F64))
    am = np.abs(np.asarray(mu, F64))[:, None]
    e_re = (W + 2) * U * (ax @ C) + U * am * C.sum(axis=0)[None, :]
    e_im = (W + 2) * U * (ax @ S) + U * am * S.sum(axis=0)[None, :]
    P = re * re + im * im
    dP = 2 * np.abs(re) * e_re + e_re ** 2 + 2 * np.abs(im) * e_im + e_im ** 2
    dP = dP + 2 * U * (P + dP)
    if fb is None:
        m, dm = P, dP
    else:
        f = np.asarray(fb, F32).astype(F64).T
        m, dm = P @ f, dP @ f
        dm = dm + f.shape[0] * U * (m + dm)
    if energy:
        E = lin[:, :1]
        S2 = (scale * scale) * ((ax + am) ** 2).sum(axis=1, keepdims=True)
        m, dm = np.concatenate([E, m], axis=1), np.concatenate([U * E + 2.0 ** -40 * S2, dm], axis=1)
    l = np.log(np.maximum(m, F64(EPS)))
    return dm / np.maximum(m - dm, F64(EPS)) + 2 * U * np.maximum(np.abs(l), 1.0)


def frame_matrix_window(row, a, b, W, hop, snip):
    """The window form of frame_matrix for a row that is +0.0 outside a few windows (tests/sparse_rows.py: one line, row.n its
    len): frames [a, b), every index by sym_index's rule at the row's true ends"""
    n = row.n
    assert accepted(n, W, hop, snip) and 0 <= a <= b <= n_frames(n, W, hop, snip)
    i = (np.arange(a, b, dtype=np.int64) * hop + first_index(0, W, hop, snip))[:, None] + np.arange(W, dtype=np.int64)[None, :]
    i = np.where(i < 0, -i - 1, i)
    i = np.where(i >= n, 2 * n - 1 - i, i)
    return row.gather(i)[0]
