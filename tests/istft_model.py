"""The model of the inverse spectral frames (include/lewton_amd.h, "inverse spectral frames of rows") for the CPU and the GPU suite,
independent of the kernel source.  Three things:

  the bit model   table() / window2() build the tables in numpy float64 (table_f32: rounded once); istft() runs the contract over
                  table bits it is GIVEN (the suites pass the library's own, lw_istft_basis / lw_istft_window2, which
                  tests/test_host_istft.py holds against table() and window2()): the frame chains with spec_model.fmaf, l ascending,
                  the overlap-add and the envelope as explicit loops over t ascending, indices in Python integers.
  the yardstick   yardstick(): numpy.fft.irfft times the window, overlap-added and divided by the envelope, all in float64 -- the
                  published algorithm of torch.istft.
  the bound       bound(): how far the bit model may lie from the yardstick, DERIVED per sample from the operands, in the manner
                  of tests/kaldi_model.py; stft_bound() is the same for the forward chains, and the round trip composes the two.

U = 2^-24 is the unit roundoff of float32.  An fmaf chain of n terms over operands a_i b_i lies within n U / (1 - n U) sum |a_i b_i|
of the exact sum (Higham, Accuracy and Stability, 3.1, with one rounding per term); a table entry rounded once adds U |a_i b_i|
per term, which is the "+ 1"."""
import numpy as np

from spec_model import fmaf

U = 2.0 ** -24
TINY = 2.0 ** -149                       # the spacing of the float32 subnormals: what one rounding down there can cost at most


def window(name, W):
    i = np.arange(W, dtype=np.float64)
    if name == "rect":
        return np.ones(W)
    if name == "hann":
        return 0.5 - 0.5 * np.cos(2.0 * np.pi * i / W)
    a = 2.0 * np.pi * i / (W - 1)
    return {"hann_sym": lambda: 0.5 - 0.5 * np.cos(a), "hamming_sym": lambda: 0.54 - 0.46 * np.cos(a),
            "povey": lambda: (0.5 - 0.5 * np.cos(a)) ** 0.85, "blackman_sym": lambda: 0.42 - 0.5 * np.cos(a) + 0.08 * np.cos(2.0 * a)}[name]()


def geometry(n_fft, win_length, hop, center, T):
    """(B, o, pad, P, natural length)"""
    pad = n_fft // 2 if center else 0
    P = 0 if T == 0 else n_fft + (T - 1) * hop
    return n_fft // 2 + 1, (n_fft - win_length) // 2, pad, P, (0 if T == 0 else P - 2 * pad)


def table(n_fft, win_length, name):
    """float64 [2 B][win_length]: the cosine lines, then the sine lines; +0.0 exactly on the sine lines irfft ignores"""
    B, o = n_fft // 2 + 1, (n_fft - win_length) // 2
    w = window(name, win_length)
    k, j = np.arange(win_length, dtype=np.int64)[None, :], np.arange(B, dtype=np.int64)[:, None]
    a = 2.0 * np.pi * (((k + o) * j) % n_fft).astype(np.float64) / n_fft
    c = np.full((B, 1), 2.0)
    c[0] = 1.0
    if n_fft % 2 == 0:
        c[n_fft // 2] = 1.0
    gc = w[None, :] * c * np.cos(a) / n_fft
    gs = -(w[None, :] * c * np.sin(a)) / n_fft
    gs[(c == 1.0)[:, 0]] = 0.0
    return np.concatenate([gc, gs])


def table_f32(n_fft, win_length, name):
    return table(n_fft, win_length, name).astype(np.float32)


def window2(name, W):
    w = window(name, W)
    return w * w


def frame_signals(G, X):
    """G float32 [2 B][W], X float32 [2 B][T] -> y float32 [T][W]: ONE chain per (t, k) over the lines, ascending"""
    G, X = np.asarray(G, np.float32), np.asarray(X, np.float32)
    y = np.zeros((X.shape[1], G.shape[1]), np.float32)
    for l in range(G.shape[0]):
        y = fmaf(X[l][:, None], G[l][None, :], y)
    return y


def overlap_add(y, n_fft, win_length, hop, dtype=np.float32):
    """[T][W] -> [P]: for every p the fold over the frames that touch it, t ascending, one rounded add each, from +0.0"""
    T, o = y.shape[0], (n_fft - win_length) // 2
    P = 0 if T == 0 else n_fft + (T - 1) * hop
    xh = np.zeros(P, dtype)
    with np.errstate(invalid="ignore", over="ignore"):
        for t in range(T):
            at = t * hop + o
            xh[at:at + win_length] = (xh[at:at + win_length] + y[t].astype(dtype)).astype(dtype)
    return xh


def envelope(w2, T, n_fft, hop):
    """float64 [P]: the same fold of w2, in double"""
    w2 = np.asarray(w2, np.float64)
    return overlap_add(np.broadcast_to(w2, (T, len(w2))), n_fft, len(w2), hop, np.float64)


def _cut(v, pad, P, length):
    """samples [0, length) of the row from padded coordinates: +0.0 where p >= P"""
    out = np.zeros(length, v.dtype)
    n = max(0, min(length, P - pad))
    out[:n] = v[pad:pad + n]
    return out


def istft(G, w2, X, n_fft, hop, center, length=None):
    """the contract: float32 [length] of one row and channel from its lines X float32 [2 B][T]"""
    win_length, T = np.asarray(G).shape[1], np.asarray(X).shape[1]
    _, _, pad, P, natural = geometry(n_fft, win_length, hop, center, T)
    length = natural if length is None else int(length)
    xh = overlap_add(frame_signals(G, X), n_fft, win_length, hop)
    env = envelope(w2, T, n_fft, hop)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        v = np.where(env > 1e-11, (xh.astype(np.float64) / env).astype(np.float32), np.float32(0.0)).astype(np.float32)
    return _cut(v, pad, P, length)


def window_rows(G, w2, row, a, b, T, n_fft, hop, center, length, before):
    """The window form of istft() for ONE row and channel whose lines are +0.0 outside a few windows (tests/sparse_rows.py: row a
    SparseRow of the 2 B lines, of at least T frames): samples [a, b) of the destination after the call, from `before` float32
    [b - a].  Only the frames that touch the padded samples [a + pad, b + pad) are ever held; the overlap-add and the envelope of
    those samples are the complete ascending folds, because every frame that touches one of them is among these"""
    win_length = np.asarray(G).shape[1]
    _, o, pad, P, _ = geometry(n_fft, win_length, hop, center, T)
    assert 0 <= a <= b
    out = np.array(before, np.float32, copy=True)
    hi = min(b, int(length))
    if hi <= a:
        return out
    out[:hi - a] = 0.0                                                 # behind what the frames cover
    p0, p1 = a + pad, min(hi + pad, P)
    if p1 <= p0:
        return out
    t0 = max(0, -(-(p0 - o - win_length + 1) // hop))                  # the first frame with t hop + o + W - 1 >= p0
    t1 = min(T - 1, (p1 - 1 - o) // hop)                               # the last with t hop + o <= p1 - 1
    if t1 < t0:
        return out
    X = row.clipped(T).take(t0, t1 + 1)
    base = t0 * hop                                                    # the padded sample at which the local fold starts
    xh = overlap_add(frame_signals(G, X), n_fft, win_length, hop)
    env = envelope(w2, t1 + 1 - t0, n_fft, hop)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        v = np.where(env > 1e-11, (xh.astype(np.float64) / env).astype(np.float32), np.float32(0.0)).astype(np.float32)
    lo, up = max(p0, base), min(p1, base + len(v))
    if up > lo:
        out[lo - pad - a:up - pad - a] = v[lo - base:up - base]
    return out


def yardstick(Xc, name, n_fft, win_length, hop, center, length=None):
    """float64 [length] from complex128 [B][T]: irfft, window, overlap-add, division by the envelope; NaN where the envelope is
    not above 1e-11 (where torch.istft raises) and 0 behind what the frames cover"""
    Xc = np.asarray(Xc, np.complex128)
    T = Xc.shape[1]
    _, o, pad, P, natural = geometry(n_fft, win_length, hop, center, T)
    length = natural if length is None else int(length)
    w = window(name, win_length)
    y = np.fft.irfft(Xc.T, n=n_fft, axis=1)[:, o:o + win_length] * w[None, :] if T else np.zeros((0, win_length))
    xh = overlap_add(y, n_fft, win_length, hop, np.float64)
    env = envelope(w * w, T, n_fft, hop)
    with np.errstate(divide="ignore", invalid="ignore"):
        v = np.where(env > 1e-11, xh / env, np.nan)
    return _cut(v, pad, P, length)


def bound(G, w2, X, n_fft, hop, center, length=None, dX=None):
    """float64 [length]: |istft() - yardstick| is at most this on every sample where the envelope is above 1e-11 (+inf elsewhere
    in the covered part: the yardstick has no value there).  G is the float32 table the model ran with.  Derivation, per sample:
      y    the chain of 2 B terms over a table rounded once: (2 B + 1) U / (1 - (2 B + 1) U) * S, S = sum_l |X[l][t]| |G[l][k]|,
           plus one subnormal spacing per term; irfft's own error in double is below 2 B 2^-52 S and is added.
      dX   (the round trip) an error of at most dX[l][t] on the source reaches y through the exact transform: sum_l dX |G|.
      add  n adds of one rounding each: n U / (1 - n U) times the sum of the magnitudes, sum_t (|y_t| + e_t) <= sum_t (S_t + e_t).
      /    the quotient in double and its rounding to float32: U (1 + 2^-28) relative (the envelope's own fold and the division
           in double cost a few 2^-53, inside the 2^-28), plus one subnormal spacing."""
    G64, X64 = np.abs(np.asarray(G, np.float32).astype(np.float64)), np.abs(np.asarray(X, np.float32).astype(np.float64))
    L, W = G64.shape
    T = X64.shape[1]
    _, _, pad, P, natural = geometry(n_fft, W, hop, center, T)
    length = natural if length is None else int(length)
    S = X64.T @ G64                                                    # [T][W]
    n = L + 1
    e_y = n * U / (1.0 - n * U) * S + L * TINY + L * 2.0 ** -52 * S
    if dX is not None:
        e_y = e_y + np.asarray(dX, np.float64).T @ G64
    count = overlap_add(np.ones((T, W)), n_fft, W, hop, np.float64)
    mag = overlap_add(S + e_y, n_fft, W, hop, np.float64)
    e_x = overlap_add(e_y, n_fft, W, hop, np.float64) + count * U / (1.0 - count * U) * mag + count * TINY
    env = envelope(w2, T, n_fft, hop)
    with np.errstate(divide="ignore", invalid="ignore"):
        e = np.where(env > 1e-11, (e_x + (mag + e_x) * U * (1.0 + 2.0 ** -28)) / env + TINY, np.inf)
    return _cut(e, pad, P, length)


def stft_bound(basis, X):
    """float64 [2 B][T]: how far the forward chains (spec_model.features' re and im over the frame matrix X [T][W], basis
    float32 [2][W][B] rounded once) may lie from the exact transform: (W + 1) U / (1 - (W + 1) U) sum_k |x_k| |C[k][j]|"""
    basis = np.abs(np.asarray(basis, np.float32).astype(np.float64))
    X = np.abs(np.asarray(X, np.float32).astype(np.float64))
    n = basis.shape[1] + 1
    S = np.concatenate([X @ basis[0], X @ basis[1]], axis=1).T        # [2 B][T]
    return n * U / (1.0 - n * U) * S + basis.shape[1] * TINY
