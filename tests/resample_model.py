"""The fold of lw_resample_rows (include/lewton_amd.h, "resampling rows") in numpy float32, as tests/rows_resample_gpu_cases.py
writes it (taps in ascending k, the first product is the accumulator, every later one is added, each operation one rounded float32
operation; x = +0.0 outside [0, len)), and its window form for a row that is +0.0 outside a few windows.  base and phase of an
output are formed in int64 -- output indices here pass 2^32 -- and base_phase() gives them in Python integers to compare."""
import numpy as np

F32 = np.float32


def base_phase(n, orig, new):
    """(floor(n orig / new), (n orig) mod new) of output n, in Python integers"""
    n, orig, new = int(n), int(orig), int(new)
    return n * orig // new, n * orig % new


def out_len(n, orig, new):
    return -(-int(n) * int(new) // int(orig))


def _fold(h, ph, xv):
    """h [new][K], ph [outputs], xv [K][outputs] -> [outputs]"""
    acc = None
    for k in range(h.shape[1]):
        p = h[ph, k] * xv[k]
        assert p.dtype == F32
        acc = p if acc is None else acc + p
    return acc


def fold(h, orig, new, w, x, n_out):
    """one row and channel: x float32 [len] -> float32 [n_out]"""
    x = np.asarray(x, F32)
    n = np.arange(n_out, dtype=np.int64)
    base, ph = n * orig // new, n * orig % new
    L = len(x)
    xp = np.concatenate([x, np.zeros(1, F32)])                          # index L: the +0.0 outside [0, len)
    idx = base[None, :] - w + np.arange(h.shape[1], dtype=np.int64)[:, None]
    return _fold(h, ph, xp[np.where((idx >= 0) & (idx < L), idx, L)])


def fold_window(h, orig, new, w, row, a, b):
    """The window form of fold for a row that is +0.0 outside a few windows (tests/sparse_rows.py: one line, row.n its len):
    outputs [a, b) of the out_len(len), +0.0 outside [0, len) at the row's true ends"""
    L = row.n
    assert 0 <= a <= b <= out_len(L, orig, new) and b * max(orig, new) < 1 << 62
    n = np.arange(a, b, dtype=np.int64)
    base, ph = n * orig // new, n * orig % new
    idx = base[None, :] - w + np.arange(h.shape[1], dtype=np.int64)[:, None]
    inside = (idx >= 0) & (idx < L)
    return _fold(h, ph, np.where(inside, row.gather(np.where(inside, idx, 0))[0], F32(0.0)).astype(F32))
