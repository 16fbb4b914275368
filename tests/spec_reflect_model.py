"""Reflect padding of the spectral frames (include/lewton_amd.h, "spectral frames of rows", reflect) for the CPU and the GPU suite:
the centred frames of a row under LW_SPEC_PAD_REFLECT are the uncentred frames (tests/spec_model.py) of the row padded by numpy."""
import numpy as np

import spec_model as M


def min_len(n_fft):
    """the shortest row one reflection serves"""
    return n_fft - n_fft // 2 + 1


def index(i, n):
    """where x[i] of a row of n samples is read, in Python integers"""
    if i < 0:
        i = -i
    if i >= n:
        i = 2 * (n - 1) - i
    assert 0 <= i < n
    return i


def frame_matrix(x, n_fft, win_length, hop):
    """float32 [1 + len // hop][win_length]: numpy pads n_fft // 2 in front and n_fft - n_fft // 2 behind -- for even n_fft what
    torch.stft pads, for odd n_fft one sample more, which the frame at len / hop needs when hop divides len"""
    x = np.asarray(x, np.float32)
    if len(x) == 0:
        return np.zeros((0, win_length), np.float32)
    assert len(x) >= min_len(n_fft)
    pad = n_fft // 2
    X = M.frame_matrix(np.pad(x, (pad, n_fft - pad), "reflect"), n_fft, win_length, hop, False)
    assert len(X) == 1 + len(x) // hop
    return X


def frame_matrix_window(row, a, b, n_fft, win_length, hop):
    """The window form of frame_matrix for a row that is +0.0 outside a few windows (tests/sparse_rows.py: one line, row.n its
    len): frames [a, b) of the 1 + len // hop, every index reflected at the row's true ends as index() does"""
    L = row.n
    assert L >= min_len(n_fft) and 0 <= a <= b <= 1 + L // hop
    o = (n_fft - win_length) // 2
    i = np.arange(a, b, dtype=np.int64)[:, None] * hop - n_fft // 2 + o + np.arange(win_length, dtype=np.int64)[None, :]
    i = np.where(i < 0, -i, i)
    i = np.where(i >= L, 2 * (L - 1) - i, i)
    return row.gather(i)[0]
