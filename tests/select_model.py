"""The model of lw_select_rows (include/lewton_amd.h, "frame decisions and frame selection") for the CPU and the GPU suite,
independent of the kernel source: numpy's boolean indexing of every line, on the bit patterns."""
import numpy as np

F32 = np.float32

SENT = 0x7FC0DEAD                     # a NaN: the destination's sentinel, and what the source holds at and beyond n
SENT_F = np.array(SENT, np.uint32).view(F32)
SENT_MASK = 0xA5                      # what the mask holds at and beyond n: a kept frame, were it read


def rows(x, mask, n, fill_to, dst):
    """x float32 [rows][ch][F][cap], mask uint8 [rows][ch][cap]; dst: the destination before the call, of x's shape.  Returns (the
    destination after the call, K as int64 [rows][ch])"""
    xb = np.ascontiguousarray(x, F32).view(np.uint32)
    out = np.array(dst, F32, copy=True)
    ob = out.view(np.uint32)
    R, C = xb.shape[:2]
    counts = np.zeros((R, C), np.int64)
    for r in range(R):
        T = int(n[r])
        end = max(T, int(fill_to[r]) if fill_to is not None else 0)
        for c in range(C):
            keep = np.flatnonzero(np.asarray(mask[r, c, :T]) != 0)
            K = len(keep)
            counts[r, c] = K
            ob[r, c, :, :K] = xb[r, c][:, keep]
            ob[r, c, :, K:end] = 0
    return out, counts


def window_rows(row, mask, a, b, T, fill_end, before):
    """The window form of rows() for ONE row and channel whose lines are +0.0 outside a few windows and whose mask is constant
    outside a few (tests/sparse_rows.py: row a SparseRow of the F lines, mask a SparseMask, both of at least T frames): positions
    [a, b) of every destination line after the call, from `before` float32 [F][b - a], and K.  The places of the kept frames come
    from the mask's stretches in Python integers; the values travel as bit patterns"""
    assert 0 <= a <= b and T <= fill_end
    out = np.array(before, F32, copy=True)
    ob = out.view(np.uint32)
    m = mask.clipped(T)
    K = m.count()
    hi = min(b, K)
    if hi > a:
        at = m.places(a, hi)
        assert len(at) == hi - a and (len(at) < 2 or (np.diff(at) > 0).all())
        ob[:, :hi - a] = row.clipped(T).gather(at).view(np.uint32)
    f0, f1 = min(max(a, K), fill_end), min(b, fill_end)
    if f1 > f0:
        ob[:, f0 - a:f1 - a] = 0
    return out, K


def same_bits(got, want):
    """every bit, NaN payloads included: the pass copies"""
    g, w = (np.ascontiguousarray(v, F32).view(np.uint32) for v in (got, want))
    assert g.shape == w.shape, (g.shape, w.shape)
    same = g == w
    assert same.all(), (int((~same).sum()), np.argwhere(~same)[:4].tolist(), g[~same][:4].tolist(), w[~same][:4].tolist())


def source(n, ch, F, cap, seed):
    """float32 [rows][ch][F][cap]: noise with NaNs of several payloads, infinities, zeros of both signs and subnormals strewn in; the
    sentinel NaN at and beyond each n"""
    rng = np.random.default_rng(seed)
    x = np.full((len(n), ch, F, cap), SENT_F, F32)
    odd = np.array([0, 0x80000000, 1, 0x80000001, 0x7F800000, 0xFF800000, 0x7FC00001, 0xFFC12345, 0x7F800001], np.uint32).view(F32)
    for r, k in enumerate(n):
        v = (rng.standard_normal((ch, F, k)) * 3.0 - 12.0).astype(F32)
        pick = rng.random((ch, F, k)) < 0.1
        v[pick] = odd[rng.integers(0, len(odd), int(pick.sum()))]
        x[r, :, :, :k] = v
    return x


KINDS = ["zero", "one", "alternating", "random", "last", "bytes"]


def mask(kind, n, ch, cap, seed):
    """uint8 [rows][ch][cap]: nothing kept, everything, every other frame, half at random, only the last frame, or random BYTES (any
    non-zero value keeps); SENT_MASK at and beyond each n"""
    rng = np.random.default_rng(seed)
    m = np.full((len(n), ch, cap), SENT_MASK, np.uint8)
    for r, k in enumerate(n):
        if kind == "zero":
            v = np.zeros((ch, k), np.uint8)
        elif kind == "one":
            v = np.ones((ch, k), np.uint8)
        elif kind == "alternating":
            v = np.tile((np.arange(k) % 2).astype(np.uint8), (ch, 1))
            v[1:] ^= 1
        elif kind == "random":
            v = (rng.random((ch, k)) < 0.5).astype(np.uint8)
        elif kind == "last":
            v = np.zeros((ch, k), np.uint8)
            v[:, k - 1:] = 1
        else:
            v = rng.integers(0, 256, (ch, k)).astype(np.uint8) * (rng.random((ch, k)) < 0.7)
        m[r, :, :k] = v
    return m
