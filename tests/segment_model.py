"""The rule of include/lewton_amd.h ("segments of a frame mask") in numpy, twice: pointwise, as the header states it, and
sequentially on run lists (pad and clamp the intervals, merge where the gap is < min_off, delete where the length is < min_on: the
way pyannote's Timeline.support reads).  tests/test_segment_model.py holds the two against each other.  Integers only."""
import numpy as np

SENT_MASK = 0xA5                      # what a test's masks hold where nothing may be read or written
SENT_SPAN = 0x7E7E7E7E7E7E7E7E        # ... and its spans and counts


def runs(o):
    """the maximal runs of a boolean line as a list of (a, b), b exclusive"""
    o = np.asarray(o, bool)
    d = np.diff(np.concatenate([[0], o.astype(np.int8), [0]]))
    return list(zip(np.flatnonzero(d == 1).tolist(), np.flatnonzero(d == -1).tolist()))


def pointwise(m, pad_onset, pad_offset, min_off, min_on):
    """O of the header's rules 1 to 3 for one line m (any non-zero entry is set), frame by frame"""
    m = np.asarray(m) != 0
    T = len(m)
    if T == 0:
        return np.zeros(0, bool)
    t = np.arange(T)
    # 1. pad: some set u with t - pad_offset <= u <= t + pad_onset, u in [0, T)
    before = np.concatenate([[0], np.cumsum(m)])
    lo, hi = np.maximum(t - pad_offset, 0), np.minimum(t + pad_onset, T - 1)
    P = before[hi + 1] - before[lo] > 0
    # 2. fill: the nearest set frames a < t < b, with b - a - 1 < min_off
    a = np.maximum.accumulate(np.where(P, t, -1))                       # the last set frame at or before t
    a = np.concatenate([[-1], a[:-1]])                                  # ... strictly before
    b = np.minimum.accumulate(np.where(P, t, T)[::-1])[::-1]
    b = np.concatenate([b[1:], [T]])
    C = P | ((a >= 0) & (b < T) & (b - a - 1 < min_off))
    # 3. drop: the maximal run of C that holds t has at least min_on frames
    O = np.zeros(T, bool)
    for s, e in runs(C):
        if e - s >= min_on:
            O[s:e] = True
    return O


def literal(m, pad_onset, pad_offset, min_off, min_on):
    """the same, word for word from the header with Python loops and no arithmetic trick; for short lines"""
    m = [bool(v) for v in m]
    T = len(m)
    P = [any(m[u] for u in range(max(0, t - pad_offset), min(T - 1, t + pad_onset) + 1)) for t in range(T)]
    C = [P[t] or any(P[a] and P[b] and b - a - 1 < min_off for a in range(t) for b in range(t + 1, T)) for t in range(T)]
    O = []
    for t in range(T):
        s, e = t, t
        while C[t] and s > 0 and C[s - 1]:
            s -= 1
        while C[t] and e < T - 1 and C[e + 1]:
            e += 1
        O.append(C[t] and e - s + 1 >= min_on)
    return np.asarray(O, bool)


def sequential_runs(raw, T, pad_onset, pad_offset, min_off, min_on):
    """the segments of a line of T frames whose raw runs are `raw` (ascending, disjoint, not touching), by interval arithmetic in
    Python integers; works at any T"""
    padded = [(max(0, s - pad_onset), min(T, e + pad_offset)) for s, e in raw]
    merged = []
    for s, e in padded:
        if merged and (s - merged[-1][1] <= 0 or s - merged[-1][1] < min_off):
            merged[-1] = (merged[-1][0], max(merged[-1][1], e))
        else:
            merged.append((s, e))
    return [(s, e) for s, e in merged if e - s >= min_on]


def sequential(m, pad_onset, pad_offset, min_off, min_on):
    return sequential_runs(runs(np.asarray(m) != 0), len(m), pad_onset, pad_offset, min_off, min_on)


def rows(mask, n, fill_to, params, spans, counts, smooth):
    """lw_segment_rows on the host: mask uint8 [R][C][cap]; spans uint64 [R][C][seg_capacity][2], counts uint64 [R][C] and smooth uint8
    [R][C][cap] are the sentinel-filled destinations (None: not wanted), written as the header says and returned"""
    R, C, cap = mask.shape
    spans, counts, smooth = (None if v is None else v.copy() for v in (spans, counts, smooth))
    for r in range(R):
        T = int(n[r])
        end = max(T, int(fill_to[r]) if fill_to is not None else 0)
        for c in range(C):
            O = pointwise(mask[r, c, :T], *params)
            segs = runs(O)
            if spans is not None:
                k = min(len(segs), spans.shape[2])
                spans[r, c, :k] = np.asarray(segs[:k], np.uint64).reshape(k, 2)
            if counts is not None:
                counts[r, c] = len(segs)
            if smooth is not None:
                smooth[r, c, :T] = O
                smooth[r, c, T:end] = 0
    return spans, counts, smooth


def source(n, C, cap, seed, burst=12):
    """a mask uint8 [len(n)][C][cap] of bursts: runs and gaps in turn, of random lengths around `burst` or around 2, one gap in seven a longer
    pause, set bytes of any non-zero value, the sentinel at and beyond each length"""
    rng = np.random.default_rng(seed)
    x = np.full((len(n), C, cap), SENT_MASK, np.uint8)
    for r, T in enumerate(n):
        for c in range(C):
            line, t, on = np.zeros(T, np.uint8), 0, bool(rng.integers(2))
            while t < T:
                k = int(rng.geometric(1.0 / burst if rng.random() < 0.7 else 0.5))
                if not on and rng.random() < 0.15:
                    k += int(rng.geometric(1.0 / (6 * burst + 40)))               # a pause
                if on:
                    line[t:t + k] = rng.integers(1, 256, min(k, T - t))
                t, on = t + k, not on
            x[r, c, :T] = line
    return x


def same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        raise AssertionError("%s: %d entries differ, first at %r: got %r, want %r" % (
            what, len(bad), tuple(bad[0]), got[tuple(bad[0])], want[tuple(bad[0])]))
