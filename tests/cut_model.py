"""The rule of include/lewton_amd.h ("cutting rows into segment rows") in numpy: bit copies of [start, end) of every line of a job's
row, zero bits behind them up to fill_to, nothing else written.  Values travel as unsigned integers of the element's size."""
import numpy as np

UINT = {2: np.uint16, 4: np.uint32}
SENT = {2: 0x7EAD, 4: 0x7FC0DEAD}       # the destination's sentinel: a NaN with a payload as f32
SENT_SRC = {2: 0x5BCD, 4: 0x7FC00ABC}   # ... and the source's at and beyond each length


def source(n, C, F, cap, elem, seed):
    """[len(n)][C][F][cap] of random bit patterns (NaNs and infinities among them), the source's sentinel at and beyond each length"""
    rng = np.random.default_rng(seed)
    x = np.full((len(n), C, F, cap), SENT_SRC[elem], UINT[elem])
    for r, T in enumerate(n):
        x[r, :, :, :T] = rng.integers(0, 1 << (8 * elem), (C, F, T), dtype=np.uint64).astype(UINT[elem])
    return x


def rows(src, jobs, fill_to, out):
    """lw_cut_rows on the host: src [R][C][F][cap] and out [n][C][F][out_cap] of one unsigned type; out is the sentinel-filled
    destination, returned written"""
    out = out.copy()
    for i, (row, start, end) in enumerate(np.asarray(jobs, np.uint64).reshape(-1, 3).tolist()):
        ln = end - start
        out[i, :, :, :ln] = src[row, :, :, start:end]
        out[i, :, :, ln:max(ln, int(fill_to[i]) if fill_to is not None else 0)] = 0
    return out


def same(got, want, what="cut"):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        raise AssertionError("%s: %d elements differ, first at %r: got %#x, want %#x" % (
            what, len(bad), tuple(bad[0]), int(got[tuple(bad[0])]), int(want[tuple(bad[0])])))
