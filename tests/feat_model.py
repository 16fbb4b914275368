"""The model of lw_feat_rows (include/lewton_amd.h, "finishing feature rows") for the CPU and the GPU suite, independent of the
kernel source: LOG in numpy float64 exactly as the contract writes it (numpy's elementwise * + - / are single IEEE operations,
nothing fused), steps 1, 4 and 5 in float32, the maximum in the total order in which +0.0 lies above -0.0."""
import numpy as np

NONE, LN, LOG10, DB = 0, 1, 2, 3
ROW, CHANNEL = 0, 1
LOGS = {"none": NONE, "ln": LN, "log10": LOG10, "db": DB}
RH = float.fromhex("0x1.6a09e667f3bcdp-1")
LN2 = float.fromhex("0x1.62e42fefa39efp-1")
LOG10E = float.fromhex("0x1.bcb7b1526e50ep-2")
F32 = np.float32


def log(kind, v):
    """step 2 for float32 v that step 1 can produce (positive, +inf included; anything for NONE)"""
    v = np.asarray(v, F32)
    if kind == NONE:
        return v.copy()
    inf = np.isinf(v)
    d = np.where(inf, 1.0, v.astype(np.float64))
    m, e = np.frexp(d)
    low = m < RH
    m = np.where(low, m * 2.0, m)
    e = (e - low).astype(np.float64)
    s = (m - 1.0) / (m + 1.0)
    z = s * s
    p = np.full_like(z, 1.0 / 19.0)
    for k in range(8, -1, -1):
        p = p * z + 1.0 / (2 * k + 1)
    r = e * LN2 + (s + s) * p
    if kind in (LOG10, DB):
        r = r * LOG10E
    if kind == DB:
        r = r * 10.0
    with np.errstate(over="ignore"):
        out = r.astype(F32)
    return np.where(inf, F32(np.inf), out).astype(F32)


def key(f):
    """int32 keys whose integer order is the total order of the floats"""
    i = np.ascontiguousarray(f, F32).view(np.int32)
    return np.where(i < 0, i ^ 0x7FFFFFFF, i).astype(np.int32)


def unkey(k):
    k = np.asarray(k, np.int32)
    return np.where(k < 0, k ^ 0x7FFFFFFF, k).astype(np.int32).view(F32)


def total_max(l):
    return unkey(key(l).max()).reshape(())[()]


def finish(l, M, top, add, mul):
    """steps 4 and 5, float32"""
    top, add, mul, M = F32(top), F32(add), F32(mul), F32(M)
    with np.errstate(over="ignore", invalid="ignore"):
        tt = F32(-np.inf) if np.isposinf(top) else F32(M - top)
        l = np.asarray(l, F32)
        y = np.where(l > tt, l, tt).astype(F32)
        s = (y + add).astype(F32)
        return (s * mul).astype(F32)


def rows(x, n_frames, fill_to, dst, kind=LOG10, scope=ROW, floor=1e-10, top=8.0, add=4.0, mul=0.25):
    """x float32 [rows][ch][F][cap]; dst: the destination before the call (x itself in place).  Returns (the destination after
    the call, M as float32 [rows] or [rows][ch])"""
    x = np.asarray(x, F32)
    out = np.array(dst, F32, copy=True)
    R, C = x.shape[:2]
    floor = F32(floor)
    l0 = log(kind, np.array([floor], F32))[0]
    Ms = np.zeros((R,) if scope == ROW else (R, C), F32)
    for r in range(R):
        n = int(n_frames[r])
        end = max(n, int(fill_to[r]) if fill_to is not None else 0)
        part = x[r, :, :, :n]
        with np.errstate(invalid="ignore"):
            v = np.where(part > floor, part, floor).astype(F32)
        l = log(kind, v)
        for c in range(C):
            if scope == ROW:
                M = total_max(l) if n else l0
                Ms[r] = M
            else:
                M = total_max(l[c]) if n else l0
                Ms[r, c] = M
            out[r, c, :, :n] = finish(l[c], M, top, add, mul)
            out[r, c, :, n:end] = finish(np.array([l0], F32), M, top, add, mul)[0]
    return out, Ms


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


SENT = 0x7FC0DEAD                     # a NaN: the destination's sentinel, and what the source holds beyond n_frames
SENT_F = np.array(SENT, np.uint32).view(F32)
BASE_FRAMES = [0, 1, 2, 3, 4, 5, 31, 32, 33, 36, 37]


def source(n_frames, ch, F, cap, floor, seed, inf_row=None):
    """float32 [rows][ch][F][cap]: positive values over many decades with negatives, +-0, NaN, subnormals, exactly the floor and
    FLT_MAX strewn in, +inf in row inf_row only, the sentinel NaN beyond each n_frames"""
    rng = np.random.default_rng(seed)
    x = np.full((len(n_frames), ch, F, cap), SENT_F, F32)
    odd = np.array([-1.5, 0.0, -0.0, np.nan, 1e-42, 1.4e-45, floor, 3.4028234663852886e38, 1.0, -np.inf], F32)
    for r, n in enumerate(n_frames):
        v = (10.0 ** rng.uniform(-14, 3, (ch, F, n))).astype(F32)
        pick = rng.random((ch, F, n)) < 0.3
        v[pick] = odd[rng.integers(0, len(odd), int(pick.sum()))]
        if r == inf_row and n:
            v[0, F - 1, n // 2] = np.inf
        x[r, :, :, :n] = v
    return x


def window(row, C, F, a, b, n, fill_end, before, kind=LOG10, scope=ROW, floor=1e-10, top=8.0, add=4.0, mul=0.25):
    """The window form of rows() for ONE row that is +0.0 outside a few windows (tests/sparse_rows.py: row has C * F lines,
    channel-major, of at least n elements): positions [a, b) of every line of the destination after the call, from `before`
    float32 [C][F][b - a], what they held before it.  The maximum is taken over every element of the row: the windows' values, and
    what x = +0.0 gives wherever the row has an element outside them.  Returns (after, M as float32 [] or [C])"""
    assert row.lines == C * F and 0 <= a <= b and n <= fill_end
    floor = F32(floor)
    l0 = log(kind, np.array([floor], F32))[0]
    src = row.clipped(n)

    def step12(x):
        with np.errstate(invalid="ignore"):
            return log(kind, np.where(x > floor, x, floor).astype(F32))
    l = step12(src.values()).reshape(C, F, -1)
    rest = step12(np.zeros(1, F32)) if src.covered() < n else np.zeros(0, F32)
    if n == 0:
        Ms = np.full((C,), l0, F32)
    elif scope == ROW:
        Ms = np.full((C,), total_max(np.concatenate([l.ravel(), rest])), F32)
    else:
        Ms = np.array([total_max(np.concatenate([l[c].ravel(), rest])) for c in range(C)], F32)
    out = np.array(before, F32, copy=True).reshape(C, F, b - a)
    lo, hi = min(a, n), min(b, n)
    x = src.take(lo, hi).reshape(C, F, hi - lo)
    for c in range(C):
        out[c, :, lo - a:hi - a] = finish(step12(x[c]), Ms[c], top, add, mul)
        f0, f1 = min(max(a, n), fill_end), min(b, fill_end)
        if f1 > f0:
            out[c, :, f0 - a:f1 - a] = finish(np.array([l0], F32), Ms[c], top, add, mul)[0]
    return out, (Ms[0] if scope == ROW else Ms)
