"""The model of lw_norm_rows (include/lewton_amd.h, "normalising rows") for the CPU and the GPU suite, independent of the kernel
source: steps 1 to 4 in numpy float64 exactly as the contract writes them (numpy's elementwise + - * / and sqrt are single
correctly rounded IEEE operations, nothing fused), the pair trees as v[0::2] + v[1::2], the peak by uint32 views, the final cast to
float32."""
import numpy as np

NONE, STD, RMS, PEAK = 0, 1, 2, 3
ROW, CHANNEL, LINE = 0, 1, 2
SCALES = {None: NONE, "none": NONE, "std": STD, "rms": RMS, "peak": PEAK}
SCOPES = {"row": ROW, "channel": CHANNEL, "line": LINE}
F32, F64 = np.float32, np.float64

SENT = 0x7FC0DEAD                     # a NaN: the destination's sentinel, and what the source holds at and beyond n
SENT_F = np.array(SENT, np.uint32).view(F32)


def _tree(v):
    """[groups][64] -> [groups]: t[j] = t[2j] + t[2j + 1], six levels"""
    assert v.shape[-1] == 64
    with np.errstate(over="ignore", invalid="ignore"):
        for _ in range(6):
            v = v[..., 0::2] + v[..., 1::2]
    return v[..., 0]


def _tree_max(v):
    for _ in range(6):
        v = np.maximum(v[..., 0::2], v[..., 1::2])
    return v[..., 0]


def chunk_triples(lines, n):
    """step 1.  lines: float32 [..., >= n]; returns (a, b, pk) of shape [..., C], pk as uint32 bit patterns of |x|"""
    lines = np.asarray(lines, F32)
    C = -(-n // 256)
    lead = lines.shape[:-1]
    x = np.zeros(lead + (C * 256,), F32)
    x[..., :n] = lines[..., :n]
    d = x.astype(F64).reshape(lead + (C, 64, 4))
    with np.errstate(over="ignore", invalid="ignore"):
        a = ((d[..., 0] + d[..., 1]) + d[..., 2]) + d[..., 3]
        b = ((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]) + d[..., 3] * d[..., 3]
    pk = (x.view(np.uint32) & np.uint32(0x7FFFFFFF)).reshape(lead + (C, 256)).max(axis=-1) if C else np.zeros(lead + (0,), np.uint32)
    return _tree(a), _tree(b), pk


def fold(a, b, pk):
    """step 2 for one scope's list (1-D arrays in line-major order) -> (S1, S2, P as a float32)"""
    a, b, pk = np.asarray(a, F64).ravel(), np.asarray(b, F64).ravel(), np.asarray(pk, np.uint32).ravel()
    assert len(a) == len(b) == len(pk) and len(a)
    while len(a) > 1:
        g = -(-len(a) // 64)
        pad = g * 64 - len(a)
        a = _tree(np.concatenate([a, np.zeros(pad, F64)]).reshape(g, 64))
        b = _tree(np.concatenate([b, np.zeros(pad, F64)]).reshape(g, 64))
        pk = _tree_max(np.concatenate([pk, np.zeros(pad, np.uint32)]).reshape(g, 64))
    return a[0], b[0], pk.view(F32)[0]


def scalars(center, scale, eps, target, S1, S2, P, N):
    """step 3, elementwise over arrays (N > 0 everywhere) -> (m, g) float64"""
    S1, S2, N = np.asarray(S1, F64), np.asarray(S2, F64), np.asarray(N, np.uint64).astype(F64)
    P = np.asarray(P, F32)
    with np.errstate(all="ignore"):
        mu = S1 / N
        q = S2 / N
        v = q - mu * mu
        v = np.where(v > 0, v, 0.0)
        m = mu if center else np.zeros_like(mu)
        if scale == NONE:
            g = np.ones_like(mu)
        elif scale == STD:
            g = 1.0 / np.sqrt(v + F64(eps))
        elif scale == RMS:
            g = F64(target) / np.sqrt(q + F64(eps))
        else:
            g = np.where(P == 0, 1.0, F64(target) / P.astype(F64))
    return m, g


def apply(x, m, g):
    """step 4"""
    with np.errstate(all="ignore"):
        return ((np.asarray(x, F32).astype(F64) - m) * g).astype(F32)


def scope_stats(part, n, center, scale, eps, target):
    """(m, g) of one scope: part float32 [lines][>= n]"""
    if n == 0:
        return 0.0, 1.0
    a, b, pk = chunk_triples(part, n)
    S1, S2, P = fold(a, b, pk)
    m, g = scalars(center, scale, eps, target, S1, S2, P, part.shape[0] * n)
    return float(m), float(g)


def rows(x, n, fill_to, dst, center=1, scale=STD, scope=ROW, eps=1e-7, target=1.0):
    """x float32 [rows][ch][F][cap]; dst: the destination before the call (x itself in place).  Returns (the destination after the
    call, the stats as float64 [rows][2], [rows][ch][2] or [rows][ch][F][2])"""
    x = np.asarray(x, F32)
    out = np.array(dst, F32, copy=True)
    R, C, F, cap = x.shape
    stats = np.zeros(((R, 1, 1), (R, C, 1), (R, C, F))[scope] + (2,), F64)
    for r in range(R):
        k = int(n[r])
        end = max(k, int(fill_to[r]) if fill_to is not None else 0)
        if scope == LINE and k:                                    # all lines of the row at once
            a, b, pk = chunk_triples(x[r], k)
            if a.shape[-1] == 1:
                S1, S2, P = a[..., 0], b[..., 0], pk[..., 0].view(F32)
            else:
                f = [fold(a[c, l], b[c, l], pk[c, l]) for c in range(C) for l in range(F)]
                S1, S2, P = (np.array([t[i] for t in f]).reshape(C, F) for i in range(3))
            m, g = scalars(center, scale, eps, target, S1, S2, P, np.full((C, F), k, np.uint64))
            stats[r, :, :, 0], stats[r, :, :, 1] = m, g
        else:
            for c in range(stats.shape[1]):
                for l in range(stats.shape[2]):
                    part = x[r].reshape(1, C * F, cap) if scope == ROW else x[r, c:c + 1] if scope == CHANNEL else x[r, c, l:l + 1][None]
                    stats[r, c, l] = scope_stats(part.reshape(-1, cap), k, center, scale, eps, target)
        for c in range(C):
            for l in range(F):
                m, g = stats[r, c if scope != ROW else 0, l if scope == LINE else 0]
                out[r, c, l, :k] = apply(x[r, c, l, :k], m, g)
                out[r, c, l, k:end] = 0.0
    return out, stats.reshape(((R, 2), (R, C, 2), (R, C, F, 2))[scope])


def same_bits(got, want, sentinel=None):
    """bits; a NaN result equals any NaN (which NaN it is, is outside the contract) except the destination's sentinel, which marks
    what must not have been written"""
    dt = np.asarray(want).dtype
    u = np.uint32 if dt == F32 else np.uint64
    g, w = (np.ascontiguousarray(v, dt) for v in (got, want))
    assert g.shape == w.shape, (g.shape, w.shape)
    gb, wb = g.view(u), w.view(u)
    nan = np.isnan(g) & np.isnan(w)
    if sentinel is not None:
        nan &= (gb != sentinel) & (wb != sentinel)
    same = (gb == wb) | nan
    assert same.all(), (int((~same).sum()), np.argwhere(~same)[:4].tolist(), g[~same][:4].tolist(), w[~same][:4].tolist())


def source(n, ch, F, cap, seed, offset=0.0, special=False):
    """float32 [rows][ch][F][cap]: noise of differing level per line around `offset`; special: NaN, +-inf, +-0, subnormals and
    FLT_MAX strewn in per row (row 0 none, then one kind more per row, cyclically); the sentinel NaN at and beyond each n"""
    rng = np.random.default_rng(seed)
    x = np.full((len(n), ch, F, cap), SENT_F, F32)
    odd = np.array([0.0, -0.0, 1e-42, -1.4e-45, 3.4028234663852886e38, np.inf, -np.inf, np.nan], F32)
    for r, k in enumerate(n):
        v = (rng.standard_normal((ch, F, k)) * 10.0 ** rng.uniform(-3, 1, (ch, F, 1)) + offset).astype(F32)
        if special and r % (len(odd) + 1):
            pick = rng.random((ch, F, k)) < 0.2
            v[pick] = odd[rng.integers(0, r % (len(odd) + 1), int(pick.sum()))]
        x[r, :, :, :k] = v
    return x


def exact_sums(values):
    """(S1, S2, P) of float32 values that are integers / 1024 of magnitude at most 1024, in Python integers: both sums are
    exactly representable in float64 and every partial sum of any bracketing is too, so the contract's tree gives these bits
    whatever its shape.  Zeros add nothing: a row that is +0.0 outside its windows has the sums of its windows"""
    v = np.asarray(values, F32).ravel()
    k = v.astype(F64) * 1024.0
    assert np.array_equal(k, np.rint(k)) and (np.abs(k) <= 1 << 20).all(), "values must be integers / 1024"
    ints = [int(i) for i in k]
    s1, s2 = sum(ints), sum(i * i for i in ints)
    assert abs(s1) < 1 << 53 and s2 < 1 << 53
    P = (v.view(np.uint32) & np.uint32(0x7FFFFFFF)).max().view(F32) if len(v) else F32(0)
    return float(s1) / 1024.0, float(s2) / float(1 << 20), P


def window(row, C, F, a, b, n, fill_end, before, center=1, scale=STD, scope=ROW, eps=1e-7, target=1.0, scalars_of=None):
    """The window form of rows() for ONE row that is +0.0 outside a few windows (tests/sparse_rows.py: row has C * F lines,
    channel-major, of at least n elements, its values integers / 1024): positions [a, b) of every line of the destination after
    the call, from `before` float32 [C][F][b - a].  S1, S2 and P are exact_sums of the windows, N the scope's lines times n.
    scalars_of(S1, S2, P, N) -> (m, g): step 3 (None: scalars() above).  Returns (after, stats float64 [], [C] or [C][F] + [2])"""
    assert row.lines == C * F and 0 <= a <= b and n <= fill_end
    src = row.clipped(n)
    vals = src.values().reshape(C, F, -1)
    stats = np.zeros((C, F, 2), F64)
    groups = [[(c, l) for c in range(C) for l in range(F)]] if scope == ROW else \
        [[(c, l) for l in range(F)] for c in range(C)] if scope == CHANNEL else [[(c, l)] for c in range(C) for l in range(F)]
    for grp in groups:
        if n == 0:
            m, g = 0.0, 1.0
        else:
            S1, S2, P = exact_sums(np.concatenate([vals[c, l] for c, l in grp]))
            if scalars_of is None:
                m, g = (float(v) for v in scalars(center, scale, eps, target, S1, S2, P, len(grp) * n))
            else:
                m, g = scalars_of(S1, S2, P, len(grp) * n)
        for c, l in grp:
            stats[c, l] = m, g
    out = np.array(before, F32, copy=True).reshape(C, F, b - a)
    lo, hi = min(a, n), min(b, n)
    x = src.take(lo, hi).reshape(C, F, hi - lo)
    for c in range(C):
        for l in range(F):
            out[c, l, lo - a:hi - a] = apply(x[c, l], stats[c, l, 0], stats[c, l, 1])
    f0, f1 = min(max(a, n), fill_end), min(b, fill_end)
    if f1 > f0:
        out[:, :, f0 - a:f1 - a] = 0.0
    return out, (stats[0, 0] if scope == ROW else stats[:, 0] if scope == CHANNEL else stats)
