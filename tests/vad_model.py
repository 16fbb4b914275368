"""The model of lw_vad_rows (include/lewton_amd.h, "energy voice-activity decisions of feature rows") for the CPU and the GPU suite,
independent of the kernel source: the line's sum from tests/norm_model.py's chunk_triples and fold restricted to s1 (so the two
contracts are tied), rules 1 and 3 in numpy float32 scalars (numpy's * / + on float32 are single correctly rounded IEEE operations,
nothing fused), the windows in integers.  tree_sum restates the summation order plainly; kaldi restates voice-activity-detection.cc
(a sequential double sum, the same f32 steps, two loops) for the comparison with Kaldi."""
import numpy as np

import norm_model as NM

F32, F64 = np.float32, np.float64

SENT = NM.SENT                        # a NaN: what the source holds at and beyond n
SENT_F = NM.SENT_F
SENT_MASK = 0xA5                      # the mask's sentinel: what must not have been written
DEFAULT = (5.0, 0.5, 0, 0.6)          # Kaldi's defaults: energy_threshold, energy_mean_scale, frames_context, proportion_threshold
SRE = (5.5, 0.5, 2, 0.12)             # the SRE recipes' vad.conf


def line_sum(e, T):
    """S of rule 1: steps 1 and 2 of "normalising rows" over the one line, n = T (T > 0)"""
    a, b, pk = NM.chunk_triples(np.asarray(e, F32)[None, :T], T)
    return F64(NM.fold(a[0], b[0], pk[0])[0])


def tree_sum(e, T):
    """the same sum, restated plainly: chunks of 256 from frame 0, ((d0 + d1) + d2) + d3, the adjacent-pair tree, the chunk list
    folded 64 at a time, a list of one entry being that entry"""
    def tree(v):
        v = list(v)
        assert len(v) == 64
        while len(v) > 1:
            v = [v[2 * j] + v[2 * j + 1] for j in range(len(v) // 2)]
        return v[0]
    x = np.zeros(-(-T // 256) * 256, F64)
    x[:T] = np.asarray(e, F32)[:T].astype(F64)
    with np.errstate(over="ignore", invalid="ignore"):
        lst = [tree([((c[4 * i] + c[4 * i + 1]) + c[4 * i + 2]) + c[4 * i + 3] for i in range(64)]) for c in x.reshape(-1, 256)]
        while len(lst) > 1:
            lst = lst + [F64(0.0)] * (-len(lst) % 64)
            lst = [tree(lst[g:g + 64]) for g in range(0, len(lst), 64)]
    return F64(lst[0])


def threshold(S, T, energy_threshold, energy_mean_scale):
    """rule 1 behind the sum: four f32 operations"""
    thr, scale = F32(energy_threshold), F32(energy_mean_scale)
    if scale == 0 or T == 0:
        return thr
    assert T < 1 << 53                                                  # exact as a double: ONE rounding to float32
    with np.errstate(all="ignore"):
        sf = F32(F64(S))
        p = scale * sf
        q = p / F32(float(T))
        return F32(thr + q)


def voiced(num, den, proportion_threshold):
    """rule 3: ONE rounded f32 multiply"""
    return bool(F32(num) >= F32(den) * F32(proportion_threshold))


def window(t, T, ctx):
    """(lo, hi) of frame t, in Python integers"""
    return max(0, t - ctx), min(T, t + ctx + 1)


def decide(e, T, thr, ctx, prop):
    """rules 2 and 3 for one line: uint8 [T]"""
    e = np.asarray(e, F32)[:T]
    with np.errstate(invalid="ignore"):
        d = (e > F32(thr)).astype(np.int64)                            # a NaN on either side: 0
    c = np.concatenate([[0], np.cumsum(d)])
    t = np.arange(T, dtype=np.int64)
    lo, hi = np.maximum(0, t - ctx), np.minimum(T, t + ctx + 1)
    num, den = c[hi] - c[lo], hi - lo
    return (num.astype(F32) >= den.astype(F32) * F32(prop)).astype(np.uint8)


def decide_plain(e, T, thr, ctx, prop):
    """the same, frame by frame with window() and voiced()"""
    e = np.asarray(e, F32)
    with np.errstate(invalid="ignore"):
        d = [bool(e[t] > F32(thr)) for t in range(T)]
    out = np.zeros(T, np.uint8)
    for t in range(T):
        lo, hi = window(t, T, ctx)
        out[t] = voiced(sum(d[lo:hi]), hi - lo, prop)
    return out


def line(e, T, cfg):
    """(mask uint8 [T], thr float32) of one line under cfg = (energy_threshold, energy_mean_scale, frames_context, proportion_threshold)"""
    thr0, scale, ctx, prop = cfg
    thr = threshold(line_sum(e, T) if T and F32(scale) != 0 else 0.0, T, thr0, scale)
    return decide(e, T, thr, ctx, prop), thr


def rows(x, n, fill_to, dst, cfg, line_i=0):
    """x float32 [rows][ch][F][cap]; dst: the mask before the call, uint8 [rows][ch][cap].  Returns (the mask after the call, the
    thresholds float32 [rows][ch])"""
    x = np.asarray(x, F32)
    out = np.array(dst, np.uint8, copy=True)
    R, C = x.shape[:2]
    thr = np.zeros((R, C), F32)
    for r in range(R):
        T = int(n[r])
        end = max(T, int(fill_to[r]) if fill_to is not None else 0)
        for c in range(C):
            out[r, c, :T], thr[r, c] = line(x[r, c, line_i], T, cfg)
            out[r, c, T:end] = 0
    return out, thr


def kaldi(e, T, cfg):
    """voice-activity-detection.cc restated: (mask uint8 [T], the float32 threshold).  The sum is sequential, in double, and leaves
    as a float; scale * sum / T + threshold are float operations; the window is two loops and int >= int * float"""
    thr0, scale, ctx, prop = cfg
    e = np.asarray(e, F32)
    energy_threshold = F32(thr0)
    if F32(scale) != 0 and T:
        s = 0.0
        for t in range(T):
            s += float(e[t])
        energy_threshold = F32(energy_threshold + F32(scale) * F32(s) / F32(float(T)))
    out = np.zeros(T, np.uint8)
    for t in range(T):
        num_count = den_count = 0
        for t2 in range(t - ctx, t + ctx + 1):
            if 0 <= t2 < T:
                den_count += 1
                if e[t2] > energy_threshold:
                    num_count += 1
        out[t] = F32(num_count) >= F32(den_count) * F32(prop)
    return out, energy_threshold


def same_thr(got, want):
    """bits; a NaN threshold equals any NaN"""
    g, w = (np.ascontiguousarray(v, F32) for v in (got, want))
    assert g.shape == w.shape, (g.shape, w.shape)
    same = (g.view(np.uint32) == w.view(np.uint32)) | (np.isnan(g) & np.isnan(w))
    assert same.all(), (int((~same).sum()), np.argwhere(~same)[:4].tolist(), g[~same][:4].tolist(), w[~same][:4].tolist())


def same_mask(got, want):
    """every byte of the exact-size mask, the sentinel beyond each span included"""
    g, w = (np.ascontiguousarray(v).view(np.uint8) for v in (got, want))
    assert g.shape == w.shape, (g.shape, w.shape)
    same = g == w
    assert same.all(), (int((~same).sum()), np.argwhere(~same)[:4].tolist(), g[~same][:4].tolist(), w[~same][:4].tolist())


ODD = np.array([0.0, -0.0, np.inf, -np.inf, np.nan], F32)


def source(n, ch, F, cap, seed, line_i=0, special=False, others_nan=False):
    """float32 [rows][ch][F][cap]: the energy line N(12, 3) with a level of its own per row and channel, the other lines noise (or
    all NaN); special: +-0, +-inf and NaN strewn into the energy line (row 0 none, then one kind more per row, cyclically); the
    sentinel NaN at and beyond each n"""
    rng = np.random.default_rng(seed)
    x = np.full((len(n), ch, F, cap), SENT_F, F32)
    for r, k in enumerate(n):
        v = (rng.standard_normal((ch, F, k)) * 3.0 - 12.0).astype(F32)
        if others_nan:
            v[:] = np.nan
        e = (rng.standard_normal((ch, k)) * 3.0 + 12.0 + rng.uniform(-2, 2, (ch, 1))).astype(F32)
        if special and r % (len(ODD) + 1):
            pick = rng.random((ch, k)) < 0.05
            e[pick] = ODD[rng.integers(0, r % (len(ODD) + 1), int(pick.sum()))]
        v[:, line_i] = e
        x[r, :, :, :k] = v
    return x


def exact_line(T, seed):
    """energies that are multiples of 2^-6 in [-8, 24): every sum of up to 4096 of them is exact in double in any order, and in
    float32 too (below 2^17 in steps of 2^-6: 23 bits)"""
    rng = np.random.default_rng(seed)
    return (rng.integers(-8 * 64, 24 * 64, T).astype(F64) / 64.0).astype(F32)
