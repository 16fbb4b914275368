"""The model of lw_specaug_rows (include/lewton_amd.h, "masking feature rows") for the CPU and the GPU suite, independent of the kernel
source: Philox4x32-10 and the two bounded draws in Python integers, the span rule in Python integers, the masking in numpy on the
BITS of the float32 elements (uint32 views: fill's own bits, NaN payloads and -0.0 included).  philox_np is the same generator on
numpy uint64 arrays, for the sweeps that draw 100 000 spans; the tests hold it against the integer one."""
from fractions import Fraction

import numpy as np

F32, U32, U64 = np.float32, np.uint32, np.uint64
M32, M64 = (1 << 32) - 1, (1 << 64) - 1
PHILOX_M0, PHILOX_M1 = 0xD2511F53, 0xCD9E8D57          # on counter word 0, on counter word 2
PHILOX_W0, PHILOX_W1 = 0x9E3779B9, 0xBB67AE85          # added to the key before every round but the first
MAX_MASKS, MAX_WIDTH = 32, 65535                      # LW_SPECAUG_MAX_MASKS, LW_SPECAUG_MAX_WIDTH
SENT = 0x7FC0DEAD                                     # a NaN with a payload: what must not have been written, or read
SENT_DST = 0x7FC00ABC                                 # another: what a destination holds before a call out of place
TIME, FREQ = 0, 1


def philox(counter, key):
    """Philox4x32-10: four counter words and two key words -> four words"""
    c0, c1, c2, c3 = (int(v) & M32 for v in counter)
    k0, k1 = (int(v) & M32 for v in key)
    for r in range(10):
        if r:
            k0, k1 = (k0 + PHILOX_W0) & M32, (k1 + PHILOX_W1) & M32
        p0, p1 = PHILOX_M0 * c0, PHILOX_M1 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & M32, (p0 >> 32) ^ c3 ^ k1, p0 & M32
    return c0, c1, c2, c3


def philox_np(c0, c1, c2, c3, k0, k1):
    """the same on uint64 arrays that hold 32-bit words (the products stay below 2^64)"""
    c0, c1, c2, c3, k0, k1 = (np.asarray(v, U64) & U64(M32) for v in np.broadcast_arrays(c0, c1, c2, c3, k0, k1))
    m = U64(M32)
    for r in range(10):
        if r:
            k0, k1 = (k0 + U64(PHILOX_W0)) & m, (k1 + U64(PHILOX_W1)) & m
        p0, p1 = U64(PHILOX_M0) * c0, U64(PHILOX_M1) * c2
        c0, c1, c2, c3 = (p1 >> U64(32)) ^ c1 ^ k0, p1 & m, (p0 >> U64(32)) ^ c3 ^ k1, p0 & m
    return c0, c1, c2, c3


def below32(x, n):
    return (x * n) >> 32


def below64(x, n):
    return (x * n) >> 64


class Params:
    """lw_specaug_params; ratio: None, or (ratio_num, ratio_den)"""

    def __init__(self, seed=0, num_t=2, min_t=0, max_t=50, ratio=None, num_f=2, min_f=0, max_f=10, per_channel=False, fill_bits=0):
        self.seed, self.num_t, self.min_t, self.max_t = int(seed), num_t, min_t, max_t
        self.ratio_num, self.ratio_den = ratio if ratio else (0, 0)
        self.num_f, self.min_f, self.max_f, self.per_channel, self.fill_bits = num_f, min_f, max_f, bool(per_channel), int(fill_bits)

    @property
    def masks(self):
        return self.num_t + self.num_f


def ratio_of(p):
    """the constructor's p as (ratio_num, ratio_den); 1.0 is no ratio"""
    if p == 1.0:
        return (0, 0)
    f = Fraction(p).limit_denominator(65535)
    return (f.numerator, f.denominator)


def widths(P, d, n):
    """(lo, W) of a mask of kind d over n"""
    W = min(P.max_t if d == TIME else P.max_f, n)
    if d == TIME and P.ratio_den:
        W = min(W, (n // P.ratio_den) * P.ratio_num + ((n % P.ratio_den) * P.ratio_num) // P.ratio_den)
    return min(P.min_t if d == TIME else P.min_f, W), W


def span(P, id_, g, d, k, n):
    """(start, end) of mask k of kind d of group g of utterance id_ over n frames or bins"""
    x = philox((id_ & M32, id_ >> 32, k | g << 16, d), (P.seed & M32, P.seed >> 32))
    lo, W = widths(P, d, n)
    w = lo + below32(x[0], W - lo + 1)
    start = below64(x[1] << 32 | x[2], n - w + 1)
    return start, start + w


def plan(P, id_, g, T, F):
    """[num_t + num_f] (start, end), time masks first: what lw_specaug_plan and d_spans hold"""
    return [span(P, id_, g, TIME, k, T) for k in range(P.num_t)] + [span(P, id_, g, FREQ, k, F) for k in range(P.num_f)]


def masked(P, id_, g, T, F):
    """bool [F][T]: the elements of one group's lines that receive fill"""
    m = np.zeros((F, T), bool)
    for k, (a, b) in enumerate(plan(P, id_, g, T, F)):
        if k < P.num_t:
            m[:, a:b] = True
        else:
            m[a:b, :] = True
    return m


def rows(P, x_bits, n, fill_to, ids, dst_bits):
    """x_bits uint32 [rows][ch][F][cap]: the source's bits; dst_bits: the destination before the call (the source itself for the
    call in place).  Returns (the destination after the call, the spans int64 [rows][G][masks][2])"""
    x, out = np.asarray(x_bits, U32), np.array(dst_bits, U32, copy=True)
    R, C, F, cap = x.shape
    G = C if P.per_channel else 1
    spans = np.zeros((R, G, P.masks, 2), np.int64)
    for r in range(R):
        T, id_ = int(n[r]), int(ids[r]) if ids is not None else r
        end = max(T, int(fill_to[r]) if fill_to is not None else 0)
        for g in range(G):
            spans[r, g] = np.array(plan(P, id_, g, T, F), np.int64).reshape(P.masks, 2)
        for c in range(C):
            m = masked(P, id_, c if P.per_channel else 0, T, F)
            out[r, c, :, :T] = np.where(m, U32(P.fill_bits), x[r, c, :, :T])
            out[r, c, :, T:end] = 0
    return out, spans


def same_bits(got, want):
    g, w = (np.ascontiguousarray(v).view(U32) for v in (got, want))
    assert g.shape == w.shape, (g.shape, w.shape)
    same = g == w
    assert same.all(), (int((~same).sum()), np.argwhere(~same)[:4].tolist(), [hex(v) for v in g[~same][:4]], [hex(v) for v in w[~same][:4]])


def bits_of(v):
    with np.errstate(over="ignore"):
        return int(np.array(v, F32).view(U32))


ODD_BITS = np.array([0x7FC12345, 0xFFC00001, 0x7F800000, 0xFF800000, 0x00000001, 0x807FFFFF, 0x80000000, 0x7F812345], U32)


def source(n, ch, F, cap, seed, special=False):
    """uint32 [rows][ch][F][cap]: the bits of N(0, 1) float32 features, the sentinel NaN at and beyond each n; special: NaNs with
    payloads, infinities, subnormals and -0.0 strewn in"""
    rng = np.random.default_rng(seed)
    x = np.full((len(n), ch, F, cap), SENT, U32)
    for r, k in enumerate(n):
        v = rng.standard_normal((ch, F, k)).astype(F32).view(U32)
        if special:
            pick = rng.random((ch, F, k)) < 0.1
            v[pick] = ODD_BITS[rng.integers(0, len(ODD_BITS), int(pick.sum()))]
        x[r, :, :, :k] = v
    return x
