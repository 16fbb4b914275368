"""The model of lw_pack_rows (include/lewton_amd.h, "frame-major model input") for the CPU and the GPU suite, independent of the
kernel source: the frames of a row and the clamp in Python integers, the shift and the scale as np.float32 operations of their
own, bf16 by the integer rule on the bit pattern (the NaN case first), f16 by numpy's astype(np.float16) (IEEE round to nearest
even, subnormals kept).  Results are bit patterns: uint32 for f32, uint16 for bf16 and f16."""
import numpy as np

F32 = np.float32
SENT = 0x7FC0DEAD                     # a NaN: what the source holds at and beyond n, and the f32 destination's sentinel
SENT_F = np.array(SENT, np.uint32).view(F32)
SENT16 = 0x7FAD                       # a NaN in bf16 and in f16 alike: the 16-bit destinations' sentinel
SENT_MASK = 0xA5
REPLICATE, VALID = "replicate", "valid"
OUT_DTYPE = {"f32": np.uint32, "bf16": np.uint16, "f16": np.uint16}


def sentinel(dtype):
    return SENT if dtype == "f32" else SENT16


def out_frames(T, left, right, stride, edge):
    W = left + right + 1
    if edge == VALID:
        return 0 if T < W else (T - W) // stride + 1
    return -(-T // stride)


def source_frames(T, left, right, stride, edge):
    """[T_out][W] Python integers: the source frame of context position k of output frame u"""
    W = left + right + 1
    if edge == VALID:
        return [[u * stride + k for k in range(W)] for u in range(out_frames(T, left, right, stride, edge))]
    return [[min(max(u * stride - left + k, 0), T - 1) for k in range(W)] for u in range(out_frames(T, left, right, stride, edge))]


def bf16_bits(x):
    """float32 array -> uint16 bit patterns by the contract's integer rule"""
    u = np.ascontiguousarray(x, F32).view(np.uint32).astype(np.uint64)
    nan = (u & 0x7FFFFFFF) > 0x7F800000
    r = (u + 0x7FFF + ((u >> 16) & 1)) >> 16
    return np.where(nan, (u >> 16) | 0x40, r).astype(np.uint16)


def f16_bits(x):
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        return np.ascontiguousarray(x, F32).astype(np.float16).view(np.uint16)


def convert(x, dtype):
    """float32 array -> the destination's bit patterns"""
    x = np.ascontiguousarray(x, F32)
    return x.view(np.uint32).copy() if dtype == "f32" else bf16_bits(x) if dtype == "bf16" else f16_bits(x)


def frames_of(x, T, left, right, stride, edge, shift, scale, dtype):
    """x float32 [F][>= T] -> bit patterns [T_out][W * F]"""
    idx = source_frames(T, left, right, stride, edge)
    F, W = x.shape[0], left + right + 1
    if not idx:
        return np.zeros((0, W * F), OUT_DTYPE[dtype])
    v = np.ascontiguousarray(x[:, np.array(idx, np.int64)].transpose(1, 2, 0)).reshape(len(idx), W * F)   # [u][k][f]
    assert v.dtype == F32
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        if shift is not None:
            v = v + np.asarray(shift, F32)[None, :]
        if scale is not None:
            v = v * np.asarray(scale, F32)[None, :]
    assert v.dtype == F32
    return convert(v, dtype)


def rows(x, n, fill_to, dst, mask, left, right, stride, edge, dtype, shift=None, scale=None, pad=0.0):
    """x float32 [rows][ch][F][cap]; dst: the destination's bit patterns before the call, [rows][ch][out_cap][W * F]; mask: uint8
    [rows][out_cap] before the call, or None.  Returns (the destination, the mask, out_frames) after the call"""
    x = np.asarray(x, F32)
    out = np.array(dst, copy=True)
    msk = None if mask is None else np.array(mask, copy=True)
    pad_bits = convert(np.array([pad], F32), dtype)[0]
    R, C = x.shape[:2]
    t_out = []
    for r in range(R):
        T = int(n[r])
        k = out_frames(T, left, right, stride, edge)
        end = max(k, int(fill_to[r]) if fill_to is not None else 0)
        t_out.append(k)
        for c in range(C):
            if k:
                out[r, c, :k] = frames_of(x[r, c], T, left, right, stride, edge, shift, scale, dtype)
            out[r, c, k:end] = pad_bits
        if msk is not None:
            msk[r, :k] = 1
            msk[r, k:end] = 0
    return out, msk, t_out


def is_nan_bits(b, dtype):
    b = np.asarray(b)
    if dtype == "f32":
        return (b & 0x7FFFFFFF) > 0x7F800000
    if dtype == "bf16":
        return (b & 0x7FFF) > 0x7F80
    return (b & 0x7FFF) > 0x7C00


def same_bits(got, want, dtype, sent=None):
    """bit patterns; a NaN result equals any NaN (which NaN is outside the contract) except the destination's sentinel, which
    marks what must not have been written"""
    g, w = np.asarray(got), np.asarray(want)
    assert g.shape == w.shape and g.dtype == w.dtype, (g.shape, w.shape, g.dtype, w.dtype)
    nan = is_nan_bits(g, dtype) & is_nan_bits(w, dtype)
    if sent is not None:
        nan &= (g != sent) & (w != sent)
    same = (g == w) | nan
    assert same.all(), (int((~same).sum()), np.argwhere(~same)[:4].tolist(), [hex(v) for v in g[~same][:4]], [hex(v) for v in w[~same][:4]])


def source(n, ch, F, cap, seed, special=False):
    """float32 [rows][ch][F][cap]: dB-like noise; special: the values of SPECIALS strewn in; the sentinel NaN at and beyond each n"""
    rng = np.random.default_rng(seed)
    x = np.full((len(n), ch, F, cap), SENT_F, F32)
    for r, k in enumerate(n):
        v = (rng.standard_normal((ch, F, k)) * rng.uniform(2.0, 20.0, (ch, F, 1)) - 40.0).astype(F32)
        if special:
            pick = rng.random((ch, F, k)) < 0.5
            v[pick] = SPECIALS[rng.integers(0, len(SPECIALS), int(pick.sum()))]
        x[r, :, :, :k] = v
    return x


def vector(D, seed, scale=False):
    """D float32 values for shift= or scale=, a zero, a negative zero and a subnormal among them"""
    rng = np.random.default_rng(seed)
    v = (rng.standard_normal(D) * (0.5 if scale else 30.0) + (1.0 if scale else 0.0)).astype(F32)
    v[::7] = 0.0
    v[3::11] = -0.0
    v[5::13] = 1e-41
    return v


def plan(F, W, stride):
    """the tile plan of lewton_amd/csrc/lw_pack.hpp restated: (tile, pitch, lines)"""
    tile = 256
    while tile > 16 and (tile - 1) * stride + W > 288:
        tile //= 2
    span = (tile - 1) * stride + W
    return tile, ((span + 30) & ~31) + 1, min(F, 32)


def lds_conflicts(tile, pitch, W, stride, E, G, nu=None):
    """k_pack's LDS accesses for one group of G lines of a tile of nu output frames, under MI355X's banking rules for ds_write_b32
    and ds_read_b32 (MI355X_MICROARCH.md: both are served in two groups of 32 lanes on 32 banks of 4 bytes; a group costs as many
    cycles as its busiest bank has distinct dwords).  Returns (extra cycles of the stores, extra cycles of the loads): (0, 0) is
    conflict-free.  The index arithmetic is the kernel's, restated."""
    nu = tile if nu is None else nu
    span = (nu - 1) * stride + W

    def extra(groups):
        n = 0
        for addrs in groups:
            busy = {}
            for a in addrs:
                busy.setdefault(a % 32, set()).add(a)
            n += max((len(v) for v in busy.values()), default=1) - 1
        return n

    stores = []
    for it in range(-(-span // 64)):                    # lw_pk_load: wave w takes lines w, w + 4, ..; its lanes the frames
        for jt in range(-(-G // 4)):
            for half in range(8):                       # 256 lanes = 8 halves of 32
                lanes = range(32 * half, 32 * half + 32)
                stores.append([((t >> 6) + 4 * jt) * pitch + (t & 63) + 64 * it for t in lanes
                               if (t & 63) + 64 * it < span and (t >> 6) + 4 * jt < G])
    loads = []
    Q = 32 // E
    units = nu * W * Q
    for base in range(0, units, 32):                    # lw_pk_store: 32 consecutive units are one half of a wave
        for i in range(E):
            addrs = []
            for L in range(base, min(base + 32, units)):
                g0, p = (L % Q) * E, L // Q
                if g0 >= G:
                    continue
                u, k = divmod(p, W)
                s = u * stride + k
                addrs.append((g0 + ((i + p - s) % E)) * pitch + s)
            loads.append(addrs)
    return extra(stores), extra(loads)


# +-0, subnormals, +-inf, NaNs with payloads, 0x7f7fffff (rounds to the bf16 infinity), the f16 overflow boundary 65504, 65519.996
# and 65520, f16 subnormal ties (2^-25, 3 * 2^-25, just above and below), the smallest f16 normal and its neighbours, bf16 ties
SPECIAL_BITS = [0x00000000, 0x80000000, 0x00000001, 0x807FFFFF, 0x00800000, 0x7F800000, 0xFF800000, 0x7FC00000, 0x7F800001, 0xFFFFFFFF,
                0x7FBFFFFF, 0x7F7FFFFF, 0xFF7FFFFF, 0x477FE000, 0x477FEFFF, 0x477FF000, 0xC77FF000, 0x47800000, 0x33000000, 0x33000001,
                0x32FFFFFF, 0xB3000000, 0x33C00000, 0x33800000, 0x34400000, 0x387FC000, 0x387FE000, 0x387FF000, 0x38800000, 0x38801000,
                0x3F808000, 0x3F818000, 0x3F808001, 0x3F807FFF, 0xBF808000, 0x3F800000, 0x7F7F8000, 0x7F7F7FFF]
SPECIALS = np.array(SPECIAL_BITS, np.uint32).view(F32)


def window(row, a, b, T, fill_end, before, mask_before, left, right, stride, edge, dtype, shift=None, scale=None, pad=0.0):
    """The window form of rows() for ONE row and channel that is +0.0 outside a few windows (tests/sparse_rows.py: row has F lines
    of at least T frames): output frames [a, b) after the call, from `before` (bit patterns [b - a][W * F]) and mask_before (uint8
    [b - a], or None).  The source frames and the clamp at the row's true ends in Python integers.  Returns (after, mask)"""
    W, F = left + right + 1, row.lines
    k = out_frames(T, left, right, stride, edge)
    assert 0 <= a <= b and k <= fill_end
    out = np.array(before, copy=True)
    msk = None if mask_before is None else np.array(mask_before, copy=True)
    lo, hi = min(a, k), min(b, k)
    if hi > lo:
        if edge == VALID:
            idx = [[u * stride + j for j in range(W)] for u in range(lo, hi)]
        else:
            idx = [[min(max(u * stride - left + j, 0), T - 1) for j in range(W)] for u in range(lo, hi)]
        v = np.ascontiguousarray(row.clipped(T).gather(np.array(idx, np.int64)).transpose(1, 2, 0)).reshape(hi - lo, W * F)   # [u][k][f]
        with np.errstate(over="ignore", invalid="ignore", under="ignore"):
            if shift is not None:
                v = v + np.asarray(shift, F32)[None, :]
            if scale is not None:
                v = v * np.asarray(scale, F32)[None, :]
        assert v.dtype == F32
        out[lo - a:hi - a] = convert(v, dtype)
        if msk is not None:
            msk[lo - a:hi - a] = 1
    f0, f1 = min(max(a, k), fill_end), min(b, fill_end)
    if f1 > f0:
        out[f0 - a:f1 - a] = convert(np.array([pad], F32), dtype)[0]
        if msk is not None:
            msk[f0 - a:f1 - a] = 0
    return out, msk
