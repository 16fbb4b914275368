"""The rows chain past element 2^32 INSIDE a row, on the GPU: k_resample, k_spec, k_spec_complex, k_istft, k_feat, k_norm, k_slide,
k_select and k_pack on one row of 2^32 + 2^20 + 5 elements.  The cases of tests/test_gpu_rows_long_row.py, which runs this file with pytest in a process of its own,
torch imported first (tests/rows_gpu_cases.py says why).

tests/rows_large_gpu_cases.py crosses 2^32 through every index of the layout with short rows; here the position within ONE row
crosses it (c x s.el and n x d.el of k_resample, f0 x hop + lead + k and t.f0 + f of k_spec, at + t0 of k_feat and k_norm,
(u0 + u) x D of k_pack, t.t0 and the windows of k_slide, t.t0, base and K of k_select, (bin + line0) x d_line of k_spec_complex,
t.s0, tf0, r0 and (p - pad) x d.el of k_istft), and a row length above 2^32 reaches the kernels as a count.  A (uint32_t) on one of these gives the samples
of the row's start under LW_OK without a fault: position 2^32 + k is position k of the same row in 32 bits.

Windows and constant middles.  A row has N = 2^32 + 2^20 + 5 elements (odd: the 16-byte paths have a scalar tail) in a capacity of
N + 3, the NaN 0x7FC0DEAD from the length on.  The source is +0.0 except in three windows of a few thousand elements, [0, w),
[2^32 - w, 2^32 + w) and [N - w, N), each with random data of its own -- where a truncated offset lands (window 0) lie other bits
than where it should have gone, which Python integers assert per case.  The whole destination holds the sentinel before a call.
Afterwards the windows of the destination that the source windows reach equal the window forms of the models (tests/*_model.py,
tests/sparse_rows.py; tests/test_window_models.py checks them against the whole-array models) bit for bit, -0 as +0 where the
cases of the kernel's own file do so, and EVERY other element is compared on the device, one torch reduction per stretch, with the
constant a +0.0 source gives there: 0 (k_resample: the bits of the fold of zeros, per phase; unlogged k_spec, k_spec_complex and
k_istft: a zero of either sign; k_slide and k_select: +0.0, taken from the model on a short zero row), LOG(floor) clamped and
finished (k_feat), (0 - m) g (k_norm), the shift / scale vector per column (k_pack); beyond the fill end, the sentinel.  No
tolerance anywhere.

k_spec_complex and k_istft share one geometry, (n_fft, win_length, hop) = (256, 256, 128), hann, centred: the transform of the long
row has 258 lines of 2^25 + 2^13 + 1 frames, twice the waveform's size as at any hop of n_fft / 2 (hop = n_fft would halve it,
but then no sample has two frames and the overlap-add, whose frames tf0 and r0 place, would fold nothing: the geometry is kept).
k_spec_complex with more than 2^32 FRAMES has no case: four lines of 2^32 frames are 69 GB, and its store is the
lw_sp_store_lines that k_spec's 32_hop1_mel1_zero crosses.

k_cep has no case here: lw_cep_rows refuses a line of more than 2^24 - 1 tiles (LW_ERR_CAPACITY, include/lewton_amd.h; a tile has
at most 256 frames), so no frame index of k_cep reaches 2^32 -- DESIGN 6.1.

Memory: ONE allocation of CAP + 258 x (2^25 + 2^13 + 4) + 8 floats (51.8 GB: the waveform's line and its complex transform) for
the whole file, viewed per case, and k_select's mask of N + 3 bytes (4.3 GB) while its two cases run: 56.1 GB at the peak.
PEAK_BYTES bounds what the process may hold at its peak, is asserted below 72 GB in Python integers here, and against torch's own
peak figure when the file is done."""
import torch  # noqa: F401  (first: see above)

import time

import numpy as np
import pytest

import feat_model as FM
import istft_model as IM
import kaldi_model as K
import norm_model as NM
import pack_model as PM
import resample_model as RM
import select_model as SEL
import slide_model as SLM
import spec_model as SM
import spec_reflect_model as XM
from sparse_rows import SparseMask, SparseRow

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
SENT = 0x7FC0DEAD
SENT_F = np.array(SENT, np.uint32).view(F32)
X = 1 << 32                            # the crossing
N = X + (1 << 20) + 5                  # elements of the long row
CAP = N + 3
CX_FFT, CX_HOP = 256, 128              # the complex transform of the long row: 258 lines of CX_T frames, and its inverse
CX_T = 1 + N // CX_HOP                 # 2^25 + 2^13 + 1 frames
CX_LINES, CX_FCAP = CX_FFT + 2, CX_T + 3
CX_ELEMS = CX_LINES * CX_FCAP          # the transform: 2 slots and 67 M elements more
ELEMS = CAP + CX_ELEMS + 8             # the waveform's slot and the transform (+ 8: a destination line may start one element off the 16-byte boundaries)
MASK_BYTES = CAP                       # k_select's mask of the long row: a uint8 tensor of its own, alive during those cases only
PEAK_BYTES = 4 * ELEMS + MASK_BYTES + (4 << 30)   # the allocation, the mask, and 4 GiB for torch's context, the small tensors and the read-backs
assert N % 2 == 1 and CAP % 4 == 0 and CX_T == (1 << 25) + (1 << 13) + 1 and 2 * CAP < CX_ELEMS < 2 * CAP + (1 << 27)
assert 4 * ELEMS == 51_820_695_648 and PEAK_BYTES == 60_411_678_824 and PEAK_BYTES < 72_000_000_000


def _signed(v, bits=32):
    return v - (1 << bits) if v >= 1 << (bits - 1) else v


SENT_I = _signed(SENT)


# ---- the buffer, lines and windows

@pytest.fixture(scope="module")
def buf():
    """one allocation for the whole file, flat float32"""
    free, _ = torch.cuda.mem_get_info(0)
    if free < PEAK_BYTES:
        pytest.skip("less than %.1f GB of device memory free" % (PEAK_BYTES / 1e9))
    torch.cuda.reset_peak_memory_stats(0)
    t0 = time.perf_counter()
    b = torch.empty(ELEMS, dtype=torch.float32, device="cuda:0")
    yield b
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated(0)
    print("\n[rows_long_row] %.1f s from the allocation on, peak device memory %.2f GB" % (time.perf_counter() - t0, peak / 1e9))
    del b
    torch.cuda.empty_cache()
    assert peak <= PEAK_BYTES, (peak, PEAK_BYTES)


def _ints(t):
    return t.view({4: torch.int32, 2: torch.int16, 1: torch.uint8}[t.element_size()])


def _windows(n, w, x=X):
    """the three windows of a row of n elements that crosses x: its start, the crossing, its end"""
    assert 0 < w < x - w and x + w < n - w
    return [(0, w), (x - w, x + w), (n - w, n)]


def _load(line, n, wins):
    """a source line [positions][el]: +0.0 in [0, n), the sentinel from n to the capacity, then the windows' data by bits"""
    line[:n].zero_()
    _ints(line[n:]).fill_(SENT_I)
    for off, d in wins:
        d = np.ascontiguousarray(d, F32).reshape(-1, line.shape[1])
        assert off + len(d) <= n
        _ints(line[off:off + len(d)]).copy_(torch.from_numpy(d.view(np.int32)))


def _read(line, a, b):
    """positions [a, b) of a line as host bits, [b - a][el]"""
    h = _ints(line[a:b]).cpu().numpy()
    return h.view({4: np.uint32, 2: np.uint16, 1: np.uint8}[h.itemsize])


def _all_bits(t, bits, what):
    """on the device, one reduction: every element of the integer tensor t is `bits`"""
    if t.numel():
        lo, hi = torch.aminmax(t)
        assert int(lo) == int(hi) == bits, "%s: bits %#x .. %#x, not %#x" % (what, int(lo) & 0xFFFFFFFF, int(hi) & 0xFFFFFFFF, bits & 0xFFFFFFFF)


def mid_bits(bits):
    """every element of the stretch holds one bit pattern"""
    return lambda line, g0, g1: _all_bits(_ints(line[g0:g1]), _signed(bits, 8 * line.element_size()), "positions [%d, %d)" % (g0, g1))


def mid_zero(line, g0, g1):
    """every element of the stretch is a zero of either sign (a NaN fails: aminmax propagates it)"""
    if g1 > g0:
        lo, hi = torch.aminmax(line[g0:g1])
        assert float(lo) == 0.0 and float(hi) == 0.0, "positions [%d, %d): %r .. %r, not 0" % (g0, g1, float(lo), float(hi))


def mid_columns(vec, period=1):
    """the stretch repeats the bit patterns vec [period][el] from a position that is a multiple of period on: one reduction along
    the positions gives every column's smallest and largest pattern"""
    vec = np.ascontiguousarray(vec).reshape(period, -1)

    def check(line, g0, g1):
        assert g0 % period == 0
        if g1 <= g0:
            return
        want = torch.from_numpy(vec.view({4: np.int32, 2: np.int16}[vec.itemsize]).reshape(-1)).to(line.device)
        flat = _ints(line[g0:g1]).reshape(-1)
        wide = want.repeat(1024)                                      # (1024 periods to a row: torch reduces a tall, narrow matrix slowly)
        rows = flat.numel() // wide.numel()
        if rows:
            lo, hi = torch.aminmax(flat[:rows * wide.numel()].view(rows, wide.numel()), dim=0)
            assert bool((lo == wide).all()) and bool((hi == wide).all()), "positions [%d, %d): not the constant columns" % (g0, g1)
        rest = flat[rows * wide.numel():]
        assert bool((rest == wide[:rest.numel()]).all()), "positions [%d, %d): not the constant columns at the end" % (g0, g1)
    return check


def _verify(line, end, checks, want, mid, same, sent=SENT):
    """A destination line [capacity][el] after a call.  checks: ascending disjoint stretches [a, b) that are read back and compared
    with want(a, b) (bit patterns [b - a][el]; what the line held before the call is the sentinel) by same(got, want).  Every other
    position is compared on the device: below `end` (the fill end) by mid(line, g0, g1), from `end` on with the sentinel"""
    cap, pos = line.shape[0], 0
    for a, b in list(checks) + [(cap, cap)]:
        assert pos <= a <= b <= cap, (pos, a, b, cap)
        if min(a, end) > pos:
            mid(line, pos, min(a, end))
        if a > max(pos, end):
            mid_bits(sent)(line, max(pos, end), a)
        if b > a:
            same(_read(line, a, b), np.ascontiguousarray(want(a, b)).reshape(b - a, -1))
        pos = b


def _assert_crosses(checks, end, x=X):
    """Python integers: a stretch that is read back spans position x, and positions beyond it are written"""
    assert end > x and any(a < x < b for a, b in checks), (checks, end)


def _assert_alias_differs(want, k, x=X):
    """where a position truncated to 32 bits lands, the destination holds other bits: [x, x + k) against [0, k)"""
    here, there = (np.ascontiguousarray(want(a, a + k)).reshape(k, -1) for a in (x, 0))
    assert (here != there).mean() > 0.5, "the crossing window repeats window 0"


def _u32(v):
    return np.ascontiguousarray(v, F32).view(np.uint32)


def _zero_sign(b):
    """-0 counts as +0 (the sign of a zero is outside k_spec's contract)"""
    b = b.copy()
    b[b == 0x80000000] = 0
    return b


def _same(got, want):
    same = got == want
    assert same.all(), (int((~same).sum()), np.argwhere(~same)[:4].tolist(), [hex(v) for v in got[~same][:4]], [hex(v) for v in want[~same][:4]])


def _same_nan(got, want):
    """bits; a NaN result equals any NaN but the sentinel (the rule of FM / NM.same_bits)"""
    g, w = got.view(F32), want.view(F32)
    nan = np.isnan(g) & np.isnan(w) & (got != SENT) & (want != SENT)
    same = (got == want) | nan
    assert same.all(), (int((~same).sum()), np.argwhere(~same)[:4].tolist(), [hex(v) for v in got[~same][:4]], [hex(v) for v in want[~same][:4]])


def _same_zero_sign(got, want):
    _same(_zero_sign(got), _zero_sign(want))


class _Clock:
    """where a case's seconds go, printed (the runner's output shows it)"""

    def __init__(self, name):
        self.name, self.t, self.parts = name, time.perf_counter(), []

    def lap(self, what):
        torch.cuda.synchronize()
        now = time.perf_counter()
        self.parts.append("%s %.2f" % (what, now - self.t))
        self.t = now

    def done(self):
        print("\n[rows_long_row] %s: %s (seconds)" % (self.name, ", ".join(self.parts)))


def _line(buf, start, cap=CAP, el=1):
    return buf[start:start + cap * el].view(cap, el)


# ---- k_feat

W_EL = 3000                            # a window of the elementwise kernels: more than two runs of 1024, and no multiple of four
# name -> (in place, top, want_max, (n', fill_to) or None)
FEAT = {
    "two_launches": (False, 8.0, True, None),
    "two_launches_in_place": (True, 8.0, True, None),
    "one_launch": (False, float("inf"), False, None),
    "one_launch_in_place": (True, float("inf"), False, None),
    "fill_straddles": (False, 8.0, True, (X - 100, X + 100)),        # the data ends just below the crossing, the fill crosses it
}


def _feat_values(n, seed):
    """six decades up to 1e3, which the clamp 8 below the row's maximum of 3e5 leaves apart; one value in ten is a negative, a
    zero, a NaN, a subnormal, the floor itself or -inf: all of them the floor after step 1, and clamped"""
    rng = np.random.default_rng(seed)
    v = (10.0 ** rng.uniform(-3, 3, n)).astype(F32)
    odd = np.array([-1.5, 0.0, -0.0, np.nan, 1e-42, 1.4e-45, 1e-10, -np.inf], F32)
    pick = rng.random(n) < 0.1
    v[pick] = odd[rng.integers(0, len(odd), int(pick.sum()))]
    return v


@pytest.mark.parametrize("name", list(FEAT))
def test_k_feat_inside_a_row_past_2_to_the_32(buf, name):
    """[1][1][1][N].  The row's maximum sits in the crossing window, beyond 2^32 (just below it in the fill case): a second launch
    that re-read l or folded the maxima at a truncated position would clamp with another M"""
    from lewton_amd.rows import LogCompress
    inplace, top, want_max, straddle = FEAT[name]
    n, end = straddle or (N, N)
    wins = [(a, _feat_values(b - a, 11 + i)) for i, (a, b) in enumerate(_windows(N, W_EL))]
    wins[1][1][W_EL + 7 if straddle is None else W_EL - 107] = 3e5   # everything else is at most 1e3
    row = SparseRow(N, [(a, d[None]) for a, d in wins]).clipped(n)
    args = (FM.LOG10, FM.ROW, 1e-10, top, 4.0, 0.25)
    checks = [(0, W_EL + 5), (X - W_EL - 5, X + W_EL + 5), (N - W_EL - 5, CAP)]

    def want(a, b):
        return _u32(FM.window(row, 1, 1, a, b, n, end, np.full((1, 1, b - a), SENT_F, F32), *args)[0])
    M = FM.window(row, 1, 1, 0, 0, n, end, np.zeros((1, 1, 0), F32), *args)[1]
    assert float(M) == float(FM.log(FM.LOG10, np.array([3e5], F32))[0])
    _assert_crosses(checks, end)
    _assert_alias_differs(want, 100)
    clock = _Clock("k_feat " + name)
    src = _line(buf, 0)
    dst = src if inplace else _line(buf, CAP + 1)                    # out of place: the lines sit differently against 16 bytes
    _load(src, n, [(a, d[:max(0, min(len(d), n - a))]) for a, d in wins if a < n])
    if not inplace:
        _ints(dst).fill_(SENT_I)
    lc = LogCompress("log10", 1e-10, top, 4.0, 0.25, "row")
    try:
        torch.cuda.synchronize()
        clock.lap("load")
        res = lc.run(src.view(1, 1, 1, CAP), [n], out=None if inplace else dst.view(1, 1, 1, CAP), fill_to=[end], want_max=want_max)
        clock.lap("run")
        assert lc.last_launches() == (2 if want_max or top != float("inf") else 1)
        fill_bits = int(_u32(FM.finish(FM.log(FM.LOG10, np.array([1e-10], F32)), M, top, 4.0, 0.25))[0])
        _verify(dst, end, checks, want, mid_bits(fill_bits), _same_nan)
        clock.lap("verify")
        clock.done()
        if want_max:
            FM.same_bits(res[1].cpu().numpy(), np.array([M], F32))
    finally:
        lc.close()


# ---- k_norm

# name -> (constructor arguments, lines F, 3-D tensor, in place, (n', fill_to) or None)
NORM = {
    "wav2vec2": ((True, "std", 1e-7, 1.0, "channel"), 1, True, False, None),
    "cmvn_two_lines_in_place": ((True, "std", 1e-20, 1.0, "line"), 2, False, True, None),
    "peak_in_place": ((False, "peak", 0.0, 0.5, "row"), 1, False, True, None),
    "fill_straddles": ((True, "std", 1e-7, 1.0, "channel"), 1, True, False, (X - 100, X + 100)),
}


@pytest.mark.parametrize("name", list(NORM))
def test_k_norm_inside_a_row_past_2_to_the_32(buf, name):
    """Values that are integers / 1024: S1 and S2 are exact in double under any bracketing of the tree, so the model is integer
    arithmetic (NM.exact_sums) fed to lw_norm_scalars with N = n > 2^32 -- the count the fold kernel turns into a double.  Every
    line's largest |x| sits beyond 2^32"""
    from lewton_amd.rows import Normalize
    (center, scale, eps, target, scope), F, squeeze, inplace, straddle = NORM[name]
    n, end = straddle or (N, N)
    rng = np.random.default_rng(70 + len(name))
    wins = []
    for a, b in _windows(N, W_EL):
        d = (rng.integers(-1023, 1024, (F, b - a)) / 1024.0).astype(F32)
        if a < X < b:
            d[:, W_EL + 11 if straddle is None else W_EL - 111] = 1.0
        wins.append((a, d))
    row = SparseRow(N, wins, F).clipped(n)
    nm = Normalize(center, scale, eps, target, scope)
    try:
        model = (int(center), NM.SCALES[scale], NM.SCOPES[scope], eps, target)

        def scalars_of(S1, S2, P, count):
            got = nm.scalars(S1, S2, P, count)
            assert got == tuple(float(v) for v in NM.scalars(model[0], model[1], eps, target, S1, S2, P, count)) and count > X - 101
            return got

        def window(a, b):
            return NM.window(row, 1, F, a, b, n, end, np.full((1, F, b - a), SENT_F, F32), *model, scalars_of=scalars_of)
        stats = np.asarray(window(0, 0)[1], F64).reshape(-1, 2)       # [F or 1][2]
        checks = [(0, W_EL + 5), (X - W_EL - 5, X + W_EL + 5), (N - W_EL - 5, CAP)]
        _assert_crosses(checks, end)
        src = [_line(buf, l * CAP) for l in range(F)]
        dst = src if inplace else [_line(buf, CAP + 1)]
        assert inplace or F == 1
        for l in range(F):
            _load(src[l], n, [(a, d[l, :max(0, min(d.shape[1], n - a))]) for a, d in wins if a < n])
        if not inplace:
            _ints(dst[0]).fill_(SENT_I)
        shape = (1, 1, CAP) if squeeze else (1, 1, F, CAP)
        whole = buf[:F * CAP].view(shape)
        out = None if inplace else dst[0].view(shape)
        clock = _Clock("k_norm " + name)
        clock.lap("load")
        res = nm.run(whole, [n], out=out, fill_to=[end], want_stats=True)
        clock.lap("run")
        assert nm.last_launches() == 3
        NM.same_bits(res[1].cpu().numpy().reshape(-1, 2), stats[:F] if scope == "line" else stats[:1])
        for l in range(F):
            m, g = stats[l if scope == "line" else 0]

            def want(a, b, l=l):
                return _u32(window(a, b)[0][0, l])
            _assert_alias_differs(want, 100)
            _verify(dst[l], end, checks, want, mid_bits(int(_u32(NM.apply(np.zeros(1, F32), m, g))[0])), _same_nan)
        clock.lap("verify")
        clock.done()
    finally:
        nm.close()


# ---- k_pack

PK_F, PK_LEFT, PK_RIGHT = 16, 7, 8
PK_D = (PK_LEFT + PK_RIGHT + 1) * PK_F                               # 256 elements per output frame
PK_T = (1 << 24) + (1 << 10) + 3                                    # frames: output frame 2^24 starts at element 2^32 of its row
PK_W = 300                                                           # frames per window: more than a tile of 256


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_k_pack_inside_a_row_past_2_to_the_32(buf, dtype):
    """[1][1][16][T + 5] -> [1][1][T + 2][256] with W = 16 at stride 1, shift, scale and the mask: (u0 + u) x D passes 2^32 at
    output frame 2^24, inside the row.  One frame of pad behind the row, one frame of the sentinel behind that"""
    from lewton_amd.rows import FramePack
    T, scap, ocap, end = PK_T, PK_T + 5, PK_T + 2, PK_T + 1
    xu = X // PK_D
    assert xu * PK_D == X and xu + PK_W < T - PK_W and T * PK_D > X and ocap * PK_D <= CAP and PK_F * scap <= CAP
    rng = np.random.default_rng(90)
    wins = [(a, (rng.standard_normal((PK_F, b - a)) * 10.0 - 40.0).astype(F32)) for a, b in _windows(T, PK_W, xu)]
    row = SparseRow(T, wins, PK_F)
    shift, scale = PM.vector(PK_D, 1), PM.vector(PK_D, 2, True)
    pk = FramePack(PK_F, PK_LEFT, PK_RIGHT, 1, "replicate", dtype, shift=shift, scale=scale, pad=-1.0)
    try:
        assert pk.tile_frames == 256 and pk.frames(T) == T
        od = PM.OUT_DTYPE[dtype]

        def window(a, b):
            return PM.window(row, a, b, T, end, np.full((b - a, PK_D), PM.sentinel(dtype), od), np.full(b - a, PM.SENT_MASK, np.uint8),
                             PK_LEFT, PK_RIGHT, 1, PM.REPLICATE, dtype, pk._shift, pk._scale, -1.0)
        m = PK_LEFT + PK_RIGHT + 2
        checks = [(0, PK_W + m), (xu - PK_W - m, xu + PK_W + m), (T - PK_W - m, ocap)]
        want = lambda a, b: window(a, b)[0]
        _assert_crosses(checks, end, xu)
        _assert_alias_differs(want, PK_W // 2, xu)
        src = buf[:PK_F * scap].view(PK_F, scap)
        for f in range(PK_F):
            _load(src[f].view(scap, 1), T, [(a, d[f]) for a, d in wins])
        flat = buf[CAP:CAP + (ocap * PK_D if dtype == "f32" else ocap * PK_D // 2)]
        dst = (flat if dtype == "f32" else flat.view(torch.bfloat16)).view(ocap, PK_D)
        _ints(dst).fill_(_signed(PM.sentinel(dtype), 8 * dst.element_size()))
        msk = torch.full((1, ocap), PM.SENT_MASK, dtype=torch.uint8, device="cuda:0")
        clock = _Clock("k_pack " + dtype)
        clock.lap("load")
        _, frames, _ = pk.run(src.view(1, 1, PK_F, scap), [T], out=dst.view(1, 1, ocap, PK_D), fill_to=[end], want_mask=msk)
        clock.lap("run")
        assert frames.tolist() == [T] and pk.last_launches() == 1
        with np.errstate(all="ignore"):
            zero_frame = PM.convert((np.zeros(PK_D, F32) + pk._shift) * pk._scale, dtype)
        assert len(set(zero_frame.tolist())) > PK_D // 2
        _verify(dst, end, checks, want, mid_columns(zero_frame), lambda g, w: PM.same_bits(g, w.astype(od), dtype, PM.sentinel(dtype)),
                sent=PM.sentinel(dtype))
        assert bool((msk[0, :T] == 1).all()) and bool((msk[0, T:end] == 0).all()) and bool((msk[0, end:] == PM.SENT_MASK).all())
        assert np.array_equal(window(T - 3, ocap)[1], msk[0, T - 3:].cpu().numpy())
        clock.lap("verify")
        clock.done()
        for a, d in wins:                                             # the source was only read
            assert np.array_equal(src[:, a:a + d.shape[1]].cpu().numpy().view(np.uint32), d.view(np.uint32))
    finally:
        pk.close()


# ---- k_resample

RS_W = 2100                            # samples per window of the source
IT = (1 << 30) + (1 << 18) + 1         # samples of the interleaved row of four channels: 4 IT = 2^32 + 2^20 + 4
# name -> (in_rate, out_rate, interleaved, source samples, route)
RESAMPLE = {
    "planar_copy": (16000, 16000, False, N, 3),
    "planar_48k_16k_source_crosses": (48000, 16000, False, N, 0),
    "planar_16k_48k_destination_crosses": (16000, 48000, False, N // 3, 0),
    "interleaved_48k_16k_source_crosses": (48000, 16000, True, IT, 0),
    "interleaved_16k_48k_destination_crosses": (16000, 48000, True, IT // 3, 0),
    "interleaved_copy": (16000, 16000, True, IT, 3),
}


def _pcm(shape, seed):
    rng = np.random.default_rng(seed)
    v = rng.uniform(-1, 1, shape).astype(F32)
    v[..., 5::11] *= F32(-0.0)
    v[..., 3::13] *= F32(1e-39)
    return v


@pytest.mark.parametrize("name", list(RESAMPLE))
def test_k_resample_inside_a_row_past_2_to_the_32(buf, name):
    """One row, one channel ([1][1][CAP]) or four interleaved ([1][IT + 1][4]: c x s.el and n x d.el pass 2^32 while the sample
    index stays below it).  Whichever side is the longer one has its middle window across element 2^32 of the row, the other
    side's follows by the rate; base and phase of the outputs there are Python integers"""
    from lewton_amd.rows import Resampler, resample_geometry
    in_rate, out_rate, itl, n, route = RESAMPLE[name]
    el = 4 if itl else 1
    rs = Resampler(in_rate, out_rate)
    try:
        orig, new, hw, Kt = resample_geometry(in_rate, out_rate)
        assert (orig, new, hw, Kt) == (rs.orig, rs.new, rs.half_width, rs.taps_per_phase)
        out = rs.out_len(n)
        assert out == RM.out_len(n, orig, new)
        longer = max(n, out)
        assert longer * el > X and (n * el > X) == ("copy" in name or "source" in name) and (out * el > X) == ("copy" in name or "destination" in name)
        xs = X // el * orig // max(orig, new)                          # the source sample whose output lies at the crossing
        swin = _windows(n, RS_W, xs)
        data = [_pcm((el, b - a), 60 + len(name) + i) for i, (a, b) in enumerate(swin)]
        rows = [SparseRow(n, [(a, d[c][None]) for (a, _), d in zip(swin, data)]) for c in range(el)]
        h = rs.taps() if orig != new else None

        def want(a, b):
            """bit patterns [b - a][el]: outputs [a, b) below out_len, the sentinel from there on"""
            hi = max(a, min(b, out))
            if h is None:
                y = np.stack([_u32(r.take(a, hi)[0]) for r in rows], axis=1)
            else:
                y = np.stack([_u32(RM.fold_window(h, orig, new, hw, r, a, hi)) for r in rows], axis=1)
            return np.concatenate([y, np.full((b - hi, el), SENT, np.uint32)])
        # the outputs the source windows reach, widened to multiples of `new` (a stretch of constant columns starts at phase 0)
        checks = []
        for a, b in swin:
            lo, hi = max(0, (a - Kt) * new // orig // new * new), min(out, -(-((b + Kt) * new // orig + 1) // new) * new)
            checks.append((lo, hi))
        scap = dcap = CAP // el
        checks[-1] = (checks[-1][0], min(dcap, out + 8))               # (the sentinel behind that is compared on the device)
        assert checks[-1][0] <= out - 1 and n <= scap and out <= dcap
        xd = X // el if out * el > X else xs * new // orig
        assert any(a < xd < b for a, b in checks) and checks[1][0] > checks[0][1] and checks[2][0] > checks[1][1]
        if out * el > X:
            _assert_alias_differs(want, 60, X // el)
            base, ph = RM.base_phase(X // el + 1, orig, new)           # an output past the crossing, in Python integers
            assert base == (X // el + 1) * orig // new and 0 <= ph < new and base + Kt < n
        if n * el > X:                                                 # outputs whose taps lie past element 2^32 of the source
            k = -(-(X // el + hw) * new // orig) + 1
            assert (RM.base_phase(k, orig, new)[0] - hw) * el >= X and checks[1][0] < k < checks[1][1]
            far = want(k, k + 60)
            near = want(k - (X // el) * new // orig, k - (X // el) * new // orig + 60) if (X // el) * new % orig == 0 else None
            assert near is None or (far != near).mean() > 0.5
        src, dst = _line(buf, 0, scap, el), _line(buf, CAP, dcap, el)
        _load(src, n, [(a, d.T) for (a, _), d in zip(swin, data)])
        _ints(dst).fill_(SENT_I)
        if h is None:
            zero = np.zeros((1, el), np.uint32)
        else:                                                          # the fold of zeros: +0.0 or -0.0 by the signs of a phase's taps
            z = _u32(RM.fold_window(h, orig, new, hw, SparseRow(n, []), checks[0][1], checks[0][1] + new))
            zero = np.repeat(z[:, None], el, axis=1)
            assert not (z & 0x7FFFFFFF).any()
        clock = _Clock("k_resample " + name)
        clock.lap("load")
        shape_s, shape_d = ((1, scap, el), (1, dcap, el)) if itl else ((1, 1, scap), (1, 1, dcap))
        assert rs.run(src.view(shape_s), [n], out=dst.view(shape_d), samples="f32_interleaved" if itl else "f32") is not None
        clock.lap("run")
        assert rs.last_route == route
        _verify(dst, out, checks, want, mid_columns(zero, new if h is not None else 1), _same)
        clock.lap("verify")
        clock.done()
        for (a, _), d in zip(swin, data):                              # the source was only read
            assert np.array_equal(_read(src, a, a + d.shape[1]), _u32(d.T))
    finally:
        rs.close()


# ---- k_spec

SP_W = 8192                            # samples per window of the source: 51 frames at hop 160, more than a tile of 32
# name -> (n_fft, win_length, hop, pad mode or "kaldi", routes)
SPEC = {
    "400_160_mel1_zero": (400, 400, 160, "zero", (0, 1)),
    "400_160_mel1_reflect": (400, 400, 160, "reflect", (0, 1)),
    # the frame index itself crosses: the destination line is longer than 2^32.  Route 0 only: the per-lane fmaf chains of route 1 take
    # 5.6 s for these 2^32 frames (1.9 s on the matrix cores), and the index arithmetic around them is the same code
    "32_hop1_mel1_zero": (32, 32, 1, "zero", (0,)),
    "kaldi_512_400_160_dc_energy": (512, 400, 160, "kaldi", (0, 1)),
}


@pytest.mark.parametrize("name", list(SPEC))
def test_k_spec_inside_a_row_past_2_to_the_32(buf, name):
    """[1][1][CAP] of N samples -> one mel band ([1][1][1][frames + 3]; with Kaldi's framing the energy line in front of it), on
    both routes (at hop 1 on route 0 alone: SPEC says why).  f0 x hop + lead + k passes 2^32 in the source; under reflect and under Kaldi's symmetric padding the last frames
    read back from len - 1 > 2^32; at hop 1 the frame index t.f0 + f passes it too"""
    from lewton_amd.rows import Spectrogram, kaldi_mel_banks, mel_filterbank
    n_fft, win, hop, pad, routes = SPEC[name]
    kaldi = pad == "kaldi"
    if kaldi:
        mel = kaldi_mel_banks(16000, n_fft, 1)
        sp = Spectrogram(n_fft, hop, win, "povey", center=False, mel=mel, framing="kaldi", snip_edges=False, preemphasis=0.97, remove_dc=True,
                         energy=True, scale=32768.0)
    else:
        mel = mel_filterbank(16000, n_fft, 1)
        sp = Spectrogram(n_fft, hop, mel=mel, pad_mode=pad)
    try:
        frames, F = sp.frames(N), sp.features
        fcap = frames + 3
        assert F == (2 if kaldi else 1) and F * fcap <= CAP + 8 and frames == (K.n_frames(N, win, hop, False) if kaldi else 1 + N // hop)
        swin = _windows(N, SP_W)
        data = [np.random.default_rng(40 + len(name) + i).uniform(-1, 1, b - a).astype(F32) for i, (a, b) in enumerate(swin)]
        row = SparseRow(N, [(a, d[None]) for (a, _), d in zip(swin, data)])
        basis = sp.basis()

        memo = {}

        def lines(a, b):
            """float32 [F][b - a]: frames [a, b) below `frames`, the sentinel from there on (computed once: both routes ask)"""
            if (a, b) not in memo:
                memo[a, b] = _lines(a, b)
            return memo[a, b]

        def _lines(a, b):
            out = np.full((F, b - a), SENT_F, F32)
            hi = min(b, frames)
            if hi > a:
                if kaldi:
                    Y = K.features(basis, mel, K.frame_matrix_window(row, a, hi, win, hop, False), True, True, 32768.0)
                elif pad == "reflect":
                    Y = SM.features(basis, mel, XM.frame_matrix_window(row, a, hi, n_fft, win, hop))
                else:
                    Y = SM.features(basis, mel, SM.frame_matrix_window(row, a, hi, n_fft, win, hop, True))
                out[:, :hi - a] = Y.T
            return out
        checks = [(max(0, (a - 2 * n_fft) // hop - 1), min(frames, (b + 2 * n_fft) // hop + 2)) for a, b in swin]
        checks[-1] = (checks[-1][0], fcap)
        xf = X // hop                                                  # the frame whose support lies at sample 2^32
        assert any(a < xf < b for a, b in checks) and (frames - 1) * hop + win > X and checks[1][0] > checks[0][1]
        assert (frames > X) == (hop == 1)
        if hop == 1:
            _assert_crosses(checks, frames)
            _assert_alias_differs(lambda a, b: _u32(lines(a, b)[0]), 60)
        else:                                                          # the frames at the crossing are no copy of the frames at the start
            assert (_zero_sign(_u32(lines(xf, xf + 20))) != _zero_sign(_u32(lines(0, 20)))).all()
        live = lines(xf, xf + 8)
        assert not np.isnan(live).any() and (live[-1] > 0).all()
        src = _line(buf, 0)
        dst = [_line(buf, CAP + l * fcap, fcap) for l in range(F)]
        _load(src, N, [(a, d) for (a, _), d in zip(swin, data)])
        clock = _Clock("k_spec " + name)
        for route in routes:
            sp.set_route(route)
            for d in dst:
                _ints(d).fill_(SENT_I)
            clock.lap("load")
            out, got_frames = sp.run(src.view(1, 1, CAP), [N], out=buf[CAP:CAP + F * fcap].view(1, 1, F, fcap))
            clock.lap("route %d" % route)
            assert sp.last_route() == route and got_frames.tolist() == [frames]
            for l in range(F):
                _verify(dst[l], frames, checks, lambda a, b, l=l: _u32(lines(a, b)[l]), mid_zero, _same_zero_sign)
            clock.lap("verify")
        clock.done()
        for (a, _), d in zip(swin, data):                              # the source was only read
            assert np.array_equal(_read(src, a, a + len(d))[:, 0], _u32(d))
    finally:
        sp.close()


# ---- k_slide

SL_W = 3000                            # frames per window of the source: more than two tiles of 1024
# name -> ((W, min, center, norm_vars), (n', fill_to) or None)
SLIDE = {
    "centred_vars": ((300, 100, 1, 1), None),
    "causal": ((8, 3, 0, 0), None),
    "fill_straddles": ((300, 100, 1, 1), (X - 100, X + 100)),       # the data ends just below the crossing, the fill crosses it
}


def _zero_row_gives(model):
    """what the model makes of a +0.0 source, taken from the model on a short zero row: one bit pattern"""
    bits = set(_u32(model(np.zeros((1, 1, 1, 700), F32))).ravel().tolist())
    assert len(bits) == 1
    return bits.pop()


@pytest.mark.parametrize("name", list(SLIDE))
def test_k_slide_inside_a_row_past_2_to_the_32(buf, name):
    """[1][1][1][N + 3] at the default tile of 1024 frames: t.t0, the windows s and e of rule 1 in int64 against t.lo, and the
    loads and stores at t.at + t.lo + i and t.at + t.t0 + i pass 2^32; the row's T reaches the kernel as a count above 2^32"""
    from lewton_amd.rows import SlidingCMVN
    cfg, straddle = SLIDE[name]
    n, end = straddle or (N, N)
    W = cfg[0]
    rng = np.random.default_rng(20 + len(name))
    wins = [(a, (rng.standard_normal((1, b - a)) * 3.0 - 12.0).astype(F32)) for a, b in _windows(N, SL_W)]
    row = SparseRow(N, wins).clipped(n)
    args = (cfg[0], cfg[1], bool(cfg[2]), bool(cfg[3]))
    m = SL_W + W + 5                                                 # a frame's window reaches at most W frames to either side
    checks = [(0, m), (X - m, X + m), (N - m, CAP)]
    tiles = -(-end // 1024)
    assert tiles == (1 << 22) + 1025 - (straddle is not None) * 1024 and tiles <= 0xFFFFFF

    def want(a, b):
        return _u32(SLM.window_rows(row, a, b, n, end, np.full((1, b - a), SENT_F, F32), *args)).T
    zero = _zero_row_gives(lambda x: SLM.rows(x, [700], None, x, *args))
    assert zero == 0
    _assert_crosses(checks, end)
    if straddle is None:
        _assert_alias_differs(want, 100)
    clock = _Clock("k_slide " + name)
    src, dst = _line(buf, 0), _line(buf, CAP + 1)
    _load(src, n, [(a, d[0, :max(0, min(d.shape[1], n - a))]) for a, d in wins if a < n])
    _ints(dst).fill_(SENT_I)
    sl = SlidingCMVN(*args)
    try:
        assert sl.tile_frames == 1024
        clock.lap("load")
        assert sl.run(src.view(1, 1, 1, CAP), [n], out=dst.view(1, 1, 1, CAP), fill_to=[end]) is not None
        clock.lap("run")
        assert sl.last_launches() == 1
        _verify(dst, end, checks, want, mid_bits(zero), _same_nan)
        clock.lap("verify")
        clock.done()
        for a, d in row.wins:                                         # the source was only read
            assert np.array_equal(_read(src, a, a + d.shape[1])[:, 0], _u32(d[0]))
    finally:
        sl.close()


def test_k_slide_refuses_more_tiles_than_a_grid_counts(buf):
    """a tile of 16 frames on this row is 2^28 tiles and more: LW_ERR_CAPACITY before anything is queued, nothing written"""
    from lewton_amd.rows import SlidingCMVN
    src, dst = _line(buf, 0), _line(buf, CAP + 1)
    src[:N].zero_()
    _ints(dst).fill_(SENT_I)
    sl = SlidingCMVN(8, 3, False, False)
    try:
        sl.set_tile_frames(16)
        assert -(-N // 16) > 0xFFFFFF
        with pytest.raises(ValueError):
            sl.run(src.view(1, 1, 1, CAP), [N], out=dst.view(1, 1, 1, CAP))
        torch.cuda.synchronize()
        mid_bits(SENT)(dst, 0, CAP)
    finally:
        sl.close()


# ---- k_select_count and k_select

SE_W = 5000                            # frames per window: more than two tiles of 2048
SE_TILE = 2048                         # every workgroup of k_select adds up ALL tile counts of its row: 2^21 + 513 of them here


@pytest.mark.parametrize("name", ["keep_most", "drop_middle"])
def test_k_select_inside_a_row_past_2_to_the_32(buf, name):
    """[1][1][1][N + 3] with a mask of N + 3 bytes of its own.  keep_most: the mask is 1 except for random bytes in the three windows
    (one in ten is 0), so the kept frames of the crossing window land at p - dropped_before(p), at and past 2^32, K > 2^32, and the
    base of the later tiles sums past 2^32.  drop_middle: the mask is 0 between the first and the last window, so the frames of the
    last window, gathered from past 2^32, land near the row's start, and the zeroed tail [K, N) runs across 2^32"""
    from lewton_amd.rows import SelectFrames
    rng = np.random.default_rng(30 + len(name))
    ranges = _windows(N, SE_W)
    wins = [(a, SEL.source([b - a], 1, 1, b - a, 40 + i)[0, 0]) for i, (a, b) in enumerate(ranges)]
    row = SparseRow(N, wins)
    if name == "keep_most":
        bytes_ = [(rng.integers(1, 256, b - a) * (rng.random(b - a) >= 0.1)).astype(np.uint8) for a, b in ranges]
        sm = SparseMask(N, [(0, SE_W, bytes_[0]), (SE_W, X - SE_W, 1), (X - SE_W, X + SE_W, bytes_[1]), (X + SE_W, N - SE_W, 1), (N - SE_W, N, bytes_[2])])
    else:
        bytes_ = [(rng.random(b - a) < 0.5).astype(np.uint8) for a, b in ranges]
        sm = SparseMask(N, [(0, SE_W, bytes_[0]), (SE_W, N - SE_W, 0), (N - SE_W, N, bytes_[2])])
    K = sm.count()
    d0, d1 = (int((v == 0).sum()) for v in bytes_[:2])
    if name == "keep_most":
        assert K == N - d0 - d1 - int((bytes_[2] == 0).sum()) and K > X and 0 < d0 and d0 + d1 < SE_W
        checks = [(0, SE_W + 5), (X - SE_W - d0 - 5, X + SE_W + 5), (K - SE_W - 5, CAP)]
        assert X - SE_W < int(sm.places(X - 1, X)[0]) < int(sm.places(X, X + 1)[0]) < X + SE_W               # the crossing is fed from the window
    else:
        k0 = SE_W - d0
        assert K == k0 + int((bytes_[2] != 0).sum()) and k0 < K < 2 * SE_W and int(sm.places(K - 1, K)[0]) > X
        checks = [(0, 2 * SE_W + 5), (X - 5, X + 5), (N - 5, CAP)]

    def want(a, b):
        return _u32(SEL.window_rows(row, sm, a, b, N, N, np.full((1, b - a), SENT_F, F32))[0]).T
    zero = _zero_row_gives(lambda x: SEL.rows(x, np.ones((1, 1, 700), np.uint8), [700], None, x)[0])
    assert zero == 0
    _assert_crosses(checks, N)
    if name == "keep_most":
        _assert_alias_differs(want, 100)
    clock = _Clock("k_select " + name)
    src, dst = _line(buf, 0), _line(buf, CAP + 1)
    _load(src, N, [(a, d) for a, d in wins])
    _ints(dst).fill_(SENT_I)
    dm = torch.empty(CAP, dtype=torch.uint8, device="cuda:0")
    se = SelectFrames()
    try:
        dm[N:].fill_(SEL.SENT_MASK)
        for lo, hi, v in sm.pieces:
            if isinstance(v, np.ndarray):
                dm[lo:hi].copy_(torch.from_numpy(v))
            else:
                dm[lo:hi].fill_(int(v))
        se.set_tile_frames(SE_TILE)
        assert -(-N // SE_TILE) == (1 << 21) + 513 <= 0xFFFFFF
        clock.lap("load")
        _, counts = se.run(src.view(1, 1, 1, CAP), [N], dm.view(1, 1, CAP), out=dst.view(1, 1, 1, CAP))
        clock.lap("run")
        assert se.last_launches() == 2 and counts.cpu().tolist() == [[K]]
        _verify(dst, N, checks, want, mid_bits(zero), _same)
        clock.lap("verify")
        clock.done()
        for a, d in wins:                                             # the source and the mask were only read
            assert np.array_equal(_read(src, a, a + d.shape[1])[:, 0], _u32(d[0]))
        for lo, hi, v in sm.pieces:
            if isinstance(v, np.ndarray):
                assert np.array_equal(dm[lo:hi].cpu().numpy(), v)
    finally:
        se.close()
        del dm
        torch.cuda.empty_cache()


# ---- k_spec_complex and k_istft: one geometry, (n_fft, win_length, hop) = (256, 256, 128), hann, centred

def _verify_lines(lines, end, checks, want, same):
    """_verify for a destination [lines][capacity], every line at once: checks are stretches [a, b) of frames, read back and
    compared with want(a, b) (float32 [lines][b - a]) by same() on the bit patterns; every other frame below `end` is a zero of
    either sign, from `end` on the sentinel, each stretch one reduction along the lines on the device (along: a reduction over
    all of a strided stretch would copy it first, 34 GB of it)"""
    cap, pos = lines.shape[1], 0
    for a, b in list(checks) + [(cap, cap)]:
        assert pos <= a <= b <= cap, (pos, a, b, cap)
        if min(a, end) > pos:
            lo, hi = torch.aminmax(lines[:, pos:min(a, end)], dim=1)   # (a NaN fails: aminmax propagates it)
            lo, hi = float(lo.min()), float(hi.max())
            assert lo == 0.0 and hi == 0.0, "frames [%d, %d): %r .. %r, not 0" % (pos, min(a, end), lo, hi)
        if a > max(pos, end):
            lo, hi = torch.aminmax(_ints(lines[:, max(pos, end):a]), dim=1)
            _all_bits(torch.stack([lo, hi]), SENT_I, "frames [%d, %d)" % (max(pos, end), a))
        if b > a:
            same(_ints(lines[:, a:b]).cpu().numpy().view(np.uint32), _u32(want(a, b)))
        pos = b


def _chains(basis, Xf):
    """the two chains of the contract over a frame matrix [T][W]: float32 [2 B][T], the re lines, then the im lines"""
    re, im = (np.zeros((Xf.shape[0], basis.shape[2]), F32) for _ in range(2))
    for k in range(basis.shape[1]):
        re, im = SM.fmaf(Xf[:, k:k + 1], basis[0][k][None, :], re), SM.fmaf(Xf[:, k:k + 1], basis[1][k][None, :], im)
    return np.concatenate([re, im], axis=1).T


# name -> (pad mode, routes).  reflect runs both (route 1, the per-lane fmaf chains, takes 0.57 s for the 2^25 frames); zero runs route 0
# alone: the index arithmetic around the fold is the same code on both routes
COMPLEX = {"complex_256_128_reflect": ("reflect", (0, 1)), "complex_256_128_zero": ("zero", (0,))}


@pytest.mark.parametrize("name", list(COMPLEX))
def test_k_spec_complex_inside_a_row_past_2_to_the_32(buf, name):
    """L[complex_256_128]: [1][1][CAP] of N samples -> [1][1][258][CX_T + 3].  The source sample index f0 x hop + lead + k and, under
    reflect, the tail read back from len - 1 > 2^32 run in the complex instantiation; its store puts re[j] on line j and im[j] on
    line 129 + j of a destination of 8.66 G elements, so (bin + line0) x d_line passes 2^32 (at line 128) and 2^33"""
    from lewton_amd.rows import Spectrogram
    pad, routes = COMPLEX[name]
    sp = Spectrogram(CX_FFT, CX_HOP, pad_mode=pad, output="complex")
    try:
        frames, F = sp.frames(N), sp.features
        assert frames == CX_T and F == CX_LINES and (F - 1) * CX_FCAP > 1 << 33 and 128 * CX_FCAP >= X > 127 * CX_FCAP
        swin = _windows(N, SP_W)
        data = [np.random.default_rng(50 + len(pad) + i).uniform(-1, 1, b - a).astype(F32) for i, (a, b) in enumerate(swin)]
        row = SparseRow(N, [(a, d[None]) for (a, _), d in zip(swin, data)])
        basis = sp.basis()
        memo = {}

        def lines(a, b):
            if (a, b) not in memo:
                out = np.full((F, b - a), SENT_F, F32)
                hi = min(b, frames)
                if hi > a:
                    Xf = (XM.frame_matrix_window(row, a, hi, CX_FFT, CX_FFT, CX_HOP) if pad == "reflect" else
                          SM.frame_matrix_window(row, a, hi, CX_FFT, CX_FFT, CX_HOP, True))
                    out[:, :hi - a] = _chains(basis, Xf)
                memo[a, b] = out
            return memo[a, b]
        checks = [(max(0, (a - 2 * CX_FFT) // CX_HOP - 1), min(frames, (b + 2 * CX_FFT) // CX_HOP + 2)) for a, b in swin]
        checks[-1] = (checks[-1][0], CX_FCAP)
        xf = X // CX_HOP
        assert any(a < xf < b for a, b in checks) and (frames - 1) * CX_HOP + CX_FFT > X and checks[1][0] > checks[0][1]
        assert (_zero_sign(_u32(lines(xf, xf + 20))) != _zero_sign(_u32(lines(0, 20)))).mean() > 0.9
        assert not np.isnan(lines(xf, xf + 8)).any()
        src = _line(buf, 0)
        dst = buf[CAP:CAP + CX_ELEMS].view(F, CX_FCAP)
        _load(src, N, [(a, d) for (a, _), d in zip(swin, data)])
        clock = _Clock("k_spec_complex " + name)
        for route in routes:
            sp.set_route(route)
            _ints(dst).fill_(SENT_I)
            clock.lap("load")
            out, got_frames = sp.run(src.view(1, 1, CAP), [N], out=dst.view(1, 1, F, CX_FCAP))
            clock.lap("route %d" % route)
            assert sp.last_route() == route and got_frames.tolist() == [frames]
            _verify_lines(dst, frames, checks, lines, _same_zero_sign)
            clock.lap("verify")
        clock.done()
        for (a, _), d in zip(swin, data):                              # the source was only read
            assert np.array_equal(_read(src, a, a + len(d))[:, 0], _u32(d))
    finally:
        sp.close()


IS_W = 8192                            # samples per window of the destination that the source's frame windows reach
IT_T = (1 << 24) + (1 << 12) + 1       # frames of the interleaved case: 2 channels of 2^31 + 2^19 samples, 2^32 + 2^20 elements
# name -> (channels, frames, samples written per channel, frames per tile (None: the plan's), routes)
ISTFT = {
    "istft_256_128_planar": (1, CX_T, N, None, (0, 1)),
    "istft_256_128_interleaved": (2, IT_T, (IT_T - 1) * CX_HOP + 3, None, (0, 1)),       # (p - pad) x d.el crosses while p does not
    "istft_256_128_tile_frames_1": (1, CX_T, N, 1, (0,)),                               # more tiles than one launch takes: tile0 != 0
}


@pytest.mark.parametrize("name", list(ISTFT))
def test_k_istft_inside_a_row_past_2_to_the_32(buf, name):
    """L[istft_256_128]: random spectral data in the frame windows that map to the three sample windows, +0.0 elsewhere, ->
    a PCM row.  t.s0 = (tile0 + bx) x span, tf0 and the frame index t.tf0 + fc cross with the sample; r0 is what is left of s0
    once tf0 x hop is taken off; the store (p - pad) x d.el crosses in the interleaved layout at half the sample index"""
    from lewton_amd.rows import InverseSpectrogram
    C, T, length, m1, routes = ISTFT[name]
    inv = InverseSpectrogram(CX_FFT, CX_HOP)
    try:
        natural = inv.out_len(T)
        xs = X // C                                                    # the sample (per channel) whose element lies at 2^32
        fcap = CX_ELEMS // (C * CX_LINES)
        cap = CAP // C
        assert natural == (T - 1) * CX_HOP and natural < length <= cap and length * C > X and T < fcap and 2 * inv.bins == CX_LINES
        assert (length > X) == (C == 1)
        if m1:
            inv.set_tile_frames(m1)
        span = inv.tile_frames * CX_HOP
        tiles = -(-(CX_FFT // 2 + length) // span)
        assert (tiles > 0xFFFFFF) == bool(m1) and (not m1 or (0xFFFFFF * span < X < tiles * span))
        G, w2 = inv.basis(), inv.window2()
        fwin = [(max(0, a // CX_HOP - 2), min(T, b // CX_HOP + 3)) for a, b in _windows(natural, IS_W, xs)]
        rng = np.random.default_rng(60 + len(name))
        data = [rng.uniform(-1, 1, (C, CX_LINES, b - a)).astype(F32) for a, b in fwin]
        rows = [SparseRow(T, [(a, d[c]) for (a, _), d in zip(fwin, data)], CX_LINES) for c in range(C)]
        m = 2 * CX_FFT
        checks = [(max(0, a * CX_HOP - m), min(cap, b * CX_HOP + m)) for a, b in fwin]
        checks[-1] = (checks[-1][0], cap)
        memo = {}

        def want(a, b):
            if (a, b) not in memo:
                memo[a, b] = np.stack([_u32(IM.window_rows(G, w2, r, a, b, T, CX_FFT, CX_HOP, True, length, np.full(b - a, SENT_F, F32))) for r in rows], axis=1)
            return memo[a, b]
        assert any(a < xs < b for a, b in checks) and checks[1][0] > checks[0][1] and checks[2][0] > checks[1][1]
        here, there = _zero_sign(want(xs, xs + 100)), _zero_sign(want(0, 100))
        assert (here != there).mean() > 0.9 and (here != 0).mean() > 0.9
        src = buf[CAP:CAP + C * CX_LINES * fcap].view(C * CX_LINES, fcap)
        dst = _line(buf, 0, cap, C)
        clock = _Clock("k_istft " + name)
        src[:, :T].zero_()
        _ints(src[:, T:]).fill_(SENT_I)
        for (a, _), d in zip(fwin, data):
            _ints(src[:, a:a + d.shape[2]]).copy_(torch.from_numpy(d.reshape(C * CX_LINES, -1).view(np.int32)))
        for route in routes:
            inv.set_route(route)
            _ints(dst).fill_(SENT_I)
            clock.lap("load")
            shape_d = (1, cap, C) if C > 1 else (1, 1, cap)
            out, got = inv.run(src.view(1, C, CX_LINES, fcap), [T], lengths=[length], out=dst.view(shape_d), samples="f32_interleaved" if C > 1 else "f32")
            clock.lap("route %d" % route)
            assert inv.last_route() == route and got.tolist() == [length]
            _verify(dst, length, checks, want, mid_zero, _same_zero_sign)
            clock.lap("verify")
        clock.done()
        for (a, _), d in zip(fwin, data):                              # the source was only read
            assert np.array_equal(_ints(src[:, a:a + d.shape[2]]).cpu().numpy().view(np.uint32), _u32(d.reshape(C * CX_LINES, -1)))
    finally:
        inv.close()
