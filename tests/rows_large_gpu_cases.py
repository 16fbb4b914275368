"""The rows chain past element 2^32 of a tensor and past 65535 rows of a call, on the GPU: k_rows_mix, k_resample, k_spec,
k_spec_complex, k_istft, k_feat, k_norm, k_cep, k_slide, k_select_count and k_select.  The cases of tests/test_gpu_rows_large.py, which runs this file with pytest in a process of its own, torch
imported first (tests/rows_gpu_cases.py says why).

Part A.  Every kernel forms its addresses from several products (row x row size, channel x channel size, line x line_el, position x
ch for the interleaved layouts, o x row_capacity), each with casts of its own.  One flat allocation of 2 x 18 x (2^28 + 8) floats
(38.7 GB) is made once and re-viewed per case as [R][C][F][cap] with cap = 2^28 or 2^28 + 5 (lines off the 16-byte boundaries), so
that 17 lines ("slots") of cap elements exist: slot 9 starts past 2^31, slot 16 at or past 2^32 -- the alias of slot 0 in 32 bits.
Slot 16 is reached through each index of the layout in a case of its own.  Only a window [0, W) of every slot is ever touched: the
lengths are a few hundred to a few thousand, the work is tiny, the offsets are huge.  Before a call the window of EVERY slot of the
destination holds the sentinel 0x7FC0DEAD and the source holds it from each length on; afterwards the live slots equal the model
bit for bit up to their fill end, everything else is still the sentinel (slot 0 is where a truncated offset lands; it holds other
data than slot 16 where it is live), and a source that is not the destination is unchanged.  Python integers assert that the last
live element lies past 2^32, and one past 2^31, so no case can quietly stop crossing.  The byte mask of k_select is a uint8 tensor
of its own, allocated in the case and freed behind it (4.6 GB for 17 rows of 2^28 + 5 bytes): 43.2 GB of device memory at the peak.

Part B.  Every entry point cuts a call into launches of 65535 rows and hands row0 to the kernel, which adds it to blockIdx.z for the
row record, the tensor offsets and the per-row scratch.  65 540 rows of a few dozen elements, a dozen of them live on both sides of
the cut, each with data and a length of its own: the live rows equal the model bit for bit, every other element of the destination
is still the sentinel (compared on the device).

The models are those of the other cases files (tests/cep_model.py, norm_model.py, feat_model.py, spec_model.py,
spec_reflect_model.py, istft_model.py, slide_model.py, select_model.py, the resampler's fold and the mix fold), evaluated over the
windows / the live rows only.  No tolerance anywhere."""
import torch  # noqa: F401  (first: see above)

import math
import time

import numpy as np
import pytest

import cep_model as CM
import feat_model as FM
import norm_model as NM
import rows_feat_gpu_cases as FC
import rows_istft_gpu_cases as IC
import rows_mix_gpu_cases as MX
import rows_resample_gpu_cases as RC
import rows_spec_gpu_cases as S
import select_model as SEL
import slide_model as SLM
import spec_model as SM
import spec_reflect_model as XR
from common import SETUPS
from rows_gpu_cases import _Cursor, _oracle_rows, _product, _streams

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
SENT = 0x7FC0DEAD
SENT_F = np.array(SENT, np.uint32).view(F32)
SENT_I = int(np.array(SENT, np.uint32).view(np.int32))
CAP = 1 << 28
ODD = CAP + 5                          # lines start at every residue against 16 bytes
HALF = 18 * (CAP + 8)                  # elements of one buffer: 18 slots (k_cep's 6 x 3 destination lines) of either capacity
MASK_BYTES = 17 * ODD                  # the largest mask of a k_select case: uint8 [17][1][2^28 + 5], a tensor of its own per case
KIND = {None: NM.NONE, "std": NM.STD, "rms": NM.RMS, "peak": NM.PEAK}


# ---- part A: the buffers and their windows

class _Bufs:
    a = b = big = None


@pytest.fixture(scope="module")
def bufs():
    """one allocation for the whole file: .a and .b are its halves (source and destination), .big all of it (k_rows_mix)"""
    free, _ = torch.cuda.mem_get_info(0)
    if free < 2 * HALF * 4 + MASK_BYTES + (4 << 30):
        pytest.skip("less than %.1f GB of device memory free" % ((2 * HALF * 4 + MASK_BYTES + (4 << 30)) / 1e9))
    torch.cuda.reset_peak_memory_stats(0)
    t0 = time.perf_counter()
    B = _Bufs()
    B.big = torch.empty(2 * HALF, dtype=torch.float32, device="cuda:0")
    B.a, B.b = B.big[:HALF], B.big[HALF:]
    yield B
    torch.cuda.synchronize()
    print("\n[rows_large] part A: %.1f s from the allocation on, peak device memory %.2f GB" % (
        time.perf_counter() - t0, torch.cuda.max_memory_allocated(0) / 1e9))
    B.a = B.b = B.big = None
    torch.cuda.empty_cache()


def _view(buf, shape):
    n = math.prod(shape)
    assert n <= buf.numel(), (shape, n, buf.numel())
    return buf[:n].view(shape)


def _win(v, W, itl=False):
    """the windows [0, W) of every line of a view, as int32; itl: of [R][cap][C]"""
    iv = v.view(torch.int32)
    return iv[:, :W, :] if itl else iv[..., :W]


def _put(v, x, itl=False):
    """host [..][W] (itl: [R][C][W]) -> the windows of v, by bits"""
    h = np.ascontiguousarray(x.transpose(0, 2, 1) if itl else x).view(np.int32)
    _win(v, x.shape[-1], itl).copy_(torch.from_numpy(h))


def _get(v, W, itl=False):
    """the windows of v as host float32 [..][W] (itl: as [R][C][W])"""
    h = _win(v, W, itl).cpu().numpy()
    return np.ascontiguousarray(h.transpose(0, 2, 1) if itl else h).view(F32)


def _sentinel(v, W, itl=False):
    _win(v, W, itl).fill_(SENT_I)


def _offset(shape, idx):
    """element offset of idx in a contiguous tensor, in Python integers"""
    off = 0
    for s, i in zip(shape, idx):
        assert 0 <= i < s
        off = off * s + i
    return off


def _assert_crosses(shape, last, itl=False):
    """last: elements written in the LAST line of the tensor; slot 9 is the line whose start lies 9 capacities in.  The last line's
    last written element lies past 2^32 and its window is the alias of slot 0's; a line in between starts past 2^31"""
    cap = shape[1] if itl else shape[-1]
    lines = math.prod(shape) // cap
    assert last >= 1
    if itl:                                                            # [R][cap][C]: the last row's sample last - 1, channel C - 1
        hi = _offset(shape, (shape[0] - 1, last - 1, shape[2] - 1))
        assert hi > 1 << 32 and _offset(shape, (shape[0] - 1, 0, 0)) >= 1 << 32, shape
        assert any(1 << 31 < _offset(shape, (r, 0, 0)) < 1 << 32 for r in range(shape[0])), shape
        return
    hi = _offset(shape, tuple(s - 1 for s in shape[:-1]) + (last - 1,))
    assert hi > 1 << 32 and any(1 << 31 < k * cap < 1 << 32 for k in range(lines)), shape
    by = [k for k, s in enumerate(shape[:-1]) if s > 1][0]            # the index of the layout this case crosses through:
    alone = tuple(s - 1 if k == by else 0 for k, s in enumerate(shape[:-1])) + (0,)
    assert _offset(shape, alone) >= 1 << 32, (shape, by)              # its own product reaches 2^32, with every other index at 0


def _row_map(R, hi, mid):
    """rows=: source row hi -> a low destination row (1), source row 0 -> destination row hi, mid -> mid; the empty rows take the
    destination rows that are left, in order"""
    m = {hi: 1, 0: hi, mid: mid}
    rest = [d for d in range(R) if d not in m.values()]
    out = [m[r] if r in m else rest.pop(0) for r in range(R)]
    assert sorted(out) == list(range(R))
    return out


def _lens(R, live, values):
    n = [0] * R
    for r, v in zip(live, values):
        n[r] = v
    return n


def _lines_case(bufs, sshape, dshape, x, inplace, call, model, same, whole=False):
    """one call of a [rows][C][F][cap] kernel: x host [rows][C][F][W] -> the windows of the source view; call(src, dst or None);
    model(destination windows before the call) -> the windows after it.  whole: the destination is more than a half, so it lies
    at the start of the whole allocation and the source behind it.  Returns what call returned"""
    W = x.shape[-1]
    if whole:
        assert not inplace
        dst = _view(bufs.big, dshape)
        src = _view(bufs.big[math.prod(dshape):], sshape)
    else:
        src = _view(bufs.a, sshape)
        dst = src if inplace else _view(bufs.b, dshape)
    _put(src, x)
    before = x
    if not inplace:
        _sentinel(dst, W)
        before = np.full(tuple(dshape[:-1]) + (W,), SENT_F, F32)
    torch.cuda.synchronize()
    res = call(src, None if inplace else dst)
    torch.cuda.synchronize()
    same(_get(dst, W), model(before), SENT)
    if not inplace:
        assert np.array_equal(_get(src, W).view(np.uint32), x.view(np.uint32)), "the source was written"
    return res


# geometry name -> (rows, channels, lines; live rows)
GEO = {"rows": (17, 1, 1, (0, 9, 16)), "channels": (1, 17, 1, (0,)), "lines": (1, 1, 17, (0,))}


# ---- A.1 k_cep

# name -> (source [R][C][n_in], n_out (None: the identity), order, live rows, capacity, lengths, fill_to of the live rows).  A row
# or a channel of the destination is n_out x (1 + order) lines, and 18 slots is what there is: through the row and the channel index
# the matrix goes with order 1 (nine rows of two lines), through the line index with order 2 (6 x 3 lines)
CEP = {
    "rows_identity_copy": ((17, 1, 1), None, 0, (0, 9, 16), CAP, (700, 300, 1031), (0, 310, 1040)),
    "rows_matrix_order1": ((9, 1, 1), 1, 1, (0, 5, 8), ODD, (700, 300, 1031), (705, 0, 1031)),       # [9][1][2]: row 8 holds slots 16 and 17
    "channels_identity_copy": ((1, 17, 1), None, 0, (0,), ODD, (777,), (790,)),
    "channels_matrix_order1": ((1, 9, 1), 1, 1, (0,), CAP, (777,), None),
    "lines_identity_copy": ((1, 1, 17), None, 0, (0,), CAP, (600,), (611,)),
    "lines_matrix_order2": ((1, 1, 17), 6, 2, (0,), ODD, (777,), (780,)),                              # 17 lines in, 6 x 3 out
    # the store's line is (level x n_out + q0) + j, q0 the first output of a group of 32, j < 32, each times line_el on its own.  The
    # cases above reach slot 16 by j (17 lines in one group) or by the sum (12 + 5); these by q0 = 32 at 2^27 + 3 frames per line
    # (the identity: the source's (q0 + j) x line_el too), and by level x n_out = 16 at 2^28 (32 lines: the whole allocation)
    "lines_second_group_matrix": ((1, 1, 2), 33, 0, (0,), (1 << 27) + 3, (777,), (780,)),
    "lines_second_group_identity": ((1, 1, 33), None, 0, (0,), 1 << 27, (600,), None),
    "lines_delta_level": ((1, 1, 2), 16, 1, (0,), CAP, (777,), (790,)),
}


@pytest.mark.parametrize("name", list(CEP))
def test_k_cep_past_2_to_the_32(bufs, name):
    from lewton_amd.rows import Cepstrum
    (R, C, n_in), n_out, order, live, cap, lens, fills = CEP[name]
    m = None if n_out is None else CM.matrix(n_out, n_in, 7) if n_in > 1 else np.full((n_out, 1), 0.75, F32)   # (CM.matrix's [0][0] is 0)
    cp = Cepstrum(n_in, m, order, 2)
    try:
        assert cp.tile_frames == 256 - 4 * order and max(lens) > 2 * cp.tile_frames
        n = _lens(R, live, lens)
        fill = None if fills is None else _lens(R, live, fills)
        W = max(max(n), max(fill or [0])) + 41
        x = CM.source(n, C, n_in, W, 900 + len(name))
        sshape, dshape = (R, C, n_in, cap), (R, C, cp.features, cap)
        _assert_crosses(dshape, max(n[-1], (fill or n)[-1]))
        if math.prod(sshape) > 1 << 32:
            _assert_crosses(sshape, n[-1])
        if "second_group" in name:
            assert cp.features == 33 and 32 * cap >= 1 << 32
        if name == "lines_delta_level":
            assert cp.n_out * cap >= 1 << 32 > (cp.n_out - 1) * cap
        _lines_case(bufs, sshape, dshape, x, False, lambda s, d: cp.run(s, n, out=d, fill_to=fill),
                    lambda before: CM.rows(x, n, fill, before, m, order, 2), CM.same_bits, whole=math.prod(dshape) > HALF)
        assert cp.last_launches() == 1
    finally:
        cp.close()


# ---- A.2 k_norm

# name -> (geometry, capacity, scope, scale, in place, want_stats, fill_to - n or None, squeeze to 3-D)
NORM = {
    "rows_scope_row_in_place": ("rows", CAP, "row", "std", True, True, None, False),
    "rows_scope_line": ("rows", ODD, "line", "peak", False, False, 9, False),
    "rows_waveform_3d": ("rows", ODD, "channel", "std", False, True, 3, True),
    "channels_scope_channel": ("channels", ODD, "channel", "rms", False, True, 5, False),
    "channels_scope_row_in_place": ("channels", CAP, "row", "std", True, False, None, False),
    "channels_waveform_3d_in_place": ("channels", CAP, "channel", "peak", True, True, 2, True),
    "lines_scope_line_in_place": ("lines", ODD, "line", "std", True, True, 7, False),
    "lines_scope_channel": ("lines", CAP, "channel", "std", False, True, None, False),
    "lines_scope_row": ("lines", ODD, "row", "rms", False, False, 4, False),
}


@pytest.mark.parametrize("name", list(NORM))
def test_k_norm_past_2_to_the_32(bufs, name):
    from lewton_amd.rows import Normalize
    geo, cap, scope, scale, inplace, want_stats, extra, squeeze = NORM[name]
    R, C, F, live = GEO[geo]
    nm = Normalize(True, scale, 1e-7, 0.5, scope)
    try:
        n = _lens(R, live, (700, 300, 1031) if len(live) == 3 else (1031,))
        fill = None if extra is None else [v + extra if v else 0 for v in n]
        W = max(n) + 41
        x = NM.source(n, C, F, W, 700 + len(name), offset=0.2)
        shape = (R, C, F, cap)
        _assert_crosses(shape, max(n[-1], (fill or n)[-1]))
        dev = (R, C, cap) if squeeze else shape                      # the 3-D waveform tensor is the same memory
        want = NM.rows(x, n, fill, x, 1, KIND[scale], NM.SCOPES[scope], 1e-7, 0.5)[1]

        def call(s, d):
            return nm.run(s.view(dev), n, out=None if d is None else d.view(dev), fill_to=fill, want_stats=want_stats)
        res = _lines_case(bufs, shape, shape, x, inplace, call,
                          lambda before: NM.rows(x, n, fill, before, 1, KIND[scale], NM.SCOPES[scope], 1e-7, 0.5)[0], NM.same_bits)
        if want_stats:
            NM.same_bits(res[1].cpu().numpy().reshape(want.shape), want)
        assert nm.last_launches() == 3
    finally:
        nm.close()


# ---- A.3 k_feat

# name -> (geometry, capacity, scope, top, in place, want_max, fill_to - n or None)
FEAT = {
    "rows_two_launches_in_place": ("rows", CAP, "row", 8.0, True, True, 6),
    "rows_one_launch": ("rows", ODD, "row", float("inf"), False, False, 3),
    "rows_scope_channel": ("rows", ODD, "channel", 8.0, False, True, None),
    "channels_scope_channel": ("channels", ODD, "channel", 8.0, False, True, 5),
    "channels_scope_row_in_place": ("channels", CAP, "row", 8.0, True, False, None),
    "channels_one_launch_in_place": ("channels", CAP, "channel", float("inf"), True, False, 9),
    "lines_scope_row": ("lines", ODD, "row", 8.0, False, True, 7),
    "lines_scope_channel_in_place": ("lines", CAP, "channel", 8.0, True, False, 2),
    "lines_one_launch": ("lines", CAP, "row", float("inf"), False, False, None),
}


@pytest.mark.parametrize("name", list(FEAT))
def test_k_feat_past_2_to_the_32(bufs, name):
    from lewton_amd.rows import LogCompress
    geo, cap, scope, top, inplace, want_max, extra = FEAT[name]
    R, C, F, live = GEO[geo]
    lc = LogCompress("log10", 1e-10, top, 4.0, 0.25, scope)
    try:
        n = _lens(R, live, (700, 300, 1031) if len(live) == 3 else (1031,))
        fill = None if extra is None else [v + extra if v else 0 for v in n]
        W = max(n) + 41
        x = FM.source(n, C, F, W, 1e-10, 300 + len(name))
        x[x > 1e30] = 1.0                                                # (FLT_MAX in every scope would clamp nearly everything to one value)
        shape = (R, C, F, cap)
        _assert_crosses(shape, max(n[-1], (fill or n)[-1]))
        args = (FM.LOG10, FM.ROW if scope == "row" else FM.CHANNEL, 1e-10, top, 4.0, 0.25)
        res = _lines_case(bufs, shape, shape, x, inplace, lambda s, d: lc.run(s, n, out=d, fill_to=fill, want_max=want_max),
                          lambda before: FM.rows(x, n, fill, before, *args)[0], FM.same_bits)
        if want_max:
            FM.same_bits(res[1].cpu().numpy(), FM.rows(x, n, fill, x, *args)[1])
        assert lc.last_launches() == (1 if top == float("inf") and not want_max else 2)
    finally:
        lc.close()


# ---- A.4 k_spec

# name -> (source [R][C], interleaved, live rows, capacity, mel bands (None: the power spectrum), pad mode, source in the large
# buffer).  n_fft = 32, hop = 8: 17 bins; mel 1 makes one line per channel, so that rows and channels alone reach slot 16
SPEC = {
    "rows_mel1_zero": ((17, 1), False, (0, 9, 16), CAP, 1, "zero", True),                  # source and destination cross by the row
    "rows_mel1_reflect": ((17, 1), False, (0, 9, 16), ODD, 1, "reflect", True),
    "channels_mel1_reflect": ((1, 17), False, (0,), ODD, 1, "reflect", True),              # ... by the channel
    "channels_mel1_zero": ((1, 17), False, (0,), CAP, 1, "zero", True),
    "interleaved_rows_mel1_zero": ((9, 2), True, (0, 5, 8), ODD, 1, "zero", True),         # [9][cap][2]: row 8 holds slots 16 and 17
    "lines_power_reflect": ((1, 1), False, (0,), ODD, None, "reflect", False),             # the power store: bin x d_line
    "lines_power_zero": ((1, 1), False, (0,), CAP, None, "zero", False),
    "lines_mel17_zero": ((1, 1), False, (0,), ODD, 17, "zero", False),                     # the mel store: q x d_line
    "lines_mel17_reflect": ((1, 1), False, (0,), CAP, 17, "reflect", False),
}


def _spec_want(sp, mel, x, lengths, rows, n_dst, W):
    if sp.pad_mode == "zero":
        return S._expected(sp, mel, x, lengths, rows, n_dst, W)
    by_src = FC._expected_reflect(sp, mel, x, lengths, len(lengths), W)
    want = np.full((n_dst,) + by_src.shape[1:], SENT_F, F32)
    for r, d in enumerate(rows):
        want[d] = by_src[r]
    return want


def _same_spec(got, want):
    """spec_model.same_bits (-0 counts as +0), and the sentinel exactly where the model leaves it"""
    SM.same_bits(got, want)
    assert np.array_equal(got.view(np.uint32) == SENT, want.view(np.uint32) == SENT)


@pytest.mark.parametrize("name", list(SPEC))
def test_k_spec_past_2_to_the_32(bufs, name):
    from lewton_amd.rows import Spectrogram, mel_filterbank
    (R, C), itl, live, cap, n_mels, pad, big_src = SPEC[name]
    mel = None if n_mels is None else mel_filterbank(16000, 32, n_mels)
    sp = Spectrogram(32, 8, mel=mel, pad_mode=pad)
    try:
        assert sp.tile_frames == 32 and sp.features == (n_mels or 17)
        lengths = _lens(R, live, (700, 333, 1001))
        rows = _row_map(R, live[2], live[1]) if len(live) == 3 else None
        Ws = max(lengths) + 41
        Wd = sp.frames(max(lengths)) + 9
        assert min(sp.frames(v) for v in lengths if v) > sp.tile_frames
        x = S._source(lengths, C, Ws, 40 + len(name))
        scap = cap if big_src else Ws
        sshape = (R, scap, C) if itl else (R, C, scap)
        dshape = (R, C, sp.features, cap)
        _assert_crosses(dshape, sp.frames(lengths[(rows or [0]).index(R - 1)]))
        if big_src:
            _assert_crosses(sshape, lengths[-1], itl)
        src, dst = _view(bufs.a, sshape), _view(bufs.b, dshape)
        _put(src, x, itl)
        want = _spec_want(sp, mel, x, lengths, rows or list(range(R)), R, Wd)
        for route in (0, 1):
            sp.set_route(route)
            _sentinel(dst, Wd)
            torch.cuda.synchronize()
            out, frames = sp.run(src, lengths, out=dst, rows=rows, samples="f32_interleaved" if itl else "f32")
            torch.cuda.synchronize()
            assert out is dst and sp.last_route() == route and frames.tolist() == [sp.frames(v) for v in lengths]
            _same_spec(_get(dst, Wd), want)
        assert np.array_equal(_get(src, Ws, itl).view(np.uint32), x.view(np.uint32)), "the source was written"
    finally:
        sp.close()


# ---- A.5 k_resample

def _pcm(lengths, ch, W, seed):
    """host [row][ch][W]: noise in every channel, zeros of both signs and a run of subnormals in it, the sentinel beyond each length"""
    rng = np.random.default_rng(seed)
    x = np.full((len(lengths), ch, W), SENT_F, F32)
    for r, n in enumerate(lengths):
        v = rng.uniform(-1, 1, (ch, n)).astype(F32)
        v[:, 5::11] *= F32(-0.0)
        v[:, 3::13] *= F32(1e-39)
        x[r, :, :n] = v
    return x


def _rs_tile(rs, taps_in_lds=True):
    """outputs per workgroup, by the plan csrc/lw_resample.hpp writes down: 512 lanes, 20480 floats of LDS, 8 passes at most"""
    orig, new, K = rs.orig, rs.new, rs.taps_per_phase
    if orig == new:
        return 2048
    up4 = lambda v: (v + 3) & ~3
    span = lambda j, m: up4(m * j * orig + K - 1)
    room, table = 20480, up4(new * K)
    if taps_in_lds and table + span(1, 1) <= room:
        room -= table
    elif span(1, 1) > room:
        return 512
    j = 4 if span(4, 1) <= room else 2 if span(2, 1) <= room else 1
    best, blocks, m = None, 1, 1
    while span(j, m) <= room:
        units = m * new
        cost = -(-units // 512) * 512 * 65536 // units
        if best is None or cost < best:
            best, blocks = cost, m
        if units >= 8 * 512:
            break
        m += 1
    return blocks * j * new


# name -> (source [R][C], interleaved, live rows, capacity, (in_rate, out_rate), filter, route, rows= map)
RESAMPLE = {
    "rows_lds": ((17, 1), False, (0, 9, 16), CAP, (44100, 16000), {}, 0, True),
    "rows_lds_odd_capacity": ((17, 1), False, (0, 9, 16), ODD, (16000, 44100), {}, 0, False),
    "rows_global_taps": ((17, 1), False, (0, 9, 16), ODD, (48000, 16000), {"window": "kaiser", "zeros": 16}, 1, True),
    "rows_all_global": ((17, 1), False, (0, 9, 16), CAP, (2000, 1), {}, 2, True),
    "rows_copy": ((17, 1), False, (0, 9, 16), ODD, (44100, 44100), {}, 3, True),
    "channels_lds": ((1, 17), False, (0,), ODD, (44100, 48000), {}, 0, False),
    "channels_global_taps": ((1, 17), False, (0,), CAP, (22050, 44100), {}, 1, False),
    "interleaved_rows_lds": ((9, 2), True, (0, 5, 8), ODD, (48000, 16000), {}, 0, True),
    "interleaved_rows_copy": ((9, 2), True, (0, 5, 8), CAP, (16000, 16000), {}, 3, True),
}


@pytest.mark.parametrize("name", list(RESAMPLE))
def test_k_resample_past_2_to_the_32(bufs, name):
    from lewton_amd import _native as N
    from lewton_amd.rows import Resampler
    (R, C), itl, live, cap, pair, filt, route, mapped = RESAMPLE[name]
    rs = Resampler(pair[0], pair[1], **filt)
    try:
        if route == 1:
            N.lw_resampler_set_taps_in_lds(rs._h, 0)
        tile = _rs_tile(rs, route != 1)
        longest = -(-(tile + 77) * rs.orig // rs.new)                  # the last live row: two tiles
        short = {0: (1000, rs.half_width - 1), 1: (1000, rs.half_width - 1), 2: (9001, 3001), 3: (1000, 300)}[route]
        lengths = _lens(R, live, short + (longest,) if len(live) == 3 else (longest,))
        assert rs.out_len(longest) > tile and max(lengths) == longest < 1 << 21
        rows = _row_map(R, live[2], live[1]) if mapped else None
        Ws, Wd = longest + 41, rs.out_len(longest) + 41
        x = _pcm(lengths, C, Ws, 60 + len(name))
        sshape = (R, cap, C) if itl else (R, C, cap)
        _assert_crosses(sshape, lengths[-1], itl)
        _assert_crosses(sshape, rs.out_len(lengths[(rows or list(range(R))).index(R - 1)]), itl)     # the destination: the same shape
        src, dst = _view(bufs.a, sshape), _view(bufs.b, sshape)
        _put(src, x, itl)
        _sentinel(dst, Wd, itl)
        torch.cuda.synchronize()
        assert rs.run(src, lengths, out=dst, rows=rows, samples="f32_interleaved" if itl else "f32") is dst
        torch.cuda.synchronize()
        assert rs.last_route == route
        want = RC._expected(rs, x, lengths, rows or list(range(R)), R, Wd)
        RC._same(_get(dst, Wd, itl).view(np.int32), want)
        assert np.array_equal(_get(src, Ws, itl).view(np.uint32), x.view(np.uint32)), "the source was written"
    finally:
        rs.close()


# ---- A.6 k_rows_mix

MIX8 = [[1, 0], [0, 1], [0.5, 0.5], [-1, 1], [0.25, 0.75], [0.70710678, 0], [0, -0.5], [0.3, 0.3]]       # not a routing matrix
MIX2 = [[0.5, 0.5], [1, -1]]
# name -> (format, rows, capacity, matrix, live rows).  Five rows of [2][2^29], not three: 3 x 2 x 2^29 floats end at 3 x 2^30,
# short of 2^32 (the i16 case of tests/rows_gpu_cases.py has [3][2][2^30]); row 4 starts at 2^32 exactly, row 2 at 2^31
MIX = {
    "planar_out_channels_vector": ("f32", 1, (1 << 29) + 4, MIX8, (0,)),                    # byte offsets o x row_capacity x 4: 16-byte stores
    "planar_out_channels_scalar": ("f32", 1, 5 * (1 << 27) + 5, MIX8, (0,)),                # o x row_capacity itself passes 2^32 at o = 7
    "planar_rows": ("f32", 5, 1 << 29, MIX2, (0, 2, 4)),
    "interleaved_rows": ("f32_interleaved", 5, 1 << 29, MIX2, (0, 2, 4)),
}


@pytest.mark.parametrize("name", list(MIX))
def test_k_rows_mix_past_2_to_the_32(bufs, name):
    """stereo streams through Rows.synth(mix=) into the END of their rows, as the k_rows case of tests/rows_gpu_cases.py does:
    the windows at both ends of every row and channel hold the sentinel before, the oracle's rows folded by the matrix behind"""
    from lewton_amd.batch import Batch
    from lewton_amd.rows import Rows
    fmt, R, cap, matrix, live = MIX[name]
    itl = fmt.endswith("interleaved")
    m = np.asarray(matrix, F32)
    oc = m.shape[0]
    setup = SETUPS["stereo"]()
    audio, ident, st = _product(setup)
    dec = audio.decoder_for(ident, st)
    streams = _streams(setup, "LLSL", [9, 8, 7][:len(live)], seed=19)
    want_rows = _oracle_rows(setup, streams, "f32")
    totals = [row.shape[1] for row, _ in want_rows]
    W = max(totals) + 64
    shape = (R, cap, oc) if itl else (R, oc, cap)
    tensor = _view(bufs.big, shape)
    iv = tensor.view(torch.int32)
    head, tail = (iv[:, :W, :], iv[:, cap - W:, :]) if itl else (iv[..., :W], iv[..., cap - W:])
    head.fill_(SENT_I)
    tail.fill_(SENT_I)
    last = (R - 1, cap - 1, oc - 1) if itl else (R - 1, oc - 1, cap - 1)
    assert _offset(shape, last) > 1 << 32
    if R > 1:
        assert _offset(shape, (live[1], 0, 0)) >= 1 << 31 and _offset(shape, (live[2], 0, 0)) >= 1 << 32
    else:
        assert 1 << 31 < _offset(shape, (0, 4, 0)) < 1 << 32 and ((oc - 1) * cap > 1 << 32) == ("scalar" in name)
    items = [(s, t) for s in range(len(streams)) for t in range(len(streams[s]))]
    bt, rows = Batch(dec, len(items), fmt), Rows(dec, len(items), fmt)
    try:
        pws = [audio.PreviousWindowRight() for _ in streams]
        res = bt.entropy([(streams[s][t], pws[s]) for s, t in items], n_threads=1)
        bt.upload()
        cur = _Cursor(len(streams))
        places = []
        for (s, t), (status, k, off) in zip(items, res):
            assert status == 0
            row, sk, kp, t0 = cur.place(s, k)
            places.append((live[s], sk, kp, t0 + cap - totals[s] if kp else 0))       # every stream ends exactly at the end of its row
        torch.cuda.synchronize()
        rows.synth(bt, places, tensor, mix=m)
        torch.cuda.synchronize()
        assert bt.device_status() == 0 and rows.last_copied_elems == sum(totals) * oc
    finally:
        bt.close()
        rows.close()
    got_head, got_tail = head.cpu().numpy(), tail.cpu().numpy()
    if itl:
        got_head, got_tail = got_head.transpose(0, 2, 1), got_tail.transpose(0, 2, 1)
    want = np.full((R, oc, W), SENT_I, np.int32)
    for s, (row, _) in enumerate(want_rows):
        want[live[s], :, W - totals[s]:] = MX._fold(m, row).view(np.int32)
    same = got_tail == want
    assert same.all(), (int((~same).sum()), np.argwhere(~same)[:4].tolist())
    assert (got_head == SENT_I).all(), "written at the start of a row: a destination offset was truncated to 32 bits"
    assert not (want[live[-1]] == SENT_I).all()


# ---- A.7 k_slide

def _sl_lines(F, W, tile):
    """lines a workgroup of k_slide stages at a time, by the plan csrc/lw_slide.hpp writes down: 64 KiB of LDS, 16 lines at most"""
    cols = (tile + W + 30) & ~15
    per_line = (cols + cols // 32 + 1) * 4 + cols // 16 * 16
    lines = min(16, 65536 // per_line)
    return min(F, lines & ~3 if lines >= 4 else lines)


WIDE = 18 << 24                        # a capacity at which 16 lines are 18 slots: line 15 starts past 2^32, inside ONE group of lines
SL_BIG, SL_SMALL = (300, 100, 1, 1), (8, 3, 0, 0)                     # (W, min, center, norm_vars)
# name -> (geometry, or (rows, channels, lines; live rows); capacity; configuration; fill_to - n or None).  t.at is ((row x ch + by)
# x F + f0) x line_el, f0 the first line of a group of `lines` lines; the lines of a group lie g x line_el behind it, g < 16.  The three
# geometries reach slot 16 by the row, the channel and (17 lines in two groups of 16) by f0 = 16; second_group by f0 = 32 at 2^27
# frames per line; in_group by g = 15 at WIDE
SLIDE = {
    "rows_centred_vars": ("rows", CAP, SL_BIG, 9),
    "rows_causal": ("rows", ODD, SL_SMALL, None),
    "channels_centred_vars": ("channels", ODD, SL_BIG, None),
    "channels_causal": ("channels", CAP, SL_SMALL, 5),
    "lines_centred_vars": ("lines", ODD, SL_BIG, 7),
    "lines_causal": ("lines", CAP, SL_SMALL, None),
    "lines_second_group_centred_vars": ((1, 1, 33, (0,)), 1 << 27, SL_BIG, 4),
    "lines_second_group_causal": ((1, 1, 33, (0,)), 1 << 27, SL_SMALL, None),
    "lines_in_group_centred_vars": ((1, 1, 16, (0,)), WIDE, SL_BIG, None),
    "lines_in_group_causal": ((1, 1, 16, (0,)), WIDE, SL_SMALL, 3),
}
SL_TILE = 256                          # frames of a tile here (the default is 1024): rows of 600 to 1031 frames span three to five


def _geometry(geo):
    return GEO[geo] if isinstance(geo, str) else geo


@pytest.mark.parametrize("name", list(SLIDE))
def test_k_slide_past_2_to_the_32(bufs, name):
    from lewton_amd.rows import SlidingCMVN
    geo, cap, cfg, extra = SLIDE[name]
    R, C, F, live = _geometry(geo)
    sl = SlidingCMVN(cfg[0], cfg[1], bool(cfg[2]), bool(cfg[3]))
    try:
        sl.set_tile_frames(SL_TILE)
        n = _lens(R, live, (700, 600, 1031) if len(live) == 3 else (1031,))
        assert sl.tile_frames == SL_TILE and min(v for v in n if v) > 2 * SL_TILE
        fill = None if extra is None else [v + extra if v else 0 for v in n]
        W = max(n) + 41
        x = SLM.source(n, C, F, W, 500 + len(name))
        shape = (R, C, F, cap)
        _assert_crosses(shape, max(n[-1], (fill or n)[-1]))
        lines = _sl_lines(F, cfg[0], SL_TILE)
        assert lines == min(F, 16)
        if "second_group" in name:
            assert F == 2 * lines + 1 and 2 * lines * cap >= 1 << 32 > (2 * lines - 1) * cap     # f0 x line_el on its own
        if "in_group" in name:
            assert F == lines and (F - 1) * cap >= 1 << 32                                       # g x line_el on its own
        _lines_case(bufs, shape, shape, x, False, lambda s, d: sl.run(s, n, out=d, fill_to=fill),
                    lambda before: SLM.rows(x, n, fill, before, cfg[0], cfg[1], bool(cfg[2]), bool(cfg[3])), SLM.same_bits)
        assert sl.last_launches() == 1
    finally:
        sl.close()


# ---- A.8 k_select_count and k_select

# name -> (geometry, capacity, mask kind, tile, fill_to - n or None).  The mask is [rows][ch][capacity] BYTES: t.mask_at = (row x ch +
# by) x line_el reaches 2^32 through rows and channels only, t.at as k_slide's (groups of 16 lines whatever the tile)
SELECT = {
    "rows_random_256": ("rows", CAP, "random", 256, 9),
    "rows_last_1024": ("rows", ODD, "last", 1024, None),
    "channels_random_1024": ("channels", ODD, "random", 1024, None),
    "channels_last_256": ("channels", CAP, "last", 256, 5),
    "lines_random_256": ("lines", ODD, "random", 256, 7),
    "lines_last_1024": ("lines", CAP, "last", 1024, None),
    "lines_in_group_random_1024": ((1, 1, 16, (0,)), WIDE, "random", 1024, 3),
}


@pytest.mark.parametrize("name", list(SELECT))
def test_k_select_past_2_to_the_32(bufs, name):
    """the kept frames of every line at its front, the zeroed tail, the sentinel behind it, and K of every row and channel"""
    from lewton_amd.rows import SelectFrames
    geo, cap, kind, tile, extra = SELECT[name]
    R, C, F, live = _geometry(geo)
    se = SelectFrames()
    dm = None
    try:
        se.set_tile_frames(tile)
        n = _lens(R, live, (2 * tile + 188, 2 * tile + 60, 2 * tile + 519) if len(live) == 3 else (2 * tile + 519,))
        assert se.tile_frames == tile and min(v for v in n if v) > 2 * tile
        fill = None if extra is None else [v + extra if v else 0 for v in n]
        W = max(n) + 41
        x = SEL.source(n, C, F, W, 600 + len(name))
        mask = SEL.mask(kind, n, C, W, 31 + len(name))
        shape, mshape = (R, C, F, cap), (R, C, cap)
        _assert_crosses(shape, max(n[-1], (fill or n)[-1]))
        assert math.prod(mshape) <= MASK_BYTES
        if R * C > 1:
            _assert_crosses(mshape, n[-1])                               # the mask's own product, in bytes
        if "in_group" in name:
            assert F == 16 and (F - 1) * cap >= 1 << 32
        dm = torch.empty(mshape, dtype=torch.uint8, device="cuda:0")
        dm[..., :W].copy_(torch.from_numpy(mask))
        want_k = SEL.rows(x, mask, n, fill, np.zeros((R, C, F, W), F32))[1]
        out, counts = _lines_case(bufs, shape, shape, x, False, lambda s, d: se.run(s, n, dm, out=d, fill_to=fill),
                                  lambda before: SEL.rows(x, mask, n, fill, before)[0], lambda g, w, s: SEL.same_bits(g, w))
        assert se.last_launches() == 2 and counts.dtype == torch.int64
        assert np.array_equal(counts.cpu().numpy(), want_k) and (want_k[-1, -1] == 1 if kind == "last" else want_k[-1, -1] > tile)
        assert np.array_equal(dm[..., :W].cpu().numpy(), mask), "the mask was written"
    finally:
        se.close()
        dm = None
        torch.cuda.empty_cache()


# ---- A.9 k_istft

# name -> (source [R][C] of 18 lines, frame capacity, destination rows, capacity, interleaved destination, live source rows,
# (win_length, hop, window, center), lengths longer than natural by (None: the natural lengths), rows= map).  n_fft = 16: 2 B = 18 lines,
# a half of the buffer exactly.  t.s_at = (row0 + bz) x s_row + by x s_ch, lc x s_line, t.d_at = dst_row x d.row + by x d.ch
IS_HANN, IS_RECT = (16, 4, "hann"), (16, 16, "rect")
ISTFT = {
    "lines_hann": ((1, 1), CAP, 1, CAP, False, (0,), IS_HANN + (True,), None, None),                     # line 16, im[7], starts at 2^32
    "lines_rect_uncentred": ((1, 1), CAP, 1, ODD, False, (0,), IS_RECT + (False,), 9, None),
    "rows_hann": ((16, 1), 1 << 24, 17, CAP, False, (0, 8, 15), IS_HANN + (True,), 7, {15: 16, 0: 15, 8: 9}),  # source row 15 -> row 16
    "rows_hann_uncentred": ((16, 1), 1 << 24, 17, ODD, False, (0, 8, 15), IS_HANN + (False,), None, {15: 16, 0: 15, 8: 1}),
    "interleaved_rows_hann": ((8, 2), 1 << 24, 9, ODD, True, (0, 4, 7), IS_HANN + (True,), 5, {7: 8, 0: 7, 4: 1}),
    "channels_hann": ((1, 17), 15_000_001, 1, CAP, False, (0,), IS_HANN + (True,), None, None),            # channel 16 of both
    "channels_rect": ((1, 17), 15_000_001, 1, ODD, False, (0,), IS_RECT + (True,), 11, None),
}


@pytest.mark.parametrize("name", list(ISTFT))
def test_k_istft_past_2_to_the_32(bufs, name):
    """routes 0 and 1; the source lies in one half of the buffer, the destination in the other"""
    from lewton_amd.rows import InverseSpectrogram
    (R, C), fcap, n_dst, cap, itl, live, (win, hop, window, center), longer, rmap = ISTFT[name]
    inv = InverseSpectrogram(16, hop, win, window, center)
    try:
        m, B = inv.tile_frames, inv.bins
        assert 2 * B == 18
        frames = _lens(R, live, (300, 211, 333) if len(live) == 3 else (333,))
        nat = [inv.out_len(T) for T in frames]
        assert min(v for v in nat if v) > 2 * m * hop                    # more than two tiles of m x hop samples
        lens = None if longer is None else [v + longer if v else 0 for v in nat]
        rows = None
        if rmap is not None:
            rest = [d for d in range(n_dst) if d not in rmap.values()]
            rows = [rmap[r] if r in rmap else rest.pop(0) for r in range(R)]
            assert len(set(rows)) == R and rows[R - 1] == n_dst - 1
        Ws, Wd = max(frames) + 41, max(lens or nat) + 41
        x = IC._source(frames, C, B, Ws, 800 + len(name))
        sshape = (R, C, 18, fcap)
        dshape = (n_dst, cap, C) if itl else (n_dst, C, cap)
        assert math.prod(sshape) <= HALF and math.prod(dshape) <= HALF
        last_src = (rows or list(range(R))).index(n_dst - 1) if n_dst > 1 else 0
        if n_dst * C > 1:
            _assert_crosses(dshape, (lens or nat)[last_src], itl)
        if name.startswith("lines"):
            assert _offset(sshape, (0, 0, 16, 0)) == 1 << 32 and _offset(sshape, (0, 0, B + 7, 0)) == 1 << 32    # im[7]
        if name.startswith("interleaved"):                              # the row and the channel product together
            assert _offset(sshape, (R - 1, 1, 0, 0)) >= 1 << 32 > _offset(sshape, (R - 1, 0, 0, 0)) > 1 << 31
        else:
            _assert_crosses(sshape, frames[-1])
        src, dst = _view(bufs.a, sshape), _view(bufs.b, dshape)
        _put(src, x)
        want = IC._expected(inv, (inv.basis(), inv.window2()), x, frames, lens or nat, rows or list(range(R)), n_dst, Wd)
        assert not (want[n_dst - 1, C - 1].view(np.uint32) == SENT).all()
        for route in (0, 1):
            inv.set_route(route)
            _sentinel(dst, Wd, itl)
            torch.cuda.synchronize()
            out, got_lens = inv.run(src, frames, lengths=lens, out=dst, rows=rows, samples="f32_interleaved" if itl else "f32")
            torch.cuda.synchronize()
            assert out is dst and inv.last_route() == route and got_lens.tolist() == (lens or nat)
            IC.same_bits(_get(dst, Wd, itl), want)
        assert np.array_equal(_get(src, Ws).view(np.uint32), x.view(np.uint32)), "the source was written"
    finally:
        inv.close()


# ---- A.10 k_spec_complex

# name -> (source [R][C], live rows, frame capacity, pad mode, rows= map).  n_fft = 16, hop = 4: the destination is [R][C][18][frame
# capacity], re[j] on line j, im[j] on line 9 + j.  The store is (bin + line0) x d_line with line0 = 9 for the im lines; t.d_at =
# dst_row x d_row + by x d_ch with d_ch = 18 x d_line.  Nine rows or channels of 18 lines of 2^25 frames are 18 slots of 2^28 and
# half a slot more, so those destinations take the start of the whole allocation and the source lies behind them
COMPLEX = {
    "lines_zero": ((1, 1), (0,), CAP, "zero", False),
    "lines_reflect": ((1, 1), (0,), ODD, "reflect", False),
    "rows_zero": ((9, 1), (0, 5, 8), (1 << 25) + 5, "zero", True),
    "rows_reflect": ((9, 1), (0, 5, 8), 1 << 25, "reflect", True),
    "channels_zero": ((1, 9), (0,), 1 << 25, "zero", False),
    "channels_reflect": ((1, 9), (0,), (1 << 25) + 5, "reflect", False),
}


def _complex_want(sp, x, lengths, rows, n_dst, W):
    """float32 [n_dst][C][2 B][W]: the two chains of the contract over the frame matrices of the pad mode, the sentinel elsewhere"""
    basis = sp.basis()
    want = np.full((n_dst, x.shape[1], sp.features, W), SENT_F, F32)
    for r, n in enumerate(lengths):
        for c in range(x.shape[1]):
            if n == 0:
                assert sp.frames(0) == 0
                continue
            X = (XR.frame_matrix(x[r, c, :n], sp.n_fft, sp.win_length, sp.hop) if sp.pad_mode == "reflect" else
                 SM.frame_matrix(x[r, c, :n], sp.n_fft, sp.win_length, sp.hop, True))
            assert len(X) == sp.frames(n)
            want[rows[r], c, :, :len(X)] = IC._chains(basis, X).T
    return want


@pytest.mark.parametrize("name", list(COMPLEX))
def test_k_spec_complex_past_2_to_the_32(bufs, name):
    from lewton_amd.rows import Spectrogram
    (R, C), live, fcap, pad, mapped = COMPLEX[name]
    sp = Spectrogram(16, 4, pad_mode=pad, output="complex")
    try:
        B = sp.bins
        assert sp.tile_frames == 32 and sp.features == 18 and B == 9
        lengths = _lens(R, live, (700, 333, 1001))
        rows = _row_map(R, live[2], live[1]) if mapped else None
        Ws = max(lengths) + 41
        Wd = sp.frames(max(lengths)) + 9
        assert min(sp.frames(v) for v in lengths if v) > 2 * sp.tile_frames
        x = S._source(lengths, C, Ws, 70 + len(name))
        sshape, dshape = (R, C, Ws), (R, C, 18, fcap)
        _assert_crosses(dshape, sp.frames(lengths[(rows or [0]).index(R - 1)]))
        if name.startswith("lines"):                                    # every re line below 2^32, im[7] at or past it
            assert _offset(dshape, (0, 0, B - 1, fcap - 1)) < 1 << 32 <= _offset(dshape, (0, 0, B + 7, 0)) and 1 << 31 < _offset(dshape, (0, 0, B, 0))
        else:                                                           # t.d_at of the last row / channel on its own
            assert (R * C - 1) * 18 * fcap >= 1 << 32 and HALF < math.prod(dshape) < 2 * HALF - R * C * Ws
        dst = _view(bufs.big if math.prod(dshape) > HALF else bufs.b, dshape)
        src = _view(bufs.big[math.prod(dshape):] if math.prod(dshape) > HALF else bufs.a, sshape)
        src.view(torch.int32).copy_(torch.from_numpy(x.view(np.int32)))
        want = _complex_want(sp, x, lengths, rows or list(range(R)), R, Wd)
        for route in (0, 1):
            sp.set_route(route)
            _sentinel(dst, Wd)
            torch.cuda.synchronize()
            out, frames = sp.run(src, lengths, out=dst, rows=rows)
            torch.cuda.synchronize()
            assert out is dst and sp.last_route() == route and frames.tolist() == [sp.frames(v) for v in lengths]
            _same_spec(_get(dst, Wd), want)
        assert np.array_equal(src.cpu().numpy().view(np.uint32), x.view(np.uint32)), "the source was written"
    finally:
        sp.close()


# ---- part B: 65 540 rows in one call

NR = 65540
LIVE = [0, 1, 7, 32768, 40000, 65533, 65534, 65535, 65536, 65537, 65538, 65539]      # the second launch starts at row 65535
assert sum(r < 65535 for r in LIVE) == 7 and NR - 1 in LIVE


def _live_lengths(cap):
    """a length of its own per live row, the capacity among them"""
    return [cap - i for i in range(len(LIVE))]


def _all_rows(live_values):
    out = [0] * NR
    for r, v in zip(LIVE, live_values):
        out[r] = v
    return out


def _many(x_live, itl=False):
    """host [live][..] -> a device tensor [NR][..] that holds the sentinel in every other row; itl: [live][C][W] goes as [W][C]"""
    h = np.ascontiguousarray(x_live.transpose(0, 2, 1) if itl else x_live)
    t = S._filled((NR,) + h.shape[1:])
    t[LIVE] = torch.from_numpy(h).to("cuda:0")
    return t


def _rest_is_sentinel(t, dst_rows):
    """on the device: with the rows dst_rows blanked, every element of t is the sentinel"""
    iv = t.view(torch.int32).clone()
    iv[list(dst_rows)] = SENT_I
    assert bool((iv == SENT_I).all()), "written outside the live rows"


def _live_of(t, dst_rows, itl=False):
    h = t[list(dst_rows)].cpu().numpy()
    return np.ascontiguousarray(h.transpose(0, 2, 1) if itl else h)


@pytest.mark.parametrize("fmt", ["f32", "f32_interleaved"])
@pytest.mark.parametrize("pair", [(48000, 16000), (16000, 16000)])
def test_resample_65540_rows(pair, fmt):
    """[65540][2][48] -> [65540][2][17] in reversed row order, so a row's record, its source offset and its destination offset
    all differ; 3 -> 1 and the copy route"""
    from lewton_amd.rows import Resampler
    itl = fmt.endswith("interleaved")
    rs = Resampler(*pair)
    try:
        lens = _live_lengths(48)
        x, _ = RC._source(lens, 2, 48, False, 5)
        dcap = rs.out_len(48) + 1
        dst_rows = [NR - 1 - r for r in LIVE]
        src, dst = _many(x, itl), RC._filled((NR, 2, dcap), itl)
        rs.run(src, _all_rows(lens), out=dst, rows=[NR - 1 - r for r in range(NR)], samples=fmt)
        torch.cuda.synchronize()
        want = RC._expected(rs, x, lens, list(range(len(LIVE))), len(LIVE), dcap)
        RC._same(_live_of(dst, dst_rows, itl).view(np.int32), want)
        _rest_is_sentinel(dst, dst_rows)
    finally:
        rs.close()


@pytest.mark.parametrize("pad", ["zero", "reflect"])
@pytest.mark.parametrize("mel", [None, 5])
def test_spec_65540_rows(mel, pad):
    """[65540][2][40] -> [65540][2][9 or 5][12] in reversed row order, n_fft = 16, hop = 4, both routes"""
    from lewton_amd.rows import Spectrogram, mel_filterbank
    fb = None if mel is None else mel_filterbank(16000, 16, mel)
    sp = Spectrogram(16, 4, mel=fb, pad_mode=pad)
    try:
        lens = _live_lengths(40)
        x = S._source(lens, 2, 40, 9)
        fcap = sp.frames(40) + 1
        dst_rows = [NR - 1 - r for r in LIVE]
        src = _many(x)
        want = _spec_want(sp, fb, x, lens, list(range(len(LIVE))), len(LIVE), fcap)
        for route in (0, 1):
            sp.set_route(route)
            dst = S._filled((NR, 2, sp.features, fcap))
            _, frames = sp.run(src, _all_rows(lens), out=dst, rows=[NR - 1 - r for r in range(NR)])
            torch.cuda.synchronize()
            assert sp.last_route() == route and [int(frames[r]) for r in LIVE] == [sp.frames(v) for v in lens]
            _same_spec(_live_of(dst, dst_rows), want)
            _rest_is_sentinel(dst, dst_rows)
    finally:
        sp.close()


@pytest.mark.parametrize("inplace", [False, True])
@pytest.mark.parametrize("scope", ["row", "channel"])
def test_feat_65540_rows(scope, inplace):
    """[65540][2][3][24] with a finite top: both launches of both row ranges, the tiles' maxima of the second range at row0 onwards
    (part_at), d_max of every row"""
    from lewton_amd.rows import LogCompress
    lc = LogCompress("log10", 1e-10, 8.0, 4.0, 0.25, scope)
    try:
        n = _live_lengths(24)
        fill = [min(24, v + 2) for v in n]
        x = FM.source(n, 2, 3, 24, 1e-10, 77)
        x[x > 1e30] = 1.0
        for i in range(len(LIVE)):
            x[i, i % 2, i % 3, 0] = 10.0 ** (i + 4)                     # a maximum of its own in every live row, on both sides of the cut
        src = _many(x)
        dst = src if inplace else S._filled((NR, 2, 3, 24))
        _, mx = lc.run(src, _all_rows(n), out=None if inplace else dst, fill_to=_all_rows(fill), want_max=True)
        torch.cuda.synchronize()
        assert lc.last_launches() == 4
        before = x if inplace else np.full(x.shape, SENT_F, F32)
        want, Ms = FM.rows(x, n, fill, before, FM.LOG10, FM.ROW if scope == "row" else FM.CHANNEL, 1e-10, 8.0, 4.0, 0.25)
        FM.same_bits(_live_of(dst, LIVE), want, FM.SENT)
        _rest_is_sentinel(dst, LIVE)
        all_M = np.full((NR,) + Ms.shape[1:], F32(-10.0), F32)        # an empty row: LOG(floor)
        all_M[LIVE] = Ms
        FM.same_bits(mx.cpu().numpy(), all_M)
        assert len(set(np.asarray(Ms).ravel().tolist())) >= len(LIVE)
    finally:
        lc.close()


@pytest.mark.parametrize("scale", ["std", "peak"])
@pytest.mark.parametrize("scope", ["row", "channel", "line"])
def test_norm_65540_rows(scope, scale):
    """[65540][2][3][24]: the chunk lists (part_at), the scalars (sc_at) and the stats of the second row range"""
    from lewton_amd.rows import Normalize
    nm = Normalize(scale == "std", scale, 1e-7, 0.5, scope)
    try:
        n = _live_lengths(24)
        fill = [min(24, v + 2) for v in n]
        x = NM.source(n, 2, 3, 24, 78, offset=0.3)
        x[9, 1, 2, 3] = 1e4                                             # the peak of row 65537
        for inplace in (False, True):
            src = _many(x)
            dst = src if inplace else S._filled((NR, 2, 3, 24))
            _, st = nm.run(src, _all_rows(n), out=None if inplace else dst, fill_to=_all_rows(fill), want_stats=True)
            torch.cuda.synchronize()
            assert nm.last_launches() == 6
            before = x if inplace else np.full(x.shape, SENT_F, F32)
            want, stats = NM.rows(x, n, fill, before, int(scale == "std"), KIND[scale], NM.SCOPES[scope], 1e-7, 0.5)
            NM.same_bits(_live_of(dst, LIVE), want, NM.SENT)
            _rest_is_sentinel(dst, LIVE)
            all_st = np.zeros((NR,) + stats.shape[1:], F64)
            all_st[..., 1] = 1.0                                        # an empty row: m = 0, g = 1
            all_st[LIVE] = stats
            NM.same_bits(st.cpu().numpy(), all_st)
    finally:
        nm.close()


def test_norm_65540_rows_workgroup_fold():
    """[65540][1][66][8] with scope "row": a list of 66 chunks, more than a wave folds, so the levels' lists go through the scope's
    own scratch, which the second row range finds from row0 on"""
    from lewton_amd.rows import Normalize
    nm = Normalize(True, "std", 1e-7, 1.0, "row")
    try:
        n = [8 - i % 8 for i in range(len(LIVE))]
        x = NM.source(n, 1, 66, 8, 79, offset=-0.1)
        src = _many(x)
        _, st = nm.run(src, _all_rows(n), want_stats=True)
        torch.cuda.synchronize()
        assert nm.last_launches() == 6
        want, stats = NM.rows(x, n, None, x, 1, NM.STD, NM.ROW, 1e-7, 1.0)
        NM.same_bits(_live_of(src, LIVE), want, NM.SENT)
        _rest_is_sentinel(src, LIVE)
        all_st = np.zeros((NR, 2), F64)
        all_st[:, 1] = 1.0
        all_st[LIVE] = stats
        NM.same_bits(st.cpu().numpy(), all_st)
    finally:
        nm.close()


@pytest.mark.parametrize("identity", [False, True])
def test_cep_65540_rows(identity):
    """[65540][2][5][24] -> 3 cepstra with deltas and delta-deltas (9 lines), and the 5 lines themselves (the bit copy)"""
    from lewton_amd.rows import Cepstrum
    m = None if identity else CM.matrix(3, 5, 3)
    order = 0 if identity else 2
    cp = Cepstrum(5, m, order, 2)
    try:
        n = _live_lengths(24)
        fill = [min(24, v + 2) for v in n]
        x = CM.source(n, 2, 5, 24, 80)
        src, dst = _many(x), S._filled((NR, 2, cp.features, 24))
        cp.run(src, _all_rows(n), out=dst, fill_to=_all_rows(fill))
        torch.cuda.synchronize()
        assert cp.last_launches() == 2
        want = CM.rows(x, n, fill, np.full((len(LIVE), 2, cp.features, 24), SENT_F, F32), m, order, 2)
        CM.same_bits(_live_of(dst, LIVE), want, CM.SENT)
        _rest_is_sentinel(dst, LIVE)
        assert np.array_equal(_live_of(src, LIVE).view(np.uint32), x.view(np.uint32))
    finally:
        cp.close()


def test_slide_65540_rows():
    """[65540][2][3][24] under (W, min, center, norm_vars) = (8, 3, 0, 1): the row record and t.at of the second row range"""
    from lewton_amd.rows import SlidingCMVN
    sl = SlidingCMVN(8, 3, False, True)
    try:
        n = _live_lengths(24)
        fill = [min(24, v + 2) for v in n]
        x = SLM.source(n, 2, 3, 24, 81)
        src, dst = _many(x), S._filled((NR, 2, 3, 24))
        sl.run(src, _all_rows(n), out=dst, fill_to=_all_rows(fill))
        torch.cuda.synchronize()
        assert sl.last_launches() == 2
        want = SLM.rows(x, n, fill, np.full(x.shape, SENT_F, F32), 8, 3, False, True)
        SLM.same_bits(_live_of(dst, LIVE), want, SLM.SENT)
        _rest_is_sentinel(dst, LIVE)
        assert np.array_equal(_live_of(src, LIVE).view(np.uint32), x.view(np.uint32))
    finally:
        sl.close()


SEL_LIVE = [0, 1, 2, 3, 4, 65535, 65536, 65537, 65538, 65539]        # rows k and 65535 + k share the scratch entries of blockIdx.z = k


def test_select_65540_rows():
    """[65540][1][2][300] with a tile of 256: every live row has two tiles, so k_select reads its scratch list.  The second pair of
    launches reuses the entries of the first: row 65535 + k those of row k, whose mask and length differ -- a list_at formed from the
    global row, or a cnt_at formed from blockIdx.z, shows.  counts of all 65 540 rows: zeros for the empty ones"""
    from lewton_amd.rows import SelectFrames
    se = SelectFrames()
    try:
        se.set_tile_frames(256)
        n = [300 - 3 * i for i in range(len(SEL_LIVE))]
        fill = [min(300, v + 2) for v in n]
        assert min(n) > 256
        x = SEL.source(n, 1, 2, 300, 82)
        mask = SEL.mask("random", n, 1, 300, 83)
        want, k = SEL.rows(x, mask, n, fill, np.full(x.shape, SENT_F, F32))
        assert len(set(k[:, 0].tolist())) > 5 and all(k[i, 0] != k[i + 5, 0] for i in range(5))
        src = S._filled((NR, 1, 2, 300))
        src[SEL_LIVE] = torch.from_numpy(x).to("cuda:0")
        dm = torch.full((NR, 1, 300), SEL.SENT_MASK, dtype=torch.uint8, device="cuda:0")
        dm[SEL_LIVE] = torch.from_numpy(mask).to("cuda:0")
        dst = S._filled((NR, 1, 2, 300))
        all_n, all_fill = [0] * NR, [0] * NR
        for r, v, f in zip(SEL_LIVE, n, fill):
            all_n[r], all_fill[r] = v, f
        _, counts = se.run(src, all_n, dm, out=dst, fill_to=all_fill)
        torch.cuda.synchronize()
        assert se.last_launches() == 4
        SEL.same_bits(_live_of(dst, SEL_LIVE), want)
        _rest_is_sentinel(dst, SEL_LIVE)
        all_k = np.zeros((NR, 1), np.int64)
        all_k[SEL_LIVE] = k
        assert np.array_equal(counts.cpu().numpy(), all_k)
        assert np.array_equal(_live_of(src, SEL_LIVE).view(np.uint32), x.view(np.uint32))
    finally:
        se.close()


@pytest.mark.parametrize("fmt", ["f32", "f32_interleaved"])
def test_istft_65540_rows(fmt):
    """[65540][2][6][9] -> [65540][2][8] in reversed row order (a live source row below the cut goes to a destination row above it
    and the other way round), n_fft = 4, hop = 1, both routes: the row record, t.s_at and the record's dst_row of the second range"""
    from lewton_amd.rows import InverseSpectrogram
    itl = fmt.endswith("interleaved")
    inv = InverseSpectrogram(4, 1)
    try:
        frames = [9 - i % 4 for i in range(len(LIVE))]
        x = IC._source(frames, 2, inv.bins, 9, 84)
        nat = [inv.out_len(T) for T in frames]
        lens = [v + (i % 3) - 1 for i, v in enumerate(nat)]
        cap = max(lens) + 1
        dst_rows = [NR - 1 - r for r in LIVE]
        assert any(r < 65535 <= d for r, d in zip(LIVE, dst_rows)) and any(d < 65535 <= r for r, d in zip(LIVE, dst_rows))
        src = _many(x)
        want = IC._expected(inv, (inv.basis(), inv.window2()), x, frames, lens, list(range(len(LIVE))), len(LIVE), cap)
        for route in (0, 1):
            inv.set_route(route)
            dst = S._filled((NR, cap, 2) if itl else (NR, 2, cap))
            inv.run(src, _all_rows(frames), lengths=_all_rows(lens), out=dst, rows=[NR - 1 - r for r in range(NR)], samples=fmt)
            torch.cuda.synchronize()
            assert inv.last_route() == route
            IC.same_bits(_live_of(dst, dst_rows, itl), want)
            _rest_is_sentinel(dst, dst_rows)
        assert np.array_equal(_live_of(src, LIVE).view(np.uint32), x.view(np.uint32))
    finally:
        inv.close()


@pytest.mark.parametrize("pad", ["zero", "reflect"])
def test_spec_complex_65540_rows(pad):
    """[65540][2][40] -> [65540][2][18][12] in reversed row order, n_fft = 16, hop = 4, both routes: test_spec_65540_rows with the re
    and the im lines"""
    from lewton_amd.rows import Spectrogram
    sp = Spectrogram(16, 4, pad_mode=pad, output="complex")
    try:
        lens = _live_lengths(40)
        x = S._source(lens, 2, 40, 9)
        fcap = sp.frames(40) + 1
        dst_rows = [NR - 1 - r for r in LIVE]
        src = _many(x)
        want = _complex_want(sp, x, lens, list(range(len(LIVE))), len(LIVE), fcap)
        for route in (0, 1):
            sp.set_route(route)
            dst = S._filled((NR, 2, sp.features, fcap))
            _, frames = sp.run(src, _all_rows(lens), out=dst, rows=[NR - 1 - r for r in range(NR)])
            torch.cuda.synchronize()
            assert sp.last_route() == route and [int(frames[r]) for r in LIVE] == [sp.frames(v) for v in lens]
            _same_spec(_live_of(dst, dst_rows), want)
            _rest_is_sentinel(dst, dst_rows)
    finally:
        sp.close()
