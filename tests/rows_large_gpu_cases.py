"""The rows chain past element 2^32 of a tensor and past 65535 rows of a call, on the GPU: k_rows_mix, k_resample, k_spec, k_feat,
k_norm and k_cep.  The cases of tests/test_gpu_rows_large.py, which runs this file with pytest in a process of its own, torch
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
live element lies past 2^32, and one past 2^31, so no case can quietly stop crossing.

Part B.  Every entry point cuts a call into launches of 65535 rows and hands row0 to the kernel, which adds it to blockIdx.z for the
row record, the tensor offsets and the per-row scratch.  65 540 rows of a few dozen elements, a dozen of them live on both sides of
the cut, each with data and a length of its own: the live rows equal the model bit for bit, every other element of the destination
is still the sentinel (compared on the device).

The models are those of the other cases files (tests/cep_model.py, norm_model.py, feat_model.py, spec_model.py,
spec_reflect_model.py, the resampler's fold and the mix fold), evaluated over the windows / the live rows only.  No tolerance
anywhere."""
import torch  # noqa: F401  (first: see above)

import math
import time

import numpy as np
import pytest

import cep_model as CM
import feat_model as FM
import norm_model as NM
import rows_feat_gpu_cases as FC
import rows_mix_gpu_cases as MX
import rows_resample_gpu_cases as RC
import rows_spec_gpu_cases as S
import spec_model as SM
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
KIND = {None: NM.NONE, "std": NM.STD, "rms": NM.RMS, "peak": NM.PEAK}


# ---- part A: the buffers and their windows

class _Bufs:
    a = b = big = None


@pytest.fixture(scope="module")
def bufs():
    """one allocation for the whole file: .a and .b are its halves (source and destination), .big all of it (k_rows_mix)"""
    free, _ = torch.cuda.mem_get_info(0)
    if free < 2 * HALF * 4 + (4 << 30):
        pytest.skip("less than %.1f GB of device memory free" % ((2 * HALF * 4 + (4 << 30)) / 1e9))
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
