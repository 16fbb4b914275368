"""Spectral frames of rows on the GPU: Spectrogram.run (lw_spec_rows / k_spec).  The cases of tests/test_gpu_rows_spec.py, which
runs this file with pytest in a process of its own, torch imported first (tests/rows_gpu_cases.py says why).

The rule of include/lewton_amd.h ("spectral frames of rows") is a contract on BITS.  The model (tests/spec_model.py) is an fmaf
chain in numpy over the library's own table bits (Spectrogram.basis(), themselves checked against the formula in
tests/test_host_spec.py, as is the fmaf emulation against glibc's).  Every shape runs on route 0 (the matrix cores) and on route
1 (per-lane fmaf chains), and route 0 == route 1 == model is asserted over EVERY element of a sentinel-filled destination, -0
mapped to +0, with no tolerance.  The source holds NaN between each length and the capacity."""
import torch  # noqa: F401  (first: see above)

import ctypes as C

import numpy as np
import pytest

import spec_model as M

pytestmark = pytest.mark.gpu

SENT = 0x7FC0DEAD                     # a NaN: the destination's sentinel, and what the source holds between len and its capacity
SENT_F = np.array(SENT, np.uint32).view(np.float32)
LENS_400 = [0, 1, 159, 160, 199, 200, 399, 400, 401, 1999]


def _mel(name, n_fft):
    from lewton_amd.rows import mel_filterbank
    if name is None:
        return None
    n_mels, scale = name
    return mel_filterbank(16000, n_fft, n_mels, scale=scale)


# name -> (n_fft, win_length, hop, window, center, mel, lengths, channels)
SHAPES = {
    "400_mel80": (400, 400, 160, "hann", True, (80, "htk"), LENS_400, 2),
    "400_power": (400, 400, 160, "hann", True, None, LENS_400, 2),
    "400_mel1": (400, 400, 160, "hann", True, (1, "htk"), [401, 1999], 1),
    "400_mel128_slaney": (400, 400, 160, "hann", True, (128, "slaney"), [401, 1999], 1),
    "512_400_160": (512, 400, 160, "hann", True, (80, "htk"), [0, 1, 255, 256, 1999], 2),       # the support starts at 56
    "16_rect_uncentred": (16, 16, 4, "rect", False, None, [15, 16, 17, 19, 20], 2),
    "25_25_7": (25, 25, 7, "hann", True, None, [1, 6, 7, 24, 25, 333], 2),                      # odd n_fft, an odd K tail, B = 13
    "64_hop100": (64, 64, 100, "hann", True, (1, "htk"), [99, 100, 101, 1000], 2),              # hop > n_fft
    "32_hop1": (32, 32, 1, "hann", True, None, [1, 31, 100], 2),
    "2048_one_short_row": (2048, 2048, 512, "hann", True, (128, "htk"), [700], 1),
    "2048_power": (2048, 2048, 512, "hann", False, None, [2048 + 512], 1),                      # five passes over the bins
    "a_tile_of_frames_and_one_more": (400, 400, 160, "hann", True, (80, "htk"), [31 * 160, 32 * 160, 32 * 160 - 1], 1),
}


def _filled(shape):
    import torch
    t = torch.empty(shape, dtype=torch.float32, device="cuda:0")
    t.view(torch.int32).fill_(int(np.array(SENT, np.uint32).view(np.int32)))
    return t


def _source(lengths, ch, cap, seed):
    """host [row][ch][cap] float32 with NaN beyond each length"""
    rng = np.random.default_rng(seed)
    x = np.full((len(lengths), ch, cap), SENT_F, np.float32)
    for r, n in enumerate(lengths):
        v = rng.uniform(-1, 1, (ch, n)).astype(np.float32)
        if r == 3:
            v = (v * np.float32(1e-20)).astype(np.float32)              # small enough that P lies among the subnormals
        if n and ch > 1:
            v[ch - 1] = 0
            v[ch - 1, n // 2] = 1                                       # the last of several channels: one impulse
        if n:
            v[0, ::7] *= -0.0 if r == 4 else 1
        x[r, :, :n] = v
    return x


def _device(x, itl):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x.transpose(0, 2, 1) if itl else x)).to("cuda:0")


def _expected(sp, mel, x, lengths, rows, n_dst, fcap):
    """float32 [n_dst][ch][F][fcap]: the sentinel everywhere but [0, frames) of every line of the mapped rows"""
    basis = sp.basis()
    want = np.full((n_dst, x.shape[1], sp.features, fcap), SENT_F, np.float32)
    X, where = [], []
    for r, n in enumerate(lengths):
        T = sp.frames(n)
        assert T == M.n_frames(n, sp.n_fft, sp.hop, sp.center)
        for c in range(x.shape[1]):
            X.append(M.frame_matrix(x[r, c, :n], sp.n_fft, sp.win_length, sp.hop, sp.center))
            where.append((rows[r], c, T))
    Y = M.features(basis, mel, np.concatenate(X))                       # all frames of the case at once
    at = 0
    for row, c, T in where:
        want[row, c, :, :T] = Y[at:at + T].T
        at += T
    assert at == len(Y)
    return want


def _both_routes(sp, src, lengths, fmt, shape, want, rows=None):
    import torch
    for route in (0, 1):
        sp.set_route(route)
        dst = _filled(shape)
        out, frames = sp.run(src, lengths, out=dst, rows=rows, samples=fmt)
        torch.cuda.synchronize()
        assert out is dst and sp.last_route() == route
        assert frames.tolist() == [sp.frames(n) for n in lengths]
        M.same_bits(dst.cpu().numpy(), want)


@pytest.mark.parametrize("name", list(SHAPES))
def test_route_0_is_route_1_is_the_model(name):
    """rows in a source of odd capacity into a destination of odd frame capacity with a row more than needed, planar and
    interleaved; NaN between len and the capacity must not reach the output, the sentinel beyond each frame count must stay"""
    from lewton_amd.rows import Spectrogram
    n_fft, win, hop, window, center, mel_name, lengths, ch = SHAPES[name]
    mel = _mel(mel_name, n_fft)
    sp = Spectrogram(n_fft, hop, win, window, center, mel)
    try:
        assert sp.tile_frames == 32 and sp.bins == n_fft // 2 + 1 and sp.features == (sp.bins if mel is None else len(mel))
        cap = (max(lengths) + 3) | 1
        fcap = (max(sp.frames(n) for n in lengths) + 2) | 1
        x = _source(lengths, ch, cap, 17 + len(name))
        n_dst = len(lengths) + 1
        want = _expected(sp, mel, x, lengths, list(range(len(lengths))), n_dst, fcap)
        written = want.view(np.uint32) != SENT
        assert written.any() and not np.isnan(want[written]).any()
        if name == "a_tile_of_frames_and_one_more":
            assert [sp.frames(n) for n in lengths] == [sp.tile_frames, sp.tile_frames + 1, sp.tile_frames]
        for fmt in ("f32", "f32_interleaved"):
            _both_routes(sp, _device(x, fmt.endswith("interleaved")), lengths, fmt, (n_dst, ch, sp.features, fcap), want)
    finally:
        sp.close()


def test_a_dst_row_permutation_with_a_gap():
    from lewton_amd.rows import Spectrogram
    mel = _mel((80, "htk"), 400)
    sp = Spectrogram(mel=mel)
    try:
        lengths, rows = [1000, 0, 1999, 160], [5, 2, 0, 3]
        x = _source(lengths, 2, 2001, 5)
        want = _expected(sp, mel, x, lengths, rows, 7, 15)
        _both_routes(sp, _device(x, False), lengths, "f32", (7, 2, 80, 15), want, rows=rows)
        _both_routes(sp, _device(x, True), np.asarray(lengths), "f32_interleaved", (7, 2, 80, 15), want, rows=torch.tensor(rows))
    finally:
        sp.close()


def test_two_objects_queued_back_to_back_on_one_stream():
    """five calls of one object with five lengths arrays (more than it has record slots) and a second object in between, all on
    one side stream with nothing synchronised until the end"""
    import torch
    from lewton_amd.rows import Spectrogram
    mel = _mel((80, "htk"), 400)
    a, b = Spectrogram(mel=mel), Spectrogram(64, 16, window="rect", center=False)
    try:
        x = _source([1500] * 3, 2, 1501, 11)
        src = _device(x, False)
        calls = []
        st = torch.cuda.Stream(device=0)
        torch.cuda.synchronize()
        with torch.cuda.stream(st):
            for k in range(5):
                for sp, m in ((a, mel), (b, None)) if k < 2 else ((a, mel),):
                    sp.set_route(k & 1)
                    lengths = [1500 - 100 * k, 3 * k, 700 + k]
                    dst = _filled((3, 2, sp.features, sp.frames(1500) + 1))
                    sp.run(src, lengths, out=dst)
                    calls.append((sp, m, lengths, dst))
        st.synchronize()
        for sp, m, lengths, dst in calls:
            M.same_bits(dst.cpu().numpy(), _expected(sp, m, x, lengths, [0, 1, 2], 3, dst.shape[3]))
    finally:
        a.close()
        b.close()


def test_out_none_allocates_zeros():
    import torch
    from lewton_amd.rows import Spectrogram
    sp = Spectrogram(64, 16)
    try:
        lengths = [10, 1000, 0]
        x = _source(lengths, 2, 1001, 9)
        out, frames = sp.run(_device(x, False), torch.tensor(lengths))
        torch.cuda.synchronize()
        assert tuple(out.shape) == (3, 2, 33, sp.frames(1000)) and out.dtype == torch.float32 and frames.tolist() == [1, 63, 0]
        assert frames.dtype == torch.int64
        want = _expected(sp, None, x, lengths, [0, 1, 2], 3, sp.frames(1000))
        want[want.view(np.uint32) == SENT] = 0
        M.same_bits(out.cpu().numpy(), want)
    finally:
        sp.close()


@pytest.mark.parametrize("log", ["log10", "ln"])
def test_log_is_torchs_own_at_the_written_positions_and_leaves_the_rest(log):
    import torch
    from lewton_amd.rows import Spectrogram
    mel = _mel((80, "htk"), 400)
    sp = Spectrogram(mel=mel)
    try:
        lengths, rows = [1000, 0, 1999], [2, 0, 3]
        x = _source(lengths, 2, 2001, 3)
        src = _device(x, False)
        lin = _filled((4, 2, 80, 15))
        sp.run(src, lengths, out=lin, rows=rows)
        torch.cuda.synchronize()
        want_lin = _expected(sp, mel, x, lengths, rows, 4, 15)
        M.same_bits(lin.cpu().numpy(), want_lin)                          # the bit-exact linear output
        dst = _filled((4, 2, 80, 15))
        out, frames = sp.run(src, lengths, out=dst, rows=rows, log=log, floor=1e-10)
        torch.cuda.synchronize()
        assert out is dst and frames.tolist() == [7, 0, 13]
        written = torch.from_numpy(want_lin.view(np.uint32) != SENT).to("cuda:0")
        fn = torch.log10 if log == "log10" else torch.log
        want = torch.where(written, fn(torch.clamp(lin, min=1e-10)), lin)
        assert torch.equal(dst.view(torch.int32), want.view(torch.int32))
        assert bool((dst.view(torch.int32)[~written] == int(np.array(SENT, np.uint32).view(np.int32))).all())
        lowest = -10 if log == "log10" else float(np.log(1e-10))                    # the floor's logarithm, rounded to float32 by torch
        assert bool(written.any()) and bool((dst[written] >= lowest - 1e-3).all()) and bool((dst[written] > lowest + 1).any())
        with pytest.raises(ValueError):
            sp.run(src, lengths, out=dst, rows=rows, log="log2")
    finally:
        sp.close()


def test_refusals_on_the_gpu_write_nothing():
    import torch
    from lewton_amd import _native as N
    from lewton_amd.rows import Spectrogram
    sp = Spectrogram()
    try:
        lengths = [1000, 500, 0]
        x = _source(lengths, 2, 1001, 13)
        src = _device(x, False)
        full = sp.frames(1000)
        dst = _filled((4, 2, 201, full))
        bad = [dict(lengths=[1002, 500, 0]), dict(lengths=[1000, 500]), dict(lengths=[1000, -1, 0]),
               dict(rows=[0, 0, 1]), dict(rows=[0, 1, 4]), dict(rows=[0, 1]), dict(rows=[2, 1, 1]),          # (the empty row too)
               dict(out=dst[:, :, :, :full - 1].contiguous()), dict(out=dst[:, :, :, :full - 1]), dict(out=dst[:, :1].contiguous()),
               dict(out=dst[:, :, :200].contiguous()), dict(out=dst[:2].contiguous()), dict(out=dst.to(torch.float64)),
               dict(out=torch.zeros((4, 2, 201, full))), dict(out=dst[0]), dict(samples="i16"), dict(src=src.to(torch.int16)),
               dict(src=src.cpu()), dict(log="log2")]
        for kw in bad:
            args = dict(src=src, lengths=lengths, out=dst)
            args.update(kw)
            with pytest.raises(ValueError):
                sp.run(**args)
        with pytest.raises(ValueError):
            sp.set_route(2)

        def c_call(fmt=N.FMT_F32_PLANAR, ch=2, s=src.data_ptr(), d=dst.data_ptr(), h=sp._h):
            lens = np.asarray(lengths, np.uint64)
            return N.lw_spec_rows(h, fmt, ch, C.c_void_p(s), 3, 1001, lens.ctypes.data_as(C.c_void_p), None, C.c_void_p(d), 4, full, None)
        assert c_call(fmt=N.FMT_I16_PLANAR) == N.ERR_UNSUPPORTED and c_call(fmt=N.FMT_I16_INTERLEAVED) == N.ERR_UNSUPPORTED
        assert c_call(ch=0) == N.ERR_CAPACITY and c_call(ch=256) == N.ERR_CAPACITY
        assert c_call(s=None) == N.ERR_NULL_ARG and c_call(d=None) == N.ERR_NULL_ARG and c_call(h=None) == N.ERR_NULL_ARG
        err = C.c_int(0)
        assert not N.lw_spec_create(0, 400, 400, 160, 0, 1, 80, None, C.byref(err)) and err.value == N.ERR_NULL_ARG
        assert not N.lw_spec_create(0, 4096, 400, 160, 0, 1, 0, None, C.byref(err)) and err.value == N.ERR_UNSUPPORTED
        torch.cuda.synchronize()
        sent = int(np.array(SENT, np.uint32).view(np.int32))
        assert bool((dst.view(torch.int32) == sent).all())
        sp.run(src, lengths, out=dst)                                               # exactly full is accepted
        torch.cuda.synchronize()
        M.same_bits(dst.cpu().numpy(), _expected(sp, None, x, lengths, [0, 1, 2], 4, full))
    finally:
        sp.close()
