"""The row resampler on the GPU: Resampler.run (lw_resample_rows / k_resample), decode_streams and decode_ogg_files with
sample_rate=.  The cases of tests/test_gpu_rows_resample.py, which runs this file with pytest in a process of its own, torch
imported first (tests/rows_gpu_cases.py says why).

The rule of include/lewton_amd.h ("resampling rows") is a contract on BITS.  The model is a numpy float32 fold with the library's
own taps (Resampler.taps(), themselves checked against the formula in tests/test_host_resample.py): taps in ascending k, the first
product is the accumulator, every later one is added, each operation one rounded float32 operation.  Every comparison is over
EVERY element of a sentinel-filled destination through integer views, with no tolerance."""
import torch  # noqa: F401  (first: see above)

import ctypes as C
import functools

import numpy as np
import pytest

from common import SETUPS, sg
from rows_gpu_cases import _product
from rows_mix_gpu_cases import _ogg_file

pytestmark = pytest.mark.gpu

SENT = 0x7FC0DEAD                     # a NaN: the destination's sentinel, and what the source holds between len and its capacity
PAIRS = [(48000, 16000), (44100, 16000), (44100, 48000), (22050, 44100), (16000, 44100)]      # 3->1 441->160 147->160 1->2 160->441
FILTERS = {"hann": {}, "kaiser": {"window": "kaiser", "zeros": 16}}
CAP = 4101


def _model(h, orig, new, w, x, n_out, f64=False):
    """the fold of one row and channel: x float32 [len] -> float32 [n_out]; f64: (the float64 fold, sum of |h x|) of the same taps"""
    n = np.arange(n_out, dtype=np.int64)
    base, ph = n * orig // new, n * orig % new
    L = len(x)
    xp = np.concatenate([x, np.zeros(1, x.dtype)])                      # index L: the +0.0 outside [0, len)
    acc = mag = None
    for k in range(h.shape[1]):
        idx = base - w + k
        xv = xp[np.where((idx >= 0) & (idx < L), idx, L)]
        if f64:
            p = h[ph, k].astype(np.float64) * xv.astype(np.float64)
            acc, mag = (p, np.abs(p)) if acc is None else (acc + p, mag + np.abs(p))
        else:
            p = h[ph, k] * xv
            assert p.dtype == np.float32
            acc = p if acc is None else acc + p
    return (acc, mag) if f64 else acc


def _views(t, itl):
    """[row][ch][sample] view of a host array in either layout"""
    return t.transpose(0, 2, 1) if itl else t


def _filled(shape, itl):
    import torch
    t = torch.empty((shape[0], shape[2], shape[1]) if itl else shape, dtype=torch.float32, device="cuda:0")
    t.view(torch.int32).fill_(int(np.array(SENT, np.uint32).view(np.int32)))
    return t


def _source(lengths, ch, cap, itl, seed):
    """host [row][ch][cap] float32 with NaN beyond each length, and the device tensor in the format's layout"""
    import torch
    rng = np.random.default_rng(seed)
    x = np.full((len(lengths), ch, cap), np.array(SENT, np.uint32).view(np.float32), np.float32)
    for r, n in enumerate(lengths):
        v = rng.uniform(-1, 1, (ch, n)).astype(np.float32)
        if r == 3:
            v = (v * np.float32(1e-39)).astype(np.float32)              # a row of subnormals
            assert n == 0 or (np.abs(v[v != 0]) < np.finfo(np.float32).tiny).all()
        if n:
            v[ch - 1] = 0
            v[ch - 1, n // 2] = 1                                       # the last channel of every row: one impulse
            v[0, ::7] *= -0.0 if r == 4 else 1                          # zeros of both signs in the longest row
        x[r, :, :n] = v
    dev = torch.from_numpy(np.ascontiguousarray(x.transpose(0, 2, 1) if itl else x)).to("cuda:0")
    return x, dev


def _expected(rs, x, lengths, rows, n_dst, dcap):
    """int32 [n_dst][ch][dcap]: the sentinel everywhere but [0, out_len) of the mapped rows"""
    h = rs.taps()
    want = np.full((n_dst, x.shape[1], dcap), np.array(SENT, np.uint32).view(np.float32), np.float32)
    for r, n in enumerate(lengths):
        out = rs.out_len(n)
        assert out == -(-n * rs.new // rs.orig)
        for c in range(x.shape[1]):
            want[rows[r], c, :out] = x[r, c, :n] if rs.orig == rs.new else _model(h, rs.orig, rs.new, rs.half_width, x[r, c, :n], out)
    return want.view(np.int32)


def _got(t, itl):
    return np.ascontiguousarray(_views(t.cpu().numpy(), itl)).view(np.int32)


def _same(got, want):
    same = got == want
    assert same.all(), (int((~same).sum()), np.argwhere(~same)[:4].tolist())


@pytest.mark.parametrize("fmt", ["f32", "f32_interleaved"])
@pytest.mark.parametrize("filt", list(FILTERS))
@pytest.mark.parametrize("pair", PAIRS)
def test_run_is_the_fold_bit_for_bit(pair, filt, fmt):
    """5 rows of lengths 0, 1, W - 1, 1000 and 4099 in a source of odd capacity, 1, 2 and 6 channels, into a larger destination in
    permuted row order; NaN between len and the capacity must not reach the output, the sentinel beyond out_len must stay"""
    import torch
    from lewton_amd.rows import Resampler
    itl = fmt.endswith("interleaved")
    rs = Resampler(pair[0], pair[1], **FILTERS[filt])
    try:
        lengths = [0, 1, rs.half_width - 1, 1000, 4099]
        rows = [5, 2, 0, 6, 3]
        dcap = rs.out_len(4099) + (3 if rs.out_len(4099) % 2 == 0 else 2)           # odd, and not exactly full
        for ch in (1, 2, 6):
            x, src = _source(lengths, ch, CAP, itl, 100 * ch + PAIRS.index(pair))
            dst = _filled((7, ch, dcap), itl)
            assert rs.run(src, lengths, out=dst, rows=rows, samples=fmt) is dst
            torch.cuda.synchronize()
            assert rs.last_route == 0
            got, want = _got(dst, itl), _expected(rs, x, lengths, rows, 7, dcap)
            _same(got, want)
            written = want != np.array(SENT, np.uint32).view(np.int32)
            assert not np.isnan(got.view(np.float32)[written]).any()
            if ch == 2:
                # against the float64 fold of the same taps: the standard bound of recursive summation, (K + 1) 2^-24 sum |h x|.
                # That bound models every rounding as relative, which holds without underflow; the row of subnormals is all
                # underflow, where a product is rounded to a multiple of 2^-149 instead: at most 2^-150 absolute per product
                # (sums of two floats are exact down there), K products -- 3e-44 for K = 40, nothing next to any normal value.
                h = rs.taps()
                underflow = h.shape[1] * 2.0 ** -150
                for r, n in enumerate(lengths):
                    y64, mag = _model(h, rs.orig, rs.new, rs.half_width, x[r, 0, :n], rs.out_len(n), f64=True)
                    y32 = got.view(np.float32)[rows[r], 0, :rs.out_len(n)].astype(np.float64)
                    assert (np.abs(y32 - y64) <= (h.shape[1] + 1) * 2.0 ** -24 * mag + underflow).all()
                # the same call again, and through the global-taps route: the same bits
                rs.run(src, lengths, out=dst, rows=rows, samples=fmt)
                torch.cuda.synchronize()
                _same(_got(dst, itl), want)
                from lewton_amd import _native as N
                N.lw_resampler_set_taps_in_lds(rs._h, 0)
                dst2 = _filled((7, ch, dcap), itl)
                rs.run(src, lengths, out=dst2, rows=rows, samples=fmt)
                torch.cuda.synchronize()
                assert rs.last_route == 1
                N.lw_resampler_set_taps_in_lds(rs._h, 1)
                _same(_got(dst2, itl), want)
    finally:
        rs.close()


@pytest.mark.parametrize("fmt", ["f32", "f32_interleaved"])
def test_a_table_too_large_for_lds_goes_the_global_taps_route(fmt):
    """kaiser, zeros 32, 16000 -> 44100: 441 phases of 68 taps = 117 KiB, more than the workgroup's 80 KiB of LDS"""
    import torch
    from lewton_amd.rows import Resampler
    itl = fmt.endswith("interleaved")
    rs = Resampler(16000, 44100, zeros=32, window="kaiser")
    try:
        assert (rs.new, rs.taps_per_phase) == (441, 68) and rs.new * rs.taps_per_phase * 4 > 80 * 1024
        lengths = [0, 1, rs.half_width - 1, 1000, 1487]
        x, src = _source(lengths, 2, 1489, itl, 7)
        dcap = rs.out_len(1487) + 2
        dst = _filled((5, 2, dcap), itl)
        rs.run(src, lengths, out=dst, samples=fmt)
        torch.cuda.synchronize()
        assert rs.last_route == 1
        _same(_got(dst, itl), _expected(rs, x, lengths, list(range(5)), 5, dcap))
    finally:
        rs.close()


def test_a_span_too_large_for_lds_goes_the_all_global_route():
    """2000 -> 1: one phase of 24 246 taps over an input span of 26 245 samples, more than the workgroup's LDS: one output per lane,
    taps and samples from global memory, the same fold"""
    import torch
    from lewton_amd.rows import Resampler
    rs = Resampler(2000, 1)
    try:
        assert (rs.orig, rs.new, rs.taps_per_phase) == (2000, 1, 24246)
        lengths = [0, 1, 2001, 3000, 9001]
        x, src = _source(lengths, 2, 9003, True, 21)
        dst = _filled((5, 2, 7), True)
        rs.run(src, lengths, out=dst, samples="f32_interleaved")
        torch.cuda.synchronize()
        assert rs.last_route == 2 and [rs.out_len(n) for n in lengths] == [0, 1, 2, 2, 5]
        # the same fold with the loop over the 24 246 taps inside numpy: add.accumulate adds strictly in order, in float32
        h = rs.taps()
        want = np.full((5, 2, 7), np.array(SENT, np.uint32).view(np.float32), np.float32)
        for r, n in enumerate(lengths):
            for c in range(2):
                base = np.arange(rs.out_len(n), dtype=np.int64) * rs.orig // rs.new
                idx = base[:, None] - rs.half_width + np.arange(h.shape[1])[None, :]
                xp = np.concatenate([x[r, c, :n], np.zeros(1, np.float32)])
                p = h[0][None, :] * xp[np.where((idx >= 0) & (idx < n), idx, n)]
                assert p.dtype == np.float32
                want[r, c, :rs.out_len(n)] = np.add.accumulate(p, axis=1)[:, -1] if len(base) else 0
        _same(_got(dst, True), want.view(np.int32))
        two = _model(h, rs.orig, rs.new, rs.half_width, x[2, 0, :2001], 2)       # ... and one row by the model the other tests use
        assert np.array_equal(two.view(np.int32), want[2, 0, :2].view(np.int32))
    finally:
        rs.close()


@pytest.mark.parametrize("fmt", ["f32", "f32_interleaved"])
def test_equal_rates_copy_bits(fmt):
    import torch
    from lewton_amd.rows import Resampler
    itl = fmt.endswith("interleaved")
    rs = Resampler(44100, 44100)
    try:
        assert (rs.orig, rs.new) == (1, 1)
        lengths = [0, 1, 6, 1000, 4099]
        x, src = _source(lengths, 3, CAP, itl, 5)
        x[4, 1, 5:9] = np.array([0x7FC12345, 0xFFC00001, 0x00000001, 0x80000000], np.uint32).view(np.float32)   # NaN payloads, a subnormal, -0.0
        src = torch.from_numpy(np.ascontiguousarray(x.transpose(0, 2, 1) if itl else x).view(np.int32)).to("cuda:0").view(torch.float32)
        dst = _filled((6, 3, 4099), itl)
        rs.run(src, lengths, out=dst, rows=[1, 0, 3, 2, 5], samples=fmt)
        torch.cuda.synchronize()
        assert rs.last_route == 3
        _same(_got(dst, itl), _expected(rs, x, lengths, [1, 0, 3, 2, 5], 6, 4099))
    finally:
        rs.close()


def test_out_none_allocates_zeros_and_identity_rows():
    import torch
    from lewton_amd.rows import Resampler
    rs = Resampler(44100, 16000)
    try:
        lengths = [10, 1000, 0]
        x, src = _source(lengths, 2, 1001, False, 9)
        out = rs.run(src, torch.tensor(lengths))
        torch.cuda.synchronize()
        assert tuple(out.shape) == (3, 2, rs.out_len(1000)) and out.dtype == torch.float32
        want = _expected(rs, x, lengths, [0, 1, 2], 3, rs.out_len(1000))
        want[want == np.array(SENT, np.uint32).view(np.int32)] = 0
        _same(_got(out, False), want)
    finally:
        rs.close()


def test_calls_queued_back_to_back_each_give_their_own_result():
    """five calls of one resampler with five lengths arrays (more than it has record slots) and two more resamplers in between,
    all on one side stream with nothing synchronised until the end"""
    import torch
    from lewton_amd.rows import Resampler
    a, b, c = Resampler(44100, 16000), Resampler(48000, 16000, window="kaiser", zeros=16), Resampler(16000, 44100)
    try:
        x, src = _source([1500] * 4, 2, 1501, False, 11)
        calls = []
        st = torch.cuda.Stream(device=0)
        torch.cuda.synchronize()
        with torch.cuda.stream(st):
            for k in range(5):
                for rs in (a, b, c) if k < 2 else (a,):
                    lengths = [1500 - 100 * k, 3 * k, 1500, 700 + k]
                    dcap = rs.out_len(1500) + 1
                    dst = _filled((4, 2, dcap), False)
                    rs.run(src, lengths, out=dst)
                    calls.append((rs, lengths, dst, dcap))
        st.synchronize()
        for rs, lengths, dst, dcap in calls:
            _same(_got(dst, False), _expected(rs, x, lengths, [0, 1, 2, 3], 4, dcap))
    finally:
        for rs in (a, b, c):
            rs.close()


def test_refusals_on_the_gpu_write_nothing():
    import torch
    from lewton_amd import _native as N
    from lewton_amd.rows import Resampler
    rs = Resampler(44100, 16000)
    try:
        lengths = [1000, 500, 0]
        x, src = _source(lengths, 2, 1001, False, 13)
        full = rs.out_len(1000)
        dst = _filled((4, 2, full), False)
        bad = [dict(lengths=[1002, 500, 0]), dict(lengths=[1000, 500]), dict(lengths=[1000, -1, 0]),
               dict(rows=[0, 0, 1]), dict(rows=[0, 1, 4]), dict(rows=[0, 1]), dict(rows=[2, 1, 1]),          # (the empty row too)
               dict(out=dst[:, :, :full - 1].contiguous()), dict(out=dst[:, :, :full - 1]), dict(out=dst[:, :1].contiguous()),
               dict(out=dst[:2].contiguous()), dict(out=dst.to(torch.float64)), dict(out=torch.zeros((4, 2, full))),
               dict(out=dst[0]), dict(samples="i16"), dict(src=src.to(torch.int16)), dict(src=src.cpu())]
        for kw in bad:
            args = dict(src=src, lengths=lengths, out=dst)
            args.update(kw)
            with pytest.raises(ValueError):
                rs.run(**args)

        def c_call(fmt=N.FMT_F32_PLANAR, ch=2, s=src.data_ptr(), d=dst.data_ptr(), h=rs._h):
            lens = np.asarray(lengths, np.uint64)
            return N.lw_resample_rows(h, fmt, ch, C.c_void_p(s), 3, 1001, lens.ctypes.data_as(C.c_void_p), None, C.c_void_p(d), 4, full, None)
        assert c_call(fmt=N.FMT_I16_PLANAR) == N.ERR_UNSUPPORTED and c_call(fmt=N.FMT_I16_INTERLEAVED) == N.ERR_UNSUPPORTED
        assert c_call(ch=0) == N.ERR_CAPACITY and c_call(ch=256) == N.ERR_CAPACITY
        assert c_call(s=None) == N.ERR_NULL_ARG and c_call(d=None) == N.ERR_NULL_ARG and c_call(h=None) == N.ERR_NULL_ARG
        torch.cuda.synchronize()
        sent = int(np.array(SENT, np.uint32).view(np.int32))
        assert bool((dst.view(torch.int32) == sent).all())
        rs.run(src, lengths, out=dst)                                               # exactly full is accepted
        torch.cuda.synchronize()
        _same(_got(dst, False), _expected(rs, x, lengths, [0, 1, 2], 4, full))
    finally:
        rs.close()
    for kw in [dict(zeros=0), dict(rolloff=1.5), dict(window="blackman"), dict(out_rate=0)]:
        args = dict(in_rate=44100, out_rate=16000)
        args.update(kw)
        with pytest.raises(ValueError):
            Resampler(**args)


# ---- the public functions

@functools.lru_cache(maxsize=None)
def _stereo_case():
    setup = SETUPS["stereo"]()
    streams = [sg.make_stream(setup, "LLSSLSL", c, seed=5 + 31 * s) for s, c in enumerate((9, 5, 7))]
    return setup, streams


def _resampled(native, lengths, fmt, rs):
    """the model over a native-rate tensor as decode_* returns it -> int32 [row][ch][T'] with zero beyond each output length"""
    itl = fmt.endswith("interleaved")
    x = _views(native.cpu().numpy(), itl)
    h = rs.taps()
    outs = [rs.out_len(n) for n in lengths]
    want = np.zeros((x.shape[0], x.shape[1], -(-max(outs) // 64) * 64), np.float32)
    for r, n in enumerate(lengths):
        for c in range(x.shape[1]):
            want[r, c, :outs[r]] = _model(h, rs.orig, rs.new, rs.half_width, np.ascontiguousarray(x[r, c, :n]), outs[r])
    return want.view(np.int32), outs


@pytest.mark.parametrize("channels", [None, "mono"])
@pytest.mark.parametrize("fmt", ["f32", "f32_interleaved"])
def test_decode_streams_sample_rate(fmt, channels):
    import torch
    from lewton_amd.rows import Resampler, decode_streams
    setup, streams = _stereo_case()
    _, ident, st = _product(setup)
    assert ident.audio_sample_rate == 44100
    itl = fmt.endswith("interleaved")
    kw = dict(max_packets=8, run=3, skip=[3, 0, 0], keep=[None, 333, None], channels=channels)
    native, nat_len, errors = decode_streams(ident, st, streams, fmt, **kw)         # pinned to the oracle by the existing tests
    assert errors == [] and nat_len[1].item() == 333 and len(set(nat_len.tolist())) == 3
    for resample in (None, {"window": "kaiser", "zeros": 16}):
        rs = Resampler(44100, 16000, **(resample or {}))
        try:
            want, outs = _resampled(native, nat_len.tolist(), fmt, rs)
        finally:
            rs.close()
        pcm, lengths, errors = decode_streams(ident, st, streams, fmt, sample_rate=16000, resample=resample, **kw)
        assert errors == [] and lengths.tolist() == outs and lengths.dtype == torch.int64
        assert tuple(pcm.shape) == ((3, want.shape[2], want.shape[1]) if itl else want.shape)
        _same(_got(pcm, itl), want)                                                  # (zero beyond each length included)
    # out=: checked against the output length, filled in place
    out = torch.full(tuple(pcm.shape[:1]) + ((pcm.shape[1] + 64, pcm.shape[2]) if itl else (pcm.shape[1], pcm.shape[2] + 64)), 7.0, device="cuda:0")
    pcm2, lengths2, _ = decode_streams(ident, st, streams, fmt, sample_rate=16000, resample=resample, out=out, **kw)
    assert pcm2 is out and lengths2.tolist() == outs
    _same(_got(pcm2, itl)[:, :, :want.shape[2]], want)
    assert not bool(_got(pcm2, itl)[:, :, want.shape[2]:].any())
    assert want.shape[2] > 64
    with pytest.raises(ValueError):                                                 # one pad_to short of the output length
        decode_streams(ident, st, streams, fmt, sample_rate=16000, **kw,
                       out=torch.zeros(tuple(pcm.shape[:1]) + ((pcm.shape[1] - 64, pcm.shape[2]) if itl else (pcm.shape[1], pcm.shape[2] - 64)),
                                       device="cuda:0"))
    # the stream's own rate: the old path, identical bits
    same, same_len, _ = decode_streams(ident, st, streams, fmt, sample_rate=44100, **kw)
    assert same_len.tolist() == nat_len.tolist() and torch.equal(same.view(torch.int32), native.view(torch.int32))
    with pytest.raises(ValueError, match="f32"):
        decode_streams(ident, st, streams, "i16", sample_rate=16000)


@functools.lru_cache(maxsize=None)
def _three_rates():
    return [_ogg_file(SETUPS["stereo"](), "LLSLSSL", 9, 3, 0x11, trim=333),
            _ogg_file(sg.mono_setup(sample_rate=48000), "SLLS", 8, 4, 0x22, trim=37),
            _ogg_file(sg.mono_setup(sample_rate=16000), "SLLS", 7, 6, 0x33)]


@pytest.mark.parametrize("fmt", ["f32", "f32_interleaved"])
def test_decode_ogg_files_of_three_rates_to_16k_mono(fmt):
    import torch
    from lewton_amd.rows import Resampler, decode_ogg_files
    files = _three_rates()
    itl = fmt.endswith("interleaved")
    with pytest.raises(ValueError, match="source 1.*Hz"):
        decode_ogg_files(files, fmt, channels="mono")                               # without sample_rate: as before
    pcm, lengths, rate = decode_ogg_files(files, fmt, channels="mono", sample_rate=16000, max_packets=8, run=3)
    assert rate == 16000 and tuple(pcm.shape[:1] + pcm.shape[2:] if itl else pcm.shape[:2]) == (3, 1)
    got = _got(pcm, itl)
    assert got.shape[2] == -(-int(lengths.max()) // 64) * 64
    for i, (data, native_rate) in enumerate(zip(files, (44100, 48000, 16000))):
        native, nat_len, r = decode_ogg_files([data], fmt, channels="mono")        # the file's own native-rate decode
        assert r == native_rate and nat_len[0].item() > 0
        if native_rate == 16000:
            want, outs = _got(native, itl), nat_len.tolist()
        else:
            rs = Resampler(native_rate, 16000)
            try:
                want, outs = _resampled(native, nat_len.tolist(), fmt, rs)
            finally:
                rs.close()
        assert lengths[i].item() == outs[0]
        _same(got[i, :, :outs[0]], want[0, :, :outs[0]])
        assert not got[i, :, outs[0]:].any()
    with pytest.raises(ValueError, match="source 0.*f32"):
        decode_ogg_files(files, "i16", channels={2: [[1, 0]], 1: [[1]]}, sample_rate=16000)
