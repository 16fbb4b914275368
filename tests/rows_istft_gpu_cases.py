"""Inverse spectral frames of rows on the GPU: InverseSpectrogram.run (lw_istft_rows / k_istft) and the complex output of
Spectrogram (k_spec_complex).  The cases of tests/test_gpu_rows_istft.py, which runs this file with pytest in a process of its
own, torch imported first (tests/rows_gpu_cases.py says why).

The rule of include/lewton_amd.h ("inverse spectral frames of rows") is a contract on BITS.  The model (tests/istft_model.py) runs
over the library's own table bits (InverseSpectrogram.basis() / window2(), themselves checked against the formula in
tests/test_host_istft.py).  Every shape runs on route 0 (the matrix cores) and on route 1 (per-lane fmaf chains), and
route 0 == route 1 == model is asserted over EVERY element of a sentinel-filled destination, -0 mapped to +0, with no tolerance.
The source holds NaN beyond each row's frame count.  The shapes are the smallest at which the kernel can still go wrong."""
import torch  # noqa: F401  (first: see above)

import ctypes as C

import numpy as np
import pytest

import istft_model as IM
import kaldi_model as K
import spec_model as M
import spec_reflect_model as R

pytestmark = pytest.mark.gpu

SENT = 0x7FC0DEAD                     # a NaN: the destination's sentinel, and what the source holds beyond each frame count
SENT_F = np.array(SENT, np.uint32).view(np.float32)
# name -> (n_fft, win_length, hop, window, center)
SHAPES = {
    "16_16_4": (16, 16, 4, "hann", True),
    "25_25_7_odd": (25, 25, 7, "hann", True),                             # no Nyquist bin
    "32_20_5_offset": (32, 20, 5, "hann", True),                          # o > 0
    "64_rect_ov1": (64, 64, 64, "rect", False),
    "32_32_2_ov16": (32, 32, 2, "hann", True),                            # the limit
    "16_16_4_uncentred": (16, 16, 4, "hann", False),                      # env = 0 at sample 0
    "512_400_160": (512, 400, 160, "hann", True),
    "2048_2048_512": (2048, 2048, 512, "hann_sym", True),                 # the largest table
}


def _filled(shape):
    t = torch.empty(shape, dtype=torch.float32, device="cuda:0")
    t.view(torch.int32).fill_(int(np.array(SENT, np.uint32).view(np.int32)))
    return t


def _source(frames, ch, B, fcap, seed):
    """host [row][ch][2 B][fcap] float32 with NaN beyond each frame count"""
    rng = np.random.default_rng(seed)
    x = np.full((len(frames), ch, 2 * B, fcap), SENT_F, np.float32)
    for r, T in enumerate(frames):
        x[r, :, :, :T] = rng.uniform(-1, 1, (ch, 2 * B, T)).astype(np.float32)
    return x


def _expected(inv, tables, x, frames, lens, rows, n_dst, cap):
    """float32 [n_dst][ch][cap]: the sentinel everywhere but [0, lens[i]) of the mapped rows"""
    G, w2 = tables
    want = np.full((n_dst, x.shape[1], cap), SENT_F, np.float32)
    for r, T in enumerate(frames):
        assert inv.out_len(T) == IM.geometry(inv.n_fft, inv.win_length, inv.hop, inv.center, T)[4]
        for c in range(x.shape[1]):
            want[rows[r], c, :lens[r]] = IM.istft(G, w2, x[r, c, :, :T], inv.n_fft, inv.hop, inv.center, lens[r])
    return want


def same_bits(got, want):
    """bits, -0 as +0; which NaN a NaN is stays outside the contract, except that a computed NaN is never the sentinel"""
    g, w = (np.ascontiguousarray(v, np.float32).view(np.uint32).copy() for v in (got, want))
    assert g.shape == w.shape
    for v in (g, w):
        v[v == 0x80000000] = 0
    nan = np.isnan(np.asarray(want, np.float32)) & (w != SENT)
    assert not (g[nan] == SENT).any() and np.isnan(np.asarray(got, np.float32)[nan]).all()
    same = (g == w) | nan
    assert same.all(), (int((~same).sum()), np.argwhere(~same)[:4].tolist())


def _both_routes(inv, spec, frames, lens, fmt, shape, want, rows=None):
    itl = fmt.endswith("interleaved")
    outs = []
    for route in (0, 1):
        inv.set_route(route)
        dst = _filled((shape[0], shape[2], shape[1]) if itl else shape)
        out, got_lens = inv.run(spec, frames, lengths=lens, out=dst, rows=rows, samples=fmt)
        torch.cuda.synchronize()
        assert out is dst and inv.last_route() == route
        assert got_lens.tolist() == ([inv.out_len(int(T)) for T in frames] if lens is None else [int(v) for v in lens])
        got = dst.cpu().numpy()
        outs.append(got.transpose(0, 2, 1) if itl else got)
        same_bits(outs[-1], want)
    return outs[0]


@pytest.mark.parametrize("name", list(SHAPES))
def test_route_0_is_route_1_is_the_model(name):
    """frame counts 0, 1, m - 1, m, m + 1 and 2 m + 1 of the object's m (a tile edge, with and without a halo beyond either end of
    the row) as two calls of three rows: two channels planar at the natural lengths, one channel interleaved at lengths shorter
    than, equal to and longer than natural; odd capacities, a spare destination row"""
    from lewton_amd.rows import InverseSpectrogram
    n_fft, win, hop, window, center = SHAPES[name]
    inv = InverseSpectrogram(n_fft, hop, win, window, center)
    try:
        m, B = inv.tile_frames, inv.bins
        assert B == n_fft // 2 + 1 and 1 <= m <= 32 - -(-win // hop)
        tables = (inv.basis(), inv.window2())
        big = name.startswith("2048")
        for call, frames in enumerate(([0, 1, m - 1], [m, m + 1, 2 * m + 1])):
            ch, fmt = (2, "f32") if call == 0 and not big else (1, "f32_interleaved" if call else "f32")
            nat = [inv.out_len(T) for T in frames]
            lens = None if call == 0 else [max(nat[0] - 3, 0), nat[1], nat[2] + 2 * hop + 5]
            fcap = (max(frames) + 2) | 1
            cap = (max(lens or nat) + 3) | 1
            x = _source(frames, ch, B, fcap, 31 + len(name) + call)
            want = _expected(inv, tables, x, frames, lens or nat, [0, 1, 2], 4, cap)
            written = want.view(np.uint32) != SENT
            assert not np.isnan(want[written]).any()
            got = _both_routes(inv, torch.from_numpy(x).to("cuda:0"), frames, lens, fmt, (4, ch, cap), want)
            if name == "16_16_4_uncentred" and call:
                assert (got[:3, 0, 0].view(np.uint32) == 0).all() and got[1, 0, 1] != 0      # hann(0)^2 = 0: +0.0, not a quotient
    finally:
        inv.close()


@pytest.mark.parametrize("name", ["512_400_160", "32_32_2_ov16", "32_20_5_offset"])
def test_two_tile_sizes_give_the_same_bits(name):
    from lewton_amd.rows import InverseSpectrogram
    n_fft, win, hop, window, center = SHAPES[name]
    inv = InverseSpectrogram(n_fft, hop, win, window, center)
    try:
        m = inv.tile_frames
        frames = [2 * m + 1, m, 3]
        x = _source(frames, 2, inv.bins, 2 * m + 2, 77)
        spec = torch.from_numpy(x).to("cuda:0")
        outs = []
        for mm in (m, max(1, m // 2 - 1), 1):
            inv.set_tile_frames(mm)
            assert inv.tile_frames == mm
            for route in (0, 1):
                inv.set_route(route)
                out, _ = inv.run(spec, frames, out=_filled((3, 2, inv.out_len(2 * m + 1) + 1)))
                torch.cuda.synchronize()
                outs.append(out.cpu().numpy().view(np.uint32).copy())
        assert all(np.array_equal(outs[0], o) for o in outs[1:])
        with pytest.raises(ValueError):
            inv.set_tile_frames(m + 1)
        with pytest.raises(ValueError):
            inv.set_tile_frames(0)
    finally:
        inv.close()


def test_special_values_reach_exactly_the_samples_the_model_says():
    """a NaN in a cosine line of frame 3 and an Inf in the ignored imaginary part of bin 0 of frame 9 (dense: Inf * +0.0 = NaN)
    poison exactly the samples those frames touch; a row of subnormal-scale input comes out among the subnormals, not as zeros"""
    from lewton_amd.rows import InverseSpectrogram
    inv = InverseSpectrogram(32, 5, 20, "hann", True)
    try:
        B, frames = inv.bins, [14, 14]
        x = _source(frames, 1, B, 15, 3)
        x[0, 0, 5, 3] = np.nan
        x[0, 0, B, 9] = np.inf
        x[1, 0, :, :14] *= np.float32(1e-38)
        x[1, 0, :, :14:3] *= np.float32(-0.0)
        nat = inv.out_len(14)
        want = _expected(inv, (inv.basis(), inv.window2()), x, frames, [nat, nat], [0, 1], 2, nat + 1)
        bad = np.isnan(want[0, 0, :nat])
        o, pad = (32 - 20) // 2, 16
        touched = np.zeros(nat, bool)
        for t in (3, 9):
            lo, hi = t * 5 + o - pad, t * 5 + o + 20 - pad
            touched[max(lo, 0):hi] = True
        assert (bad == touched).all() and 0 < bad.sum() < nat
        got = _both_routes(inv, torch.from_numpy(x).to("cuda:0"), frames, None, "f32", (2, 1, nat + 1), want)
        tiny = np.abs(got[1, 0, :nat])
        assert (tiny < np.finfo(np.float32).tiny).all() and np.count_nonzero(tiny) > nat // 2
    finally:
        inv.close()


def test_a_dst_row_permutation_with_a_gap():
    from lewton_amd.rows import InverseSpectrogram
    inv = InverseSpectrogram(512, 160, 400)
    try:
        frames, rows = [7, 0, 13, 2], [5, 2, 0, 3]
        nat = [inv.out_len(T) for T in frames]
        lens = [nat[0] - 100, 9, nat[2], nat[3] + 50]
        x = _source(frames, 2, inv.bins, 15, 5)
        cap = max(lens) + 7
        want = _expected(inv, (inv.basis(), inv.window2()), x, frames, lens, rows, 7, cap)
        assert (want[[1, 4, 6]].view(np.uint32) == SENT).all() and (want[2, :, :9] == 0).all()
        spec = torch.from_numpy(x).to("cuda:0")
        _both_routes(inv, spec, frames, lens, "f32", (7, 2, cap), want, rows=rows)
        _both_routes(inv, spec, np.asarray(frames), torch.tensor(lens), "f32_interleaved", (7, 2, cap), want, rows=torch.tensor(rows))
    finally:
        inv.close()


def test_two_objects_queued_back_to_back_on_a_side_stream():
    """five calls of one object with five frames arrays (more than it has record slots) and a second object in between, all on one
    side stream with nothing synchronised until the end"""
    from lewton_amd.rows import InverseSpectrogram
    a, b = InverseSpectrogram(512, 160, 400), InverseSpectrogram(16, 4, window="hann", center=False)
    try:
        xs = {a: _source([12] * 3, 2, a.bins, 13, 11), b: _source([12] * 3, 2, b.bins, 13, 12)}
        src = {k: torch.from_numpy(v).to("cuda:0") for k, v in xs.items()}
        calls = []
        st = torch.cuda.Stream(device=0)
        torch.cuda.synchronize()
        with torch.cuda.stream(st):
            for k in range(5):
                for inv in (a, b) if k < 2 else (a,):
                    inv.set_route(k & 1)
                    frames = [12 - k, k, 5 + k]
                    dst = _filled((3, 2, inv.out_len(12) + 1))
                    inv.run(src[inv], frames, out=dst)
                    calls.append((inv, frames, dst))
        st.synchronize()
        for inv, frames, dst in calls:
            lens = [inv.out_len(T) for T in frames]
            same_bits(dst.cpu().numpy(), _expected(inv, (inv.basis(), inv.window2()), xs[inv], frames, lens, [0, 1, 2], 3, dst.shape[2]))
    finally:
        a.close()
        b.close()


def test_refusals_on_the_gpu_write_nothing():
    from lewton_amd import _native as N
    from lewton_amd.rows import InverseSpectrogram, Spectrogram
    inv = InverseSpectrogram(16, 4)
    try:
        frames = [9, 5, 0]
        x = _source(frames, 2, inv.bins, 9, 13)
        spec = torch.from_numpy(x).to("cuda:0")
        full = inv.out_len(9)
        dst = _filled((4, 2, full))
        bad = [dict(frames=[10, 5, 0]), dict(frames=[9, 5]), dict(frames=[9, -1, 0]), dict(lengths=[full + 1, 1, 1]), dict(lengths=[1, 1]),
               dict(lengths=[1, -1, 1]), dict(rows=[0, 0, 1]), dict(rows=[0, 1, 4]), dict(rows=[0, 1]), dict(rows=[2, 1, 1]),
               dict(out=dst[:, :, :full - 1].contiguous()), dict(out=dst[:, :, :full - 1]), dict(out=dst[:, :1].contiguous()),
               dict(out=dst[:2].contiguous()), dict(out=dst.to(torch.float64)), dict(out=torch.zeros((4, 2, full))), dict(out=dst[0]),
               dict(samples="i16"), dict(spec=spec.to(torch.float64)), dict(spec=spec.cpu()), dict(spec=spec[:, :, :17].contiguous()),
               dict(spec=spec[:, :, :, :8]), dict(spec=spec[0])]
        for kw in bad:
            args = dict(spec=spec, frames=frames, out=dst)
            args.update(kw)
            with pytest.raises(ValueError):
                inv.run(**args)
        with pytest.raises(ValueError):
            inv.set_route(2)
        for kw in [dict(hop=17), dict(n_fft=400, hop=24), dict(n_fft=1), dict(window="kaiser"), dict(win_length=17)]:
            args = dict(n_fft=16, hop=4)
            args.update(kw)
            with pytest.raises(ValueError):
                InverseSpectrogram(**args)
        for kw in [dict(output="magnitude"), dict(output="complex", mel=np.zeros((4, 201), np.float32)), dict(output="complex", energy=True),
                   dict(output="complex", remove_dc=True, framing="kaldi", center=False)]:
            with pytest.raises(ValueError):
                Spectrogram(**kw)

        def c_call(fmt=N.FMT_F32_PLANAR, ch=2, s=spec.data_ptr(), d=dst.data_ptr(), h=inv._h):
            T = np.asarray(frames, np.uint64)
            return N.lw_istft_rows(h, ch, C.c_void_p(s), 3, 9, T.ctypes.data_as(C.c_void_p), None, None, fmt, C.c_void_p(d), 4, full, None)
        assert c_call(fmt=N.FMT_I16_PLANAR) == N.ERR_UNSUPPORTED and c_call(fmt=N.FMT_I16_INTERLEAVED) == N.ERR_UNSUPPORTED
        assert c_call(ch=0) == N.ERR_CAPACITY and c_call(ch=256) == N.ERR_CAPACITY
        assert c_call(s=None) == N.ERR_NULL_ARG and c_call(d=None) == N.ERR_NULL_ARG and c_call(h=None) == N.ERR_NULL_ARG
        err = C.c_int(0)
        assert not N.lw_istft_create(0, None, C.byref(err)) and err.value == N.ERR_NULL_ARG
        p = N.IstftParams(400, 400, 24, 0, 1, 0)
        assert not N.lw_istft_create(0, C.byref(p), C.byref(err)) and err.value == N.ERR_UNSUPPORTED
        torch.cuda.synchronize()
        assert bool((dst.view(torch.int32) == int(np.array(SENT, np.uint32).view(np.int32))).all())
        inv.run(spec, frames, out=dst)                                              # exactly full is accepted
        torch.cuda.synchronize()
        lens = [inv.out_len(T) for T in frames]
        same_bits(dst.cpu().numpy(), _expected(inv, (inv.basis(), inv.window2()), x, frames, lens, [0, 1, 2], 4, full))
        out, lens2 = inv.run(spec, frames)                                          # out=None: zeros, the natural lengths
        torch.cuda.synchronize()
        assert tuple(out.shape) == (3, 2, full) and lens2.tolist() == lens and lens2.dtype == torch.int64
    finally:
        inv.close()


# ---- the complex output of k_spec

def _chains(basis, X):
    re, im = (np.zeros((X.shape[0], basis.shape[2]), np.float32) for _ in range(2))
    for k in range(basis.shape[1]):
        re, im = M.fmaf(X[:, k:k + 1], basis[0][k][None, :], re), M.fmaf(X[:, k:k + 1], basis[1][k][None, :], im)
    return np.concatenate([re, im], axis=1)                               # [T][2 B]


SPEC_SHAPES = {"16_16_4": (16, 16, 4, [15, 17, 20, 150]), "25_25_7": (25, 25, 7, [14, 25, 333]), "512_400_160": (512, 400, 160, [300, 1999, 32 * 160])}


@pytest.mark.parametrize("pad", ["zero", "reflect", "symmetric"])
@pytest.mark.parametrize("name", list(SPEC_SHAPES))
def test_complex_spec_route_0_is_route_1_is_the_model(name, pad):
    """the re lines, then the im lines: the two chains of the contract as they are, under all three pad modes (symmetric is the
    Kaldi framing without snip_edges), two channels, both formats, a tile of frames and one more"""
    from lewton_amd.rows import Spectrogram
    n_fft, win, hop, lengths = SPEC_SHAPES[name]
    if pad == "symmetric":
        sp = Spectrogram(n_fft, hop, win, "hann", False, framing="kaldi", snip_edges=False, output="complex")
    else:
        sp = Spectrogram(n_fft, hop, win, "hann", True, pad_mode=pad, output="complex")
    try:
        B = n_fft // 2 + 1
        assert sp.features == 2 * B and sp.bins == B
        basis = sp.basis()
        rng = np.random.default_rng(len(name) + len(pad))
        cap = (max(lengths) + 3) | 1
        fcap = (max(sp.frames(n) for n in lengths) + 2) | 1
        x = np.full((len(lengths), 2, cap), SENT_F, np.float32)
        want = np.full((len(lengths) + 1, 2, 2 * B, fcap), SENT_F, np.float32)
        for r, n in enumerate(lengths):
            x[r, :, :n] = rng.uniform(-1, 1, (2, n)).astype(np.float32)
            x[r, 1, :n:5] *= np.float32(1e-24)
            for c in range(2):
                X = (K.frame_matrix(x[r, c, :n], win, hop, False) if pad == "symmetric" else R.frame_matrix(x[r, c, :n], n_fft, win, hop)
                     if pad == "reflect" else M.frame_matrix(x[r, c, :n], n_fft, win, hop, True))
                assert len(X) == sp.frames(n)
                want[r, c, :, :len(X)] = _chains(basis, X).T
        for fmt in ("f32", "f32_interleaved"):
            src = torch.from_numpy(np.ascontiguousarray(x.transpose(0, 2, 1) if fmt.endswith("interleaved") else x)).to("cuda:0")
            for route in (0, 1):
                sp.set_route(route)
                dst = _filled(want.shape)
                out, frames = sp.run(src, lengths, out=dst, samples=fmt)
                torch.cuda.synchronize()
                assert out is dst and sp.last_route() == route and frames.tolist() == [sp.frames(n) for n in lengths]
                M.same_bits(dst.cpu().numpy(), want)
        z = Spectrogram.as_complex(dst)
        assert z.dtype == torch.complex64 and tuple(z.shape) == (len(lengths) + 1, 2, B, fcap)
        assert torch.equal(torch.nan_to_num(z.real), torch.nan_to_num(dst[:, :, :B]))      # (the sentinel is a NaN)
        assert torch.equal(torch.nan_to_num(z.imag), torch.nan_to_num(dst[:, :, B:]))
    finally:
        sp.close()


# ---- the round trip through the public classes

@pytest.mark.parametrize("shape", [(512, 400, 160), (64, 64, 16)])
def test_round_trip_through_the_public_classes(shape):
    """Spectrogram(output="complex", pad_mode="reflect") then InverseSpectrogram with lengths= the input lengths: every sample
    within the DERIVED bound of the input (the forward chains' bound carried through the exact inverse, plus the inverse's own:
    istft_model.bound with dX = istft_model.stft_bound) and within the inverse's bound of torch.istft over torch.stft's float64
    result on the same lines"""
    from lewton_amd.rows import InverseSpectrogram, Spectrogram
    n_fft, win, hop = shape
    sp, inv = Spectrogram(n_fft, hop, win, pad_mode="reflect", output="complex"), InverseSpectrogram(n_fft, hop, win)
    try:
        lengths = [40 * hop, 23 * hop + 7, n_fft]
        rng = np.random.default_rng(9)
        x = np.zeros((3, 1, max(lengths)), np.float32)
        for r, n in enumerate(lengths):
            x[r, 0, :n] = rng.uniform(-1, 1, n).astype(np.float32)
        spec, frames = sp.run(torch.from_numpy(x).to("cuda:0"), lengths)
        pcm, lens = inv.run(spec, frames, lengths=lengths)
        torch.cuda.synchronize()
        assert lens.tolist() == lengths and tuple(pcm.shape) == (3, 1, max(lengths))
        got, X = pcm.cpu().numpy().astype(np.float64), spec.cpu().numpy()
        G, w2, basis = inv.basis(), inv.window2(), sp.basis()
        B = n_fft // 2 + 1
        window = torch.from_numpy(IM.window("hann", win))
        for r, n in enumerate(lengths):
            T = int(frames[r])
            Xr = X[r, 0, :, :T]
            dX = IM.stft_bound(basis, R.frame_matrix(x[r, 0, :n], n_fft, win, hop))
            lim = IM.bound(G, w2, Xr, n_fft, hop, True, n, dX=dX)
            err = np.abs(got[r, 0, :n] - x[r, 0, :n].astype(np.float64))
            print("round trip %s row %d: max error %.3g, at most %.3g of the composed bound" % (shape, r, err.max(), (err / lim).max()))
            assert np.isfinite(lim).all() and (err <= lim).all()
            assert (got[r, 0, n:] == 0).all()
            # torch.istft in float64 over the kernel's own lines: the yardstick's algorithm by another hand
            z = torch.complex(torch.from_numpy(Xr[:B].astype(np.float64)), torch.from_numpy(Xr[B:].astype(np.float64)))
            ref = torch.istft(z, n_fft, hop, win, window, center=True, length=n).numpy()
            lim = IM.bound(G, w2, Xr, n_fft, hop, True, n)
            err = np.abs(got[r, 0, :n] - ref)
            print("against torch.istft %s row %d: max error %.3g, at most %.3g of the bound" % (shape, r, err.max(), (err / lim).max()))
            assert (err <= lim).all()
            # ... and torch.istft(torch.stft(x)) in float64 is x to a few ulp of double, so the composed bound holds against it too
            zz = torch.stft(torch.from_numpy(x[r, 0, :n].astype(np.float64)), n_fft, hop, win, window, center=True, pad_mode="reflect",
                            return_complex=True)
            both = torch.istft(zz, n_fft, hop, win, window, center=True, length=n).numpy()
            assert (np.abs(got[r, 0, :n] - both) <= IM.bound(G, w2, Xr, n_fft, hop, True, n, dX=dX)).all()
    finally:
        sp.close()
        inv.close()
