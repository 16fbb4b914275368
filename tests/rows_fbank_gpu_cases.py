"""The Kaldi-compatible front end on the GPU: Spectrogram(framing="kaldi", ...) and KaldiFbank (lw_spec_create_ex / k_spec with its
per-frame prologue and symmetric padding).  The cases of tests/test_gpu_rows_fbank.py, which runs this file with pytest in a process
of its own, torch imported first (tests/rows_gpu_cases.py says why).

The models are in tests/kaldi_model.py (the bit model over the library's own table bits, themselves checked against the formula in
tests/test_host_fbank.py; the float64 yardstick; the derived bound), tests/feat_model.py and tests/norm_model.py.  Every shape
runs on route 0 (the matrix cores) and on route 1 (per-lane fmaf chains), and route 0 == route 1 == model is asserted over EVERY
element of a sentinel-filled destination, -0 mapped to +0, with no tolerance.  The source holds NaN between each length and the
capacity: under symmetric padding the last frames read right up to the last sample and back."""
import torch  # noqa: F401  (first: see above)

import numpy as np
import pytest

import feat_model as FM
import kaldi_model as K
import norm_model as NM
import spec_model as M

pytestmark = pytest.mark.gpu

SENT = 0x7FC0DEAD
SENT_F = np.array(SENT, np.uint32).view(np.float32)
SENT_I = int(np.array(SENT, np.uint32).view(np.int32))


def _banks(n_fft, n_mels):
    from lewton_amd.rows import kaldi_mel_banks
    return kaldi_mel_banks(16000, n_fft, n_mels) if n_mels else None


def _filled(shape):
    t = torch.empty(shape, dtype=torch.float32, device="cuda:0")
    t.view(torch.int32).fill_(SENT_I)
    return t


def _lengths(W, hop, snip):
    tile = [W + (T - 1) * hop if snip else T * hop - hop // 2 for T in (32, 33, 65)]
    return [0, W - 1, W, W + hop - 1, W + hop] + tile


def _source(lengths, ch, seed, offset=0.25):
    """host [row][ch][cap] float32 of odd capacity, NaN beyond each length"""
    rng = np.random.default_rng(seed)
    x = np.full((len(lengths), ch, (max(lengths) + 3) | 1), SENT_F, np.float32)
    for r, n in enumerate(lengths):
        x[r, :, :n] = (rng.uniform(-1, 1, (ch, n)) + offset * (r % 3)).astype(np.float32)
    return x


def _device(x, itl):
    return torch.from_numpy(np.ascontiguousarray(x.transpose(0, 2, 1) if itl else x)).to("cuda:0")


def _frames(sp, x):
    """the frame matrix of one row and channel by the object's framing"""
    if sp.framing == "kaldi":
        return K.frame_matrix(x, sp.win_length, sp.hop, sp.snip_edges)
    return M.frame_matrix(x, sp.n_fft, sp.win_length, sp.hop, sp.center)


def _expected(sp, mel, x, lengths, rows, n_dst, fcap):
    """float32 [n_dst][ch][F][fcap]: the sentinel everywhere but [0, frames) of every line of the mapped rows"""
    basis = sp.basis()
    want = np.full((n_dst, x.shape[1], sp.features, fcap), SENT_F, np.float32)
    X, where = [], []
    for r, n in enumerate(lengths):
        T = sp.frames(n)
        if sp.framing == "kaldi":
            assert T == K.n_frames(n, sp.win_length, sp.hop, sp.snip_edges)
        for c in range(x.shape[1]):
            X.append(_frames(sp, x[r, c, :n]).reshape(T, sp.win_length))
            where.append((rows[r], c, T))
    Y = K.features(basis, mel, np.concatenate(X), sp.remove_dc, sp.energy, sp.scale)      # all frames of the case at once
    at = 0
    for row, c, T in where:
        want[row, c, :, :T] = Y[at:at + T].T
        at += T
    assert at == len(Y)
    return want


def _both_routes(sp, src, lengths, fmt, shape, want, rows=None):
    for route in (0, 1):
        sp.set_route(route)
        dst = _filled(shape)
        out, frames = sp.run(src, lengths, out=dst, rows=rows, samples=fmt)
        torch.cuda.synchronize()
        assert out is dst and sp.last_route() == route
        assert frames.tolist() == [sp.frames(n) for n in lengths]
        K.same_bits(dst.cpu().numpy(), want, SENT)
        assert bool((torch.from_numpy(want.view(np.int32) == SENT_I) == (dst.cpu().view(torch.int32) == SENT_I)).all())


# name -> (n_fft, W, hop, bands, window, snip_edges, remove_dc, energy, preemphasis, scale)
SHAPES = {}
for _name, _s in (("32_25_10_mel5", (32, 25, 10, 5)), ("512_400_160_mel80", (512, 400, 160, 80)), ("256_200_80_mel23", (256, 200, 80, 23))):
    for _snip in (True, False):
        _e = "snip" if _snip else "edges"
        SHAPES["%s_%s_dc_energy" % (_name, _e)] = _s + ("povey", _snip, True, True, 0.97, 32768.0)
        SHAPES["%s_%s_plain" % (_name, _e)] = _s + ("povey", _snip, False, False, 0.97 if _snip else 0.0, 1.0)
    SHAPES[_name + "_snip_dc_only"] = _s + ("povey", True, True, False, 0.0, 1.0)
    SHAPES[_name + "_edges_energy_only"] = _s + ("povey", False, False, True, 0.97, 1.0)
SHAPES["256_200_80_power_behind_energy"] = (256, 200, 80, 0, "hamming_sym", False, True, True, 0.97, 1.0)
SHAPES["32_25_10_power_behind_energy"] = (32, 25, 10, 0, "povey", True, False, True, 0.0, 32768.0)
for _w in ("hann", "rect", "povey", "hamming_sym", "hann_sym", "blackman_sym"):
    SHAPES["window_" + _w] = (32, 25, 10, 5, _w, False, True, True, 0.97, 1.0)


@pytest.mark.parametrize("name", list(SHAPES))
def test_route_0_is_route_1_is_the_model(name):
    """two channels, planar and interleaved, a destination of odd frame capacity with a row more than needed; the lengths around
    the window and at the tile seams (exactly 32, 33 and 65 frames)"""
    from lewton_amd.rows import Spectrogram
    n_fft, W, hop, bands, window, snip, dc, energy, c, scale = SHAPES[name]
    mel = _banks(n_fft, bands)
    sp = Spectrogram(n_fft, hop, W, window, center=False, mel=mel, framing="kaldi", snip_edges=snip, preemphasis=c, remove_dc=dc, energy=energy,
                     scale=scale)
    try:
        assert sp.features == (bands or sp.bins) + int(energy)
        lengths = _lengths(W, hop, snip)
        assert [sp.frames(n) for n in lengths[-3:]] == [32, 33, 65]
        x = _source(lengths, 2, 17 + len(name))
        fcap = (max(sp.frames(n) for n in lengths) + 2) | 1
        n_dst = len(lengths) + 1
        want = _expected(sp, mel, x, lengths, list(range(len(lengths))), n_dst, fcap)
        written = want.view(np.uint32) != SENT
        assert written.any() and not np.isnan(want[written]).any()
        for fmt in ("f32", "f32_interleaved"):
            _both_routes(sp, _device(x, fmt.endswith("interleaved")), lengths, fmt, (n_dst, 2, sp.features, fcap), want)
    finally:
        sp.close()


def test_stft_framing_takes_the_new_options_too():
    """orthogonal: centred STFT frames, zero and reflect padding, with DC removal, energy, pre-emphasis and a symmetric window"""
    from lewton_amd.rows import Spectrogram
    for pad in ("zero", "reflect"):
        sp = Spectrogram(64, 16, 50, "blackman_sym", center=True, pad_mode=pad, preemphasis=0.5, remove_dc=True, energy=True, scale=2.0)
        try:
            lengths = [40, 64, 1000]
            x = _source(lengths, 2, 5)
            want = np.full((3, 2, sp.features, sp.frames(1000) + 1), SENT_F, np.float32)
            for r, n in enumerate(lengths):
                for c in range(2):
                    row = np.pad(x[r, c, :n], 32, "reflect") if pad == "reflect" else x[r, c, :n]
                    X = M.frame_matrix(row, 64, 50, 16, pad == "zero")
                    want[r, c, :, :len(X)] = K.features(sp.basis(), None, X, True, True, 2.0).T
                    assert len(X) == sp.frames(n)
            _both_routes(sp, _device(x, False), lengths, "f32", want.shape, want)
        finally:
            sp.close()


def test_a_constant_row_with_remove_dc():
    """every power line is +0 and E == 0; through KaldiFbank every value has the bits of LOG(FLT_EPSILON)"""
    from lewton_amd.rows import KaldiFbank, Spectrogram
    x = np.full((1, 1, 2001), np.float32(0.3), np.float32)
    src = _device(x, False)
    for snip in (True, False):
        sp = Spectrogram(512, 160, 400, "povey", center=False, framing="kaldi", snip_edges=snip, preemphasis=0.97, remove_dc=True, energy=True,
                         scale=32768.0)
        fb = KaldiFbank(num_mel_bins=80, snip_edges=snip, use_energy=True, energy_floor=0.0, scale=32768.0)
        try:
            for route in (0, 1):
                sp.set_route(route)
                dst = _filled((1, 1, 258, 14))
                _, frames = sp.run(src, [2000], out=dst)
                T = int(frames[0])
                got = dst.cpu().numpy().view(np.uint32)
                assert T == (11 if snip else 13) and not (got[0, 0, :, :T] & 0x7FFFFFFF).any() and (got[0, 0, :, T:] == SENT).all()
                fb.spec.set_route(route)
                out, frames = fb.run(src, [2000])
                lowest = np.float32(fb.log.log(K.EPS))
                assert tuple(out.shape) == (1, 1, 81, T) and lowest == FM.log(FM.LN, np.array([K.EPS], np.float32))[0]
                assert (out.cpu().numpy().view(np.uint32) == lowest.view(np.uint32)).all()
        finally:
            sp.close()
            fb.close()


@pytest.mark.parametrize("dc", [False, True])
def test_special_values(dc):
    """a NaN sample reaches exactly the frames that contain it (the energy of such a frame is 0 by the contract: Ed > 0 fails);
    subnormal samples are kept; +-inf as the model says"""
    from lewton_amd.rows import Spectrogram
    mel = _banks(32, 5)
    sp = Spectrogram(32, 10, 25, "povey", center=False, mel=mel, framing="kaldi", snip_edges=False, preemphasis=0.97, remove_dc=dc, energy=True)
    try:
        lengths = [400, 400, 400, 400, 400]
        x = _source(lengths, 1, 23, offset=0.0)
        x[0, 0, 203] = np.nan
        x[1, 0, :400] = (x[1, 0, :400] * np.float32(1e-20)).astype(np.float32)              # powers and energies among the subnormals
        x[2, 0, 99], x[2, 0, 300] = np.inf, -np.inf
        x[3, 0, 399] = np.nan                                                               # in the reflected tail: read twice
        x[4, 0, :400] = (x[4, 0, :400] * np.float32(1e-39)).astype(np.float32)              # subnormal samples: mu and x' are too
        want = _expected(sp, mel, x, lengths, [0, 1, 2, 3, 4], 5, 41)
        T = sp.frames(400)
        first = [K.first_index(t, 25, 10, False) for t in range(T)]
        hit = np.array([any(K.sym_index(f + k, 400) == 203 for k in range(25)) for f in first])
        assert hit.sum() == 3 and np.isnan(want[0, 0, 1:, :T][:, hit]).all() and not np.isnan(want[0, 0, :, :T][:, ~hit]).any()
        assert not want[0, 0, 0, :T][hit].any()                                             # E of those frames
        tiny = (np.abs(want[1, 0, :, :T]) < np.finfo(np.float32).tiny) & (want[1, 0, :, :T] != 0)
        assert tiny[0].all() and tiny[1:].any()                                             # subnormal results, kept
        assert np.isnan(want[3, 0, 1:, T - 1]).all() and not np.isnan(want[3, 0, :, :T - 1]).any()
        _both_routes(sp, _device(x, False), lengths, "f32", want.shape, want)
    finally:
        sp.close()


def test_the_shortest_row_kaldi_edges_accepts_and_one_sample_below():
    from lewton_amd.rows import Spectrogram
    sp = Spectrogram(512, 160, 400, "povey", center=False, framing="kaldi", snip_edges=False, remove_dc=True, energy=True)
    try:
        ok = [K.accepted(n, 400, 160, False) for n in range(801)]
        L = min(n for n in range(1, 801) if ok[n] and K.n_frames(n, 400, 160, False))       # the shortest row with a frame
        assert not ok[L - 1] and K.n_frames(L - 1, 400, 160, False) and L == 140
        x = _source([1000, L], 1, 3)
        src = _device(x, False)
        dst = _filled((2, 1, 258, 7))
        with pytest.raises(ValueError):
            sp.run(src, [1000, L - 1], out=dst)
        torch.cuda.synchronize()
        assert bool((dst.view(torch.int32) == SENT_I).all())
        want = _expected(sp, None, x, [1000, L], [0, 1], 2, 7)
        _both_routes(sp, src, [1000, L], "f32", (2, 1, 258, 7), want)
        with pytest.raises(ValueError):
            Spectrogram(512, 160, 400, framing="kaldi", center=True)
        with pytest.raises(ValueError):
            Spectrogram(512, 160, 400, framing="kaldi", center=False, pad_mode="reflect")
        with pytest.raises(ValueError):
            Spectrogram(512, 160, 1, "povey", center=False)
        for kw in (dict(preemphasis=1.5), dict(scale=0.0), dict(scale=float("nan")), dict(framing="htk"), dict(window="kaiser"), dict(window="blackman")):
            with pytest.raises(ValueError):
                Spectrogram(512, 160, 400, center=False, **kw)
    finally:
        sp.close()


def test_a_dst_row_permutation_with_a_gap_and_two_objects_back_to_back_on_a_side_stream():
    """energy on: five calls of one object (more than it has record slots) with a second object in between, on one side stream with
    nothing synchronised until the end; rows permuted with a gap"""
    from lewton_amd.rows import Spectrogram
    mel = _banks(256, 23)
    a = Spectrogram(256, 80, 200, "povey", center=False, mel=mel, framing="kaldi", snip_edges=False, preemphasis=0.97, remove_dc=True, energy=True)
    b = Spectrogram(32, 10, 25, "hamming_sym", center=False, framing="kaldi", snip_edges=True, energy=True)
    try:
        x = _source([1500] * 3, 2, 11)
        src = _device(x, False)
        rows = [4, 0, 2]
        calls = []
        st = torch.cuda.Stream(device=0)
        torch.cuda.synchronize()
        with torch.cuda.stream(st):
            for k in range(5):
                for sp, m in ((a, mel), (b, None)) if k < 2 else ((a, mel),):
                    sp.set_route(k & 1)
                    lengths = [1500 - 100 * k, 0 if k & 1 else 130, 700 + k]
                    dst = _filled((5, 2, sp.features, sp.frames(1500) + 1))
                    sp.run(src, lengths, out=dst, rows=rows)
                    calls.append((sp, m, lengths, dst))
        st.synchronize()
        for sp, m, lengths, dst in calls:
            K.same_bits(dst.cpu().numpy(), _expected(sp, m, x, lengths, rows, 5, dst.shape[3]), SENT)
    finally:
        a.close()
        b.close()


def _signals(n):
    rng = np.random.default_rng(11)
    t = np.arange(n) / 16000.0
    walk = np.cumsum(rng.standard_normal(n))
    walk = walk - np.linspace(walk[0], walk[-1], n)
    return [0.3 * rng.standard_normal(n), 0.4 * walk / np.abs(walk).max() + 0.1 * np.sin(2 * np.pi * 150.0 * t), 0.25 + 0.5 * np.sin(2 * np.pi * 60.0 * t)]


@pytest.mark.parametrize("snip", [True, False])
@pytest.mark.parametrize("use_energy", [False, True])
@pytest.mark.parametrize("subtract_mean", [False, True])
def test_kaldi_fbank_is_the_three_models_composed_and_within_the_bound_of_the_yardstick(snip, use_energy, subtract_mean):
    """80 bands at 16 kHz: white noise, a speech-like walk with a 150 Hz tone, a 60 Hz tone with DC, and an empty row; filled to 40
    frames.  Bit for bit kaldi_model -> feat_model -> (the energy floor) -> norm_model; and within kaldi_model.bound of the float64
    yardstick (with subtract_mean: the bound plus its mean over the row's frames, the mean's own share)"""
    from lewton_amd.rows import KaldiFbank
    fb = KaldiFbank(num_mel_bins=80, snip_edges=snip, use_energy=use_energy, subtract_mean=subtract_mean)
    try:
        n = 5000
        lengths = [n, n, n, 0]
        x = np.full((4, 1, n + 3), SENT_F, np.float32)
        for r, s in enumerate(_signals(n)):
            x[r, 0, :n] = s.astype(np.float32)
        out, frames = fb.run(_device(x, False), lengths, fill_to=40)
        torch.cuda.synchronize()
        T = K.n_frames(n, 400, 160, snip)
        F = 80 + int(use_energy)
        assert frames.tolist() == [T, T, T, 0] and tuple(out.shape) == (4, 1, F, 40) and fb.features == F
        # ---- the models composed
        lin = np.zeros((4, 1, F, 40), np.float32)
        basis = fb.spec.basis()
        for r in range(3):
            lin[r, 0, :, :T] = K.features(basis, fb.banks, K.frame_matrix(x[r, 0, :n], 400, 160, snip), True, use_energy, 1.0).T
        want, _ = FM.rows(lin, frames.tolist(), [40] * 4, lin, FM.LN, FM.ROW, K.EPS, np.inf, 0.0, 1.0)
        if use_energy:
            for r in range(3):
                want[r, 0, 0, :T] = np.maximum(want[r, 0, 0, :T], np.float32(np.log(1.0)))         # energy_floor = 1
        logged = want.copy()
        if subtract_mean:
            want, _ = NM.rows(want, frames.tolist(), [40] * 4, want, 1, NM.NONE, NM.LINE, 1e-20, 1.0)
        NM.same_bits(out.cpu().numpy(), want)
        # ---- the yardstick
        for r in range(3):
            ref, re, im, ref_lin = K.yardstick(x[r, 0, :n], 512, 400, 160, snip, K.POVEY, fb.banks, 0.97, True, use_energy, 1.0, parts=True)
            X = K.frame_matrix(x[r, 0, :n], 400, 160, snip)
            b = K.bound(basis, fb.banks, K.prologue(X, True, 1.0)[0], X.astype(np.float64).mean(axis=1), re, im, ref_lin, use_energy, 1.0)
            if use_energy:
                ref[:, 0] = np.maximum(ref[:, 0], 0.0)
            if subtract_mean:
                ref = ref - ref.mean(axis=0, keepdims=True)
                b = b + b.mean(axis=0, keepdims=True) + 2 * K.U * np.abs(logged[r, 0, :, :T].T.astype(np.float64)).max()
            err = np.abs(out[r, 0, :, :T].cpu().numpy().T.astype(np.float64) - ref)
            print("row %d: largest difference %.3e, largest share of the bound %.3f" % (r, err.max(), (err / b).max()))
            assert (err <= b).all()
    finally:
        fb.close()


def test_kaldi_fbank_refuses_what_it_does_not_offer():
    from lewton_amd.rows import KaldiFbank
    for kw in (dict(dither=1.0), dict(htk_compat=True), dict(raw_energy=False), dict(use_power=False), dict(use_log_fbank=False), dict(vtln_warp=1.1),
               dict(blackman_coeff=0.4), dict(channel=0), dict(min_duration=1.0), dict(window_type="kaiser"), dict(num_mel_bins=0),
               dict(frame_length=0.0), dict(energy_floor=-1.0), dict(preemphasis_coefficient=2.0), dict(scale=0.0), dict(high_freq=9000.0),
               dict(round_to_power_of_two=False, frame_length=25.0 + 1.0 / 16)):
        with pytest.raises(ValueError):
            KaldiFbank(**kw)
    fb = KaldiFbank(round_to_power_of_two=False, window_type="hanning", num_mel_bins=40)          # n_fft = 400
    try:
        assert fb.spec.n_fft == 400 and fb.spec.window == "hann_sym" and fb.features == 40
    finally:
        fb.close()
