"""Finishing feature rows and reflect-padded frames on the GPU: LogCompress.run (lw_feat_rows / k_feat) and
Spectrogram(pad_mode="reflect") (k_spec).  The cases of tests/test_gpu_rows_feat.py, which runs this file with pytest in a process
of its own, torch imported first (tests/rows_gpu_cases.py says why).

Both rules of include/lewton_amd.h are contracts on BITS.  The models are tests/feat_model.py (LOG in numpy float64 as the contract
writes it) and tests/spec_model.py over tests/spec_reflect_model.py's padded rows.  Every comparison is over EVERY element of a
sentinel-filled destination, with no tolerance; the source holds NaN beyond each n_frames (each length) and in all padding."""
import torch  # noqa: F401  (first: see above)

import itertools

import numpy as np
import pytest

import feat_model as FM
import rows_spec_gpu_cases as S
import spec_model as M
import spec_reflect_model as RM

pytestmark = pytest.mark.gpu

F32 = np.float32
KINDS = {"none": (None, -1.0), "ln": ("ln", 1e-10), "log10": ("log10", 1e-10), "db": ("db", 1e-42)}
FILLS = {"none": lambda n, cap: None, "frames": lambda n, cap: list(n), "capacity": lambda n, cap: [cap] * len(n),
         "below": lambda n, cap: [max(0, v - 2) for v in n]}


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to("cuda:0")


def _check(lc, x, n_frames, fill_to, inplace, want_max):
    """one call against the model: the whole destination, and M"""
    src = _dev(x)
    dst = src if inplace else S._filled(x.shape)
    before = x if inplace else np.full(x.shape, FM.SENT_F, F32)
    r = lc.run(src, n_frames, out=None if inplace else dst, fill_to=fill_to, want_max=want_max)
    torch.cuda.synchronize()
    out, mx = r if want_max else (r, None)
    assert out is dst
    want, Ms = FM.rows(x, n_frames, fill_to, before, FM.LOGS[lc.log_kind or "none"], FM.ROW if lc.scope == "row" else FM.CHANNEL,
                       lc.floor, lc.top, lc.add, lc.mul)
    FM.same_bits(dst.cpu().numpy(), want, FM.SENT)
    if not inplace:
        assert np.array_equal(src.cpu().numpy().view(np.uint32), x.view(np.uint32))       # the source is only read
    if want_max:
        FM.same_bits(mx.cpu().numpy(), Ms)
    assert lc.last_launches() == (1 if lc.top == float("inf") and not want_max else 2)
    return want


@pytest.mark.parametrize("kind", list(KINDS))
def test_k_feat_is_the_model_on_the_base_shape(kind):
    """F = 3, capacity 37, n_frames 0 .. 37 over the rows of one call; one and two channels, both scopes, top 8 / 0 / inf, in place
    and not, fill_to absent / n_frames / the capacity / below n_frames; negatives, +-0, NaN, subnormals, the floor itself and
    FLT_MAX in the input, +inf in one row only"""
    from lewton_amd.rows import LogCompress
    log, floor = KINDS[kind]
    n = FM.BASE_FRAMES
    made = {}
    try:
        for i, (ch, scope, top, inplace, fill) in enumerate(itertools.product((1, 2), ("row", "channel"), (8.0, 0.0, float("inf")),
                                                                               (False, True), sorted(FILLS))):
            if (scope, top) not in made:
                made[scope, top] = LogCompress(log, floor, top, 4.0, 0.25, scope)
            x = FM.source(n, ch, 3, 37, floor, 300 + i, inf_row=4 if i % 3 == 0 else None)
            _check(made[scope, top], x, n, FILLS[fill](n, 37), inplace, want_max=(i + i // 4) % 2 == 0)
    finally:
        for lc in made.values():
            lc.close()


@pytest.mark.parametrize("where", ["first", "last", "tile_end", "tile_start"])
def test_one_long_scope_over_several_tiles(where):
    """F = 5, 5000 frames in a capacity of 5003: lines at every residue against 16 bytes, 100 runs of 256 frames in the scope, 25
    tiles; the row's maximum at the first element, the last, the last of the first tile (frame 1023: torch's buffers start at a
    16-byte boundary) and the first of the next.  d_max is compared as well"""
    from lewton_amd.rows import LogCompress
    n, cap, F = 5000, 5003, 5
    x = FM.source([n], 1, F, cap, 1e-10, 5)
    x[0, :, :, :n] = np.minimum(x[0, :, :, :n], F32(100.0))
    x[0][{"first": (0, 0, 0), "last": (0, F - 1, n - 1), "tile_end": (0, 0, 1023), "tile_start": (0, 0, 1024)}[where]] = 1e6
    lc = LogCompress.whisper()
    try:
        for inplace in (False, True):
            want = _check(lc, x, [n], [cap], inplace, want_max=True)
            assert want[0, :, :, :n].max() == F32(2.5) and (want[0, :, :, :n] >= F32(0.5)).all()      # (6 + 4) / 4, (6 - 8 + 4) / 4
    finally:
        lc.close()


@pytest.mark.parametrize("kind", ["ln", "log10", "db"])
def test_the_devices_log_is_the_models_on_a_million_bit_patterns(kind):
    """top = inf, add = 0, mul = 1: the output is l itself.  Random positive finite f32 bit patterns (subnormals included), the
    values around 1.0 and the edge values, in lines of an odd length"""
    from lewton_amd.rows import LogCompress
    rng = np.random.default_rng(11)
    one = int(np.array(1.0, F32).view(np.uint32))
    cap, F = 131075, 8
    bits = rng.integers(1, 0x7F800000, F * cap, dtype=np.uint32)
    bits[:4] = [1, 0x00800000, 0x7F7FFFFF, 0x7F800000]
    bits[cap:cap + 65536] = np.arange(one - 32768, one + 32768, dtype=np.uint32)
    x = bits.view(F32).reshape(1, 1, F, cap)
    lc = LogCompress(kind, 1e-45, float("inf"), 0.0, 1.0)
    try:
        out = lc.run(_dev(x), [cap], out=S._filled(x.shape))
        torch.cuda.synchronize()
        want = FM.log(FM.LOGS[kind], x)
        assert np.array_equal(out.cpu().numpy().view(np.uint32), (want + F32(0.0)).view(np.uint32))
    finally:
        lc.close()


def test_rows_and_channels_do_not_leak():
    """four rows with different maxima, the largest of each in channel 1 only: the scopes differ exactly as the model's do"""
    from lewton_amd.rows import LogCompress
    n = [30, 37, 5, 33]
    x = FM.source(n, 2, 3, 37, 1e-10, 9)
    for r in range(4):
        x[r, :, :, :n[r]] = np.minimum(x[r, :, :, :n[r]], F32(1.0))
        x[r, 1, 2, n[r] - 1] = 10.0 ** (3 + 2 * r)
    outs = []
    for scope in ("row", "channel"):
        lc = LogCompress(scope=scope)
        try:
            outs.append(_check(lc, x, n, [37] * 4, False, True))
        finally:
            lc.close()
    assert not np.array_equal(outs[0][:, 0], outs[1][:, 0]) and np.array_equal(outs[0][:, 1], outs[1][:, 1])


def test_no_maximum_no_second_launch_and_the_host_log():
    from lewton_amd.rows import LogCompress
    lc = LogCompress("db", 1e-10, float("inf"), 0.0, 1.0)
    try:
        assert lc.last_launches() == -1
        x = FM.source([20, 0, 37], 1, 3, 37, 1e-10, 2)
        _check(lc, x, [20, 0, 37], [37, 5, 0], False, want_max=False)
        assert lc.last_launches() == 1
        _check(lc, x, [20, 0, 37], None, True, want_max=True)
        v = np.array([1e-10, 1.0, 2.0, 12345.678, 3e38], F32)
        assert [F32(lc.log(t)) for t in v] == FM.log(FM.DB, v).tolist()
        with pytest.raises(ValueError):
            lc.run(_dev(x), [20, 0, 38])
        with pytest.raises(ValueError):
            lc.run(_dev(x), [20, 0, 37], fill_to=38)
        with pytest.raises(ValueError):
            lc.run(_dev(x), [20, 0])
        with pytest.raises(ValueError):
            lc.run(_dev(x), [20, 0, 37], out=S._filled((3, 1, 3, 36)))
    finally:
        lc.close()


def test_calls_queued_back_to_back_on_one_stream():
    """five calls of one object (more than it has record slots), different counts each, on a side stream, nothing synchronised
    until the end"""
    from lewton_amd.rows import LogCompress
    lc = LogCompress.whisper()
    try:
        x = FM.source([37] * 3, 2, 3, 37, 1e-10, 21)
        x[np.isnan(x)] = 0
        src = _dev(x)
        calls = []
        st = torch.cuda.Stream(device=0)
        torch.cuda.synchronize()
        with torch.cuda.stream(st):
            for k in range(5):
                n = [37 - 7 * k, 3 * k, 11 + k]
                dst = S._filled(x.shape)
                lc.run(src, n, out=dst, fill_to=[k, 37, 0])
                calls.append((n, [k, 37, 0], dst))
        st.synchronize()
        for n, fill, dst in calls:
            FM.same_bits(dst.cpu().numpy(), FM.rows(x, n, fill, np.full(x.shape, FM.SENT_F, F32))[0], FM.SENT)
    finally:
        lc.close()


# ---- reflect

# name -> (n_fft, win_length, hop, window, mel, lengths, channels)
REFLECT = {
    "400_mel80": (400, 400, 160, "hann", (80, "slaney"), [201, 202, 400, 1599, 1600, 1601, 0], 2),
    "400_power": (400, 400, 160, "hann", None, [201, 1600, 1601], 1),
    "25_25_7": (25, 25, 7, "hann", None, [14, 15, 21, 0, 28, 333], 2),                      # odd n_fft; hop divides 21 and 28
    "16_16_4": (16, 16, 4, "rect", None, [9, 10, 16, 17, 64], 2),
    "2048_2048_512": (2048, 2048, 512, "hann", (128, "htk"), [1025, 1536], 1),
}


def _expected_reflect(sp, mel, x, lengths, n_dst, fcap):
    want = np.full((n_dst, x.shape[1], sp.features, fcap), S.SENT_F, F32)
    X, where = [], []
    for r, n in enumerate(lengths):
        T = sp.frames(n)
        assert T == M.n_frames(n, sp.n_fft, sp.hop, True)
        for c in range(x.shape[1]):
            X.append(RM.frame_matrix(x[r, c, :n], sp.n_fft, sp.win_length, sp.hop))
            where.append((r, c, T))
    Y = M.features(sp.basis(), mel, np.concatenate(X))
    at = 0
    for row, c, T in where:
        want[row, c, :, :T] = Y[at:at + T].T
        at += T
    assert at == len(Y)
    return want


@pytest.mark.parametrize("name", list(REFLECT))
def test_reflect_route_0_is_route_1_is_the_model(name):
    """as tests/rows_spec_gpu_cases.py: odd capacities, a destination row more than needed, planar and interleaved, NaN between
    len and the capacity, the sentinel beyond each frame count; lengths from the shortest one reflection serves"""
    from lewton_amd.rows import Spectrogram
    n_fft, win, hop, window, mel_name, lengths, ch = REFLECT[name]
    mel = S._mel(mel_name, n_fft)
    sp = Spectrogram(n_fft, hop, win, window, True, mel, pad_mode="reflect")
    try:
        assert min(n for n in lengths if n) == RM.min_len(n_fft)
        cap = (max(lengths) + 3) | 1
        fcap = (max(sp.frames(n) for n in lengths) + 2) | 1
        x = S._source(lengths, ch, cap, 41 + len(name))
        n_dst = len(lengths) + 1
        want = _expected_reflect(sp, mel, x, lengths, n_dst, fcap)
        for fmt in ("f32", "f32_interleaved"):
            S._both_routes(sp, S._device(x, fmt.endswith("interleaved")), lengths, fmt, (n_dst, ch, sp.features, fcap), want)
        # one sample short: refused, nothing written; the same row is served with zero padding
        short = list(lengths)
        short[-1] = RM.min_len(n_fft) - 1
        dst = S._filled((n_dst, ch, sp.features, fcap))
        with pytest.raises(ValueError):
            sp.run(S._device(x, False), short, out=dst)
        torch.cuda.synchronize()
        assert bool((dst.view(torch.int32) == int(np.array(S.SENT, np.uint32).view(np.int32))).all())
    finally:
        sp.close()


@pytest.mark.parametrize("shape", [(400, 160, 1600), (400, 160, 1733), (25, 7, 70), (512, 128, 1000)])
def test_reflect_is_the_uncentred_transform_of_torchs_padded_rows(shape):
    """on the device: centred reflect frames of x == uncentred frames of torch.nn.functional.pad(x, reflect) over their common
    frames (all of them for even n_fft), bitwise but for the sign of a zero, which the spec contract leaves open"""
    from lewton_amd.rows import Spectrogram
    n_fft, hop, n = shape
    mel = S._mel((80, "htk"), n_fft)
    a, b = Spectrogram(n_fft, hop, mel=mel, pad_mode="reflect"), Spectrogram(n_fft, hop, mel=mel, center=False)
    try:
        x = torch.from_numpy(np.random.default_rng(3).uniform(-1, 1, (3, 2, n)).astype(F32)).to("cuda:0")
        p = torch.nn.functional.pad(x, (n_fft // 2, n_fft // 2), mode="reflect").contiguous()
        ya, fa = a.run(x, [n] * 3)
        yb, fb = b.run(p, [p.shape[2]] * 3)
        torch.cuda.synchronize()
        T = min(int(fa[0]), int(fb[0]))
        assert T == int(fb[0]) and int(fa[0]) - T == (1 if n_fft % 2 and n % hop == 0 else 0) and T > 3
        M.same_bits(ya[..., :T].cpu().numpy(), yb[..., :T].cpu().numpy())
        z = Spectrogram(n_fft, hop, mel=mel)
        try:
            yz, _ = z.run(x, [n] * 3)
            assert not torch.equal(yz[..., 0], ya[..., 0]) and not torch.equal(yz[..., T - 1], ya[..., T - 1])      # the edges differ
            inner = slice(n_fft // 2 // hop + 1, (n - n_fft // 2) // hop)
            assert torch.equal(yz[..., inner], ya[..., inner])                                                  # ... and nothing else
        finally:
            z.close()
    finally:
        a.close()
        b.close()


# ---- the chain

def test_rows_to_whisper_features_is_the_two_models_composed():
    """[3][1][4000] with lengths 4000, 1601 and 0 through the reflect spectrogram with 80 slaney bands, then LogCompress.whisper()
    in place with every line filled to the capacity: bit for bit the models composed, the empty row included"""
    from lewton_amd.rows import LogCompress, Spectrogram, mel_filterbank
    mel = mel_filterbank(16000, 400, 80, scale="slaney", norm="slaney")
    sp, lc = Spectrogram(mel=mel, pad_mode="reflect"), LogCompress.whisper()
    try:
        lengths = [4000, 1601, 0]
        x = S._source(lengths, 1, 4000, 77)
        fcap = 29
        feats = S._filled((3, 1, 80, fcap))
        out, frames = sp.run(S._device(x, False), lengths, out=feats)
        assert frames.tolist() == [26, 11, 0]
        res, mx = lc.run(out, frames, fill_to=[fcap, 20, fcap], want_max=True)
        torch.cuda.synchronize()
        assert res is feats
        lin = _expected_reflect(sp, mel, x, lengths, 3, fcap)
        want, Ms = FM.rows(lin, frames.tolist(), [fcap, 20, fcap], lin)
        FM.same_bits(feats.cpu().numpy(), want, FM.SENT)
        FM.same_bits(mx.cpu().numpy(), Ms)
        assert (want[2] == F32(-1.5)).all() and Ms[2] == F32(-10.0)                      # (max(-10, -10 - 8) + 4) / 4
        assert (want[1, 0, :, 20:].view(np.uint32) == FM.SENT).all()
    finally:
        sp.close()
        lc.close()
