"""Sliding-window normalisation of feature rows on the GPU: SlidingCMVN.run (lw_slide_rows / k_slide).  The cases of
tests/test_gpu_rows_slide.py, which runs this file with pytest in a process of its own, torch imported first
(tests/rows_gpu_cases.py says why).

The rule of include/lewton_amd.h ("sliding-window normalisation of feature rows") is a contract on BITS, the order of its double
sums included.  The model is tests/slide_model.py (numpy float64, the windows and the lists of terms in Python integers).  Every
comparison with it is over EVERY element of a sentinel-filled exact-size destination, with no tolerance; the source holds a NaN at
and beyond each length."""
import torch  # noqa: F401  (first: see above)

import numpy as np
import pytest

import slide_model as M
import rows_spec_gpu_cases as S

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to("cuda:0")


def _make(cfg):
    from lewton_amd.rows import SlidingCMVN
    return SlidingCMVN(cfg[0], cfg[1], bool(cfg[2]), bool(cfg[3]))


def _want(x, n, fill_to, cfg):
    return M.rows(x, n, fill_to, np.full(x.shape, M.SENT_F, F32), cfg[0], cfg[1], bool(cfg[2]), bool(cfg[3]))


def _check(sl, x, n, fill_to, cfg, want=None):
    """one call against the model: the whole destination; the source is only read"""
    src = _dev(x)
    dst = S._filled(x.shape)
    out = sl.run(src, n, out=dst, fill_to=fill_to)
    torch.cuda.synchronize()
    assert out is dst
    if want is None:
        want = _want(x, n, fill_to, cfg)
    M.same_bits(dst.cpu().numpy(), want, M.SENT)
    assert np.array_equal(src.cpu().numpy().view(np.uint32).ravel(), x.view(np.uint32).ravel())
    assert sl.last_launches() == int(max(max(n), max(fill_to) if fill_to is not None else 0) > 0)
    return want


FILLS = [lambda n, cap: None, lambda n, cap: [cap] * len(n), lambda n, cap: [max(0, v - 2) for v in n],
         lambda n, cap: [min(cap, (v * 7 + 3) % (cap + 1)) for v in n]]


@pytest.mark.parametrize("part", ["small", "mid", "big"])
def test_k_slide_is_the_model(part):
    """[3][2][5][longest + 3], one row empty: lengths 0, 1, 2, 15, 16, 17, 31, 33, 64, 70 under (W, min, center, norm_vars) = (4, 2, 1, *),
    (8, 3, 0, *), (33, 33, 0, 0), (16, 1, 1, 1); 99, 100, 101, 599, 600, 601, 700 under (600, 100, 0, 0) and (600, 100, 1, 1); 300, 2047, 2049,
    2100 under (2048, 1, 0, 1); every kind of fill_to in rotation; the odd capacities take the lines over every residue against 16
    bytes"""
    cfgs, calls = {"small": M.SMALL, "mid": M.MID, "big": M.BIG}[part]
    i = 0
    for cfg in cfgs:
        sl = _make(cfg)
        try:
            assert sl.tile_frames == 1024 and sl.last_launches() == -1
            for n in calls:
                i += 1
                cap = max(n) + 3
                _check(sl, M.source(n, M.CH, M.LINES, cap, 1000 + i), n, FILLS[i % 4](n, cap), cfg)
        finally:
            sl.close()


@pytest.mark.parametrize("cfg", [(300, 100, 1, 1), (8, 3, 0, 0)])
def test_tile_seams(cfg):
    """identical bits -- the model's -- for three tiles: 16 frames (the smallest), the default, and 48, which divides neither length"""
    n = [700, 0, 257]
    x = M.source(n, 2, 5, 701, 60 + cfg[0])
    sl = _make(cfg)
    try:
        want = _check(sl, x, n, [701, 9, 0], cfg)
        for tile in (16, 48):
            sl.set_tile_frames(tile)
            assert sl.tile_frames == tile and 700 % tile and 257 % tile
            _check(sl, x, n, [701, 9, 0], cfg, want=want)
        for bad in (0, 8, 24, 4112):
            with pytest.raises(ValueError):
                sl.set_tile_frames(bad)
    finally:
        sl.close()


def test_special_values():
    """NaN, +-inf, +-0, subnormals and FLT_MAX in the data, one kind more per row, and a constant line whose variance is at the
    floor: every bit that is not a NaN is the model's, the sign of a zero included"""
    n = [300] * 9
    x = M.source(n, 1, 4, 301, 31, special=True)
    for cfg in ((8, 3, 0, 1), (16, 1, 1, 1), (8, 3, 0, 0), (300, 100, 1, 1)):
        sl = _make(cfg)
        try:
            want = _check(sl, x, n, None, cfg)
            assert (want[:, 0, 0, :300].view(np.uint32) == 0).all()     # the constant line
            assert np.isnan(want[1:, :, :, :300]).any() and not np.isnan(want[0, :, :, :300]).any()
        finally:
            sl.close()


def test_rows_and_channels_do_not_leak():
    """rows of 300, 0, 650 and 17 frames in one call give the bits each gives alone, in another order and with an empty row moved
    between them; nothing outside [0, max(T, fill_to)) of a line is touched"""
    n = [300, 0, 650, 17]
    x = M.source(n, 2, 3, 650, 41)
    cfg = (300, 100, 1, 1)
    sl = _make(cfg)
    try:
        want = _check(sl, x, n, [650, 5, 0, 20], cfg)
        assert (want[1, :, :, :5].view(np.uint32) == 0).all() and (want[1, :, :, 5:].view(np.uint32) == M.SENT).all()
        assert (want[3, :, :, 20:].view(np.uint32) == M.SENT).all()
        order = [2, 3, 1, 0]
        got = _check(sl, x[order], [n[r] for r in order], None, cfg)
        for k, r in enumerate(order):
            M.same_bits(got[k, :, :, :n[r]], want[r, :, :, :n[r]])
        for r in range(4):
            alone = _check(sl, x[r:r + 1], n[r:r + 1], None, cfg)
            M.same_bits(alone[0, :, :, :n[r]], want[r, :, :, :n[r]])
    finally:
        sl.close()


def test_calls_queued_back_to_back_on_one_stream_and_on_a_side_stream():
    """five calls of one object (more than it has record slots), different lengths each, nothing synchronised until the end: on
    torch's current stream, then on a side stream"""
    cfg = (300, 100, 1, 1)
    sl = _make(cfg)
    try:
        x = M.source([700] * 3, 2, 5, 701, 21)
        src = _dev(x)
        for side in (False, True):
            calls = []
            st = torch.cuda.Stream(device=0) if side else torch.cuda.current_stream(0)
            torch.cuda.synchronize()
            with torch.cuda.stream(st):
                for k in range(5):
                    n = [700 - 130 * k, 3 * k, 257 + k]
                    dst = S._filled(x.shape)
                    sl.run(src, n, out=dst, fill_to=[k, 701, 0])
                    calls.append((n, [k, 701, 0], dst))
            st.synchronize()
            for n, fill, dst in calls:
                M.same_bits(dst.cpu().numpy(), _want(x, n, fill, cfg), M.SENT)
    finally:
        sl.close()


def test_refusals_are_value_errors():
    from lewton_amd.rows import SlidingCMVN
    for kw in (dict(cmn_window=0), dict(cmn_window=2049), dict(min_cmn_window=0), dict(cmn_window=50), dict(center=2), dict(norm_vars=-1)):
        with pytest.raises(ValueError):
            SlidingCMVN(**kw)
    sl = SlidingCMVN(300, 100, center=True)
    try:
        assert sl.window(0, 700) == (0, 300) and sl.window(699, 700) == (400, 700) and sl.window(350, 700) == (200, 500)
        n = [300, 0, 650, 17]
        x = _dev(M.source(n, 2, 3, 650, 41))
        bad = [lambda: sl.run(x, [300, 0, 651, 17]), lambda: sl.run(x, n, fill_to=651), lambda: sl.run(x, n[:3]), lambda: sl.run(x, n, out=x),
               lambda: sl.run(x, n, out=S._filled((4, 2, 3, 649))), lambda: sl.run(x[:, :, :, :600], n), lambda: sl.run(x[0], n[:2]),
               lambda: sl.run(x.double(), n), lambda: sl.run(x, [-1, 0, 0, 0]), lambda: sl.window(700, 700), lambda: sl.window(-1, 700)]
        for call in bad:
            with pytest.raises(ValueError):
                call()
        out = sl.run(x, n)                                                # out=None: a zeroed tensor of feats' shape
        torch.cuda.synchronize()
        assert out.shape == x.shape and not out[1].any() and not out[3, :, :, 17:].any() and out[0, :, :, :300].any()
    finally:
        sl.close()


@pytest.mark.parametrize("cfg", [(300, 100, 1, 1), (600, 100, 0, 0), (600, 100, 0, 1), (2048, 1, 0, 1)])
def test_against_torchs_cumulative_sums_in_float64(cfg):
    """the second witness: the same windows from torch.cumsum of the line and of its squares in float64 on the device, (x - mu) and
    1 / sqrt(max(v, 1e-10)) in float64.  Within the model file's bound of the exact value, with what a float64 running sum of T
    terms may itself be off by (T * 2^-53 * the line's sum of magnitudes, at either end of the window) given to the sums"""
    W, mn, center, nv = cfg
    T = 2100 if W > 600 else 700
    x = M.source([T], 1, 3, T, 5 + W)
    sl = _make(cfg)
    try:
        got = sl.run(_dev(x), [T]).cpu().numpy().astype(F64)[0, 0]
    finally:
        sl.close()
    wins = [M.window(t, T, W, mn, bool(center)) for t in range(T)]
    s = torch.tensor([w[0] for w in wins], device="cuda:0")
    e = torch.tensor([w[1] for w in wins], device="cuda:0")
    n = (e - s).double()
    d = _dev(x[0, 0]).double()
    zero = torch.zeros((3, 1), dtype=torch.float64, device="cuda:0")
    c1, c2 = (torch.cat([zero, torch.cumsum(v, dim=1)], dim=1) for v in (d, d * d))
    mu = (c1[:, e] - c1[:, s]) / n
    z = d - mu
    if nv:
        v = (c2[:, e] - c2[:, s]) / n - mu * mu
        z = z / torch.sqrt(torch.clamp(v, min=1e-10))
        z = torch.where((n == 1)[None, :], torch.zeros_like(z), z)
    z = z.cpu().numpy()
    for f in range(3):
        a = np.abs(x[0, 0, f].astype(F64))
        b = M.bound(x[0, 0, f], W, mn, bool(center), bool(nv), extra_S=2 * T * M.U * a.sum(), extra_Q=2 * T * M.U * (a * a).sum())
        ratio = np.abs(got[f] - z[f]) / b
        print("W %d line %d: largest difference %.3g of its bound" % (W, f, ratio.max()))
        assert (ratio <= 1.0).all()


# ---- frame selection: SelectFrames.run (lw_select_rows / k_select_count, k_select) against tests/select_model.py, every bit

import select_model as SM  # noqa: E402

SEL_N, SEL_CAP = [1100, 0, 257, 600], 1103


def _select(se, x, mask, n, fill_to, as_bool=False):
    src = _dev(x)
    dm = _dev(mask)
    dst = S._filled(x.shape)
    out, counts = se.run(src, n, dm.bool() if as_bool else dm, out=dst, fill_to=fill_to)
    torch.cuda.synchronize()
    assert out is dst and counts.dtype == torch.int64 and counts.device == src.device
    want, k = SM.rows(x, mask, n, fill_to, np.full(x.shape, SM.SENT_F, F32))
    SM.same_bits(dst.cpu().numpy(), want)
    assert np.array_equal(counts.cpu().numpy(), k)
    assert np.array_equal(src.cpu().numpy().view(np.uint32).ravel(), x.view(np.uint32).ravel())
    span = max(max(n), max(fill_to) if fill_to is not None else 0)
    assert se.last_launches() == (0 if span == 0 else 2 if max(n) else 1)
    return want, k


@pytest.mark.parametrize("F", [1, 3, 81])
def test_k_select_is_the_model(F):
    """[4][2][F][1103] with lengths 1100, 0, 257 and 600: all-zero, all-one, alternating, random and random-byte masks and one that keeps
    only the last frame; tiles of 256 (the longest row crosses four seams) and the default 1024 (one); the counts, the zeroed tail
    up to max(T, fill_to) and the sentinel beyond it; a bool mask and a uint8 one"""
    from lewton_amd.rows import SelectFrames
    x = SM.source(SEL_N, 2, F, SEL_CAP, 50 + F)
    se = SelectFrames()
    try:
        assert se.tile_frames == 1024 and se.last_launches() == -1
        for i, kind in enumerate(SM.KINDS):
            mask = SM.mask(kind, SEL_N, 2, SEL_CAP, 9 + i)
            for tile in (256, 1024):
                se.set_tile_frames(tile)
                _, k = _select(se, x, mask, SEL_N, FILLS[(i + tile // 1024) % 4](SEL_N, SEL_CAP), as_bool=kind != "bytes" and bool(i % 2))
            if kind in ("zero", "one", "last"):
                assert k[:, 0].tolist() == [{"zero": 0, "one": T, "last": min(T, 1)}[kind] for T in SEL_N]
        for bad in (0, 128, 300, 2304):
            with pytest.raises(ValueError):
                se.set_tile_frames(bad)
    finally:
        se.close()


def test_select_rows_do_not_leak_and_refusals():
    """every row alone gives the bits it gives among the others; calls whose rows are all empty; five calls queued back to back on a
    side stream; each refusal is ValueError"""
    from lewton_amd.rows import SelectFrames
    x = SM.source(SEL_N, 2, 3, SEL_CAP, 41)
    mask = SM.mask("random", SEL_N, 2, SEL_CAP, 3)
    se = SelectFrames()
    try:
        se.set_tile_frames(256)
        together, k = _select(se, x, mask, SEL_N, [SEL_CAP, 5, 0, 700])
        for r in range(4):
            alone, ka = _select(se, x[r:r + 1], mask[r:r + 1], SEL_N[r:r + 1], None)
            SM.same_bits(alone[0, :, :, :SEL_N[r]], together[r, :, :, :SEL_N[r]])
            assert np.array_equal(ka[0], k[r])
        _select(se, x, mask, [0] * 4, None)
        _select(se, x, mask, [0] * 4, [3, 0, SEL_CAP, 1])
        src, dm, calls = _dev(x), _dev(mask), []
        st = torch.cuda.Stream(device=0)
        torch.cuda.synchronize()
        with torch.cuda.stream(st):
            for j in range(5):
                n = [1100 - 200 * j, 3 * j, 257 + j, 600]
                dst = S._filled(x.shape)
                calls.append((n, [j, SEL_CAP, 0, 0], dst, se.run(src, n, dm, out=dst, fill_to=[j, SEL_CAP, 0, 0])[1]))
        st.synchronize()
        for n, fill, dst, counts in calls:
            want, kk = SM.rows(x, mask, n, fill, np.full(x.shape, SM.SENT_F, F32))
            SM.same_bits(dst.cpu().numpy(), want)
            assert np.array_equal(counts.cpu().numpy(), kk)
        bad = [lambda: se.run(src, [1104, 0, 0, 0], dm), lambda: se.run(src, SEL_N, dm, fill_to=1104), lambda: se.run(src, SEL_N[:3], dm),
               lambda: se.run(src, SEL_N, dm, out=src), lambda: se.run(src, SEL_N, dm[:, :1]), lambda: se.run(src, SEL_N, dm.float()),
               lambda: se.run(src, SEL_N, dm.cpu()), lambda: se.run(src, SEL_N, dm, out=S._filled((4, 2, 3, 1102))), lambda: se.run(src[0], SEL_N[:2], dm[0])]
        for call in bad:
            with pytest.raises(ValueError):
                call()
        out, counts = se.run(src, SEL_N, dm)                             # out=None: a zeroed tensor of feats' shape
        torch.cuda.synchronize()
        assert np.array_equal(counts.cpu().numpy(), SM.rows(x, mask, SEL_N, None, np.zeros(x.shape, F32))[1]) and not out[1].any()
    finally:
        se.close()


# ---- the chain

def test_fbank_to_sliding_cmvn_to_selected_frames_to_model_input_is_the_models_composed():
    """three short utterances (5000, 3300 and 0 samples) through KaldiFbank(use_energy=True) -> SlidingCMVN(300, 100, center=True) -> a
    mask on the normalised energy line (a comparison by torch on the device, standing in for any voice-activity decision) ->
    SelectFrames -> FramePack.splice(81, 1, 1), with counts.cpu() the one synchronisation in between: bit for bit kaldi_model ->
    feat_model -> slide_model -> select_model -> pack_model"""
    import feat_model as FM
    import kaldi_model as K
    import pack_model as PM
    from lewton_amd.rows import FramePack, KaldiFbank, SelectFrames, SlidingCMVN
    fb, sl, se, pk = KaldiFbank(num_mel_bins=80, use_energy=True), SlidingCMVN(300, 100, center=True), SelectFrames(), FramePack.splice(81, 1, 1)
    try:
        lengths = [5000, 3300, 0]
        rng = np.random.default_rng(8)
        x = np.full((3, 1, 5003), M.SENT_F, F32)
        for r, n in enumerate(lengths):
            env = 0.02 + (np.sin(np.arange(n) / 300.0 + r) > 0) * 0.5       # bursts: the energy line crosses its window's mean
            x[r, 0, :n] = (rng.standard_normal(n) * env).astype(F32)
        feats, frames = fb.run(S._device(x, False), lengths, fill_to=40)
        cmvn = sl.run(feats, frames, fill_to=40)
        mask = cmvn[:, :, 0, :] > 0.0
        kept, counts = se.run(cmvn, frames, mask.contiguous(), fill_to=40)
        n_kept = counts.cpu().reshape(3).tolist()                            # the one synchronisation
        packed, out_frames, pmask = pk.run(kept, n_kept, fill_to=40, want_mask=True)
        torch.cuda.synchronize()
        T = [K.n_frames(n, 400, 160, True) for n in lengths]
        assert frames.tolist() == T and T[2] == 0 and 0 < n_kept[0] < T[0] and 0 < n_kept[1] < T[1] and n_kept[2] == 0
        lin = np.zeros((3, 1, 81, 40), F32)
        basis = fb.spec.basis()
        for r in range(2):
            lin[r, 0, :, :T[r]] = K.features(basis, fb.banks, K.frame_matrix(x[r, 0, :lengths[r]], 400, 160, True), True, True, 1.0).T
        want, _ = FM.rows(lin, T, [40] * 3, lin, FM.LN, FM.ROW, K.EPS, np.inf, 0.0, 1.0)
        for r in range(2):
            want[r, 0, 0, :T[r]] = np.maximum(want[r, 0, 0, :T[r]], F32(np.log(1.0)))                # energy_floor = 1
        M.same_bits(feats.cpu().numpy(), want)
        want = M.rows(want, T, [40] * 3, np.zeros((3, 1, 81, 40), F32), 300, 100, True, False)
        M.same_bits(cmvn.cpu().numpy(), want)
        wmask = np.zeros((3, 1, 40), np.uint8)
        for r in range(3):
            wmask[r, 0, :T[r]] = want[r, 0, 0, :T[r]] > 0.0
        assert np.array_equal(mask.cpu().numpy()[:, :, :max(T)], wmask[:, :, :max(T)].astype(bool))
        want, k = SM.rows(want, wmask, T, [40] * 3, np.zeros((3, 1, 81, 40), F32))
        SM.same_bits(kept.cpu().numpy(), want)
        assert k.reshape(3).tolist() == n_kept
        want, wm, t_out = PM.rows(want, n_kept, [40] * 3, np.zeros((3, 1, 40, 243), PM.OUT_DTYPE["f32"]), np.zeros((3, 40), np.uint8), 1, 1, 1, PM.REPLICATE,
                                "f32")
        PM.same_bits(packed.cpu().numpy().view(np.uint32), want, "f32")
        assert np.array_equal(pmask.cpu().numpy(), wm) and list(out_frames) == list(t_out) == n_kept
    finally:
        for o in (fb, sl, se, pk):
            o.close()
