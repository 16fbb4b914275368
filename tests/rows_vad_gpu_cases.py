"""Energy voice-activity decisions of feature rows on the GPU: EnergyVad.run (lw_vad_rows / k_vad, k_vad_sum, k_vad_fold,
k_vad_decide).  The cases of tests/test_gpu_rows_vad.py, which runs this file with pytest in a process of its own, torch imported
first (tests/rows_gpu_cases.py says why).

The rule of include/lewton_amd.h ("energy voice-activity decisions of feature rows") is a contract on BITS, the order of its double
sum included.  The model is tests/vad_model.py.  Every comparison with it is over EVERY byte of a sentinel-filled exact-size mask
and every threshold, with no tolerance; the source holds a NaN at and beyond each length."""
import torch  # noqa: F401  (first: see above)

import numpy as np
import pytest

import vad_model as M
import rows_spec_gpu_cases as S

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
N, CAP = [1100, 0, 257, 600], 1103


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to("cuda:0")


def _make(cfg, line=0):
    from lewton_amd.rows import EnergyVad
    return EnergyVad(cfg[0], cfg[1], cfg[2], cfg[3], line)


def _sentinel(shape):
    return torch.full(shape, M.SENT_MASK, dtype=torch.uint8, device="cuda:0")


def _launches(vad_cfg, n, fill_to, route, want_thr=True):
    span = max(max(n), max(fill_to) if fill_to is not None else 0)
    if span == 0:
        return int(want_thr)
    sums = vad_cfg[1] != 0 and max(n) > 0
    return 3 if sums and (route == "split" or (route == "auto" and span > 16384)) else 1


def _check(vad, x, n, fill_to, cfg, route="auto", line=0, want=None, src=None):
    """one call against the model: the whole mask and every threshold; the source is only read"""
    vad.set_route(route)
    if src is None:
        src = _dev(x)
    R, C, F, cap = x.shape
    dst = _sentinel((R, C, cap))
    mask, thr = vad.run(src, n, out=dst, fill_to=fill_to, want_threshold=True)
    torch.cuda.synchronize()
    assert mask.dtype == torch.bool and mask.data_ptr() == dst.data_ptr() and tuple(mask.shape) == (R, C, cap)
    assert thr.dtype == torch.float32 and tuple(thr.shape) == (R, C)
    if want is None:
        want = M.rows(x, n, fill_to, np.full((R, C, cap), M.SENT_MASK, np.uint8), cfg, line)
    M.same_mask(dst.cpu().numpy(), want[0])
    M.same_thr(thr.cpu().numpy(), want[1])
    assert np.array_equal(src.cpu().numpy().view(np.uint32).ravel(), x.view(np.uint32).ravel())
    assert vad.last_launches() == _launches(cfg, n, fill_to, route)
    return want


FILLS = [lambda n, cap: None, lambda n, cap: [cap] * len(n), lambda n, cap: [max(0, v - 2) for v in n],
         lambda n, cap: [min(cap, (v * 7 + 3) % (cap + 1)) for v in n]]


@pytest.mark.parametrize("F", [1, 3, 81])
def test_k_vad_is_the_model(F):
    """[4][2][F][1103] with lengths 1100, 0, 257 and 600, the energy in line 0 and in line F - 1 (every other line NaN), a context of
    0, 2 and 256 frames, tiles of 256 (five in the longest row) and 1024 (two), both routes, every kind of fill_to in rotation; the
    odd capacity takes the rows and channels over every residue of the mask against 4 bytes and of the line against 16"""
    i = 0
    for line in sorted({0, F - 1}):
        x = M.source(N, 2, F, CAP, 50 + F + line, line_i=line, others_nan=bool(line))
        src = _dev(x)
        for ctx, prop in ((0, 0.6), (2, 0.12), (256, 0.6), (2, 0.6)):
            cfg = (6.0, 0.5, ctx, prop)
            vad = _make(cfg, line)
            try:
                assert vad.tile_frames == 1024 and vad.last_launches() == -1
                for tile in (256, 1024):
                    vad.set_tile_frames(tile)
                    for route in ("fused", "split"):
                        i += 1
                        want = _check(vad, x, N, FILLS[i % 4](N, CAP), cfg, route, line, src=src)
                assert ctx or 0.0 < want[0][0, :, :1100].mean() < 1.0       # both decisions occur
            finally:
                vad.close()


@pytest.mark.parametrize("T", [0, 1, 2, 255, 256, 257, 16384, 16385, 40000])
def test_lengths_where_the_tree_changes_shape(T):
    """no frame, one, a short chunk, a whole one, two, 64 chunks (ONE tree, the fused form's longest row), 65 (two fold levels, the
    split form by itself) and 157 (40000 frames); up to 16384 frames fused == split == the model"""
    cap = T + 3
    x = M.source([T, min(T, 5)], 2, 2, cap, 300 + T % 1000, line_i=1)
    fill = [T if T == 16384 else cap, 0]                                  # (the fused form's limit is on max(T, fill_to))
    vad = _make(M.SRE, 1)
    try:
        if T <= 16384:
            want = _check(vad, x, [T, min(T, 5)], fill, M.SRE, "fused", 1)
            _check(vad, x, [T, min(T, 5)], fill, M.SRE, "split", 1, want=want)
        want = _check(vad, x, [T, min(T, 5)], fill, M.SRE, "auto", 1)
        assert T < 255 or 0.0 < want[0][0, :, :T].mean() < 1.0
        if T > 16384:
            vad.set_route("fused")
            with pytest.raises(ValueError):
                vad.run(_dev(x), [T, 5])
    finally:
        vad.close()


def test_fused_is_split_is_the_model_on_one_input():
    """the route forced, at three tiles each: 256, the default and 768, which divides neither length; identical bits, the model's"""
    n = [3000, 700, 0, 257]
    x = M.source(n, 2, 3, 3001, 60)
    src = _dev(x)
    for cfg in (M.SRE, (5.5, 0.5, 2, 0.6), (5.0, 0.5, 256, 0.3)):
        vad = _make(cfg)
        try:
            want = None
            for tile in (256, 1024, 768):
                vad.set_tile_frames(tile)
                assert vad.tile_frames == tile and (tile == 256 or (3000 % tile and 700 % tile))
                for route in ("fused", "split", "auto"):
                    want = _check(vad, x, n, [3001, 9, 5, 0], cfg, route, want=want, src=src)
            for bad in (0, 128, 300, 2304):
                with pytest.raises(ValueError):
                    vad.set_tile_frames(bad)
            with pytest.raises(ValueError):
                vad.set_route("both")
        finally:
            vad.close()


def test_special_values():
    """NaN, +-inf and +-0 in the energy line, one kind more per row: with a mean, an infinity or a NaN of the line reaches its
    threshold (a NaN threshold unvoices the row); without a mean it decides its own frame alone"""
    n = [300] * 6
    x = M.source(n, 1, 2, 301, 31, special=True)
    for cfg in ((5.0, 0.5, 2, 0.6), (5.0, 0.0, 1, 0.12), (0.0, 0.0, 0, 0.6)):
        vad = _make(cfg)
        try:
            for route in ("fused", "split"):
                mask, thr = _check(vad, x, n, None, cfg, route)
            if cfg[1]:
                assert np.isnan(thr[5]).all() and not mask[5, :, :300].any() and np.isfinite(thr[:3]).all() and mask[0, :, :300].any()
            else:
                assert mask[5, :, :300].any() and (thr == F32(cfg[0])).all()
        finally:
            vad.close()


def test_rows_and_channels_do_not_leak():
    """rows of 1100, 0, 257 and 600 frames in one call give the bits each gives alone and in another order; the other lines are NaN
    and never reach the result; nothing outside [0, max(T, fill_to)) of a row and channel is touched"""
    x = M.source(N, 2, 3, CAP, 41, line_i=1, others_nan=True)
    cfg = (5.5, 0.5, 2, 0.6)
    vad = _make(cfg, 1)
    try:
        mask, thr = _check(vad, x, N, [CAP, 5, 0, 700], cfg, "fused", 1)
        assert (mask[1, :, :5] == 0).all() and (mask[1, :, 5:] == M.SENT_MASK).all() and (mask[3, :, 700:] == M.SENT_MASK).all()
        assert np.isfinite(thr).all() and (thr[1] == F32(5.5)).all() and thr[0, 0] != thr[0, 1]
        order = [2, 3, 1, 0]
        got, gthr = _check(vad, x[order], [N[r] for r in order], None, cfg, "split", 1)
        for k, r in enumerate(order):
            assert np.array_equal(got[k, :, :N[r]], mask[r, :, :N[r]]) and gthr[k].tobytes() == thr[r].tobytes()
        for r in range(4):
            alone, ta = _check(vad, x[r:r + 1], N[r:r + 1], None, cfg, "auto", 1)
            assert np.array_equal(alone[0, :, :N[r]], mask[r, :, :N[r]]) and ta[0].tobytes() == thr[r].tobytes()
    finally:
        vad.close()


def test_without_a_mean_and_calls_with_nothing_to_write():
    """energy_mean_scale == 0: the decide launch alone whatever the route, every threshold energy_threshold, a NaN line harmless; with
    no byte to write the thresholds alone are filled, and without them nothing is queued"""
    cfg = (12.0, 0.0, 2, 0.6)
    x = M.source(N, 2, 2, CAP, 43)
    vad = _make(cfg)
    try:
        for route in ("auto", "fused", "split"):
            mask, thr = _check(vad, x, N, [CAP, 5, 0, 700], cfg, route)
            assert vad.last_launches() == 1 and (thr == F32(12.0)).all() and 0.1 < mask[0, :, :1100].mean() < 0.9
        _check(vad, x, [0] * 4, None, cfg)
        assert vad.last_launches() == 1
        _check(vad, x, [0] * 4, [3, 0, CAP, 1], cfg)
        out = vad.run(_dev(x), [0] * 4)
        assert vad.last_launches() == 0 and out.dtype == torch.bool and not out.any()
    finally:
        vad.close()


def test_calls_queued_back_to_back_on_one_stream_and_on_a_side_stream():
    """five calls of one object (more than it has record slots), different lengths each, the routes in rotation, nothing
    synchronised until the end: on torch's current stream, then on a side stream"""
    cfg = M.SRE
    vad = _make(cfg)
    try:
        x = M.source([700] * 3, 2, 2, 701, 21)
        src = _dev(x)
        for side in (False, True):
            calls = []
            st = torch.cuda.Stream(device=0) if side else torch.cuda.current_stream(0)
            torch.cuda.synchronize()
            with torch.cuda.stream(st):
                for k in range(5):
                    n = [700 - 130 * k, 3 * k, 257 + k]
                    dst = _sentinel((3, 2, 701))
                    vad.set_route(("fused", "split", "auto")[k % 3])
                    calls.append((n, [k, 701, 0], dst, vad.run(src, n, out=dst, fill_to=[k, 701, 0], want_threshold=True)[1]))
            st.synchronize()
            for n, fill, dst, thr in calls:
                want, wthr = M.rows(x, n, fill, np.full((3, 2, 701), M.SENT_MASK, np.uint8), cfg)
                M.same_mask(dst.cpu().numpy(), want)
                M.same_thr(thr.cpu().numpy(), wthr)
    finally:
        vad.close()


def test_refusals_are_value_errors():
    from lewton_amd.rows import EnergyVad
    for kw in (dict(energy_threshold=float("inf")), dict(energy_mean_scale=-1.0), dict(frames_context=257), dict(proportion_threshold=0.0),
               dict(proportion_threshold=1.0), dict(line=-1), dict(device=-1)):
        with pytest.raises(ValueError):
            EnergyVad(**kw)
    vad = EnergyVad(5.5, 0.5, 2, 0.6)
    try:
        assert vad.voiced(3, 5) and vad.voiced(6, 10) and not vad.voiced(2, 5)            # the pinned f32 products
        assert vad.threshold(1024.0, 128) == F32(9.5) and vad.threshold(float("nan"), 0) == F32(5.5)
        assert vad.threshold(1e300, 3) == F32(np.inf)
        x = _dev(M.source(N, 2, 3, CAP, 41))
        bad = [lambda: vad.run(x, [1104, 0, 0, 0]), lambda: vad.run(x, N, fill_to=1104), lambda: vad.run(x, N[:3]),
               lambda: vad.run(x, N, out=torch.zeros((4, 2, 1102), dtype=torch.uint8, device="cuda:0")),
               lambda: vad.run(x, N, out=torch.zeros((4, 2, 1103), dtype=torch.float32, device="cuda:0")),
               lambda: vad.run(x, N, out=torch.zeros((4, 2, 1103), dtype=torch.uint8)), lambda: vad.run(x[:, :, :, :600], N), lambda: vad.run(x[0], N[:2]),
               lambda: vad.run(x.double(), N), lambda: vad.run(x, [-1, 0, 0, 0]), lambda: vad.voiced(6, 5), lambda: vad.threshold(1.0, -1)]
        for call in bad:
            with pytest.raises(ValueError):
                call()
        with pytest.raises(ValueError):                                           # line 3 of three lines
            v3 = EnergyVad(line=3)
            try:
                v3.run(x, N)
            finally:
                v3.close()
        out = vad.run(x, N, out=torch.zeros((4, 2, 1103), dtype=torch.bool, device="cuda:0"))   # a bool out; out=None is above
        torch.cuda.synchronize()
        assert out.dtype == torch.bool and not out[1].any() and out[0, :, :1100].any() and not out[3, :, 600:].any()
    finally:
        vad.close()


@pytest.mark.parametrize("T", [256, 1024, 4096])
def test_kaldi_restatement_on_exact_inputs(T):
    """energies that are multiples of 2^-6 in [-8, 24) under (5.5, 0.5, 2, 0.6): every sum is exact in Kaldi's sequential order and in
    the tree's, so the kernel's thresholds and masks are IDENTICAL to voice-activity-detection.cc restated (tests/vad_model.kaldi)"""
    cfg = (5.5, 0.5, 2, 0.6)
    x = np.stack([M.exact_line(T, 11 + T), M.exact_line(T, 12 + T)])[:, None, None, :]
    vad = _make(cfg)
    try:
        for route in ("fused", "split"):
            mask, thr = _check(vad, x, [T, T], None, cfg, route)
            for r in range(2):
                want, kthr = M.kaldi(x[r, 0, 0], T, cfg)
                assert thr[r, 0].tobytes() == kthr.tobytes() and np.array_equal(mask[r, 0], want) and 0.2 < want.mean() < 0.8
    finally:
        vad.close()


# ---- the chain

CHAIN_LENGTHS, CHAIN_SEED, CHAIN_CAP = [24000, 16000, 0], 8, 150


def chain_signal():
    """three utterances of noise in bursts: envelope 0.0005 + 0.5 * (sin(i / 1500 + r) > 0)"""
    rng = np.random.default_rng(CHAIN_SEED)
    x = np.full((3, 1, max(CHAIN_LENGTHS) + 3), M.SENT_F, F32)
    for r, n in enumerate(CHAIN_LENGTHS):
        env = 0.0005 + 0.5 * (np.sin(np.arange(n) / 1500.0 + r) > 0)
        x[r, 0, :n] = (rng.standard_normal(n) * env).astype(F32)
    return x


def test_fbank_to_energy_vad_to_sliding_cmvn_to_selected_frames_to_model_input_is_the_models_composed():
    """utterances of 24000, 16000 and 0 samples through KaldiFbank(num_mel_bins=80, use_energy=True, scale=32768: Kaldi's 16-bit sample
    range, which vad.conf's 5.5 is meant for) -> EnergyVad(5.5, 0.5, 2, 0.12) on the RAW features -> SlidingCMVN(300, 100,
    center=True) -> SelectFrames with that mask -> FramePack.splice(81, 1, 1), with counts.cpu() the one synchronisation in
    between: bit for bit kaldi_model -> feat_model -> vad_model -> slide_model -> select_model -> pack_model.  The context changes
    decisions (kept != the raw count) and some frames go (0 < kept < T) in both rows"""
    import feat_model as FM
    import kaldi_model as K
    import pack_model as PM
    import select_model as SM
    import slide_model as SL
    from lewton_amd.rows import EnergyVad, FramePack, KaldiFbank, SelectFrames, SlidingCMVN
    fb, vad, sl = KaldiFbank(num_mel_bins=80, use_energy=True, scale=32768.0), EnergyVad(5.5, 0.5, 2, 0.12), SlidingCMVN(300, 100, center=True)
    se, pk = SelectFrames(), FramePack.splice(81, 1, 1)
    try:
        lengths, cap = CHAIN_LENGTHS, CHAIN_CAP
        x = chain_signal()
        feats, frames = fb.run(S._device(x, False), lengths, fill_to=cap)
        mask = vad.run(feats, frames, fill_to=cap)
        cmvn = sl.run(feats, frames, fill_to=cap)
        kept, counts = se.run(cmvn, frames, mask, fill_to=cap)
        n_kept = counts.cpu().reshape(3).tolist()                            # the one synchronisation
        packed, out_frames, pmask = pk.run(kept, n_kept, fill_to=cap, want_mask=True)
        torch.cuda.synchronize()
        T = [K.n_frames(n, 400, 160, True) for n in lengths]
        assert frames.tolist() == T == [148, 98, 0]
        lin = np.zeros((3, 1, 81, cap), F32)
        basis = fb.spec.basis()
        for r in range(2):
            lin[r, 0, :, :T[r]] = K.features(basis, fb.banks, K.frame_matrix(x[r, 0, :lengths[r]], 400, 160, True), True, True, 32768.0).T
        want, _ = FM.rows(lin, T, [cap] * 3, lin, FM.LN, FM.ROW, K.EPS, np.inf, 0.0, 1.0)
        for r in range(2):
            want[r, 0, 0, :T[r]] = np.maximum(want[r, 0, 0, :T[r]], F32(np.log(1.0)))                # energy_floor = 1
        K.same_bits(feats.cpu().numpy(), want)
        wmask, wthr = M.rows(want, T, [cap] * 3, np.zeros((3, 1, cap), np.uint8), M.SRE)
        M.same_mask(mask.cpu().numpy(), wmask)
        raw = [int((want[r, 0, 0, :T[r]] > wthr[r, 0]).sum()) for r in range(3)]
        k = [int(wmask[r, 0, :T[r]].sum()) for r in range(3)]
        print("chain: frames %r, raw decisions %r, voiced %r, thresholds %r" % (T, raw, k, wthr.ravel().tolist()))
        assert all(0 < k[r] < T[r] and k[r] != raw[r] for r in range(2)) and k[2] == 0
        wcm = SL.rows(want, T, [cap] * 3, np.zeros((3, 1, 81, cap), F32), 300, 100, True, False)
        SL.same_bits(cmvn.cpu().numpy(), wcm)
        wsel, wk = SM.rows(wcm, wmask, T, [cap] * 3, np.zeros((3, 1, 81, cap), F32))
        SM.same_bits(kept.cpu().numpy(), wsel)
        assert wk.reshape(3).tolist() == n_kept == k
        wp, wm, t_out = PM.rows(wsel, n_kept, [cap] * 3, np.zeros((3, 1, cap, 243), PM.OUT_DTYPE["f32"]), np.zeros((3, cap), np.uint8), 1, 1, 1, PM.REPLICATE,
                                "f32")
        PM.same_bits(packed.cpu().numpy().view(np.uint32), wp, "f32")
        assert np.array_equal(pmask.cpu().numpy(), wm) and list(out_frames) == list(t_out) == n_kept
    finally:
        for o in (fb, vad, sl, se, pk):
            o.close()
