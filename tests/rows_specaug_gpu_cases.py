"""SpecAugment masks over feature rows on the GPU: SpecAugment.run (lw_specaug_rows / k_specaug).  The cases of
tests/test_gpu_rows_specaug.py, which runs this file with pytest in a process of its own, torch imported first
(tests/rows_gpu_cases.py says why).

The rule of include/lewton_amd.h ("masking feature rows") is a contract on BITS.  The model is tests/specaug_model.py.  Every
comparison with it is over EVERY element of an exact-size tensor as uint32, with no tolerance: out of place the destination is
sentinel-filled before the call, in place the source holds another sentinel at and beyond each length; the spans are compared as
int64."""
import torch  # noqa: F401  (first: see above)

import numpy as np
import pytest

import specaug_model as M

pytestmark = pytest.mark.gpu

F32, U32 = np.float32, np.uint32
N, CAP = [1100, 0, 1, 3, 255, 256, 257, 1023, 1024, 1025], 1103      # the odd capacity puts the lines at every residue against 16 bytes
IDS = [3 * i + 1 for i in range(len(N))]
TILES = (256, 1024, 2048)


def _dev(bits):
    return torch.from_numpy(np.ascontiguousarray(bits, U32).view(F32)).to("cuda:0")


def _host(t):
    return t.cpu().numpy().view(U32)


def _make(P, **kw):
    """the object of a model's parameters (the fill through its float32 value: its bits arrive)"""
    from lewton_amd.rows import SpecAugment
    from fractions import Fraction
    p = Fraction(P.ratio_num, P.ratio_den) if P.ratio_den else 1.0
    return SpecAugment(P.num_t, P.max_t, P.num_f, P.max_f, P.min_t, P.min_f, p, P.per_channel, np.array(P.fill_bits, U32).view(F32)[()], P.seed, **kw)


def _launches(P, n, fill_to, in_place, want_spans):
    span = max([max(n)] + ([fill_to] * len(n) if isinstance(fill_to, int) else list(fill_to) if fill_to is not None else []))
    fill = [fill_to] * len(n) if isinstance(fill_to, int) else fill_to
    fills = fill is not None and any(f > v for f, v in zip(fill, n))
    writes = (fills or (P.masks and max(n) > 0)) if in_place else span > 0
    return int(bool(writes or (want_spans and P.masks)))


def _check(sa, P, x, n, fill_to, ids, in_place, want_spans=True):
    """one call against the model: every element and every span; out of place the source is only read"""
    src = _dev(x)
    dst = src if in_place else torch.empty_like(src).view(torch.int32).fill_(M.SENT_DST).view(torch.float32)
    before = x if in_place else np.full(x.shape, M.SENT_DST, U32)
    got = sa.run(src, n, ids=ids, out=None if in_place else dst, fill_to=fill_to, want_spans=want_spans)
    torch.cuda.synchronize()
    out, spans = got if want_spans else (got, None)
    assert out.data_ptr() == dst.data_ptr()
    want, wspans = M.rows(P, x, n, fill_to, ids, before)
    M.same_bits(_host(dst), want)
    if want_spans:
        assert spans.dtype == torch.int64 and np.array_equal(spans.cpu().numpy(), wspans)
    if not in_place:
        M.same_bits(_host(src), x)
    assert sa.last_launches() == _launches(P, n, fill_to, in_place, want_spans)
    return want, wspans


FILLS = [lambda n, cap: None, lambda n, cap: [cap] * len(n), lambda n, cap: [max(0, v - 2) for v in n],
         lambda n, cap: [min(cap, (v * 7 + 3) % (cap + 1)) for v in n]]


# ---- 1. the kernel equals the model

@pytest.mark.parametrize("F,ch", [(1, 1), (1, 2), (3, 1), (3, 2), (80, 1), (80, 2)])
def test_k_specaug_is_the_model(F, ch):
    """[10][ch][F][1103] with lengths 1100, 0, 1, 3, 255, 256, 257, 1023, 1024 and 1025 under tiles of 256, 1024 and 2048, in place
    and out of place, every kind of fill_to in rotation; the WeNet preset's widths, and five wide time masks that meet the tile
    seams and the rows' ends.  Out of place everything outside [0, max(T, fill_to)) is still the sentinel"""
    x = M.source(N, ch, F, CAP, 60 + F + ch, special=True)
    i = 0
    for P in (M.Params(seed=2024, min_t=1, max_t=50, min_f=1, max_f=min(10, F), per_channel=ch > 1, fill_bits=0x7FC12345),
              M.Params(seed=11, num_t=5, min_t=0, max_t=700, num_f=1, max_f=min(2, F), fill_bits=0x80000000)):
        sa = _make(P)
        try:
            assert sa.tile_frames == 2048 and sa.last_launches() == -1
            for tile in TILES:
                sa.set_tile_frames(tile)
                for in_place in (False, True):
                    i += 1
                    fill = FILLS[i % 4](N, CAP)
                    want, _ = _check(sa, P, x, N, fill, IDS if i % 3 else None, in_place, want_spans=bool(i % 2))
                    if not in_place:
                        for r, T in enumerate(N):
                            assert (want[r, :, :, max(T, fill[r] if fill else 0):] == M.SENT_DST).all()
            live = want[0, :, :, :1100]
            assert (live == P.fill_bits).any() and (F < 80 or (live != P.fill_bits).any())      # (frequency masks may hold all of a few lines)
        finally:
            sa.close()


# ---- 2. ids picked WITH the model

def test_masks_at_the_ends_at_a_seam_empty_overlapping_and_whole_rows():
    """a mask that starts at 0, one that ends at T, one that crosses the seam of two tiles of 256, an empty one, two that overlap,
    and one that covers the whole of a row of 3 frames: each found in the model first, then asked of the GPU"""
    P = M.Params(seed=2024, num_t=2, min_t=0, max_t=50, num_f=0)
    T = 600
    found = {}
    for id_ in range(20000):
        (a0, b0), (a1, b1) = M.plan(P, id_, 0, T, 1)
        for what, hit in (("starts at 0", a0 == 0 and b0 > 0), ("ends at T", b0 == T and a0 < T), ("crosses a seam", a0 < 256 < b0 or a0 < 512 < b0),
                          ("empty", a0 == b0), ("overlap", a0 < b1 and a1 < b0 and a0 != a1)):
            if hit:
                found.setdefault(what, id_)
        if len(found) == 5:
            break
    assert len(found) == 5, found
    ids = [found[w] for w in ("starts at 0", "ends at T", "crosses a seam", "empty", "overlap")]
    x = M.source([T] * 5, 1, 1, T + 3, 8)
    sa = _make(P)
    try:
        sa.set_tile_frames(256)
        for in_place in (False, True):
            want, spans = _check(sa, P, x, [T] * 5, None, ids, in_place)
        s = spans[:, 0, 0]
        assert s[0, 0] == 0 and s[1, 1] == T and s[3, 0] == s[3, 1] and (want[0, 0, 0, 0] == 0) and (want[1, 0, 0, T - 1] == 0)
    finally:
        sa.close()
    Q = M.Params(seed=2024, num_t=1, min_t=5, max_t=50, num_f=0)
    assert M.plan(Q, 7, 0, 3, 1) == [(0, 3)]
    x = M.source([3, 3], 2, 1, 7, 9)
    sa = _make(Q)
    try:
        want, _ = _check(sa, Q, x, [3, 3], [5, 0], [7, 7], False)
        assert (want[:, :, 0, :3] == 0).all() and (want[0, :, 0, 3:5] == 0).all() and (want[0, :, 0, 5:] == M.SENT_DST).all()
    finally:
        sa.close()


# ---- 3. fill bits and special sources

@pytest.mark.parametrize("bits", [0x00000000, 0x80000000, 0x7FC12345, 0xFF800000])
def test_fill_bits_and_special_sources(bits):
    """+0.0, -0.0, a NaN with a payload and -inf as the fill; the sources hold NaN payloads, infinities, subnormals and -0.0, which
    are bit copies where unmasked"""
    n = [300, 0, 40]
    x = M.source(n, 2, 3, 301, 12, special=True)
    P = M.Params(seed=4, num_t=2, max_t=80, num_f=1, min_f=1, max_f=2, fill_bits=bits)
    sa = _make(P)
    try:
        sa.set_tile_frames(256)
        for in_place in (False, True):
            want, _ = _check(sa, P, x, n, [301, 2, 0], None, in_place)
        live = want[0, :, :, :300]
        assert (live == bits).any() and all((live == v).any() for v in M.ODD_BITS)
    finally:
        sa.close()


# ---- 4. determinism

def test_masks_depend_on_seed_and_id_alone():
    """the same id gives the same mask at another row position, in another batch size and under another tile; another seed or id gives
    other spans; ids=None equals arange"""
    T, F = 700, 5
    P = M.Params(seed=77, num_t=3, max_t=100, num_f=2, max_f=3)
    x1 = M.source([T], 1, F, T, 5)
    sa = _make(P)
    try:
        alone, s_alone = _check(sa, P, x1, [T], None, [42], False)
        for tile, pos, rows in ((256, 0, 3), (2048, 2, 3), (1024, 4, 6)):
            sa.set_tile_frames(tile)
            xs = M.source([T] * rows, 1, F, T, 6)
            xs[pos] = x1[0]
            ids = [1000 + r for r in range(rows)]
            ids[pos] = 42
            got, s = _check(sa, P, xs, [T] * rows, None, ids, True)
            assert np.array_equal(got[pos], alone[0]) and np.array_equal(s[pos], s_alone[0])
            assert all(not np.array_equal(s[r], s_alone[0]) for r in range(rows) if r != pos)
        x4 = M.source([T] * 4, 1, F, T, 7)
        a, sa_spans = _check(sa, P, x4, [T] * 4, None, None, False)
        b, sb_spans = _check(sa, P, x4, [T] * 4, None, list(range(4)), False)
        assert np.array_equal(a, b) and np.array_equal(sa_spans, sb_spans)
        assert sa.plan(42, T, F) == [tuple(int(v) for v in p) for p in s_alone[0, 0]]
    finally:
        sa.close()
    Q = M.Params(seed=78, num_t=3, max_t=100, num_f=2, max_f=3)
    sq = _make(Q)
    try:
        _, s_other = _check(sq, Q, x1, [T], None, [42], False)
        assert not np.array_equal(s_other, s_alone)
    finally:
        sq.close()


# ---- 5. per_channel

def test_per_channel():
    """off: the channels of a row are masked alike; on: every channel is a group of its own, per the model"""
    n = [500, 300]
    x = M.source(n, 2, 8, 501, 3)
    for per_channel in (False, True):
        P = M.Params(seed=9, num_t=2, max_t=60, num_f=1, min_f=1, max_f=4, per_channel=per_channel, fill_bits=0x7FC12345)
        sa = _make(P)
        try:
            want, spans = _check(sa, P, x, n, None, [11, 12], False)
            filled = want == 0x7FC12345
            assert spans.shape == (2, 2 if per_channel else 1, 3, 2)
            assert all(np.array_equal(filled[r, 0], filled[r, 1]) for r in range(2)) != per_channel
            _check(sa, P, x, n, None, [11, 12], True)
        finally:
            sa.close()


# ---- 6. want_spans == plan == model

def test_spans_are_the_plan_are_the_model():
    P = M.Params(seed=(1 << 63) + 5, num_t=4, min_t=3, max_t=200, ratio=(1, 5), num_f=3, min_f=0, max_f=9, per_channel=True)
    n = [1000, 0, 17, 3]
    ids = [0, (1 << 64) - 1, (1 << 40) + 3, 6099]
    x = M.source(n, 2, 12, 1001, 14)
    sa = _make(P)
    try:
        _, spans = _check(sa, P, x, n, None, ids, True)
        for r in range(4):
            for g in range(2):
                assert sa.plan(ids[r], n[r], 12, group=g) == M.plan(P, ids[r], g, n[r], 12) == [tuple(int(v) for v in p) for p in spans[r, g]]
        assert all(b - a <= 200 for a, b in M.plan(P, 0, 0, 1000, 12)[:4]) and all(b - a <= 3 for a, b in M.plan(P, ids[2], 0, 17, 12)[:4])
        big = M.Params(seed=2024, num_t=32, max_t=65535, num_f=0)
        sb = _make(big)
        try:
            assert sb.plan(6099, (1 << 32) + (1 << 20) + 5, 1)[18] == (4294953827, 4294968123)
        finally:
            sb.close()
        for bad in (lambda: sa.plan(-1, 10, 1), lambda: sa.plan(0, 1 << 63, 1), lambda: sa.plan(0, 10, 65536), lambda: sa.plan(0, 10, 1, group=65536),
                    lambda: sa.plan(0.5, 10, 1)):
            with pytest.raises(ValueError):
                bad()
    finally:
        sa.close()


# ---- 7. queuing

def test_calls_queued_back_to_back_on_one_stream_and_on_a_side_stream():
    """five calls of one object (more than it has record slots), different lengths and ids each, in place and out of place in
    rotation, nothing synchronised until the end: on torch's current stream, then on a side stream"""
    P = M.Params(seed=31, num_t=2, max_t=120, num_f=1, min_f=1, max_f=2, fill_bits=0xFF800000)
    sa = _make(P)
    try:
        x = M.source([700] * 3, 2, 3, 701, 21)
        for side in (False, True):
            calls = []
            st = torch.cuda.Stream(device=0) if side else torch.cuda.current_stream(0)
            torch.cuda.synchronize()
            with torch.cuda.stream(st):
                for k in range(5):
                    n, ids, fill = [700 - 130 * k, 3 * k, 257 + k], [k, 100 + k, 7], [k, 701, 0]
                    in_place = bool(k % 2)
                    src = _dev(x)
                    dst = src if in_place else torch.empty_like(src).view(torch.int32).fill_(M.SENT_DST).view(torch.float32)
                    out, spans = sa.run(src, n, ids=ids, out=None if in_place else dst, fill_to=fill, want_spans=True)
                    calls.append((n, ids, fill, in_place, out, spans))
            st.synchronize()
            for n, ids, fill, in_place, out, spans in calls:
                want, wspans = M.rows(P, x, n, fill, ids, x if in_place else np.full(x.shape, M.SENT_DST, U32))
                M.same_bits(_host(out), want)
                assert np.array_equal(spans.cpu().numpy(), wspans)
    finally:
        sa.close()


# ---- 8. refusals

def test_refusals_are_value_errors():
    from lewton_amd.rows import SpecAugment
    for kw in (dict(num_time_masks=33), dict(time_mask_param=65536), dict(min_time=51), dict(min_freq=11), dict(p=1.5), dict(per_channel=2),
               dict(seed=-1), dict(device=-1), dict(fill="0")):
        with pytest.raises(ValueError):
            SpecAugment(**kw)
    sa = SpecAugment(seed=5)
    try:
        x = _dev(M.source(N[:4], 2, 3, CAP, 41))
        n = N[:4]
        out = torch.empty_like(x).view(torch.int32).fill_(M.SENT_DST).view(torch.float32)
        bad = [lambda: sa.run(x, [1104, 0, 0, 0], out=out), lambda: sa.run(x, n, out=out, fill_to=1104), lambda: sa.run(x, n[:3], out=out),
               lambda: sa.run(x, n, out=out, ids=[1, 2, 3]), lambda: sa.run(x, n, out=out, ids=[1, 2, 3, -1]), lambda: sa.run(x, n, out=out, ids=[1, 2, 3, 1 << 64]),
               lambda: sa.run(x, n, out=out[:, :, :, :600]), lambda: sa.run(x, n, out=out.double()), lambda: sa.run(x, n, out=out.cpu()),
               lambda: sa.run(x[:, :, :, :600], n, out=out), lambda: sa.run(x.double(), n), lambda: sa.run(x[0, 0], n[:3]), lambda: sa.run(x, [-1, 0, 0, 0], out=out),
               lambda: sa.set_tile_frames(300), lambda: sa.set_tile_frames(0), lambda: sa.set_tile_frames(2304)]
        for call in bad:
            with pytest.raises(ValueError):
                call()
        torch.cuda.synchronize()
        assert bool((out.view(torch.int32) == M.SENT_DST).all()) and sa.last_launches() == -1
        wave = sa.run(x[:, :, 0, :].contiguous(), n)                              # a waveform [rows][C][capacity] is F = 1
        torch.cuda.synchronize()
        assert wave.dim() == 3 and sa.last_launches() == 1
        lb, ld, wn = SpecAugment.paper("LB"), SpecAugment.paper("LD", seed=3), SpecAugment.wenet(seed=3)
        try:
            assert (lb.num_time_masks, lb.num_freq_masks, ld.num_time_masks, ld.num_freq_masks, wn.num_time_masks, wn.num_freq_masks) == (1, 1, 2, 2, 2, 2)
            P = M.Params(seed=3, min_t=1, max_t=50, min_f=1, max_f=10)
            assert wn.plan(9, 3000, 80) == M.plan(P, 9, 0, 3000, 80)
            assert ld.plan(9, 3000, 80) == M.plan(M.Params(seed=3, max_t=100, max_f=27), 9, 0, 3000, 80)
        finally:
            for o in (lb, ld, wn):
                o.close()
    finally:
        sa.close()


# ---- 9. the chain

def test_fbank_to_cmvn_to_specaug_to_lfr_input_is_the_models_composed():
    """utterances of 24000, 16000 and 0 samples through KaldiFbank(num_mel_bins=80) -> Normalize.cmvn() -> SpecAugment.wenet(seed=5)
    with ids -> FramePack.lfr(80): bit for bit kaldi_model -> feat_model -> norm_model -> specaug_model -> pack_model"""
    import feat_model as FM
    import kaldi_model as K
    import norm_model as NM
    import pack_model as PM
    import rows_vad_gpu_cases as V
    import rows_spec_gpu_cases as S
    from lewton_amd.rows import FramePack, KaldiFbank, Normalize, SpecAugment
    fb, nm, sa, pk = KaldiFbank(num_mel_bins=80), Normalize.cmvn(), SpecAugment.wenet(seed=5), FramePack.lfr(80)
    try:
        lengths, cap, ids = V.CHAIN_LENGTHS, V.CHAIN_CAP, [901, 17, 4]
        x = V.chain_signal()
        feats, frames = fb.run(S._device(x, False), lengths, fill_to=cap)
        nm.run(feats, frames, fill_to=cap)
        _, spans = sa.run(feats, frames, ids=ids, fill_to=cap, want_spans=True)
        packed, out_frames = pk.run(feats, frames, fill_to=cap)
        torch.cuda.synchronize()
        T = [K.n_frames(n, 400, 160, True) for n in lengths]
        assert frames.tolist() == T == [148, 98, 0]
        lin = np.zeros((3, 1, 80, cap), F32)
        basis = fb.spec.basis()
        for r in range(2):
            lin[r, 0, :, :T[r]] = K.features(basis, fb.banks, K.frame_matrix(x[r, 0, :lengths[r]], 400, 160, True), True, False, 1.0).T
        want, _ = FM.rows(lin, T, [cap] * 3, lin, FM.LN, FM.ROW, K.EPS, np.inf, 0.0, 1.0)
        want, _ = NM.rows(want, T, [cap] * 3, want, 1, NM.STD, NM.LINE, 1e-20, 1.0)
        P = M.Params(seed=5, min_t=1, max_t=50, min_f=1, max_f=10)
        wbits, wspans = M.rows(P, want.view(U32), T, [cap] * 3, ids, want.view(U32))
        M.same_bits(_host(feats), wbits)
        assert np.array_equal(spans.cpu().numpy(), wspans)
        masked = [int((wbits[r, 0, :, :T[r]] == 0).sum()) for r in range(2)]
        print("chain: frames %r, spans %r, masked elements %r" % (T, wspans[:, 0].tolist(), masked))
        assert all(m >= T[r] + 80 - 1 for r, m in enumerate(masked))               # at least one frame and one bin each
        wp, _, t_out = PM.rows(wbits.view(F32), T, [cap] * 3, np.zeros(tuple(packed.shape), PM.OUT_DTYPE["f32"]), None, 3, 3, 6, PM.REPLICATE, "f32")
        PM.same_bits(packed.cpu().numpy().view(U32), wp, "f32")
        assert list(out_frames) == list(t_out)
    finally:
        for o in (fb, nm, sa, pk):
            o.close()
