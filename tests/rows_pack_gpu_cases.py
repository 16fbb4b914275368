"""Frame-major model input on the GPU: FramePack.run (lw_pack_rows / k_pack).  The cases of tests/test_gpu_rows_pack.py, which runs
this file with pytest in a process of its own, torch imported first (tests/rows_gpu_cases.py says why).

The rule of include/lewton_amd.h ("frame-major model input") is a contract on BITS.  The model is tests/pack_model.py (numpy, the
clamp in Python integers, bf16 by the integer rule, f16 by numpy).  Every comparison with it is over EVERY element of a
sentinel-filled exact-size destination and mask, with no tolerance; the source holds a NaN at and beyond each length."""
import torch  # noqa: F401  (first: see above)

import itertools

import numpy as np
import pytest

import pack_model as M

pytestmark = pytest.mark.gpu

F32 = np.float32
DTYPES = ["f32", "bf16", "f16"]
EDGES = [M.REPLICATE, M.VALID]
TORCH = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
INT = {"f32": torch.int32, "bf16": torch.int16, "f16": torch.int16}


def _signed(v, bits):
    return v - (1 << bits) if v >= 1 << (bits - 1) else v


def _dev(x, off=0):
    """host float32 -> a contiguous device tensor whose data starts `off` BYTES behind a 16-byte boundary"""
    x = np.ascontiguousarray(x, F32)
    flat = torch.empty(x.size + 4, dtype=torch.float32, device="cuda:0")
    t = flat[off // 4:off // 4 + x.size].view(x.shape)
    t.copy_(torch.from_numpy(x))
    assert t.data_ptr() % 16 == off and t.is_contiguous()
    return t


def _filled(shape, dtype, off=0):
    """a sentinel-filled destination of the dtype, `off` bytes behind a 16-byte boundary"""
    es = 4 if dtype == "f32" else 2
    n = int(np.prod(shape))
    flat = torch.empty(n + 16 // es, dtype=TORCH[dtype], device="cuda:0")
    t = flat[off // es:off // es + n].view(shape)
    t.view(INT[dtype]).fill_(_signed(M.sentinel(dtype), 8 * es))
    assert t.data_ptr() % 16 == off and t.is_contiguous()
    return t


def _mask(shape):
    return torch.full(shape, M.SENT_MASK, dtype=torch.uint8, device="cuda:0")


def _bits(t, dtype):
    return t.view(INT[dtype]).cpu().numpy().view(M.OUT_DTYPE[dtype])


def _check(pk, x, n, fill_to, out_cap, mask=True, offs=(0, 0), src=None):
    """one call against the model: the whole destination and mask; the source is only read"""
    R, C, F, cap = x.shape
    src = _dev(x, offs[0]) if src is None else src
    dst = _filled((R, C, out_cap, pk.width), pk.dtype, offs[1])
    msk = _mask((R, out_cap)) if mask else None
    res = pk.run(src, n, out=dst, fill_to=fill_to, want_mask=msk if mask else False)
    torch.cuda.synchronize()
    assert res[0] is dst and len(res) == (3 if mask else 2) and (not mask or res[2] is msk)
    want, wmask, t_out = M.rows(x, n, fill_to, np.full(tuple(dst.shape), M.sentinel(pk.dtype), M.OUT_DTYPE[pk.dtype]),
                                np.full((R, out_cap), M.SENT_MASK, np.uint8) if mask else None, pk.left, pk.right, pk.stride, pk.edge, pk.dtype,
                                pk._shift, pk._scale, pk.pad)
    M.same_bits(_bits(dst, pk.dtype), want, pk.dtype, M.sentinel(pk.dtype))
    if mask:
        assert np.array_equal(msk.cpu().numpy(), wmask)
    assert res[1].dtype == np.uint64 and res[1].tolist() == t_out == [pk.frames(v) for v in n]
    assert np.array_equal(src.cpu().numpy().view(np.uint32).ravel(), x.view(np.uint32).ravel())
    assert pk.last_launches() == int(max(max(t_out), max(fill_to) if fill_to is not None else 0) > 0)
    return want


FILLS = {"none": lambda t, cap: None, "t_out": lambda t, cap: list(t), "capacity": lambda t, cap: [cap] * len(t),
         "below": lambda t, cap: [max(0, v - 2) for v in t], "mixed": lambda t, cap: [min(cap, (v * 7 + 3) % (cap + 1)) for v in t]}
CONTEXTS = [(0, 0, 1), (3, 3, 6), (5, 5, 1), (0, 2, 3), (0, 0, 4), (16, 16, 16), (1, 0, 1), (0, 16, 1)]
LINES = [1, 7, 31, 32, 33, 80]


@pytest.mark.parametrize("ctx", CONTEXTS)
def test_k_pack_is_the_model_on_the_base_shape(ctx):
    """the CPU suite's sweep (tests/test_host_pack.py) on the device: [6][2][F][1031], n_frames out of 0, 1, 2, W - 1, W, W + 1, 255,
    256, 257, 1031, F = 1, 7, 31, 32, 33, 80, the three dtypes; edges, fills, shift / scale / mask and the buffers' residues
    against 16 bytes in rotation"""
    from lewton_amd.rows import FramePack
    left, right, stride = ctx
    W = left + right + 1
    pool = [0, 1, 2, W - 1, W, W + 1, 255, 256, 257, 1031]
    i = CONTEXTS.index(ctx)
    for F, dtype in itertools.product(LINES, DTYPES):
        i += 1
        n = [pool[(i + 3 * r) % len(pool)] for r in range(5)] + [1031]
        edge = EDGES[i % 2]
        t_out = [M.out_frames(T, left, right, stride, edge) for T in n]
        out_cap = max(t_out) + 3
        es = 4 if dtype == "f32" else 2
        D = W * F
        pk = FramePack(F, left, right, stride, edge, dtype, shift=M.vector(D, i) if i % 7 in (1, 2, 4) else None,
                       scale=M.vector(D, i + 1, True) if i % 7 in (2, 3, 4, 5) else None, pad=[0.0, -1.5, 1e-7][i % 3])
        try:
            assert pk.width == D and pk.tile_frames == M.plan(F, W, stride)[0]
            _check(pk, M.source(n, 2, F, 1031, 1000 * i + F), n, FILLS[sorted(FILLS)[i % 5]](t_out, out_cap), out_cap, mask=bool(i % 4),
                   offs=(4 * (i % 4), 0 if i % 3 == 0 else es * (i % (16 // es))))
        finally:
            pk.close()


@pytest.mark.parametrize("stride,tile", [(1, 256), (2, 128), (4, 64), (6, 32), (16, 16)])
def test_tile_seams(stride, tile):
    """every tile plan, REPLICATE with left = right = 16: rows of k tiles - 1, k tiles and k tiles + 1 output frames for k = 1 and 3,
    so the halo crosses a seam and both ends of the row"""
    from lewton_amd.rows import FramePack
    t_out = [k * tile + d for k in (1, 3) for d in (-1, 0, 1)]
    n = [v * stride - (r % stride) for r, v in enumerate(t_out)]
    for dtype in DTYPES:
        pk = FramePack(8, 16, 16, stride, "replicate", dtype)
        try:
            assert pk.tile_frames == tile and [pk.frames(v) for v in n] == t_out
            _check(pk, M.source(n, 2, 8, max(n) + 1, 60 + stride), n, [max(t_out) + 2] * 6, max(t_out) + 2)
        finally:
            pk.close()


@pytest.mark.parametrize("F", [1, 31, 32, 33, 63, 64, 65, 80, 257])
def test_line_groups(F):
    """F across the 32-line groups of the image, W = 1 and 7, the three dtypes: odd D under bf16 and f16 (a frame is then not
    dword-aligned), odd capacities, a row of two tiles and a short one"""
    from lewton_amd.rows import FramePack
    n = [300, 5]
    x = M.source(n, 1, F, 301, 50 + F)
    for (left, right), dtype in itertools.product(((0, 0), (3, 3)), DTYPES):
        pk = FramePack(F, left, right, 1, "replicate", dtype, pad=1.0)
        try:
            _check(pk, x, n, [0, 9], 301)
        finally:
            pk.close()


def test_special_values():
    """+-0, subnormals, +-inf, NaNs, 0x7f7fffff, the f16 overflow boundary, f16 subnormal ties and bf16 ties: through the copy,
    through shift and scale, and as pad; f32 without shift and scale keeps NaN payloads"""
    from lewton_amd.rows import FramePack
    n = [300, 7]
    x = M.source(n, 1, 8, 301, 31, special=True)
    for dtype in DTYPES:
        for pad in M.SPECIALS[[1, 11, 14, 18, 5]]:
            pk = FramePack.lfr(8, dtype=dtype, pad=float(pad))
            try:
                _check(pk, x, n, [60, 60], 60)
                assert pk.convert(pad) == int(M.convert(np.array([pad], F32), dtype)[0])
            finally:
                pk.close()
        for kw in (dict(shift=M.vector(8, 1), scale=M.vector(8, 2, True)), dict(scale=np.full(8, 1.0, F32))):
            pk = FramePack.transpose(8, dtype=dtype, **kw)
            try:
                _check(pk, x, n, None, 300, offs=(4, 8))
            finally:
                pk.close()
    pk = FramePack.transpose(8)
    try:
        out, _ = pk.run(_dev(x), n)
        assert np.array_equal(_bits(out, "f32")[0, 0, :300], x[0, 0, :, :300].T.view(np.uint32))   # a bit copy, payloads included
        assert np.isnan(x[0, 0, :, :300]).any()
    finally:
        pk.close()


# ---- the conversion, exhaustively

def _rule(u, dtype):
    """the header's integer rule on int64 bit patterns, in torch integer operations; NaN inputs give any value (masked by the caller)"""
    if dtype == "bf16":
        return (u + 0x7FFF + ((u >> 16) & 1)) >> 16
    s, a = (u >> 16) & 0x8000, u & 0x7FFFFFFF
    m = a - 0x38000000
    normal = (m + 0xFFF + ((m >> 13) & 1)) >> 13
    sh = torch.clamp(126 - (a >> 23), 14, 24)
    M_ = (a & 0x7FFFFF) | 0x800000
    r = M_ >> sh
    one = torch.ones_like(a)
    rem, half = M_ & ((one << sh) - 1), one << (sh - 1)
    sub = r + ((rem > half) | ((rem == half) & ((r & 1) == 1))).to(torch.int64)
    out = torch.where(a >= 0x47800000, torch.full_like(a, 0x7C00), torch.where(a >= 0x38800000, normal, torch.where(a < 0x33000000, torch.zeros_like(a), sub)))
    return s | out


@pytest.mark.parametrize("part", range(16))
@pytest.mark.parametrize("dtype", ["bf16", "f16"])
def test_every_f32_bit_pattern(dtype, part):
    """all 2^32 patterns in 16 calls of 2^28 through FramePack.transpose(1, dtype=...), made and compared on the device: equal to the
    integer rule on every non-NaN input, NaN -> NaN; torch's own conversion is the second witness"""
    from lewton_amd.rows import FramePack
    n = 1 << 28
    u = torch.arange(part * n, (part + 1) * n, dtype=torch.int64, device="cuda:0")
    src = torch.where(u >= 1 << 31, u - (1 << 32), u).to(torch.int32).view(torch.float32).view(1, 1, 1, n)
    pk = FramePack.transpose(1, dtype=dtype)
    try:
        out, frames = pk.run(src, [n])
        assert frames.tolist() == [n] and tuple(out.shape) == (1, 1, n, 1)
        got = out.view(torch.int16).view(n).to(torch.int64) & 0xFFFF
        nan_in = (u & 0x7FFFFFFF) > 0x7F800000
        nan_out = (got & 0x7FFF) > (0x7F80 if dtype == "bf16" else 0x7C00)
        assert bool((nan_in == nan_out).all()), "a NaN must stay a NaN and nothing else become one"
        bad = (got != _rule(u, dtype)) & ~nan_in
        assert not bool(bad.any()), [hex(v) for v in u[bad][:4].tolist()]
        del bad
        witness = src.view(n).to(TORCH[dtype]).view(torch.int16).to(torch.int64) & 0xFFFF
        bad = (got != witness) & ~nan_in
        assert not bool(bad.any()), [hex(v) for v in u[bad][:4].tolist()]
    finally:
        pk.close()


# ---- rows, channels, mask

def test_rows_and_channels_do_not_leak():
    """rows of 300, 0, 1000 and 17 frames and 3 channels in one call give the bits each gives alone in a call; everything else is
    the sentinel (checked by _check); the source is unchanged"""
    from lewton_amd.rows import FramePack
    n = [300, 0, 1000, 17]
    x = M.source(n, 3, 7, 1000, 41)
    pk = FramePack.lfr(7, dtype="bf16")
    try:
        want = _check(pk, x, n, [170, 5, 0, 20], 170)
        assert (want[1, :, :5] == 0).all() and (want[1, :, 5:] == M.SENT16).all()
        for r in range(4):
            alone = _check(pk, x[r:r + 1], n[r:r + 1], None, 170)
            k = pk.frames(n[r])
            assert np.array_equal(alone[0, :, :k], want[r, :, :k])
        src = _dev(x)
        for bad in (lambda: pk.run(src, [300, 0, 1001, 17]), lambda: pk.run(src, n, fill_to=171, out=_filled((4, 3, 170, 49), "bf16")),
                    lambda: pk.run(src, n[:3]), lambda: pk.run(src, n, out=_filled((4, 3, 166, 49), "bf16")),
                    lambda: pk.run(src, n, out=_filled((4, 3, 170, 49), "f16")), lambda: pk.run(src[:, :, :6], n),
                    lambda: pk.run(src, n, want_mask=_mask((4, 169)))):
            with pytest.raises(ValueError):
                bad()
    finally:
        pk.close()


def test_mask_and_counts():
    """the mask is arange < T_out on [0, fill_end) and the sentinel beyond, the same for 1 and 3 channels; out_frames is
    lw_pack_frames; the default out holds the largest of the frames and fill_to and is zero beyond them"""
    from lewton_amd.rows import FramePack
    n = [300, 0, 45, 17, 6]
    fill = [10, 4, 20, 0, 9]
    for edge in EDGES:
        pk = FramePack(5, 0, 6, 3, edge, "f16", pad=-2.0)
        try:
            masks = []
            for C in (1, 3):
                x = M.source(n, C, 5, 300, 70 + C)
                msk = _mask((5, 101))
                _, frames, got = pk.run(_dev(x), n, out=_filled((5, C, 101, 35), "f16"), fill_to=fill, want_mask=msk)
                t_out = [M.out_frames(T, 0, 6, 3, edge) for T in n]
                assert frames.tolist() == t_out and got is msk
                h = msk.cpu().numpy()
                for r in range(5):
                    end = max(t_out[r], fill[r])
                    assert np.array_equal(h[r, :end], (np.arange(end) < t_out[r]).astype(np.uint8)) and (h[r, end:] == M.SENT_MASK).all()
                masks.append(h)
                _check(pk, x, n, fill, 101)
            assert np.array_equal(masks[0], masks[1])
            out, frames, msk = pk.run(_dev(x), n, fill_to=fill, want_mask=True)
            cap = max(frames.tolist() + fill)
            assert tuple(out.shape) == (5, 3, cap, 35) and out.dtype == torch.float16 and tuple(msk.shape) == (5, cap)
            assert np.array_equal(msk.cpu().numpy(), np.arange(cap)[None, :] < frames[:, None].astype(np.int64))
        finally:
            pk.close()


def test_calls_queued_back_to_back_on_one_stream():
    """five calls of one object (more than it has record slots), different lengths each, on a side stream, the host arrays
    overwritten as soon as each call returns, nothing synchronised until the end"""
    from lewton_amd.rows import FramePack
    sh, sc = M.vector(49, 5), M.vector(49, 6, True)
    pk = FramePack.lfr(7, shift=sh, scale=sc, dtype="bf16")
    try:
        assert pk.last_launches() == -1
        x = M.source([700] * 3, 2, 7, 701, 21)
        src = _dev(x)
        calls = []
        st = torch.cuda.Stream(device=0)
        torch.cuda.synchronize()
        with torch.cuda.stream(st):
            for k in range(5):
                n = np.array([700 - 130 * k, 3 * k, 257 + k], np.uint64)
                fill = np.array([k, 117, 0], np.uint64)
                dst, msk = _filled((3, 2, 117, 49), "bf16"), _mask((3, 117))
                pk.run(src, n, out=dst, fill_to=fill, want_mask=msk)
                calls.append((n.tolist(), fill.tolist(), dst, msk))
                n[:] = 9
                fill[:] = 99
        st.synchronize()
        for n, fill, dst, msk in calls:
            want, wmask, _ = M.rows(x, n, fill, np.full((3, 2, 117, 49), M.SENT16, np.uint16), np.full((3, 117), M.SENT_MASK, np.uint8), 3, 3, 6,
                                    M.REPLICATE, "bf16", sh, sc)
            M.same_bits(_bits(dst, "bf16"), want, "bf16", M.SENT16)
            assert np.array_equal(msk.cpu().numpy(), wmask)
    finally:
        pk.close()


# ---- the chain

def test_samples_to_lfr_input_is_the_models_composed():
    """[4][1][5000] samples -> KaldiFbank(num_mel_bins=80) -> FramePack.lfr(80, shift=, scale=, dtype="bf16"): the kaldi model, the
    log model and pack_model composed, bit for bit.  With dtype="f32" and no affine step: exactly torch's clamped index_select,
    permute and reshape of the features"""
    import feat_model as FM
    import kaldi_model as K
    import rows_fbank_gpu_cases as FB
    from lewton_amd.rows import FramePack, KaldiFbank
    fb = KaldiFbank(num_mel_bins=80)
    sh, sc = M.vector(560, 3), M.vector(560, 4, True)
    pk, plain = FramePack.lfr(80, shift=sh, scale=sc, dtype="bf16"), FramePack.lfr(80)
    try:
        n = 5000
        lengths = [n, n, n, 0]
        x = np.full((4, 1, n + 3), FB.SENT_F, F32)
        for r, s in enumerate(FB._signals(n)):
            x[r, 0, :n] = s.astype(F32)
        feats, frames = fb.run(FB._device(x, False), lengths)
        T = K.n_frames(n, 400, 160, True)
        assert frames.tolist() == [T, T, T, 0]
        out, out_frames, mask = pk.run(feats, frames, fill_to=6, want_mask=True)
        torch.cuda.synchronize()
        lin = np.zeros((4, 1, 80, T), F32)
        for r in range(3):
            lin[r, 0, :, :T] = K.features(fb.spec.basis(), fb.banks, K.frame_matrix(x[r, 0, :n], 400, 160, True), True, False, 1.0).T
        logs, _ = FM.rows(lin, frames.tolist(), None, lin, FM.LN, FM.ROW, K.EPS, np.inf, 0.0, 1.0)
        cap = -(-T // 6)
        assert cap == 5                                                        # filled to 6: one frame of padding per row
        want, wmask, t_out = M.rows(logs, frames.tolist(), [6] * 4, np.zeros((4, 1, 6, 560), np.uint16), np.zeros((4, 6), np.uint8), 3, 3, 6,
                                    M.REPLICATE, "bf16", sh, sc)
        assert out_frames.tolist() == t_out == [cap] * 3 + [0] and tuple(out.shape) == (4, 1, 6, 560)
        M.same_bits(_bits(out, "bf16"), want, "bf16")
        assert np.array_equal(mask.cpu().numpy(), wmask)
        got, _ = plain.run(feats, frames)
        idx = torch.clamp(torch.arange(cap, device="cuda:0")[:, None] * 6 - 3 + torch.arange(7, device="cuda:0")[None, :], 0, T - 1)
        ref = feats[:3, 0].index_select(2, idx.reshape(-1)).reshape(3, 80, cap, 7).permute(0, 2, 3, 1).reshape(3, cap, 560)
        assert torch.equal(got[:3, 0].view(torch.int32), ref.contiguous().view(torch.int32)) and not bool(got[3].any())
    finally:
        fb.close()
        pk.close()
        plain.close()


# ---- 65535 rows

NR = 65540
LIVE = [0, 1, 7, 32768, 40000, 65533, 65534, 65535, 65536, 65537, 65538, 65539]      # the second launch starts at row 65535


@pytest.mark.parametrize("dtype", DTYPES)
def test_65540_rows(dtype):
    """[65540][2][3][12] -> LFR 3/2, a dozen rows live on both sides of the cut between the launches, each with a length of its own:
    the live rows equal the model, every other element of the destination and the mask is still the sentinel (compared on the
    device)"""
    from lewton_amd.rows import FramePack
    assert sum(r < 65535 for r in LIVE) == 7 and NR - 1 in LIVE
    pk = FramePack.lfr(3, 3, 2, dtype=dtype, pad=0.5)
    try:
        n = [12 - i for i in range(len(LIVE))]
        t_out = [pk.frames(v) for v in n]
        fill = [min(7, v + 1) for v in t_out]
        x = M.source(n, 2, 3, 12, 80)
        src = torch.empty((NR, 2, 3, 12), dtype=torch.float32, device="cuda:0")
        src.view(torch.int32).fill_(_signed(M.SENT, 32))
        src[LIVE] = torch.from_numpy(x).to("cuda:0")
        dst, msk = _filled((NR, 2, 7, 9), dtype), _mask((NR, 7))
        counts, fills = [0] * NR, [0] * NR
        for r, a, b in zip(LIVE, n, fill):
            counts[r], fills[r] = a, b
        pk.run(src, counts, out=dst, fill_to=fills, want_mask=msk)
        torch.cuda.synchronize()
        assert pk.last_launches() == 2
        want, wmask, _ = M.rows(x, n, fill, np.full((len(LIVE), 2, 7, 9), M.sentinel(dtype), M.OUT_DTYPE[dtype]),
                                np.full((len(LIVE), 7), M.SENT_MASK, np.uint8), 1, 1, 2, M.REPLICATE, dtype, pad=0.5)
        M.same_bits(_bits(dst[LIVE], dtype), want, dtype, M.sentinel(dtype))
        assert np.array_equal(msk[LIVE].cpu().numpy(), wmask)
        iv, im = dst.view(INT[dtype]).clone(), msk.clone()
        iv[LIVE] = _signed(M.sentinel(dtype), 32 if dtype == "f32" else 16)
        im[LIVE] = M.SENT_MASK
        assert bool((iv == _signed(M.sentinel(dtype), 32 if dtype == "f32" else 16)).all()) and bool((im == M.SENT_MASK).all()), "written outside the live rows"
    finally:
        pk.close()
