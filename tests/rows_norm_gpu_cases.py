"""Normalising rows on the GPU: Normalize.run (lw_norm_rows / k_norm_sum, k_norm_fold, k_norm_apply) and normalize= of
decode_ogg_files.  The cases of tests/test_gpu_rows_norm.py, which runs this file with pytest in a process of its own, torch
imported first (tests/rows_gpu_cases.py says why).

The rule of include/lewton_amd.h ("normalising rows") is a contract on BITS, the order of its double sums included.  The model is
tests/norm_model.py (numpy float64, the pair trees as v[0::2] + v[1::2]).  Every comparison is over EVERY element of a
sentinel-filled destination and every stat, with no tolerance; the source holds a NaN at and beyond each length."""
import torch  # noqa: F401  (first: see above)

import functools
import itertools
import os

import numpy as np
import pytest

import feat_model as FM
import norm_model as M
import rows_feat_gpu_cases as FC
import rows_spec_gpu_cases as S
from common import ROOT

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
KIND = {None: M.NONE, "std": M.STD, "rms": M.RMS, "peak": M.PEAK}


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to("cuda:0")


def _launches(nm, n, fill_to, want_stats):
    plain = not nm.center and nm.scale is None
    span = max(max(n), max(fill_to) if fill_to is not None else 0)
    return (0 if plain else int(max(n) > 0) + 1) + int(plain and want_stats) + int(span > 0)


def _check(nm, x, n, fill_to, inplace, want_stats, squeeze=False):
    """one call against the model: the whole destination, and the stats.  squeeze: [rows][C][1][cap] goes as the 3-D tensor"""
    shape = x.shape[:2] + x.shape[3:] if squeeze else x.shape
    src = _dev(x.reshape(shape))
    dst = src if inplace else S._filled(shape)
    before = x if inplace else np.full(x.shape, M.SENT_F, F32)
    r = nm.run(src, n, out=None if inplace else dst, fill_to=fill_to, want_stats=want_stats)
    torch.cuda.synchronize()
    out, st = r if want_stats else (r, None)
    assert out is dst
    want, stats = M.rows(x, n, fill_to, before, int(nm.center), KIND[nm.scale], M.SCOPES[nm.scope], nm.eps, nm.target)
    M.same_bits(dst.cpu().numpy().reshape(x.shape), want, M.SENT)
    if not inplace:
        assert np.array_equal(src.cpu().numpy().view(np.uint32).ravel(), x.view(np.uint32).ravel())       # the source is only read
    if want_stats:
        got = st.cpu().numpy()
        assert got.shape == (stats.shape if not (squeeze and nm.scope == "line") else stats.shape[:2] + (2,))
        M.same_bits(got.reshape(stats.shape), stats)
    assert nm.last_launches() == _launches(nm, n, fill_to, want_stats)
    return want, stats


BASE_N = [0, 1, 3, 4, 5, 255, 256, 257, 1031]
FILLS = {"none": lambda n, cap: None, "n": lambda n, cap: list(n), "capacity": lambda n, cap: [cap] * len(n),
         "below": lambda n, cap: [max(0, v - 2) for v in n], "above": lambda n, cap: [min(cap, v + 3) for v in n]}


@pytest.mark.parametrize("scale", [None, "std", "rms", "peak"])
def test_k_norm_is_the_model_on_the_base_shape(scale):
    """[3][2][3][1031], lines at every alignment against 16 bytes; n = 0, 1, 3, 4, 5, 255, 256, 257, 1031 three at a time across
    calls; the three scopes, centred or not, in place and out of place, fill_to absent, at, below and above n and at the capacity,
    the stats asked for or not"""
    from lewton_amd.rows import Normalize
    made = {}
    try:
        for i, (scope, center, inplace) in enumerate(itertools.product(("row", "channel", "line"), (True, False), (False, True))):
            nm = made[scope, center] = made.get((scope, center)) or Normalize(center, scale, 1e-7 if (i // 2) % 2 else 0.0, 0.5, scope)
            for k in range(3):
                n = [BASE_N[(3 * k + i + j * (k + 1)) % 9] for j in range(3)] if i % 4 else BASE_N[3 * k:3 * k + 3]
                fill = FILLS[sorted(FILLS)[(i + k) % len(FILLS)]](n, 1031)
                x = M.source(n, 2, 3, 1031, 500 + 3 * i + k, offset=0.3 * (i % 3))
                _check(nm, x, n, fill, inplace, want_stats=(i + k) % 3 != 1)
    finally:
        for nm in made.values():
            nm.close()


@pytest.mark.parametrize("n", [16127, 16383, 16384, 16385, 1_048_577])
def test_list_level_boundaries_of_one_line(n):
    """63 and 64 chunks take the wave fold, 65 the workgroup fold with two levels, 4097 three; as a 3-D waveform tensor"""
    from lewton_amd.rows import Normalize
    nm = Normalize.wav2vec2()
    try:
        x = M.source([n], 1, 1, n + 2, 7, offset=-0.2)
        _check(nm, x, [n], [n + 1], n == 16385, True, squeeze=True)
    finally:
        nm.close()


def test_a_row_scope_whose_list_crosses_lines_mid_group():
    """ch = 2, F = 3, n = 5500: six lines of 22 chunks, a list of 132, so groups of 64 end in the middle of a line"""
    from lewton_amd.rows import Normalize
    nm = Normalize(True, "std", 1e-7, 1.0, "row")
    try:
        x = M.source([5500, 300], 2, 3, 5501, 5, offset=0.1)
        _check(nm, x, [5500, 300], [5501, 0], False, True)
    finally:
        nm.close()


@pytest.mark.parametrize("scale,center", [(None, False), ("peak", False), ("std", True), ("rms", False)])
def test_special_values(scale, center):
    """NaN, +-inf, +-0, subnormals and FLT_MAX in the data, one kind more per row: every bit that is not a NaN is the model's, the
    sign of a zero and a subnormal result included; a NaN in the data makes the peak, and with it g, a NaN"""
    from lewton_amd.rows import Normalize
    nm = Normalize(center, scale, 1e-7, 1.0, "channel")
    try:
        n = [700] * 9
        x = M.source(n, 1, 2, 701, 31, special=True)
        want, stats = _check(nm, x, n, None, False, True)
        if scale == "peak":
            assert np.isnan(stats[8, 0, 1]) and stats[5, 0, 1] == 1.0 / float(np.finfo(F32).max) and stats[6, 0, 1] == 0.0
        if scale is None:
            keep = ~np.isnan(x[..., :700])
            assert np.array_equal(want[..., :700].view(np.uint32)[keep], x[..., :700].view(np.uint32)[keep])             # a bit copy
    finally:
        nm.close()


@functools.lru_cache(maxsize=None)
def _million_scopes():
    """[256][1][4096][4] and its chunk triples.  With n = 4 only lane 0 of a chunk holds data, and a tree of (t, +0.0 x 63) is
    t + 0.0, whatever the level: that shortcut spares a gigabyte of zero padding, and row 0 is put through the model proper"""
    rng = np.random.default_rng(43)
    x = (rng.standard_normal((256, 1, 4096, 4)) * 10.0 ** rng.uniform(-12, 12, (256, 1, 4096, 1))).astype(F32)
    x[:, :, 7, :] = x[:, :, 7, :1]
    x[:, :, 9, :] = 0.0
    x[:, :, 11, :] = -0.0
    d = x.astype(F64)
    a = (((d[..., 0] + d[..., 1]) + d[..., 2]) + d[..., 3]) + 0.0
    b = (((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]) + d[..., 3] * d[..., 3]) + 0.0
    pk = (x.view(np.uint32) & np.uint32(0x7FFFFFFF)).max(axis=-1)
    a0, b0, pk0 = M.chunk_triples(x[0], 4)
    assert np.array_equal(a0[..., 0].view(np.uint64), a[0].view(np.uint64)) and np.array_equal(b0[..., 0].view(np.uint64), b[0].view(np.uint64))
    assert np.array_equal(pk0[..., 0], pk[0])
    return x, a, b, pk.view(F32)


@pytest.mark.parametrize("scale,eps", [("std", 1e-7), ("std", 0.0), ("rms", 1e-7), ("rms", 0.0)])
def test_the_devices_scalars_are_the_models_on_a_million_scopes(scale, eps):
    """[256][1][4096][4] with scope "line": 1 048 576 scopes of four elements, each one chunk, so S1 and S2 are four-term sums and
    (m, g) come straight from the device's division and its sqrt expansion.  Levels over 24 decades, a constant line (v clamps to
    0), a line of +0.0 and one of -0.0 in every row"""
    from lewton_amd.rows import Normalize
    x, a, b, pk = _million_scopes()
    nm = Normalize(True, scale, eps, 0.25, "line")
    try:
        _, st = nm.run(_dev(x), [4] * 256, out=S._filled(x.shape), want_stats=True)
        torch.cuda.synchronize()
        m, g = M.scalars(1, KIND[scale], eps, 0.25, a, b, pk, np.full(a.shape, 4, np.uint64))
        got = st.cpu().numpy()
        differ = int((got[..., 1].view(np.uint64) != g.view(np.uint64)).sum())
        print("%s eps %g: g differs on %d of %d scopes" % (scale, eps, differ, g.size))
        M.same_bits(got[..., 0], m)
        M.same_bits(got[..., 1], g)
    finally:
        nm.close()


@pytest.mark.parametrize("scope", ["row", "channel", "line"])
def test_rows_do_not_leak_and_both_fold_plans_agree_with_the_model(scope):
    """rows of different lengths and an empty row in one call: every row's stats are what the row has alone in a call.  The call
    with a row of 17 000 has more than 64 chunks in a scope (the workgroup fold, also for its short rows), the call without it at
    most 64 in every scope (the wave fold)"""
    from lewton_amd.rows import Normalize
    nm = Normalize(True, "std", 1e-7, 1.0, scope)
    try:
        for n in ([300, 0, 17000, 17], [300, 0, 1000, 17]):
            x = M.source(n, 2, 2, max(n) + 1, 41)
            want, stats = _check(nm, x, n, [1000, 5, 0, 20], False, True)
            assert (stats[1].reshape(-1, 2) == [0.0, 1.0]).all()
            for r in range(4):
                M.same_bits(stats[r:r + 1], M.rows(x[r:r + 1], n[r:r + 1], None, x[r:r + 1], 1, M.STD, M.SCOPES[scope])[1])
    finally:
        nm.close()


def test_one_launch_for_copy_and_fill_and_the_host_scalars():
    from lewton_amd.rows import Normalize
    nm = Normalize(False, None, scope="line")
    try:
        assert nm.last_launches() == -1
        n = [20, 0, 700]
        x = M.source(n, 2, 3, 701, 2)
        _check(nm, x, n, [701, 5, 0], False, want_stats=False)
        assert nm.last_launches() == 1
        _check(nm, x, n, None, True, want_stats=True)
        assert nm.last_launches() == 2                                       # the fold alone writes the (0, 1) that are owed
        with pytest.raises(ValueError):
            nm.run(_dev(x), [20, 0, 702])
        with pytest.raises(ValueError):
            nm.run(_dev(x), n, fill_to=702)
        with pytest.raises(ValueError):
            nm.run(_dev(x), [20, 0])
        with pytest.raises(ValueError):
            nm.run(_dev(x), n, out=S._filled((3, 2, 3, 700)))
    finally:
        nm.close()
    nm = Normalize.wav2vec2()
    try:
        for q in ((12.5, 40.0, 3.0, 100), (-3.0, 9.0, 1.0, 1), (0.0, 0.0, 0.0, 7), (1.0, 2.0, 0.5, 0)):
            m, g = M.scalars(1, M.STD, 1e-7, 1.0, *q) if q[3] else (0.0, 1.0)
            assert nm.scalars(*q) == (float(m), float(g))
    finally:
        nm.close()


def test_calls_queued_back_to_back_on_one_stream():
    """five calls of one object (more than it has record slots), different lengths each, on a side stream, nothing synchronised
    until the end"""
    from lewton_amd.rows import Normalize
    nm = Normalize.cmvn()
    try:
        x = M.source([700] * 3, 2, 3, 701, 21)
        src = _dev(x)
        calls = []
        st = torch.cuda.Stream(device=0)
        torch.cuda.synchronize()
        with torch.cuda.stream(st):
            for k in range(5):
                n = [700 - 130 * k, 3 * k, 257 + k]
                dst = S._filled(x.shape)
                _, stats = nm.run(src, n, out=dst, fill_to=[k, 701, 0], want_stats=True)
                calls.append((n, [k, 701, 0], dst, stats))
        st.synchronize()
        for n, fill, dst, stats in calls:
            want, ws = M.rows(x, n, fill, np.full(x.shape, M.SENT_F, F32), 1, M.STD, M.LINE, 1e-20)
            M.same_bits(dst.cpu().numpy(), want, M.SENT)
            M.same_bits(stats.cpu().numpy(), ws)
    finally:
        nm.close()


# ---- the pipeline

def test_decode_ogg_files_normalize_is_the_model_over_the_plain_call():
    """tests/golden/invalid_keypress.ogg to 16 kHz mono: with normalize="wav2vec2" the rows are the numpy model of the rows
    without it, zero beyond the length; without it the call is what it was, the resampler over the native decode"""
    from lewton_amd.rows import Normalize, Resampler, decode_ogg_files
    path = os.path.join(ROOT, "tests", "golden", "invalid_keypress.ogg")
    kw = dict(sample_rate=16000, channels="mono")
    plain, lengths, rate = decode_ogg_files([path], **kw)
    native, nat_len, nat_rate = decode_ogg_files([path], channels="mono")
    rs = Resampler(nat_rate, 16000)
    try:
        want = rs.run(native, nat_len.tolist())
        torch.cuda.synchronize()
        n = rs.out_len(int(nat_len[0]))
    finally:
        rs.close()
    assert rate == 16000 and int(lengths[0]) == n and n > 256
    p = plain.cpu().numpy()
    assert np.array_equal(p[:, :, :n].view(np.uint32), want.cpu().numpy()[:, :, :n].view(np.uint32)) and not p[:, :, n:].any()
    model, _ = M.rows(p[:, :, None, :], [n], None, p[:, :, None, :], 1, M.STD, M.CHANNEL, 1e-7)
    for normalize in ("wav2vec2", Normalize.wav2vec2()):
        got, l2, r2 = decode_ogg_files([path], normalize=normalize, **kw)
        assert r2 == 16000 and l2.tolist() == lengths.tolist() and got.shape == plain.shape
        M.same_bits(got.cpu().numpy(), model[:, :, 0, :])
        if not isinstance(normalize, str):
            normalize.close()
    z = got.cpu().numpy()[0, 0, :n].astype(F64)
    assert abs(z.mean()) < 1e-6 and 0.5 < z.std() < 1.0 + 1e-6
    peak, _, _ = decode_ogg_files([path], normalize="peak", **kw)
    assert float(peak.abs().max()) == 1.0
    for bad in (dict(samples="i16"), dict(samples="f32_interleaved"), dict(normalize="cmvn")):
        with pytest.raises(ValueError):
            decode_ogg_files([path], **dict(dict(kw, normalize="wav2vec2"), **bad))


def test_rows_to_cmvn_features_is_the_models_composed():
    """[3][1][4000] with lengths 4000, 1601 and 0 through the reflect spectrogram with 80 slaney bands, LogCompress (ln, no clamp)
    and Normalize.cmvn() in place, every line filled to the capacity: bit for bit the models composed, the empty row included"""
    from lewton_amd.rows import LogCompress, Normalize, Spectrogram, mel_filterbank
    mel = mel_filterbank(16000, 400, 80, scale="slaney", norm="slaney")
    sp, lc, nm = Spectrogram(mel=mel, pad_mode="reflect"), LogCompress("ln", 1e-10, float("inf"), 0.0, 1.0), Normalize.cmvn()
    try:
        lengths = [4000, 1601, 0]
        x = S._source(lengths, 1, 4000, 77)
        fcap = 29
        feats = S._filled((3, 1, 80, fcap))
        out, frames = sp.run(S._device(x, False), lengths, out=feats)
        assert frames.tolist() == [26, 11, 0]
        lc.run(out, frames)
        res, stats = nm.run(out, frames, fill_to=[fcap, 20, fcap], want_stats=True)
        torch.cuda.synchronize()
        assert res is feats
        lin = FC._expected_reflect(sp, mel, x, lengths, 3, fcap)
        logs, _ = FM.rows(lin, frames.tolist(), None, lin, FM.LN, FM.ROW, 1e-10, float("inf"), 0.0, 1.0)
        want, ws = M.rows(logs, frames.tolist(), [fcap, 20, fcap], logs, 1, M.STD, M.LINE, 1e-20)
        M.same_bits(feats.cpu().numpy(), want, M.SENT)
        M.same_bits(stats.cpu().numpy(), ws)
        assert not want[2].any() and (want[1, 0, :, 20:].view(np.uint32) == M.SENT).all()
        z = want[0, 0, :, :26].astype(F64)
        assert np.abs(z.mean(axis=1)).max() < 1e-6 and np.abs(z.std(axis=1) - 1.0).max() < 1e-6
    finally:
        sp.close()
        lc.close()
        nm.close()
