"""The energy VAD (lw_vad_*, lw_vad_rows, k_vad, k_vad_sum, k_vad_fold, k_vad_decide) in the CPU suite: tests/san/vad_host.cpp links
lw_vad.cpp against the HIP stand-ins (tests/san/hip_standins.inc) under ASan / UBSan and compiles the kernel source itself,
lw_kernels_vad.hip, for the host, where its stand-in launchers run it workgroup by workgroup and phase by phase over exact-size
buffers.

The model is the rule of include/lewton_amd.h ("energy voice-activity decisions of feature rows") in numpy (tests/vad_model.py).
What the kernels make of real device memory, LDS, the shuffles, the ballots and the barriers is checked on the GPU
(tests/test_gpu_rows_vad.py)."""
import os

import numpy as np
import pytest

import norm_model as NM
import vad_model as M
import host_harness as H
from common import ROOT
from host_harness import CAPACITY, CS, DEVICE, NULL_ARG, OK, UNSUPPORTED

SRC = [os.path.join(ROOT, "tests", "san", "vad_host.cpp"), os.path.join(CS, "lw_vad.cpp")]
F32, F64 = np.float32, np.float64
N, CAP = [1100, 0, 257, 600], 1103                                      # two seams of the default tile's quarter, one of the default
AUTO, FUSED, SPLIT = 0, 1, 2


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return H.build(tmp_path_factory, "vad_host", SRC)


_run = H.run


def _bits(v):
    with np.errstate(over="ignore"):
        return int(np.array(v, F32).view(np.uint32))


# ---- refusals, and what is queued

def test_create_and_the_hooks(harness):
    ok = (5.0, 0.5, 0, 0.6, 0, 0)
    for device, code in ((0, OK), (1, DEVICE), (-1, DEVICE), (1 << 20, DEVICE)):              # the stand-ins have one device
        thr, scale, ctx, prop, line, res = ok
        assert _run(harness, "create", device, _bits(thr), _bits(scale), ctx, _bits(prop), line, res) == ["RC %d" % code], device
    cases = [((np.inf, 0.5, 0, 0.6, 0, 0), UNSUPPORTED), ((np.nan, 0.5, 0, 0.6, 0, 0), UNSUPPORTED), ((-np.inf, 0.5, 0, 0.6, 0, 0), UNSUPPORTED),
             ((5.0, np.nan, 0, 0.6, 0, 0), UNSUPPORTED), ((5.0, -0.5, 0, 0.6, 0, 0), UNSUPPORTED), ((5.0, np.inf, 0, 0.6, 0, 0), UNSUPPORTED),
             ((5.0, 0.5, 257, 0.6, 0, 0), UNSUPPORTED), ((5.0, 0.5, 0, 0.0, 0, 0), UNSUPPORTED), ((5.0, 0.5, 0, 1.0, 0, 0), UNSUPPORTED),
             ((5.0, 0.5, 0, -0.1, 0, 0), UNSUPPORTED), ((5.0, 0.5, 0, np.nan, 0, 0), UNSUPPORTED), ((5.0, 0.5, 0, 0.6, 0, 1), UNSUPPORTED),
             ((-3.0, 0.0, 256, 0.999, 65534, 0), OK), ((5.0, -0.0, 0, 1e-30, 0, 0), OK)]
    for (thr, scale, ctx, prop, line, res), code in cases:
        assert _run(harness, "create", 0, _bits(thr), _bits(scale), ctx, _bits(prop), line, res) == ["RC %d" % code], (thr, scale, ctx, prop, line, res)
    for tile, code in ((256, OK), (512, OK), (2048, OK), (1024, OK), (0, UNSUPPORTED), (128, UNSUPPORTED), (300, UNSUPPORTED), (2304, UNSUPPORTED)):
        assert _run(harness, "tile", tile) == ["RC %d TILE %d" % (code, tile if code == OK else 1024)]
    for route, code in ((AUTO, OK), (FUSED, OK), (SPLIT, OK), (3, UNSUPPORTED), (-1, UNSUPPORTED)):
        assert _run(harness, "route", route) == ["RC %d" % code]


ROW_REFUSALS = [("null_v", NULL_ARG), ("null_n", NULL_ARG), ("null_src", NULL_ARG), ("null_src_scale0", NULL_ARG), ("null_mask", NULL_ARG),
                ("null_mask_fill_only", NULL_ARG), ("n_over", CAPACITY), ("fill_over", CAPACITY), ("ch0", CAPACITY), ("ch256", CAPACITY),
                ("f0", CAPACITY), ("f65536", CAPACITY), ("line_over", CAPACITY), ("too_large", CAPACITY), ("too_many_tiles", CAPACITY),
                ("fused_too_long", UNSUPPORTED)]
UNTOUCHED = "THR" + " 77" * 6


@pytest.mark.parametrize("case,code", ROW_REFUSALS)
def test_refusals_queue_nothing(harness, case, code):
    assert _run(harness, "refuse", case) == ["RC %d" % code, "LAUNCHES 0", "LAST -1", UNTOUCHED]


def test_accepted_calls_and_their_launches(harness):
    """one launch per 65535 rows in the fused form and without a mean (whatever the route), three in the split form, which a row of
    16385 frames takes by itself; where no row has a frame nothing is summed: the decide launch alone; with no byte of the mask to
    write one workgroup fills the thresholds with energy_threshold, and without d_thr or rows nothing is queued"""
    for case, n in (("ok", 1), ("ok_split", 3), ("ok_scale0", 1), ("ok_scale0_split", 1), ("ok_fused_longest", 1), ("ok_auto_long", 3),
                    ("ok_no_rows", 0), ("ok_nothing", 1), ("ok_nothing_no_thr", 0), ("ok_fill_only", 1), ("ok_most_tiles", 1), ("ok_rows65536", 2),
                    ("ok_rows65536_split", 6)):
        out = _run(harness, "refuse", case)
        assert out[:3] == ["RC 0", "LAUNCHES %d" % n, "LAST %d" % n], case
        assert out[3] == ("THR" + " 5" * 6 if case == "ok_nothing" else UNTOUCHED), case


def test_two_calls_back_to_back_each_reach_their_own_records(harness):
    """the second call's records do not replace the first's, which its kernels read later; the caller's arrays are free at once"""
    assert _run(harness, "two") == ["RC 0 LAST 1", "RC 0 LAST 3", "ROWS 3000/3000 0/3 4/4", "ROWS 1/1 257/257 13/13", "LAUNCHES 4"]


# ---- the kernel source on the host

def _kernel(harness, tmp_path, x, n, fill_to, cfg, tile, route, line=0, want_thr=True, offs=(0, 0)):
    R, C, F, cap = x.shape
    src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(src, "wb") as f:
        f.write(np.asarray(n, np.uint64).tobytes())
        f.write(np.asarray(fill_to if fill_to is not None else [0] * R, np.uint64).tobytes())
        f.write(np.ascontiguousarray(x, F32).tobytes())
    out = _run(harness, "run", tile, route, C, F, line, R, cap, int(fill_to is not None), int(want_thr), offs[0], offs[1], _bits(cfg[0]), _bits(cfg[1]),
               cfg[2], _bits(cfg[3]), src, dst)
    assert out[0] == "RC 0" and out[2] == "TILE %d" % tile, out
    raw = np.fromfile(dst, np.uint8)
    return raw[:R * C * cap].reshape(R, C, cap), raw[R * C * cap:].view(F32).reshape(R, C), int(out[1].split()[1])


def _check(harness, tmp_path, x, n, fill_to, cfg, tile, route, line=0, want_thr=True, offs=(0, 0)):
    got, gthr, launches = _kernel(harness, tmp_path, x, n, fill_to, cfg, tile, route, line, want_thr, offs)
    R, C, F, cap = x.shape
    want, thr = M.rows(x, n, fill_to, np.full((R, C, cap), M.SENT_MASK, np.uint8), cfg, line)
    M.same_mask(got, want)
    if want_thr:
        M.same_thr(gthr, thr)
    else:
        assert (gthr.view(np.uint32) == 0xEEEEEEEE).all()
    span = max(max(n), max(fill_to) if fill_to is not None else 0)
    sums = cfg[1] != 0 and max(n) > 0
    assert launches == (int(want_thr) if span == 0 else 3 if sums and route == SPLIT else 1)
    return want, thr


FILLS = [lambda n, cap: None, lambda n, cap: [cap] * len(n), lambda n, cap: [max(0, v - 2) for v in n],
         lambda n, cap: [min(cap, (v * 7 + 3) % (cap + 1)) for v in n]]


@pytest.mark.parametrize("F", [1, 3, 81])
def test_kernel_on_the_host_is_the_model_at_every_shape_of_the_gpu_suite(harness, tmp_path, F):
    """[4][2][F][1103] with lengths 1100, 0, 257 and 600, the energy in line 0 and in line F - 1, a context of 0, 2 and 256 frames,
    tiles of 256 (five in the longest row) and 1024 (two), both routes, the four kinds of fill_to, whether the thresholds are
    wanted, and the buffers at every residue against 4 bytes for the mask and 16 for the source, in rotation"""
    i = 0
    for line in sorted({0, F - 1}):
        x = M.source(N, 2, F, CAP, 50 + F + line, line_i=line, others_nan=bool(line))
        for ctx, prop in ((0, 0.6), (2, 0.12), (256, 0.6), (2, 0.6)):
            for tile in (256, 1024):
                for route in (FUSED, SPLIT):
                    i += 1
                    _check(harness, tmp_path, x, N, FILLS[i % 4](N, CAP), (12.0, 0.0, ctx, prop) if i % 5 == 0 else (6.0, 0.5, ctx, prop), tile, route, line=line,
                           want_thr=bool(i % 3), offs=(4 * (i % 4), (i // 2) % 4))


def test_every_residue_of_the_mask_against_four_bytes_and_every_kind_of_fill(harness, tmp_path):
    """the dword stores and the bytes at the ragged head and tail of every tile's span: all four residues of the mask's address,
    with all four kinds of fill_to each, at a capacity that moves every row and channel to another residue"""
    x = M.source(N, 2, 1, CAP, 77)
    for off in range(4):
        for k in range(4):
            _check(harness, tmp_path, x, N, FILLS[k](N, CAP), M.SRE, 256, FUSED if (off + k) % 2 else SPLIT, offs=(4 * ((off + k) % 4), off))


def test_rows_do_not_leak_and_empty_calls(harness, tmp_path):
    """every row alone gives the bits it gives among the others; a call whose rows are all empty writes the thresholds and nothing
    else; rows that only fill need no source"""
    x = M.source(N, 2, 3, CAP, 41, line_i=1)
    cfg = (5.5, 0.5, 2, 0.6)
    together, thr = _check(harness, tmp_path, x, N, [CAP, 5, 0, 700], cfg, 256, FUSED, line=1)
    assert (together[1, :, :5] == 0).all() and (together[1, :, 5:] == M.SENT_MASK).all() and (thr[1] == F32(5.5)).all()
    assert 0.1 < together[0, :, :1100].mean() < 0.9
    for r in range(4):
        alone, ta = _check(harness, tmp_path, x[r:r + 1], N[r:r + 1], None, cfg, 1024, SPLIT, line=1)
        assert np.array_equal(alone[0, :, :N[r]], together[r, :, :N[r]])
        M.same_thr(ta[0], thr[r])
    _check(harness, tmp_path, x, [0] * 4, None, cfg, 1024, AUTO, line=1)
    _check(harness, tmp_path, x, [0] * 4, None, cfg, 1024, AUTO, line=1, want_thr=False)
    _check(harness, tmp_path, x, [0] * 4, [3, 0, CAP, 1], cfg, 1024, SPLIT, line=1)


def test_lengths_where_the_tree_changes_shape(harness, tmp_path):
    """1, 255, 256 and 257 frames in one call, 16384 (64 chunks: the fused form's longest row, ONE tree) and 16385 (the split form
    by itself, two levels) alone; fused == split == the model"""
    n = [1, 255, 256, 257, 2]
    x = M.source(n, 1, 2, 259, 5)
    for route in (FUSED, SPLIT):
        _check(harness, tmp_path, x, n, [259, 0, 258, 0, 1], M.SRE, 256, route)
    x = M.source([16384], 1, 1, 16385, 6)
    a, ta = _check(harness, tmp_path, x, [16384], None, M.SRE, 2048, FUSED)
    b, tb = _check(harness, tmp_path, x, [16384], None, M.SRE, 768, SPLIT)
    assert np.array_equal(a, b) and ta.tobytes() == tb.tobytes()
    x = M.source([16385], 1, 1, 16385, 7)
    got, _, launches = _kernel(harness, tmp_path, x, [16385], None, M.SRE, 1024, AUTO)
    assert launches == 3
    M.same_mask(got, _check(harness, tmp_path, x, [16385], None, M.SRE, 1024, SPLIT)[0])


def test_special_values(harness, tmp_path):
    """NaN, +-inf and +-0 in the energy line, one kind more per row: a NaN or an infinity in a line with a mean reaches its threshold,
    without a mean it decides its own frame alone"""
    n = [300] * 6
    x = M.source(n, 1, 2, 301, 31, special=True)
    for cfg in ((5.0, 0.5, 2, 0.6), (5.0, 0.0, 1, 0.12), (0.0, 0.0, 0, 0.6)):
        for route in (FUSED, SPLIT):
            want, thr = _check(harness, tmp_path, x, n, None, cfg, 256, route)
        if cfg[1]:
            assert np.isnan(thr[5]).all() and not want[5, :, :300].any() and np.isfinite(thr[:3]).all()
        else:
            assert want[5, :, :300].any()


def test_a_tile_far_up_a_row_past_frame_2_to_the_32(harness, tmp_path):
    """one row of 2^32 + 4096 + 5000 frames in tiles of 2048 of which only the last 5000 exist: the chunks in front of them count as
    256 frames of 12.0 (16.8 million list entries, four fold levels), the tiles from the second existing one on are run, so the
    offsets of the energy line, of the halo and of the mask, the chunk numbers and (float)T are all beyond 32 bits"""
    base, keep, tile = (1 << 32) + 4096, 5000, 2048
    cfg = (5.5, 0.5, 2, 0.6)
    e = M.source([keep], 1, 1, keep, 77)[0, 0, 0]
    src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    e.tofile(src)
    out = _run(harness, "far", tile, base, keep, _bits(cfg[0]), _bits(cfg[1]), cfg[2], _bits(cfg[3]), src, dst)
    assert out == ["RC 0", "LAUNCHES 3"], out
    raw = np.fromfile(dst, np.uint8)
    got, thr = raw[:keep], raw[keep:].view(F32)[0]
    a, b, pk = NM.chunk_triples(e[None], keep)
    lst = np.concatenate([np.full(base // 256, 3072.0, F64), a[0]])
    S = NM.fold(lst, lst, np.zeros(len(lst), np.uint32))[0]
    want_thr = M.threshold(S, base + keep, cfg[0], cfg[1])
    assert thr.tobytes() == want_thr.tobytes() and abs(float(thr) - 11.5) < 1e-3
    assert (got[:tile] == M.SENT_MASK).all()
    assert np.array_equal(got[tile:], M.decide(e, keep, want_thr, cfg[2], cfg[3])[tile:]) and 0.2 < got[tile:].mean() < 0.8


def test_threshold_and_voiced_on_the_host_are_the_model(harness, tmp_path):
    rng = np.random.default_rng(3)
    S = np.concatenate([rng.standard_normal(200) * 10.0 ** rng.uniform(-3, 12, 200), [0.0, -0.0, np.inf, -np.inf, np.nan, 1e300, 5e-324]])
    T = np.concatenate([rng.integers(1, 1 << 40, 200), [0, 1, (1 << 24) + 1, (1 << 32) + (1 << 20) + 5, (1 << 53) - 1, 3, 7]]).astype(np.uint64)
    pairs = np.array([(num, den) for den in range(1, 514) for num in range(den + 1)], np.uint64)
    src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    for thr0, scale, prop in ((5.5, 0.5, 0.6), (5.0, 0.0, 0.3), (-2.0, 3.25, 0.12)):
        with open(src, "wb") as f:
            f.write(np.uint64(len(S)).tobytes())
            f.write(np.rec.fromarrays([S, T]).tobytes())
            f.write(np.uint64(len(pairs)).tobytes())
            f.write(pairs.tobytes())
        _run(harness, "scalars", _bits(thr0), _bits(scale), _bits(prop), src, dst)
        raw = np.fromfile(dst, np.uint8)
        got_thr, got_v = raw[:4 * len(S)].view(F32), raw[4 * len(S):]
        M.same_thr(got_thr, np.array([M.threshold(s, int(t), thr0, scale) for s, t in zip(S, T)], F32))
        assert np.array_equal(got_v, np.array([M.voiced(int(num), int(den), prop) for num, den in pairs], np.uint8))


# ---- Python

def test_python_parameter_errors_need_no_gpu():
    from lewton_amd.rows import EnergyVad
    for kw in [dict(device=-1), dict(device=1.5), dict(device="0"), dict(device=True), dict(energy_threshold=float("inf")),
               dict(energy_threshold=float("nan")), dict(energy_threshold=1e39), dict(energy_threshold="5"), dict(energy_mean_scale=-0.5),
               dict(energy_mean_scale=float("nan")), dict(energy_mean_scale=float("inf")), dict(frames_context=257), dict(frames_context=-1),
               dict(frames_context=1.0), dict(proportion_threshold=0.0), dict(proportion_threshold=1.0), dict(proportion_threshold=1e-50),
               dict(proportion_threshold=float("nan")), dict(line=-1), dict(line=65535), dict(line=True)]:
        with pytest.raises(ValueError):
            EnergyVad(**kw)
