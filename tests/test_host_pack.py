"""Frame-major model input (lw_pack_*, lw_pack_rows, k_pack) in the CPU suite: tests/san/pack_host.cpp links lw_pack.cpp against the
HIP stand-ins (tests/san/hip_standins.inc) under ASan / UBSan and compiles the kernel source itself, lw_kernels_pack.hip, for the
host, where its stand-in launcher runs it workgroup by workgroup and phase by phase over exact-size buffers.

The model is the rule of include/lewton_amd.h ("frame-major model input") in numpy (tests/pack_model.py).  What the kernel makes of
real device memory, LDS and the barriers is checked on the GPU (tests/test_gpu_rows_pack.py)."""
import itertools
import os

import numpy as np
import pytest

import pack_model as M
import host_harness as H
from common import ROOT
from host_harness import CAPACITY, CS, DEVICE, NULL_ARG, OK, UNSUPPORTED

SRC = [os.path.join(ROOT, "tests", "san", "pack_host.cpp"), os.path.join(CS, "lw_pack.cpp")]
F32 = np.float32
DTYPES = ["f32", "bf16", "f16"]
EDGES = [M.REPLICATE, M.VALID]


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return H.build(tmp_path_factory, "pack_host", SRC)


_run = H.run


# ---- refusals, and what is queued

# (F, left, right, stride, edge, dtype, pad)
CREATE = [((0, 0, 0, 1, 0, 0, 0), UNSUPPORTED), ((65536, 0, 0, 1, 0, 0, 0), UNSUPPORTED), ((7, 17, 0, 1, 0, 0, 0), UNSUPPORTED),
          ((7, 0, 17, 1, 0, 0, 0), UNSUPPORTED), ((7, 0, 0, 0, 0, 0, 0), UNSUPPORTED), ((7, 0, 0, 17, 0, 0, 0), UNSUPPORTED),
          ((7, 0, 0, 1, 2, 0, 0), UNSUPPORTED), ((7, 0, 0, 1, -1, 0, 0), UNSUPPORTED), ((7, 0, 0, 1, 0, 3, 0), UNSUPPORTED),
          ((7, 0, 0, 1, 0, -1, 0), UNSUPPORTED), ((7, 0, 0, 1, 0, 1, "nan"), UNSUPPORTED), ((7, 0, 0, 1, 0, 0, 0), OK),
          ((65535, 16, 16, 16, 1, 2, -1.5), OK), ((1, 16, 16, 1, 0, 1, "inf"), OK), ((80, 3, 3, 6, 0, 1, 0), OK)]


def test_create_refusals(harness):
    for args, code in CREATE:
        assert _run(harness, "create", *args) == ["RC %d" % code], args
    ok = (80, 3, 3, 6, 0, 1, 0)
    for device, code in ((0, OK), (1, DEVICE), (-1, DEVICE), (1 << 20, DEVICE)):              # the stand-ins have one device
        assert _run(harness, "create", *ok, device) == ["RC %d" % code], device
    assert _run(harness, "create", 7, 0, 0, 0, 0, 0, 0, 1) == ["RC %d" % UNSUPPORTED]          # parameters are judged first


ROW_REFUSALS = [("null_pk", NULL_ARG), ("null_n", NULL_ARG), ("null_src", NULL_ARG), ("null_dst", NULL_ARG),
                ("null_dst_fill_only", NULL_ARG), ("n_over", CAPACITY), ("out_over", CAPACITY), ("fill_over", CAPACITY), ("ch0", CAPACITY),
                ("ch256", CAPACITY), ("src_too_large", CAPACITY), ("dst_too_large", CAPACITY), ("too_many_tiles", CAPACITY)]


@pytest.mark.parametrize("case,code", ROW_REFUSALS)
def test_refusals_queue_nothing(harness, case, code):
    assert _run(harness, "refuse", case) == ["RC %d" % code, "LAUNCHES 0", "LAST -1"]


def test_accepted_calls_and_their_launches(harness):
    """one launch per call; none without rows, with nothing to write (all rows empty, or VALID rows shorter than the window, which
    need no source either); one for a fill alone; 2^24 - 1 tiles is the most a launch is given"""
    for case, n in (("ok", 1), ("ok_no_rows", 0), ("ok_nothing", 0), ("ok_valid_too_short", 0), ("ok_fill_only", 1), ("ok_most_tiles", 1)):
        assert _run(harness, "refuse", case) == ["RC 0", "LAUNCHES %d" % n, "LAST %d" % n], case


def test_two_calls_back_to_back_each_reach_their_own_records(harness):
    """the second call's records do not replace the first's, which its kernel reads later; the caller's arrays are free at once"""
    out = _run(harness, "two")
    assert out == ["RC 0 LAST 1", "RC 0 LAST 1", "ROWS 300/50/60 0/0/3 4/1/1", "ROWS 1/1/1 257/43/43 13/3/3", "LAUNCHES 2"]


def test_lw_pack_frames_is_the_formula(harness):
    for left, right, stride in itertools.product((0, 1, 3, 16), (0, 1, 3, 16), (1, 2, 6, 16)):
        W = left + right + 1
        for e, edge in enumerate(EDGES):
            got = [int(v) for v in _run(harness, "frames", left, right, stride, e)[0].split()[1:]]
            want = [(-(-T // stride)) if edge == M.REPLICATE else (0 if T < W else (T - W) // stride + 1) for T in range(201)]
            assert got == want, (left, right, stride, edge)
            assert want == [M.out_frames(T, left, right, stride, edge) for T in range(201)]


# ---- the kernel source on the host

def _kernel(harness, tmp_path, x, n, fill_to, out_cap, left, right, stride, edge, dtype, shift=None, scale=None, pad=0.0, mask=True, offs=(0, 0)):
    R, C, F, cap = x.shape
    D = (left + right + 1) * F
    src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(src, "wb") as f:
        f.write(np.asarray(n, np.uint64).tobytes())
        f.write(np.asarray(fill_to if fill_to is not None else [0] * R, np.uint64).tobytes())
        for v in (shift, scale):
            f.write(np.ascontiguousarray(v if v is not None else np.zeros(D), F32).tobytes())
        f.write(np.array([pad], F32).tobytes())
        f.write(np.ascontiguousarray(x, F32).tobytes())
    out = _run(harness, "run", F, left, right, stride, EDGES.index(edge), DTYPES.index(dtype), C, R, cap, out_cap, int(fill_to is not None),
               int(shift is not None), int(scale is not None), int(mask), offs[0], offs[1], src, dst)
    assert out[0] == "RC 0" and out[2] == "TILE %d" % M.plan(F, left + right + 1, stride)[0], out
    raw = np.fromfile(dst, np.uint8)
    nd = R * C * out_cap * D * (4 if dtype == "f32" else 2)
    got = raw[:nd].view(M.OUT_DTYPE[dtype]).reshape(R, C, out_cap, D)
    return got, raw[nd:].reshape(R, out_cap), int(out[1].split()[1]), int(out[3].split()[1])


def _check(harness, tmp_path, x, n, fill_to, out_cap, left, right, stride, edge, dtype, shift=None, scale=None, pad=0.0, mask=True, offs=(0, 0)):
    got, gmask, launches, vec = _kernel(harness, tmp_path, x, n, fill_to, out_cap, left, right, stride, edge, dtype, shift, scale, pad, mask, offs)
    R, C, F, _ = x.shape
    D = (left + right + 1) * F
    want, wmask, t_out = M.rows(x, n, fill_to, np.full((R, C, out_cap, D), M.sentinel(dtype), M.OUT_DTYPE[dtype]),
                                np.full((R, out_cap), M.SENT_MASK, np.uint8) if mask else None, left, right, stride, edge, dtype, shift, scale, pad)
    M.same_bits(got, want, dtype, M.sentinel(dtype))
    assert np.array_equal(gmask, wmask if mask else np.full((R, out_cap), M.SENT_MASK, np.uint8))
    assert launches == int(max(max(t_out), max(fill_to) if fill_to is not None else 0) > 0)
    return want, vec


FILLS = {"none": lambda t, cap: None, "t_out": lambda t, cap: list(t), "capacity": lambda t, cap: [cap] * len(t),
         "below": lambda t, cap: [max(0, v - 2) for v in t], "mixed": lambda t, cap: [min(cap, (v * 7 + 3) % (cap + 1)) for v in t]}
CONTEXTS = [(0, 0, 1), (3, 3, 6), (5, 5, 1), (0, 2, 3), (0, 0, 4), (16, 16, 16), (1, 0, 1), (0, 16, 1)]
LINES = [1, 7, 31, 32, 33, 80]


@pytest.mark.parametrize("ctx", CONTEXTS)
def test_kernel_on_the_host_is_the_model_on_the_base_shape(harness, tmp_path, ctx):
    """[6][2][F][1031] with n_frames out of 0, 1, 2, W - 1, W, W + 1, 255, 256, 257, 1031 (six per call, in rotation), F = 1, 7, 31, 32,
    33 and 80, the three dtypes: every element of a sentinel-filled exact-size destination and mask.  The product with both edges,
    every kind of fill_to, shift / scale / mask given or not and every residue of the buffers against 16 bytes is pruned: each
    run takes the next value of every one of them, the periods coprime, so every value meets every context, F and dtype class."""
    left, right, stride = ctx
    W = left + right + 1
    pool = [0, 1, 2, W - 1, W, W + 1, 255, 256, 257, 1031]
    vecs = set()
    i = CONTEXTS.index(ctx)
    for F, dtype in itertools.product(LINES, DTYPES):
        i += 1
        n = [pool[(i + 3 * r) % len(pool)] for r in range(5)] + [1031]
        edge = EDGES[i % 2]
        t_out = [M.out_frames(T, left, right, stride, edge) for T in n]
        out_cap = max(t_out) + 3
        fill = FILLS[sorted(FILLS)[i % 5]](t_out, out_cap)
        es = 4 if dtype == "f32" else 2
        offs = (4 * (i % 4), 0 if i % 3 == 0 else es * (i % (16 // es)))
        D = W * F
        x = M.source(n, 2, F, 1031, 1000 * i + F)
        _, vec = _check(harness, tmp_path, x, n, fill, out_cap, left, right, stride, edge, dtype,
                        shift=M.vector(D, i) if i % 7 in (1, 2, 4) else None, scale=M.vector(D, i + 1, True) if i % 7 in (2, 3, 4, 5) else None,
                        pad=[0.0, -1.5, 1e-7][i % 3], mask=bool(i % 4), offs=offs)
        assert vec == int(offs[1] % 16 == 0 and F % (16 // es) == 0)
        vecs.add(vec)
    assert vecs == {0, 1}                                                    # the 16-byte stores and the element stores both ran


def test_special_values_on_the_host(harness, tmp_path):
    """+-0, subnormals, +-inf, NaNs, the values that round to infinity, the f16 overflow boundary, ties: through the copy, through
    shift and scale, and as pad; f32 without shift and scale keeps every NaN's payload"""
    n = [300, 7]
    x = M.source(n, 1, 8, 301, 31, special=True)
    for dtype in DTYPES:
        for pad in M.SPECIALS[[1, 11, 14, 18, 5]]:
            want, _ = _check(harness, tmp_path, x, n, [60, 60], 60, 3, 3, 6, M.REPLICATE, dtype, pad=float(pad))
        _check(harness, tmp_path, x, n, None, 300, 0, 0, 1, M.REPLICATE, dtype, shift=M.vector(8, 1), scale=M.vector(8, 2, True))
        _check(harness, tmp_path, x, n, None, 300, 0, 0, 1, M.REPLICATE, dtype, scale=np.full(8, 1.0, F32), offs=(4, 8))
    got, _, _, _ = _kernel(harness, tmp_path, x, n, None, 300, 0, 0, 1, M.REPLICATE, "f32")
    assert np.array_equal(got[0, 0, :300], x[0, 0, :, :300].T.view(np.uint32))                 # a bit copy, payloads included
    assert np.isnan(x[0, 0, :, :300]).any()


def test_rows_do_not_leak(harness, tmp_path):
    """rows of different lengths and an empty row between them give the bits each gives alone"""
    n = [300, 0, 1000, 17]
    x = M.source(n, 2, 7, 1000, 41)
    fill = [170, 5, 0, 20]
    together, _ = _check(harness, tmp_path, x, n, fill, 170, 3, 3, 6, M.REPLICATE, "bf16")
    assert (together[1, :, :5] == 0).all() and (together[1, :, 5:] == M.SENT16).all()
    for r in range(4):
        alone, _ = _check(harness, tmp_path, x[r:r + 1], n[r:r + 1], None, 170, 3, 3, 6, M.REPLICATE, "bf16")
        k = M.out_frames(n[r], 3, 3, 6, M.REPLICATE)
        assert np.array_equal(alone[0, :, :k], together[r, :, :k]) and (alone[0, :, k:] == M.SENT16).all()


# ---- the conversions

def _patterns():
    mant = [0, 1, 0x7FFF, 0x8000, 0x8001, 0xFFFF, 0x10000, 0x17FFF, 0x18000, 0x18001, 0x7F7FFF, 0x7F8000, 0x7FFFFF, 0xFFF, 0x1000, 0x1001,
            0x1FFF, 0x2000, 0x2FFF, 0x3000, 0x3001]
    mant = np.concatenate([np.array(mant, np.uint32), np.random.default_rng(9).integers(0, 1 << 23, 2000).astype(np.uint32)])
    exp = np.arange(256, dtype=np.uint32)[:, None] << 23
    half = (exp | mant[None, :]).ravel()
    return np.concatenate([half, half | np.uint32(0x80000000), np.array(M.SPECIAL_BITS, np.uint32)])


@pytest.mark.parametrize("dtype", DTYPES)
def test_lw_pack_convert_is_the_model_and_torchs_cpu_conversion(harness, tmp_path, dtype):
    """all 256 exponents x both signs x boundary mantissas and the f16 ties x 2000 random mantissas: lw_pack_convert == the model ==
    torch's CPU .to(); NaNs compared as NaN"""
    import torch
    u = _patterns()
    src, dst = str(tmp_path / "u.bin"), str(tmp_path / "c.bin")
    u.tofile(src)
    _run(harness, "convert", DTYPES.index(dtype), src, dst)
    got = np.fromfile(dst, np.uint32)
    want = M.convert(u.view(F32), dtype)
    assert dtype == "f32" or (got >> 16 == 0).all()
    M.same_bits(got.astype(M.OUT_DTYPE[dtype]), want, dtype)
    if dtype != "f32":
        t = torch.from_numpy(u.view(F32).copy()).to(torch.bfloat16 if dtype == "bf16" else torch.float16).view(torch.int16).numpy().view(np.uint16)
        M.same_bits(t, want, dtype)
        assert M.is_nan_bits(want, dtype).sum() == M.is_nan_bits(u, "f32").sum()               # a NaN stays a NaN, nothing else becomes one
        naive = ((u.astype(np.uint64) + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)     # the formula without the NaN case first
        if dtype == "bf16":
            assert (M.is_nan_bits(u, "f32") & ~M.is_nan_bits(naive, "bf16")).any()


# ---- FunASR's LFR

def _apply_lfr(inputs, m, n):
    """FunASR's apply_lfr (funasr/frontends/wav_frontend.py), restated in numpy: [T][F] -> [ceil(T / n)][m * F]"""
    T = inputs.shape[0]
    T_lfr = int(np.ceil(T / n))
    left_padding = np.tile(inputs[0], ((m - 1) // 2, 1))
    inputs = np.vstack((left_padding, inputs))
    T = T + (m - 1) // 2
    out = []
    for i in range(T_lfr):
        if m <= T - i * n:
            out.append(inputs[i * n:i * n + m].reshape(1, -1))
        else:
            num_padding = m - (T - i * n)
            frame = inputs[i * n:].reshape(-1)
            for _ in range(num_padding):
                frame = np.hstack((frame, inputs[-1]))
            out.append(frame.reshape(1, -1))
    return np.vstack(out)


@pytest.mark.parametrize("m,n", [(7, 6), (5, 3), (1, 4), (4, 2)])
def test_replicate_is_funasrs_lfr(m, n):
    left = (m - 1) // 2
    right = m - 1 - left
    for T in range(1, 60):
        x = np.random.default_rng(T).standard_normal((5, T)).astype(F32)
        got = M.frames_of(x, T, left, right, n, M.REPLICATE, None, None, "f32")
        assert np.array_equal(got, _apply_lfr(x.T.copy(), m, n).astype(F32).view(np.uint32)), (m, n, T)


# ---- the LDS banks

def test_tile_plan_is_the_headers(harness):
    for F, (left, right, stride) in itertools.product((1, 31, 32, 80), itertools.product((0, 3, 16), (0, 3, 16), range(1, 17))):
        tile, pitch, lines = M.plan(F, left + right + 1, stride)
        assert _run(harness, "plan", F, left, right, stride) == ["TILE %d PITCH %d LINES %d LDS %d" % (tile, pitch, lines, 4 * lines * pitch)]
        assert (tile - 1) * stride + left + right + 1 <= pitch <= 289 and pitch % 32 == 1 and 4 * lines * pitch <= 160 * 1024


def test_both_sides_of_the_lds_image_are_free_of_bank_conflicts():
    """every tile plan (every stride, the narrowest and the widest window and LFR's), every unit width (1, 4, 8 elements) and line
    group sizes either side of each: no store shares a bank among its 32 lanes (ds_write_b32, 32 banks), no load either
    (ds_read_b32, 32 banks); a last tile of a row (fewer frames) included"""
    plans = set()
    for stride, W in itertools.product(range(1, 17), (1, 2, 7, 11, 33)):
        tile, pitch, _ = M.plan(32, W, stride)
        plans.add(tile)
        for E in (1, 4, 8):
            for G in sorted({E, 8, 16, 24, 32} | ({1, 7, 31} if E == 1 else set())):
                for nu in (tile, 5):
                    assert M.lds_conflicts(tile, pitch, W, stride, E, G, nu) == (0, 0), (stride, W, E, G, nu)
    assert plans == {256, 128, 64, 32, 16}
    assert M.lds_conflicts(32, 192, 7, 6, 4, 32)[1] > 0                     # the simulation does see a conflict: an even pitch


# ---- Python

def test_python_parameter_errors_need_no_gpu():
    from lewton_amd.rows import FramePack
    for kw in [dict(n_in=0), dict(n_in=65536), dict(n_in=7.0), dict(n_in=True), dict(n_in=7, left=17), dict(n_in=7, left=-1), dict(n_in=7, right=17),
               dict(n_in=7, right=1.5), dict(n_in=7, stride=0), dict(n_in=7, stride=17), dict(n_in=7, edge="zero"), dict(n_in=7, dtype="fp8"),
               dict(n_in=7, dtype=np.float32), dict(n_in=7, pad=float("nan")), dict(n_in=7, pad="x"), dict(n_in=7, shift=np.zeros(8)),
               dict(n_in=7, left=1, scale=np.zeros(7)), dict(n_in=7, shift="x")]:
        with pytest.raises(ValueError):
            FramePack(**kw)
    for make in (lambda: FramePack.lfr(80, 0, 6), lambda: FramePack.lfr(80, 40, 6), lambda: FramePack.stack(80, 0, 3), lambda: FramePack.stack(80, 4, 0),
                 lambda: FramePack.subsample(80, 0), lambda: FramePack.splice(80, 17, 0), lambda: FramePack.transpose(0)):
        with pytest.raises(ValueError):
            make()
