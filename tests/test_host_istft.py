"""Inverse spectral frames of rows (lw_istft_*, lw_istft_rows, k_istft) in the CPU suite: tests/san/istft_host.cpp links
lw_istft.cpp against the HIP stand-ins (tests/san/hip_standins.inc) under ASan / UBSan and compiles the kernel source itself,
lw_kernels_istft.hip, for the host (its route with per-lane fmaf chains), where its stand-in launcher runs it workgroup by
workgroup and lane by lane over exact-size buffers.

The model is the rule of include/lewton_amd.h ("inverse spectral frames of rows"), tests/istft_model.py: the tables in numpy
float64, the indices in Python integers, the chains with spec_model.fmaf.  What the kernel makes of real device memory, and whether
the matrix instruction gives the same bits, is checked on the GPU (tests/test_gpu_rows_istft.py)."""
import os

import numpy as np
import pytest

import istft_model as IM
import spec_model as M
import host_harness as H
from common import ROOT
from host_harness import CAPACITY, CS, NULL_ARG, UNSUPPORTED

SRC = [os.path.join(ROOT, "tests", "san", "istft_host.cpp"), os.path.join(CS, "lw_istft.cpp")]
WINDOWS = {"hann": 0, "rect": 1, "hann_sym": 4}
SENT = 0x7FC00ABC
# (n_fft, win_length, hop, window, center): the shapes of the GPU suite
SHAPES = [(16, 16, 4, "hann", 1), (25, 25, 7, "hann", 1), (32, 20, 5, "hann", 1), (64, 64, 64, "rect", 0), (32, 32, 2, "hann", 1),
          (16, 16, 4, "hann", 0), (512, 400, 160, "hann", 1), (2048, 2048, 512, "hann_sym", 1)]


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return H.build(tmp_path_factory, "istft_host", SRC)


_run = H.run


def _shape_args(shape):
    n_fft, win, hop, window, center = shape
    return [n_fft, win, hop, WINDOWS[window], center]


def _tables(harness, tmp_path, shape):
    g, w = str(tmp_path / "g.bin"), str(tmp_path / "w2.bin")
    out = _run(harness, "basis", *_shape_args(shape), g, w)
    B, o, ov, m = [int(v) for v in out[0].split()[1:]]
    return np.fromfile(g, np.float32).reshape(2 * B, shape[1]), np.fromfile(w, np.float64), (B, o, ov, m)


@pytest.mark.parametrize("shape", SHAPES)
def test_tables_are_the_formula_rounded_once(harness, tmp_path, shape):
    n_fft, win, hop, window, _ = shape
    G, w2, (B, o, ov, m) = _tables(harness, tmp_path, shape)
    assert (B, o, ov) == (n_fft // 2 + 1, (n_fft - win) // 2, -(-win // hop))
    assert 1 <= m and m + ov <= 32 and m * hop <= 7168 and (m + 1 + ov > 32 or (m + 1) * hop > 7168)
    want = IM.table(n_fft, win, window)
    # two double evaluations differ by a few 1e-16 relative; after the one rounding to f32 that is at most one f32 ulp
    tol = np.spacing(np.abs(want).astype(np.float32)).astype(np.float64) + 1e-18
    err = np.abs(G.astype(np.float64) - want)
    assert (err <= tol).all(), (float(err.max()), np.argwhere(err > tol)[:4].tolist())
    # the sine lines irfft ignores are +0.0 exactly, not sin(pi k) in double
    assert not G[B].view(np.uint32).any() and (n_fft % 2 or not G[B + n_fft // 2].view(np.uint32).any())
    assert np.count_nonzero(G[B + 1]) > 0.4 * win
    want2 = IM.window2(window, win)
    assert np.abs(w2 - want2).max() <= 4 * np.spacing(1.0)           # cos in two libraries, squared: a few ulp of 1
    if window == "rect":
        assert (w2 == 1).all() and (G[0] == np.float32(1.0 / n_fft)).all()


def test_natural_lengths_in_64_bits(harness):
    Ts = [0, 1, 2, 3, 31, 32, 33, (1 << 31) - 1, 1 << 32, (1 << 40) + 7]
    for shape in SHAPES:
        n_fft, win, hop, _, center = shape
        out = _run(harness, "lens", *_shape_args(shape), *Ts)
        assert [tuple(int(v) for v in ln.split()[1:]) for ln in out] == [(T, IM.geometry(n_fft, win, hop, center, T)[4]) for T in Ts]


def test_a_tile_far_up_a_row_keeps_its_offsets_in_64_bits(harness):
    """the tile's first owned sample, first frame, position relative to that frame, P and the destination offset, by the
    kernel's own lw_is_tile, against Python integers: past sample 2^32, frame 2^31 and element 2^33"""
    for (n_fft, win, hop, center, m), tile in [((512, 400, 160, 1, 29), (1 << 32) // (29 * 160) + 5), ((32, 20, 5, 1, 28), (1 << 35) // 140 + 3),
                                               ((2048, 2048, 512, 0, 14), 1 << 23), ((16, 16, 4, 1, 28), 0), ((32, 20, 5, 0, 3), 0)]:
        o, pad = (n_fft - win) // 2, (n_fft // 2 if center else 0)
        s0 = tile * m * hop
        T = (s0 + m * hop) // hop + 2                                      # frames beyond the tile's
        out_len, drow, cap = s0 + 10, 3, s0 + 17
        out = _run(harness, "tile", n_fft, win, hop, center, m, tile, T, out_len, drow, cap)
        lo = s0 - o - win + 1
        tf0 = 0 if lo <= 0 else -(-lo // hop)
        want = (s0, tf0, min(32, T - tf0), s0 - o - tf0 * hop, n_fft + (T - 1) * hop, drow * 2 * cap + cap)
        assert [int(v) for v in out[0].split()[1:]] == list(want)
        # every frame that touches the span is among the tile's 32
        last = (s0 + m * hop - 1 - o) // hop
        assert tf0 <= max(last, 0) < tf0 + 32


CREATE_REFUSALS = [(1, 1, 1, 0, 1, 0), (2049, 400, 160, 0, 1, 0), (400, 0, 160, 0, 1, 0), (400, 401, 160, 0, 1, 0), (400, 400, 0, 0, 1, 0),
                   (400, 400, 160, 6, 1, 0), (400, 400, 160, -1, 1, 0), (400, 400, 160, 0, 2, 0), (400, 400, 160, 0, 1, 1),
                   (400, 200, 201, 0, 1, 0),            # hop > win_length: gaps no frame covers
                   (400, 400, 23, 0, 1, 0), (32, 32, 1, 0, 1, 0), (64, 33, 2, 1, 0, 0)]          # ov = 18, 32, 17


def test_create_refusals_and_the_limits(harness):
    for args in CREATE_REFUSALS:
        assert _run(harness, "create", *args) == ["RC %d" % UNSUPPORTED], args
    for args in [(2, 1, 1, 0, 0, 0), (2048, 2048, 128, 1, 1, 0), (400, 400, 25, 0, 1, 0), (64, 32, 2, 4, 0, 0), (400, 200, 200, 0, 1, 0),
                 (2048, 2048, 2048, 5, 0, 0)]:
        assert _run(harness, "create", *args) == ["RC 0"], args


ROW_REFUSALS = [("null_is", NULL_ARG), ("null_frames", NULL_ARG), ("null_src", NULL_ARG), ("null_dst", NULL_ARG),
                ("i16", UNSUPPORTED), ("i16_interleaved", UNSUPPORTED), ("bad_fmt", UNSUPPORTED), ("ch0", CAPACITY), ("ch256", CAPACITY),
                ("frames_over", CAPACITY), ("len_over", CAPACITY), ("natural_over", CAPACITY), ("row_over", CAPACITY),
                ("row_over_identity", CAPACITY), ("row_twice", CAPACITY), ("row_twice_empty", CAPACITY), ("bytes_over", CAPACITY),
                ("bad_route", UNSUPPORTED), ("bad_m", UNSUPPORTED), ("bad_m0", UNSUPPORTED)]


@pytest.mark.parametrize("case,code", ROW_REFUSALS)
def test_refusals_launch_nothing_and_write_nothing(harness, case, code):
    assert _run(harness, "refuse", case) == ["RC %d" % code, "LAUNCHES 0", "WRITTEN 0"]


def test_exactly_full_is_accepted(harness):
    assert _run(harness, "refuse", "ok") == ["RC 0", "LAUNCHES 1", "WRITTEN %d" % (2 * (32 + 7 + 40))]
    assert _run(harness, "refuse", "ok_natural") == ["RC 0", "LAUNCHES 1", "WRITTEN %d" % (2 * (32 + 0 + 16))]


# ---- the kernel on the host against the bit model

def _source(rng, B, frames, ch, fcap):
    """float32 [rows][ch][2 B][fcap], NaN beyond each row's frames"""
    x = np.full((len(frames), ch, 2 * B, fcap), np.array(SENT, np.uint32).view(np.float32), np.float32)
    for r, T in enumerate(frames):
        x[r, :, :, :T] = rng.uniform(-1, 1, (ch, 2 * B, T)).astype(np.float32)
    return x


def _kernel_case(harness, tmp_path, shape, frames, ch, fmt, lens=None, rows=None, m=0, x=None, seed=1):
    n_fft, win, hop, window, center = shape
    G, w2, (B, _, _, m_obj) = _tables(harness, tmp_path, shape)
    fcap = (max(frames) + 1) | 1
    if x is None:
        x = _source(np.random.default_rng(seed), B, frames, ch, fcap)
    natural = [IM.geometry(n_fft, win, hop, center, T)[4] for T in frames]
    want_len = natural if lens is None else lens
    dcap = (max(want_len) + 2) | 1
    ndst = (max(rows) + 1 if rows else len(frames)) + 1
    src, dst = str(tmp_path / "x.bin"), str(tmp_path / "y.bin")
    x.tofile(src)
    csv = lambda v: "-" if v is None else ",".join(str(int(i)) for i in v)
    out = _run(harness, "run", *_shape_args(shape), m, 3 if fmt == "itl" else 2, ch, len(frames), fcap, ndst, dcap, src, dst, csv(frames), csv(rows),
               csv(lens))
    assert out[0] == "RC 0" and out[1] == "M %d" % (m or m_obj)
    got = np.fromfile(dst, np.float32).reshape((ndst, dcap, ch) if fmt == "itl" else (ndst, ch, dcap))
    want = np.full((ndst, ch, dcap), np.array(SENT, np.uint32).view(np.float32), np.float32)
    for r, T in enumerate(frames):
        for c in range(ch):
            want[rows[r] if rows else r, c, :want_len[r]] = IM.istft(G, w2, x[r, c, :, :T], n_fft, hop, center, want_len[r])
    M.same_bits(got.transpose(0, 2, 1) if fmt == "itl" else got, want)
    return got, want, (m or m_obj)


@pytest.mark.parametrize("shape", SHAPES[:7])
def test_kernel_on_the_host_is_bit_identical_to_the_model(harness, tmp_path, shape):
    """three rows whose frame counts cross a tile edge with and without a halo beyond either end of the row, two channels,
    both formats, lengths shorter than, equal to and longer than natural, a NaN-filled source beyond each frame count, a
    sentinel in the destination and a spare destination row; then the same rows with another tile size"""
    n_fft, win, hop, window, center = shape
    m = _tables(harness, tmp_path, shape)[2][3]
    nat = lambda T: IM.geometry(n_fft, win, hop, center, T)[4]
    for frames in ([0, 1, m - 1], [m, m + 1, 2 * m + 1]):
        _kernel_case(harness, tmp_path, shape, frames, 2, "planar")
        lens = [max(nat(frames[0]) - 3, 0), nat(frames[1]), nat(frames[2]) + 2 * hop + 5]
        _kernel_case(harness, tmp_path, shape, frames, 1, "itl", lens=lens, rows=[2, 0, 3], m=max(1, m // 3), seed=2)


def test_kernel_on_the_host_at_the_largest_table(harness, tmp_path):
    shape = SHAPES[7]
    m = _tables(harness, tmp_path, shape)[2][3]
    assert m == 14
    _kernel_case(harness, tmp_path, shape, [m + 1, 1], 1, "planar", m=5)


def test_where_the_envelope_vanishes_the_sample_is_plus_zero(harness, tmp_path):
    got, _, _ = _kernel_case(harness, tmp_path, (16, 16, 4, "hann", 0), [5], 1, "planar")
    assert got[0, 0, 0].view(np.uint32) == 0 and np.count_nonzero(got[0, 0, 1:32]) == 31
