"""Segments of a frame mask (lw_segment_*, lw_segment_rows, k_segment_count, k_segment) in the CPU suite: tests/san/segment_host.cpp
links lw_segment.cpp against the HIP stand-ins (tests/san/hip_standins.inc) under ASan / UBSan and compiles the kernel source
itself, lw_kernels_segment.hip, for the host, where its stand-in launchers run it workgroup by workgroup and phase by phase over
exact-size buffers.

The model is the rule of include/lewton_amd.h ("segments of a frame mask") in numpy (tests/segment_model.py).  Every comparison is
over every byte of sentinel-filled exact-size buffers; the mask holds non-zero sentinel bytes at and beyond each length.  What the
kernels make of real device memory, LDS, the ballots and the barriers is checked on the GPU (tests/test_gpu_rows_segment.py)."""
import os

import numpy as np
import pytest

import segment_model as M
import host_harness as H
from common import ROOT
from host_harness import CAPACITY, CS, DEVICE, NULL_ARG, OK, UNSUPPORTED

SRC = [os.path.join(ROOT, "tests", "san", "segment_host.cpp"), os.path.join(CS, "lw_segment.cpp")]
N, CAP = [1100, 0, 257, 600], 1103                                      # four seams of the smallest tile, one of the default
PARAMS = [(0, 0, 0, 0), (3, 7, 5, 4), (0, 40, 0, 0), (1024, 1024, 1024, 1024)]
U64 = np.uint64


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return H.build(tmp_path_factory, "segment_host", SRC)


_run = H.run


# ---- refusals, and what is queued

def test_create_and_the_hooks(harness):
    for device, code in ((0, OK), (1, DEVICE), (-1, DEVICE), (1 << 20, DEVICE)):              # the stand-ins have one device
        assert _run(harness, "create", device, 2, 8, 10, 5, 0) == ["RC %d" % code], device
    for p, code in (((0, 0, 0, 0, 0), OK), ((1024, 1024, 1024, 1024, 0), OK), ((1025, 0, 0, 0, 0), UNSUPPORTED), ((0, 1025, 0, 0, 0), UNSUPPORTED),
                    ((0, 0, 1025, 0, 0), UNSUPPORTED), ((0, 0, 0, 1025, 0), UNSUPPORTED), ((0, 0, 0, 1 << 31, 0), UNSUPPORTED), ((2, 8, 10, 5, 1), UNSUPPORTED)):
        assert _run(harness, "create", 0, *p) == ["RC %d" % code], p
    for tile, code in ((256, OK), (512, OK), (2048, OK), (1024, OK), (0, UNSUPPORTED), (128, UNSUPPORTED), (300, UNSUPPORTED), (2304, UNSUPPORTED)):
        assert _run(harness, "tile", tile) == ["RC %d TILE %d" % (code, tile if code == OK else 1024)]


ROW_REFUSALS = [("null_sg", NULL_ARG), ("null_n", NULL_ARG), ("null_mask", NULL_ARG), ("n_over", CAPACITY), ("fill_over", CAPACITY),
                ("fill_over_no_smooth", CAPACITY), ("ch0", CAPACITY), ("ch256", CAPACITY), ("segcap0", CAPACITY), ("too_large", CAPACITY),
                ("too_large_spans", CAPACITY), ("too_many_tiles", CAPACITY)]


@pytest.mark.parametrize("case,code", ROW_REFUSALS)
def test_refusals_queue_nothing_and_leave_the_outputs_untouched(harness, case, code):
    assert _run(harness, "refuse", case) == ["RC %d" % code, "LAUNCHES 0", "LAST -1", "OUT 1 1 1 0"]


def test_accepted_calls_and_their_launches(harness):
    """two launches per 65535 rows; the count launch is left out where no row has a frame and where neither spans nor counts are
    wanted; with nothing to write there is no launch and the counts are zeroed by a memset"""
    for case, n in (("ok", 2), ("ok_smooth_only", 1), ("ok_counts_only", 2), ("ok_spans_only", 2), ("ok_segcap0_no_spans", 2), ("ok_no_frames", 1),
                    ("ok_nothing", 0), ("ok_fill_without_smooth", 0), ("ok_no_outputs", 0), ("ok_no_rows", 0), ("ok_most_tiles", 1), ("ok_rows65536", 4)):
        out = _run(harness, "refuse", case)
        assert out[:3] == ["RC 0", "LAUNCHES %d" % n, "LAST %d" % n], (case, out)
        assert out[3] == ("OUT 1 0 1 1" if case in ("ok_nothing", "ok_fill_without_smooth") else "OUT 1 1 1 0"), (case, out)


def test_two_calls_back_to_back_each_reach_their_own_records(harness):
    """the second call's records do not replace the first's, which its kernels read later; the caller's arrays are free at once"""
    assert _run(harness, "two") == ["RC 0 LAST 2", "RC 0 LAST 1", "ROWS 3000/3000 0/3 4/4", "ROWS 3000/3000 0/3 4/4", "ROWS 1/1 257/257 13/13",
                                    "LAUNCHES 3"]


# ---- the kernel source on the host

def _kernel(harness, tmp_path, mask, n, fill_to, params, tile, segcap, want=(1, 1, 1), offs=(0, 0)):
    R, C, cap = mask.shape
    src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(src, "wb") as f:
        f.write(np.asarray(n, U64).tobytes())
        f.write(np.asarray(fill_to if fill_to is not None else [0] * R, U64).tobytes())
        f.write(np.ascontiguousarray(mask, np.uint8).tobytes())
    out = _run(harness, "run", tile, C, R, cap, segcap, int(fill_to is not None), want[0], want[1], want[2], offs[0], offs[1], *params, src, dst)
    assert out[0] == "RC 0" and out[2] == "TILE %d" % tile, out
    raw = np.fromfile(dst, np.uint8)
    ns, nc = R * C * segcap * 16, R * C * 8
    return (raw[:ns].view(U64).reshape(R, C, segcap, 2), raw[ns:ns + nc].view(U64).reshape(R, C), raw[ns + nc:].reshape(R, C, cap),
            int(out[1].split()[1]))


def _check(harness, tmp_path, mask, n, fill_to, params, tile, segcap, want=(1, 1, 1), offs=(0, 0)):
    spans, counts, smooth, launches = _kernel(harness, tmp_path, mask, n, fill_to, params, tile, segcap, want, offs)
    R, C, cap = mask.shape
    ws, wc, wo = M.rows(mask, n, fill_to, params, np.full((R, C, segcap, 2), M.SENT_SPAN, U64), np.full((R, C), M.SENT_SPAN, U64),
                        np.full((R, C, cap), M.SENT_MASK, np.uint8))
    if not want[0]:
        ws[:] = M.SENT_SPAN
    if not want[1]:
        wc[:] = M.SENT_SPAN
    if not want[2]:
        wo[:] = M.SENT_MASK
    M.same(spans, ws, "spans"), M.same(counts, wc, "counts"), M.same(smooth, wo, "smooth")
    span = max(max(n), max(fill_to) if fill_to is not None else 0) if want[2] else max(n)
    if span == 0 or not any(want):
        assert launches == 0
    else:
        assert launches == 1 + int(max(n) > 0 and bool(want[0] or want[1]))
    return ws, wc, wo


FILLS = [lambda n, cap: None, lambda n, cap: [cap] * len(n), lambda n, cap: [max(0, v - 2) for v in n],
         lambda n, cap: [min(cap, (v * 7 + 3) % (cap + 1)) for v in n]]
WANTS = [(1, 1, 1), (1, 0, 0), (0, 1, 0), (0, 0, 1)]


@pytest.mark.parametrize("params", PARAMS)
def test_kernel_on_the_host_is_the_model(harness, tmp_path, params):
    """[4][2][1103] with lengths 1100, 0, 257 and 600, tiles of 256 (five in the longest row; with the largest parameters the halo
    spans every tile of the row) and 1024 (two), seg_capacity at 1, exact and larger, each output alone and all together, the four
    kinds of fill_to and every residue of the masks' addresses against 4 bytes, in rotation"""
    i = 0
    for burst in (3, 30):
        mask = M.source(N, 2, CAP, 50 + burst, burst=burst)
        _, wc, _ = M.rows(mask, N, None, params, None, np.zeros((4, 2), U64), None)
        exact = max(1, int(wc.max()))
        for tile in (256, 1024):
            for segcap in (1, exact, exact + 3):
                for want in WANTS:
                    i += 1
                    _check(harness, tmp_path, mask, N, FILLS[i % 4](N, CAP), params, tile, segcap, want, offs=(i % 4, (i // 4) % 4))
        assert params[3] > 600 or wc.max() > 1


def test_every_residue_of_the_masks_against_four_bytes_and_every_kind_of_fill(harness, tmp_path):
    """the dword stores and the bytes at the ragged head and tail of every tile's span: all four residues of the smoothed mask's
    address, with all four kinds of fill_to each, at a capacity that moves every row and channel to another residue"""
    mask = M.source(N, 2, CAP, 77)
    for off in range(4):
        for k in range(4):
            _check(harness, tmp_path, mask, N, FILLS[k](N, CAP), (3, 7, 5, 4), 256, 40, offs=((off + k) % 4, off))


def test_runs_and_gaps_across_every_seam(harness, tmp_path):
    """runs of min_on - 1 and min_on frames and gaps of min_off - 1 and min_off frames laid so that each begins, ends and straddles a
    tile seam of 256 frames"""
    pad_on, pad_off, min_off, min_on = 0, 0, 6, 9
    T = 1100
    lines = []
    for shift in range(-9, 3):
        m = np.zeros(T, np.uint8)
        for seam in (256, 512, 768, 1024):
            k = (seam // 256) % 4
            length = (min_on - 1, min_on, min_on + min_off - 1, min_on + min_off)[k]
            m[seam + shift:seam + shift + length] = 1
            if k >= 2:                                               # two runs of min_on frames with a gap of min_off - 1 or min_off between them
                gap = min_off - 1 if k == 2 else min_off
                m[seam + shift + min_on:seam + shift + min_on + gap] = 0
                m[seam + shift + min_on + gap:seam + shift + 2 * min_on + gap] = 1
        lines.append(m)
    mask = np.full((len(lines), 1, T + 3), M.SENT_MASK, np.uint8)
    mask[:, 0, :T] = np.stack(lines)
    for tile in (256, 1024):
        _, wc, _ = _check(harness, tmp_path, mask, [T] * len(lines), None, (pad_on, pad_off, min_off, min_on), tile, 8)
        assert (wc == 4).all()                                       # min_on stays, the short gap is filled, the long one splits, min_on - 1 goes
    _check(harness, tmp_path, mask, [T] * len(lines), [T + 3] * len(lines), (2, 3, min_off, min_on), 256, 8)


def test_rows_do_not_leak_and_trivial_lines(harness, tmp_path):
    """every row alone gives what it gives among the others; T in {0, 1, 2}; all set, none set, 1010..., bytes 2 and 255"""
    mask = M.source(N, 2, CAP, 41)
    params = (3, 7, 5, 4)
    ws, wc, wo = _check(harness, tmp_path, mask, N, [CAP, 5, 0, 700], params, 256, 64)
    for r in range(4):
        s1, c1, o1 = _check(harness, tmp_path, mask[r:r + 1], N[r:r + 1], None, params, 1024, 64)
        assert np.array_equal(s1[0], ws[r]) and np.array_equal(c1[0], wc[r]) and np.array_equal(o1[0, :, :N[r]], wo[r, :, :N[r]])
    n = [0, 1, 2, 300, 300, 301, 10]
    m = np.full((7, 1, 303), M.SENT_MASK, np.uint8)
    m[1, 0, :1], m[2, 0, :2], m[3, 0, :300], m[4, 0, :300] = 1, [0, 9], 1, 0
    m[5, 0, :301] = np.arange(301) % 2 == 0
    m[6, 0, :10] = [0, 2, 0, 0, 255, 1, 0, 0, 0, 7]
    for params in ((0, 0, 0, 0), (1, 0, 0, 2)):
        for tile in (256, 1024):
            _, wc, _ = _check(harness, tmp_path, m, n, None, params, tile, 151)
        if params == (0, 0, 0, 0):
            assert wc[:, 0].tolist() == [0, 1, 1, 1, 0, 151, 3]
    _check(harness, tmp_path, m, [0] * 7, None, (0, 0, 0, 0), 1024, 4)
    _check(harness, tmp_path, m, [0] * 7, [3, 0, 303, 1, 0, 0, 0], (0, 0, 0, 0), 1024, 4)


def test_a_tile_far_up_a_row_past_frame_2_to_the_32(harness, tmp_path):
    """one row of 2^32 + 4096 + 9000 frames in tiles of 2048 of which only the last 9000 exist: the tile whose halo would reach in
    front of them is not run (its frames are unset), the others are, so the offsets of the mask, of the halo and of the smoothed
    bytes, the tile numbers (2^21 list entries in front) and the spans are all beyond 32 bits"""
    base, keep, tile = (1 << 32) + 4096, 9000, 2048
    params = (2, 8, 10, 5)
    m = M.source([keep], 1, keep, 99)[0, 0]
    m[:tile + 64] = 0
    src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    m.tofile(src)
    out = _run(harness, "far", tile, base, keep, 400, *params, src, dst)
    assert out == ["RC 0", "LAUNCHES 2"], out
    raw = np.fromfile(dst, np.uint8)
    spans, count, smooth = raw[:6400].view(U64).reshape(400, 2), int(raw[6400:6408].view(U64)[0]), raw[6408:]
    O = M.pointwise(m, *params)
    segs = M.runs(O)
    assert 20 < len(segs) == count < 400 and segs[0][0] > tile
    assert spans[:count].tolist() == [[base + a, base + b] for a, b in segs] and (spans[count:] == M.SENT_SPAN).all()
    assert (smooth[:tile] == M.SENT_MASK).all() and np.array_equal(smooth[tile:], O[tile:].astype(np.uint8))


# ---- Python

def test_python_parameter_errors_need_no_gpu():
    from lewton_amd.rows import CutRows, Segments
    for kw in [dict(device=-1), dict(device=1.5), dict(device="0"), dict(device=True), dict(pad_onset=1025), dict(pad_offset=-1), dict(min_off=1.0),
               dict(min_on=1025), dict(min_on=True), dict(pad_onset="3")]:
        with pytest.raises(ValueError):
            Segments(**kw)
    for kw in [dict(device=-1), dict(device=1.5), dict(device=True)]:
        with pytest.raises(ValueError):
            CutRows(**kw)


def test_jobs_converts_frames_to_elements_on_the_host():
    """Segments.jobs is plain host arithmetic on what it copies: rows numbered row * C + c, ascending, the ends clamped to the
    row's length, a count above seg_capacity refused"""
    import torch
    from lewton_amd.rows import Segments
    spans = torch.zeros((2, 2, 3, 2), dtype=torch.int64)
    spans[0, 0, :2] = torch.tensor([[0, 4], [10, 12]])
    spans[0, 1, :1] = torch.tensor([[3, 5]])
    spans[1, 1, :3] = torch.tensor([[1, 2], [5, 9], [20, 25]])
    counts = torch.tensor([[2, 1], [0, 3]])
    jobs, out_len = Segments.jobs(spans, counts)
    assert jobs.dtype == np.uint64 and jobs.tolist() == [[0, 0, 4], [0, 10, 12], [1, 3, 5], [3, 1, 2], [3, 5, 9], [3, 20, 25]]
    assert out_len.tolist() == [4, 2, 2, 1, 4, 5]
    jobs, out_len = Segments.jobs(spans, counts, hop=160, window=400, lengths=[2000, 4100])
    assert jobs.tolist() == [[0, 0, 880], [0, 1600, 2000], [1, 480, 1040], [3, 160, 560], [3, 800, 1680], [3, 3200, 4100]]
    assert out_len.tolist() == [880, 400, 560, 400, 880, 900]
    empty, none = Segments.jobs(spans, torch.zeros((2, 2), dtype=torch.int64))
    assert empty.shape == (0, 3) and empty.dtype == np.uint64 and none.tolist() == []
    with pytest.raises(ValueError):
        Segments.jobs(spans, torch.tensor([[2, 1], [0, 4]]))
    for kw in (dict(hop=0), dict(window=-1), dict(lengths=[1]), dict(hop=1.5)):
        with pytest.raises(ValueError):
            Segments.jobs(spans, counts, **kw)
