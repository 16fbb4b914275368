"""Segments of a frame mask and segment rows on the GPU: Segments.run (lw_segment_rows / k_segment_count, k_segment), Segments.jobs and
CutRows.run (lw_cut_rows / k_cut).  The cases of tests/test_gpu_rows_segment.py, which runs this file with pytest in a process of
its own, torch imported first (tests/rows_gpu_cases.py says why).

Both rules of include/lewton_amd.h ("segments of a frame mask", "cutting rows into segment rows") are on integers and bit copies.
The models are tests/segment_model.py and tests/cut_model.py.  Every comparison with them is over EVERY byte of sentinel-filled
exact-size buffers, with no tolerance; the mask holds non-zero sentinel bytes at and beyond each length."""
import torch  # noqa: F401  (first: see above)

import numpy as np
import pytest

import cut_model as CM
import segment_model as M
import rows_spec_gpu_cases as S

pytestmark = pytest.mark.gpu

F32, U64 = np.float32, np.uint64
N, CAP = [1100, 0, 257, 600], 1103
PARAMS = [(0, 0, 0, 0), (3, 7, 5, 4), (0, 40, 0, 0), (1024, 1024, 1024, 1024)]
SENT_I64 = int(np.array(M.SENT_SPAN, U64).view(np.int64))


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to("cuda:0")


def _make(params):
    from lewton_amd.rows import Segments
    return Segments(*params)


def _raw(seg, mask, n, fill_to, segcap, want=(1, 1, 1), src=None):
    """lw_segment_rows itself, so that every output can be left out and every destination holds a sentinel: (spans, counts, smooth)
    as numpy arrays, the sentinel where nothing was written; the mask is only read"""
    from lewton_amd import rows as R
    R_, C_, cap = mask.shape
    if src is None:
        src = _dev(mask)
    spans = torch.full((R_, C_, segcap, 2), SENT_I64, dtype=torch.int64, device="cuda:0")
    counts = torch.full((R_, C_), SENT_I64, dtype=torch.int64, device="cuda:0")
    smooth = torch.full((R_, C_, cap), M.SENT_MASK, dtype=torch.uint8, device="cuda:0")
    cnt = np.asarray(n, U64)
    fill = None if fill_to is None else np.asarray(fill_to, U64)
    seg._call(R.N.lw_segment_rows, C_, R._tensor_ptr(src), R._tensor_ptr(spans if want[0] else None), R._tensor_ptr(counts if want[1] else None),
              R._tensor_ptr(smooth if want[2] else None), R_, cap, segcap, R._array_ptr(cnt), R._array_ptr(fill), None)
    torch.cuda.synchronize()
    assert np.array_equal(src.cpu().numpy(), mask)
    return spans.cpu().numpy().view(U64), counts.cpu().numpy().view(U64), smooth.cpu().numpy()


def _launches(n, fill_to, want):
    span = max(max(n), max(fill_to) if fill_to is not None else 0) if want[2] else max(n)
    if span == 0 or not any(want):
        return 0
    return 1 + int(max(n) > 0 and bool(want[0] or want[1]))


def _check(seg, mask, n, fill_to, params, segcap, want=(1, 1, 1), src=None):
    """one call against the model: every span, count and byte of the smoothed mask"""
    spans, counts, smooth = _raw(seg, mask, n, fill_to, segcap, want, src)
    R_, C_, cap = mask.shape
    ws, wc, wo = M.rows(mask, n, fill_to, params, np.full((R_, C_, segcap, 2), M.SENT_SPAN, U64), np.full((R_, C_), M.SENT_SPAN, U64),
                        np.full((R_, C_, cap), M.SENT_MASK, np.uint8))
    if not want[0]:
        ws[:] = M.SENT_SPAN
    if not want[1]:
        wc[:] = M.SENT_SPAN
    if not want[2]:
        wo[:] = M.SENT_MASK
    M.same(spans, ws, "spans"), M.same(counts, wc, "counts"), M.same(smooth, wo, "smooth")
    assert seg.last_launches() == _launches(n, fill_to, want)
    return ws, wc, wo


FILLS = [lambda n, cap: None, lambda n, cap: [cap] * len(n), lambda n, cap: [max(0, v - 2) for v in n],
         lambda n, cap: [min(cap, (v * 7 + 3) % (cap + 1)) for v in n]]
WANTS = [(1, 1, 1), (1, 0, 0), (0, 1, 0), (0, 0, 1)]


@pytest.mark.parametrize("params", PARAMS)
def test_k_segment_is_the_model(params):
    """[4][2][1103] with lengths 1100, 0, 257 and 600, tiles of 256 (five in the longest row; with the largest parameters the halo
    spans every tile of the row) and 1024 (two), seg_capacity at 1, exact and larger, each output alone and all together, every
    kind of fill_to in rotation; the odd capacity takes the rows and channels over every residue of the masks against 4 bytes"""
    seg = _make(params)
    try:
        assert seg.tile_frames == 1024 and seg.last_launches() == -1
        i = 0
        for burst in (3, 30):
            mask = M.source(N, 2, CAP, 50 + burst, burst=burst)
            src = _dev(mask)
            _, wc, _ = M.rows(mask, N, None, params, None, np.zeros((4, 2), U64), None)
            exact = max(1, int(wc.max()))
            for tile in (256, 1024):
                seg.set_tile_frames(tile)
                for segcap in (1, exact, exact + 3):
                    for want in WANTS:
                        i += 1
                        _check(seg, mask, N, FILLS[i % 4](N, CAP), params, segcap, want, src=src)
            assert params[3] > 600 or wc.max() > 1
    finally:
        seg.close()


@pytest.mark.parametrize("T", [0, 1, 2, 255, 256, 257, 1023, 1024, 1025, 4097])
def test_lengths_at_the_tile_seams(T):
    """no frame, one, two, one short of a tile, a tile, one more, at both tile sizes, and seventeen tiles of 256 and a frame; the second
    row is all set, the third 1010...: K = ceil(T / 2), which the default seg_capacity just holds"""
    cap = T + 3
    mask = M.source([T, T, T], 2, cap, 300 + T, burst=5)
    mask[1, :, :T] = 1
    mask[2, :, :T] = (np.arange(T) % 2 == 0) * 255
    src = _dev(mask)
    for params in ((0, 0, 0, 0), (2, 8, 10, 5)):
        seg = _make(params)
        try:
            for tile in (256, 1024):
                seg.set_tile_frames(tile)
                _, wc, _ = _check(seg, mask, [T, T, T], [cap, 0, T], params, max(1, (cap + 1) // 2), src=src)
                if params == (0, 0, 0, 0):
                    assert wc[1].tolist() == [min(T, 1)] * 2 and wc[2].tolist() == [-(-T // 2)] * 2
        finally:
            seg.close()


def seam_lines(T, min_off, min_on):
    """lines with, at the seams 256, 512, 768 and 1024 moved by -9 .. 2 frames: a run of min_on frames, two such runs a gap of
    min_off - 1 frames apart, two a gap of min_off frames apart, and a run of min_on - 1 frames"""
    lines = []
    for shift in range(-9, 3):
        m = np.zeros(T, np.uint8)
        for seam in (256, 512, 768, 1024):
            k, at = (seam // 256) % 4, seam + shift
            if k == 0:
                m[at:at + min_on - 1] = 1
            elif k == 1:
                m[at:at + min_on] = 2
            else:
                gap = min_off - 1 if k == 2 else min_off
                m[at:at + min_on] = 255
                m[at + min_on + gap:at + 2 * min_on + gap] = 1
        lines.append(m)
    return np.stack(lines)


def test_runs_and_gaps_across_every_seam():
    """runs of min_on - 1 and min_on frames and gaps of min_off - 1 and min_off frames that begin in front of, at and behind every seam
    of the small tile and the one of the default; the short run goes, the short gap is filled, the long one splits: K = 4"""
    min_off, min_on, T = 6, 9, 1100
    lines = seam_lines(T, min_off, min_on)
    mask = np.full((len(lines), 1, T + 3), M.SENT_MASK, np.uint8)
    mask[:, 0, :T] = lines
    for params in ((0, 0, min_off, min_on), (2, 3, min_off, min_on)):
        seg = _make(params)
        try:
            for tile in (256, 1024):
                seg.set_tile_frames(tile)
                _, wc, _ = _check(seg, mask, [T] * len(lines), [T + 3] * len(lines), params, 8)
                assert (wc == 4).all()              # (with the pads the gap of min_off frames closes and the run of min_on - 1 stays)
        finally:
            seg.close()


def test_bytes_2_and_255_count_as_set_and_trivial_lines():
    n = [0, 1, 2, 300, 300, 301, 10]
    m = np.full((7, 1, 303), M.SENT_MASK, np.uint8)
    m[1, 0, :1], m[2, 0, :2], m[3, 0, :300], m[4, 0, :300] = 1, [0, 9], 1, 0
    m[5, 0, :301] = np.arange(301) % 2 == 0
    m[6, 0, :10] = [0, 2, 0, 0, 255, 1, 0, 0, 0, 7]
    for params in ((0, 0, 0, 0), (1, 0, 0, 2)):
        seg = _make(params)
        try:
            ws, wc, _ = _check(seg, m, n, None, params, 151)
            if params == (0, 0, 0, 0):
                assert wc[:, 0].tolist() == [0, 1, 1, 1, 0, 151, 3] and ws[6, 0, :3].tolist() == [[1, 2], [4, 6], [9, 10]]
            _check(seg, m, [0] * 7, None, params, 4)
            assert seg.last_launches() == 0
            _check(seg, m, [0] * 7, [3, 0, 303, 1, 0, 0, 0], params, 4)
            assert seg.last_launches() == 1
        finally:
            seg.close()


def test_rows_and_channels_do_not_leak():
    """rows of 1100, 0, 257 and 600 frames in one call give what each gives alone and in another order; nothing outside
    [0, max(T, fill_to)) of a row and channel of the smoothed mask is touched"""
    mask = M.source(N, 2, CAP, 41)
    params = (3, 7, 5, 4)
    seg = _make(params)
    try:
        ws, wc, wo = _check(seg, mask, N, [CAP, 5, 0, 700], params, 64)
        assert (wo[1, :, :5] == 0).all() and (wo[1, :, 5:] == M.SENT_MASK).all() and (wo[3, :, 700:] == M.SENT_MASK).all()
        assert wc[0, 0] > 2 and not np.array_equal(ws[0, 0], ws[0, 1])
        order = [2, 3, 1, 0]
        seg.set_tile_frames(256)
        gs, gc, go = _check(seg, mask[order], [N[r] for r in order], None, params, 64)
        for k, r in enumerate(order):
            assert np.array_equal(gs[k], ws[r]) and np.array_equal(gc[k], wc[r]) and np.array_equal(go[k, :, :N[r]], wo[r, :, :N[r]])
        for r in range(4):
            s1, c1, o1 = _check(seg, mask[r:r + 1], N[r:r + 1], None, params, 64)
            assert np.array_equal(s1[0], ws[r]) and np.array_equal(c1[0], wc[r]) and np.array_equal(o1[0, :, :N[r]], wo[r, :, :N[r]])
    finally:
        seg.close()


def test_run_and_jobs_and_more_segments_than_seg_capacity():
    """Segments.run: the default seg_capacity, zeroed spans behind K, bool masks in and out; with K > seg_capacity the counts are true,
    the tail of the spans is untouched and jobs() raises; jobs() converts frames to elements"""
    from lewton_amd.rows import Segments
    mask = M.source(N, 2, CAP, 43)
    params = (2, 8, 10, 5)
    seg = _make(params)
    try:
        ws, wc, wo = M.rows(mask, N, [CAP] * 4, params, np.zeros((4, 2, 552, 2), U64), np.zeros((4, 2), U64), np.full((4, 2, CAP), M.SENT_MASK, np.uint8))
        spans, counts, smooth = seg.run(_dev(mask), N, want_mask=True, fill_to=CAP)
        assert spans.dtype == torch.int64 and tuple(spans.shape) == (4, 2, 552, 2) and counts.dtype == torch.int64 and smooth.dtype == torch.bool
        jobs, out_len = Segments.jobs(spans, counts)                              # the one synchronisation
        M.same(spans.cpu().numpy().view(U64), ws, "spans"), M.same(counts.cpu().numpy().view(U64), wc, "counts")
        M.same(smooth.cpu().numpy().view(np.uint8), wo, "smooth")
        want_jobs = [(r * 2 + c, a, b) for r in range(4) for c in range(2) for a, b in ws[r, c, :int(wc[r, c])].tolist()]
        assert jobs.dtype == U64 and jobs.tolist() == [list(j) for j in want_jobs] and out_len.tolist() == [b - a for _, a, b in want_jobs]
        j2, l2 = Segments.jobs(spans, counts, hop=160, window=400, lengths=[v * 160 + 240 for v in N])
        assert j2.tolist() == [[r, a * 160, min((N[r // 2]) * 160 + 240, (b - 1) * 160 + 400)] for r, a, b in want_jobs]
        assert Segments.jobs(spans, counts, hop=3)[0].tolist() == [[r, 3 * a, 3 * b] for r, a, b in want_jobs]
        k = int(wc.max())
        assert k > 3
        bspans, bcounts = seg.run(_dev(mask != 0), N, seg_capacity=k - 1)              # a bool mask; one span too few
        torch.cuda.synchronize()
        M.same(bcounts.cpu().numpy().view(U64), wc, "counts")
        M.same(bspans.cpu().numpy().view(U64), ws[:, :, :k - 1], "spans")
        with pytest.raises(ValueError):
            Segments.jobs(bspans, bcounts)
        out = torch.full((4, 2, CAP), M.SENT_MASK, dtype=torch.uint8, device="cuda:0")
        _, _, sm = seg.run(_dev(mask), N, out_mask=out)
        torch.cuda.synchronize()
        assert sm.data_ptr() == out.data_ptr()
        M.same(out.cpu().numpy(), M.rows(mask, N, None, params, None, None, np.full((4, 2, CAP), M.SENT_MASK, np.uint8))[2], "smooth")
    finally:
        seg.close()


def test_calls_queued_back_to_back_on_one_stream_and_on_a_side_stream():
    """five calls of one object (more than it has record slots), different lengths each, nothing synchronised until the end: on
    torch's current stream, then on a side stream"""
    params = (2, 8, 10, 5)
    seg = _make(params)
    try:
        seg.set_tile_frames(256)
        mask = M.source([700] * 3, 2, 701, 21)
        src = _dev(mask)
        for side in (False, True):
            calls = []
            st = torch.cuda.Stream(device=0) if side else torch.cuda.current_stream(0)
            torch.cuda.synchronize()
            with torch.cuda.stream(st):
                for k in range(5):
                    n = [700 - 130 * k, 3 * k, 257 + k]
                    out = torch.full((3, 2, 701), M.SENT_MASK, dtype=torch.uint8, device="cuda:0")
                    spans, counts, _ = seg.run(src, n, seg_capacity=40, out_mask=out, fill_to=[k, 701, 0])
                    calls.append((n, [k, 701, 0], spans, counts, out))
            st.synchronize()
            for n, fill, spans, counts, out in calls:
                ws, wc, wo = M.rows(mask, n, fill, params, np.zeros((3, 2, 40, 2), U64), np.zeros((3, 2), U64), np.full((3, 2, 701), M.SENT_MASK, np.uint8))
                M.same(spans.cpu().numpy().view(U64), ws, "spans"), M.same(counts.cpu().numpy().view(U64), wc, "counts")
                M.same(out.cpu().numpy(), wo, "smooth")
    finally:
        seg.close()


def test_refusals_are_value_errors():
    from lewton_amd.rows import CutRows, Segments
    for kw in (dict(pad_onset=1025), dict(pad_offset=-1), dict(min_off=1.5), dict(min_on=1 << 20), dict(device=-1)):
        with pytest.raises(ValueError):
            Segments(**kw)
    seg, cut = Segments(1, 1, 1, 1), CutRows()
    try:
        m = _dev(M.source(N, 2, CAP, 41))
        for bad_tile in (0, 128, 300, 2304):
            with pytest.raises(ValueError):
                seg.set_tile_frames(bad_tile)
        bad = [lambda: seg.run(m, [1104, 0, 0, 0]), lambda: seg.run(m, N, fill_to=1104), lambda: seg.run(m, N[:3]), lambda: seg.run(m, N, seg_capacity=0),
               lambda: seg.run(m, [-1, 0, 0, 0]), lambda: seg.run(m, N, out_mask=m), lambda: seg.run(m.float(), N), lambda: seg.run(m[0], N[:2]),
               lambda: seg.run(m[:, :, :600], N), lambda: seg.run(m.cpu(), N),
               lambda: seg.run(m, N, out_mask=torch.zeros((4, 2, 1102), dtype=torch.uint8, device="cuda:0")),
               lambda: Segments.jobs(torch.zeros((2, 1, 4, 2), dtype=torch.int64), torch.zeros((2, 2), dtype=torch.int64)),
               lambda: Segments.jobs(torch.zeros((2, 1, 4, 2), dtype=torch.int64), torch.zeros((2, 1), dtype=torch.int64), hop=0),
               lambda: Segments.jobs(torch.zeros((2, 1, 4, 2), dtype=torch.int64), torch.zeros((2, 1), dtype=torch.int64), lengths=[1])]
        x = _dev(np.zeros((2, 2, 100), F32))
        bad += [lambda: cut.run(x, [100, 40], [(2, 0, 1)]), lambda: cut.run(x, [100, 40], [(0, 5, 4)]), lambda: cut.run(x, [100, 40], [(1, 0, 41)]),
                lambda: cut.run(x, [100], [(0, 0, 1)]), lambda: cut.run(x, [100, 40], [(0, 0, 1, 2)]), lambda: cut.run(x, [100, 40], [(0, -1, 1)]),
                lambda: cut.run(x, [100, 40], [(0, 0, 50)], out=torch.zeros((1, 2, 49), device="cuda:0")),
                lambda: cut.run(x, [100, 40], [(0, 0, 50)], out=torch.zeros((2, 2, 50), device="cuda:0")),
                lambda: cut.run(x, [100, 40], [(0, 0, 50)], out=torch.zeros((1, 2, 1, 50), device="cuda:0")),
                lambda: cut.run(x, [100, 40], [(0, 0, 50)], fill_to=[1, 2]), lambda: cut.run(x, [100, 40], [(0, 0, 50)], samples="i16"),
                lambda: cut.run(x, [100, 40], [(0, 0, 50)], samples="f64"), lambda: cut.run(x, [101, 40], [(0, 0, 50)])]
        for call in bad:
            with pytest.raises(ValueError):
                call()
        torch.cuda.synchronize()
        assert seg.last_launches() == -1 and cut.last_launches() == -1
        out, out_len = cut.run(x, [100, 40], [])                                   # no jobs: an empty tensor, no launch
        assert tuple(out.shape) == (0, 2, 0) and out_len.tolist() == [] and cut.last_launches() == 0
    finally:
        seg.close()
        cut.close()


def test_smoothed_mask_into_select_frames_is_the_two_models_composed():
    """want_mask -> SelectFrames: selection with a hangover, with no synchronisation in between"""
    import select_model as SM
    from lewton_amd.rows import SelectFrames
    params = (0, 8, 0, 3)
    x = SM.source(N, 2, 3, CAP, 9)
    mask = M.source(N, 2, CAP, 10, burst=4)
    seg, se = _make(params), SelectFrames()
    try:
        _, _, smooth = seg.run(_dev(mask), N, want_mask=True, fill_to=CAP)
        kept, counts = se.run(_dev(x), N, smooth, out=S._filled((4, 2, 3, CAP)), fill_to=[CAP, 5, 0, 700])
        torch.cuda.synchronize()
        wo = M.rows(mask, N, [CAP] * 4, params, None, None, np.full((4, 2, CAP), M.SENT_MASK, np.uint8))[2]
        want, wk = SM.rows(x, wo, N, [CAP, 5, 0, 700], np.full((4, 2, 3, CAP), SM.SENT_F, F32))
        SM.same_bits(kept.cpu().numpy(), want)
        raw = [int((mask[r, c, :N[r]] != 0).sum()) for r in range(4) for c in range(2)]
        assert counts.cpu().numpy().tolist() == wk.tolist() and wk.reshape(-1).tolist() != raw and 0 < wk[0, 0] < 1100
    finally:
        seg.close()
        se.close()


# ---- CutRows

def _cut_check(cut, x, n, jobs, fill_to, outcap, elem, src=None):
    """one call against the model: every element of a sentinel-filled destination, as bit patterns"""
    tdt = torch.float32 if elem == 4 else torch.int16
    sdt = np.float32 if elem == 4 else np.int16
    if src is None:
        src = _dev(x.view(sdt))
    dst = _dev(np.full((len(jobs),) + x.shape[1:-1] + (outcap,), CM.SENT[elem], CM.UINT[elem]).view(sdt))
    out, out_len = cut.run(src, n, jobs, out=dst, fill_to=fill_to, samples="f32" if elem == 4 else "i16")
    torch.cuda.synchronize()
    assert out is dst and out.dtype == tdt and out_len.tolist() == [b - a for _, a, b in jobs]
    x4 = x if x.ndim == 4 else x[:, :, None, :]
    want = CM.rows(x4, jobs, fill_to, np.full((len(jobs),) + x4.shape[1:-1] + (outcap,), CM.SENT[elem], CM.UINT[elem]))
    CM.same(dst.cpu().numpy().view(CM.UINT[elem]).reshape(want.shape), want)
    assert np.array_equal(src.cpu().numpy().view(CM.UINT[elem]), x)
    span = max([b - a for _, a, b in jobs] + (list(fill_to) if fill_to is not None else []), default=0)
    assert cut.last_launches() == (1 if span else 0)
    return want


@pytest.mark.parametrize("elem", [2, 4])
def test_k_cut_is_the_model_at_every_source_residue_and_length(elem):
    """[2][2][F][157] for F in {1, 3} and a 3-D source [2][2][157]: a job for every start in 16 bytes' worth of elements (an i16 source at
    an odd start among them) times every length in 0 .. 40, into rows of 43 elements (an odd pitch: every residue of the destination
    lines) and of 48 (aligned lines); without fill_to, filled to the row's end, and filled a few elements past each length"""
    from lewton_amd.rows import CutRows
    n = [157, 90]
    jobs = [(k % 2, 37 + s, 37 + s + ln) for k, (s, ln) in enumerate((s, ln) for s in range(16 // elem) for ln in range(41))]
    cut = CutRows()
    try:
        assert cut.last_launches() == -1
        for F in (1, 3, None):
            x = CM.source(n, 2, F or 1, 157, elem, 5 + elem + (F or 0))
            if F is None:
                x = x[:, :, 0, :]
            src = _dev(x.view(np.float32 if elem == 4 else np.int16))
            for fill in (None, [43] * len(jobs), [min(43, ((b - a) * 3) % 47) for _, a, b in jobs]):
                _cut_check(cut, x, n, jobs, fill, 43, elem, src)
            _cut_check(cut, x, n, jobs, None, 48, elem, src)
    finally:
        cut.close()


@pytest.mark.parametrize("elem", [2, 4])
def test_k_cut_long_jobs_repeated_and_overlapping(elem):
    """lines longer than a workgroup's 16384 bytes, starts of every residue, the same stretch twice, one job inside another, whole
    rows, empty jobs and the ends of both rows; then out=None: a zeroed tensor that just holds the longest job and fill_to"""
    from lewton_amd.rows import CutRows
    n = [10007, 9001]
    x = CM.source(n, 1, 2, 10007, elem, 9 + elem)
    jobs = [(0, 0, 10007), (1, 0, 9001), (0, 1, 10007), (0, 3, 9000), (0, 3, 9000), (1, 4097, 9001), (0, 5000, 5000), (1, 9001, 9001), (0, 5, 4101),
            (1, 7, 8200), (0, 10006, 10007)]
    cut = CutRows()
    try:
        want = _cut_check(cut, x, n, jobs, [0, 10008, 3, 10001, 0, 0, 5, 0, 4100, 9000, 10009], 10009, elem)
        assert np.array_equal(want[0, :, :, 1:10007], want[2, :, :, :10006])
        _cut_check(cut, x, n, jobs, None, 10008, elem)
        sdt = np.float32 if elem == 4 else np.int16
        out, out_len = cut.run(_dev(x.view(sdt)), n, np.asarray(jobs, U64), fill_to=10011, samples="f32" if elem == 4 else "i16")
        torch.cuda.synchronize()
        assert tuple(out.shape) == (11, 1, 2, 10011) and out_len.tolist() == [b - a for _, a, b in jobs]
        CM.same(out.cpu().numpy().view(CM.UINT[elem]), CM.rows(x, jobs, [10011] * 11, np.zeros((11, 1, 2, 10011), CM.UINT[elem])))
    finally:
        cut.close()


def test_cut_calls_queued_back_to_back_on_a_side_stream():
    from lewton_amd.rows import CutRows
    n = [3000, 2000]
    x = CM.source(n, 2, 1, 3000, 4, 17)
    src = _dev(x.view(F32))
    cut = CutRows()
    try:
        st = torch.cuda.Stream(device=0)
        torch.cuda.synchronize()
        calls = []
        with torch.cuda.stream(st):
            for k in range(5):
                jobs = [(0, k, 3000 - 7 * k), (1, 3 * k + 1, 2000), (k % 2, 100 * k, 100 * k + k)]
                dst = _dev(np.full((3, 2, 1, 3001), CM.SENT[4], np.uint32).view(F32))
                cut.run(src, n, jobs, out=dst, fill_to=[0, 3001, k])
                calls.append((jobs, [0, 3001, k], dst))
        st.synchronize()
        for jobs, fill, dst in calls:
            CM.same(dst.cpu().numpy().view(np.uint32), CM.rows(x, jobs, fill, np.full((3, 2, 1, 3001), CM.SENT[4], np.uint32)))
    finally:
        cut.close()


LIFECYCLE = {"Segments": lambda R: R(), "CutRows": lambda R: R()}


@pytest.mark.parametrize("name", sorted(LIFECYCLE))
def test_handle_lifecycle(name):
    """what tests/rows_gpu_cases.py checks for the other classes over a handle, with the smallest legal arguments and no launch: a
    handle after construction, -1 launches before any call, close() twice, then the finaliser; nothing raises"""
    import gc
    import sys
    from lewton_amd import rows as R
    unraisable, hook = [], sys.unraisablehook
    sys.unraisablehook = unraisable.append                                     # (where an exception in __del__ ends up)
    try:
        obj = LIFECYCLE[name](getattr(R, name))
        assert obj._h and obj.last_launches() == -1
        obj.close()
        assert obj._h is None
        obj.close()
        assert obj._h is None
        del obj
        gc.collect()
    finally:
        sys.unraisablehook = hook
    assert not unraisable, [repr(u.exc_value) for u in unraisable]


# ---- the chain

CHAIN_LENGTHS, CHAIN_SEED, CHAIN_CAP = [24000, 16000], 8, 150
CHAIN_SEG = (2, 8, 10, 5)


def chain_signal(seed=CHAIN_SEED):
    """two utterances of 1.5 s and 1 s at 16 kHz, noise in long bursts with short breaks inside them and long pauses between them: the
    envelope is 0.0005 + 0.5 * (sin(i / 1500 + r) > 0.2 and sin(i / 330 + 2 r) > -0.6)"""
    rng = np.random.default_rng(seed)
    x = np.full((2, 1, max(CHAIN_LENGTHS) + 3), S.SENT_F, F32)
    for r, n in enumerate(CHAIN_LENGTHS):
        i = np.arange(n)
        env = 0.0005 + 0.5 * ((np.sin(i / 1500.0 + r) > 0.2) & (np.sin(i / 330.0 + 2 * r) > -0.6))
        x[r, 0, :n] = (rng.standard_normal(n) * env).astype(F32)
    return x


def chain_models(x, basis, banks, mel, spec_basis):
    """the models composed, on the host: (fbank features, VAD mask, spans, counts, jobs, the cut rows, the Whisper features of every
    segment row, their frame counts, the frame capacity)"""
    import feat_model as FM
    import kaldi_model as K
    import spec_model as SP
    import spec_reflect_model as RM
    import vad_model as VM
    lengths, cap = CHAIN_LENGTHS, CHAIN_CAP
    T = [K.n_frames(n, 400, 160, True) for n in lengths]
    lin = np.zeros((2, 1, 81, cap), F32)
    for r in range(2):
        lin[r, 0, :, :T[r]] = K.features(basis, banks, K.frame_matrix(x[r, 0, :lengths[r]], 400, 160, True), True, True, 32768.0).T
    feats, _ = FM.rows(lin, T, [cap] * 2, lin, FM.LN, FM.ROW, K.EPS, np.inf, 0.0, 1.0)
    for r in range(2):
        feats[r, 0, 0, :T[r]] = np.maximum(feats[r, 0, 0, :T[r]], F32(np.log(1.0)))                   # energy_floor = 1
    vmask, _ = VM.rows(feats, T, [cap] * 2, np.zeros((2, 1, cap), np.uint8), VM.SRE)
    segcap = (cap + 1) // 2
    spans, counts, _ = M.rows(vmask, T, None, CHAIN_SEG, np.zeros((2, 1, segcap, 2), U64), np.zeros((2, 1), U64), None)
    jobs = [(r, a * 160, min(lengths[r], (b - 1) * 160 + 400)) for r in range(2) for a, b in spans[r, 0, :int(counts[r, 0])].tolist()]
    out_len = [b - a for _, a, b in jobs]
    cut = CM.rows(x.view(np.uint32)[:, :, None, :], jobs, None, np.zeros((len(jobs), 1, 1, max(out_len)), np.uint32))[:, :, 0, :].view(F32)
    frames = [SP.n_frames(n, 400, 160, True) for n in out_len]
    fcap = max(frames) + 2
    wlin = np.zeros((len(jobs), 1, 80, fcap), F32)
    for i, n in enumerate(out_len):
        wlin[i, 0, :, :frames[i]] = SP.features(spec_basis, mel, RM.frame_matrix(cut[i, 0, :n], 400, 400, 160)).T
    wfeat, _ = FM.rows(wlin, frames, [fcap] * len(jobs), wlin)
    return T, feats, vmask, spans, counts, jobs, cut, wfeat, frames, fcap


def chain_shows_what_it_must(T, vmask, spans, counts):
    """at least two segments in one row, and at least one segment that the smoothing changed: the segments are not the raw runs"""
    raw = [M.runs(vmask[r, 0, :T[r]] != 0) for r in range(2)]
    seg = [[tuple(s) for s in spans[r, 0, :int(counts[r, 0])].tolist()] for r in range(2)]
    return max(len(s) for s in seg) >= 2 and min(len(s) for s in seg) >= 1 and any(s not in raw[r] for r in range(2) for s in seg[r]), raw, seg


def test_fbank_to_vad_to_segments_to_cut_waveform_to_whisper_features_is_the_models_composed():
    """utterances of 24000 and 16000 samples through KaldiFbank(num_mel_bins=80, use_energy=True, scale=32768) -> EnergyVad(5.5, 0.5, 2,
    0.12) -> Segments(pad_onset=2, pad_offset=8, min_off=10, min_on=5) -> Segments.jobs(hop=160, window=400, lengths=...), the ONE
    synchronisation -> CutRows on the waveform -> Spectrogram(400, 160, mel=slaney, pad_mode="reflect") -> LogCompress.whisper() with
    every line filled: bit for bit kaldi_model -> feat_model -> vad_model -> segment_model -> cut_model -> spec_reflect_model ->
    feat_model.  The models alone show at least two segments in one row and segments that are not runs of the raw mask"""
    import feat_model as FM
    from lewton_amd.rows import CutRows, EnergyVad, KaldiFbank, LogCompress, Segments, Spectrogram, mel_filterbank
    mel = mel_filterbank(16000, 400, 80, scale="slaney", norm="slaney")
    fb, vad, seg, cut = KaldiFbank(num_mel_bins=80, use_energy=True, scale=32768.0), EnergyVad(5.5, 0.5, 2, 0.12), Segments(*CHAIN_SEG), CutRows()
    sp, lc = Spectrogram(400, 160, mel=mel, pad_mode="reflect"), LogCompress.whisper()
    try:
        lengths, cap = CHAIN_LENGTHS, CHAIN_CAP
        x = chain_signal()
        pcm = S._device(x, False)
        feats, frames = fb.run(pcm, lengths, fill_to=cap)
        mask = vad.run(feats, frames, fill_to=cap)
        spans, counts = seg.run(mask, frames)
        jobs, out_len = Segments.jobs(spans, counts, hop=160, window=400, lengths=lengths)          # the one synchronisation
        rows_, seg_len = cut.run(pcm, lengths, jobs)
        T, wfeats, wvmask, wspans, wcounts, wjobs, wcut, wfeat, wframes, fcap = chain_models(x, fb.spec.basis(), fb.banks, mel, sp.basis())
        wf, f2 = sp.run(rows_, seg_len, out=torch.zeros((len(jobs), 1, 80, fcap), device="cuda:0"))
        lc.run(wf, f2, fill_to=fcap)
        torch.cuda.synchronize()
        shows, raw, segs = chain_shows_what_it_must(T, wvmask, wspans, wcounts)
        print("chain: frames %r, raw runs %r, segments %r, jobs %r" % (T, raw, segs, wjobs))
        assert shows and frames.tolist() == T == [148, 98]
        import kaldi_model as K
        import vad_model as VM
        K.same_bits(feats.cpu().numpy(), wfeats)
        VM.same_mask(mask.cpu().numpy().view(np.uint8), wvmask)
        M.same(spans.cpu().numpy().view(U64), wspans, "spans"), M.same(counts.cpu().numpy().view(U64), wcounts, "counts")
        assert jobs.tolist() == [list(j) for j in wjobs] and out_len.tolist() == seg_len.tolist() == [b - a for _, a, b in wjobs]
        assert min(out_len.tolist()) >= (CHAIN_SEG[3] - 1) * 160 + 400 or any(b == lengths[r] for r, a, b in wjobs)
        CM.same(rows_.cpu().numpy().view(np.uint32), wcut.view(np.uint32))
        assert f2.tolist() == wframes
        FM.same_bits(wf.cpu().numpy(), wfeat)
    finally:
        for o in (fb, vad, seg, cut, sp, lc):
            o.close()
