"""Segments and segment rows past 65535 rows of a call, past frame 2^32 of ONE mask line and past byte 2^32 of a source, on the GPU:
k_segment_count, k_segment and k_cut.  The cases of tests/test_gpu_rows_segment_large.py, which runs this file with pytest in a process
of its own, torch imported first (tests/rows_gpu_cases.py says why).

Part A.  65 540 rows of 40 frames, a dozen of them live on both sides of row 65535, each with a mask and a length of its own: the
second launch has row0 != 0 in k_segment_count and k_segment, whose tile counts are indexed by the row of the LAUNCH and whose spans,
counts and smoothed bytes by the row of the call.  The live rows equal the model on every byte, every other span and smoothed byte
is still the sentinel (compared on the device), the counts of the other rows are 0.  Then 65 540 jobs of k_cut, every one a few
elements at a start of its own, into rows of 8 elements.

Part B.  One flat allocation of 2^32 + 2^20 + 5 + 64 bytes for a mask and one for the smoothed mask (8.6 GB together), made once.
  B.1  ONE mask line of 2^32 + 2^20 + 5 frames in tiles of 2048 (2^21 + 513 of them: every workgroup of k_segment adds up the list in
       front of its tile), with runs at the line's start, in the middle, across frame 2^32 (with a short break and a short gap
       behind it) and up to the line's end, and short runs that are dropped.  Spans and counts equal the model computed from the
       run list in Python integers; the smoothed mask is 1 on every segment and 0 between them (min and max on the device), the
       bytes behind the line are still the sentinel.
  B.2  ONE job of k_cut on the same allocation read as int16: its source offset lies past BYTE 2^32, at an odd element.
A few seconds and under 10 GB of device memory."""
import torch  # noqa: F401  (first: see above)

import time

import numpy as np
import pytest

import cut_model as CM
import segment_model as M

pytestmark = pytest.mark.gpu

U64 = np.uint64
NR = 65540
LIVE = [0, 1, 7, 32768, 40000, 65533, 65534, 65535, 65536, 65537, 65538, 65539]      # the second launch starts at row 65535
assert sum(r < 65535 for r in LIVE) == 7 and NR - 1 in LIVE
LONG = (1 << 32) + (1 << 20) + 5
SENT_I64 = int(np.array(M.SENT_SPAN, U64).view(np.int64))


# ---- part A

def test_segments_65540_rows():
    """[65540][1][40], parameters (0, 1, 2, 2), eight spans per row"""
    from lewton_amd.rows import Segments
    params, cap, segcap = (0, 1, 2, 2), 40, 8
    seg = Segments(*params)
    try:
        n = [40 - 2 * i for i in range(len(LIVE))]
        fill = [min(cap, v + 3) for v in n]
        m = M.source(n, 1, cap, 84, burst=3)
        ws, wc, wo = M.rows(m, n, fill, params, np.full((len(LIVE), 1, segcap, 2), M.SENT_SPAN, U64), np.zeros((len(LIVE), 1), U64),
                            np.full((len(LIVE), 1, cap), M.SENT_MASK, np.uint8))
        assert len({w.tobytes() for w in ws}) == len(LIVE) and 1 <= wc.min() and 3 < wc.max() <= segcap
        mask = torch.full((NR, 1, cap), M.SENT_MASK, dtype=torch.uint8, device="cuda:0")
        mask[LIVE] = torch.from_numpy(m).to("cuda:0")
        out = torch.full((NR, 1, cap), M.SENT_MASK, dtype=torch.uint8, device="cuda:0")
        all_n, all_fill = [0] * NR, [0] * NR
        for r, v, f in zip(LIVE, n, fill):
            all_n[r], all_fill[r] = v, f
        spans, counts, smooth = seg.run(mask, all_n, seg_capacity=segcap, out_mask=out, fill_to=all_fill)
        torch.cuda.synchronize()
        assert seg.last_launches() == 4 and smooth.data_ptr() == out.data_ptr()
        got = spans[LIVE].cpu().numpy().view(U64)
        want = ws.copy()
        want[want == M.SENT_SPAN] = 0                                          # (run() hands out zeroed spans)
        M.same(got, want, "spans"), M.same(out[LIVE].cpu().numpy(), wo, "smooth")
        all_k = np.zeros((NR, 1), U64)
        all_k[LIVE] = wc
        M.same(counts.cpu().numpy().view(U64), all_k, "counts")
        rest, rest_spans = out.clone(), spans.clone()
        rest[LIVE], rest_spans[LIVE] = M.SENT_MASK, 0
        assert bool((rest == M.SENT_MASK).all()) and bool((rest_spans == 0).all()), "written outside the live rows"
    finally:
        seg.close()


def test_cut_65540_jobs():
    """65 540 jobs over [3][1][100] int16 into [65540][1][8]: job i copies i % 7 elements from start i % 93 of row i % 3 and fills to
    i % 9 (at most 8)"""
    from lewton_amd.rows import CutRows
    cut = CutRows()
    try:
        x = CM.source([100, 100, 100], 1, 1, 100, 2, 5)
        i = np.arange(NR)
        jobs = np.stack([i % 3, i % 93, i % 93 + i % 7], axis=1).astype(U64)
        fill = np.minimum(i % 9, 8)
        dst = torch.from_numpy(np.full((NR, 1, 8), CM.SENT[2], np.uint16).view(np.int16)).to("cuda:0")
        out, out_len = cut.run(torch.from_numpy(x[:, :, 0, :].view(np.int16)).to("cuda:0"), [100] * 3, jobs, out=dst, fill_to=fill, samples="i16")
        torch.cuda.synchronize()
        assert cut.last_launches() == 2 and out_len.tolist() == (i % 7).tolist()
        want = CM.rows(x, jobs, fill, np.full((NR, 1, 1, 8), CM.SENT[2], np.uint16))
        CM.same(dst.cpu().numpy().view(np.uint16).reshape(NR, 1, 1, 8), want)
    finally:
        cut.close()


# ---- part B

class _Bufs:
    mask = smooth = None


@pytest.fixture(scope="module")
def bufs():
    free, _ = torch.cuda.mem_get_info(0)
    need = 2 * (LONG + 64) + (1 << 30)
    if free < need:
        pytest.skip("less than %.1f GB of device memory free" % (need / 1e9))
    torch.cuda.reset_peak_memory_stats(0)
    t0 = time.perf_counter()
    B = _Bufs()
    B.mask = torch.empty(LONG + 64, dtype=torch.uint8, device="cuda:0")
    B.smooth = torch.empty(LONG + 64, dtype=torch.uint8, device="cuda:0")
    yield B
    torch.cuda.synchronize()
    print("\n[rows_segment_large] part B: %.1f s from the allocation on, peak device memory %.2f GB" % (
        time.perf_counter() - t0, torch.cuda.max_memory_allocated(0) / 1e9))
    B.mask = B.smooth = None
    torch.cuda.empty_cache()


def test_one_mask_line_past_frame_2_to_the_32(bufs):
    """B.1"""
    from lewton_amd.rows import Segments
    params, T, X = (2, 8, 10, 30), LONG, 1 << 32
    raw = [(0, 40), (1000, 5000), (5004, 5010), ((1 << 31) + 17, (1 << 31) + 20), (X - 300, X + 100), (X + 104, X + 700), (X + 717, X + 900),
           (X + 2048 * 3 - 1, X + 2048 * 3 + 1), (T - 1500, T - 40), (T - 25, T)]
    want = M.sequential_runs(raw, T, *params)
    assert want == [(0, 48), (998, 5018), (X - 302, X + 908), (T - 1502, T)]          # merged, padded and clamped; the short runs are gone
    seg = Segments(*params)
    try:
        seg.set_tile_frames(2048)
        assert -(-T // 2048) == (1 << 21) + 513 <= 0xFFFFFF
        mask, sm = bufs.mask, bufs.smooth
        mask[:T].zero_()
        mask[T:].fill_(M.SENT_MASK)
        for k, (a, b) in enumerate(raw):
            mask[a:b] = (1, 2, 255)[k % 3]
        sm.fill_(M.SENT_MASK)
        t0 = time.perf_counter()
        spans, counts, _ = seg.run(mask[:T].view(1, 1, T), [T], seg_capacity=6, out_mask=sm[:T].view(1, 1, T))
        torch.cuda.synchronize()
        print("\n[rows_segment_large] B.1: %.2f s for the call" % (time.perf_counter() - t0))
        assert seg.last_launches() == 2
        assert counts.cpu().tolist() == [[len(want)]] and spans.cpu()[0, 0].tolist() == [list(s) for s in want] + [[0, 0]] * 2
        assert bool((sm[T:] == M.SENT_MASK).all()), "written behind the line"
        at = 0
        for a, b in want + [(T, T)]:
            if a > at:
                lo, hi = torch.aminmax(sm[at:a])
                assert int(lo) == int(hi) == 0, (at, a, int(lo), int(hi))
            if b > a:
                lo, hi = torch.aminmax(sm[a:b])
                assert int(lo) == int(hi) == 1, (a, b, int(lo), int(hi))
            at = b
        assert int(mask[X]) == 2 and int(mask[X + 101]) == 0                         # the mask was only read
    finally:
        seg.close()


def test_cut_job_past_byte_2_to_the_32(bufs):
    """B.2"""
    from lewton_amd.rows import CutRows
    cut = CutRows()
    try:
        src = bufs.mask[:(LONG + 64) // 2 * 2].view(torch.int16)                     # 2^31 + 2^19 + 34 elements
        cap = src.shape[0]
        start, end = (1 << 31) + 4097, (1 << 31) + 4097 + 20011                    # bytes 2^32 + 8194 ..: an odd element
        assert start * 2 > 1 << 32 and start % 2 and end < cap
        w = CM.source([end - start + 16], 1, 1, end - start + 16, 2, 23)[0, 0, 0]
        src[start - 8:end + 8] = torch.from_numpy(w.view(np.int16)).to("cuda:0")
        dst = torch.from_numpy(np.full((1, 1, 20020), CM.SENT[2], np.uint16).view(np.int16)).to("cuda:0")
        out, out_len = cut.run(src.view(1, 1, cap), [cap], [(0, start, end)], out=dst, fill_to=20015, samples="i16")
        torch.cuda.synchronize()
        got = dst.cpu().numpy().view(np.uint16)[0, 0]
        assert cut.last_launches() == 1 and out_len.tolist() == [20011]
        assert np.array_equal(got[:20011], w[8:-8]) and (got[20011:20015] == 0).all() and (got[20015:] == CM.SENT[2]).all()
    finally:
        cut.close()
