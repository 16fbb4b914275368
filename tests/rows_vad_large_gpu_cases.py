"""The energy VAD past 65535 rows of a call, past byte 2^32 of a mask and element 2^32 of a source, and past frame 2^32 of ONE row,
on the GPU: k_vad, k_vad_sum, k_vad_fold and k_vad_decide.  The cases of tests/test_gpu_rows_vad_large.py, which runs this file with
pytest in a process of its own, torch imported first (tests/rows_gpu_cases.py says why).

Part A.  65 540 rows of a short capacity, a dozen of them live on both sides of row 65535 (tests/rows_large_gpu_cases.py's LIVE), each
with data and a length of its own, through both routes: the second launch has row0 != 0 in k_vad and in all three kernels of the
split form, whose chunk lists, fold scratch and thresholds are indexed by the row of the CALL.  The live rows equal the model on
every byte, every other byte of the mask is still the sentinel (compared on the device), the thresholds of all 65 540 rows are
the model's (energy_threshold for the empty ones).

Part B.  One flat allocation of 17 x (2^28 + 5) floats (18.3 GB) and one of as many mask bytes (4.6 GB), made once.
  B.1  [17][1][1][2^28 + 5]: the energy line of row 16 starts past element 2^32 of the source and its mask past BYTE 2^32, in one
       call; rows 0, 8 and 16 are live with a few thousand frames, only a window of every row is touched.  Both routes, tiles of 256
       and 1024.  The live windows equal the model, the windows of the other rows are still the sentinel.
  B.2  ONE row of 2^32 + 2^20 + 5 frames through the split route: 16 781 313 chunks, more than 64^4, so FIVE fold levels.  The line is
       10.0 with stretches of 14.0 (one across frame 2^32, one up to the row's end), a lone 14.0 and a lone 10.0: every value is a
       small integer, so the sum is exact in double in any order and S comes from Python integers; the threshold (6.0, 0.5, 2, 0.6)
       lies between the two levels.  The mask is compared with the model in windows of 2048 frames around every change of the
       line and must be constant (min == max on the device) between them; the bytes behind the row are still the sentinel.

Measured on an MI355X: the child run takes 4.2 s for its 7 cases (2.6 s inside pytest), with 23.89 GB of device memory allocated
through torch at the peak (the object's own chunk list of B.2, 134 MB, comes on top)."""
import torch  # noqa: F401  (first: see above)

import time

import numpy as np
import pytest

import vad_model as M
import rows_spec_gpu_cases as S

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
NR = 65540
LIVE = [0, 1, 7, 32768, 40000, 65533, 65534, 65535, 65536, 65537, 65538, 65539]      # the second launch starts at row 65535
assert sum(r < 65535 for r in LIVE) == 7 and NR - 1 in LIVE
ODD = (1 << 28) + 5
ROWS = 17
ELEMS = ROWS * ODD
LONG = (1 << 32) + (1 << 20) + 5
assert ELEMS > LONG > 1 << 32 and (ROWS - 1) * ODD >= 1 << 32


# ---- part A

@pytest.mark.parametrize("route", ["fused", "split"])
def test_vad_65540_rows(route):
    """[65540][1][2][300], the energy in line 1, a tile of 256 (two tiles per live row)"""
    from lewton_amd.rows import EnergyVad
    cfg = (5.5, 0.5, 2, 0.6)
    vad = EnergyVad(*cfg, 1)
    try:
        vad.set_tile_frames(256)
        vad.set_route(route)
        n = [300 - 3 * i for i in range(len(LIVE))]
        fill = [min(300, v + 2) for v in n]
        assert min(n) > 256
        x = M.source(n, 1, 2, 300, 82, line_i=1, others_nan=True)
        want, thr = M.rows(x, n, fill, np.full((len(LIVE), 1, 300), M.SENT_MASK, np.uint8), cfg, 1)
        assert len({t.tobytes() for t in thr[:, 0]}) == len(LIVE) and all(0 < want[i, 0, :n[i]].mean() < 1 for i in range(len(LIVE)))
        src = S._filled((NR, 1, 2, 300))
        src[LIVE] = torch.from_numpy(x).to("cuda:0")
        dst = torch.full((NR, 1, 300), M.SENT_MASK, dtype=torch.uint8, device="cuda:0")
        all_n, all_fill = [0] * NR, [0] * NR
        for r, v, f in zip(LIVE, n, fill):
            all_n[r], all_fill[r] = v, f
        mask, got_thr = vad.run(src, all_n, out=dst, fill_to=all_fill, want_threshold=True)
        torch.cuda.synchronize()
        assert vad.last_launches() == (2 if route == "fused" else 6) and mask.data_ptr() == dst.data_ptr()
        M.same_mask(dst[LIVE].cpu().numpy(), want)
        rest = dst.clone()
        rest[LIVE] = M.SENT_MASK
        assert bool((rest == M.SENT_MASK).all()), "written outside the live rows"
        all_thr = np.full((NR, 1), F32(5.5), F32)
        all_thr[LIVE] = thr
        M.same_thr(got_thr.cpu().numpy(), all_thr)
        assert np.array_equal(src[LIVE].cpu().numpy().view(np.uint32), x.view(np.uint32))
    finally:
        vad.close()


# ---- part B

class _Bufs:
    src = mask = None


@pytest.fixture(scope="module")
def bufs():
    free, _ = torch.cuda.mem_get_info(0)
    need = ELEMS * 5 + (2 << 30)
    if free < need:
        pytest.skip("less than %.1f GB of device memory free" % (need / 1e9))
    torch.cuda.reset_peak_memory_stats(0)
    t0 = time.perf_counter()
    B = _Bufs()
    B.src = torch.empty(ELEMS, dtype=torch.float32, device="cuda:0")
    B.mask = torch.empty(ELEMS, dtype=torch.uint8, device="cuda:0")
    yield B
    torch.cuda.synchronize()
    print("\n[rows_vad_large] part B: %.1f s from the allocation on, peak device memory %.2f GB" % (
        time.perf_counter() - t0, torch.cuda.max_memory_allocated(0) / 1e9))
    B.src = B.mask = None
    torch.cuda.empty_cache()


@pytest.mark.parametrize("route,tile", [("fused", 256), ("split", 1024), ("split", 256), ("fused", 1024)])
def test_k_vad_past_2_to_the_32(bufs, route, tile):
    """B.1"""
    from lewton_amd.rows import EnergyVad
    cfg = M.SRE
    vad = EnergyVad(*cfg)
    try:
        vad.set_tile_frames(tile)
        vad.set_route(route)
        live = (0, 8, 16)
        n = [0] * ROWS
        for r, v in zip(live, (2 * tile + 188, 2 * tile + 60, 2 * tile + 519)):
            n[r] = v
        fill = [v + 9 if v else 0 for v in n]
        W = max(n) + 41
        x = M.source(n, 1, 1, W, 600 + tile)
        src, dst = bufs.src.view(ROWS, 1, 1, ODD), bufs.mask.view(ROWS, 1, ODD)
        last = (ROWS - 1) * ODD + n[-1] - 1                              # the last live frame: its element and its byte
        assert last > 1 << 32 and 8 * ODD > 1 << 31
        src[..., :W].copy_(torch.from_numpy(x))
        dst[..., :W].fill_(M.SENT_MASK)
        mask, thr = vad.run(src, n, out=dst, fill_to=fill, want_threshold=True)
        torch.cuda.synchronize()
        assert vad.last_launches() == (1 if route == "fused" else 3)
        want, wthr = M.rows(x, n, fill, np.full((ROWS, 1, W), M.SENT_MASK, np.uint8), cfg)
        M.same_mask(dst[..., :W].cpu().numpy(), want)
        M.same_thr(thr.cpu().numpy(), wthr)
        assert 0 < want[16, 0, :n[16]].mean() < 1 and (want[1] == M.SENT_MASK).all() and wthr[16, 0] != wthr[0, 0]
        assert np.array_equal(src[..., :W].cpu().numpy().view(np.uint32), x.view(np.uint32))
    finally:
        vad.close()


def test_one_row_past_frame_2_to_the_32(bufs):
    """B.2"""
    from lewton_amd.rows import EnergyVad
    cfg = (6.0, 0.5, 2, 0.6)
    T, lo, hi = LONG, 10.0, 14.0
    stretches = [(1000, 5000), ((1 << 31) + 17, (1 << 31) + 18), ((1 << 32) - 300, (1 << 32) + 700), (T - 1500, T)]
    hole = (1 << 32) + 100                                                    # a lone 10.0 inside the stretch across 2^32
    vad = EnergyVad(*cfg)
    try:
        assert vad.tile_frames == 1024
        src, dst = bufs.src[:T], bufs.mask[:T + 64]
        src.fill_(lo)
        for a, b in stretches:
            src[a:b] = hi
        src[hole] = lo
        dst.fill_(M.SENT_MASK)
        n_hi = sum(b - a for a, b in stretches) - 1
        S_int = 10 * (T - n_hi) + 14 * n_hi                                   # exact: below 2^53
        want_thr = M.threshold(float(S_int), T, cfg[0], cfg[1])
        assert lo < want_thr < hi and -(-T // 256) > 64 ** 4
        mask, thr = vad.run(src.view(1, 1, 1, T), [T], out=dst[:T].view(1, 1, T), want_threshold=True)
        torch.cuda.synchronize()
        assert vad.last_launches() == 3
        assert thr.cpu().numpy()[0, 0].tobytes() == want_thr.tobytes()
        assert bool((dst[T:] == M.SENT_MASK).all()), "written behind the row"
        edges = sorted({e for a, b in stretches for e in (a, b)} | {hole})
        at, ones = 0, 0
        for e in edges:
            w0, w1 = max(0, e - 1024), min(T, e + 1024)
            c0, c1 = max(0, w0 - 256), min(T, w1 + 256)                      # the model's slice, with more context than the rule takes
            local = M.decide(src[c0:c1].cpu().numpy(), c1 - c0, want_thr, cfg[2], cfg[3])[w0 - c0:w1 - c0]
            got = dst[w0:w1].cpu().numpy()
            assert np.array_equal(got, local), (e, np.flatnonzero(got != local)[:4].tolist())
            if w0 > at:                                                        # constant between the windows
                gap = dst[at:w0]
                v = int(gap[0])
                assert int(gap.min()) == int(gap.max()) == v and v == int(got[0]) and v in (0, 1), (at, w0, v)
                ones += v * (w0 - at)
            ones += int(local[max(at, w0) - w0:].sum())
            at = max(at, w1)
        assert at == T
        voiced = sum(int(c.sum(dtype=torch.int64)) for c in dst[:T].split(1 << 27))      # (in pieces: the sum casts its input to int64 first)
        assert voiced == ones and 5000 < voiced < 7000, (voiced, ones)
        assert int(dst[(1 << 31) + 17]) == 0 and int(dst[hole]) == 1 and int(dst[T - 1]) == 1 and int(dst[1 << 32]) == 1
    finally:
        vad.close()
