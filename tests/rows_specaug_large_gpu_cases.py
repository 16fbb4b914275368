"""SpecAugment masks past 65535 rows of a call, past element 2^32 of a tensor and past frame 2^32 of ONE row, on the GPU: k_specaug.
The cases of tests/test_gpu_rows_specaug_large.py, which runs this file with pytest in a process of its own, torch imported first
(tests/rows_gpu_cases.py says why).

Part A.  65 540 rows of [1][3][40] out of place, ids=None, so every row's id is its index IN THE CALL: the second launch has
row0 != 0.  Rows 0, 1, 65534 .. 65539 equal the model on every element and every span; every row keeps what lies outside its span.

Part B.  One flat allocation of 3 x (2^31 + 7) floats (25.8 GB), made once and filled with 1.0; both calls are in place, so they
write the masked elements alone and what they did is counted on the device.
  B.1  [1][1][3][2^31 + 7]: line 2 starts past element 2^32.  Three time masks of up to 65535 frames and one frequency mask of one
       bin, the id picked with the model so that the masked line is line 2.  The masked line is all fill, the time masks' spans of
       the other lines are fill and 4096 frames either side of each are the model's; the count of fill in the whole tensor is the
       model's, so nothing else was written.
  B.2  ONE F = 1 line of 2^32 + 2^20 + 5 frames, seed 2024, 32 time masks of up to 65535 frames, id 6099: mask 18 straddles frame
       2^32 ([4294953827, 4294968123)).  Every span with 4096 frames either side equals the model, the count of fill in the whole
       line is the length of the spans' union, the floats behind the line are untouched."""
import torch  # noqa: F401  (first: see above)

import time

import numpy as np
import pytest

import specaug_model as M

pytestmark = pytest.mark.gpu

F32, U32 = np.float32, np.uint32
NR = 65540
LIVE = [0, 1, 65534, 65535, 65536, 65537, 65538, 65539]                            # the second launch starts at row 65535
ODD = (1 << 31) + 7
ELEMS = 3 * ODD
LONG = (1 << 32) + (1 << 20) + 5
assert ELEMS > LONG + 64 and 2 * ODD > 1 << 32
BASE, FILL = 1.0, -2.5
FILL_BITS = M.bits_of(FILL)


# ---- part A

def test_specaug_65540_rows():
    """[65540][1][3][40]: two launches; a row's id is its index in the call"""
    from lewton_amd.rows import SpecAugment
    P = M.Params(seed=8, num_t=2, min_t=1, max_t=12, num_f=1, min_f=0, max_f=2, fill_bits=FILL_BITS)
    sa = SpecAugment(2, 12, 1, 2, 1, 0, fill=FILL, seed=8)
    try:
        sa.set_tile_frames(256)
        g = torch.Generator(device="cuda:0").manual_seed(5)
        src = torch.randn((NR, 1, 3, 40), device="cuda:0", generator=g)
        n = [40 - r % 7 for r in range(NR)]
        fill = [min(40, v + r % 3) for r, v in enumerate(n)]
        dst = torch.empty_like(src).view(torch.int32).fill_(M.SENT_DST).view(torch.float32)
        out, spans = sa.run(src, n, out=dst, fill_to=fill, want_spans=True)
        torch.cuda.synchronize()
        assert sa.last_launches() == 2 and out.data_ptr() == dst.data_ptr() and tuple(spans.shape) == (NR, 1, 3, 2)
        x = src[LIVE].cpu().numpy().view(U32)
        want, wspans = M.rows(P, x, [n[r] for r in LIVE], [fill[r] for r in LIVE], LIVE, np.full(x.shape, M.SENT_DST, U32))
        M.same_bits(dst[LIVE].cpu().numpy(), want)
        assert np.array_equal(spans[LIVE].cpu().numpy(), wspans) and len({s.tobytes() for s in wspans}) == len(LIVE)
        ends = torch.tensor(fill, device="cuda:0")[:, None, None, None]
        beyond = torch.arange(40, device="cuda:0")[None, None, None, :] >= ends
        assert bool((dst.view(torch.int32)[beyond.expand_as(dst)] == M.SENT_DST).all()), "written beyond a row's span"
        inside = dst.view(torch.int32)[(~beyond).expand_as(dst)]
        assert not bool((inside == M.SENT_DST).any()), "a position inside a row's span was not written"
        s = spans[:, 0, :2]
        assert bool(((s[..., 0] >= 0) & (s[..., 1] <= torch.tensor(n, device="cuda:0")[:, None]) & (s[..., 1] - s[..., 0] >= 1) & (s[..., 1] - s[..., 0] <= 12)).all())
    finally:
        sa.close()


# ---- part B

@pytest.fixture(scope="module")
def buf():
    free, _ = torch.cuda.mem_get_info(0)
    need = ELEMS * 4 + (3 << 30)
    if free < need:
        pytest.skip("less than %.1f GB of device memory free" % (need / 1e9))
    torch.cuda.reset_peak_memory_stats(0)
    t0 = time.perf_counter()
    b = torch.empty(ELEMS, dtype=torch.float32, device="cuda:0")
    yield b
    torch.cuda.synchronize()
    print("\n[rows_specaug_large] part B: %.1f s from the allocation on, peak device memory %.2f GB" % (
        time.perf_counter() - t0, torch.cuda.max_memory_allocated(0) / 1e9))
    del b
    torch.cuda.empty_cache()


def _count(t, value):
    """elements of the flat tensor t equal to value, in pieces (the comparison makes a temporary)"""
    return sum(int((c == value).sum()) for c in t.split(1 << 28))


def _union(spans):
    merged = []
    for a, b in sorted(s for s in spans if s[0] < s[1]):
        if merged and a <= merged[-1][1]:
            merged[-1][1] = max(merged[-1][1], b)
        else:
            merged.append([a, b])
    return merged


def _windows_are_the_model(line, T, spans):
    """every merged span of the line with 4096 frames either side against the model; returns the union's length"""
    merged = _union(spans)
    for a, b in merged:
        w0, w1 = max(0, a - 4096), min(T, b + 4096)
        want = np.full(w1 - w0, BASE, F32)
        for s, e in merged:
            lo, hi = max(s, w0), min(e, w1)
            if lo < hi:
                want[lo - w0:hi - w0] = FILL
        got = line[w0:w1].cpu().numpy()
        assert np.array_equal(got.view(U32), want.view(U32)), ((a, b), np.flatnonzero(got != want)[:4].tolist())
    return sum(b - a for a, b in merged)


def test_line_past_element_2_to_the_32_in_place(buf):
    """B.1"""
    from lewton_amd.rows import SpecAugment
    P = M.Params(seed=2024, num_t=3, min_t=100, max_t=65535, num_f=1, min_f=1, max_f=1, fill_bits=FILL_BITS)
    id_ = next(i for i in range(1000) if M.plan(P, i, 0, ODD, 3)[3] == (2, 3))
    plan = M.plan(P, id_, 0, ODD, 3)
    sa = SpecAugment(3, 65535, 1, 1, 100, 1, fill=FILL, seed=2024)
    try:
        assert sa.tile_frames == 2048
        buf.fill_(BASE)
        x = buf.view(1, 1, 3, ODD)
        out, spans = sa.run(x, [ODD], ids=[id_], want_spans=True)
        torch.cuda.synchronize()
        assert out.data_ptr() == buf.data_ptr() and sa.last_launches() == 1
        assert [tuple(int(v) for v in p) for p in spans[0, 0].cpu()] == plan
        assert _count(x[0, 0, 2], FILL) == ODD                                          # the masked line, past element 2^32
        u = 0
        for f in (0, 1):
            u = _windows_are_the_model(x[0, 0, f], ODD, plan[:3])
            assert _count(x[0, 0, f], FILL) == u and _count(x[0, 0, f], BASE) == ODD - u
        assert 300 <= u <= 3 * 65535
    finally:
        sa.close()


def test_one_row_past_frame_2_to_the_32_in_place(buf):
    """B.2"""
    from lewton_amd.rows import SpecAugment
    P = M.Params(seed=2024, num_t=32, min_t=0, max_t=65535, num_f=0, fill_bits=FILL_BITS)
    plan = M.plan(P, 6099, 0, LONG, 1)
    assert plan[18] == (4294953827, 4294968123) and not any(a <= 4294968123 < b for a, b in plan)
    sa = SpecAugment(32, 65535, 0, 0, fill=FILL, seed=2024)
    try:
        assert sa.tile_frames == 2048
        buf[:LONG + 64].fill_(BASE)
        line = buf[:LONG]
        out, spans = sa.run(line.view(1, 1, LONG), [LONG], ids=[6099], want_spans=True)
        torch.cuda.synchronize()
        assert out.data_ptr() == buf.data_ptr() and sa.last_launches() == 1
        assert [tuple(int(v) for v in p) for p in spans[0, 0].cpu()] == plan
        u = _windows_are_the_model(line, LONG, plan)
        assert _count(line, FILL) == u and bool((buf[LONG:LONG + 64] == BASE).all())
        assert float(line[(1 << 32) - 1]) == FILL and float(line[1 << 32]) == FILL and float(line[4294968123]) == BASE
    finally:
        sa.close()
