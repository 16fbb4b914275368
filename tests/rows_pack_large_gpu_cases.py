"""k_pack past element 2^32 of its source and of its destination, on the GPU.  The cases of tests/test_gpu_rows_pack_large.py, which
runs this file with pytest in a process of its own, torch imported first (tests/rows_gpu_cases.py says why).

The kernel forms its addresses from several products (row x channel x lines x frame_capacity and line x frame_capacity on the source
side, row x channel x out_capacity x D and frame x D on the destination side, row x out_capacity for the mask), in elements, and the
destination's in bytes of a dtype.  Each index reaches 2^32 in a case of its own, in views of one source allocation of 24 lines of
2^28 + 5 frames (lines off the 16-byte boundaries):
  rows      source [3][1][8][2^28 + 5] (a row is 2^31 + 40 elements: row 1 starts past 2^31, row 2 past 2^32), destination
            [3][1][2^24 + 3][128] with W = 16 (a row is 2^31 + 384 elements); one case per dtype: the byte offsets differ.
  channels  source [1][9][2][2^28 + 5] (a channel is 2^29 + 10 elements: channel 8 starts past 2^32, channel 5 past 2^31),
            destination [1][9][2^24 + 3][32] with W = 16 (a channel is 2^29 + 96 elements); f32 and bf16.
  lines     source [1][1][17][2^28 + 5]: line 16 starts past 2^32 -- (f0 + g) x line_el; the destination is small.
Only windows are touched: a few hundred frames at the start of every source line and of every destination row and channel; the
work is tiny, the offsets are huge.  Before the call every destination window and the whole mask hold a sentinel and the source
holds one from each length on; afterwards the windows equal the model bit for bit -- the windows of row 0, channel 0 and line 0 are
where a truncated offset would land, and they hold other data.  Python integers assert the crossings.  (The position INSIDE a row,
(u0 + u) x D, crosses in tests/rows_long_row_gpu_cases.py.)  No tolerance."""
import torch  # noqa: F401  (first: see above)

import numpy as np
import pytest

import pack_model as M
from rows_pack_gpu_cases import INT, TORCH, _signed

pytestmark = pytest.mark.gpu

F32 = np.float32
CAP = (1 << 28) + 5
OCAP = (1 << 24) + 3
F, LEFT, RIGHT, STRIDE = 8, 7, 8, 3
D = (LEFT + RIGHT + 1) * F
SRC_ELEMS, DST_ELEMS = 3 * F * CAP, 3 * OCAP * D
WIN, OWIN = 304, 120                   # source frames per line and destination frames per row that the case looks at


@pytest.fixture(scope="module")
def source():
    """the source allocation, flat: 24 lines of CAP frames"""
    free, _ = torch.cuda.mem_get_info(0)
    need = 4 * SRC_ELEMS + 4 * DST_ELEMS + (4 << 30)
    if free < need:
        pytest.skip("less than %.1f GB of device memory free" % (need / 1e9))
    src = torch.empty(SRC_ELEMS, dtype=torch.float32, device="cuda:0")
    yield src
    del src
    torch.cuda.empty_cache()


def _case(flat, shape, ocap, left, right, stride, dtype, n, fill, seed):
    """one call: the source viewed as shape + [CAP], the destination [rows][ch][ocap][D] allocated for the call; the windows of
    both against the model.  Returns the output frames"""
    from lewton_amd.rows import FramePack
    R, C, Fl = shape
    Dl = (left + right + 1) * Fl
    assert R * C * Fl * CAP <= flat.numel() and R * C * ocap * Dl <= DST_ELEMS
    src = flat[:R * C * Fl * CAP].view(R, C, Fl, CAP)
    x = M.source(n, C, Fl, WIN, seed)
    src[..., :WIN].copy_(torch.from_numpy(x).to("cuda:0"))
    owin = min(OWIN, ocap)
    dst = torch.empty(R * C * ocap * Dl, dtype=TORCH[dtype], device="cuda:0").view(R, C, ocap, Dl)
    sent = _signed(M.sentinel(dtype), 32 if dtype == "f32" else 16)
    dst.view(INT[dtype])[:, :, :owin].fill_(sent)
    msk = torch.full((R, ocap), M.SENT_MASK, dtype=torch.uint8, device="cuda:0")
    pk = FramePack(Fl, left, right, stride, "replicate", dtype, shift=M.vector(Dl, 1), scale=M.vector(Dl, 2, True), pad=-1.0)
    try:
        _, frames, _ = pk.run(src, n, out=dst, fill_to=fill, want_mask=msk)
        torch.cuda.synchronize()
        assert pk.last_launches() == 1
        want, wmask, _ = M.rows(x, n, fill, np.full((R, C, owin, Dl), M.sentinel(dtype), M.OUT_DTYPE[dtype]), np.full((R, owin), M.SENT_MASK, np.uint8),
                                left, right, stride, M.REPLICATE, dtype, pk._shift, pk._scale, -1.0)
        got = dst.view(INT[dtype])[:, :, :owin].cpu().numpy().view(M.OUT_DTYPE[dtype])
        M.same_bits(got, want, dtype, M.sentinel(dtype))
        assert np.array_equal(msk[:, :owin].cpu().numpy(), wmask) and bool((msk[:, owin:] == M.SENT_MASK).all())
        assert np.array_equal(src[..., :WIN].cpu().numpy().view(np.uint32), x.view(np.uint32))
        # where a truncated offset of the last row, channel or line would land lie other bits
        assert not np.array_equal(x[R - 1, C - 1, Fl - 1], x[0, 0, 0]) and (R * C == 1 or not np.array_equal(want[R - 1, C - 1], want[0, 0]))
        return frames.tolist()
    finally:
        pk.close()
        del dst
        torch.cuda.empty_cache()


@pytest.mark.parametrize("dtype", ["f32", "bf16", "f16"])
def test_k_pack_past_2_to_the_32(source, dtype):
    # the crossings, in Python integers: the last row of each buffer starts past 2^32, the middle one past 2^31
    assert 2 * F * CAP > 1 << 32 and 1 << 31 < F * CAP < 1 << 32
    assert 2 * OCAP * D > 1 << 32 and 1 << 31 < OCAP * D < 1 << 32
    assert (2 * F * CAP) % (1 << 32) < WIN and (2 * OCAP * D) % (1 << 32) < OWIN * D          # where a 32-bit offset would land: row 0's windows
    frames = _case(source, (3, 1, F), OCAP, LEFT, RIGHT, STRIDE, dtype, [300, 200, 257], [110, 0, 90], 90)
    assert frames == [100, 67, 86]


# name -> (source [R][C][F], out capacity, stride)
INDEX = {
    "channels": ((1, 9, 2), OCAP, 3),
    "lines": ((1, 1, 17), 130, 3),
}


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("name", list(INDEX))
def test_k_pack_channel_and_line_past_2_to_the_32(source, name, dtype):
    """the two other indices of the layout: (row x ch + by) x F x line_el and (row x ch + by) x out_cap x D through the channel, and
    (f0 + g) x line_el through the line (17 lines: no 16-byte stores, F is no multiple of four)"""
    (R, C, Fl), ocap, stride = INDEX[name]
    Dl = (LEFT + RIGHT + 1) * Fl
    if name == "channels":                                           # the last channel starts past 2^32 in both buffers, one before past 2^31
        assert 8 * Fl * CAP > 1 << 32 and (8 * Fl * CAP) % (1 << 32) < WIN and any(1 << 31 < c * Fl * CAP < 1 << 32 for c in range(C))
        assert 8 * ocap * Dl > 1 << 32 and (8 * ocap * Dl) % (1 << 32) < OWIN * Dl and any(1 << 31 < c * ocap * Dl < 1 << 32 for c in range(C))
    else:                                                            # the last line of the source starts past 2^32
        assert 16 * CAP > 1 << 32 and (16 * CAP) % (1 << 32) < WIN and any(1 << 31 < g * CAP < 1 << 32 for g in range(Fl)) and Fl % 4
    frames = _case(source, (R, C, Fl), ocap, LEFT, RIGHT, stride, dtype, [300], [110], 91 + len(name))
    assert frames == [100]
