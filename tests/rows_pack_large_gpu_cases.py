"""k_pack past element 2^32 of its source and of its destination, on the GPU.  The cases of tests/test_gpu_rows_pack_large.py, which
runs this file with pytest in a process of its own, torch imported first (tests/rows_gpu_cases.py says why).

The kernel forms its addresses from several products (row x channel x lines x frame_capacity on the source side, row x channel x
out_capacity x D and frame x D on the destination side, row x out_capacity for the mask), in elements, and the destination's in
bytes of a dtype.  The source is viewed as [3][1][8][2^28 + 5] (a row is 2^31 + 40 elements: row 1 starts past 2^31, row 2 past
2^32; lines off the 16-byte boundaries), the destination as [3][1][2^24 + 3][128] with W = 16 (a row is 2^31 + 384 elements).  Only
windows are touched: a few hundred frames at the start of every source line and of every destination row; the work is tiny, the
offsets are huge.  Before the call every destination window and the whole mask hold a sentinel and the source holds one from each
length on; afterwards the windows equal the model bit for bit -- row 0's window is where a truncated offset of row 2 would land,
and it holds other data.  Python integers assert the crossings.  One case per dtype: the byte offsets differ.  No tolerance."""
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
    free, _ = torch.cuda.mem_get_info(0)
    need = 4 * SRC_ELEMS + 4 * DST_ELEMS + (4 << 30)
    if free < need:
        pytest.skip("less than %.1f GB of device memory free" % (need / 1e9))
    src = torch.empty(SRC_ELEMS, dtype=torch.float32, device="cuda:0").view(3, 1, F, CAP)
    yield src
    del src
    torch.cuda.empty_cache()


@pytest.mark.parametrize("dtype", ["f32", "bf16", "f16"])
def test_k_pack_past_2_to_the_32(source, dtype):
    from lewton_amd.rows import FramePack
    # the crossings, in Python integers: the last row of each buffer starts past 2^32, the middle one past 2^31
    assert 2 * F * CAP > 1 << 32 and 1 << 31 < F * CAP < 1 << 32
    assert 2 * OCAP * D > 1 << 32 and 1 << 31 < OCAP * D < 1 << 32
    assert (2 * F * CAP) % (1 << 32) < WIN and (2 * OCAP * D) % (1 << 32) < OWIN * D          # where a 32-bit offset would land: row 0's windows
    n = [300, 200, 257]
    fill = [110, 0, 90]
    x = M.source(n, 1, F, WIN, 90)
    source[..., :WIN].copy_(torch.from_numpy(x).to("cuda:0"))
    dst = torch.empty(DST_ELEMS, dtype=TORCH[dtype], device="cuda:0").view(3, 1, OCAP, D)
    sent = _signed(M.sentinel(dtype), 32 if dtype == "f32" else 16)
    dst.view(INT[dtype])[:, :, :OWIN].fill_(sent)
    msk = torch.full((3, OCAP), M.SENT_MASK, dtype=torch.uint8, device="cuda:0")
    pk = FramePack(F, LEFT, RIGHT, STRIDE, "replicate", dtype, shift=M.vector(D, 1), scale=M.vector(D, 2, True), pad=-1.0)
    try:
        _, frames, _ = pk.run(source, n, out=dst, fill_to=fill, want_mask=msk)
        torch.cuda.synchronize()
        assert frames.tolist() == [100, 67, 86] and pk.last_launches() == 1
        want, wmask, _ = M.rows(x, n, fill, np.full((3, 1, OWIN, D), M.sentinel(dtype), M.OUT_DTYPE[dtype]), np.full((3, OWIN), M.SENT_MASK, np.uint8),
                                LEFT, RIGHT, STRIDE, M.REPLICATE, dtype, pk._shift, pk._scale, -1.0)
        got = dst.view(INT[dtype])[:, :, :OWIN].cpu().numpy().view(M.OUT_DTYPE[dtype])
        M.same_bits(got, want, dtype, M.sentinel(dtype))
        assert np.array_equal(msk[:, :OWIN].cpu().numpy(), wmask) and bool((msk[:, OWIN:] == M.SENT_MASK).all())
        assert np.array_equal(source[..., :WIN].cpu().numpy().view(np.uint32), x.view(np.uint32))
    finally:
        pk.close()
        del dst
        torch.cuda.empty_cache()
