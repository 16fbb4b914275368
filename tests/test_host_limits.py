"""The size limits of the batch records and the state pool in the CPU suite (include/lewton_amd.h, "Limits"):
tests/san/limits_host.cpp links the PRODUCT sources against stand-ins for the HIP runtime, built with ASan + UBSan and
-DLW_CHECK_NARROW, and prints what the library says.  The expected lw_batch_max_packets comes from a model of its own: the
planner's offset expressions for the LAST packet of a batch of n worst-case packets, in Python integers, and the largest n for
which every one of them fits its 32-bit field.  Nothing sanitized is loaded into Python."""
import os
import struct

import pytest

import host_harness as H
from common import FLOOR0_SETUPS, ROOT, SETUPS, sg
from host_harness import CAPACITY as ERR_CAPACITY, CS

SRC = [os.path.join(ROOT, "tests", "san", "limits_host.cpp")] + [
    os.path.join(CS, n) for n in ("lw_shard.cpp", "lw_ring.cpp", "lw_rows.cpp", "lw_runtime.cpp", "lw_batch.cpp", "lw_packet.cpp",
                                  "lw_pool.cpp", "lw_dev_entropy.cpp", "lw_entropy.cpp", "lw_headers.cpp", "lw_fast.cpp")]
U32_MAX = (1 << 32) - 1
SIZE_MAX = (1 << 64) - 1

LIMIT_SETUPS = {
    "stereo": SETUPS["stereo"], "surround51": SETUPS["surround51"], "stereo_6_13": SETUPS["stereo_6_13"],
    "stereo_10_12": SETUPS["stereo_10_12"], "mono_small": SETUPS["mono_small"],
    "multichannel12": lambda: sg.multichannel_setup(12), "floor0": FLOOR0_SETUPS["floor0"],
}


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return H.build(tmp_path_factory, "limits_host_asan", SRC)


def model_max_packets(ch, bs0, bs1, fstride):
    """the largest n such that the offsets the planner and the kernels form for packet n - 1 of a batch of n long blocks (the
    worst case: ch * n1 / 2 residue floats, (3 n1 - n0) / 4 samples per channel each) all fit 32 bits"""
    n0, n1 = 1 << bs0, 1 << bs1
    max_m = (3 * n1 - n0) // 4

    def fits(n):
        last = n - 1
        res_off = last * ch * (n1 // 2)                       # LwPacketRec.res_off
        floor_off = last * ch * fstride                       # LwPacketRec.floor_off
        out_off = last * ch * max_m                           # LwPacketRec.out_off
        biggest = [
            res_off + (ch - 1) * (n1 // 2) + n1 // 2 - 1,     # the last residue of the last channel
            2 * res_off + (ch - 1) * n1 + n1 - 1,             # the last sample of its time-domain block (cur_off, prev_off, src_arg)
            out_off + (ch - 1) * max_m + max_m - 1,           # its last output element
            floor_off + (ch - 1) * fstride + fstride - 1,     # its last floor entry
            3 * last + 2,                                     # the padding words behind the packets in front of it (word_off)
        ]
        if bs0 in (8, 9):                                     # the raw right edge of its last channel: blocksize_0 / 4 values
            biggest.append(((2 * last + 1) * ch + ch - 1) * (n0 // 4) + n0 // 4 - 1)
        return all(v <= U32_MAX for v in biggest)

    lo, hi = 1, 1 << 33                                       # fits(lo), not fits(hi)
    assert fits(lo) and not fits(hi)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if fits(mid):
            lo = mid
        else:
            hi = mid
    return lo


def _run(harness, tmp_path, setup, with_packet=False):
    idp, _, stp = setup.headers()
    hdr = str(tmp_path / "headers.bin")
    with open(hdr, "wb") as f:
        for b in (idp, stp):
            f.write(struct.pack("<I", len(b)) + bytes(b))
    args = [harness, hdr]
    if with_packet:
        pk = sg.make_stream(setup, "L", 1, seed=3)[0]
        pkf = str(tmp_path / "packet.bin")
        with open(pkf, "wb") as f:
            f.write(struct.pack("<I", len(pk)) + bytes(pk))
        args.append(pkf)
    return [ln.split() for ln in H.run(*args, timeout=300, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))]


@pytest.mark.parametrize("name", list(LIMIT_SETUPS))
def test_batch_limit_equals_the_model_and_larger_batches_are_refused_before_any_allocation(harness, tmp_path, name):
    setup = LIMIT_SETUPS[name]()
    lines = _run(harness, tmp_path, setup)
    shape = [int(v) for v in next(ln for ln in lines if ln[0] == "SHAPE")[1:]]
    ch, bs0, bs1, fstride = shape
    assert (ch, bs0, bs1) == (setup.channels, setup.bs0, setup.bs1) and 2 <= fstride <= 66 and fstride % 2 == 0
    want = model_max_packets(ch, bs0, bs1, fstride)
    assert want == (1 << 32) // (ch << bs1)                   # (the time-domain scratch is the tightest for every setup here)
    assert int(next(ln for ln in lines if ln[0] == "MAX")[1]) == want
    refusals = [ln for ln in lines if ln[0] == "REFUSE"]
    assert sorted((ln[1], int(ln[2])) for ln in refusals) == sorted(
        (e, n) for e in ("batch", "ring", "sharder", "rows") for n in (want + 1, 2 * want, SIZE_MAX // 64))
    for _, entry, n, ptr, err, allocs in refusals:
        assert (int(ptr), int(err), int(allocs)) == (0, ERR_CAPACITY, 0), (entry, n, ptr, err, allocs)


def test_state_pool_reserve_and_slot_limit(harness, tmp_path):
    lines = _run(harness, tmp_path, LIMIT_SETUPS["stereo"](), with_packet=True)
    by = {ln[0]: ln[1:] for ln in lines}
    assert by["RESERVE_OVER"] == [str(ERR_CAPACITY), "0"]              # 2^31 slots: refused before allocating
    assert by["RESERVE"] == ["10", "0", "1"]                           # ONE allocation
    assert by["SLOTS"] == [str(k) for k in range(10)] + ["0"]          # ascending slots, the pool does not grow
    assert by["RESERVE_BELOW"] == ["0", "0"]                           # below the capacity: a no-op
    assert by["GROW"][0] == "10" and int(by["GROW"][1]) == 1           # the eleventh handle grows the pool, once
    # device entropy stage: six packets of "3 GiB" pass the 32-bit word offsets of the packet pool; refused, nothing allocated
    assert by["POOL_SMALL"] == ["0"]
    assert by["POOL"] == [str(ERR_CAPACITY), "0"]
