"""LW_FMT_F32_INTERLEAVED (InterleavedSamples<f32>) in the host layers, CPU suite: tests/san/fmt_host.cpp links the product
sources against the HIP stand-ins (tests/san/hip_standins.inc: sample values are zero, every status, count and offset is what
the host decides) and prints a trace of one sample format.  The new format must be accepted by batch, ring, sharder, the
single-packet call and the stream calls, and decide everything exactly as f32 planar does (4-byte elements, the same element
counts, the same LW_ERR_CAPACITY thresholds, the stream's trimmed last packet); -1 and 4 stay refused.  The sample values of the
same calls are checked on the GPU (tests/test_gpu_f32_interleaved.py)."""
import os
import struct

import pytest

import host_harness as H
from common import ROOT, sg
from host_harness import CS, NULL_ARG
from test_ogg import _vorbis_stream

SRC = [os.path.join(ROOT, "tests", "san", "fmt_host.cpp")] + [
    os.path.join(CS, n) for n in ("lw_ogg.cpp", "lw_shard.cpp", "lw_ring.cpp", "lw_runtime.cpp", "lw_batch.cpp", "lw_packet.cpp",
                                  "lw_pool.cpp", "lw_dev_entropy.cpp", "lw_entropy.cpp", "lw_headers.cpp", "lw_fast.cpp")]
F32_PLANAR, F32_INTERLEAVED = 2, 3


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return H.build(tmp_path_factory, "fmt_host", SRC)


def _run(exe, path, *args):
    return H.run(exe, path, *args, timeout=300)


def _packets_file(tmp_path, setup, pattern, count, seed):
    idp, cmt, stp = setup.headers()
    pk = sg.make_stream(setup, pattern, count, seed=seed)
    path = str(tmp_path / "packets.bin")
    with open(path, "wb") as f:
        for p in [idp, cmt, stp] + pk:
            f.write(struct.pack("<I", len(p)) + bytes(p))
    return path


def _ogg_file(tmp_path, name, pattern, count, trim):
    path = str(tmp_path / ("%s.ogg" % name))
    with open(path, "wb") as f:
        f.write(_vorbis_stream(name, pattern, count, per_page=4, trim=trim)[2].bytes())
    return path


def test_format_values_accepted_and_refused(harness, tmp_path):
    path = _packets_file(tmp_path, sg.stereo_setup(), "LLSL", 6, 1)
    got = {}
    for ln in _run(harness, path, "api"):
        what, f, rc = ln.split()
        got[(what, int(f))] = int(rc)
    for what in ("batch", "ring", "sharder", "packet"):
        assert got[(what, F32_INTERLEAVED)] == 0, what
        assert got[(what, F32_INTERLEAVED)] == got[(what, F32_PLANAR)], what
        assert got[(what, -1)] == NULL_ARG and got[(what, 4)] == NULL_ARG, what


@pytest.mark.parametrize("name,pattern", [("stereo", "LLSSLSL"), ("surround51", "LSSL"), ("mono_small", "SLLS")])
def test_batch_ring_sharder_same_as_f32_planar(harness, tmp_path, name, pattern):
    from common import SETUPS
    path = _packets_file(tmp_path, SETUPS[name](), pattern, 14, 3)
    a = _run(harness, path, "batch", F32_INTERLEAVED)
    b = _run(harness, path, "batch", F32_PLANAR)
    assert a == b
    assert "B synth 0" in a and "B synth_short %d" % 34 in a      # LW_ERR_CAPACITY one element short
    assert "G submit 0" in a and "H decode 0" in a
    assert any(ln.startswith("R 0 ") and ln.split()[2] != "0" for ln in a)


@pytest.mark.parametrize("read_ahead", [0, 3])
@pytest.mark.parametrize("name,pattern,trim", [("stereo", "LLSLSSL", 333), ("surround51", "LLSSSL", 37)])
def test_stream_calls_same_as_f32_planar(harness, tmp_path, read_ahead, name, pattern, trim):
    path = _ogg_file(tmp_path, name, pattern, 30, trim)
    runs = [("seq", read_ahead), ("ahead", 4), ("skip", 700), ("skip", 5000)]
    for mode, arg in runs:
        a = _run(harness, path, mode, F32_INTERLEAVED, arg)
        b = _run(harness, path, mode, F32_PLANAR, arg)
        assert a == b, (mode, arg)
    seq = _run(harness, path, "seq", F32_INTERLEAVED, read_ahead)
    assert "C 34" in seq                                            # one element short of ch << blocksize_1: LW_ERR_CAPACITY
    counts = [int(ln.split()[1]) for ln in seq if ln.startswith("P ")]
    assert counts and counts[-1] < max(counts)                       # the trimmed last packet


def test_stream_refuses_other_values(harness, tmp_path):
    path = _ogg_file(tmp_path, "stereo", "LLSL", 8, 0)
    for f in (-1, 4):
        assert _run(harness, path, "seq", f, 0)[1:2] == ["E %d" % NULL_ARG]
        assert _run(harness, path, "ahead", f, 4) == ["E %d" % NULL_ARG]
