"""GPU tests (-m gpu) of the pair paths of k_long (lw_kernels_long.hip, lw_long_body.inc): the shared floor indexing of a pair whose
channels use ONE staged floor (spectrum_pair_shared / floor_values_shared), the unshared form next to it, the round loop and the
textual include of the body in k_mix.  Every case decodes through Batch and compares every sample of every compared packet with
oracle.pyoracle for equality, as test_gpu_parity.py does."""
import numpy as np
import pytest

from common import oracle_headers, po, sg

pytestmark = pytest.mark.gpu

OFMT = {"i16": "i16", "f32": "f32", "i16_interleaved": "i16_itl"}


def _product(setup):
    from lewton_amd import audio, header
    idp, _, stp = setup.headers()
    ident = header.read_header_ident(idp)
    st = header.read_header_setup(stp, ident.audio_channels, (ident.blocksize_0, ident.blocksize_1))
    return audio, ident, st


def _decode(setup, streams, fmt, rounds=0):
    """all streams' packets in ONE launch, listed stream by stream; rounds: lw_debug_batch_set_rounds (0 = the planner's choice; a forced
    count also keeps the planner from spreading a small batch over the chip: 16 packets of one stream are then ONE workgroup).
    Returns ({(stream, packet): (status, samples)}, kernels of the launch)"""
    from lewton_amd.batch import Batch
    audio, ident, st = _product(setup)
    dec = audio.decoder_for(ident, st)
    pws = [audio.PreviousWindowRight() for _ in streams]
    items = [(s, t) for s in range(len(streams)) for t in range(len(streams[s]))]
    bt = Batch(dec, len(items), fmt)
    if rounds:
        bt.debug_set_rounds(rounds)
    res = bt.entropy([(streams[s][t], pws[s]) for s, t in items], n_threads=4)
    bt.upload()
    flat = bt.synth_to_host()
    kernels = bt.last_kernels
    out = {}
    for key, r, blk in zip(items, res, bt.split(flat, ident.audio_channels)):
        out[key] = (r[0], np.asarray(blk).reshape(-1))
    bt.close()
    return out, kernels


def _oracle_stream(setup, pkts, fmt):
    o_id, o_st = oracle_headers(setup)
    opw = po.Pwr()
    return [np.asarray(po.read_audio_packet(o_id, o_st, p, opw, OFMT[fmt])).reshape(-1) for p in pkts]


def _same(got, want, fmt):
    if fmt == "f32":
        return got.size == want.size and np.array_equal(got.view(np.uint32), want.view(np.uint32))
    return got.size == want.size and np.array_equal(got, want)


def _check(setup, streams, fmt, rounds=0, expect="k_long", compare=None, want_of=None):
    got, kernels = _decode(setup, streams, fmt, rounds)
    assert expect in kernels, (expect, kernels)
    checked = 0
    for s in (range(len(streams)) if compare is None else compare):
        want = want_of[s] if want_of is not None else _oracle_stream(setup, streams[s], fmt)
        for t, w in enumerate(want):
            rc, g = got[(s, t)]
            assert rc == 0, (s, t, rc)
            assert _same(g, w, fmt), (s, t, fmt)
            checked += w.size
    assert checked > 0


def _floor_flags(pkt):
    """(channel A's floor used, channel B's floor used or None when it cannot be read without decoding A's floor) of a long stereo
    packet of a two-mode setup: bit 0 packet type, bit 1 mode, bits 2-3 window flags, bit 4 A's flag, and bit 5 B's if A's is clear"""
    b = pkt[0]
    a_used = bool(b >> 4 & 1)
    return a_used, (None if a_used else bool(b >> 5 & 1))


FMTS = ["i16", "i16_interleaved", "f32"]


@pytest.mark.parametrize("rounds", [1, 0])
@pytest.mark.parametrize("fmt", FMTS)
def test_stereo_one_stream_both_paths(fmt, rounds):
    """stereo 8/11, ONE stream x 16 long packets, one staged floor shared by the channels (29 + 29 posts).  rounds = 1 (forced): one
    workgroup, waves 0-6 on the fused path, waves 7-15 floor-first.  rounds = 0: the planner's own shape for the same packets."""
    setup = sg.stereo_setup()
    _check(setup, [sg.make_stream(setup, "L", 16, seed=3)], fmt, rounds)


@pytest.mark.parametrize("seed", [11, 12, 13])
@pytest.mark.parametrize("fmt", FMTS)
def test_stereo_one_stream_unused_floors(fmt, seed):
    """the same with unused floors (audio.rs:1021-1024): one channel, the other, and both, in some packets of the workgroup -- those
    units leave the shared path for the per-channel one"""
    setup = sg.stereo_setup()
    pkts = sg.make_stream(setup, "L", 16, seed=seed, p_floor_unused=0.4)
    flags = [_floor_flags(p) for p in pkts]
    assert any(a for a, _ in flags) and any(not a and b for a, b in flags) and any(not a and b is False for a, b in flags), flags
    _check(setup, [pkts], fmt, 1)


@pytest.mark.parametrize("fmt", FMTS)
def test_surround51_two_streams(fmt):
    """5.1, 2 streams x 8 packets: three units per packet, a pair with two DIFFERENT staged floors (centre + LFE: no sharing),
    uncoupled pairs"""
    setup = sg.surround51_setup()
    streams = [sg.make_stream(setup, "L", 8, seed=5 + 31 * s, p_floor_unused=0.05) for s in range(2)]
    _check(setup, streams, fmt, 1)
    _check(setup, streams, fmt, 0)


def _stereo_40_posts():
    """stereo 8/11 whose long floor has 40 posts: more than 32, the segment tables are built one channel at a time"""
    st = sg.stereo_setup(44100, 8, 11)
    long_floor = st.mappings[st.modes[1].mapping].submap_floor[0]
    st.floors[long_floor] = sg.random_floor1(np.random.default_rng(5), st.codebooks, 11, posts=40)
    return st


@pytest.mark.parametrize("fmt", FMTS)
def test_stereo_long_floor_of_40_posts(fmt):
    setup = _stereo_40_posts()
    assert len(setup.floors[setup.mappings[setup.modes[1].mapping].submap_floor[0]].x_list) == 40
    pw = sg.RandomPacketWriter(setup, 9, p_floor_unused=0.1)   # (draws among the entries the random floor's books use)
    _check(setup, [[pw.packet(1, 1, 1) for _ in range(16)]], fmt, 1)


def test_stereo_round_loop():
    """stereo, 513 streams x 16 packets = 8208 packets: more than 16 per CU, so the planner runs several rounds per workgroup -- the
    round loop with the lane register and the spectrum registers carried from one round to the next.  Compared: streams 0, 255, 256, 512
    (five distinct packet sequences; stream s carries sequence s % 5)."""
    setup = sg.stereo_setup()
    seqs = [sg.make_stream(setup, "L", 16, seed=40 + q, p_floor_unused=0.05) for q in range(5)]
    streams = [seqs[s % 5] for s in range(513)]
    want = {s: _oracle_stream(setup, streams[s], "i16") for s in (0, 255, 256, 512)}
    _check(setup, streams, "i16", 0, compare=(0, 255, 256, 512), want_of=want)


@pytest.mark.parametrize("fmt", FMTS)
def test_mixed_stream_through_k_mix(fmt):
    """one mixed short / long stream, 64 packets: the long blocks run the body inside k_mix"""
    setup = sg.stereo_setup()
    _check(setup, [sg.make_stream(setup, "LLSSSSSSSSL", 64, seed=17, p_floor_unused=0.05)], fmt, 0, expect="k_mix")
