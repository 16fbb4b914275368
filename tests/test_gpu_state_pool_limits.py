"""Streams whose window state lies beyond element 2^32 of the decoder's state pool (-m gpu), every packet against the ORACLE.

The state pool is [slots][2][ch][n1 / 2] floats.  A reader that forms `(2 slot + parity) * ch * n1 / 2` in 32 bits reads the state
of ANOTHER stream once that product reaches 2^32: slot 2^20 aliases slot 0 for stereo 256/2048, slot 2^19 for stereo 1024/4096.
The pool is therefore reserved at 2^32 floats plus eight slots (16 GiB; lw_decoder_reserve_streams, one allocation), four live
streams sit in slots 0..3 and four in the slots from the alias slot upwards, each with its own seed: a truncated read finds a
different live stream's state, in bounds, and the comparison fails.  Only the eight live slots are ever touched.

Which kernel reads the pool, per case (asserted from lw_batch_last_kernels, so that no case is vacuous):

* stereo 256/2048, default path: k_long reads a long block's predecessor, the short role of k_mix (or k_short<16>) a short block's
  and the LW_SS_EDGE slot of a long block with a short left slope;
* stereo 1024/4096, default path: k_long12 for (long, long, long) windows, k_short<32> for the short blocks, and -- the pair has
  no edge form -- k_ola_generic through its packed descriptors (LwOlaDesc) for every long block next to a short one;
* forced generic: k_ola_generic through the packet records.  That reader has always formed the address in size_t, so this case
  was green before the fix as well; the descriptor path of k_ola_generic is reached by the 1024/4096 default case only.

Every cut of the pattern "LLSSLSL" (nine packets: all four predecessor / successor pairs) starts a launch whose first packets read
the pool; the one-packet-per-stream-per-launch run does so for every packet."""
import ctypes as C
import time

import numpy as np
import pytest

from common import SETUPS, oracle_headers, po, sg

pytestmark = pytest.mark.gpu

PATTERN, N_PACKETS, N_STREAMS = "LLSSLSL", 9, 8
CASES = {"stereo": 1 << 20, "stereo_10_12": 1 << 19}   # setup -> the slot whose state starts at float 2^32 of the pool
OFMT = {"i16": "i16", "f32": "f32"}


def _product(setup):
    from lewton_amd import audio, header
    idp, _, stp = setup.headers()
    ident = header.read_header_ident(idp)
    st = header.read_header_setup(stp, ident.audio_channels, (ident.blocksize_0, ident.blocksize_1))
    return audio, ident, st


class _Pool:
    pass


@pytest.fixture(scope="module", params=list(CASES))
def pool(request):
    """One decoder per setup (the first is destroyed before the second is made), its pool reserved in one allocation, a handle
    in every slot up to the last live one, and the oracle's packets and final states of the eight streams."""
    from lewton_amd import _native as N
    name, alias = request.param, CASES[request.param]
    setup = SETUPS[name]()
    audio, ident, st = _product(setup)
    ch = setup.channels
    assert 2 * alias * ch * (1 << setup.bs1) // 2 == 1 << 32          # state of slot `alias` starts at float 2^32
    dec = audio.Decoder(ident, st, 0)
    t0 = time.perf_counter()
    rc = N.lw_decoder_reserve_streams(dec._h, alias + N_STREAMS)
    t_reserve = time.perf_counter() - t0
    if rc == N.ERR_DEVICE:
        dec.close()
        pytest.skip("less than 16 GiB of device memory free")
    assert rc == 0, rc
    assert N.lw_decoder_reserve_streams(dec._h, 5) == 0                # below the capacity: a no-op
    t0 = time.perf_counter()
    handles = [N.lw_pwr_new(dec._h) for _ in range(alias + N_STREAMS // 2)]   # slots come in ascending order from a fresh pool
    t_loop = time.perf_counter() - t0
    assert all(handles[-8:]) and all(handles[:8])
    slots = [0, 1, 2, 3, alias, alias + 1, alias + 2, alias + 3]
    for s in slots:
        assert N.lw_debug_pwr_slot(handles[s]) == s
    P = _Pool()
    P.name, P.setup, P.audio, P.dec, P.ch, P.slots, P.alias = name, setup, audio, dec, ch, slots, alias
    P.handles = handles
    P.pwrs = [audio.PreviousWindowRight(dec, handles[s]) for s in slots]
    P.packets = [sg.make_stream(setup, PATTERN, N_PACKETS, seed=500 + 17 * k) for k in range(N_STREAMS)]
    o_id, o_st = oracle_headers(setup)
    P.want, P.want_state = {}, {}
    for fmt in OFMT:
        P.want[fmt], P.want_state[fmt] = [], []
        for k in range(N_STREAMS):
            opw = po.Pwr()
            P.want[fmt].append([np.asarray(po.read_audio_packet(o_id, o_st, p, opw, OFMT[fmt])) for p in P.packets[k]])
            P.want_state[fmt].append(opw.data(ch))
    print("\n[%s] reserve %d slots: %.3f s; %d x lw_pwr_new: %.3f s" % (name, alias + N_STREAMS, t_reserve, len(handles), t_loop))
    yield P
    for pw in P.pwrs:
        pw._h = None                                                   # (freed with the others below)
    t0 = time.perf_counter()
    for h in handles:
        N.lw_pwr_free(h)
    print("\n[%s] %d x lw_pwr_free: %.3f s" % (name, len(handles), time.perf_counter() - t0))
    dec.close()


def _same(got, want, fmt):
    got, want = np.asarray(got).reshape(-1), np.asarray(want).reshape(-1)
    if got.size != want.size:
        return False
    return np.array_equal(got.view(np.uint32), want.view(np.uint32)) if fmt == "f32" else np.array_equal(got, want)


def _launch(P, bt, fmt, first, last, bad):
    """packets [first, last) of every stream, stream-major, in one launch; the packets that differ from the oracle go to `bad`"""
    items = [(P.packets[k][t], P.pwrs[k]) for k in range(N_STREAMS) for t in range(first, last)]
    res = bt.entropy(items, n_threads=2)
    bt.upload()
    got = bt.split(bt.synth_to_host(), P.ch)
    assert bt.device_status() == 0
    i = 0
    for k in range(N_STREAMS):
        for t in range(first, last):
            assert res[i][0] == 0, (k, t, res[i])
            if not _same(got[i], P.want[fmt][k][t], fmt):
                bad.append((P.slots[k], t))
            i += 1
    return bt.last_kernels


def _check_states(P, fmt, bad):
    from lewton_amd import _native as N
    for k in range(N_STREAMS):
        stt = N.PwrState()
        N.lw_pwr_get_state(P.pwrs[k]._h, C.byref(stt))
        want = P.want_state[fmt][k]
        assert stt.present == 1 and stt.len == want.shape[1], (k, stt.present, stt.len)
        if not np.array_equal(P.pwrs[k].data().view(np.uint32), want.view(np.uint32)):
            bad.append((P.slots[k], "state"))


@pytest.mark.parametrize("fmt", ["i16", "f32"])
@pytest.mark.parametrize("path", ["default", "generic", "device_entropy"])
def test_streams_beyond_2_to_the_32_floats_of_the_state_pool(pool, path, fmt):
    """Two launches cut after packet k, for every k (k = 8: one launch), then one packet per stream per launch; every packet and
    the final state of all eight streams against the oracle, and the kernels that read the pool named by the launches."""
    from lewton_amd.batch import Batch
    P = pool
    bt = Batch(P.dec, N_STREAMS * N_PACKETS, fmt)
    if path == "generic":
        bt.set_force_generic(True)
    if path == "device_entropy":
        assert bt.set_entropy_on_device(True)
    bad, from_pool = [], []          # from_pool: the kernels of the launches whose first packets read the state pool
    t0 = time.perf_counter()
    for cut in range(N_PACKETS):
        for pw in P.pwrs:
            pw.reset()
        here = []
        _launch(P, bt, fmt, 0, cut + 1, here)
        if cut + 1 < N_PACKETS:
            from_pool.append(_launch(P, bt, fmt, cut + 1, N_PACKETS, here))
        _check_states(P, fmt, here)
        bad += [("cut", cut) + b for b in here]
    for pw in P.pwrs:
        pw.reset()
    here = []
    for t in range(N_PACKETS):
        k = _launch(P, bt, fmt, t, t + 1, here)
        if t:
            from_pool.append(k)
    _check_states(P, fmt, here)
    bad += [("step",) + b for b in here]
    bt.close()
    print("\n[%s %s %s] %.3f s; kernels of the launches that read the pool: %s" %
          (P.name, path, fmt, time.perf_counter() - t0, sorted(set(from_pool))))
    names = set(n for k in from_pool for n in k.split(","))
    if path == "generic":
        assert "k_ola_generic" in names and not names & {"k_short", "k_mix", "k_long", "k_long12"}
    elif P.name == "stereo":
        assert names & {"k_short", "k_mix"}
    else:
        assert "k_ola_generic" in names and names & {"k_short", "k_long10", "k_long12"}
    if path == "device_entropy":
        assert "k_entropy" in names
    low = [b for b in bad if b[-2] < P.alias]
    assert not bad, "%d wrong results, %d of them in slots 0..3; first: %s" % (len(bad), len(low), bad[:12])
