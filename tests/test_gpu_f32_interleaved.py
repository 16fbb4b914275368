"""Interleaved f32 output (LW_FMT_F32_INTERLEAVED = InterleavedSamples<f32>, samples.rs:48-78, :86-90) on the GPU (-m gpu).

Expected samples are the oracle's f32 planar output interleaved in numpy; the comparison is bit-exact on uint32 views
(a NaN equals a NaN, see common.f32_identical).  Every batch shape is also decoded as f32 planar on the GPU: interleaved,
that must be bit-identical to the new format, and both formats must run the same kernels (Batch.last_kernels) -- a launcher
that fell back to the planar store form would write planar samples into the interleaved buffer and fail the first check."""
import numpy as np
import pytest

from common import SETUPS, oracle_headers, po, sg
from lewton_amd import inside_ogg as IO
from lewton_amd.workloads import surround51_libvorbis_coupling
from oracle import pyogg
from test_ogg import _vorbis_stream

pytestmark = pytest.mark.gpu

FMT = "f32_interleaved"


def _itl(planar):
    return np.ascontiguousarray(np.asarray(planar, np.float32).T).reshape(-1)


def _bits_equal(a, b):
    a, b = np.asarray(a, np.float32).reshape(-1), np.asarray(b, np.float32).reshape(-1)
    return a.size == b.size and bool(np.all((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))))


def _product(setup):
    from lewton_amd import audio, header
    idp, _, stp = setup.headers()
    ident = header.read_header_ident(idp)
    st = header.read_header_setup(stp, ident.audio_channels, (ident.blocksize_0, ident.blocksize_1))
    return audio, ident, st


def _uncoupled(bs0=8, bs1=11):
    st = sg.stereo_setup(44100, bs0, bs1)
    for m in st.mappings:
        m.coupling = []
    return st


def _floor_posts_beyond_the_block():
    """range bits 15: posts past the block (such floors are evaluated by k_prep, test_gpu_prep.py)"""
    st = sg.stereo_setup(44100, 8, 11)
    f = st.floors[1]
    f.rangebits = 15
    f.x_rest = list(f.x_rest[:-4]) + [5000, 20000, 31880, 131]
    return st


def _surround51_8_10():
    st = sg.surround51_setup(48000, 8, 10)
    st.floors[3].x_rest = [64, 16, 256, 128, 32, 384]   # (the generator's LFE floor has a post at x = 512, the end post for bs 10)
    return st


def _decode(setup, streams, fmt, launches=1, force_generic=False, device_entropy=False):
    """all streams' packets, stream-interleaved, in `launches` batches (the window state crosses them); returns
    (statuses, per-packet sample blocks, kernels of every launch)"""
    from lewton_amd.batch import Batch
    audio, ident, st = _product(setup)
    dec = audio.decoder_for(ident, st)
    pws = [audio.PreviousWindowRight() for _ in streams]
    order = [(s, t) for t in range(max(len(x) for x in streams)) for s in range(len(streams)) if t < len(streams[s])]
    cuts = np.linspace(0, len(order), launches + 1).astype(int)
    bt = Batch(dec, max(b - a for a, b in zip(cuts[:-1], cuts[1:])), fmt)
    if force_generic:
        bt.set_force_generic(True)
    if device_entropy:
        assert bt.set_entropy_on_device(True)
    out, kernels = {}, []
    for a, b in zip(cuts[:-1], cuts[1:]):
        items = order[a:b]
        res = bt.entropy([(streams[s][t], pws[s]) for s, t in items], n_threads=2)
        bt.upload()
        flat = bt.synth_to_host()
        kernels.append(bt.last_kernels)
        for (s, t), r, blk in zip(items, res, bt.split(flat, ident.audio_channels)):
            out[(s, t)] = (r[0], blk)
    bt.close()
    return out, kernels


def _oracle(setup, streams):
    o_id, o_st = oracle_headers(setup)
    want = {}
    for s, pk in enumerate(streams):
        opw = po.Pwr()
        for t, p in enumerate(pk):
            try:
                want[(s, t)] = (0, po.read_audio_packet(o_id, o_st, p, opw, "f32"))
            except po.OracleError as e:
                want[(s, t)] = (e.code, None)
    return want


def _check(setup, streams, launches=1, expect=None, **kw):
    got, k_itl = _decode(setup, streams, FMT, launches, **kw)
    ref, k_pl = _decode(setup, streams, "f32", launches, **kw)
    assert k_itl == k_pl, (k_itl, k_pl)
    if expect:
        assert any(expect in k for k in k_itl), (expect, k_itl)
    want = _oracle(setup, streams)
    checked = 0
    for key, (rc, w) in want.items():
        g_rc, g = got[key]
        assert g_rc == rc == ref[key][0], (key, g_rc, rc)
        if rc:
            continue
        assert g.ndim == 1 and g.size == w.size
        assert np.array_equal(g.view(np.uint32), _itl(ref[key][1]).view(np.uint32)), key   # GPU planar, interleaved
        assert _bits_equal(g, _itl(w)), key                                                  # the oracle
        checked += 1
    assert checked > 0
    return k_itl


def _streams(setup, pattern, count, n, seed=0, **kw):
    return [sg.make_stream(setup, pattern, count, seed=seed + 31 * s, **kw) for s in range(n)]


K_LONG = {
    "coupled_stereo": (lambda: sg.stereo_setup(), "L", 64, "k_long"),             # the stereo unit form
    "uncoupled_stereo": (_uncoupled, "L", 64, "k_long"),
    "surround51": (lambda: sg.surround51_setup(), "L", 24, "k_long"),
    "libvorbis_51_coupling": (surround51_libvorbis_coupling, "L", 24, "k_long"),  # PRE
    "k_prep_routed": (_floor_posts_beyond_the_block, "L", 24, "k_prep"),
    "mixed_256_2048_dense": (lambda: sg.stereo_setup(), "LLSSL", 512, "k_short"),  # k_long EDGE + k_short
    "mixed_256_2048_small": (lambda: sg.stereo_setup(), "LSSL", 2, "k_mix"),
}


@pytest.mark.parametrize("name", list(K_LONG))
def test_k_long_shapes(name):
    mk, pattern, n, kern = K_LONG[name]
    setup = mk()
    _check(setup, _streams(setup, pattern, 16, n, seed=5, p_floor_unused=0.05), expect=kern)


L10 = {
    "stereo_9_10": (lambda: sg.stereo_setup(22050, 9, 10), "L", 48, "k_long10"),
    "stereo_8_10_t1_mixed": (lambda: sg.stereo_setup(22050, 8, 10, residue_type=1), "LLSSL", 512, "k_short"),
    "stereo_8_10_mix10": (lambda: sg.stereo_setup(22050, 8, 10, residue_type=1), "LSSL", 2, "k_mix10"),
    "surround51_8_10": (_surround51_8_10, "L", 16, "k_long10"),
}


@pytest.mark.parametrize("name", list(L10))
def test_k_long10_shapes(name):
    mk, pattern, n, kern = L10[name]
    setup = mk()
    _check(setup, _streams(setup, pattern, 16, n, seed=7), expect=kern)


L12 = {
    "stereo_9_12": (lambda: sg.stereo_setup(44100, 9, 12), "L", 32, "k_long12"),
    "stereo_9_12_edge": (lambda: sg.stereo_setup(44100, 9, 12), "LLSSL", 32, "k_long12"),   # EDGE 512 / 4096
    "surround51_9_12": (lambda: sg.surround51_setup(48000, 9, 12), "L", 8, "k_long12"),
}


@pytest.mark.parametrize("name", list(L12))
def test_k_long12_shapes(name):
    mk, pattern, n, kern = L12[name]
    setup = mk()
    _check(setup, _streams(setup, pattern, 12, n, seed=9), expect=kern)


@pytest.mark.parametrize("bs0,bs1", [(8, 11), (9, 12), (10, 12)])
def test_k_short_256_512_1024(bs0, bs1):
    setup = sg.stereo_setup(44100, bs0, bs1)
    _check(setup, _streams(setup, "SSSL", 16, 512 if bs0 == 8 else 24, seed=11), expect="k_short")   # (fewer: k_mix)


def test_k_big_blocksize_13():
    setup = sg.stereo_setup(44100, 6, 13)
    _check(setup, _streams(setup, "LLSL", 8, 8, seed=13), expect="k_big")


@pytest.mark.parametrize("name", ["stereo_7_7", "mono_small"])
def test_generic_small_blocks(name):
    setup = SETUPS[name]()
    _check(setup, _streams(setup, "SLLS", 16, 8, seed=15), expect="k_ola_generic")


def test_force_generic():
    setup = sg.surround51_setup()
    _check(setup, _streams(setup, "LLSSL", 12, 6, seed=17), force_generic=True, expect="k_ola_generic")


def test_device_entropy_tier():
    setup = sg.stereo_setup()
    _check(setup, _streams(setup, "LLSL", 16, 32, seed=19), device_entropy=True, expect="k_entropy")


@pytest.mark.parametrize("name", ["stereo", "surround51", "stereo_9_12"])
def test_state_crosses_launches(name):
    setup = SETUPS[name]()
    _check(setup, _streams(setup, "LLSLSSL", 21, 12, seed=21), launches=5)


@pytest.mark.parametrize("seed", [3, 17, 40, 101, 977])
def test_random_setups(seed):
    rng = np.random.default_rng(seed)
    setup = sg.random_setup(rng)
    streams = [sg.random_stream(setup, rng, 20, seed=1000 * seed + q, p_damage=0.04) for q in range(6)]
    _check(setup, streams, launches=2)


def test_read_audio_packet_single_packets():
    setup = sg.surround51_setup()
    audio, ident, st = _product(setup)
    o_id, o_st = oracle_headers(setup)
    pw, opw = audio.PreviousWindowRight(), po.Pwr()
    pk = sg.make_stream(setup, "LLSSLSL", 14, seed=23)
    for p in pk:
        got = audio.read_audio_packet_generic(ident, st, p, pw, FMT)
        want = po.read_audio_packet(o_id, o_st, p, opw, "f32")
        assert got.dtype == np.float32 and got.ndim == 1 and _bits_equal(got, _itl(want))


def test_ring_three_slots():
    from lewton_amd.ring import Ring
    setup = sg.stereo_setup()
    audio, ident, st = _product(setup)
    o_id, o_st = oracle_headers(setup)
    dec = audio.decoder_for(ident, st)
    streams = _streams(setup, "LLSL", 12, 4, seed=25)
    ring = Ring(dec, 3, 4 * 12, FMT)
    pws = [audio.PreviousWindowRight() for _ in streams]
    ring.submit(ring.marshal([(p, pws[s]) for s in range(4) for p in streams[s]]), n_threads=1)
    res, pcm = ring.collect()
    assert pcm.dtype == np.float32
    k = 0
    for s in range(4):
        opw = po.Pwr()
        for p in streams[s]:
            want = po.read_audio_packet(o_id, o_st, p, opw, "f32")
            status, m, off = res[k]
            assert status == 0 and _bits_equal(pcm[off:off + m * 2], _itl(want)), k
            k += 1
    ring.release()
    ring.close()


def test_sharder_device_0():
    from lewton_amd.shard import Sharder
    setup = sg.surround51_setup()
    audio, ident, st = _product(setup)
    o_id, o_st = oracle_headers(setup)
    streams = _streams(setup, "LLSL", 8, 6, seed=27)
    sh = Sharder(ident, st, [0, 0], 64, FMT)
    blocks, res = sh.decode([(s, streams[s][t]) for t in range(8) for s in range(6)])
    k = 0
    opws = [po.Pwr() for _ in streams]
    for t in range(8):
        for s in range(6):
            want = po.read_audio_packet(o_id, o_st, streams[s][t], opws[s], "f32")
            assert res[k][0] == 0 and _bits_equal(blocks[k], _itl(want)), k
            k += 1
    sh.close()


def _ogg_files():
    import os
    from common import ROOT
    gold = os.path.join(ROOT, "tests", "golden")
    return [open(os.path.join(gold, n), "rb").read() for n in ("synth_stereo_mixed.ogg", "synth_surround51.ogg")] + [
        _vorbis_stream("stereo", "LLSLSSL", 40, per_page=4, trim=333)[2].bytes()]      # a trimmed last packet


@pytest.mark.parametrize("read_ahead", [0, 4])
def test_ogg_reader_generic_and_batched(read_ahead):
    for data in _ogg_files():
        s, o = IO.OggStreamReader(data), pyogg.OggStreamReader(data, "f32")
        if read_ahead:
            s.set_read_ahead(read_ahead, 2)
        n = 0
        while True:
            a, b = s.read_dec_packet_generic(FMT), o.read_dec_packet()
            assert (a is None) == (b is None), n
            if a is None:
                break
            assert a.dtype == np.float32 and _bits_equal(a, _itl(b)), n
            assert s.get_last_absgp() == o.get_last_absgp()
            n += 1
        assert n > 0
        s.close()
        s, o = IO.OggStreamReader(data), pyogg.OggStreamReader(data, "f32")
        if read_ahead:
            s.set_read_ahead(read_ahead, 2)
        while True:
            r = s.read_dec_packets(5, FMT, n_threads=2)
            if r is None:
                assert o.read_dec_packet() is None
                break
            assert r, "no chain boundary in these files"
            for a in r:
                b = o.read_dec_packet()
                assert b is not None and _bits_equal(a, _itl(b))
        s.close()


@pytest.mark.parametrize("read_ahead", [0, 4])
@pytest.mark.parametrize("to_skip", [0, 700, 5000])
def test_ogg_skip_samples_linear(read_ahead, to_skip):
    data = _vorbis_stream("stereo", "LSSLL", 30, per_page=4, trim=100)[2].bytes()
    s, o = IO.OggStreamReader(data), pyogg.OggStreamReader(data, "f32")
    if read_ahead:
        s.set_read_ahead(read_ahead, 2)
    (a, la), (b, lb) = s.skip_samples_linear(to_skip, FMT), o.skip_samples_linear(to_skip)
    assert la == lb and (a is None) == (b is None)
    if a is not None:
        assert _bits_equal(a, _itl(b))
    while True:
        a, b = s.read_dec_packet_generic(FMT), o.read_dec_packet()
        assert (a is None) == (b is None)
        if a is None:
            break
        assert _bits_equal(a, _itl(b))
    s.close()
