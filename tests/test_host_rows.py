"""lw_rows_synth (stream-major rows) in the host layer, CPU suite: tests/san/rows_host.cpp links the product sources and
lw_rows.cpp against the HIP stand-ins (tests/san/hip_standins.inc) under ASan / UBSan; its own stand-in for lw_launch_rows
prints the piece list the launcher was given and checks every piece against the source and destination sizes.  The expected
element mapping (destination element -> source element) is recomputed here from the printed lw_batch_results and the places, by
the rules of include/lewton_amd.h "stream-major rows"; the pieces must realise exactly that mapping, none longer than the
piece bound.  What the kernel makes of the list is checked on the GPU (tests/test_gpu_rows.py)."""
import os
import struct

import numpy as np
import pytest

import host_harness as H
from common import ROOT, SETUPS, sg
from host_harness import CAPACITY, CS, NULL_ARG, OK, STATE_MISMATCH

SRC = [os.path.join(ROOT, "tests", "san", "rows_host.cpp")] + [
    os.path.join(CS, n) for n in ("lw_rows.cpp", "lw_runtime.cpp", "lw_batch.cpp", "lw_packet.cpp", "lw_pool.cpp",
                                  "lw_dev_entropy.cpp", "lw_entropy.cpp", "lw_headers.cpp", "lw_fast.cpp")]
ALL = 0xFFFFFFFF
PIECE = 2048
FMTS = {"i16": 0, "i16_interleaved": 1, "f32": 2, "f32_interleaved": 3}
SHAPES = [("stereo", "LLSSLSL"), ("surround51", "LSSL"), ("mono_small", "SLLS")]


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return H.build(tmp_path_factory, "rows_host", SRC)


def _packets_file(tmp_path, setup, pattern, count, seed, damage=None):
    idp, cmt, stp = setup.headers()
    pk = [bytes(p) for p in sg.make_stream(setup, pattern, count, seed=seed)]
    if damage is not None:
        pk[damage] = b"\x01" + pk[damage][1:]        # the header flag: AudioIsHeader (audio.rs:923-925)
    path = str(tmp_path / "packets.bin")
    with open(path, "wb") as f:
        for p in [idp, cmt, stp] + pk:
            f.write(struct.pack("<I", len(p)) + bytes(p))
    return path


def _run(exe, *args, **kw):
    return H.run(exe, *args, timeout=300, **kw)


def _results(lines):
    return [tuple(int(x) for x in ln.split()[1:]) for ln in lines if ln.startswith("R ")]


def _synth(exe, tmp_path, path, fmt, places, n_rows, cap, case="ok"):
    pf = str(tmp_path / "places.txt")
    with open(pf, "w") as f:
        for p in places:
            f.write("%d %d %d %d\n" % p)
    out = _run(exe, path, fmt, "synth", pf, n_rows, cap, case)
    rcs = [int(ln.split()[1]) for ln in out if ln.startswith("RC ")]
    pieces = [tuple(int(x) for x in ln.split()[1:]) for ln in out if ln.startswith("S ")]
    launches = [tuple(int(x) for x in ln.split()[1:]) for ln in out if ln.startswith("LAUNCHES ")][0]
    intro = [tuple(int(x) for x in ln.split()[1:]) for ln in out if ln.startswith("N ")][0]
    return rcs, pieces, launches, intro


def _expected_segments(results, places, ch, interleaved, cap):
    """(src, count, dst) per segment, by the header's rules"""
    segs = []
    for (status, m, off), (row, skip, keep, t0) in zip(results, places):
        if status != 0 or m == 0 or skip >= m:
            continue
        kept = min(keep, m - skip)
        if kept == 0:
            continue
        if interleaved:
            segs.append((off + skip * ch, kept * ch, (row * cap + t0) * ch))
        else:
            segs += [(off + c * m + skip, kept, (row * ch + c) * cap + t0) for c in range(ch)]
    return segs


def _mapping(segs):
    """sorted (dst element, src element) pairs of a list of (src, count, dst)"""
    if not segs:
        return np.zeros((0, 2), np.uint64)
    dst = np.concatenate([np.arange(d, d + c, dtype=np.uint64) for s, c, d in segs])
    src = np.concatenate([np.arange(s, s + c, dtype=np.uint64) for s, c, d in segs])
    o = np.argsort(dst, kind="stable")
    return np.stack([dst[o], src[o]], 1)


def _check(pieces, results, places, ch, interleaved, cap, intro):
    want = _expected_segments(results, places, ch, interleaved, cap)
    assert all(0 < c <= PIECE for _, c, _ in pieces)                   # the piece bound; zero-length ones are never uploaded
    assert np.array_equal(_mapping(pieces), _mapping(want))
    total = sum(c for _, c, _ in want)
    assert intro == (len(pieces), total)
    assert len(pieces) <= sum(c // PIECE + 2 for _, c, _ in want)      # cut into pieces, not into crumbs
    return want


def _cursor_places(results, row=0, skip=0, keep_last=ALL, start=0):
    """one stream into one row: a leading skip spread over the first packets, a keep on the last packet with samples"""
    places, t, left = [], start, skip
    last = max([i for i, r in enumerate(results) if r[0] == 0 and r[1]], default=-1)
    for i, (status, m, _) in enumerate(results):
        if status or m == 0:
            places.append((row, 0, ALL, t))
            continue
        sk = min(left, m)
        left -= sk
        keep = keep_last if i == last else ALL
        places.append((row, sk, keep, t))
        t += min(keep, m - sk)
    return places, t


@pytest.mark.parametrize("fmt", list(FMTS))
@pytest.mark.parametrize("name,pattern", SHAPES)
def test_pieces_realise_the_places(harness, tmp_path, name, pattern, fmt):
    setup = SETUPS[name]()
    ch, itl = setup.channels, "interleaved" in fmt
    path = _packets_file(tmp_path, setup, pattern, 14, 3)
    res = _results(_run(harness, path, FMTS[fmt], "results"))
    assert res[0][:2] == (0, 0) and any(m for _, m, _ in res)          # the first packet of a stream: 0 samples
    block = max(m for _, m, _ in res)
    for skip, keep_last in [(0, ALL), (1, 1), (5, 5), (block, 333), (block + 7, 0), (0, block + 100)]:
        places, t = _cursor_places(res, 0, skip, keep_last)
        cap = t + 3
        rcs, pieces, launches, intro = _synth(harness, tmp_path, path, FMTS[fmt], places, 1, cap)
        assert rcs == [OK]
        want = _check(pieces, res, places, ch, itl, cap, intro)
        assert launches[0] == (1 if want else 0)
    # one packet on its own: a skip / keep of exactly its block, of more than its block, of all but one sample
    k = max(range(len(res)), key=lambda i: res[i][1])
    for skip, keep in [(block, ALL), (block + 9, ALL), (0, block), (0, block + 9), (block - 1, ALL), (3, block - 4)]:
        places = [(0, 0, 0, 0)] * len(res)
        places[k] = (0, skip, keep, 11)
        rcs, pieces, launches, intro = _synth(harness, tmp_path, path, FMTS[fmt], places, 1, block + 11)
        assert rcs == [OK]
        want = _check(pieces, res, places, ch, itl, block + 11, intro)
        assert bool(want) == (skip < block)
    # packets dealt round-robin to three rows of odd capacity, every row with its own cursor
    t = [0, 0, 0]
    places = []
    for i, (status, m, _) in enumerate(res):
        places.append((i % 3, 0, ALL, t[i % 3]))
        t[i % 3] += m if status == 0 else 0
    cap = max(t) | 1
    rcs, pieces, launches, intro = _synth(harness, tmp_path, path, FMTS[fmt], places, 3, cap)
    assert rcs == [OK]
    _check(pieces, res, places, ch, itl, cap, intro)
    # the same call twice: the same list again (idempotent)
    rcs, twice, launches, intro = _synth(harness, tmp_path, path, FMTS[fmt], places, 3, cap, "twice")
    assert rcs == [OK, OK] and launches[0] == 2 and twice == pieces + pieces


def test_first_and_corrupted_packets_yield_no_segment(harness, tmp_path):
    setup = SETUPS["stereo"]()
    path = _packets_file(tmp_path, setup, "LLSSLSL", 14, 3, damage=5)
    res = _results(_run(harness, path, 0, "results"))
    assert res[0][:2] == (0, 0) and res[5][0] != 0
    places, t = _cursor_places(res)
    rcs, pieces, launches, intro = _synth(harness, tmp_path, path, 0, places, 1, t)
    assert rcs == [OK]
    want = _check(pieces, res, places, 2, False, t, intro)
    assert len(want) == 2 * sum(1 for s, m, _ in res if s == 0 and m)
    # ... and they are not held against the row's capacity either: a t0 at the very end is fine for a packet without samples
    places[0] = (0, 0, ALL, t)
    places[5] = (0, 0, ALL, t)
    rcs, again, _, _ = _synth(harness, tmp_path, path, 0, places, 1, t)
    assert rcs == [OK] and again == pieces


REFUSALS = [("null_rows", NULL_ARG), ("null_place", NULL_ARG), ("null_batch", NULL_ARG), ("null_r", NULL_ARG),
            ("other_fmt", STATE_MISMATCH), ("other_decoder", STATE_MISMATCH), ("n_short", CAPACITY), ("small_max", CAPACITY)]


@pytest.mark.parametrize("case,code", REFUSALS)
def test_refusals_launch_nothing(harness, tmp_path, case, code):
    path = _packets_file(tmp_path, SETUPS["stereo"](), "LLSL", 8, 5)
    res = _results(_run(harness, path, 2, "results"))
    places, t = _cursor_places(res)
    rcs, pieces, launches, _ = _synth(harness, tmp_path, path, 2, places, 1, t, case)
    assert rcs == [code] and pieces == [] and launches == (0, 0)


def test_capacity_refusals_are_decided_for_every_packet_first(harness, tmp_path):
    path = _packets_file(tmp_path, SETUPS["stereo"](), "LLSL", 8, 5)
    res = _results(_run(harness, path, 2, "results"))
    places, t = _cursor_places(res)
    last = len(res) - 1
    bad_row = list(places)
    bad_row[last] = (2,) + places[last][1:]                             # row == n_rows, on the LAST packet
    one_short = (places, 1, t - 1)                                      # the last packet ends one sample behind the row
    no_samples_bad_row = list(places)
    no_samples_bad_row[0] = (7, 0, ALL, 0)                              # the first packet (0 samples) names a row that is not there
    for pl, n_rows, cap in [(bad_row, 2, t), one_short, (no_samples_bad_row, 1, t)]:
        rcs, pieces, launches, _ = _synth(harness, tmp_path, path, 2, pl, n_rows, cap, "refuse")
        assert rcs == [CAPACITY] and pieces == [] and launches == (0, 0)
    rcs, pieces, _, _ = _synth(harness, tmp_path, path, 2, places, 1, t)  # exactly full is accepted
    assert rcs == [OK] and pieces


def test_a_failed_k_rows_launch_is_a_status_and_the_next_call_is_accepted(harness, tmp_path):
    """the launch behind the descriptors' upload fails: LW_ERR_DEVICE (33), and the same call again is accepted and launches its
    whole list (the slot the failed call used stays marked: lewton_amd/csrc/lw_stage.hpp; tests/test_host_stage_ring.py has the
    model of what is in flight)"""
    path = _packets_file(tmp_path, SETUPS["stereo"](), "LLSL", 8, 5)
    res = _results(_run(harness, path, 2, "results"))
    places, t = _cursor_places(res)
    _, want, _, _ = _synth(harness, tmp_path, path, 2, places, 1, t)
    rcs, pieces, launches, _ = _synth(harness, tmp_path, path, 2, places, 1, t, "fail")
    assert rcs == [33, OK] and launches == (2, 0) and pieces == want and want


def test_destination_beyond_2_to_the_32_elements(harness, tmp_path):
    """i16 planar stereo, 3 rows of 2^30 samples: row 2 starts at element 2^32 of the rows buffer"""
    path = _packets_file(tmp_path, SETUPS["stereo"](), "LLSL", 8, 7)
    res = _results(_run(harness, path, 0, "results"))
    cap = 1 << 30
    total = sum(m for s, m, _ in res if s == 0)
    places, t = _cursor_places(res, row=2, start=cap - total)           # the packets end exactly at the end of row 2
    assert t == cap
    rcs, pieces, _, intro = _synth(harness, tmp_path, path, 0, places, 3, cap)
    assert rcs == [OK]
    _check(pieces, res, places, 2, False, cap, intro)
    first = [i for i, r in enumerate(res) if r[1]][0]
    want_dst = (2 * 2 + 0) * cap + places[first][3]                     # channel 0 of row 2
    assert want_dst > 1 << 32 and any(d == want_dst and s == res[first][2] for s, c, d in pieces)
    assert max(d + c for s, c, d in pieces) == 3 * 2 * cap              # the last element of the buffer
    assert min(d for s, c, d in pieces) > 1 << 32


def test_plan_places_is_the_per_row_cursor():
    """lewton_amd.rows.plan_places (the vectorised cursor of decode_streams, no GPU needed) against a packet-by-packet cursor:
    runs of several packets per stream, streams that come up several times in a batch, failed packets, skip and keep"""
    from lewton_amd import rows as R
    rng = np.random.default_rng(5)
    n_streams = 7
    skip = np.array([0, 1, 5, 700, 3000, 0, 12], np.int64)
    keep = np.array([1 << 62, 333, 1 << 62, 1, 2048, 0, 5000], np.int64)
    row_of = np.array([3, 0, 6, 1, 5, 2, 4], np.int64)
    decoded = np.zeros(n_streams, np.int64)
    pos = [0] * n_streams
    for batch in range(6):
        st_idx = np.concatenate([np.full(rng.integers(1, 5), s) for s in rng.permutation(np.r_[0:n_streams, 0:n_streams])]).astype(np.int64)
        m = rng.choice([0, 128, 576, 1024], len(st_idx)).astype(np.int64)
        want = []
        for s, k in zip(st_idx, m):
            s0, end = pos[s], min(pos[s] + k, skip[s] + keep[s])
            pos[s] += k
            lo, hi = min(max(skip[s] - s0, 0), k), min(max(end - s0, 0), k)
            want.append((row_of[s], lo, hi - lo, s0 + lo - skip[s]) if hi > lo else None)
        got = R.plan_places(st_idx, m, decoded, skip, keep, row_of)
        assert got.dtype == R.PLACE_DTYPE and got.itemsize == 24 and decoded.tolist() == pos
        for g, w in zip(got, want):
            if w is None:
                assert g["keep"] == 0
            else:
                assert (g["row"], g["skip"], g["keep"], g["t0"]) == w


def test_ogg_bookkeeping_matches_the_oracle_reader():
    """the host half of decode_ogg_files (demultiplexing, lewton's cur_absgp bookkeeping as the keep of the packet with
    last_in_stream; no GPU needed): per-packet sample counts add up to what the oracle's OggStreamReader returns"""
    from lewton_amd import header as H, rows as R
    from oracle import pyogg
    from test_ogg import _vorbis_stream
    golden = open(os.path.join(ROOT, "tests", "golden", "invalid_keypress.ogg"), "rb").read()
    files = [golden] + [_vorbis_stream(name, "LLSLSSL", 30, per_page=pp, trim=trim)[2].bytes()
                        for name, pp, trim in [("stereo", 4, 0), ("stereo_t1", 5, 37), ("surround51", 3, 333), ("stereo", 7, 5000)]]
    for i, data in enumerate(files):
        idp, stp, packets = R._read_ogg(data, "source %d" % i)
        ident = H.read_header_ident(idp)
        setup = H.read_header_setup(stp, ident.audio_channels, (ident.blocksize_0, ident.blocksize_1))
        keeps = R._ogg_keeps(ident, setup, packets, "source %d" % i)
        total = R._sample_bound(ident, setup, [p.data for p in packets], keeps)
        o, want = pyogg.OggStreamReader(data, "i16"), 0
        while True:
            blk = o.read_dec_packet()
            if blk is None:
                break
            want += np.asarray(blk).shape[1]
        assert total == want and want > 0, i
        assert set(keeps) <= {len(packets) - 1}


REFUSED = {"Resampler": dict(in_rate=2, out_rate=1, window="none"), "Spectrogram": dict(n_fft=1), "InverseSpectrogram": dict(n_fft=16, hop=17),
           "LogCompress": dict(log="log2"), "Normalize": dict(scope="frame"), "SlidingCMVN": dict(cmn_window=0), "SelectFrames": dict(device=-1),
           "EnergyVad": dict(line=-1), "Cepstrum": dict(n_in=0), "FramePack": dict(n_in=0), "KaldiFbank": dict(dither=1.0)}


@pytest.mark.parametrize("name", ["Rows"] + sorted(REFUSED))
def test_python_finaliser_after_a_refused_constructor(name):
    """an object whose constructor raised in parameter validation has no handle, and its finaliser must not raise (no GPU
    needed).  Rows validates nothing before it creates its handle: its object is one whose __init__ never ran"""
    import gc
    import sys
    from lewton_amd import rows as R
    cls = getattr(R, name)
    unraisable, hook = [], sys.unraisablehook
    sys.unraisablehook = unraisable.append                                      # (where an exception in __del__ ends up)
    try:
        obj = cls.__new__(cls)
        if name != "Rows":
            with pytest.raises(ValueError):
                obj.__init__(**REFUSED[name])                                   # this object stays, for close() below
            with pytest.raises(ValueError):
                cls(**REFUSED[name])                                            # the usual way: finalised as the exception goes
        assert getattr(obj, "_h", None) is None
        obj.close()
        del obj
        gc.collect()
    finally:
        sys.unraisablehook = hook
    assert not unraisable, [repr(u.exc_value) for u in unraisable]


def test_decode_ogg_files_refusals_need_no_gpu():
    from lewton_amd.rows import decode_ogg_files
    from lewton_amd import ogg
    from test_ogg import _vorbis_stream
    a = _vorbis_stream("stereo", "LLSL", 9, serial=0x11)[2]
    b = _vorbis_stream("stereo", "LSSL", 9, serial=0x22)[2]
    with pytest.raises(ValueError, match="source 1"):
        decode_ogg_files([a.bytes(), a.bytes() + b.bytes()])                    # chained
    with pytest.raises(ValueError, match="source 0"):
        decode_ogg_files([ogg.interleave_pages(a, b)])                          # multiplexed
    mono = _vorbis_stream("mono_small", "SLLS", 9)[2].bytes()
    with pytest.raises(ValueError, match="source 2"):
        decode_ogg_files([a.bytes(), b.bytes(), mono])
