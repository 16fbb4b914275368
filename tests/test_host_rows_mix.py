"""lw_rows_synth_mix (stream-major rows through a channel matrix) in the host layer, CPU suite: tests/san/rows_mix_host.cpp links
the product sources, lw_rows.cpp and lw_rows_mix.cpp against the HIP stand-ins (tests/san/hip_standins.inc) under ASan / UBSan;
its own stand-in for lw_launch_rows_mix prints the matrix and the piece list the launcher was handed and checks every piece
against the source and destination sizes.  The expected mapping (destination position -> source position, channel 0 of each)
is recomputed here from the printed lw_batch_results and the places, by the rules of include/lewton_amd.h "stream-major rows";
the pieces must realise exactly that mapping, every kept position of every packet once, none longer than the piece bound.
What the kernel makes of pieces and matrix is checked on the GPU (tests/test_gpu_rows_mix.py).  The matrix helpers of
lewton_amd.rows are checked here as well: they need no GPU."""
import os
import struct

import numpy as np
import pytest

import host_harness as H
from common import ROOT, SETUPS, sg
from host_harness import CAPACITY, CS, NULL_ARG, OK, STATE_MISMATCH, UNSUPPORTED

SRC = [os.path.join(ROOT, "tests", "san", "rows_mix_host.cpp")] + [
    os.path.join(CS, n) for n in ("lw_rows.cpp", "lw_rows_mix.cpp", "lw_runtime.cpp", "lw_batch.cpp", "lw_packet.cpp", "lw_pool.cpp",
                                  "lw_dev_entropy.cpp", "lw_entropy.cpp", "lw_headers.cpp", "lw_fast.cpp")]
ALL = 0xFFFFFFFF
PIECE = 512
FMTS = {"i16": 0, "i16_interleaved": 1, "f32": 2, "f32_interleaved": 3}
SHAPES = [("stereo", "LLSSLSL"), ("surround51", "LSSL"), ("mono_small", "SLLS")]


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return H.build(tmp_path_factory, "rows_mix_host", SRC)


def _packets_file(tmp_path, setup, pattern, count, seed):
    idp, cmt, stp = setup.headers()
    pk = [bytes(p) for p in sg.make_stream(setup, pattern, count, seed=seed)]
    path = str(tmp_path / "packets.bin")
    with open(path, "wb") as f:
        for p in [idp, cmt, stp] + pk:
            f.write(struct.pack("<I", len(p)) + bytes(p))
    return path


def _run(exe, *args, **kw):
    return H.run(exe, *args, timeout=300, **kw)


def _results(lines):
    return [tuple(int(x) for x in ln.split()[1:]) for ln in lines if ln.startswith("R ")]


def _matrix_file(tmp_path, name, m, out_ch=None, in_ch=None):
    """the matrix as text, exact (hexadecimal floats); out_ch / in_ch override what the file claims"""
    m = np.asarray(m, np.float32)
    path = str(tmp_path / name)
    with open(path, "w") as f:
        f.write("%d %d\n" % (m.shape[0] if out_ch is None else out_ch, m.shape[1] if in_ch is None else in_ch))
        f.write(" ".join(float(v).hex() for v in m.reshape(-1)) + "\n")
    return path


def _bits(m):
    return np.asarray(m, np.float32).reshape(-1).view(np.uint32).tolist()


def _synth(exe, tmp_path, path, fmt, places, n_rows, cap, case, *matrices):
    """-> (return codes, launches as [(out_ch, in_ch, cap, itl, coefficient bits, pieces)], matrices as they are at the end,
    (k_rows_mix launches, k_rows launches, synthesis ran in a refused case), (segments, copied elements))"""
    pf = str(tmp_path / "places.txt")
    with open(pf, "w") as f:
        for p in places:
            f.write("%d %d %d %d\n" % p)
    out = _run(exe, path, fmt, "synth", pf, n_rows, cap, case, *matrices)
    rcs = [int(ln.split()[1]) for ln in out if ln.startswith("RC ")]
    launches = []
    for ln in out:
        v = [int(x) for x in ln.split()[1:]]
        if ln.startswith("M "):
            launches.append((v[0], v[1], v[2], v[3], v[4:], []))
        elif ln.startswith("P "):
            launches[-1][5].append(tuple(v))
    after = [[int(x) for x in ln.split()[1:]] for ln in out if ln.startswith("A")]
    counts = [tuple(int(x) for x in ln.split()[1:]) for ln in out if ln.startswith("LAUNCHES ")][0]
    intro = [tuple(int(x) for x in ln.split()[1:]) for ln in out if ln.startswith("N ")][0]
    return rcs, launches, after, counts, intro


def _expected(results, places, ch, out_ch, interleaved, cap):
    """sorted (destination element, source element, source channel stride) of channel 0 of every kept position"""
    rows = []
    for (status, m, off), (row, skip, keep, t0) in zip(results, places):
        if status != 0 or m == 0 or skip >= m:
            continue
        kept = min(keep, m - skip)
        p = np.arange(kept, dtype=np.uint64)
        if interleaved:
            dst, src, stride = (np.uint64((row * cap + t0) * out_ch) + p * np.uint64(out_ch),
                                np.uint64(off + skip * ch) + p * np.uint64(ch), 1)
        else:
            dst, src, stride = np.uint64(row * out_ch * cap + t0) + p, np.uint64(off + skip) + p, m
        rows.append(np.stack([dst, src, np.full(kept, stride, np.uint64)], 1))
    got = np.concatenate(rows) if rows else np.zeros((0, 3), np.uint64)
    return got[np.argsort(got[:, 0], kind="stable")]


def _realised(pieces, ch, out_ch, interleaved):
    rows = []
    for src, stride, count, dst in pieces:
        p = np.arange(count, dtype=np.uint64)
        rows.append(np.stack([np.uint64(dst) + p * np.uint64(out_ch if interleaved else 1),
                              np.uint64(src) + p * np.uint64(ch if interleaved else 1), np.full(count, stride, np.uint64)], 1))
    got = np.concatenate(rows) if rows else np.zeros((0, 3), np.uint64)
    return got[np.argsort(got[:, 0], kind="stable")]


def _check(launch, results, places, ch, matrix, interleaved, cap, intro):
    out_ch, in_ch, lcap, itl, bits, pieces = launch
    matrix = np.asarray(matrix, np.float32)
    assert (out_ch, in_ch, lcap, itl) == (matrix.shape[0], ch, cap, int(interleaved)) and bits == _bits(matrix)
    assert all(0 < c <= PIECE for _, _, c, _ in pieces)               # the piece bound; zero-length ones are never uploaded
    want = _expected(results, places, ch, out_ch, interleaved, cap)
    assert np.array_equal(_realised(pieces, ch, out_ch, interleaved), want)   # every kept position exactly once
    assert intro == (len(pieces), len(want) * out_ch)
    kept = [min(k, m - s) for (st, m, _), (_, s, k, _) in zip(results, places) if st == 0 and m and s < m]
    assert len(pieces) <= sum(k // PIECE + 2 for k in kept if k)       # cut into pieces, not into crumbs
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


def _routing(in_ch, out_ch):
    """a routing matrix with a silent row when there is more than one: output o <- input (o + 1) % in_ch"""
    m = np.zeros((out_ch, in_ch), np.float32)
    for o in range(out_ch):
        if o != 1:
            m[o, (o + 1) % in_ch] = 1
    return m


@pytest.mark.parametrize("fmt", list(FMTS))
@pytest.mark.parametrize("name,pattern", SHAPES)
def test_pieces_cover_every_kept_position_once(harness, tmp_path, name, pattern, fmt):
    setup = SETUPS[name]()
    ch, itl = setup.channels, "interleaved" in fmt
    path = _packets_file(tmp_path, setup, pattern, 14, 3)
    res = _results(_run(harness, path, FMTS[fmt], "results"))
    assert res[0][:2] == (0, 0) and any(m for _, m, _ in res)          # the first packet of a stream: 0 samples
    block = max(m for _, m, _ in res)
    mats = [_routing(ch, 1), _routing(ch, 3), _routing(ch, 8)]
    if fmt.startswith("f32"):
        mats += [np.full((1, ch), 1 / ch, np.float32), np.arange(5 * ch, dtype=np.float32).reshape(5, ch) - 2]
    cases = [(0, ALL), (1, 1), (5, 5), (block, 333), (block + 7, 0), (0, block + 100)]   # odd skips, a trimmed last packet
    for k, (skip, keep_last) in enumerate(cases):
        m = mats[k % len(mats)]
        places, t = _cursor_places(res, 0, skip, keep_last, start=k)   # (k: destinations of every residue)
        cap = t + 3
        rcs, launches, after, counts, intro = _synth(harness, tmp_path, path, FMTS[fmt], places, 1, cap, "ok",
                                                     _matrix_file(tmp_path, "a.txt", m))
        assert rcs == [OK] and counts[1:] == (0, 0)
        assert len(launches) == counts[0] == 1
        _check(launches[0], res, places, ch, m, itl, cap, intro)
    # one packet on its own: a skip / keep of exactly its block, of more than its block, of all but one sample
    k = max(range(len(res)), key=lambda i: res[i][1])
    for skip, keep in [(block, ALL), (block + 9, ALL), (0, block), (0, block + 9), (block - 1, ALL), (3, block - 4)]:
        places = [(0, 0, 0, 0)] * len(res)
        places[k] = (0, skip, keep, 11)
        rcs, launches, _, counts, intro = _synth(harness, tmp_path, path, FMTS[fmt], places, 1, block + 11, "ok",
                                                 _matrix_file(tmp_path, "a.txt", mats[1]))
        assert rcs == [OK] and counts[0] == len(launches) == (1 if skip < block else 0)
        if launches:
            _check(launches[0], res, places, ch, mats[1], itl, block + 11, intro)
        else:
            assert intro == (0, 0)
    # packets dealt round-robin to three rows of odd capacity, every row with its own cursor; the same call twice
    t = [0, 0, 0]
    places = []
    for i, (status, m, _) in enumerate(res):
        places.append((i % 3, 0, ALL, t[i % 3]))
        t[i % 3] += m if status == 0 else 0
    cap = max(t) | 1
    rcs, launches, after, counts, intro = _synth(harness, tmp_path, path, FMTS[fmt], places, 3, cap, "twice",
                                                 _matrix_file(tmp_path, "a.txt", mats[2]))
    assert rcs == [OK, OK] and counts == (2, 0, 0)
    _check(launches[0], res, places, ch, mats[2], itl, cap, intro)
    assert launches[1] == launches[0]                                   # idempotent: the same list again


def _refusal_setup(harness, tmp_path, fmt="f32"):
    path = _packets_file(tmp_path, SETUPS["stereo"](), "LLSL", 8, 5)
    res = _results(_run(harness, path, FMTS[fmt], "results"))
    places, t = _cursor_places(res)
    return path, res, places, t


MONO = [[0.5, 0.5]]
REFUSALS = [("null_mix", "f32", MONO, {}, NULL_ARG), ("null_coef", "f32", MONO, {}, NULL_ARG),
            ("null_rows", "f32", MONO, {}, NULL_ARG), ("null_place", "f32", MONO, {}, NULL_ARG),
            ("null_batch", "f32", MONO, {}, NULL_ARG), ("null_r", "f32", MONO, {}, NULL_ARG),
            ("other_fmt", "f32", MONO, {}, STATE_MISMATCH), ("n_short", "f32", MONO, {}, CAPACITY),
            ("refuse", "f32", MONO, {"out_ch": 0}, CAPACITY),                          # out_ch of 0 ...
            ("refuse", "f32", [[1, 0]] * 9, {}, CAPACITY),                             # ... and of 9
            ("refuse", "i16", [[1, 0]] * 9, {}, CAPACITY),
            ("refuse", "f32", [[0.5, 0.5, 0]], {}, STATE_MISMATCH),                    # in_ch 3 for a stereo decoder
            ("refuse", "f32", [[0.5, 0.5]], {"in_ch": 1}, STATE_MISMATCH),
            ("refuse", "i16", MONO, {}, UNSUPPORTED),                                  # i16 and a matrix that mixes
            ("refuse", "i16_interleaved", [[1, 0], [1, 1]], {}, UNSUPPORTED),          # two ones in a row
            ("refuse", "i16", [[0, 1], [0.5, 0]], {}, UNSUPPORTED),                    # one coefficient, but not 1.0
            ("refuse", "i16_interleaved", [[0, -1]], {}, UNSUPPORTED)]


@pytest.mark.parametrize("case,fmt,matrix,claim,code", REFUSALS)
def test_refusals_launch_nothing(harness, tmp_path, case, fmt, matrix, claim, code):
    path, res, places, t = _refusal_setup(harness, tmp_path, fmt)
    rcs, launches, _, counts, _ = _synth(harness, tmp_path, path, FMTS[fmt], places, 1, t, case,
                                         _matrix_file(tmp_path, "a.txt", matrix, **claim))
    assert rcs == [code] and launches == [] and counts == (0, 0, 0)


def test_i16_routing_and_f32_anything_are_accepted(harness, tmp_path):
    for fmt, matrix in [("i16", [[0, 1], [0, 0], [1, 0]]), ("i16_interleaved", [[-0.0, 1]]), ("f32", [[float("nan"), -3.5]]),
                        ("f32_interleaved", [[0, 0]])]:
        path, res, places, t = _refusal_setup(harness, tmp_path, fmt)
        rcs, launches, _, counts, intro = _synth(harness, tmp_path, path, FMTS[fmt], places, 1, t, "ok",
                                                 _matrix_file(tmp_path, "a.txt", matrix))
        assert rcs == [OK] and counts == (1, 0, 0)
        _check(launches[0], res, places, 2, matrix, "interleaved" in fmt, t, intro)


def test_capacity_refusals_are_decided_for_every_packet_first(harness, tmp_path):
    path, res, places, t = _refusal_setup(harness, tmp_path)
    mf = _matrix_file(tmp_path, "a.txt", MONO)
    last = len(res) - 1
    bad_row = list(places)
    bad_row[last] = (2,) + places[last][1:]                             # row == n_rows, on the LAST packet
    no_samples_bad_row = list(places)
    no_samples_bad_row[0] = (7, 0, ALL, 0)                              # the first packet (0 samples) names a row that is not there
    for pl, n_rows, cap in [(bad_row, 2, t), (places, 1, t - 1), (no_samples_bad_row, 1, t)]:
        rcs, launches, _, counts, _ = _synth(harness, tmp_path, path, 2, pl, n_rows, cap, "refuse", mf)
        assert rcs == [CAPACITY] and launches == [] and counts == (0, 0, 0)
    rcs, launches, _, _, _ = _synth(harness, tmp_path, path, 2, places, 1, t, "ok", mf)   # exactly full is accepted
    assert rcs == [OK] and launches[0][5]


def test_a_failed_k_rows_mix_launch_is_a_status_and_the_next_call_is_accepted(harness, tmp_path):
    """the launch behind the upload of pieces and matrix fails: LW_ERR_DEVICE (33), and the same call again is accepted and is
    handed its pieces and its matrix (the slot the failed call used stays marked: lewton_amd/csrc/lw_stage.hpp)"""
    path, res, places, t = _refusal_setup(harness, tmp_path)
    rcs, launches, after, counts, intro = _synth(harness, tmp_path, path, 2, places, 1, t, "fail", _matrix_file(tmp_path, "a.txt", MONO))
    assert rcs == [33, OK] and counts == (2, 0, 0) and len(launches) == 1 and after == [_bits(MONO)]
    _check(launches[0], res, places, 2, MONO, False, t, intro)


@pytest.mark.parametrize("fmt", ["f32", "f32_interleaved"])
def test_two_matrices_back_to_back_each_launch_has_its_own(harness, tmp_path, fmt):
    """matrix A, then matrix B of another out_ch without synchronising: each launcher is handed its own matrix, and A's is
    still in place when B's call has returned (the kernel reads it later); the caller's copy of A is overwritten in between"""
    path, res, places, t = _refusal_setup(harness, tmp_path, fmt)
    A, B = [[0.25, 0.75]], [[0, 1], [1, 0], [0.5, -0.5]]
    rcs, launches, after, counts, intro = _synth(harness, tmp_path, path, FMTS[fmt], places, 1, t, "two",
                                                 _matrix_file(tmp_path, "a.txt", A), _matrix_file(tmp_path, "b.txt", B))
    assert rcs == [OK, OK] and counts == (2, 0, 0)
    _check(launches[1], res, places, 2, B, "interleaved" in fmt, t, intro)
    _check(launches[0], res, places, 2, A, "interleaved" in fmt, t, (len(launches[0][5]), intro[1] // 3))
    assert after == [_bits(A), _bits(B)]
    # ... and with a lw_rows_synth call between the two
    rcs, launches, after, counts, intro = _synth(harness, tmp_path, path, FMTS[fmt], places, 1, t, "plain_between",
                                                 _matrix_file(tmp_path, "a.txt", B), _matrix_file(tmp_path, "b.txt", A))
    assert rcs == [OK, OK, OK] and counts == (2, 1, 0)
    assert [l[4] for l in launches] == [_bits(B), _bits(A)] and after == [_bits(B), _bits(A)]


def test_destination_beyond_2_to_the_32_elements(harness, tmp_path):
    """f32 planar stereo -> 3 output channels, 2 rows of 2^30 samples: row 1 starts at element 3 * 2^30 and ends beyond 2^32"""
    path = _packets_file(tmp_path, SETUPS["stereo"](), "LLSL", 8, 7)
    res = _results(_run(harness, path, 2, "results"))
    cap = 1 << 30
    total = sum(m for s, m, _ in res if s == 0)
    places, t = _cursor_places(res, row=1, start=cap - total)           # the packets end exactly at the end of row 1
    assert t == cap
    m = [[1, 0], [0, 1], [0.5, 0.5]]
    rcs, launches, _, _, intro = _synth(harness, tmp_path, path, 2, places, 2, cap, "ok", _matrix_file(tmp_path, "a.txt", m))
    assert rcs == [OK]
    _check(launches[0], res, places, 2, m, False, cap, intro)
    pieces = launches[0][5]
    assert max(d + 2 * cap + c for _, _, c, d in pieces) == 2 * 3 * cap  # the last element of the buffer, in channel 2
    assert min(d for _, _, _, d in pieces) > 3 * cap and 2 * 3 * cap > 1 << 32


def test_matrix_helpers():
    from lewton_amd import rows as R
    for n in range(1, 9):
        m = R.mix_mono(n)
        assert m.dtype == np.float32 and m.shape == (1, n) and (m == np.float32(1) / np.float32(n)).all()
    m = R.mix_select(3, [2, None, 0, 0])
    assert m.dtype == np.float32 and m.tolist() == [[0, 0, 1], [0, 0, 0], [1, 0, 0], [1, 0, 0]]
    with pytest.raises(ValueError):
        R.mix_select(2, [2])
    table = {3: (0, 2, 1), 5: (0, 2, 1, 3, 4), 6: (0, 2, 1, 5, 3, 4), 7: (0, 2, 1, 6, 5, 3, 4), 8: (0, 2, 1, 7, 5, 6, 3, 4),
             1: (0,), 2: (0, 1), 4: (0, 1, 2, 3)}
    for n, sources in table.items():
        m = R.mix_wav_order(n)
        assert m.dtype == np.float32 and m.shape == (n, n)
        want = np.zeros((n, n), np.float32)
        for o, c in enumerate(sources):
            want[o, c] = 1
        assert np.array_equal(m, want) and R.mix_is_routing(m)
    for n in (0, 9, 255):
        with pytest.raises(ValueError):
            R.mix_wav_order(n)
    assert not R.mix_is_routing(R.mix_mono(2)) and R.mix_is_routing(R.mix_mono(1))
    assert not R.mix_is_routing(np.array([[1, 1]], np.float32)) and R.mix_is_routing(np.zeros((2, 2), np.float32))
    assert R.mix_array([[1, 0]], 2).flags["C_CONTIGUOUS"] and R.mix_array(np.eye(2)[::-1], 2).dtype == np.float32
    for bad, n in [([[1, 0]], 3), ([1, 0], 2), (np.zeros((9, 2)), 2), (np.zeros((0, 2)), 2)]:
        with pytest.raises(ValueError):
            R.mix_array(bad, n)


def test_channels_refusals_need_no_gpu():
    """what decode_streams / decode_ogg_files refuse before anything is decoded"""
    from lewton_amd import header
    from lewton_amd.rows import decode_ogg_files, decode_streams
    from test_ogg import _vorbis_stream
    setup = SETUPS["stereo"]()
    idp, _, stp = setup.headers()
    ident = header.read_header_ident(idp)
    st = header.read_header_setup(stp, ident.audio_channels, (ident.blocksize_0, ident.blocksize_1))
    with pytest.raises(ValueError, match="routing"):
        decode_streams(ident, st, [[]], "i16", channels="mono")
    with pytest.raises(ValueError):
        decode_streams(ident, st, [[]], "f32", channels=[[1, 0, 0]])
    a = _vorbis_stream("stereo", "LLSL", 9, serial=0x11)[2].bytes()
    mono = _vorbis_stream("mono_small", "SLLS", 9)[2].bytes()
    with pytest.raises(ValueError, match="source 0.*routing"):
        decode_ogg_files([a, mono], "i16_interleaved", channels="mono")
    with pytest.raises(ValueError, match="source 1"):
        decode_ogg_files([a, mono], channels={2: [[1, 0], [0, 1]], 1: [[1]]})      # out_ch 2 and 1
    with pytest.raises(ValueError, match="source 1"):
        decode_ogg_files([a, mono], channels={2: [[0.5, 0.5]]})                     # no matrix for mono
    with pytest.raises(ValueError, match="source 2"):
        decode_ogg_files([a, a, mono])                                              # channels=None: as before
