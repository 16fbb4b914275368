"""Stream-major rows through a channel matrix on the GPU: lw_rows_synth_mix / k_rows_mix (Rows.synth(mix=)), decode_streams and
decode_ogg_files with channels=.  The cases of tests/test_gpu_rows_mix.py, which runs this file with pytest in a process of its
own, torch imported first (tests/rows_gpu_cases.py says why).

The folding rule of include/lewton_amd.h is a contract on BITS, so every comparison is over EVERY element of a sentinel-filled
rows tensor, through integer views, with no tolerance (a NaN equals a NaN).  Expected rows come twice: from the same batch
through synth_to_host, folded in numpy float32 by the rule (_fold below: elementwise float32 multiply, then add, in channel
order, a coefficient 0 skipped, a coefficient 1 a copy) and placed by the same places; and from the oracle's per-packet PCM
(po.read_audio_packet, concatenated per stream), folded the same way.  The oracle's rows are decoded once per (setup, streams)
and shared."""
import torch  # noqa: F401  (first: see above)

import ctypes as C
import functools

import numpy as np
import pytest

from common import SETUPS, oracle_headers, po, sg
from rows_gpu_cases import (_assert_rows, _batches_order, _Cursor, _int_dtype, _is_f32, _itl, _new_rows_tensor, _oracle_rows,
                            _place_into, _product, _sentinel)

pytestmark = pytest.mark.gpu

S2 = 0.70710678
MATRICES = {
    "stereo": {
        "mono": [[0.5, 0.5]],
        "identity": [[1, 0], [0, 1]],
        "swap": [[0, 1], [1, 0]],
        "zero_row": [[1, 0], [0, 0], [0, 1]],                         # out_ch 3, a silent channel in the middle
        "five": [[1, 0], [0, 1], [0.5, 0.5], [-1, 1], [0, -0.0]],     # out_ch 5: copies, sums, a difference, silence
    },
    "surround51": {                                                    # Vorbis I order: FL C FR RL RR LFE
        "mono": [[1 / 6] * 6],
        "stereo": [[1, S2, 0, 0.5, 0, 0.5], [0, S2, 1, 0, 0.5, 0.5]],
        "wav": "wav",
        "front_and_lfe": [[1, 0, 0, 0, 0, 0], [0, 0, 1, 0, 0, 0], [0, 0, 0, 0, 0, 1]],
        "five": [[0, 0, 0, 0, 1, 0], [0, 0, 0, 1, 0, 0], [0, 0, 0, 0, 0, 0], [1, 0, 0, 0, 0, 0], [0, 0, 1, 0, 0, 0]],
    },
    "mono_small": {
        "identity": [[1]],
        "twice": [[1], [1]],                                           # mono -> two identical channels
        "three": [[1], [0], [0.5]],
    },
}
ROUTING = {("stereo", "identity"), ("stereo", "swap"), ("stereo", "zero_row"), ("surround51", "wav"), ("surround51", "front_and_lfe"),
           ("surround51", "five"), ("mono_small", "identity"), ("mono_small", "twice")}
PATTERNS = {"stereo": "LLSSLSL", "surround51": "LSSL", "mono_small": "SLLS"}


def _matrix(name, key):
    from lewton_amd.rows import mix_wav_order
    m = MATRICES[name][key]
    return mix_wav_order(SETUPS[name]().channels) if isinstance(m, str) else np.asarray(m, np.float32)


def _fold(matrix, x):
    """the rule of lw_rows_synth_mix in numpy: x planar [in_ch][k] (float32, or int16 for a routing matrix) -> [out_ch][k]"""
    m = np.asarray(matrix, np.float32)
    assert m.shape[1] == x.shape[0]
    out = np.zeros((m.shape[0], x.shape[1]), x.dtype)                  # no non-zero coefficient: +0.0 / 0
    for o in range(m.shape[0]):
        acc = None
        for c in range(m.shape[1]):
            k = m[o, c]
            if k == 0:
                continue
            if k == 1:
                t = x[c]                                               # the sample itself, no multiply
            else:
                assert x.dtype == np.float32
                t = k * x[c]                                           # one float32 multiply, rounded
                assert t.dtype == np.float32
            acc = t.copy() if acc is None else acc + t                 # one float32 add, rounded
        if acc is not None:
            out[o] = acc
    return out


def _streams(setup, pattern, counts, seed=0):
    return [sg.make_stream(setup, pattern, c, seed=seed + 31 * s) for s, c in enumerate(counts)]


@functools.lru_cache(maxsize=None)
def _case(name, pattern, counts, seed, f32):
    """(setup, streams, the oracle's rows) of a case: decoded once, shared by every test on the same streams, never written to"""
    setup = SETUPS[name]()
    streams = _streams(setup, pattern, list(counts), seed)
    want = _oracle_rows(setup, streams, "f32" if f32 else "i16")
    for row, _ in want:
        row.setflags(write=False)
    return setup, streams, want


def _run(case, fmt, calls, launches=2, skip=None, keep=None, cap=None, back_to_back=False, twice=False, stream=None):
    """streams -> one rows tensor per entry of `calls` (a matrix, or None for a plain lw_rows_synth), all through ONE Rows object:
    per batch, one Rows.synth per call in turn, nothing synchronised between them.  Every element of every tensor is checked
    against the oracle's rows folded by the call's matrix; unless back_to_back, behind each batch's calls the same batch goes
    through synth_to_host, and the tensors must equal its blocks folded and placed by the same places as well.  back_to_back:
    one batch object per launch and one synchronise at the very end.  Returns the expected rows (integer view) per call."""
    import torch
    from lewton_amd.batch import Batch
    from lewton_amd.rows import Rows
    setup, streams, want_rows = case
    audio, ident, st = _product(setup)
    ch = ident.audio_channels
    dec = audio.decoder_for(ident, st)
    calls = [None if m is None else np.asarray(m, np.float32) for m in calls]
    out_chs = [ch if m is None else m.shape[0] for m in calls]
    cur = _Cursor(len(streams), skip, keep)
    batches = _batches_order(streams, launches)
    max_n = max(len(b) for b in batches)
    cap = cap or -(-(max(r.shape[1] for r, _ in want_rows) + 5) // 4) * 4
    tensors = [_new_rows_tensor(fmt, len(streams), oc, cap) for oc in out_chs]
    torch.cuda.synchronize()                                                    # (the fills ran on the default stream)
    hosts = [np.full(tuple(t.shape), _sentinel(fmt), _int_dtype(fmt)) for t, _ in tensors]
    writtens = [np.zeros(tuple(t.shape), bool) for t, _ in tensors]
    pws = [audio.PreviousWindowRight() for _ in streams]
    rows = Rows(dec, max_n, fmt)
    bts = [Batch(dec, max_n, fmt) for _ in (batches if back_to_back else batches[:1])]
    hs = stream.cuda_stream if stream is not None else None
    try:
        for k, items in enumerate(batches):
            bt = bts[k if back_to_back else 0]
            res = bt.entropy([(streams[s][t], pws[s]) for s, t in items], n_threads=2)
            places = [cur.place(s, m if status == 0 else 0) for (s, t), (status, m, off) in zip(items, res)]
            for (s, t), (status, m, off) in zip(items, res):
                assert status == want_rows[s][1][t], (s, t, status)
            bt.upload(hs)
            for (tensor, _), m, oc in zip(tensors, calls, out_chs):
                for _ in range(2 if twice else 1):
                    if stream is not None:
                        with torch.cuda.stream(stream):
                            rows.synth(bt, places, tensor, mix=m)
                    else:
                        rows.synth(bt, places, tensor, mix=m)
                assert rows.last_copied_elems == sum(p[2] for p in places) * oc
            if back_to_back:
                continue
            flat = bt.synth_to_host(hs)                                         # (synchronises)
            for blk, (status, m, off), (row, sk, kp, t0) in zip(bt.split(flat, ch), res, places):
                if status == 0 and kp:
                    b2 = (blk.reshape(m, ch).T if _itl(fmt) else blk)[:, sk:sk + kp]
                    for host, written, mat in zip(hosts, writtens, calls):
                        _place_into(host, written, fmt, row, t0, b2 if mat is None else _fold(mat, b2))
        torch.cuda.synchronize()                                                # (back to back: the one synchronise)
        for bt in bts:
            assert bt.device_status() == 0
    finally:
        torch.cuda.synchronize()
        for bt in bts:
            bt.close()
        rows.close()
    wants = []
    for (tensor, iview), host, written, mat in zip(tensors, hosts, writtens, calls):
        got = iview.cpu().numpy()
        if not back_to_back:
            _assert_rows(got, host, written, fmt, "packet-major PCM of the same batches, folded")
        want = np.full(got.shape, _sentinel(fmt), got.dtype)
        wr = np.zeros(got.shape, bool)
        for s, (row, _) in enumerate(want_rows):
            sk = cur.skip[s]
            part = row[:, sk:] if cur.keep[s] is None else row[:, sk:sk + cur.keep[s]]
            assert part.shape[1] == cur.length(s)
            _place_into(want, wr, fmt, s, 0, part if mat is None else _fold(mat, part))
        if not back_to_back:
            assert np.array_equal(wr, written)
        _assert_rows(got, want, wr, fmt, "oracle, folded")
        wants.append(want[wr])
    return wants


# ---- 1. matrices x formats

MATRIX_CASES = [(name, key, fmt) for name in MATRICES for key in MATRICES[name]
                for fmt in ["f32", "f32_interleaved"] + (["i16", "i16_interleaved"] if (name, key) in ROUTING else [])]


@pytest.mark.parametrize("name,key,fmt", MATRIX_CASES)
def test_matrices_and_formats(name, key, fmt):
    """mixed short and long blocks, streams of unequal length, rows continued over 2 batches; checked batch by batch against the
    packet-major path and once more queued back to back"""
    case = _case(name, PATTERNS[name], (9, 5, 7, 6), 3, _is_f32(fmt))
    m = _matrix(name, key)
    assert ((name, key) in ROUTING) == bool(((m != 0).sum(1) <= 1).all() and ((m == 0) | (m == 1)).all())
    _run(case, fmt, [m])
    _run(case, fmt, [m], back_to_back=True)


# ---- 2. subnormals

@pytest.mark.parametrize("fmt", ["f32", "f32_interleaved"])
def test_subnormal_products_are_kept(fmt):
    """stereo -> mono with coefficients 2^-120 and 3 * 2^-121: the products are subnormal; a flush to zero or a contracted
    multiply-add is a bit difference"""
    case = _case("stereo", "LLSSLSL", (9, 5, 7, 6), 3, True)
    m = np.array([[2.0 ** -120, 3 * 2.0 ** -121]], np.float32)
    assert m[0, 0] == 2.0 ** -120 and m[0, 1] == 3 * 2.0 ** -121               # exact in float32
    want, = _run(case, fmt, [m])
    v = np.abs(want.view(np.float32))
    tiny = float(np.finfo(np.float32).tiny)
    assert int(((v > 0) & (v < tiny)).sum()) > 100, "the expected rows hold no subnormals: the case shows nothing"
    # ... and sums of two products that a fused multiply-add would round differently exist among them: here fma(k1, x1, k0 * x0)
    # is evaluated in float64 (exact product, one rounding to float32) and compared with the two-rounding rule
    rows = np.concatenate([r for r, _ in case[2]], 1)
    two = _fold(m, rows)[0]
    fused = (np.float64(m[0, 1]) * rows[1].astype(np.float64) + (m[0, 0] * rows[0]).astype(np.float64)).astype(np.float32)
    assert int((fused.view(np.int32) != two.view(np.int32)).sum()) > 0, "no sample tells a fused multiply-add from the rule"


# ---- 3. alignment

@pytest.mark.parametrize("fmt", ["f32", "f32_interleaved", "i16", "i16_interleaved"])
def test_alignment_cases(fmt):
    """stereo_6_13 (long blocks yield 4096 samples per packet: 8 pieces and more): odd skips (1, 3, 5, 7) and so odd t0 for every
    packet behind the first, a keep that ends in the middle of a packet, and rows of odd capacity (no two channels share an
    alignment) as well as of a capacity that is a multiple of 4 (16-byte stores behind unaligned loads, scalar head and tail)"""
    case = _case("stereo_6_13", "LLSLL", (7, 7, 7, 6, 5), 11, _is_f32(fmt))
    lengths = [r.shape[1] for r, _ in case[2]]
    assert max(lengths) > 4 * 4096
    skip = [1, 3, 0, 5, 7]
    keep = [None, lengths[1] - 3 - 1000, 4096 + 333, None, 1]
    mats = [[[0.5, 0.25]], [[0, 1], [1, 0], [0.75, -0.5]]] if _is_f32(fmt) else [[[0, 1]], [[0, 1], [0, 0], [1, 0]]]
    top = max(lengths)
    for cap, m in [(top | 1, mats[0]), (-(-top // 4) * 4 + 4, mats[1]), (top + 2 | 1, mats[1]), (-(-top // 4) * 4, mats[0])]:
        _run(case, fmt, [m], skip=skip, keep=keep, cap=cap)


# ---- 4. ordering and idempotence

def test_two_matrices_back_to_back():
    """per batch two calls with different matrices (and different out_ch) into two tensors, queued back to back; 5 batches without
    a synchronise (more calls than the object has descriptor slots); on torch's stream and on a side stream"""
    import torch
    for name, fmt, a, b in [("stereo", "f32", "mono", "five"), ("surround51", "f32_interleaved", "stereo", "wav"),
                            ("stereo", "i16_interleaved", "swap", "zero_row")]:
        case = _case(name, PATTERNS[name], (9, 5, 7, 6), 3, _is_f32(fmt))
        calls = [_matrix(name, a), _matrix(name, b)]
        _run(case, fmt, calls, launches=5, back_to_back=True)
        _run(case, fmt, calls, launches=5, back_to_back=True, stream=torch.cuda.Stream(device=0))
        _run(case, fmt, calls, launches=3, stream=torch.cuda.Stream(device=0))


@pytest.mark.parametrize("fmt", ["f32", "f32_interleaved", "i16"])
def test_same_call_twice_is_idempotent(fmt):
    case = _case("stereo", "LLSSLSL", (9, 5, 7, 6), 3, _is_f32(fmt))
    m = _matrix("stereo", "five" if _is_f32(fmt) else "zero_row")
    _run(case, fmt, [m], twice=True)
    _run(case, fmt, [m], twice=True, back_to_back=True)


@pytest.mark.parametrize("fmt", ["f32", "i16_interleaved"])
def test_plain_synth_between_two_mix_calls(fmt):
    """mix A, lw_rows_synth, mix B on the same object and batch: three tensors, each what its call alone gives"""
    case = _case("stereo", "LLSSLSL", (9, 5, 7, 6), 3, _is_f32(fmt))
    a, b = ("mono", "five") if _is_f32(fmt) else ("swap", "zero_row")
    calls = [_matrix("stereo", a), None, _matrix("stereo", b)]
    _run(case, fmt, calls, launches=3)
    _run(case, fmt, calls, launches=4, back_to_back=True)


# ---- 5. refusals

def test_refusals_on_the_gpu_write_nothing():
    import torch
    from lewton_amd import _native as N
    from lewton_amd.batch import Batch
    from lewton_amd.rows import Rows, places_array
    setup = SETUPS["stereo"]()
    audio, ident, st = _product(setup)
    dec = audio.decoder_for(ident, st)
    pk = sg.make_stream(setup, "LLSL", 8, seed=17)
    made = []
    for fmt in ("f32", "i16"):
        bt, rows = Batch(dec, 8, fmt), Rows(dec, 8, fmt)
        made += [bt, rows]
        pw = audio.PreviousWindowRight()
        res = bt.entropy([(p, pw) for p in pk], n_threads=1)
        bt.upload()
        cur = _Cursor(1)
        places = [cur.place(0, m) for status, m, off in res]
        total = cur.length(0)
        mono, ident2 = [[0.5, 0.5]], [[1, 0], [0, 1]]
        tensor, iv = _new_rows_tensor(fmt, 1, 1, total)
        t2, iv2 = _new_rows_tensor(fmt, 1, 2, total)
        ok_mix = mono if fmt == "f32" else [[0, 1]]
        with pytest.raises(ValueError):
            rows.synth(bt, places, tensor[:, :, :total - 1].contiguous(), mix=ok_mix)   # one sample short
        with pytest.raises(ValueError):
            rows.synth(bt, places[:-1], tensor, mix=ok_mix)
        with pytest.raises(ValueError):
            rows.synth(bt, [(1,) + p[1:] for p in places], tensor, mix=ok_mix)          # row 1 of one row
        with pytest.raises(ValueError):
            rows.synth(bt, places, t2, mix=ok_mix)                                      # two channels for out_ch 1
        with pytest.raises(ValueError):
            rows.synth(bt, places, tensor, mix=ident2)                                  # one channel for out_ch 2
        with pytest.raises(ValueError):
            rows.synth(bt, places, tensor, mix=[[0.5, 0.5, 0]])                         # in_ch 3
        with pytest.raises(ValueError):
            rows.synth(bt, places, tensor, mix=np.zeros((9, 2)))                        # out_ch 9
        if fmt == "i16":
            for bad in (mono, [[1, 1]], [[0, 0.5]]):
                with pytest.raises(ValueError):
                    rows.synth(bt, places, tensor, mix=bad)                             # i16: routing matrices only
        # below Python's own checks: the C entry point
        arr = places_array(places)
        coef = np.ones(18, np.float32)

        def c_call(out_ch, in_ch, data, mix=True):
            m = N.RowMix(out_ch, in_ch, data)
            return N.lw_rows_synth_mix(rows._h, bt._h, arr.ctypes.data_as(C.c_void_p), arr.size, C.byref(m) if mix else None,
                                       C.c_void_p(t2.data_ptr()), 1, total, None)
        data = coef.ctypes.data_as(C.c_void_p)
        assert c_call(1, 2, data, mix=False) == N.ERR_NULL_ARG and c_call(1, 2, None) == N.ERR_NULL_ARG
        assert c_call(0, 2, data) == N.ERR_CAPACITY and c_call(9, 2, data) == N.ERR_CAPACITY
        assert c_call(2, 1, data) == N.ERR_STATE_MISMATCH and c_call(2, 3, data) == N.ERR_STATE_MISMATCH
        if fmt == "i16":
            assert c_call(2, 2, data) == N.ERR_UNSUPPORTED
        torch.cuda.synchronize()
        assert bool((iv == int(_sentinel(fmt))).all()) and bool((iv2 == int(_sentinel(fmt))).all())
        rows.synth(bt, places, tensor, mix=ok_mix)                                      # exactly full is accepted
        torch.cuda.synchronize()
        assert not bool((iv == int(_sentinel(fmt))).any()) and bool((iv2 == int(_sentinel(fmt))).all())
        assert rows.last_copied_elems == total
    for x in made:
        x.close()


# ---- 6. the public functions

def _masked_equal(got, want, f32):
    same = got == want
    if f32:
        same |= np.isnan(got.view(np.float32)) & np.isnan(want.view(np.float32))
    return bool(same.all()), np.argwhere(~same)[:4].tolist()


@pytest.mark.parametrize("fmt,channels", [("f32", "mono"), ("f32_interleaved", "mono"), ("f32", "five"), ("f32_interleaved", "zero_row"),
                                          ("i16", "swap"), ("i16_interleaved", "zero_row")])
def test_decode_streams_channels(fmt, channels):
    import torch
    from lewton_amd.rows import decode_streams
    setup, streams, want_rows = _case("stereo", "LLSSLSL", (9, 5, 0, 7, 1), 21, _is_f32(fmt))
    _, ident, st = _product(setup)
    m = np.array([[0.5, 0.5]], np.float32) if channels == "mono" else _matrix("stereo", channels)
    arg = "mono" if channels == "mono" else m.tolist()
    skip, keep = [3, 0, 0, 0, 0], [None, 333, None, None, None]
    full = [r.shape[1] for r, _ in want_rows]
    want_len = [max(f - a, 0) if k is None else min(max(f - a, 0), k) for f, a, k in zip(full, skip, keep)]
    for out_extra in (None, 64):
        out = None
        if out_extra is not None:
            T = -(-max(want_len) // 64) * 64 + out_extra
            out = torch.full((5, T, len(m)) if _itl(fmt) else (5, len(m), T), 7, dtype=torch.float32 if _is_f32(fmt) else torch.int16,
                             device="cuda:0")
        pcm, lengths, errors = decode_streams(ident, st, streams, fmt, max_packets=8, run=3, skip=skip, keep=keep, out=out, channels=arg)
        assert errors == [] and lengths.tolist() == want_len and (out is None or pcm is out)
        assert tuple(pcm.shape) == ((5, pcm.shape[1], len(m)) if _itl(fmt) else (5, len(m), pcm.shape[2]))
        got = pcm.view(torch.int32 if _is_f32(fmt) else torch.int16).cpu().numpy()
        want = np.zeros(got.shape, got.dtype)                                   # zero beyond each row's length
        wr = np.zeros(got.shape, bool)
        for s, (row, _) in enumerate(want_rows):
            _place_into(want, wr, fmt, s, 0, _fold(m, row[:, skip[s]:skip[s] + want_len[s]]))
        ok, where = _masked_equal(got, want, _is_f32(fmt))
        assert ok, where
    with pytest.raises(ValueError):                                             # out= has the stream's channels, not out_ch
        decode_streams(ident, st, streams, fmt, channels=arg,
                       out=torch.zeros((5, 4096, 2) if _itl(fmt) else (5, 2, 4096), dtype=pcm.dtype, device="cuda:0")
                       if len(m) != 2 else torch.zeros((5, 4096, 3) if _itl(fmt) else (5, 3, 4096), dtype=pcm.dtype, device="cuda:0"))
    if not _is_f32(fmt):
        with pytest.raises(ValueError, match="routing"):
            decode_streams(ident, st, streams, fmt, channels="mono")


def _ogg_file(setup, pattern, count, seed, serial, per_page=4, trim=0):
    """one logical stream of `count` packets as an Ogg file (the bookkeeping of tests/test_ogg.py::_vorbis_stream, for a setup
    that is not one of SETUPS: mono at the stereo files' sample rate)"""
    from lewton_amd import ogg
    idp, cmt, stp = setup.headers()
    pk = sg.make_stream(setup, pattern, count, seed=seed)
    ident, st = oracle_headers(setup)
    w = ogg.PageWriter(serial)
    w.add_packet(idp, 0, flush=True)
    w.add_packet(cmt, 0)
    w.add_packet(stp, 0, flush=True)
    gp = 0
    for i, p in enumerate(pk):
        gp += po.get_decoded_sample_count(ident, st, p) if i else 0            # the first packet only primes the window
        last = i == len(pk) - 1
        w.add_packet(p, gp - (trim if last else 0), flush=(i % per_page == per_page - 1), eos=last)
    return w.bytes()


def _oracle_file(data, f32):
    """planar [ch][L]: the concatenation of what the oracle's OggStreamReader returns for the file"""
    from oracle import pyogg
    o, blocks = pyogg.OggStreamReader(data, "f32" if f32 else "i16"), []
    while True:
        blk = o.read_dec_packet()
        if blk is None:
            break
        blocks.append(np.asarray(blk))
    return np.concatenate(blocks, 1)


def _check_files(files, fmt, channels, matrix_of, **kw):
    import torch
    from lewton_amd.rows import decode_ogg_files
    pcm, lengths, rate = decode_ogg_files(files, fmt, channels=channels, **kw)
    got = pcm.view(torch.int32 if _is_f32(fmt) else torch.int16).cpu().numpy()
    want = np.zeros(got.shape, got.dtype)
    wr = np.zeros(got.shape, bool)
    for i, d in enumerate(files):
        row = _oracle_file(d, _is_f32(fmt))
        folded = _fold(matrix_of(row.shape[0]), row)
        assert lengths[i].item() == row.shape[1] > 0
        _place_into(want, wr, fmt, i, 0, folded)
    ok, where = _masked_equal(got, want, _is_f32(fmt))
    assert ok, where
    assert pcm.shape[1 if _itl(fmt) else 2] == -(-int(lengths.max()) // 64) * 64
    return pcm, rate


@functools.lru_cache(maxsize=None)
def _mixed_files():
    stereo, mono = SETUPS["stereo"](), sg.mono_setup(sample_rate=44100)
    return [_ogg_file(stereo, "LLSLSSL", 9, 3, 0x11, trim=333), _ogg_file(mono, "SLLS", 8, 4, 0x22, trim=37),
            _ogg_file(stereo, "LSSL", 6, 5, 0x33)]


@pytest.mark.parametrize("fmt", ["f32", "f32_interleaved"])
def test_decode_ogg_files_stereo_and_mono_to_mono(fmt):
    """a folder of stereo and mono files in one call, one tensor: what channels=None refuses"""
    from lewton_amd.rows import decode_ogg_files, mix_mono
    files = _mixed_files()
    with pytest.raises(ValueError, match="source 1"):
        decode_ogg_files(files, fmt)
    pcm, rate = _check_files(files, fmt, "mono", mix_mono, max_packets=8, run=3)
    assert rate == 44100 and tuple(pcm.shape[:1] + pcm.shape[2:] if _itl(fmt) else pcm.shape[:2]) == (3, 1)


@pytest.mark.parametrize("fmt", ["f32", "i16_interleaved"])
def test_decode_ogg_files_channels_dict_and_callable(fmt):
    """stereo stays stereo, mono goes to both channels: routing matrices, so the i16 formats take them too"""
    table = {2: np.array([[0, 1], [1, 0]], np.float32), 1: np.array([[1], [1]], np.float32)}
    _check_files(_mixed_files(), fmt, table, table.__getitem__)
    _check_files(_mixed_files(), fmt, lambda n: table[n].tolist(), table.__getitem__, max_packets=5, run=2)


def test_decode_ogg_files_wav_order_of_a_51_file():
    from lewton_amd.rows import mix_wav_order
    data = _ogg_file(SETUPS["surround51"](), "LSSL", 8, 7, 0x44, per_page=3, trim=100)
    for fmt in ("f32_interleaved", "i16"):
        pcm, rate = _check_files([data, data], fmt, "wav", mix_wav_order)
        assert rate == 48000
    row = _oracle_file(data, True)
    want = row[[0, 2, 1, 5, 3, 4]]                                              # FL FR FC LFE BL BR from FL C FR RL RR LFE
    assert np.array_equal(_fold(mix_wav_order(6), row).view(np.int32), want.view(np.int32))


def test_decode_ogg_files_channels_refusals():
    import torch
    from lewton_amd.rows import decode_ogg_files
    files = _mixed_files()
    with pytest.raises(ValueError, match="source 1"):
        decode_ogg_files(files, channels={2: [[1, 0], [0, 1]], 1: [[1]]})      # out_ch 2 and 1
    with pytest.raises(ValueError, match="source 1"):
        decode_ogg_files(files, channels={2: [[0.5, 0.5]]})                     # no matrix for mono
    with pytest.raises(ValueError, match="source 0.*routing"):
        decode_ogg_files(files, "i16", channels="mono")                         # i16 and a matrix that mixes
    with pytest.raises(ValueError, match="source 2"):
        decode_ogg_files(files[:1] + [files[0]] + [_ogg_file(sg.mono_setup(), "SLLS", 8, 4, 0x55)], channels="mono")   # 8000 Hz
    with pytest.raises(ValueError):                                             # out= is checked against out_ch
        decode_ogg_files(files, channels="mono", out=torch.zeros((3, 2, 8192), device="cuda:0"))
