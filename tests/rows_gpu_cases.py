"""Stream-major rows on the GPU: lw_rows_synth / k_rows (lewton_amd.rows.Rows), decode_streams, decode_ogg_files.  The cases of
tests/test_gpu_rows.py, which runs this file with pytest in a process of its own: torch brings its own copy of the HIP runtime,
and a process that hands torch tensors and streams to the library must have loaded torch BEFORE the library (lewton_amd/rows.py)
-- in the suite's own process the modules collected earlier have loaded the library already.  Hence `import torch` first.

The assembler moves bits, so every comparison is over EVERY element of the rows tensor, through integer views, with no
tolerance.  Before each call the tensor is filled with a sentinel (0x5A5A / the bit pattern 0x7FC0DEAD); everything outside the
ranges the places name must still hold it afterwards.  Expected rows come twice: from the same batch through synth_to_host,
re-assembled in numpy by the same places (bit-identical everywhere), and from the oracle (po.read_audio_packet per packet,
concatenated per stream; bit-exact, a NaN equals a NaN as in tests/test_gpu_f32_interleaved.py)."""
import torch  # noqa: F401  (first: see above)

import os

import numpy as np
import pytest

from common import ROOT, SETUPS, oracle_headers, po, sg
from test_ogg import _vorbis_stream

pytestmark = pytest.mark.gpu

ALL = 0xFFFFFFFF
FMTS = ["i16", "i16_interleaved", "f32", "f32_interleaved"]
SENTINEL = {2: 0x5A5A, 4: 0x7FC0DEAD}


def _product(setup):
    from lewton_amd import audio, header
    idp, _, stp = setup.headers()
    ident = header.read_header_ident(idp)
    st = header.read_header_setup(stp, ident.audio_channels, (ident.blocksize_0, ident.blocksize_1))
    return audio, ident, st


def _is_f32(fmt):
    return fmt.startswith("f32")


def _itl(fmt):
    return fmt.endswith("interleaved")


def _int_dtype(fmt):
    return np.int32 if _is_f32(fmt) else np.int16


def _sentinel(fmt):
    return np.array(SENTINEL[4 if _is_f32(fmt) else 2]).astype(np.uint32 if _is_f32(fmt) else np.uint16).view(_int_dtype(fmt))[()]


def _new_rows_tensor(fmt, n_rows, ch, cap):
    """a torch rows tensor filled with the sentinel, and its integer view"""
    import torch
    shape = (n_rows, cap, ch) if _itl(fmt) else (n_rows, ch, cap)
    t = torch.empty(shape, dtype=torch.float32 if _is_f32(fmt) else torch.int16, device="cuda:0")
    iv = t.view(torch.int32 if _is_f32(fmt) else torch.int16)
    iv.fill_(int(_sentinel(fmt)))
    return t, iv


def _oracle_rows(setup, streams, fmt):
    """per stream: ([ch][L] planar samples of the whole stream as the oracle decodes it, statuses per packet)"""
    o_id, o_st = oracle_headers(setup)
    out = []
    for pk in streams:
        opw, blocks, status = po.Pwr(), [], []
        for p in pk:
            try:
                blocks.append(np.asarray(po.read_audio_packet(o_id, o_st, p, opw, "f32" if _is_f32(fmt) else "i16")))
                status.append(0)
            except po.OracleError as e:
                status.append(e.code)
        ch = setup.channels
        row = np.concatenate(blocks, 1) if blocks else np.zeros((ch, 0), np.float32 if _is_f32(fmt) else np.int16)
        out.append((row, status))
    return out


def _place_into(dst, written, fmt, row, t0, block):
    """block: planar [ch][k] -> the row of a host rows array (integer view) at t0"""
    k = block.shape[1]
    bits = np.ascontiguousarray(block).view(_int_dtype(fmt))
    if _itl(fmt):
        dst[row, t0:t0 + k, :] = bits.T
        written[row, t0:t0 + k, :] = True
    else:
        dst[row, :, t0:t0 + k] = bits
        written[row, :, t0:t0 + k] = True


def _assert_rows(got, want, written, fmt, what):
    """every element: the sentinel outside the written ranges, the expected bits inside (a NaN equals a NaN)"""
    assert got.shape == want.shape
    outside = ~written
    assert np.array_equal(got[outside], np.full(int(outside.sum()), _sentinel(fmt), got.dtype)), what + ": written outside the ranges"
    same = got == want
    if _is_f32(fmt):
        same |= np.isnan(got.view(np.float32)) & np.isnan(want.view(np.float32)) & written
    assert bool(same.all()), (what, int((~same).sum()), np.argwhere(~same)[:4].tolist())


def _batches_order(streams, launches, run=3):
    """(stream, packet) in submission order: `run` consecutive packets of each stream in turn, cut into `launches` batches"""
    order, pos = [], [0] * len(streams)
    while any(pos[s] < len(streams[s]) for s in range(len(streams))):
        for s in range(len(streams)):
            take = min(run, len(streams[s]) - pos[s])
            order += [(s, pos[s] + j) for j in range(take)]
            pos[s] += take
    cuts = np.linspace(0, len(order), launches + 1).astype(int)
    return [order[a:b] for a, b in zip(cuts[:-1], cuts[1:]) if b > a]


class _Cursor:
    """the caller's bookkeeping: per row, samples decoded so far; a stream-level skip and a cap on the row's length"""

    def __init__(self, n, skip=None, keep=None):
        self.pos = [0] * n
        self.skip = skip or [0] * n
        self.keep = keep or [None] * n

    def place(self, s, m):
        """(row, skip, keep, t0) of the next packet of stream s with m samples"""
        s0 = self.pos[s]
        self.pos[s] += m
        end = s0 + m if self.keep[s] is None else min(s0 + m, self.skip[s] + self.keep[s])
        lo = min(max(self.skip[s] - s0, 0), m)
        hi = min(max(end - s0, 0), m)
        if hi <= lo:
            return (s, 0, 0, 0)
        return (s, lo, hi - lo, s0 + lo - self.skip[s])

    def length(self, s):
        n = max(self.pos[s] - self.skip[s], 0)
        return n if self.keep[s] is None else min(n, self.keep[s])


def _run(setup, streams, fmt, launches=1, device_entropy=False, skip=None, keep=None, cap=None, back_to_back=False,
         twice=False, stream=None):
    """streams -> a rows tensor through Rows.synth, every element checked against the oracle.  Default: one batch object; behind
    each Rows.synth the same batch goes through synth_to_host (an idempotent re-launch, which synchronises), must name the same
    kernels, and is re-assembled in numpy by the same places: the tensor must equal that bit for bit as well.  back_to_back: one
    batch object per launch, everything queued without synchronising in between, one synchronise at the end."""
    import torch
    from lewton_amd.batch import Batch
    from lewton_amd.rows import Rows
    audio, ident, st = _product(setup)
    ch = ident.audio_channels
    dec = audio.decoder_for(ident, st)
    want_rows = _oracle_rows(setup, streams, fmt)
    cur = _Cursor(len(streams), skip, keep)
    batches = _batches_order(streams, launches)
    max_n = max(len(b) for b in batches)
    cap = cap or max(r.shape[1] for r, _ in want_rows) + 5
    tensor, iview = _new_rows_tensor(fmt, len(streams), ch, cap)
    torch.cuda.synchronize()                                                    # (the fill ran on the default stream)
    host = np.full(tuple(tensor.shape), _sentinel(fmt), _int_dtype(fmt))        # the packet-major path, re-assembled
    written = np.zeros(tuple(tensor.shape), bool)
    pws = [audio.PreviousWindowRight() for _ in streams]
    rows = Rows(dec, max_n, fmt)
    bts = [Batch(dec, max_n, fmt) for _ in (batches if back_to_back else batches[:1])]
    hs = stream.cuda_stream if stream is not None else None
    try:
        for k, items in enumerate(batches):
            bt = bts[k if back_to_back else 0]
            if device_entropy:
                assert bt.set_entropy_on_device(True)
            res = bt.entropy([(streams[s][t], pws[s]) for s, t in items], n_threads=2)
            places = [cur.place(s, m if status == 0 else 0) for (s, t), (status, m, off) in zip(items, res)]
            for (s, t), (status, m, off) in zip(items, res):
                assert status == want_rows[s][1][t], (s, t, status)
            bt.upload(hs)
            for _ in range(2 if twice else 1):
                if stream is not None:
                    with torch.cuda.stream(stream):
                        rows.synth(bt, places, tensor)
                else:
                    rows.synth(bt, places, tensor)
            assert rows.last_copied_elems == sum(p[2] for p in places) * ch
            if back_to_back:
                continue
            kernels = bt.last_kernels
            flat = bt.synth_to_host(hs)
            assert bt.last_kernels == kernels, (bt.last_kernels, kernels)       # the synthesis path was not altered
            for blk, (status, m, off), (row, sk, kp, t0) in zip(bt.split(flat, ch), res, places):
                if status == 0 and kp:
                    b2 = blk.reshape(m, ch).T if _itl(fmt) else blk
                    _place_into(host, written, fmt, row, t0, b2[:, sk:sk + kp])
        torch.cuda.synchronize()                                                # (back to back: the one synchronise)
        for bt in bts:
            assert bt.device_status() == 0
    finally:
        torch.cuda.synchronize()
        for bt in bts:
            bt.close()
        rows.close()
    got = iview.cpu().numpy()
    if not back_to_back:
        assert np.array_equal(got, host), "rows differ from the packet-major PCM of the same batches"
    # the oracle: the whole stream, skip / keep applied to the concatenation
    want = np.full(got.shape, _sentinel(fmt), got.dtype)
    wr = np.zeros(got.shape, bool)
    for s, (row, _) in enumerate(want_rows):
        sk = cur.skip[s]
        part = row[:, sk:] if cur.keep[s] is None else row[:, sk:sk + cur.keep[s]]
        assert part.shape[1] == cur.length(s)
        _place_into(want, wr, fmt, s, 0, part)
    if not back_to_back:
        assert np.array_equal(wr, written)
    _assert_rows(got, want, wr, fmt, "oracle")
    return got


def _run_both(setup, streams, fmt, launches, **kw):
    """both forms: checked against the packet-major path batch by batch, and queued back to back"""
    _run(setup, streams, fmt, launches, back_to_back=True, **kw)
    return _run(setup, streams, fmt, launches, **kw)


def _streams(setup, pattern, counts, seed=0, **kw):
    return [sg.make_stream(setup, pattern, c, seed=seed + 31 * s, **kw) for s, c in enumerate(counts)]


SHAPES = ["stereo", "stereo_t1", "surround51", "mono_small", "stereo_9_12", "stereo_6_13", "stereo_8_10", "stereo_10_12"]


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("name", SHAPES)
def test_rows_equal_packet_major_and_oracle(name, fmt):
    """long, short and transition blocks; streams of unequal length; several packets of a row per batch; rows continued over
    3 batches; the kernels of the synthesis path unchanged"""
    setup = SETUPS[name]()
    _run_both(setup, _streams(setup, "LLSSLSL", [21, 9, 14, 17, 5], seed=3), fmt, 3)


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("name,pattern", [("stereo", "L"), ("stereo", "S"), ("surround51", "LSSL")])
def test_rows_single_launch_patterns(name, pattern, fmt):
    setup = SETUPS[name]()
    _run_both(setup, _streams(setup, pattern, [12, 7, 16], seed=5), fmt, 1)


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("name", ["stereo", "surround51"])
def test_rows_device_entropy(name, fmt):
    setup = SETUPS[name]()
    got = _run_both(setup, _streams(setup, "LLSL", [16, 11, 13, 16], seed=7), fmt, 3, device_entropy=True)
    assert got.size


@pytest.mark.parametrize("fmt", FMTS)
def test_rows_damaged_packets(fmt):
    """a packet that fails adds nothing to its row and nothing is written for it"""
    setup = SETUPS["stereo"]()
    streams = _streams(setup, "LLSSLSL", [14, 14, 9], seed=9)
    streams[1][6] = b"\x01" + bytes(streams[1][6])[1:]       # AudioIsHeader
    streams[2][0] = b""                                       # the priming packet itself fails: the next one primes
    _run_both(setup, streams, fmt, 2)


ALIGN = [("stereo", "i16"), ("stereo", "f32"), ("surround51", "i16_interleaved"), ("surround51", "f32_interleaved"),
         ("surround51", "i16"), ("stereo", "i16_interleaved"), ("stereo", "f32_interleaved"), ("mono_small", "f32")]


@pytest.mark.parametrize("name,fmt", ALIGN)
def test_alignment_cases(name, fmt):
    """a leading skip of 1, 3, 5, 7, 9 samples on the first kept packet, the last packet trimmed to 333 samples and to 1, rows of
    odd capacity: source and destination of a piece in every pair of residues mod 16 bytes"""
    setup = SETUPS[name]()
    streams = _streams(setup, "LLSLL", [12, 12, 12, 12, 12, 12, 12], seed=11)
    lengths = [r.shape[1] for r, _ in _oracle_rows(setup, streams, fmt)]
    last = [np.asarray(_oracle_rows(setup, [s[-2:]], fmt)[0][0]).shape[1] for s in streams]   # samples of each last packet
    skip = [1, 3, 5, 7, 9, 0, 2]
    trim = [None, None, 333, 1, None, 333, 1]                 # what the last packet keeps
    keep = [None if t is None else lengths[s] - last[s] + min(t, last[s]) - skip[s] for s, t in enumerate(trim)]
    for k in (1, 2):
        cap = 1021 * (max(lengths) // 1021 + k) + 1
        _run_both(setup, streams, fmt, 2, skip=skip, keep=keep, cap=cap)
    # a skip of more than the first packets of a row, a keep that ends inside an earlier batch
    big = max(last)
    _run_both(setup, streams, fmt, 3, skip=[big + 5, 2 * big + 1, 0, 7, big, 3, 1], keep=[None, 100, 3 * big + 3, None, 1, big, None])


def test_back_to_back_on_a_side_stream():
    """five batches queued on one non-default stream without synchronising in between (more calls than the object has
    descriptor slots), one synchronise at the end"""
    import torch
    setup = SETUPS["stereo"]()
    streams = _streams(setup, "LLSSLSL", [25, 25, 18, 25], seed=13)
    for fmt in ("f32", "i16_interleaved"):
        _run(setup, streams, fmt, 5, back_to_back=True, stream=torch.cuda.Stream(device=0))
        _run(setup, streams, fmt, 5, back_to_back=True)                         # ... and on the default stream
        _run(setup, streams, fmt, 5, stream=torch.cuda.Stream(device=0))


@pytest.mark.parametrize("fmt", ["i16", "f32_interleaved"])
def test_same_call_twice_is_idempotent(fmt):
    setup = SETUPS["stereo"]()
    _run_both(setup, _streams(setup, "LLSL", [12, 9, 12], seed=15), fmt, 2, twice=True)


def test_refusals_on_the_gpu_write_nothing():
    import torch
    from lewton_amd.batch import Batch
    from lewton_amd.rows import Rows
    setup = SETUPS["stereo"]()
    audio, ident, st = _product(setup)
    dec = audio.decoder_for(ident, st)
    pk = sg.make_stream(setup, "LLSL", 8, seed=17)
    bt, rows = Batch(dec, 8, "f32"), Rows(dec, 8, "f32")
    pw = audio.PreviousWindowRight()
    res = bt.entropy([(p, pw) for p in pk], n_threads=1)
    bt.upload()
    cur = _Cursor(1)
    places = [cur.place(0, m) for status, m, off in res]
    total = cur.length(0)
    tensor, iv = _new_rows_tensor("f32", 1, 2, total)
    with pytest.raises(ValueError):
        rows.synth(bt, places, tensor[:, :, :total - 1].contiguous())          # one sample short
    with pytest.raises(ValueError):
        rows.synth(bt, places[:-1], tensor)
    with pytest.raises(ValueError):
        rows.synth(bt, [(1,) + p[1:] for p in places], tensor)                 # row 1 of one row
    with pytest.raises(ValueError):
        rows.synth(bt, places, tensor.view(torch.int32))                       # dtype
    with pytest.raises(ValueError):
        rows.synth(bt, places, tensor.transpose(1, 2))                         # shape / contiguity
    with pytest.raises(ValueError):
        rows.synth(bt, places, tensor.cpu())
    other = Rows(dec, 8, "i16")
    with pytest.raises(ValueError):
        other.synth(bt, places, torch.empty((1, 2, total), dtype=torch.int16, device="cuda:0"))   # the batch has another fmt
    other.close()
    torch.cuda.synchronize()
    assert bool((iv == int(_sentinel("f32"))).all())
    rows.synth(bt, places, tensor)                                             # exactly full is accepted
    torch.cuda.synchronize()
    assert not bool((iv == int(_sentinel("f32"))).any())
    assert rows.last_copied_elems == 2 * total
    bt.close()
    rows.close()


def _smallest_rows(Rows):
    audio, ident, st = _product(SETUPS["mono_small"]())
    return Rows(audio.decoder_for(ident, st), 1, "i16")


LIFECYCLE = {"Rows": _smallest_rows, "Resampler": lambda R: R(2, 1), "Spectrogram": lambda R: R(16, 8), "InverseSpectrogram": lambda R: R(16, 8),
             "LogCompress": lambda R: R(), "Normalize": lambda R: R(), "SlidingCMVN": lambda R: R(2, 1), "SelectFrames": lambda R: R(),
             "EnergyVad": lambda R: R(), "Cepstrum": lambda R: R(4), "FramePack": lambda R: R(4), "KaldiFbank": lambda R: R()}


@pytest.mark.parametrize("name", sorted(LIFECYCLE))
def test_handle_lifecycle(name):
    """what the classes over a handle share, with the smallest legal arguments and no launch: a handle after construction, -1
    launches before any call where the C API counts them, close() twice, then the finaliser; nothing raises"""
    import gc
    import sys
    from lewton_amd import rows as R
    unraisable, hook = [], sys.unraisablehook
    sys.unraisablehook = unraisable.append                                     # (where an exception in __del__ ends up)
    try:
        obj = LIFECYCLE[name](getattr(R, name))
        parts = [p for p in (obj.spec, obj.log, obj.norm) if p is not None] if name == "KaldiFbank" else [obj]
        assert parts and all(p._h for p in parts)
        for p in parts:
            if hasattr(p, "last_launches"):
                assert p.last_launches() == -1
        obj.close()
        assert all(p._h is None for p in parts)
        obj.close()
        assert all(p._h is None for p in parts)
        del obj, parts, p
        gc.collect()
    finally:
        sys.unraisablehook = hook
    assert not unraisable, [repr(u.exc_value) for u in unraisable]


def test_size_256_streams_of_64_packets():
    """[256, 2, 65 536] f32 planar from 4 batches of 4096 packets, every row against the oracle"""
    import torch
    from lewton_amd.batch import Batch
    from lewton_amd.rows import Rows
    setup = SETUPS["stereo"]()
    audio, ident, st = _product(setup)
    dec = audio.decoder_for(ident, st)
    o_id, o_st = oracle_headers(setup)
    seqs = [sg.make_stream(setup, "L", 64, seed=100 + q) for q in range(8)]
    streams = [seqs[s % 8][(s // 8):] + seqs[s % 8][:(s // 8)] for s in range(256)]   # 256 different streams of long blocks
    tensor, iv = _new_rows_tensor("f32", 256, 2, 65536)
    rows = Rows(dec, 4096, "f32")
    bts = [Batch(dec, 4096, "f32") for _ in range(4)]
    pws = [audio.PreviousWindowRight() for _ in streams]
    cur = _Cursor(256)
    for k, bt in enumerate(bts):
        items = [(s, 16 * k + j) for s in range(256) for j in range(16)]
        res = bt.entropy([(streams[s][t], pws[s]) for s, t in items])
        places = [cur.place(s, m if status == 0 else 0) for (s, t), (status, m, off) in zip(items, res)]
        bt.upload()
        rows.synth(bt, places, tensor)
        assert rows.last_copied_elems == 2 * sum(m for status, m, off in res)
    torch.cuda.synchronize()
    assert all(bt.device_status() == 0 for bt in bts)
    got = iv.cpu().numpy()
    want = np.full(got.shape, _sentinel("f32"), np.int32)
    wr = np.zeros(got.shape, bool)
    for s, pk in enumerate(streams):
        opw = po.Pwr()
        row = np.concatenate([np.asarray(po.read_audio_packet(o_id, o_st, p, opw, "f32")) for p in pk], 1)
        assert row.shape == (2, 63 * 1024)
        _place_into(want, wr, "f32", s, 0, row)
    _assert_rows(got, want, wr, "f32", "oracle")
    for bt in bts:
        bt.close()
    rows.close()


def test_destination_beyond_2_to_the_32_elements():
    """i16 planar stereo rows of 2^30 samples: a handful of packets at the end of row 2 land beyond element 2^32 of the tensor,
    and the window at the same offset mod 2^32 (row 0) keeps its sentinel"""
    import torch
    from lewton_amd.batch import Batch
    from lewton_amd.rows import Rows
    free, _ = torch.cuda.mem_get_info(0)
    if free < 16 << 30:
        pytest.skip("less than 16 GB of device memory free")
    setup = SETUPS["stereo"]()
    audio, ident, st = _product(setup)
    dec = audio.decoder_for(ident, st)
    streams = _streams(setup, "LLSL", [9], seed=19)
    (want_row, _), = _oracle_rows(setup, streams, "i16")
    total = want_row.shape[1]
    cap = 1 << 30
    tensor = torch.empty((3, 2, cap), dtype=torch.int16, device="cuda:0")      # 12.9 GB; only windows of it are ever touched
    W = total + 4096
    for r in (0, 2):
        tensor[r, :, cap - W:].fill_(SENTINEL[2])
    bt, rows = Batch(dec, 9, "i16"), Rows(dec, 9, "i16")
    pw = audio.PreviousWindowRight()
    res = bt.entropy([(p, pw) for p in streams[0]], n_threads=1)
    bt.upload()
    cur = _Cursor(1)
    places = []
    for status, m, off in res:
        row, sk, kp, t0 = cur.place(0, m)
        places.append((2, sk, kp, t0 + cap - total if kp else 0))              # the stream ends exactly at the end of row 2
    assert (2 * 2 * cap + cap - total) > 1 << 32
    rows.synth(bt, places, tensor)
    torch.cuda.synchronize()
    assert bt.device_status() == 0
    got2 = tensor[2, :, cap - W:].cpu().numpy()
    got0 = tensor[0, :, cap - W:].cpu().numpy()
    assert np.array_equal(got2[:, W - total:], want_row)
    assert bool((got2[:, :W - total] == SENTINEL[2]).all())
    assert bool((got0 == SENTINEL[2]).all()), "a destination offset was truncated to 32 bits"
    bt.close()
    rows.close()
    del tensor
    torch.cuda.empty_cache()


@pytest.mark.parametrize("entropy_on_device", ["auto", False])
@pytest.mark.parametrize("fmt", FMTS)
def test_decode_streams(fmt, entropy_on_device):
    import torch
    from lewton_amd.rows import decode_streams
    setup = SETUPS["stereo"]()
    _, ident, st = _product(setup)
    streams = _streams(setup, "LLSSLSL", [30, 7, 19, 1, 24, 0], seed=21)
    streams[2][8] = b"\x01" + bytes(streams[2][8])[1:]                          # a corrupted packet in the middle of stream 2
    want_rows = _oracle_rows(setup, streams, fmt)
    full = [r.shape[1] for r, _ in want_rows]
    want_errors = [(s, t, code) for s, (_, status) in enumerate(want_rows) for t, code in enumerate(status) if code]
    assert want_errors and want_errors[0][:2] == (2, 8)
    o_id, o_st = oracle_headers(setup)

    def count(p):
        try:
            return po.get_decoded_sample_count(o_id, o_st, p)
        except po.OracleError:
            return 0
    bound = [sum(count(p) for p in pk[1:]) for pk in streams]                   # what is known up front
    for skip, keep, max_packets, out_extra in [(None, None, 16384, None), ([5, 0, 1000, 0, 3, 0], [None, 333, None, 5, 2001, None], 16, None),
                                               ([0, 1, 0, 0, 700, 0], None, 11, 128)]:
        sk = skip or [0] * 6
        kp = keep or [None] * 6
        want_len = [max(f - a, 0) if k is None else min(max(f - a, 0), k) for f, a, k in zip(full, sk, kp)]
        want_T = -(-max(max(b - a, 0) if k is None else min(max(b - a, 0), k) for b, a, k in zip(bound, sk, kp)) // 64) * 64
        out = None
        if out_extra is not None:
            T = want_T + out_extra
            out = torch.full((6, T, 2) if _itl(fmt) else (6, 2, T), 7, dtype=torch.float32 if _is_f32(fmt) else torch.int16, device="cuda:0")
        pcm, lengths, errors = decode_streams(ident, st, streams, fmt, max_packets=max_packets, run=4, skip=skip, keep=keep, out=out,
                                              entropy_on_device=entropy_on_device)
        if out is not None:
            assert pcm is out
        assert sorted(errors) == want_errors
        assert lengths.dtype == torch.int64 and lengths.tolist() == want_len
        T = pcm.shape[1 if _itl(fmt) else 2]
        assert T >= max(want_len) and T == want_T + (out_extra or 0)
        assert pcm.dtype == (torch.float32 if _is_f32(fmt) else torch.int16) and pcm.device.index == 0
        got = pcm.view(torch.int32 if _is_f32(fmt) else torch.int16).cpu().numpy()
        want = np.zeros(got.shape, got.dtype)                                   # zero beyond each row's length
        wr = np.zeros(got.shape, bool)
        for s, (row, _) in enumerate(want_rows):
            _place_into(want, wr, fmt, s, 0, row[:, sk[s]:sk[s] + want_len[s]])
        same = got == want
        if _is_f32(fmt):
            same |= np.isnan(got.view(np.float32)) & np.isnan(want.view(np.float32))
        assert bool(same.all()), (skip, keep, np.argwhere(~same)[:4].tolist())


def _reader_rows(data, fmt):
    """the concatenation of what OggStreamReader.read_dec_packet_generic returns, and of what the oracle's reader returns"""
    from lewton_amd import inside_ogg as IO
    from oracle import pyogg
    planar = "f32" if _is_f32(fmt) else "i16"
    s, o = IO.OggStreamReader(data), pyogg.OggStreamReader(data, planar)
    a, b = [], []
    while True:
        x, y = s.read_dec_packet_generic(planar), o.read_dec_packet()
        assert (x is None) == (y is None)
        if x is None:
            break
        a.append(x), b.append(np.asarray(y))
    rate = s.ident_hdr.audio_sample_rate
    s.close()
    return np.concatenate(a, 1), np.concatenate(b, 1), rate


def _check_ogg(datas, fmt, **kw):
    import torch
    from lewton_amd.rows import decode_ogg_files
    pcm, lengths, rate = decode_ogg_files(datas, fmt, **kw)
    got = pcm.view(torch.int32 if _is_f32(fmt) else torch.int16).cpu().numpy()
    want = np.zeros(got.shape, got.dtype)
    wr = np.zeros(got.shape, bool)
    for i, d in enumerate(datas):
        if isinstance(d, str):
            d = open(d, "rb").read()
        mine, oracle, r = _reader_rows(d, fmt)
        assert r == rate and mine.shape == oracle.shape and lengths[i].item() == mine.shape[1]
        ob, mb = oracle.view(_int_dtype(fmt)), mine.view(_int_dtype(fmt))
        assert bool(((ob == mb) | (np.isnan(oracle) & np.isnan(mine) if _is_f32(fmt) else False)).all())
        _place_into(want, wr, fmt, i, 0, mine)
    assert np.array_equal(got, want)
    assert pcm.shape[1 if _itl(fmt) else 2] == -(-int(lengths.max()) // 64) * 64
    return pcm, lengths


@pytest.mark.parametrize("fmt", FMTS)
def test_decode_ogg_files_golden_three_times(fmt):
    path = os.path.join(ROOT, "tests", "golden", "invalid_keypress.ogg")
    data = open(path, "rb").read()
    pcm, lengths = _check_ogg([path, data, path], fmt)
    assert lengths[0] == lengths[1] == lengths[2] and lengths[0] > 0


@pytest.mark.parametrize("fmt", FMTS)
def test_decode_ogg_files_two_setups(fmt):
    files = [_vorbis_stream("stereo", "LLSLSSL", 40, per_page=4, trim=333, seed=3)[2].bytes(),
             _vorbis_stream("stereo_t1", "LSSLL", 23, per_page=5, trim=37, seed=4)[2].bytes(),
             _vorbis_stream("stereo", "LLSL", 9, per_page=3, trim=0, seed=5)[2].bytes(),
             _vorbis_stream("stereo_t1", "LLSLSSL", 31, per_page=4, trim=333, seed=6)[2].bytes()]
    _check_ogg(files, fmt, max_packets=32, run=5)


def test_decode_ogg_files_refuses_chained_and_mixed():
    from lewton_amd.rows import decode_ogg_files
    a = _vorbis_stream("stereo", "LLSL", 9, serial=0x11)[2].bytes()
    b = _vorbis_stream("stereo", "LSSL", 9, serial=0x22)[2].bytes()
    with pytest.raises(ValueError, match="source 1"):
        decode_ogg_files([a, a + b])                                            # a chained file
    mono = _vorbis_stream("mono_small", "SLLS", 9)[2].bytes()
    with pytest.raises(ValueError, match="source 2"):
        decode_ogg_files([a, b, mono])
