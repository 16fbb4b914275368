"""Stream-major rows: whole streams decoded into ONE device tensor that stays on the GPU.

Everything else in this package hands PCM back packet-major (a batch's output is a run of per-packet blocks, the packets of
many streams mixed: lewton's call shape).  A caller that decodes many whole streams and goes on working on the GPU wants
`[stream][channel][sample]`, padded to a common length:

    pcm, lengths, errors = decode_streams(ident, setup, streams)          # streams: list of lists of audio-packet bytes
    pcm, lengths, rate = decode_ogg_files(["a.ogg", "b.ogg", data])       # first logical stream of each file

    rows = Rows(decoder, max_packets, "f32")                              # the layer below: lw_rows_* of include/lewton_amd.h
    rows.synth(batch, places, tensor)                                     # lw_batch_synth + k_rows on torch's current stream
    rows.synth(batch, places, tensor, mix=mix_mono(2))                    # ... through a channel matrix (lw_rows_synth_mix)

`pcm` is a torch tensor on `cuda:device`: [B, C, T] for the planar formats, [B, T, C] for the interleaved ones, int16 or
float32, zero beyond each row's length.  The synthesis kernels write a batch's blocks into a staging buffer as always; one more
kernel behind them (k_rows, csrc/lw_kernels_rows.hip) moves the samples into their rows, so no sample crosses PCIe.
channels= / mix= puts a channel matrix [out_ch][in_ch] into that kernel (k_rows_mix): C becomes out_ch, every output channel is
folded from the stream's channels by the rule of include/lewton_amd.h (lw_rows_synth_mix) -- mono downmix, a selection, WAVE
channel order -- and files of different channel counts fill one tensor.
sample_rate= resamples the finished rows on the GPU (Resampler, lw_resample_rows, k_resample in csrc/lw_kernels_resample.hip: a
windowed-sinc polyphase filter specified bit for bit, f32 formats), and files of different sample rates fill one tensor:

    pcm, lengths, rate = decode_ogg_files(paths, channels="mono", sample_rate=16000)
    rs = Resampler(44100, 16000); out = rs.run(tensor, lengths)             # the same pass over a caller's own rows tensor

Spectrogram turns finished rows into a power spectrum or (log-)mel features on the GPU (lw_spec_rows, k_spec in
csrc/lw_kernels_spec.hip: a windowed DFT on the f32 matrix instruction, specified bit for bit), the step between the waveform and
a speech model's input:

    sp = Spectrogram(400, 160, mel=mel_filterbank(16000, 400, 80)); feats, frames = sp.run(pcm, lengths, log="log10")

pad_mode="reflect" frames a row as torch.stft's default does, and LogCompress finishes the features on the GPU (lw_feat_rows, k_feat
in csrc/lw_kernels_feat.hip: a logarithm specified in double arithmetic, the clamp under the row's maximum, an affine map and the
fill, bit for bit) -- together the input of a Whisper-style model:

    sp = Spectrogram(400, 160, mel=mel_filterbank(16000, 400, 80, scale="slaney", norm="slaney"), pad_mode="reflect")
    feats, frames = sp.run(pcm, lengths, out=torch.zeros((B, 1, 80, 3000), device="cuda"))
    LogCompress.whisper().run(feats, frames, fill_to=3000)

output="complex" keeps the phase (the re and im lines of every bin), and InverseSpectrogram is the way back (lw_istft_rows, k_istft
in csrc/lw_kernels_istft.hip: inverse DFT on the matrix instruction, overlap-add and envelope division, bit for bit) -- what a
mask-based enhancement or separation model stands between:

    sp, inv = Spectrogram(512, 128, output="complex", pad_mode="reflect"), InverseSpectrogram(512, 128)
    spec, frames = sp.run(pcm, lengths); pcm2, _ = inv.run(model(spec), frames, lengths=lengths)

Normalize is the step the waveform models (wav2vec 2.0, HuBERT, WavLM) and utterance CMVN need (lw_norm_rows, k_norm in
csrc/lw_kernels_norm.hip: mean and deviation, RMS or peak of a row, a channel or a line from double sums in a fixed order, bit for
bit), over a waveform tensor [B, C, T] or a feature tensor [B, C, F, frames]:

    Normalize.wav2vec2().run(pcm, lengths)                                  # in place; or decode_ogg_files(..., normalize="wav2vec2")
    Normalize.cmvn().run(feats, frames, fill_to=3000)

FramePack turns the chain's [B, C, F, frames] into the [B, C, frames, W * F] most other speech models read (lw_pack_rows, k_pack in
csrc/lw_kernels_pack.hip: transpose, context splice and stride, a global shift and scale, one rounding to float32, bfloat16 or
float16, padding and the padding mask in one launch, bit for bit):

    out, out_frames, mask = FramePack.lfr(80, shift=s, scale=g, dtype="bf16").run(feats, frames, want_mask=True)

EnergyVad, SlidingCMVN and SelectFrames are what the Kaldi speaker and language recipes run between fbank and the model
(compute-vad-energy on the raw features, apply-cmvn-sliding, select-voiced-frames: lw_vad_rows, lw_slide_rows, lw_select_rows, each
bit for bit):

    voiced = EnergyVad(5.5, 0.5, 2, 0.12).run(feats, frames)
    kept, counts = SelectFrames().run(SlidingCMVN(300, 100, center=True).run(feats, frames), frames, voiced)

Segments turns a mask into stretches of speech (lw_segment_rows, k_segment: pad, fill short gaps, drop short runs, the order of
pyannote's Binarize, on integers) and CutRows makes every stretch a row of its own (lw_cut_rows, k_cut), so that a recogniser, a
speaker-embedding extractor or a diarizer gets its segments with one synchronisation and one launch:

    spans, counts = Segments(pad_onset=2, pad_offset=8, min_off=10, min_on=5).run(voiced, frames)
    jobs, _ = Segments.jobs(spans, counts, hop=160, window=400, lengths=lengths)      # the one synchronisation
    seg_pcm, seg_len = CutRows().run(pcm, lengths, jobs)

SpecAugment is the one step a training loader puts between the normalised features and the model (lw_specaug_rows, k_specaug: time
and frequency masks drawn by a counter-based generator, so an utterance's masks depend on (seed, id) alone, bit for bit):

    SpecAugment.wenet(seed=epoch).run(feats, frames, ids=utterance_ids)     # in place

torch is imported inside the functions, never at module import.
"""
import ctypes as C
from collections import deque

import numpy as np

# The HIP library is loaded on first use, BEHIND torch: torch ships its own copy of the HIP runtime, and a process has to run on
# one.  The dynamic loader lets liblewton_amd.so share the runtime torch has loaded, not the other way round, so a process that
# uses this module imports torch (or calls into this module) before it imports any other lewton_amd module that loads the library.
N = _FMT = AudioReadError = PreviousWindowRight = decoder_for = get_decoded_sample_count = None
_one_runtime = None


def _host():
    """the library and the names of lewton_amd.audio this module uses (no torch needed: headers, demultiplexing, sample counts)"""
    global N, _FMT, AudioReadError, PreviousWindowRight, decoder_for, get_decoded_sample_count
    if N is None:
        from . import _native, audio
        _FMT, AudioReadError, PreviousWindowRight = audio._FMT, audio.AudioReadError, audio.PreviousWindowRight
        decoder_for, get_decoded_sample_count = audio.decoder_for, audio.get_decoded_sample_count
        N = _native
    return N


def _gpu():
    """torch, then the library; refuses to go on when the two ended up on two copies of the HIP runtime (a stream or a device
    pointer of one means nothing to the other)"""
    global _one_runtime
    import torch
    _host()
    if _one_runtime is None:
        try:
            with open("/proc/self/maps") as f:
                copies = {ln.split()[-1] for ln in f if "libamdhip64" in ln}
        except OSError:
            copies = set()
        _one_runtime = len(copies) <= 1
    if not _one_runtime:
        raise RuntimeError("lewton_amd.rows: the HIP library was loaded before torch, so this process holds two copies of the HIP "
                           "runtime; import torch (or use lewton_amd.rows) before any other lewton_amd module")
    return torch


class _Handle:
    """What the classes over a lw_* handle share: creation with its status check, close(), a __del__ that cannot raise, and the
    call of a *_rows entry point with its status check.  _C is the prefix of the handle's functions (_C + "_create",
    _C + "_destroy"), as a string: the library is not loaded when the classes are defined."""

    _C = None
    _REFUSED_PARAMETERS = ("ERR_UNSUPPORTED", "ERR_NULL_ARG")   # create statuses that are a ValueError (names of lewton_amd._native)

    def _create(self, *args, create="_create"):
        """self._h from _C + create (args, &err), or ValueError / RuntimeError"""
        _gpu()
        err = C.c_int(0)
        self._h = getattr(N, self._C + create)(*args, C.byref(err))
        if not self._h:
            if err.value in [getattr(N, name) for name in self._REFUSED_PARAMETERS]:
                raise ValueError("%s%s refused the parameters" % (self._C, create))
            raise RuntimeError("%s%s failed (%d): %s" % (self._C, create, err.value, N.device_error()))

    def close(self):
        if getattr(self, "_h", None):
            getattr(N, self._C + "_destroy")(self._h)
            self._h = None

    def __del__(self):
        if N is not None and getattr(N, self._C + "_destroy", None) is not None:  # not during interpreter shutdown
            self.close()

    def _call(self, fn, *args):
        """fn(handle, *args) for an entry point that returns a status: ValueError for a refusal, RuntimeError for anything else"""
        rc = fn(self._h, *args)
        if rc:
            if rc in (N.ERR_NULL_ARG, N.ERR_CAPACITY, N.ERR_STATE_MISMATCH, N.ERR_UNSUPPORTED):
                raise ValueError("%s refused the call (%d)" % (fn.__name__, rc))
            raise RuntimeError("%s: %d %s" % (fn.__name__, rc, N.device_error()))


def _stream_of(stream, device):
    """the hipStream_t value a call is queued on: the caller's, or torch's current stream on the device (None: the null stream)"""
    if stream is None:
        import torch
        stream = torch.cuda.current_stream(device).cuda_stream or None
    return stream


def _tensor_ptr(t):
    """the address of a tensor's first element as a C argument; None stays None"""
    return None if t is None else C.c_void_p(t.data_ptr())


def _array_ptr(a):
    """the address of a numpy array's first element as a C argument; None stays None.  The value does not keep the array alive (and
    costs half of what data_as does): the caller holds the array for the length of the call"""
    return None if a is None else C.c_void_p(a.ctypes.data)


def _check_tensor(t, what, layout, device, dtypes, dims=None, shape=None):
    """ValueError that names `what` and the expected `layout`, unless t is a contiguous tensor of one of `dtypes` on cuda:device
    with one of the dimension counts `dims` (None: any) and, where given, exactly `shape`"""
    if (t.dtype not in dtypes or not t.is_cuda or t.get_device() != device or not t.is_contiguous() or
            (dims is not None and t.dim() not in dims) or (shape is not None and tuple(t.shape) != tuple(shape))):
        raise ValueError("%s must be a contiguous %s tensor %s on cuda:%d, not %s %r on %s" % (
            what, " or ".join(str(d) for d in dtypes), layout, device, t.dtype, tuple(t.shape), t.device))


def _pcm_shape(t, samples, what, device):
    """(n_rows, channels, row_capacity) of a float32 rows tensor [B, C, T], or [B, T, C] for an interleaved format; or ValueError"""
    _check_tensor(t, what, "[rows][channels][samples] (interleaved: [rows][samples][channels])", device, (_gpu().float32,), (3,))
    b, x, y = t.shape
    return (b, y, x) if N.fmt_interleaved(_FMT[samples]) else (b, x, y)


def _row_counts(v, n_rows, what):
    """one non-negative count per row as uint64, from a list, an array or a tensor"""
    counts = [int(c) for c in (v.tolist() if hasattr(v, "tolist") else v)]
    if len(counts) != n_rows or any(c < 0 for c in counts):
        raise ValueError("%s= needs one non-negative entry per row" % what)
    return np.asarray(counts, np.uint64)


def _row_fill(fill_to, n_rows):
    """None, or one non-negative count per row as uint64 from one count for all rows or one per row"""
    if fill_to is None:
        return None
    fill = fill_to.tolist() if hasattr(fill_to, "tolist") else fill_to
    fill = [int(fill)] * n_rows if isinstance(fill, (int, np.integer)) else [int(v) for v in fill]
    if len(fill) != n_rows or any(v < 0 for v in fill):
        raise ValueError("fill_to= needs one non-negative count, or one per row")
    return np.asarray(fill, np.uint64)


def _row_map(rows, n_rows):
    """rows= of the calls that scatter their rows -> (the destination rows as uint32 or None, the rows of a destination that just
    holds them: max(rows) + 1, or n_rows without a map)"""
    if rows is None:
        return None, n_rows
    rows = [int(v) for v in (rows.tolist() if hasattr(rows, "tolist") else rows)]
    if len(rows) != n_rows or any(not 0 <= v < 1 << 32 for v in rows):
        raise ValueError("rows= needs one destination row per source row")
    return np.asarray(rows, np.uint32), max(rows) + 1 if rows else n_rows


ALL = 0xFFFFFFFF  # lw_row_place.keep: all samples that remain behind skip
PLACE_DTYPE = np.dtype([("row", "<u4"), ("skip", "<u4"), ("keep", "<u4"), ("pad_", "<u4"), ("t0", "<u8")])   # lw_row_place
_RESULT_DTYPE = np.dtype([("status", "<i4"), ("n_samples", "<u4"), ("out_offset", "<u8")])                    # lw_packet_result
_NO_LIMIT = 1 << 62


def places_array(places):
    """lw_row_place array from an iterable of (row, skip, keep, t0); keep None = all that remain."""
    if isinstance(places, np.ndarray) and places.dtype == PLACE_DTYPE:
        return np.ascontiguousarray(places)
    places = list(places)
    arr = np.zeros(len(places), PLACE_DTYPE)
    for i, (row, skip, keep, t0) in enumerate(places):
        arr[i] = (row, skip, ALL if keep is None else keep, 0, t0)
    return arr


MIX_MAX_OUT = 8  # LW_ROWS_MIX_MAX_OUT
# Vorbis I channel order (section 4.3.9 of the specification) -> WAVE mask order (FL FR FC LFE BL BR SL SR): source of output o
_WAV_SOURCES = {1: (0,), 2: (0, 1), 3: (0, 2, 1), 4: (0, 1, 2, 3), 5: (0, 2, 1, 3, 4), 6: (0, 2, 1, 5, 3, 4),
                7: (0, 2, 1, 6, 5, 3, 4), 8: (0, 2, 1, 7, 5, 6, 3, 4)}


def mix_mono(in_ch):
    """[1][in_ch] float32: the mean of the channels, 1 / in_ch each"""
    if in_ch < 1:
        raise ValueError("no channels")
    return np.full((1, in_ch), np.float32(1) / np.float32(in_ch), np.float32)


def mix_select(in_ch, sources):
    """routing matrix [len(sources)][in_ch] float32: output channel o is a copy of input channel sources[o], silence for None"""
    sources = list(sources)
    m = np.zeros((len(sources), in_ch), np.float32)
    for o, c in enumerate(sources):
        if c is None:
            continue
        if not 0 <= c < in_ch:
            raise ValueError("source channel %r of %d" % (c, in_ch))
        m[o, c] = 1
    return m


def mix_wav_order(in_ch):
    """routing matrix from Vorbis I channel order to WAVE mask order; ValueError for channel counts Vorbis I assigns no order to"""
    if in_ch not in _WAV_SOURCES:
        raise ValueError("no WAVE channel order for %d channels" % in_ch)
    return mix_select(in_ch, _WAV_SOURCES[in_ch])


def mix_array(mix, in_ch):
    """a channel matrix as contiguous float32 [out_ch][in_ch], or ValueError"""
    m = np.ascontiguousarray(mix, dtype=np.float32)
    if m.ndim != 2 or m.shape[1] != in_ch or not 1 <= m.shape[0] <= MIX_MAX_OUT:
        raise ValueError("a channel matrix is [1..%d output channels][%d input channels], not %s" % (MIX_MAX_OUT, in_ch, m.shape))
    return m


def mix_is_routing(m):
    """every row holds at most one non-zero coefficient, and that one is 1.0 (what the i16 formats accept)"""
    return bool(((m != 0).sum(1) <= 1).all() and ((m == 0) | (m == 1)).all())


def _named_mix(channels, in_ch, fmt):
    """channels= of decode_streams: "mono" or a matrix -> float32 [out_ch][in_ch], checked against the format"""
    _host()
    m = mix_mono(in_ch) if isinstance(channels, str) and channels == "mono" else \
        mix_wav_order(in_ch) if isinstance(channels, str) and channels == "wav" else None
    if m is None:
        if isinstance(channels, str):
            raise ValueError("channels=%r: \"mono\", \"wav\" or a matrix" % channels)
        m = mix_array(channels, in_ch)
    if fmt in (N.FMT_I16_PLANAR, N.FMT_I16_INTERLEAVED) and not mix_is_routing(m):
        raise ValueError("the i16 formats take routing matrices only (one coefficient 1.0 per row at most), not %s" % m.tolist())
    return m


def torch_dtype(fmt):
    torch = _gpu()
    return torch.float32 if fmt in (N.FMT_F32_PLANAR, N.FMT_F32_INTERLEAVED) else torch.int16


class Rows(_Handle):
    """lw_rows: the staging PCM buffer and the segment arrays behind lw_rows_synth, for batches of one decoder and format."""

    _C = "lw_rows"
    _REFUSED_PARAMETERS = ()    # lw_rows_create reports max_packets == 0 as LW_ERR_NULL_ARG, and that has always been a RuntimeError

    def __init__(self, decoder, max_packets, samples="f32"):
        _gpu()
        self.dec = decoder
        self.fmt = _FMT[samples]
        self.max_packets = max_packets
        self._create(decoder._h, max_packets, self.fmt)

    create = classmethod(lambda cls, decoder, max_packets, samples="f32": cls(decoder, max_packets, samples))

    def check_tensor(self, tensor, out_ch=None):
        """(n_rows, row_capacity) of a rows tensor, or ValueError: dtype, device, contiguity and shape against the format;
        out_ch: the channels of the rows when a matrix is used (None: the decoder's)"""
        ch = self.dec.ident.audio_channels if out_ch is None else out_ch
        _check_tensor(tensor, "rows tensor", "of three dimensions", self.dec.device, (torch_dtype(self.fmt),), (3,))
        if N.fmt_interleaved(self.fmt):
            if tensor.shape[2] != ch:
                raise ValueError("interleaved rows are [rows][samples][%d channels], not %s" % (ch, tuple(tensor.shape)))
            return tensor.shape[0], tensor.shape[1]
        if tensor.shape[1] != ch:
            raise ValueError("planar rows are [rows][%d channels][samples], not %s" % (ch, tuple(tensor.shape)))
        return tensor.shape[0], tensor.shape[2]

    def synth(self, batch, places, tensor, stream=None, mix=None):
        """lw_rows_synth: the synthesis kernels of `batch` (entropy stage done, uploaded) and k_rows behind them.  places: one
        (row, skip, keep, t0) per packet of the batch, or an array of PLACE_DTYPE.  stream: a hipStream_t value; None = torch's
        current stream on the decoder's device.  mix: a channel matrix, array-like [out_ch][in_ch] (lw_rows_synth_mix, k_rows_mix
        in place of k_rows); the tensor then has out_ch channels.  Asynchronous."""
        _gpu()
        if mix is not None:
            mix = mix_array(mix, self.dec.ident.audio_channels)
        n_rows, cap = self.check_tensor(tensor, None if mix is None else mix.shape[0])
        arr = places_array(places)
        stream = _stream_of(stream, self.dec.device)
        pl = _array_ptr(arr if arr.size else None)
        if mix is None:
            self._call(N.lw_rows_synth, batch._h, pl, arr.size, _tensor_ptr(tensor), n_rows, cap, stream)
        else:
            m = N.RowMix(mix.shape[0], mix.shape[1], _array_ptr(mix))      # (the coefficients are copied by the call)
            self._call(N.lw_rows_synth_mix, batch._h, pl, arr.size, C.byref(m), _tensor_ptr(tensor), n_rows, cap, stream)

    @property
    def last_segments(self):
        return N.lw_rows_last_segments(self._h)

    @property
    def last_copied_elems(self):
        return N.lw_rows_last_copied_elems(self._h)


_WINDOWS = {"hann": 0, "kaiser": 1}          # LW_RESAMPLE_HANN, LW_RESAMPLE_KAISER
KAISER_BETA = 14.769656459379492            # the good-quality choice of include/lewton_amd.h, with zeros=16
RESAMPLE_MAX_TAPS = 65536                   # LW_RESAMPLE_MAX_TAPS


def resample_geometry(in_rate, out_rate, zeros=6, rolloff=0.99):
    """(orig, new, half width W, taps per phase K) of a resampler, by the rule of include/lewton_amd.h ("resampling rows");
    ValueError for what lw_resampler_create refuses.  Needs no GPU."""
    import math
    for name, v in (("in_rate", in_rate), ("out_rate", out_rate), ("zeros", zeros)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not 0 < v < 1 << 32:
            raise ValueError("%s=%r: a positive integer" % (name, v))
    if not 0 < rolloff <= 1:
        raise ValueError("rolloff=%r: in (0, 1]" % (rolloff,))
    g = math.gcd(int(in_rate), int(out_rate))
    orig, new = int(in_rate) // g, int(out_rate) // g
    s = float(rolloff) * (new / orig if new < orig else 1.0)
    w = math.ceil(zeros / s)
    if new * (2 * w + 2) > RESAMPLE_MAX_TAPS:
        raise ValueError("%d -> %d Hz with zeros=%d needs %d x %d taps, more than %d" % (in_rate, out_rate, zeros, new, 2 * w + 2,
                                                                                     RESAMPLE_MAX_TAPS))
    return orig, new, w, 2 * w + 2


def _resample_params(resample):
    """resample= of decode_streams / decode_ogg_files: a dict of Resampler's filter parameters, checked by name"""
    p = dict(resample or {})
    extra = set(p) - {"zeros", "rolloff", "window", "beta"}
    if extra:
        raise ValueError("resample= takes zeros, rolloff, window and beta, not %s" % ", ".join(sorted(extra)))
    return p


class Resampler(_Handle):
    """lw_resampler: rows of f32 PCM at in_rate -> rows at out_rate on the GPU (k_resample), by the windowed-sinc polyphase filter
    of include/lewton_amd.h ("resampling rows"), a contract on bits.  window: "hann" or "kaiser" (beta: KAISER_BETA when None).
    Parameter errors are ValueError and need no GPU; the object itself lives on cuda:device."""

    _C = "lw_resampler"

    def __init__(self, in_rate, out_rate, zeros=6, rolloff=0.99, window="hann", beta=None, device=0):
        if window not in _WINDOWS:
            raise ValueError("window=%r: \"hann\" or \"kaiser\"" % (window,))
        if beta is None:
            beta = KAISER_BETA if window == "kaiser" else 0.0
        if window == "kaiser" and not 0 <= beta < 700:
            raise ValueError("beta=%r: in [0, 700)" % (beta,))
        self.orig, self.new, self.half_width, self.taps_per_phase = resample_geometry(in_rate, out_rate, zeros, rolloff)
        self.in_rate, self.out_rate, self.device = int(in_rate), int(out_rate), device
        self._create(device, int(in_rate), int(out_rate), int(zeros), float(rolloff), _WINDOWS[window], float(beta))
        geo = [C.c_uint32() for _ in range(4)]
        N.lw_resampler_geometry(self._h, *[C.byref(g) for g in geo])
        assert tuple(g.value for g in geo) == (self.orig, self.new, self.half_width, self.taps_per_phase)

    def taps(self):
        """the filter [new][K], float32"""
        out = np.empty((self.new, self.taps_per_phase), np.float32)
        assert N.lw_resampler_taps(self._h, None) == out.size
        N.lw_resampler_taps(self._h, _array_ptr(out))
        return out

    def out_len(self, n):
        """output samples of a row of n input samples: ceil(n * new / orig)"""
        return int(N.lw_resampler_out_len(self._h, int(n)))

    @property
    def last_route(self):
        """0: taps and samples from LDS, 1: taps from global memory, 2: both from global memory, 3: copy (lw_resampler_last_route)"""
        return N.lw_resampler_last_route(self._h)

    def check_tensor(self, tensor, samples, what):
        """(n_rows, channels, row_capacity) of a rows tensor, or ValueError: as Rows.check_tensor, for the two f32 formats"""
        return _pcm_shape(tensor, samples, what, self.device)

    def run(self, src, lengths, out=None, rows=None, stream=None, samples="f32"):
        """lw_resample_rows: row i of src ([B, C, T], or [B, T, C] for samples="f32_interleaved"), lengths[i] samples per channel,
        -> row rows[i] of out (None: row i), out_len(lengths[i]) samples; nothing else of out is written.  out=None: a zeroed
        tensor of max(rows) + 1 rows and the longest output length.  stream: a hipStream_t value; None = torch's current stream on
        the resampler's device.  Asynchronous; returns out."""
        torch = _gpu()
        fmt = _FMT[samples]
        if fmt not in (N.FMT_F32_PLANAR, N.FMT_F32_INTERLEAVED):
            raise ValueError("the resampler works on the f32 formats, not %r" % (samples,))
        n_src, ch, cap = self.check_tensor(src, samples, "src")
        lens = _row_counts(lengths, n_src, "lengths")
        rmap, n_dst = _row_map(rows, n_src)
        if out is None:
            T = max([self.out_len(v) for v in lens.tolist()], default=0)
            out = torch.zeros((n_dst, T, ch) if N.fmt_interleaved(fmt) else (n_dst, ch, T), dtype=torch.float32, device="cuda:%d" % self.device)
        n_dst, och, dcap = self.check_tensor(out, samples, "out")
        if och != ch:
            raise ValueError("out has %d channels, src %d" % (och, ch))
        self._call(N.lw_resample_rows, fmt, ch, _tensor_ptr(src), n_src, cap, _array_ptr(lens), _array_ptr(rmap), _tensor_ptr(out),
                   n_dst, dcap, _stream_of(stream, self.device))
        return out


_SPEC_WINDOWS = {"hann": 0, "rect": 1, "povey": 2, "hamming_sym": 3, "hann_sym": 4, "blackman_sym": 5}   # LW_SPEC_HANN ... LW_SPEC_BLACKMAN
_SPEC_PAD_MODES = {"zero": 0, "reflect": 1}  # LW_SPEC_PAD_ZERO, LW_SPEC_PAD_REFLECT
_SPEC_OUTPUTS = {"power": 0, "complex": 1}   # LW_SPEC_OUT_POWER, LW_SPEC_OUT_COMPLEX
_SPEC_FRAMINGS = {("stft", True): 0, ("stft", False): 0, ("kaldi", True): 1, ("kaldi", False): 2}   # (framing, snip_edges): LW_SPEC_FRAMES_*
SPEC_MAX_FFT, SPEC_MAX_MELS = 2048, 256     # LW_SPEC_MAX_FFT, LW_SPEC_MAX_MELS
ISTFT_MAX_OVERLAP = 16                      # LW_ISTFT_MAX_OVERLAP


def _mel_scale(f, scale):
    f = np.asarray(f, np.float64)
    if scale == "htk":
        return 2595.0 * np.log10(1.0 + f / 700.0)
    with np.errstate(divide="ignore"):
        return np.where(f < 1000.0, f / (200.0 / 3), 15.0 + np.log(np.maximum(f, 1e-300) / 1000.0) / (np.log(6.4) / 27.0))


def _mel_inverse(m, scale):
    m = np.asarray(m, np.float64)
    if scale == "htk":
        return 700.0 * (10.0 ** (m / 2595.0) - 1.0)
    return np.where(m < 15.0, m * (200.0 / 3), 1000.0 * np.exp((m - 15.0) * (np.log(6.4) / 27.0)))


def mel_filterbank(sample_rate, n_fft, n_mels, fmin=0.0, fmax=None, scale="htk", norm=None):
    """[n_mels][n_fft // 2 + 1] float32 triangular filters, computed in float64 and rounded once: n_mels + 2 points p equally
    spaced on the mel scale from fmin to fmax (sample_rate / 2 when None); the weight of bin frequency f_j = j * sample_rate /
    n_fft in row q is max(0, min((f_j - p[q]) / (p[q+1] - p[q]), (p[q+2] - f_j) / (p[q+2] - p[q+1]))).  scale: "htk"
    (2595 log10(1 + f / 700)) or "slaney" (f / (200 / 3) below 1000 Hz, 15 + ln(f / 1000) / (ln(6.4) / 27) above); norm="slaney"
    multiplies row q by 2 / (p[q+2] - p[q]).  Needs no GPU."""
    if scale not in ("htk", "slaney"):
        raise ValueError("scale=%r: \"htk\" or \"slaney\"" % (scale,))
    if norm not in (None, "slaney"):
        raise ValueError("norm=%r: None or \"slaney\"" % (norm,))
    if isinstance(n_mels, bool) or not isinstance(n_mels, (int, np.integer)) or not 1 <= n_mels <= SPEC_MAX_MELS:
        raise ValueError("n_mels=%r: 1 .. %d" % (n_mels, SPEC_MAX_MELS))
    if isinstance(n_fft, bool) or not isinstance(n_fft, (int, np.integer)) or not 2 <= n_fft <= SPEC_MAX_FFT:
        raise ValueError("n_fft=%r: 2 .. %d" % (n_fft, SPEC_MAX_FFT))
    if fmax is None:
        fmax = sample_rate / 2.0
    if not (sample_rate > 0 and 0 <= fmin < fmax):
        raise ValueError("0 <= fmin < fmax and sample_rate > 0 are required")
    p = _mel_inverse(np.linspace(_mel_scale(fmin, scale), _mel_scale(fmax, scale), int(n_mels) + 2), scale)
    f = np.arange(int(n_fft) // 2 + 1, dtype=np.float64) * (float(sample_rate) / int(n_fft))
    up = (f[None, :] - p[:-2, None]) / (p[1:-1] - p[:-2])[:, None]
    down = (p[2:, None] - f[None, :]) / (p[2:] - p[1:-1])[:, None]
    w = np.maximum(0.0, np.minimum(up, down))
    if norm == "slaney":
        w = w * (2.0 / (p[2:] - p[:-2]))[:, None]
    return w.astype(np.float32)


def kaldi_mel_banks(sample_rate, n_fft, n_mels, low_freq=20.0, high_freq=0.0):
    """[n_mels][n_fft // 2 + 1] float32: Kaldi's mel banks (kaldi-native-fbank, torchaudio.compliance.kaldi.get_mel_banks without
    VTLN), triangles in the MEL domain, computed in float64 and rounded once.  mel(f) = 1127 ln(1 + f / 700); high_freq <= 0 is
    an offset from sample_rate / 2; the n_mels + 2 points are equally spaced in mel from mel(low_freq) to mel(high_freq); bin
    i < n_fft / 2 at m = mel(i * sample_rate / n_fft) gets a weight only when left < m < right: (m - left) / (centre - left) when
    m <= centre, else (right - m) / (right - centre).  The Nyquist column is zero.  n_fft must be even.  Needs no GPU."""
    if isinstance(n_mels, bool) or not isinstance(n_mels, (int, np.integer)) or not 1 <= n_mels <= SPEC_MAX_MELS:
        raise ValueError("n_mels=%r: 1 .. %d" % (n_mels, SPEC_MAX_MELS))
    if isinstance(n_fft, bool) or not isinstance(n_fft, (int, np.integer)) or not 2 <= n_fft <= SPEC_MAX_FFT or n_fft % 2:
        raise ValueError("n_fft=%r: even, 2 .. %d" % (n_fft, SPEC_MAX_FFT))
    sample_rate, low, high = float(sample_rate), float(low_freq), float(high_freq)
    if not sample_rate > 0:
        raise ValueError("sample_rate > 0 is required")
    nyquist = 0.5 * sample_rate
    if high <= 0.0:
        high += nyquist
    if not 0.0 <= low < high <= nyquist:
        raise ValueError("0 <= low_freq < high_freq <= sample_rate / 2 is required, not %r, %r" % (low_freq, high_freq))
    mel_low, mel_high = 1127.0 * np.log(1.0 + low / 700.0), 1127.0 * np.log(1.0 + high / 700.0)
    delta = (mel_high - mel_low) / (int(n_mels) + 1)
    q = np.arange(int(n_mels), dtype=np.float64)[:, None]
    left, centre, right = mel_low + q * delta, mel_low + (q + 1.0) * delta, mel_low + (q + 2.0) * delta
    m = 1127.0 * np.log(1.0 + np.arange(int(n_fft) // 2, dtype=np.float64) * (sample_rate / int(n_fft)) / 700.0)[None, :]
    w = np.where(m <= centre, (m - left) / (centre - left), (right - m) / (right - centre))
    w = np.where((m > left) & (m < right), w, 0.0)
    return np.concatenate([w, np.zeros((int(n_mels), 1))], axis=1).astype(np.float32)


def _spec_params(n_fft, hop, win_length, window, mel):
    """(win_length, the mel matrix as contiguous float32 or None), or ValueError for what lw_spec_create refuses"""
    for name, v, lo, hi in (("n_fft", n_fft, 2, SPEC_MAX_FFT), ("hop", hop, 1, 65535)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not lo <= v <= hi:
            raise ValueError("%s=%r: an integer in %d .. %d" % (name, v, lo, hi))
    if win_length is None:
        win_length = n_fft
    if isinstance(win_length, bool) or not isinstance(win_length, (int, np.integer)) or not 1 <= win_length <= n_fft:
        raise ValueError("win_length=%r: an integer in 1 .. n_fft" % (win_length,))
    if window not in _SPEC_WINDOWS:
        raise ValueError("window=%r: one of %s" % (window, ", ".join(sorted(_SPEC_WINDOWS))))
    if window not in ("hann", "rect") and win_length < 2:
        raise ValueError("window=%r needs win_length >= 2" % (window,))
    if mel is not None:
        mel = np.ascontiguousarray(mel, np.float32)
        if mel.ndim != 2 or mel.shape[1] != n_fft // 2 + 1 or not 1 <= mel.shape[0] <= SPEC_MAX_MELS:
            raise ValueError("mel= must be [n_mels <= %d][n_fft // 2 + 1 = %d], not %r" % (SPEC_MAX_MELS, n_fft // 2 + 1, mel.shape))
    return int(win_length), mel


class Spectrogram(_Handle):
    """lw_spec: rows of f32 PCM -> power spectrum or mel features on the GPU (k_spec), by the windowed DFT of
    include/lewton_amd.h ("spectral frames of rows"), a contract on bits.  window: "hann" (periodic), "rect", or the symmetric
    (i / (win_length - 1)) "povey", "hamming_sym", "hann_sym", "blackman_sym"; win_length: n_fft when None; mel: None for the power spectrum [n_fft // 2 + 1 lines], or a matrix [n_mels][n_fft // 2 + 1] (mel_filterbank).
    pad_mode: what a centred frame sees beyond the row, "zero" (+0.0) or "reflect" (x[-i], x[2 (len - 1) - i]: torch.stft's
    default; centred objects only, and run() then refuses a row of 0 < len < n_fft - n_fft // 2 + 1 samples).
    framing: "stft" (the rule above), or "kaldi": frames are counted by the window, which starts at sample 0 of the frame
    (center must then be False and pad_mode "zero"); snip_edges=True drops the incomplete tail, False centres the frames and
    reflects the row with the edge sample repeated (run() then refuses a row too short for one reflection).  preemphasis (0 .. 1)
    and scale (> 0; Kaldi's sample range is 32768) are folded into the table; remove_dc subtracts every frame's mean from it;
    energy puts the frame's energy (after remove_dc, before pre-emphasis and window, times scale^2) in line 0, the other lines
    behind it.  output: "power", or "complex": 2 * bins lines, re[j] on line j and im[j] on line bins + j, the chains themselves
    (as_complex() makes the complex tensor; InverseSpectrogram reads the lines as they are); not with mel=, remove_dc or energy.  Parameter errors are ValueError and need no GPU; the object itself lives on cuda:device."""

    _C = "lw_spec"

    def __init__(self, n_fft=400, hop=160, win_length=None, window="hann", center=True, mel=None, device=0, pad_mode="zero",
                 framing="stft", snip_edges=True, preemphasis=0.0, remove_dc=False, energy=False, scale=1.0, output="power"):
        self.win_length, self._mel = _spec_params(n_fft, hop, win_length, window, mel)
        if output not in _SPEC_OUTPUTS:
            raise ValueError("output=%r: \"power\" or \"complex\"" % (output,))
        if output == "complex" and (mel is not None or remove_dc or energy):
            raise ValueError("output=\"complex\" stores the chains themselves: not with mel=, remove_dc or energy")
        self.output = output
        if pad_mode not in _SPEC_PAD_MODES or (pad_mode == "reflect" and not center):
            raise ValueError("pad_mode=%r: \"zero\", or \"reflect\" with center=True" % (pad_mode,))
        if framing not in ("stft", "kaldi") or snip_edges not in (True, False, 0, 1):
            raise ValueError("framing=%r: \"stft\" or \"kaldi\", with snip_edges True or False" % (framing,))
        if framing == "kaldi" and (center or pad_mode != "zero"):
            raise ValueError("framing=\"kaldi\" needs center=False and pad_mode=\"zero\": snip_edges decides what a frame sees")
        if remove_dc not in (True, False, 0, 1) or energy not in (True, False, 0, 1):
            raise ValueError("remove_dc and energy are True or False")
        try:
            preemphasis, scale = float(preemphasis), float(scale)
        except (TypeError, ValueError):
            raise ValueError("preemphasis and scale must be numbers")
        if not 0.0 <= preemphasis <= 1.0 or not (scale > 0.0 and np.isfinite(scale)):
            raise ValueError("preemphasis in 0 .. 1 and a positive finite scale are required")
        self.pad_mode, self.framing, self.snip_edges = pad_mode, framing, bool(snip_edges)
        self.preemphasis, self.scale, self.remove_dc, self.energy, self.window = preemphasis, scale, bool(remove_dc), bool(energy), window
        self.n_fft, self.hop, self.center, self.device = int(n_fft), int(hop), bool(center), device
        _gpu()
        n_mels = 0 if self._mel is None else self._mel.shape[0]
        p = N.SpecParams(self.n_fft, self.win_length, self.hop, n_mels, None if self._mel is None else self._mel.ctypes.data, _SPEC_WINDOWS[window],
                         int(self.center), _SPEC_FRAMINGS[framing, bool(snip_edges)], int(self.remove_dc), int(self.energy), 0, preemphasis, scale, _SPEC_OUTPUTS[output])
        self._create(device, C.byref(p), create="_create_ex")
        assert self.bins == self.n_fft // 2 + 1
        assert self.features == (2 * self.bins if output == "complex" else (n_mels or self.bins) + int(self.energy))
        if framing == "stft" and N.lw_spec_set_pad_mode(self._h, _SPEC_PAD_MODES[pad_mode]):
            self.close()
            raise ValueError("lw_spec_set_pad_mode refused pad_mode=%r" % (pad_mode,))

    @property
    def bins(self):
        return int(N.lw_spec_bins(self._h))

    @property
    def features(self):
        """lines per row and channel of the output: n_mels, or bins without a mel matrix, and one more with energy"""
        return int(N.lw_spec_features(self._h))

    @property
    def tile_frames(self):
        return int(N.lw_spec_tile_frames(self._h))

    def frames(self, n):
        """frames of a row of n samples (lw_spec_frames)"""
        return int(N.lw_spec_frames(self._h, int(n)))

    def basis(self):
        """[2][win_length][bins] float32: C, then S, the window folded in"""
        out = np.empty((2, self.win_length, self.bins), np.float32)
        assert N.lw_spec_basis(self._h, None) == out.size
        N.lw_spec_basis(self._h, _array_ptr(out))
        return out

    @staticmethod
    def as_complex(t):
        """the complex tensor [..., B, frames] of an output="complex" result [..., 2 B, frames] (re lines, then im lines)"""
        import torch
        B = t.shape[-2] // 2
        return torch.complex(t[..., :B, :], t[..., B:, :])

    def last_route(self):
        """0: the DFT fold ran on the matrix cores, 1: per-lane fmaf chains, -1: no call yet (lw_spec_last_route)"""
        return N.lw_spec_last_route(self._h)

    def set_route(self, route):
        if N.lw_spec_set_route(self._h, int(route)):
            raise ValueError("lw_spec_set_route refused route %r" % (route,))

    def check_tensor(self, tensor, samples, what):
        """(n_rows, channels, row_capacity) of a source rows tensor, or ValueError: as Resampler.check_tensor"""
        return _pcm_shape(tensor, samples, what, self.device)

    def run(self, src, lengths, out=None, rows=None, stream=None, samples="f32", log=None, floor=1e-10):
        """lw_spec_rows: row i of src ([B, C, T], or [B, T, C] for samples="f32_interleaved"), lengths[i] samples per channel,
        -> row rows[i] of out (None: row i), float32 [rows][C][features][frame capacity], frames(lengths[i]) frames of each
        line; nothing else of out is written.  out=None: a zeroed tensor of max(rows) + 1 rows and the largest frame count.
        log: None, "ln" or "log10" -- log(max(x, floor)), applied by torch behind the kernel (plumbing: not part of the bit
        contract).  Only the written positions change, but the step is one torch.where over out[..., :max(frames)] that stores the
        other positions back unchanged: with log=, nothing else may read or write ANY row of out on another stream meanwhile.  stream: a hipStream_t value; None = torch's current stream on the object's
        device.  Asynchronous; returns (out, frames), frames an int64 host tensor with one count per row of src."""
        torch = _gpu()
        fmt = _FMT[samples]
        if fmt not in (N.FMT_F32_PLANAR, N.FMT_F32_INTERLEAVED):
            raise ValueError("the spectrogram works on the f32 formats, not %r" % (samples,))
        if log not in (None, "ln", "log10"):
            raise ValueError("log=%r: None, \"ln\" or \"log10\"" % (log,))
        n_src, ch, cap = self.check_tensor(src, samples, "src")
        lens = _row_counts(lengths, n_src, "lengths")
        frames = [self.frames(v) for v in lens.tolist()]
        rmap, n_dst = _row_map(rows, n_src)
        F = self.features
        if out is None:
            out = torch.zeros((n_dst, ch, F, max(frames, default=0)), dtype=torch.float32, device="cuda:%d" % self.device)
        _check_tensor(out, "out", "[rows][%d channels][%d features][frames]" % (ch, F), self.device, (torch.float32,), (4,))
        if out.shape[1] != ch or out.shape[2] != F:
            raise ValueError("out must be [rows][%d channels][%d features][frames], not %r" % (ch, F, tuple(out.shape)))
        n_dst, fcap = out.shape[0], out.shape[3]
        stream = _stream_of(stream, self.device)
        self._call(N.lw_spec_rows, fmt, ch, _tensor_ptr(src), n_src, cap, _array_ptr(lens), _array_ptr(rmap), _tensor_ptr(out), n_dst, fcap,
                   stream)
        if log is not None and n_dst and max(frames, default=0):
            per_row = [0] * n_dst
            for i, n in enumerate(frames):
                per_row[i if rmap is None else rmap[i]] = n
            with torch.cuda.stream(torch.cuda.ExternalStream(stream, device=self.device) if stream else torch.cuda.default_stream(self.device)):
                count = torch.tensor(per_row, dtype=torch.int64).to(out.device)
                part = out[:, :, :, :max(frames)]                        # no frame of this call lies beyond
                written = torch.arange(part.shape[3], device=out.device)[None, None, None, :] < count[:, None, None, None]
                x = torch.clamp(part, min=float(floor))
                part.copy_(torch.where(written, torch.log(x) if log == "ln" else torch.log10(x), part))
        return out, torch.tensor(frames, dtype=torch.int64)


class InverseSpectrogram(_Handle):
    """lw_istft: complex spectral frames [rows][C][2 * bins][frames] (Spectrogram(output="complex")'s lines: re, then im) -> rows
    of f32 PCM on the GPU (k_istft), by the inverse DFT, overlap-add and envelope division of include/lewton_amd.h ("inverse
    spectral frames of rows"), a contract on bits; torch.istft's algorithm with the analysis window.  window, win_length and
    center as Spectrogram's; hop <= win_length and ceil(win_length / hop) <= 16.  Where the window envelope is not above 1e-11 a
    sample is +0.0 (torch raises).  Parameter errors are ValueError and need no GPU; the object itself lives on cuda:device."""

    _C = "lw_istft"

    def __init__(self, n_fft=400, hop=160, win_length=None, window="hann", center=True, device=0):
        self.win_length, _ = _spec_params(n_fft, hop, win_length, window, None)
        if hop > self.win_length or -(-self.win_length // hop) > ISTFT_MAX_OVERLAP:
            raise ValueError("hop=%r: at most win_length, and at least win_length / %d" % (hop, ISTFT_MAX_OVERLAP))
        self.n_fft, self.hop, self.center, self.window, self.device = int(n_fft), int(hop), bool(center), window, device
        _gpu()
        p = N.IstftParams(self.n_fft, self.win_length, self.hop, _SPEC_WINDOWS[window], int(self.center), 0)
        self._create(device, C.byref(p))
        assert self.bins == self.n_fft // 2 + 1

    @property
    def bins(self):
        return int(N.lw_istft_bins(self._h))

    @property
    def tile_frames(self):
        """m: a workgroup owns m * hop samples (lw_istft_tile_frames)"""
        return int(N.lw_istft_tile_frames(self._h))

    def set_tile_frames(self, m):
        if N.lw_istft_set_tile_frames(self._h, int(m)):
            raise ValueError("lw_istft_set_tile_frames refused m=%r" % (m,))

    def out_len(self, frames):
        """the natural length of a row of `frames` frames (lw_istft_out_len)"""
        return int(N.lw_istft_out_len(self._h, int(frames)))

    def basis(self):
        """[2 * bins][win_length] float32: the cosine lines, then the sine lines, window and 1 / n_fft folded in"""
        out = np.empty((2 * self.bins, self.win_length), np.float32)
        assert N.lw_istft_basis(self._h, None) == out.size
        N.lw_istft_basis(self._h, _array_ptr(out))
        return out

    def window2(self):
        """[win_length] float64: the squared window the envelope is folded from"""
        out = np.empty(self.win_length, np.float64)
        assert N.lw_istft_window2(self._h, None) == out.size
        N.lw_istft_window2(self._h, _array_ptr(out))
        return out

    def last_route(self):
        """0: the frame signals ran on the matrix cores, 1: per-lane fmaf chains, -1: no call yet (lw_istft_last_route)"""
        return N.lw_istft_last_route(self._h)

    def set_route(self, route):
        if N.lw_istft_set_route(self._h, int(route)):
            raise ValueError("lw_istft_set_route refused route %r" % (route,))

    def run(self, spec, frames, lengths=None, out=None, rows=None, stream=None, samples="f32"):
        """lw_istft_rows: row i of spec (float32 [B, C, 2 * bins, frame capacity], frames[i] frames) -> row rows[i] of out (None:
        row i), [rows][C][T] or, for samples="f32_interleaved", [rows][T][C]; lengths[i] samples of it are written (None: the
        natural lengths, out_len(frames[i])), +0.0 behind what the frames cover; nothing else of out is written.  out=None: a
        zeroed tensor of max(rows) + 1 rows and the largest length.  stream: a hipStream_t value; None = torch's current stream
        on the object's device.  Asynchronous; returns (out, lengths), lengths an int64 host tensor with one entry per row of spec."""
        torch = _gpu()
        fmt = _FMT[samples]
        if fmt not in (N.FMT_F32_PLANAR, N.FMT_F32_INTERLEAVED):
            raise ValueError("the inverse spectrogram writes the f32 formats, not %r" % (samples,))
        _check_tensor(spec, "spec", "[rows][channels][%d lines][frames]" % (2 * self.bins), self.device, (torch.float32,), (4,))
        if spec.shape[2] != 2 * self.bins:
            raise ValueError("spec must be [rows][channels][%d lines][frames], not %r" % (2 * self.bins, tuple(spec.shape)))
        n_src, ch, _, fcap = spec.shape
        T = _row_counts(frames, n_src, "frames")
        if lengths is None:
            lens = np.asarray([self.out_len(v) for v in T.tolist()], np.uint64)
        else:
            lens = _row_counts(lengths, n_src, "lengths")
        rmap, n_dst = _row_map(rows, n_src)
        itl = N.fmt_interleaved(fmt)
        if out is None:
            cap = max(lens.tolist(), default=0)
            out = torch.zeros((n_dst, cap, ch) if itl else (n_dst, ch, cap), dtype=torch.float32, device="cuda:%d" % self.device)
        n_dst, och, cap = _pcm_shape(out, samples, "out", self.device)
        if och != ch:
            raise ValueError("out has %d channels, spec %d" % (och, ch))
        self._call(N.lw_istft_rows, ch, _tensor_ptr(spec), n_src, fcap, _array_ptr(T), _array_ptr(rmap), _array_ptr(lens), fmt,
                   _tensor_ptr(out), n_dst, cap, _stream_of(stream, self.device))
        return out, torch.tensor(lens.tolist(), dtype=torch.int64)


_FEAT_LOGS = {None: 0, "none": 0, "ln": 1, "log10": 2, "db": 3}      # LW_FEAT_LOG_*
_FEAT_SCOPES = {"row": 0, "channel": 1}                             # LW_FEAT_SCOPE_*


def _feat_params(log, floor, top, add, mul, scope):
    """(log kind, scope, the four numbers as float32), or ValueError for what lw_feat_create refuses"""
    if log not in _FEAT_LOGS:
        raise ValueError("log=%r: None, \"ln\", \"log10\" or \"db\"" % (log,))
    if scope not in _FEAT_SCOPES:
        raise ValueError("scope=%r: \"row\" or \"channel\"" % (scope,))
    try:
        with np.errstate(over="ignore"):
            floor, top, add, mul = (np.float32(v) for v in (floor, top, add, mul))
    except (TypeError, ValueError):
        raise ValueError("floor, top, add and mul must be numbers")
    if np.isnan(floor) or (_FEAT_LOGS[log] and not (floor > 0 and np.isfinite(floor))):
        raise ValueError("floor=%r: a positive finite float32 under a logarithm, never NaN" % (floor,))
    if np.isnan(top) or top < 0:
        raise ValueError("top=%r: non-negative (inf: no clamp)" % (top,))
    if np.isnan(add) or np.isnan(mul):
        raise ValueError("add and mul must not be NaN")
    return _FEAT_LOGS[log], _FEAT_SCOPES[scope], floor, top, add, mul


class LogCompress(_Handle):
    """lw_feat: finishes feature rows [rows][C][F][frame capacity] (Spectrogram.run's output) on the GPU (k_feat), by the rule of
    include/lewton_amd.h ("finishing feature rows"), a contract on bits: v = max(x, floor) (a NaN becomes the floor), l = LOG(v)
    in specified double arithmetic (log: None, "ln", "log10", "db"), M = the largest l of the scope ("row": all channels and lines
    of the row; "channel"), y = max(l, M - top) (top=inf: no clamp), z = (y + add) * mul.  The defaults are Whisper's.  Parameter
    errors are ValueError and need no GPU; the object itself lives on cuda:device."""

    _C = "lw_feat"
    WHISPER = dict(log="log10", floor=1e-10, top=8.0, add=4.0, mul=0.25, scope="row")

    def __init__(self, log="log10", floor=1e-10, top=8.0, add=4.0, mul=0.25, scope="row", device=0):
        kind, sc, floor, top, add, mul = _feat_params(log, floor, top, add, mul, scope)
        self.log_kind, self.scope, self.device = log, scope, device
        self.floor, self.top, self.add, self.mul = float(floor), float(top), float(add), float(mul)
        _gpu()
        p = N.FeatParams(kind, sc, floor, top, add, mul)
        self._create(device, C.byref(p))

    @classmethod
    def whisper(cls, device=0):
        """log10, floor 1e-10, clamp 8 below the row's maximum, (x + 4) / 4"""
        return cls(device=device, **cls.WHISPER)

    def log(self, v):
        """the contract's LOG of one float32 value, evaluated on the host (lw_feat_log)"""
        return float(N.lw_feat_log(self._h, float(np.float32(v))))

    def last_launches(self):
        """kernels the last call queued: 2, or 1 when nothing needs the maximum; -1: no call yet (lw_feat_last_launches)"""
        return N.lw_feat_last_launches(self._h)

    def run(self, feat, frames, out=None, fill_to=None, want_max=False, stream=None):
        """lw_feat_rows: frames[i] frames of every line of row i of feat (float32 [rows][C][F][frame capacity]) -> the same
        positions of out (None: feat itself, in place; otherwise a tensor of feat's shape).  fill_to: None, one count for all rows
        or one per row -- positions [frames[i], fill_to[i]) of every line receive what x = floor gives.  Nothing else of out is
        written.  want_max: also return M, float32 [rows] (scope "row") or [rows][C].  stream: a hipStream_t value; None = torch's
        current stream on the object's device.  Asynchronous; returns out, or (out, M)."""
        torch = _gpu()
        if out is None:
            out = feat
        for t, what in ((feat, "feat"), (out, "out")):
            _check_tensor(t, what, "[rows][C][F][frames]", self.device, (torch.float32,), (4,))
        if tuple(out.shape) != tuple(feat.shape):
            raise ValueError("out must have feat's shape %r, not %r" % (tuple(feat.shape), tuple(out.shape)))
        n_rows, ch, F, cap = feat.shape
        counts, fill = _row_counts(frames, n_rows, "frames"), _row_fill(fill_to, n_rows)
        mx = None
        if want_max:
            mx = torch.empty((n_rows,) if self.scope == "row" else (n_rows, ch), dtype=torch.float32, device=feat.device)
        self._call(N.lw_feat_rows, ch, F, _tensor_ptr(feat), _tensor_ptr(out), n_rows, cap, _array_ptr(counts), _array_ptr(fill),
                   _tensor_ptr(mx), _stream_of(stream, self.device))
        return (out, mx) if want_max else out


_NORM_SCALES = {None: 0, "none": 0, "std": 1, "rms": 2, "peak": 3}       # LW_NORM_SCALE_*
_NORM_SCOPES = {"row": 0, "channel": 1, "line": 2}                    # LW_NORM_SCOPE_*


def _norm_params(center, scale, eps, target, scope):
    """(center, scale kind, scope, eps, target), or ValueError for what lw_norm_create refuses"""
    if scale not in _NORM_SCALES:
        raise ValueError("scale=%r: None, \"std\", \"rms\" or \"peak\"" % (scale,))
    if scope not in _NORM_SCOPES:
        raise ValueError("scope=%r: \"row\", \"channel\" or \"line\"" % (scope,))
    if center not in (True, False, 0, 1):
        raise ValueError("center=%r: True or False" % (center,))
    try:
        eps, target = float(eps), float(target)
    except (TypeError, ValueError):
        raise ValueError("eps and target must be numbers")
    if not (eps >= 0.0 and np.isfinite(eps)):
        raise ValueError("eps=%r: non-negative and finite" % (eps,))
    if _NORM_SCALES[scale] >= 2 and not (target > 0.0 and np.isfinite(target)):
        raise ValueError("target=%r: positive and finite under \"rms\" and \"peak\"" % (target,))
    return int(bool(center)), _NORM_SCALES[scale], _NORM_SCOPES[scope], eps, target


class Normalize(_Handle):
    """lw_norm: normalises rows [rows][C][capacity] (waveforms) or [rows][C][F][capacity] (features) on the GPU (k_norm), by the
    rule of include/lewton_amd.h ("normalising rows"), a contract on bits with a fixed summation order: z = (x - m) * g in double,
    rounded once, with m the scope's mean (center) and g from its standard deviation ("std": 1 / sqrt(var + eps)), its RMS
    ("rms": target / sqrt(mean square + eps)) or its peak ("peak": target / max |x|); scale None: g = 1.  scope: "row" (all channels
    and lines of a row), "channel" or "line".  Parameter errors are ValueError and need no GPU; the object itself lives on
    cuda:device."""

    _C = "lw_norm"

    def __init__(self, center=True, scale="std", eps=1e-7, target=1.0, scope="row", device=0):
        c, kind, sc, eps, target = _norm_params(center, scale, eps, target, scope)
        self.center, self.scale, self.scope, self.eps, self.target, self.device = bool(c), scale, scope, eps, target, device
        _gpu()
        p = N.NormParams(c, kind, sc, 0, eps, target)
        self._create(device, C.byref(p))

    @classmethod
    def wav2vec2(cls, device=0):
        """(x - mean) / sqrt(var + 1e-7) over each channel of an utterance: wav2vec 2.0, HuBERT, WavLM, data2vec"""
        return cls(True, "std", 1e-7, 1.0, "channel", device)

    @classmethod
    def cmvn(cls, variance=True, eps=1e-20, device=0):
        """utterance CMVN: every feature line has its mean over time removed, and (variance) its deviation scaled to 1"""
        return cls(True, "std" if variance else None, eps, 1.0, "line", device)

    @classmethod
    def peak(cls, target=1.0, device=0):
        """the row's largest |x| becomes target; nothing is centred"""
        return cls(False, "peak", 0.0, target, "row", device)

    @classmethod
    def rms(cls, target, device=0):
        """the row's RMS becomes target; nothing is centred"""
        return cls(False, "rms", 0.0, target, "row", device)

    def scalars(self, S1, S2, P, N_):
        """step 3 of the contract on the host (lw_norm_scalars): (m, g) of a scope with sums S1, S2, peak P and N_ elements"""
        m, g = C.c_double(0), C.c_double(0)
        N.lw_norm_scalars(self._h, float(S1), float(S2), float(np.float32(P)), int(N_), C.byref(m), C.byref(g))
        return m.value, g.value

    def last_launches(self):
        """kernels the last call queued: 3, or 1 without center and scale; -1: no call yet (lw_norm_last_launches)"""
        return N.lw_norm_last_launches(self._h)

    def run(self, x, lengths, out=None, fill_to=None, want_stats=False, stream=None):
        """lw_norm_rows: lengths[i] elements of every line of row i of x (float32 [rows][C][capacity] or [rows][C][F][capacity])
        -> the same positions of out (None: x itself, in place; otherwise a tensor of x's shape).  fill_to: None, one count for all
        rows or one per row -- positions [lengths[i], fill_to[i]) of every line receive 0.  Nothing else of out is written.
        want_stats: also return (m, g) per scope, float64 [rows][2] ("row"), [rows][C][2] or [rows][C][F][2] (without the F of a
        3-D x).  stream: a hipStream_t value; None = torch's current stream on the object's device.  Asynchronous; returns out, or
        (out, stats)."""
        torch = _gpu()
        if out is None:
            out = x
        for t, what in ((x, "x"), (out, "out")):
            _check_tensor(t, what, "[rows][C][capacity] or [rows][C][F][capacity]", self.device, (torch.float32,), (3, 4))
        if tuple(out.shape) != tuple(x.shape):
            raise ValueError("out must have x's shape %r, not %r" % (tuple(x.shape), tuple(out.shape)))
        n_rows, ch, cap = x.shape[0], x.shape[1], x.shape[-1]
        F = x.shape[2] if x.dim() == 4 else 1
        counts, fill = _row_counts(lengths, n_rows, "lengths"), _row_fill(fill_to, n_rows)
        stats = None
        if want_stats:
            shape = {"row": (n_rows, 2), "channel": (n_rows, ch, 2), "line": (n_rows, ch, F, 2) if x.dim() == 4 else (n_rows, ch, 2)}[self.scope]
            stats = torch.empty(shape, dtype=torch.float64, device=x.device)
        self._call(N.lw_norm_rows, ch, F, _tensor_ptr(x), _tensor_ptr(out), n_rows, cap, _array_ptr(counts), _array_ptr(fill),
                   _tensor_ptr(stats), _stream_of(stream, self.device))
        return (out, stats) if want_stats else out


SLIDE_MAX_WINDOW = 2048                                   # LW_SLIDE_MAX_WINDOW


def _slide_params(cmn_window, min_cmn_window, center, norm_vars):
    """(cmn_window, min_cmn_window, center, norm_vars) as integers, or ValueError for what lw_slide_create refuses"""
    for v, what in ((cmn_window, "cmn_window"), (min_cmn_window, "min_cmn_window")):
        if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)):
            raise ValueError("%s=%r: an integer" % (what, v))
    if not 1 <= min_cmn_window <= cmn_window <= SLIDE_MAX_WINDOW:
        raise ValueError("1 <= min_cmn_window <= cmn_window <= %d, not %r and %r" % (SLIDE_MAX_WINDOW, min_cmn_window, cmn_window))
    for v, what in ((center, "center"), (norm_vars, "norm_vars")):
        if not isinstance(v, (bool, np.bool_, int, np.integer)) or v not in (0, 1):
            raise ValueError("%s=%r: True or False" % (what, v))
    return int(cmn_window), int(min_cmn_window), int(bool(center)), int(bool(norm_vars))


class SlidingCMVN(_Handle):
    """lw_slide: Kaldi's apply-cmvn-sliding over feature rows [rows][C][F][capacity] on the GPU (k_slide), by the rule of
    include/lewton_amd.h ("sliding-window normalisation of feature rows"), a contract on bits with a fixed summation order: every
    frame minus the mean of a window of cmn_window frames around it (center) or of the cmn_window + 1 frames up to it, and with
    norm_vars divided by the window's deviation.  The arguments have torchaudio.functional.sliding_window_cmn's names and
    defaults; the x-vector recipes use SlidingCMVN(300, 100, center=True).  Parameter errors are ValueError and need no GPU; the
    object itself lives on cuda:device."""

    _C = "lw_slide"

    def __init__(self, cmn_window=600, min_cmn_window=100, center=False, norm_vars=False, device=0):
        W, m, c, nv = _slide_params(cmn_window, min_cmn_window, center, norm_vars)
        self.cmn_window, self.min_cmn_window, self.center, self.norm_vars, self.device = W, m, bool(c), bool(nv), device
        _gpu()
        p = N.SlideParams(W, m, c, nv)
        self._create(device, C.byref(p))

    def window(self, t, T):
        """rule 1 on the host (lw_slide_window): (start, end) of the window of frame t of a line of T frames"""
        s, e = C.c_uint64(0), C.c_uint64(0)
        if not 0 <= t < T or N.lw_slide_window(self._h, int(t), int(T), C.byref(s), C.byref(e)):
            raise ValueError("window(%r, %r): 0 <= t < T" % (t, T))
        return s.value, e.value

    @property
    def tile_frames(self):
        """frames of a line a workgroup owns (lw_slide_tile_frames)"""
        return N.lw_slide_tile_frames(self._h)

    def set_tile_frames(self, m):
        """a test's handle on the seams (lw_slide_set_tile_frames): a multiple of 16 in 16 .. 4096; the bits do not depend on it"""
        if N.lw_slide_set_tile_frames(self._h, int(m)):
            raise ValueError("tile_frames=%r: a multiple of 16 in 16 .. 4096" % (m,))

    def last_launches(self):
        """kernels the last call queued: 1 per 65535 rows, 0 when nothing was to be written; -1: no call yet"""
        return N.lw_slide_last_launches(self._h)

    def run(self, feats, frames, out=None, fill_to=None, stream=None):
        """lw_slide_rows: frames[i] frames of every line of row i of feats (float32 [rows][C][F][capacity]) -> the same positions of
        out (None: a zeroed tensor of feats' shape; never feats itself: neighbours are read, there is no in-place form).  fill_to:
        None, one count for all rows or one per row -- positions [frames[i], fill_to[i]) of every line receive 0.  Nothing else of
        out is written.  stream: a hipStream_t value; None = torch's current stream on the object's device.  Asynchronous; returns
        out."""
        torch = _gpu()
        if out is None:
            out = torch.zeros_like(feats)
        for t, what in ((feats, "feats"), (out, "out")):
            _check_tensor(t, what, "[rows][C][F][capacity]", self.device, (torch.float32,), (4,))
        if tuple(out.shape) != tuple(feats.shape):
            raise ValueError("out must have feats' shape %r, not %r" % (tuple(feats.shape), tuple(out.shape)))
        if out.data_ptr() == feats.data_ptr() and feats.numel():
            raise ValueError("out must not be feats: the pass has no in-place form")
        n_rows, ch, F, cap = feats.shape
        counts, fill = _row_counts(frames, n_rows, "frames"), _row_fill(fill_to, n_rows)
        self._call(N.lw_slide_rows, ch, F, _tensor_ptr(feats), _tensor_ptr(out), n_rows, cap, _array_ptr(counts), _array_ptr(fill),
                   _stream_of(stream, self.device))
        return out


class SelectFrames(_Handle):
    """lw_select: keeps the frames of feature rows [rows][C][F][capacity] that a mask marks and moves them to the front of every
    line on the GPU (k_select), by the rule of include/lewton_amd.h ("frame decisions and frame selection"): Kaldi's
    select-voiced-frames for any mask -- an energy VAD's, a neural VAD's, a silence trim.  Bit copies; the rest of every line up to
    max(frames, fill_to) is zeroed.  The kept counts stay on the device: the chain's next pass takes HOST counts, so the caller's
    counts.cpu() is the ONE synchronisation of the step.  Channels of a row may end up with different lengths: [B][C][F][cap]
    viewed as [B * C][1][F][cap] is the same memory, and counts.reshape(B * C) are the frames of its rows.  Parameter errors are
    ValueError and need no GPU; the object itself lives on cuda:device."""

    _C = "lw_select"

    def __init__(self, device=0):
        if isinstance(device, (bool, np.bool_)) or not isinstance(device, (int, np.integer)) or device < 0:
            raise ValueError("device=%r: a device number" % (device,))
        self.device = int(device)
        self._create(self.device)

    @property
    def tile_frames(self):
        """frames of a tile (lw_select_tile_frames)"""
        return N.lw_select_tile_frames(self._h)

    def set_tile_frames(self, m):
        """a test's handle on the seams (lw_select_set_tile_frames): a multiple of 256 in 256 .. 2048; the result does not depend on it"""
        if N.lw_select_set_tile_frames(self._h, int(m)):
            raise ValueError("tile_frames=%r: a multiple of 256 in 256 .. 2048" % (m,))

    def last_launches(self):
        """kernels the last call queued: 2 per 65535 rows, 1 where no row has a frame, 0 when nothing was to be written; -1: no
        call yet"""
        return N.lw_select_last_launches(self._h)

    def run(self, feats, frames, mask, out=None, fill_to=None, stream=None):
        """lw_select_rows: of the frames[i] frames of row i of feats (float32 [rows][C][F][capacity]), those whose mask (torch.bool or
        uint8 [rows][C][capacity]) is set -> the front of every line of out (None: a zeroed tensor of feats' shape; never feats
        itself), K of them per row and channel; positions [K, max(frames[i], fill_to[i])) of every line receive 0.  fill_to: None,
        one count for all rows or one per row.  Nothing else of out is written.  stream: a hipStream_t value; None = torch's
        current stream on the object's device.  Asynchronous; returns (out, counts), counts a torch.int64 [rows][C] tensor ON THE
        DEVICE that holds K once the stream has reached it."""
        torch = _gpu()
        if out is None:
            out = torch.zeros_like(feats)
        for t, what in ((feats, "feats"), (out, "out")):
            _check_tensor(t, what, "[rows][C][F][capacity]", self.device, (torch.float32,), (4,))
        if tuple(out.shape) != tuple(feats.shape):
            raise ValueError("out must have feats' shape %r, not %r" % (tuple(feats.shape), tuple(out.shape)))
        if out.data_ptr() == feats.data_ptr() and feats.numel():
            raise ValueError("out must not be feats: the pass has no in-place form")
        n_rows, ch, F, cap = feats.shape
        _check_tensor(mask, "mask", "[rows][C][capacity] = %r" % ((n_rows, ch, cap),), self.device, (torch.bool, torch.uint8),
                      shape=(n_rows, ch, cap))
        counts, fill = _row_counts(frames, n_rows, "frames"), _row_fill(fill_to, n_rows)
        kept = torch.empty((n_rows, ch), dtype=torch.int64, device=feats.device)
        self._call(N.lw_select_rows, ch, F, _tensor_ptr(feats), _tensor_ptr(mask), _tensor_ptr(out), _tensor_ptr(kept), n_rows, cap,
                   _array_ptr(counts), _array_ptr(fill), _stream_of(stream, self.device))
        return out, kept


VAD_MAX_CONTEXT, VAD_FUSED_MAX = 256, 16384               # LW_VAD_MAX_CONTEXT, LW_VAD_FUSED_MAX
VAD_ROUTES = {"auto": 0, "fused": 1, "split": 2}          # LW_VAD_ROUTE_*


def _vad_params(energy_threshold, energy_mean_scale, frames_context, proportion_threshold, line, device):
    """the parameters as (float32, float32, int, float32, int, int), or ValueError for what lw_vad_create refuses"""
    vals = []
    for v, what in ((energy_threshold, "energy_threshold"), (energy_mean_scale, "energy_mean_scale"), (proportion_threshold, "proportion_threshold")):
        if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, float, np.integer, np.floating)):
            raise ValueError("%s=%r: a number" % (what, v))
        with np.errstate(over="ignore"):
            vals.append(np.float32(v))
    thr, scale, prop = vals
    if not np.isfinite(thr):
        raise ValueError("energy_threshold=%r: finite as a float32" % (energy_threshold,))
    if not np.isfinite(scale) or scale < 0:
        raise ValueError("energy_mean_scale=%r: finite and not negative" % (energy_mean_scale,))
    if not 0 < prop < 1:
        raise ValueError("proportion_threshold=%r: strictly inside (0, 1) as a float32" % (proportion_threshold,))
    for v, what in ((frames_context, "frames_context"), (line, "line"), (device, "device")):
        if not _is_int(v) or v < 0:
            raise ValueError("%s=%r: a non-negative integer" % (what, v))
    if frames_context > VAD_MAX_CONTEXT:
        raise ValueError("frames_context=%r: at most %d" % (frames_context, VAD_MAX_CONTEXT))
    if line > 65534:
        raise ValueError("line=%r: a feature line, below 65535" % (line,))
    return thr, scale, int(frames_context), prop, int(line), int(device)


class EnergyVad(_Handle):
    """lw_vad: Kaldi's compute-vad-energy over feature rows [rows][C][F][capacity] on the GPU (k_vad), by the rule of
    include/lewton_amd.h ("energy voice-activity decisions of feature rows"), a contract on bits: a frame's raw decision is its log
    energy (feature line `line`) above energy_threshold + energy_mean_scale * the line's mean, and a frame is voiced when at least
    proportion_threshold of the raw decisions within frames_context frames of it are set.  The arguments are Kaldi's options without
    their vad_ prefix, with Kaldi's defaults, positional in Kaldi's order: EnergyVad(5.5, 0.5, 2, 0.12) is the SRE recipes' vad.conf.
    Run it on the RAW features, before SlidingCMVN; the mask goes straight into SelectFrames.run, with no synchronisation in
    between.  Parameter errors are ValueError and need no GPU; the object itself lives on cuda:device."""

    _C = "lw_vad"

    def __init__(self, energy_threshold=5.0, energy_mean_scale=0.5, frames_context=0, proportion_threshold=0.6, line=0, device=0):
        thr, scale, ctx, prop, line, device = _vad_params(energy_threshold, energy_mean_scale, frames_context, proportion_threshold, line, device)
        self.energy_threshold, self.energy_mean_scale, self.frames_context, self.proportion_threshold = float(thr), float(scale), ctx, float(prop)
        self.line, self.device = line, device
        _gpu()
        p = N.VadParams(thr, scale, ctx, prop, line, 0)
        self._create(device, C.byref(p))

    def threshold(self, S, T):
        """rule 1 behind the sum, on the host (lw_vad_threshold): the float32 threshold of a line of T frames whose sum is S"""
        thr = C.c_float(0)
        if not _is_int(T) or T < 0 or N.lw_vad_threshold(self._h, float(S), int(T), C.byref(thr)):
            raise ValueError("threshold(%r, %r): T a non-negative frame count" % (S, T))
        return np.float32(thr.value)

    def voiced(self, num, den):
        """rule 3 on the host (lw_vad_voiced): whether num raw decisions of a window of den frames make the frame voiced"""
        if not _is_int(num) or not _is_int(den) or not 0 <= num <= den:
            raise ValueError("voiced(%r, %r): 0 <= num <= den" % (num, den))
        return N.lw_vad_voiced(self._h, int(num), int(den)) == 1

    @property
    def tile_frames(self):
        """frames of a tile (lw_vad_tile_frames)"""
        return N.lw_vad_tile_frames(self._h)

    def set_tile_frames(self, m):
        """a test's handle on the seams (lw_vad_set_tile_frames): a multiple of 256 in 256 .. 2048; the result does not depend on it"""
        if N.lw_vad_set_tile_frames(self._h, int(m)):
            raise ValueError("tile_frames=%r: a multiple of 256 in 256 .. 2048" % (m,))

    def set_route(self, route):
        """a test's handle on the two forms (lw_vad_set_route): "auto", "fused" (rows of at most 16384 frames) or "split"; the
        result does not depend on it"""
        if route not in VAD_ROUTES or N.lw_vad_set_route(self._h, VAD_ROUTES[route]):
            raise ValueError("route=%r: one of %s" % (route, ", ".join(sorted(VAD_ROUTES))))

    def last_launches(self):
        """kernels the last call queued: per 65535 rows 1 (fused, or energy_mean_scale == 0) or 3 (split); with no byte of the mask
        to write 1 for the thresholds when they are wanted, else 0; -1: no call yet"""
        return N.lw_vad_last_launches(self._h)

    def run(self, feats, frames, out=None, fill_to=None, stream=None, want_threshold=False):
        """lw_vad_rows: the decisions of the frames[i] frames of row i of feats (float32 [rows][C][F][capacity]) -> positions
        [0, frames[i]) of out (None: a zeroed tensor; else a contiguous uint8 or bool tensor [rows][C][capacity] on feats' device);
        positions [frames[i], fill_to[i]) receive 0.  fill_to: None, one count for all rows or one per row.  Nothing else of out is
        written.  stream: a hipStream_t value; None = torch's current stream on the object's device.  Asynchronous; returns the
        mask as a torch.bool [rows][C][capacity] view of out's bytes, and with want_threshold (mask, thr), thr a float32 [rows][C]
        device tensor of the thresholds."""
        torch = _gpu()
        _check_tensor(feats, "feats", "[rows][C][F][capacity]", self.device, (torch.float32,), (4,))
        n_rows, ch, F, cap = feats.shape
        if out is None:
            out = torch.zeros((n_rows, ch, cap), dtype=torch.uint8, device=feats.device)
        _check_tensor(out, "out", "[rows][C][capacity] = %r" % ((n_rows, ch, cap),), self.device, (torch.bool, torch.uint8),
                      shape=(n_rows, ch, cap))
        counts, fill = _row_counts(frames, n_rows, "frames"), _row_fill(fill_to, n_rows)
        thr = torch.empty((n_rows, ch), dtype=torch.float32, device=feats.device) if want_threshold else None
        self._call(N.lw_vad_rows, ch, F, _tensor_ptr(feats), _tensor_ptr(out), _tensor_ptr(thr), n_rows, cap, _array_ptr(counts),
                   _array_ptr(fill), _stream_of(stream, self.device))
        mask = out if out.dtype == torch.bool else out.view(torch.bool)
        return (mask, thr) if want_threshold else mask


SEG_MAX_SPAN = 1024                                       # LW_SEG_MAX_SPAN


def _device_number(device):
    if not _is_int(device) or device < 0:
        raise ValueError("device=%r: a device number" % (device,))
    return int(device)


class Segments(_Handle):
    """lw_segment: stretches of speech from a frame mask [rows][C][capacity] (EnergyVad's, a neural VAD's) on the GPU (k_segment), by
    the rule of include/lewton_amd.h ("segments of a frame mask"), pyannote's Binarize on integers: every set frame is padded by
    pad_onset frames to the front and pad_offset to the back (a Kaldi-style hangover is pad_offset alone), gaps of fewer than
    min_off frames between two set frames are filled, runs of fewer than min_on frames are dropped; the maximal runs of what remains
    are the segments.  All four are counts of frames, at most SEG_MAX_SPAN each.  Spans and counts stay on the device; jobs() is the
    ONE synchronisation of the step.  Parameter errors are ValueError and need no GPU; the object itself lives on cuda:device."""

    _C = "lw_segment"

    def __init__(self, pad_onset=0, pad_offset=0, min_off=0, min_on=0, device=0):
        for v, what in ((pad_onset, "pad_onset"), (pad_offset, "pad_offset"), (min_off, "min_off"), (min_on, "min_on")):
            if not _is_int(v) or not 0 <= v <= SEG_MAX_SPAN:
                raise ValueError("%s=%r: a count of frames in 0 .. %d" % (what, v, SEG_MAX_SPAN))
        self.pad_onset, self.pad_offset, self.min_off, self.min_on = int(pad_onset), int(pad_offset), int(min_off), int(min_on)
        self.device = _device_number(device)
        _gpu()
        p = N.SegmentParams(self.pad_onset, self.pad_offset, self.min_off, self.min_on, 0)
        self._create(self.device, C.byref(p))

    @property
    def tile_frames(self):
        """frames of a tile (lw_segment_tile_frames)"""
        return N.lw_segment_tile_frames(self._h)

    def set_tile_frames(self, m):
        """a test's handle on the seams (lw_segment_set_tile_frames): a multiple of 256 in 256 .. 2048; the result does not depend on it"""
        if N.lw_segment_set_tile_frames(self._h, int(m)):
            raise ValueError("tile_frames=%r: a multiple of 256 in 256 .. 2048" % (m,))

    def last_launches(self):
        """kernels the last call queued: per 65535 rows 2, or 1 where no row has a frame or only the smoothed mask is wanted; 0 when
        nothing was to be written; -1: no call yet"""
        return N.lw_segment_last_launches(self._h)

    def run(self, mask, frames, seg_capacity=None, want_mask=False, out_mask=None, fill_to=None, stream=None):
        """lw_segment_rows: the segments of the frames[i] frames of row i of mask (torch.bool or uint8 [rows][C][capacity]; any
        non-zero byte is set) -> spans, torch.int64 [rows][C][seg_capacity][2] ON THE DEVICE, (start, end) of segment k < K in
        frames, entries from K on unwritten (zero), and counts, torch.int64 [rows][C], the true K even where it exceeds
        seg_capacity.  seg_capacity=None: max(1, (capacity + 1) // 2), which no mask of capacity frames can exceed.  want_mask
        (or out_mask, a contiguous uint8 or bool tensor of mask's shape; never mask itself): also the smoothed mask as torch.bool,
        what SelectFrames takes -- selection with a hangover; its positions [frames[i], fill_to[i]) receive 0 (fill_to: None, one
        count for all rows or one per row), nothing else of it is written.  stream: a hipStream_t value; None = torch's current
        stream on the object's device.  Asynchronous; returns (spans, counts) or (spans, counts, smooth)."""
        torch = _gpu()
        _check_tensor(mask, "mask", "[rows][C][capacity]", self.device, (torch.bool, torch.uint8), (3,))
        n_rows, ch, cap = mask.shape
        if seg_capacity is None:
            seg_capacity = max(1, (cap + 1) // 2)
        if not _is_int(seg_capacity) or seg_capacity < 1:
            raise ValueError("seg_capacity=%r: a positive count of segments" % (seg_capacity,))
        counts, fill = _row_counts(frames, n_rows, "frames"), _row_fill(fill_to, n_rows)
        if out_mask is None and want_mask:
            out_mask = torch.zeros((n_rows, ch, cap), dtype=torch.uint8, device=mask.device)
        if out_mask is not None:
            _check_tensor(out_mask, "out_mask", "[rows][C][capacity] = %r" % ((n_rows, ch, cap),), self.device, (torch.bool, torch.uint8),
                          shape=(n_rows, ch, cap))
            if out_mask.data_ptr() == mask.data_ptr() and mask.numel():
                raise ValueError("out_mask must not be mask: the pass has no in-place form")
        spans = torch.zeros((n_rows, ch, int(seg_capacity), 2), dtype=torch.int64, device=mask.device)
        k = torch.empty((n_rows, ch), dtype=torch.int64, device=mask.device)
        self._call(N.lw_segment_rows, ch, _tensor_ptr(mask), _tensor_ptr(spans), _tensor_ptr(k), _tensor_ptr(out_mask), n_rows, cap, int(seg_capacity),
                   _array_ptr(counts), _array_ptr(fill), _stream_of(stream, self.device))
        if out_mask is None:
            return spans, k
        return spans, k, out_mask if out_mask.dtype == torch.bool else out_mask.view(torch.bool)

    @staticmethod
    def jobs(spans, counts, hop=1, window=0, lengths=None):
        """the ONE synchronisation of the step: copies spans and counts (run's results) to the host and returns (jobs, out_len) --
        jobs a numpy uint64 [n][3] array of (row, start, end) for CutRows.run, in ascending (row * C + c, k) order, where row is
        row * C + c: [B][C][..] read as [B * C][1][..], the same memory, as SelectFrames documents; out_len the n lengths
        end - start.  The spans are converted from frames to elements in Python integers: start * hop, and end * hop, or with
        lengths= (the elements of every row of what will be cut) min(lengths[row], (end - 1) * hop + window), the samples the
        segment's frames were computed from.  ValueError if any count exceeds seg_capacity.  Any policy beyond that -- splitting at
        30 s, grouping short segments into one window -- stays with the caller: the list is tiny, the caller is synchronised
        anyway, and jobs is a plain array to edit."""
        if not _is_int(hop) or hop < 1 or not _is_int(window) or window < 0:
            raise ValueError("hop=%r, window=%r: a positive and a non-negative count of elements" % (hop, window))
        sp, k = spans.cpu().numpy(), counts.cpu().numpy()
        if sp.ndim != 4 or sp.shape[3] != 2 or k.shape != sp.shape[:2]:
            raise ValueError("spans must be [rows][C][seg_capacity][2] and counts [rows][C], not %r and %r" % (sp.shape, k.shape))
        n_rows, ch, seg_cap = sp.shape[:3]
        if lengths is not None:
            lengths = [int(v) for v in (lengths.tolist() if hasattr(lengths, "tolist") else lengths)]
            if len(lengths) != n_rows or any(v < 0 for v in lengths):
                raise ValueError("lengths= needs one non-negative entry per row")
        if k.size and int(k.max()) > seg_cap:
            raise ValueError("%d segments in a row and channel, seg_capacity is %d" % (int(k.max()), seg_cap))
        jobs = []
        for r in range(n_rows):
            for c in range(ch):
                for a, b in sp[r, c, :int(k[r, c])].tolist():
                    end = b * hop if lengths is None else min(lengths[r], (b - 1) * hop + window)
                    jobs.append((r * ch + c, a * hop, max(end, a * hop)))
        jobs = np.asarray(jobs, np.uint64).reshape(len(jobs), 3)
        return jobs, (jobs[:, 2] - jobs[:, 1]).astype(np.int64)


_CUT_SAMPLES = {"f32": 4, "i16": 2}


class CutRows(_Handle):
    """lw_cut: one output row per job (row, start, end) over rows [rows][C][capacity] or [rows][C][F][capacity] of float32 or int16 on
    the GPU (k_cut), by the rule of include/lewton_amd.h ("cutting rows into segment rows"): bit copies, the rest of every line up
    to max(len, fill_to) zeroed -- the waveform or the features of every segment of Segments.jobs as a row of its own, in ONE
    launch.  Parameter errors are ValueError and need no GPU; the object itself lives on cuda:device."""

    _C = "lw_cut"

    def __init__(self, device=0):
        self.device = _device_number(device)
        self._create(self.device)

    def last_launches(self):
        """kernels the last call queued: 1 per 65535 jobs, 0 when nothing was to be written; -1: no call yet"""
        return N.lw_cut_last_launches(self._h)

    def run(self, src, lengths, jobs, out=None, fill_to=None, stream=None, samples="f32"):
        """lw_cut_rows: for job i = (row, start, end) of jobs (array-like [n][3]; 0 <= start <= end <= lengths[row]), elements
        [start, end) of every line of row `row` of src (samples="f32": float32, "i16": int16; [rows][C][capacity] or
        [rows][C][F][capacity]) -> the front of the lines of row i of out (None: a zeroed tensor [n][C]([F])[max(longest job,
        fill_to)]); positions [end - start, fill_to[i]) receive 0 (fill_to: None, one count for all jobs or one per job).  Nothing
        else of out is written.  A source whose channels were segmented apart is src.reshape(B * C, 1, ...), as Segments.jobs
        numbers its rows.  stream: a hipStream_t value; None = torch's current stream on the object's device.  Asynchronous;
        returns (out, out_len), out_len an int64 host tensor with end - start per job: the next pass's lengths."""
        torch = _gpu()
        if samples not in _CUT_SAMPLES:
            raise ValueError("samples=%r: \"f32\" or \"i16\"" % (samples,))
        dtype = torch.float32 if samples == "f32" else torch.int16
        _check_tensor(src, "src", "[rows][C][capacity] or [rows][C][F][capacity]", self.device, (dtype,), (3, 4))
        n_rows, ch = src.shape[:2]
        F, cap = (1, src.shape[2]) if src.dim() == 3 else (src.shape[2], src.shape[3])
        lens = _row_counts(lengths, n_rows, "lengths")
        try:
            jb = np.ascontiguousarray(np.asarray(jobs if len(jobs) else np.zeros((0, 3)), dtype=np.int64))
        except (TypeError, ValueError, OverflowError):
            raise ValueError("jobs= must be [n][3] integers (row, start, end)")
        if jb.ndim != 2 or jb.shape[1] != 3 or (jb < 0).any():
            raise ValueError("jobs= must be [n][3] non-negative integers (row, start, end), not %r" % (jb.shape,))
        jb = jb.astype(np.uint64)
        n_out = jb.shape[0]
        fill = _row_fill(fill_to, n_out)
        out_len = (jb[:, 2].astype(np.int64) - jb[:, 1].astype(np.int64))
        if out is None:
            T = max(int(out_len.max()) if n_out else 0, int(fill.max()) if fill is not None and n_out else 0, 0)
            out = torch.zeros((n_out, ch, T) if src.dim() == 3 else (n_out, ch, F, T), dtype=dtype, device=src.device)
        _check_tensor(out, "out", "[jobs][C][F][capacity] (three dimensions when src has three)", self.device, (dtype,), (src.dim(),))
        if out.shape[0] != n_out or tuple(out.shape[1:-1]) != tuple(src.shape[1:-1]):
            raise ValueError("out must be %r + [capacity], not %r" % ((n_out,) + tuple(src.shape[1:-1]), tuple(out.shape)))
        self._call(N.lw_cut_rows, ch, F, _CUT_SAMPLES[samples], _tensor_ptr(src), n_rows, cap, _array_ptr(lens), _array_ptr(jb if n_out else None), n_out,
                   _tensor_ptr(out), out.shape[-1], _array_ptr(fill), _stream_of(stream, self.device))
        return out, torch.tensor(out_len.tolist(), dtype=torch.int64)


SPECAUG_MAX_MASKS, SPECAUG_MAX_WIDTH = 32, 65535          # LW_SPECAUG_MAX_MASKS, LW_SPECAUG_MAX_WIDTH


def _specaug_params(num_time_masks, time_mask_param, num_freq_masks, freq_mask_param, min_time, min_freq, p, per_channel, fill, seed, device):
    """(the fields of lw_specaug_params in the structure's order, device), or ValueError for what lw_specaug_create refuses"""
    from fractions import Fraction
    for v, what, most in ((num_time_masks, "num_time_masks", SPECAUG_MAX_MASKS), (num_freq_masks, "num_freq_masks", SPECAUG_MAX_MASKS),
                          (time_mask_param, "time_mask_param", SPECAUG_MAX_WIDTH), (freq_mask_param, "freq_mask_param", SPECAUG_MAX_WIDTH),
                          (min_time, "min_time", SPECAUG_MAX_WIDTH), (min_freq, "min_freq", SPECAUG_MAX_WIDTH), (seed, "seed", (1 << 64) - 1)):
        if not _is_int(v) or not 0 <= v <= most:
            raise ValueError("%s=%r: an integer in 0 .. %d" % (what, v, most))
    if min_time > time_mask_param or min_freq > freq_mask_param:
        raise ValueError("min_time=%r, min_freq=%r: at most time_mask_param=%r, freq_mask_param=%r" % (min_time, min_freq, time_mask_param, freq_mask_param))
    if isinstance(p, (bool, np.bool_)) or not isinstance(p, (int, float, np.integer, np.floating, Fraction)) or not 0 <= p <= 1:
        raise ValueError("p=%r: a share of the row's frames in [0, 1]" % (p,))
    ratio = (p if isinstance(p, Fraction) else Fraction(float(p))).limit_denominator(65535)
    num, den = (0, 0) if p == 1.0 else (ratio.numerator, ratio.denominator)      # 1.0: no limit from the row's length
    if not isinstance(per_channel, (bool, np.bool_)):
        raise ValueError("per_channel=%r: True or False" % (per_channel,))
    if isinstance(fill, (bool, np.bool_)) or not isinstance(fill, (int, float, np.integer, np.floating)):
        raise ValueError("fill=%r: a number" % (fill,))
    with np.errstate(over="ignore"):
        fill_bits = int(np.array(fill, np.float32).view(np.uint32))               # a float32 scalar keeps its own bits
    return (int(seed), int(num_time_masks), int(min_time), int(time_mask_param), num, den, int(num_freq_masks), int(min_freq), int(freq_mask_param),
            int(bool(per_channel)), fill_bits, 0), _device_number(device)


class SpecAugment(_Handle):
    """lw_specaug: SpecAugment's time and frequency masks (Park et al. 2019, without the time warp) over feature rows
    [rows][C][F][capacity] or waveforms [rows][C][capacity] on the GPU (k_specaug), by the rule of include/lewton_amd.h ("masking
    feature rows"), a contract on bits.  The masks of an utterance are a pure function of (seed, id): the same in any batch, at any
    row position, on any grid -- log the two numbers and the augmentation can be run again.  num_time_masks masks of min_time ..
    time_mask_param frames (none wider than p times the row's own frames; p = 1.0: no such limit) and num_freq_masks masks of
    min_freq .. freq_mask_param bins, each wholly inside the row (torchaudio's form); masked elements receive fill, bit for bit.
    per_channel: every channel draws masks of its own.  Parameter errors are ValueError and need no GPU; the object itself lives
    on cuda:device."""

    _C = "lw_specaug"

    def __init__(self, num_time_masks=2, time_mask_param=50, num_freq_masks=2, freq_mask_param=10, min_time=0, min_freq=0, p=1.0, per_channel=False,
                 fill=0.0, seed=0, device=0):
        fields, self.device = _specaug_params(num_time_masks, time_mask_param, num_freq_masks, freq_mask_param, min_time, min_freq, p, per_channel, fill,
                                              seed, device)
        self.seed, self.num_time_masks, self.num_freq_masks, self.per_channel = fields[0], fields[1], fields[6], bool(fields[9])
        _gpu()
        params = N.SpecAugParams(*fields)
        self._create(self.device, C.byref(params))

    @classmethod
    def paper(cls, policy="LD", **kw):
        """the LibriSpeech policies of the paper without their time warp: F = 27, T = 100, p = 1.0; "LB" one mask of each kind,
        "LD" two"""
        if policy not in ("LB", "LD"):
            raise ValueError("policy=%r: \"LB\" or \"LD\"" % (policy,))
        m = 1 if policy == "LB" else 2
        return cls(num_time_masks=m, time_mask_param=100, num_freq_masks=m, freq_mask_param=27, p=1.0, **kw)

    @classmethod
    def wenet(cls, **kw):
        """WeNet's spec_aug defaults: two time masks of 1 .. 50 frames and two frequency masks of 1 .. 10 bins (inside the row, where
        WeNet cuts a mask at the row's end)"""
        return cls(num_time_masks=2, time_mask_param=50, num_freq_masks=2, freq_mask_param=10, min_time=1, min_freq=1, **kw)

    @property
    def tile_frames(self):
        """frames of a tile (lw_specaug_tile_frames)"""
        return N.lw_specaug_tile_frames(self._h)

    def set_tile_frames(self, m):
        """a test's handle on the seams (lw_specaug_set_tile_frames): a multiple of 256 in 256 .. 2048; the result does not depend on it"""
        if not _is_int(m) or not 0 <= m < 1 << 32 or N.lw_specaug_set_tile_frames(self._h, int(m)):
            raise ValueError("tile_frames=%r: a multiple of 256 in 256 .. 2048" % (m,))

    def last_launches(self):
        """kernels the last call queued: 1 per 65535 rows, 0 when nothing could be written; -1: no call yet"""
        return N.lw_specaug_last_launches(self._h)

    def plan(self, id, T, F, group=0):
        """the rule on the host (lw_specaug_plan): [(start, end)] of the num_time_masks + num_freq_masks masks, time masks first, of
        group `group` (a channel with per_channel, else 0) of utterance id with T frames and F bins"""
        for v, what, most in ((id, "id", (1 << 64) - 1), (T, "T", (1 << 63) - 1), (F, "F", 65535), (group, "group", 65535)):
            if not _is_int(v) or not 0 <= v <= most:
                raise ValueError("%s=%r: an integer in 0 .. %d" % (what, v, most))
        n = self.num_time_masks + self.num_freq_masks
        spans = (C.c_int64 * (2 * n + 1))()
        self._call(N.lw_specaug_plan, int(id), int(group), int(T), int(F), spans)
        return [(spans[2 * i], spans[2 * i + 1]) for i in range(n)]

    def run(self, feats, frames, ids=None, out=None, fill_to=None, want_spans=False, stream=None):
        """lw_specaug_rows: the frames[i] frames of row i of feats (float32 [rows][C][F][capacity], or a waveform [rows][C][capacity]:
        F = 1) masked as utterance ids[i] (None: the row's index) -> out (None: IN PLACE, and feats is returned; else a tensor of
        feats' shape on its device); positions [frames[i], fill_to[i]) of every line receive 0 (fill_to: None, one count for all
        rows or one per row).  Nothing else of out is written; in place only the masked elements and the fill span are.  stream: a
        hipStream_t value; None = torch's current stream on the object's device.  Asynchronous; returns out, and with want_spans
        (out, spans), spans an int64 [rows][G][masks][2] device tensor of (start, end), G = C with per_channel, else 1."""
        torch = _gpu()
        _check_tensor(feats, "feats", "[rows][C][F][capacity] or [rows][C][capacity]", self.device, (torch.float32,), (3, 4))
        n_rows, ch = feats.shape[:2]
        F, cap = (1, feats.shape[2]) if feats.dim() == 3 else (feats.shape[2], feats.shape[3])
        if out is None:
            out = feats
        _check_tensor(out, "out", "of feats' shape %r" % (tuple(feats.shape),), self.device, (torch.float32,), shape=tuple(feats.shape))
        counts, fill = _row_counts(frames, n_rows, "frames"), _row_fill(fill_to, n_rows)
        if ids is not None:
            ids = [int(v) for v in (ids.tolist() if hasattr(ids, "tolist") else ids)]
            if len(ids) != n_rows or any(not 0 <= v < 1 << 64 for v in ids):
                raise ValueError("ids= needs one utterance id in 0 .. 2^64 - 1 per row")
            ids = np.asarray(ids, np.uint64)
        spans = None
        if want_spans:
            spans = torch.empty((n_rows, ch if self.per_channel else 1, self.num_time_masks + self.num_freq_masks, 2), dtype=torch.int64,
                                device=feats.device)
        self._call(N.lw_specaug_rows, ch, F, _tensor_ptr(feats), _tensor_ptr(out), n_rows, cap, _array_ptr(counts), _array_ptr(fill), _array_ptr(ids),
                   _tensor_ptr(spans), _stream_of(stream, self.device))
        return (out, spans) if want_spans else out


CEP_MAX_IN,CEP_MAX_OUT, CEP_MAX_WIDTH = 256, 256, 16     # LW_CEP_MAX_IN, LW_CEP_MAX_OUT, LW_CEP_MAX_WIDTH


def _is_int(v):
    return isinstance(v, (int, np.integer)) and not isinstance(v, bool)


def dct_matrix(n_out, n_in, norm="ortho", lifter=0):
    """[n_out][n_in] float32 DCT-II rows cos(pi q (2 f + 1) / (2 n_in)), computed in float64 and rounded once.  norm="ortho": scaled
    by sqrt(2 / n_in), row 0 by sqrt(1 / n_in); norm=None: by 2, as scipy and torchaudio.  lifter L > 0 folds the HTK lifter
    1 + (L / 2) sin(pi q / L) into row q.  Needs no GPU."""
    if not _is_int(n_in) or not 1 <= n_in <= CEP_MAX_IN:
        raise ValueError("n_in=%r: 1 .. %d" % (n_in, CEP_MAX_IN))
    if not _is_int(n_out) or not 1 <= n_out <= CEP_MAX_OUT:
        raise ValueError("n_out=%r: 1 .. %d" % (n_out, CEP_MAX_OUT))
    if norm not in (None, "ortho"):
        raise ValueError("norm=%r: None or \"ortho\"" % (norm,))
    try:
        lifter = float(lifter)
    except (TypeError, ValueError):
        raise ValueError("lifter must be a number")
    if not (lifter >= 0.0 and np.isfinite(lifter)):
        raise ValueError("lifter=%r: non-negative and finite (0: none)" % (lifter,))
    q = np.arange(int(n_out), dtype=np.float64)[:, None]
    f = np.arange(int(n_in), dtype=np.float64)[None, :]
    m = np.cos(np.pi * q * (2.0 * f + 1.0) / (2.0 * int(n_in)))
    if norm == "ortho":
        m = m * np.where(q == 0, np.sqrt(1.0 / int(n_in)), np.sqrt(2.0 / int(n_in)))
    else:
        m = m * 2.0
    if lifter:
        m = m * (1.0 + (lifter / 2.0) * np.sin(np.pi * q / lifter))
    return m.astype(np.float32)


def _cep_params(n_in, matrix, delta_order, delta_width):
    """(n_in, n_out, the matrix as contiguous float32 or None, order, width), or ValueError for what lw_cep_create refuses"""
    if not _is_int(n_in) or not 1 <= n_in <= CEP_MAX_IN:
        raise ValueError("n_in=%r: an integer in 1 .. %d" % (n_in, CEP_MAX_IN))
    if not _is_int(delta_order) or not 0 <= delta_order <= 2:
        raise ValueError("delta_order=%r: 0, 1 or 2" % (delta_order,))
    if delta_order and (not _is_int(delta_width) or not 1 <= delta_width <= CEP_MAX_WIDTH):
        raise ValueError("delta_width=%r: an integer in 1 .. %d" % (delta_width, CEP_MAX_WIDTH))
    n_out = int(n_in)
    if matrix is not None:
        try:
            matrix = np.ascontiguousarray(matrix, np.float32)
        except (TypeError, ValueError):
            raise ValueError("matrix= must be an array of numbers")
        if matrix.ndim != 2 or matrix.shape[1] != n_in or not 1 <= matrix.shape[0] <= CEP_MAX_OUT:
            raise ValueError("matrix= must be [n_out <= %d][n_in = %d], not %r" % (CEP_MAX_OUT, n_in, matrix.shape))
        n_out = matrix.shape[0]
    return int(n_in), n_out, matrix, int(delta_order), int(delta_width) if delta_order else 0


class Cepstrum(_Handle):
    """lw_cep: feature rows [rows][C][n_in][frame capacity] -> [rows][C][n_out * (1 + delta_order)][frame capacity] on the GPU
    (k_cep), by the rule of include/lewton_amd.h ("cepstra and deltas of feature rows"), a contract on bits: static line q is the
    fmaf chain over the input lines with row q of matrix ([n_out][n_in]; None: the identity, a bit copy), the next n_out lines
    are the regression deltas over +-delta_width frames with the edge frames replicated, the next n_out the deltas of those (HTK /
    Kaldi order; what torchaudio's compute_deltas applied twice gives).  Parameter errors are ValueError and need no GPU; the
    object itself lives on cuda:device."""

    _C = "lw_cep"

    def __init__(self, n_in, matrix=None, delta_order=0, delta_width=2, device=0):
        self.n_in, self.n_out, self._matrix, self.delta_order, self.delta_width = _cep_params(n_in, matrix, delta_order, delta_width)
        self.device = device
        self._create(device, self.n_in, self.n_out, _array_ptr(self._matrix), self.delta_order, self.delta_width)
        assert self.features == self.n_out * (1 + self.delta_order)

    @classmethod
    def mfcc(cls, n_mels, n_mfcc=13, norm="ortho", lifter=0, delta_order=0, delta_width=2, device=0):
        """the first n_mfcc DCT-II coefficients of n_mels log-mel lines (dct_matrix), with deltas on request"""
        return cls(n_mels, dct_matrix(n_mfcc, n_mels, norm, lifter), delta_order, delta_width, device)

    @classmethod
    def deltas(cls, n_in, order=2, width=2, device=0):
        """the lines themselves, bit for bit, then their deltas ("fbank + deltas")"""
        return cls(n_in, None, order, width, device)

    @property
    def features(self):
        """lines per row and channel of the output: n_out * (1 + delta_order)"""
        return int(N.lw_cep_features(self._h))

    @property
    def tile_frames(self):
        """the frames one workgroup produces (lw_cep_tile_frames)"""
        return int(N.lw_cep_tile_frames(self._h))

    def matrix(self):
        """[n_out][n_in] float32 as the kernel reads it; None for the identity"""
        n = int(N.lw_cep_matrix(self._h, None))
        if n == 0:
            return None
        out = np.empty((self.n_out, self.n_in), np.float32)
        assert n == out.size
        N.lw_cep_matrix(self._h, _array_ptr(out))
        return out

    def delta_weights(self):
        """w_1 .. w_N float32 (empty without deltas)"""
        out = np.empty(int(N.lw_cep_delta_weights(self._h, None)), np.float32)
        N.lw_cep_delta_weights(self._h, _array_ptr(out))
        return out

    def last_launches(self):
        """kernels the last call queued: 1 per 65535 rows, 0 when nothing was to be written; -1: no call yet"""
        return N.lw_cep_last_launches(self._h)

    def run(self, feat, frames, out=None, fill_to=None, stream=None):
        """lw_cep_rows: frames[i] frames of every line of row i of feat (float32 [rows][C][n_in][frame capacity]) -> the same
        frames of the features lines of out (None: a zeroed tensor [rows][C][features][frame capacity]; it must not overlap feat).
        fill_to: None, one count for all rows or one per row -- positions [frames[i], fill_to[i]) of every line of out receive 0.
        Nothing else of out is written.  stream: a hipStream_t value; None = torch's current stream on the object's device.
        Asynchronous; returns out."""
        torch = _gpu()
        _check_tensor(feat, "feat", "[rows][C][%d][frames]" % self.n_in, self.device, (torch.float32,), (4,))
        if feat.shape[2] != self.n_in:
            raise ValueError("feat must be [rows][C][%d][frames], not %r" % (self.n_in, tuple(feat.shape)))
        n_rows, ch, _, cap = feat.shape
        if out is None:
            out = torch.zeros((n_rows, ch, self.features, cap), dtype=torch.float32, device=feat.device)
        shape = (n_rows, ch, self.features, cap)
        _check_tensor(out, "out", "[rows][C][features][frames] = %r" % (shape,), self.device, (torch.float32,), shape=shape)
        counts, fill = _row_counts(frames, n_rows, "frames"), _row_fill(fill_to, n_rows)
        self._call(N.lw_cep_rows, ch, _tensor_ptr(feat), _tensor_ptr(out), n_rows, cap, _array_ptr(counts), _array_ptr(fill),
                   _stream_of(stream, self.device))
        return out


FLT_EPSILON = float(np.finfo(np.float32).eps)      # Kaldi's floor under the logarithm


class KaldiFbank:
    """Kaldi's filterbank front end on the GPU: what torchaudio.compliance.kaldi.fbank and kaldi-native-fbank compute, as the chain
    Spectrogram(framing="kaldi", ...) -> LogCompress("ln", floor=FLT_EPSILON, top=inf, add=0, mul=1) in place -> (use_energy and
    energy_floor > 0) line 0 clamped at ln(energy_floor) by torch -> (subtract_mean) Normalize.cmvn(variance=False).  Argument
    names and defaults are torchaudio's; a value this front end does not offer is a ValueError: dither != 0, htk_compat,
    raw_energy=False, use_power=False, use_log_fbank=False, vtln_warp != 1, blackman_coeff != 0.42, channel != -1 (every channel of
    a row is processed), min_duration != 0.  scale (not torchaudio's): what the samples are multiplied by, 32768 where a model was
    trained on Kaldi's 16-bit sample range.  frame_length and frame_shift are milliseconds.

    The output is the chain's [row][ch][F][frame], F = num_mel_bins (+ 1 with use_energy, the energy in line 0), NOT torchaudio's
    [frame][F]: out[r, c].T is what torchaudio returns for channel c of row r."""

    def __init__(self, blackman_coeff=0.42, channel=-1, dither=0.0, energy_floor=1.0, frame_length=25.0, frame_shift=10.0, high_freq=0.0,
                 htk_compat=False, low_freq=20.0, min_duration=0.0, num_mel_bins=23, preemphasis_coefficient=0.97, raw_energy=True,
                 remove_dc_offset=True, round_to_power_of_two=True, sample_frequency=16000.0, snip_edges=True, subtract_mean=False,
                 use_energy=False, use_log_fbank=True, use_power=True, vtln_high=-500.0, vtln_low=100.0, vtln_warp=1.0, window_type="povey",
                 scale=1.0, device=0):
        for name, v, only in (("dither", dither, 0.0), ("htk_compat", htk_compat, False), ("raw_energy", raw_energy, True), ("use_power", use_power, True),
                              ("use_log_fbank", use_log_fbank, True), ("vtln_warp", vtln_warp, 1.0), ("blackman_coeff", blackman_coeff, 0.42),
                              ("channel", channel, -1), ("min_duration", min_duration, 0.0)):
            if v != only:
                raise ValueError("%s=%r is not offered (only %r)" % (name, v, only))
        windows = {"povey": "povey", "hamming": "hamming_sym", "hanning": "hann_sym", "rectangular": "rect", "blackman": "blackman_sym"}
        if window_type not in windows:
            raise ValueError("window_type=%r: one of %s" % (window_type, ", ".join(sorted(windows))))
        try:
            sample_frequency, energy_floor = float(sample_frequency), float(energy_floor)
            win = int(sample_frequency * float(frame_length) * 0.001)
            hop = int(sample_frequency * float(frame_shift) * 0.001)
        except (TypeError, ValueError, OverflowError):
            raise ValueError("sample_frequency, frame_length, frame_shift and energy_floor must be finite numbers")
        if win < 2 or hop < 1:
            raise ValueError("frame_length and frame_shift give a window of %d and a shift of %d samples" % (win, hop))
        n_fft = 1 << (win - 1).bit_length() if round_to_power_of_two else win
        if not energy_floor >= 0.0:
            raise ValueError("energy_floor=%r: non-negative" % (energy_floor,))
        self.use_energy, self.subtract_mean, self.energy_floor, self.device = bool(use_energy), bool(subtract_mean), energy_floor, device
        self.banks = kaldi_mel_banks(sample_frequency, n_fft, num_mel_bins, low_freq, high_freq)
        self.spec = Spectrogram(n_fft, hop, win, windows[window_type], center=False, mel=self.banks, device=device, framing="kaldi",
                                snip_edges=snip_edges, preemphasis=preemphasis_coefficient, remove_dc=bool(remove_dc_offset),
                                energy=self.use_energy, scale=scale)
        self.log = self.norm = None
        try:
            self.log = LogCompress("ln", floor=FLT_EPSILON, top=float("inf"), add=0.0, mul=1.0, device=device)
            if self.subtract_mean:
                self.norm = Normalize.cmvn(variance=False, device=device)
        except Exception:
            self.close()
            raise

    def close(self):
        for part in (getattr(self, "spec", None), getattr(self, "log", None), getattr(self, "norm", None)):
            if part is not None:
                part.close()

    @property
    def features(self):
        return self.spec.features

    def frames(self, n):
        return self.spec.frames(n)

    def run(self, pcm, lengths, out=None, fill_to=None, samples="f32", stream=None):
        """row i of pcm ([B, C, T] float32, or [B, T, C] for samples="f32_interleaved"), lengths[i] samples per channel -> row i
        of out, float32 [B][C][F][frame capacity] (None: a zeroed tensor that holds the largest frame count and fill_to).
        fill_to: None, one count for all rows or one per row: positions [frames[i], fill_to[i]) of every line receive
        ln(FLT_EPSILON), Kaldi's lowest value, or 0 with subtract_mean.  Asynchronous; returns (out, frames)."""
        torch = _gpu()
        if out is None:
            n_src, ch, _ = self.spec.check_tensor(pcm, samples, "pcm")
            lens, fill = _row_counts(lengths, n_src, "lengths"), _row_fill(fill_to, n_src)
            cap = max([self.spec.frames(v) for v in lens.tolist()] + ([] if fill is None else fill.tolist()), default=0)
            out = torch.zeros((n_src, ch, self.features, cap), dtype=torch.float32, device="cuda:%d" % self.device)
        stream = _stream_of(stream, self.device)
        out, frames = self.spec.run(pcm, lengths, out=out, samples=samples, stream=stream)
        self.log.run(out, frames, fill_to=fill_to, stream=stream)
        if self.use_energy and self.energy_floor > 0.0 and out.shape[3]:
            with torch.cuda.stream(torch.cuda.ExternalStream(stream, device=self.device) if stream else torch.cuda.default_stream(self.device)):
                line = out[:, :, 0, :]
                written = torch.arange(out.shape[3], device=out.device)[None, None, :] < frames.to(out.device)[:, None, None]
                line.copy_(torch.where(written, torch.clamp(line, min=float(np.log(self.energy_floor))), line))
        if self.norm is not None:
            self.norm.run(out, frames, fill_to=fill_to, stream=stream)
        return out, frames


PACK_MAX_CONTEXT, PACK_MAX_STRIDE, PACK_MAX_F = 16, 16, 65535      # LW_PACK_MAX_CONTEXT, LW_PACK_MAX_STRIDE, the limit on F
_PACK_DTYPES = {"f32": 0, "bf16": 1, "f16": 2}                     # LW_PACK_F32, LW_PACK_BF16, LW_PACK_F16
_PACK_EDGES = {"replicate": 0, "valid": 1}                         # LW_PACK_EDGE_REPLICATE, LW_PACK_EDGE_VALID


def _pack_params(n_in, left, right, stride, edge, dtype, shift, scale, pad):
    """(F, left, right, stride, edge, dtype, shift, scale, pad) checked, the two vectors as contiguous float32 [W * F] or None; or
    ValueError for what lw_pack_create refuses"""
    if not _is_int(n_in) or not 1 <= n_in <= PACK_MAX_F:
        raise ValueError("n_in=%r: an integer in 1 .. %d" % (n_in, PACK_MAX_F))
    for name, v in (("left", left), ("right", right)):
        if not _is_int(v) or not 0 <= v <= PACK_MAX_CONTEXT:
            raise ValueError("%s=%r: an integer in 0 .. %d" % (name, v, PACK_MAX_CONTEXT))
    if not _is_int(stride) or not 1 <= stride <= PACK_MAX_STRIDE:
        raise ValueError("stride=%r: an integer in 1 .. %d" % (stride, PACK_MAX_STRIDE))
    if edge not in _PACK_EDGES:
        raise ValueError("edge=%r: \"replicate\" or \"valid\"" % (edge,))
    if dtype not in _PACK_DTYPES:
        raise ValueError("dtype=%r: \"f32\", \"bf16\" or \"f16\"" % (dtype,))
    try:
        pad = float(pad)
    except (TypeError, ValueError):
        raise ValueError("pad must be a number")
    if pad != pad:
        raise ValueError("pad must not be a NaN")
    D = (int(left) + int(right) + 1) * int(n_in)
    vecs = []
    for name, v in (("shift", shift), ("scale", scale)):
        if v is not None:
            try:
                v = np.ascontiguousarray(v, np.float32)
            except (TypeError, ValueError):
                raise ValueError("%s= must be an array of numbers" % name)
            if v.shape != (D,):
                raise ValueError("%s= must hold W * n_in = %d values (one per OUTPUT element), not %r" % (name, D, v.shape))
        vecs.append(v)
    return int(n_in), int(left), int(right), int(stride), edge, dtype, vecs[0], vecs[1], pad


class FramePack(_Handle):
    """lw_pack: feature rows [rows][C][n_in][frame capacity] (float32, the chain's layout) -> [rows][C][out capacity][W * n_in]
    frames of float32, bfloat16 or float16 on the GPU (k_pack), by the rule of include/lewton_amd.h ("frame-major model input"), a
    contract on bits: W = left + right + 1 frames of context per output frame, every stride-th frame, the edge frames replicated
    (edge="replicate": ceil(T / stride) frames, FunASR's LFR) or only whole windows (edge="valid": Kaldi's splice without
    padding, "stack m skip n"); then + shift[j], * scale[j] per OUTPUT element j = k * n_in + f where given (a global CMVN), ONE
    rounding to dtype, pad beyond the frames and the padding mask.  Parameter errors are ValueError and need no GPU; the object
    itself lives on cuda:device."""

    _C = "lw_pack"

    def __init__(self, n_in, left=0, right=0, stride=1, edge="replicate", dtype="f32", shift=None, scale=None, pad=0.0, device=0):
        (self.n_in, self.left, self.right, self.stride, self.edge, self.dtype, self._shift, self._scale,
         self.pad) = _pack_params(n_in, left, right, stride, edge, dtype, shift, scale, pad)
        self.device = device
        _gpu()
        p = N.PackParams(self.n_in, self.left, self.right, self.stride, _PACK_EDGES[edge], _PACK_DTYPES[dtype], self.pad, 0)
        self._create(device, C.byref(p), _array_ptr(self._shift), _array_ptr(self._scale))
        assert self.width == (self.left + self.right + 1) * self.n_in

    @classmethod
    def transpose(cls, n_in, **kw):
        """[n_in][frame] -> [frame][n_in], nothing else"""
        return cls(n_in, **kw)

    @classmethod
    def splice(cls, n_in, left, right, **kw):
        """Kaldi's splice-feats: every frame with `left` frames before it and `right` behind, the edge frames replicated"""
        return cls(n_in, left, right, **kw)

    @classmethod
    def subsample(cls, n_in, n, **kw):
        """Kaldi's subsample-feats: every n-th frame"""
        return cls(n_in, 0, 0, n, **kw)

    @classmethod
    def stack(cls, n_in, m, n, **kw):
        """"stack m skip n": frames u * n .. u * n + m - 1, whole windows only"""
        if not _is_int(m) or m < 1:
            raise ValueError("m=%r: a positive integer" % (m,))
        return cls(n_in, 0, m - 1, n, edge="valid", **kw)

    @classmethod
    def lfr(cls, n_in, m=7, n=6, **kw):
        """FunASR's low frame rate input (apply_lfr): m frames stacked, every n-th kept, (m - 1) // 2 copies of the first frame
        in front and the last frame repeated behind"""
        if not _is_int(m) or m < 1:
            raise ValueError("m=%r: a positive integer" % (m,))
        return cls(n_in, (m - 1) // 2, m - 1 - (m - 1) // 2, n, **kw)

    @property
    def width(self):
        """elements per output frame: D = W * n_in"""
        return int(N.lw_pack_width(self._h))

    @property
    def tile_frames(self):
        """the output frames one workgroup produces (lw_pack_tile_frames)"""
        return int(N.lw_pack_tile_frames(self._h))

    def frames(self, T):
        """output frames of a row of T frames (lw_pack_frames)"""
        return int(N.lw_pack_frames(self._h, int(T)))

    def convert(self, v):
        """the contract's conversion of one float32 value on the host (lw_pack_convert): the bit pattern as an integer"""
        return int(N.lw_pack_convert(self._h, float(np.float32(v))))

    def last_launches(self):
        """kernels the last call queued: 1 per 65535 rows, 0 when nothing was to be written; -1: no call yet"""
        return N.lw_pack_last_launches(self._h)

    def run(self, feat, frames, out=None, fill_to=None, want_mask=False, stream=None):
        """lw_pack_rows: frames[i] frames of every line of row i of feat (float32 [rows][C][n_in][frame capacity]) -> out
        ([rows][C][out capacity][width] of the object's dtype; None: a zeroed tensor whose capacity is the largest of the rows'
        output frames and fill_to; it must not overlap feat).  fill_to: None, one count for all rows or one per row, in OUTPUT
        frames -- positions [out_frames[i], fill_to[i]) of every channel receive pad.  want_mask: True for a zeroed uint8 tensor
        [rows][out capacity], or such a tensor of the caller's: 1 on a row's frames, 0 on its padding up to fill_to, nothing else
        of it written.  Nothing else of out is written either.  stream: a hipStream_t value; None = torch's current stream on the object's
        device.  Asynchronous; returns (out, out_frames) or (out, out_frames, mask), out_frames a numpy uint64 array."""
        torch = _gpu()
        _check_tensor(feat, "feat", "[rows][C][%d][frames]" % self.n_in, self.device, (torch.float32,), (4,))
        if feat.shape[2] != self.n_in:
            raise ValueError("feat must be [rows][C][%d][frames], not %r" % (self.n_in, tuple(feat.shape)))
        n_rows, ch, _, cap = feat.shape
        counts, fill = _row_counts(frames, n_rows, "frames"), _row_fill(fill_to, n_rows)
        out_frames = np.asarray([self.frames(v) for v in counts.tolist()], np.uint64)
        tdtype = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}[self.dtype]
        if out is None:
            out_cap = max(out_frames.tolist() + ([] if fill is None else fill.tolist()), default=0)
            out = torch.zeros((n_rows, ch, out_cap, self.width), dtype=tdtype, device=feat.device)
        _check_tensor(out, "out", "[rows][C][frames][width]", self.device, (tdtype,), (4,))
        if tuple(out.shape[:2]) != (n_rows, ch) or out.shape[3] != self.width:
            raise ValueError("out must be (%d, %d, frames, %d), not %r" % (n_rows, ch, self.width, tuple(out.shape)))
        out_cap = out.shape[2]
        mask = None
        if want_mask is True:
            mask = torch.zeros((n_rows, out_cap), dtype=torch.uint8, device=feat.device)
        elif want_mask is not False and want_mask is not None:
            mask = want_mask
            _check_tensor(mask, "want_mask=", "[rows][out capacity] = %r (or True)" % ((n_rows, out_cap),), self.device, (torch.uint8,),
                          shape=(n_rows, out_cap))
        self._call(N.lw_pack_rows, ch, _tensor_ptr(feat), _tensor_ptr(out), n_rows, cap, out_cap, _array_ptr(counts), _array_ptr(fill),
                   _tensor_ptr(mask), _stream_of(stream, self.device))
        return (out, out_frames) if mask is None else (out, out_frames, mask)


def _normalizer(normalize, samples, device):
    """normalize= of decode_streams / decode_ogg_files -> (a Normalize or None, whether it is this call's own to close); ValueError
    before anything is decoded"""
    if normalize is None:
        return None, False
    if samples != "f32":
        raise ValueError("normalize= works on the planar f32 format, not samples=%r" % (samples,))
    if isinstance(normalize, Normalize):
        if normalize.device != device:
            raise ValueError("normalize= lives on cuda:%d, the rows on cuda:%d" % (normalize.device, device))
        return normalize, False
    if normalize == "wav2vec2":
        return Normalize.wav2vec2(device), True
    if normalize == "peak":
        return Normalize.peak(device=device), True
    raise ValueError("normalize=%r: a Normalize, \"wav2vec2\" or \"peak\"" % (normalize,))


def _normalize_rows(nm, own, pcm, lengths, device):
    """the finished rows in place, on torch's current stream; returns when it has completed"""
    import torch
    try:
        with torch.cuda.device(device):
            nm.run(pcm, lengths)
            torch.cuda.current_stream(device).synchronize()
    finally:
        if own:
            nm.close()


def _round_up(n, to):
    to = max(1, int(to))
    return (n + to - 1) // to * to


def _sample_bound(ident, setup, packets, packet_keep=None):
    """upper bound of the samples a stream yields (audio.rs:874-909): its first packet adds nothing, a packet that fails nothing"""
    _host()
    total = 0
    for t, p in enumerate(packets):
        if t == 0:
            continue
        try:
            m = get_decoded_sample_count(ident, setup, p)
        except AudioReadError:
            continue
        total += min(m, packet_keep[t]) if packet_keep and t in packet_keep else m
    return total


def _row_length(total, skip, keep):
    return min(max(total - skip, 0), _NO_LIMIT if keep is None else keep)


def plan_places(st_idx, m, decoded, skip, keep, row_of):
    """The per-row cursor for one batch, vectorised: st_idx[i] = stream of packet i (a stream's packets in order), m[i] = the
    samples it yields (0 for a failed packet), decoded[s] = samples stream s has yielded before this batch (updated in place),
    skip[s] / keep[s] = leading samples of the stream to drop / cap on its row's length, row_of[s] = its row.  Returns the
    lw_row_place array: packet i covers the stream positions [s0, s0 + m[i]), of which [skip, skip + keep) go to the row."""
    n = len(st_idx)
    # the stream position of every packet's first sample: the stream's cursor + the packets of it earlier in this batch
    order = np.argsort(st_idx, kind="stable")
    so, mo = st_idx[order], m[order]
    cs = np.cumsum(mo) - mo
    starts = np.r_[True, so[1:] != so[:-1]] if n else np.zeros(0, bool)
    base = np.maximum.accumulate(np.where(starts, cs, 0)) if n else cs
    s0 = np.empty(n, np.int64)
    s0[order] = decoded[so] + cs - base
    np.add.at(decoded, st_idx, m)
    sk, kp = skip[st_idx], keep[st_idx]
    lo = np.clip(sk - s0, 0, m)
    hi = np.clip(np.minimum(sk + kp, _NO_LIMIT) - s0, 0, m)
    kept = np.maximum(hi - lo, 0)
    places = np.zeros(n, PLACE_DTYPE)
    places["row"] = row_of[st_idx]
    places["skip"] = lo
    places["keep"] = kept
    places["t0"] = np.where(kept > 0, s0 + lo - sk, 0)
    return places


def _decode_group(dec, streams, samples, max_packets, run, entropy_on_device, skip, keep, pcm, row_of, packet_keep, mix=None):
    """The streams of ONE decoder into the rows `row_of` of pcm, on torch's current stream, through the channel matrix `mix` if
    there is one.  Returns (samples decoded per stream before skip / keep, errors as (stream, packet, code))."""
    torch = _gpu()
    from .batch import Batch
    n_streams = len(streams)
    total = sum(len(s) for s in streams)
    decoded = np.zeros(n_streams, np.int64)
    errors = []
    if total == 0:
        return decoded, errors
    cap = max(1, min(int(max_packets), total))
    run = max(1, int(run))
    skip_a = np.asarray(skip, np.int64)
    keep_a = np.asarray([_NO_LIMIT if k is None else k for k in keep], np.int64)
    row_a = np.asarray(row_of, np.int64)
    rows = Rows(dec, cap, samples)
    # two batches in turn: the host stage of one runs while the GPU works on the other; a batch's pinned staging is
    # rewritten only once its previous launches have completed
    slots = [[Batch(dec, cap, samples), None] for _ in range(2 if total > cap else 1)]
    try:
        if entropy_on_device == "auto":
            why = C.c_char_p()
            entropy_on_device = bool(N.lw_decoder_supports_device_entropy(dec._h, C.byref(why)))
        for bt, _ in slots:
            if entropy_on_device and not bt.set_entropy_on_device(True):
                raise ValueError("this stream's entropy stage cannot run on the device")
        pws = [PreviousWindowRight() for _ in streams]
        pos = [0] * n_streams
        active = deque(s for s in range(n_streams) if streams[s])
        k = 0

        def finish(slot):
            if slot[1] is not None:
                slot[1].synchronize()
                slot[1] = None
                if slot[0].device_status():
                    raise RuntimeError("device error in a batch: " + N.device_error())

        while active:
            # up to `run` consecutive packets of each stream in turn (a stream's window state moves once per run, not per packet)
            items = []
            while active and len(items) < cap:
                s = active.popleft()
                take = min(run, len(streams[s]) - pos[s], cap - len(items))
                items += [(s, pos[s] + j) for j in range(take)]
                pos[s] += take
                if pos[s] < len(streams[s]):
                    active.append(s)
            slot = slots[k % len(slots)]
            k += 1
            finish(slot)
            bt = slot[0]
            bt.entropy_marshalled(bt.marshal([(streams[s][t], pws[s]) for s, t in items]))
            n = len(items)
            res = np.ctypeslib.as_array(C.cast(N.lw_batch_results(bt._h), C.POINTER(C.c_uint8)), shape=(n * 16,)).view(_RESULT_DTYPE)
            st_idx = np.fromiter((s for s, _ in items), np.int64, n)
            bad = np.nonzero(res["status"])[0]
            errors += [(items[i][0], items[i][1], int(res["status"][i])) for i in bad]
            m = np.where(res["status"] == 0, res["n_samples"], 0).astype(np.int64)
            if packet_keep:
                for i, (s, t) in enumerate(items):
                    if packet_keep[s] and t in packet_keep[s]:
                        m[i] = min(m[i], packet_keep[s][t])
            places = plan_places(st_idx, m, decoded, skip_a, keep_a, row_a)
            bt.upload(_stream_of(None, dec.device))
            rows.synth(bt, places, pcm, mix=mix)
            ev = torch.cuda.Event()
            ev.record(torch.cuda.current_stream(dec.device))
            slot[1] = ev
        for slot in slots:
            finish(slot)
    finally:
        torch.cuda.current_stream(dec.device).synchronize()
        for bt, _ in slots:
            bt.close()
        rows.close()
    return decoded, errors


def _alloc(fmt, n_rows, ch, T, device, out):
    torch = _gpu()
    shape = (n_rows, T, ch) if N.fmt_interleaved(fmt) else (n_rows, ch, T)
    if out is None:
        return torch.zeros(shape, dtype=torch_dtype(fmt), device="cuda:%d" % device)
    t_out = out.shape[1 if N.fmt_interleaved(fmt) else 2] if out.dim() == 3 else -1
    want = shape[:1] + ((t_out, ch) if N.fmt_interleaved(fmt) else (ch, t_out))
    if (out.dim() != 3 or tuple(out.shape) != want or t_out < T or out.dtype != torch_dtype(fmt) or not out.is_contiguous() or
            out.device.type != "cuda" or out.device.index != device):
        raise ValueError("out= must be a contiguous %s tensor on cuda:%d of shape %s with at least %d samples per row" % (
            torch_dtype(fmt), device, shape, T))
    out.zero_()
    return out


def _per_stream(v, n, what):
    if v is None:
        return [None] * n
    v = list(v)
    if len(v) != n:
        raise ValueError("%s= needs one entry per stream" % what)
    return v


def decode_streams(ident, setup, streams, samples="f32", device=0, max_packets=16384, run=16, entropy_on_device="auto",
                   skip=None, keep=None, pad_to=64, out=None, channels=None, sample_rate=None, resample=None, normalize=None):
    """Whole streams of one (ident, setup) pair -> (pcm, lengths, errors).

    streams: list of lists of audio-packet bytes (a stream's first packet only primes the window, audio.rs:1140-1152).
    pcm: tensor on cuda:device, [B, C, T] (planar) or [B, T, C] (interleaved), zero beyond each row's length; T = the longest
    row's upper bound (get_decoded_sample_count over its packets) rounded up to pad_to.  out=: a tensor of that shape (or more
    samples per row) to fill instead; it is zeroed first.  lengths: int64 [B], a host tensor.  errors: (stream, packet, code)
    of the packets whose status is not LW_OK -- they add no samples and decoding goes on (lw_ogg_stream_read_dec_packets).
    skip[s] drops leading samples of stream s, keep[s] caps its length.  Batches of up to max_packets packets take up to `run`
    consecutive packets of each stream in turn.  entropy_on_device: "auto" = k_entropy where the stream is eligible.
    channels: None = the stream's own channels; "mono" = mix_mono; anything else a channel matrix [out_ch][in_ch] -- C is then
    out_ch, and out= is checked against it (i16 formats: routing matrices only, ValueError before anything is decoded).
    sample_rate: None or the stream's own rate = the samples as decoded.  Any other rate (f32 formats only, ValueError before
    anything is decoded): the streams are decoded as above -- skip, keep and channels= at the stream's rate -- into a temporary
    tensor, and a Resampler(stream's rate, sample_rate, **resample) fills pcm from it; lengths are then OUTPUT lengths,
    out_len of the decoded ones, and T is out_len of the longest row's upper bound rounded up to pad_to.  resample: a dict of
    zeros, rolloff, window, beta.  normalize: None, a Normalize or one of the names "wav2vec2", "peak" -- applied in place to the
    finished rows (their lengths; what lies beyond stays zero), after the resampler if there is one; samples="f32" only,
    ValueError before anything is decoded.  The GPU work is queued on torch's current stream; the call returns when it has
    completed."""
    import torch
    _host()
    fmt = _FMT[samples]
    mix = None if channels is None else _named_mix(channels, ident.audio_channels, fmt)
    params = _resample_params(resample)
    if normalize is not None:
        nm, own = _normalizer(normalize, samples, device)
        try:
            pcm, lengths, errors = decode_streams(ident, setup, streams, samples, device, max_packets, run, entropy_on_device, skip, keep,
                                                  pad_to, out, channels, sample_rate, resample)
        except BaseException:
            if own:
                nm.close()
            raise
        _normalize_rows(nm, own, pcm, lengths, device)
        return pcm, lengths, errors
    streams = [list(s) for s in streams]
    B = len(streams)
    skip = [0 if v is None else int(v) for v in _per_stream(skip, B, "skip")]
    keep = _per_stream(keep, B, "keep")
    bound = [_row_length(_sample_bound(ident, setup, s), skip[i], keep[i]) for i, s in enumerate(streams)]
    if sample_rate is not None and sample_rate != ident.audio_sample_rate:
        if fmt not in (N.FMT_F32_PLANAR, N.FMT_F32_INTERLEAVED):
            raise ValueError("samples=%r at %d Hz from a %d Hz stream: the resampler works on the f32 formats" % (
                samples, sample_rate, ident.audio_sample_rate))
        ch = ident.audio_channels if mix is None else mix.shape[0]
        rs = Resampler(ident.audio_sample_rate, sample_rate, device=device, **params)
        try:
            T = _round_up(max((rs.out_len(b) for b in bound), default=0), pad_to)
            with torch.cuda.device(device):
                pcm = _alloc(fmt, B, ch, T, device, out)
                native, nat_lengths, errors = decode_streams(ident, setup, streams, samples, device, max_packets, run, entropy_on_device,
                                                             skip, keep, 1, None, channels)
                rs.run(native, nat_lengths, out=pcm, samples=samples)
                torch.cuda.current_stream(device).synchronize()
            lengths = torch.tensor([rs.out_len(n) for n in nat_lengths.tolist()], dtype=torch.int64)
        finally:
            rs.close()
        return pcm, lengths, errors
    T = _round_up(max(bound, default=0), pad_to)
    with torch.cuda.device(device):
        pcm = _alloc(fmt, B, ident.audio_channels if mix is None else mix.shape[0], T, device, out)
        decoded, errors = _decode_group(decoder_for(ident, setup, device), streams, samples, max_packets, run, entropy_on_device,
                                        skip, keep, pcm, list(range(B)), None, mix)
    lengths = torch.tensor([_row_length(int(decoded[i]), skip[i], keep[i]) for i in range(B)], dtype=torch.int64)
    return pcm, lengths, errors


def _read_ogg(src, name):
    """(ident packet, setup packet, audio packets, per-packet keep) of the first logical stream of one file, with lewton's own
    bookkeeping (inside_ogg.rs:209-229): cur_absgp, and the packet with last_in_stream truncated to absgp_page - cur_absgp"""
    _host()
    from .ogg import PacketReader

    def same_stream(pck, serial):
        if pck.stream_serial() != serial:
            raise ValueError("%s: more than one logical stream (chained or multiplexed file)" % name)
        return pck

    rdr = PacketReader(src)
    try:
        pck = rdr.read_packet_expected()
        idp, serial = pck.data, pck.stream_serial()
        same_stream(rdr.read_packet_expected(), serial)                 # comment header
        stp = same_stream(rdr.read_packet_expected(), serial).data
        rdr.delete_unread_packets()
        packets = []
        while True:
            pck = rdr.read_packet()
            if pck is None:
                break
            packets.append(same_stream(pck, serial))
    finally:
        rdr.close()
    return idp, stp, packets


def _ogg_keeps(ident, setup, packets, name):
    _host()
    from .inside_ogg import VorbisError
    keeps, cur_absgp = {}, None
    for t, pck in enumerate(packets):
        try:
            m = get_decoded_sample_count(ident, setup, pck.data) if t else 0
        except AudioReadError as e:
            raise ValueError("%s: audio packet %d: %s" % (name, t, VorbisError(e.code)))
        if cur_absgp is not None and pck.last_in_stream():
            target = max(pck.absgp_page() - cur_absgp, 0)
            if target < m:
                keeps[t] = m = target
        if pck.last_in_page():
            cur_absgp = pck.absgp_page()
        elif cur_absgp is not None:
            cur_absgp += m
    return keeps


def _group_mix(channels, in_ch, fmt):
    """channels= of decode_ogg_files for a decoder group of in_ch channels"""
    if isinstance(channels, dict):
        if in_ch not in channels:
            raise ValueError("channels= has no matrix for %d channels" % in_ch)
        channels = channels[in_ch]
    elif callable(channels):
        channels = channels(in_ch)
    return _named_mix(channels, in_ch, fmt)


def decode_ogg_files(sources, samples="f32", device=0, **kw):
    """Ogg/Vorbis files (paths or bytes) -> (pcm, lengths, sample_rate); pcm and lengths as decode_streams returns them, row i =
    the first logical stream of sources[i] = the concatenation of what OggStreamReader.read_dec_packet_generic returns for it
    (the last packet truncated to the final granule position, inside_ogg.rs:219-227).  Files whose ident and setup packets are
    byte-identical share one decoder.  ValueError naming the file: a chained or multiplexed file, a packet that does not decode,
    files that differ in channel count or sample rate.  kw: max_packets, run, entropy_on_device, skip, keep, pad_to, out, channels.
    channels: None = the files' own channels.  Otherwise every decoder group goes through the matrix for ITS channel count, and
    files of different channel counts fill one tensor as long as every matrix has the same out_ch (ValueError naming the file
    otherwise; sample rates must still agree): "mono" = mix_mono, "wav" = mix_wav_order, a dict {in_ch: matrix}, or a callable
    in_ch -> matrix.  i16 formats: routing matrices only, ValueError before anything is decoded.
    sample_rate (and resample, a dict of Resampler's zeros, rolloff, window, beta): with it files of different sample rates fill
    one tensor at that rate, which is the rate returned.  Decoder groups already at sample_rate decode straight into their rows;
    every other group decodes into a temporary tensor (skip, keep and channels= at the file's rate) and a Resampler fills its rows
    from it (f32 formats only, ValueError before anything is decoded).  lengths are output lengths.  Without sample_rate the
    rates must agree as before.
    normalize: as decode_streams' -- a Normalize, "wav2vec2" or "peak", applied in place to the finished rows, after the resampler
    if there is one (samples="f32" only, ValueError before anything is decoded)."""
    import torch
    _host()
    from . import header as H
    fmt = _FMT[samples]
    if kw.get("normalize") is not None:
        nm, own = _normalizer(kw.pop("normalize"), samples, device)
        try:
            pcm, lengths, rate = decode_ogg_files(sources, samples, device, **kw)
        except BaseException:
            if own:
                nm.close()
            raise
        _normalize_rows(nm, own, pcm, lengths, device)
        return pcm, lengths, rate
    kw.pop("normalize", None)
    sources = list(sources)
    B = len(sources)
    names = [s if isinstance(s, str) else "source %d" % i for i, s in enumerate(sources)]
    skip = [0 if v is None else int(v) for v in _per_stream(kw.pop("skip", None), B, "skip")]
    keep = _per_stream(kw.pop("keep", None), B, "keep")
    pad_to, out = kw.pop("pad_to", 64), kw.pop("out", None)
    max_packets, run = kw.pop("max_packets", 16384), kw.pop("run", 16)
    entropy_on_device = kw.pop("entropy_on_device", "auto")
    channels = kw.pop("channels", None)
    sample_rate, params = kw.pop("sample_rate", None), _resample_params(kw.pop("resample", None))
    if kw:
        raise TypeError("unexpected arguments: %s" % ", ".join(sorted(kw)))
    if sample_rate is not None:
        resample_geometry(sample_rate, sample_rate)                     # (a rate that is no positive integer: ValueError)
    groups = {}   # (ident packet, setup packet) -> [ident, setup, [file index], [packets], [packet keeps]]
    shape = None
    bound = [0] * B
    for i, src in enumerate(sources):
        idp, stp, packets = _read_ogg(src, names[i])
        g = groups.get((idp, stp))
        if g is None:
            try:
                ident = H.read_header_ident(idp)
                setup = H.read_header_setup(stp, ident.audio_channels, (ident.blocksize_0, ident.blocksize_1))
            except H.HeaderReadError as e:
                raise ValueError("%s: %s" % (names[i], e))
            g = groups[(idp, stp)] = [ident, setup, [], [], [], None]
            if channels is not None:
                try:
                    g[5] = _group_mix(channels, ident.audio_channels, fmt)
                except (ValueError, KeyError) as e:
                    raise ValueError("%s: %s" % (names[i], e))
        ident, setup = g[0], g[1]
        # with sample_rate= the files' own rates may differ: the rate every row ends up with is the one that was asked for
        rate = ident.audio_sample_rate if sample_rate is None else sample_rate
        if channels is not None:
            # the channel count that has to agree is the matrices' out_ch; the files' own may differ
            if shape is None:
                shape = (g[5].shape[0], rate)
            elif shape[0] != g[5].shape[0]:
                raise ValueError("%s: its channel matrix has %d output channels, those of the files before it %d" % (
                    names[i], g[5].shape[0], shape[0]))
            elif shape[1] != rate:
                raise ValueError("%s: %d Hz, the files before it %d Hz" % (names[i], ident.audio_sample_rate, shape[1]))
        elif shape is None:
            shape = (ident.audio_channels, rate)
        elif shape != (ident.audio_channels, rate):
            raise ValueError("%s: %d channels at %d Hz, the files before it %d at %d Hz" % (
                (names[i], ident.audio_channels, rate) + shape))
        if ident.audio_sample_rate != rate and fmt not in (N.FMT_F32_PLANAR, N.FMT_F32_INTERLEAVED):
            raise ValueError("%s: samples=%r at %d Hz from a %d Hz file: the resampler works on the f32 formats" % (
                names[i], samples, rate, ident.audio_sample_rate))
        keeps = _ogg_keeps(ident, setup, packets, names[i])
        data = [p.data for p in packets]
        g[2].append(i), g[3].append(data), g[4].append(keeps)
        bound[i] = _row_length(_sample_bound(ident, setup, data, keeps), skip[i], keep[i])
    if shape is None:
        raise ValueError("no sources")
    lengths = [0] * B
    resamplers = {}   # native rate -> Resampler, for the groups that are not at sample_rate
    native_bound = list(bound)
    try:
        for ident, setup, idx, *_ in groups.values():
            r = ident.audio_sample_rate
            if r != shape[1]:
                if r not in resamplers:
                    resamplers[r] = Resampler(r, shape[1], device=device, **params)
                for i in idx:
                    bound[i] = resamplers[r].out_len(bound[i])
        T = _round_up(max(bound), pad_to)
        with torch.cuda.device(device):
            pcm = _alloc(fmt, B, shape[0], T, device, out)
            for ident, setup, idx, streams, keeps, mix in groups.values():
                rs = resamplers.get(ident.audio_sample_rate)
                dst, rows_of = pcm, idx
                if rs is not None:
                    # at the file's rate into a temporary tensor of this group's rows, then the resampler into pcm's
                    dst, rows_of = _alloc(fmt, len(idx), shape[0], max(native_bound[i] for i in idx), device, None), list(range(len(idx)))
                decoded, errors = _decode_group(decoder_for(ident, setup, device), streams, samples, max_packets, run, entropy_on_device,
                                                [skip[i] for i in idx], [keep[i] for i in idx], dst, rows_of, keeps, mix)
                if errors:
                    s, t, code = errors[0]
                    raise ValueError("%s: audio packet %d does not decode (%d)" % (names[idx[s]], t, code))
                native = [_row_length(int(decoded[j]), skip[i], keep[i]) for j, i in enumerate(idx)]
                if rs is not None:
                    rs.run(dst, native, out=pcm, rows=idx, samples=samples)
                    torch.cuda.current_stream(device).synchronize()
                for j, i in enumerate(idx):
                    lengths[i] = native[j] if rs is None else rs.out_len(native[j])
    finally:
        for rs in resamplers.values():
            rs.close()
    return pcm, torch.tensor(lengths, dtype=torch.int64), shape[1]
