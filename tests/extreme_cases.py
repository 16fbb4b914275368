"""Streams whose samples are subnormal, saturating or non-finite, and the value classes the tests name.

streamgen's packet writers never leave |x| < 1000 (the largest sample of the suite's corpora is 976), so nothing ahead of the row
pipeline has met a subnormal, an x * 32768 beyond the i32 range, an inf or a NaN.  A Vorbis setup header can carry all of it:
float32_unpack (bitpacking.rs:304-314) reaches 2^235 and 2^-788, so a codebook's `minimum` / `delta` can be huge, subnormal or inf
in f32.  `scale_vq_books` multiplies both by a power of two, which is exact, so the packets written for the unscaled setup decode
for the scaled one too (the same bits, the same symbols) and the spectrum is the unscaled one times 2^k until f32 runs out.

Value classes (CLASSES): a scale and a condition on the ORACLE's f32 samples of a corpus.  Every test asserts the condition before
it compares anything, so a case cannot go vacuous when a generator or a setup changes.  The figures in the comments are the
oracle's for stereo_setup(), "LLSSLSL", 14 packets, seeds 5 and 36, p_floor_unused = 0.05 (31 744 samples).

brink (a scale in 2^121 .. 2^125 at which finite, +-inf and NaN samples are all present in one corpus) does not exist: no scale
gives a single +-inf SAMPLE.  An inf is born in the transform's sums and meets its opposite a butterfly later, so a block is NaN
throughout as soon as one of its sums overflows (tests/test_extreme_values.py::test_no_scale_gives_an_infinite_sample keeps the
scan of the five scales).  What the scan did find is kept as `overflow`: at 2^124 the VQ tables and the spectrum are finite and the
NaN are made by the transform, in about half of the blocks, next to blocks that stay finite with |x| up to 2^127.

Blocks of one stream scaled differently (long_only, short_only): a packet returns the overlap of its block with its predecessor's
and, where the two differ in size, part of the flat (unwindowed) half of the longer one.  With the LONG blocks non-finite a short
block's packets next to them are NaN throughout; what long_only shows is a packet NaN throughout directly before one finite
throughout (a NaN packet leaves a finite right half).  With the SHORT blocks non-finite (short_only) a long block behind a short one
returns NaN in the n0/2 samples of the overlap and FINITE samples of its own flat part behind them, in one channel: the shape that
shows a kernel which lets the predecessor's NaN reach past the overlap, or multiplies a NaN by a window coefficient the reference
never applies.  one_submap: a whole channel finite beside a whole channel of NaN.
"""
import copy

import numpy as np

from common import oracle_headers, po, sg

TWO31 = np.float32(2.0 ** 31)


def scale_vq_books(setup, k, only=None, classes=None):
    """A deep copy of `setup` with `minimum` and `delta` of the value-carrying codebooks (lookup_type != 0) times 2^k.
    only = a residue number: just the books that residue's cascade names; they are copied to the end of the codebook list,
    scaled there, and that residue re-indexed, so every other residue (and floor 0) keeps the unscaled books it shared.
    classes (with only): just the cascades of these classifications of that residue."""
    st = copy.deepcopy(setup)
    f = 2.0 ** k
    if only is None:
        for cb in st.codebooks:
            if cb.lookup_type:
                cb.minimum, cb.delta = cb.minimum * f, cb.delta * f
        return st
    rs = st.residues[only]
    moved = {}
    for cl, row in enumerate(rs.books):
        for p, b in enumerate(row):
            if b < 0 or (classes is not None and cl not in classes):
                continue
            if b not in moved:
                cb = copy.deepcopy(st.codebooks[b])
                assert cb.lookup_type, "a residue pass through a book without values"
                cb.minimum, cb.delta = cb.minimum * f, cb.delta * f
                moved[b] = len(st.codebooks)
                st.codebooks.append(cb)
            row[p] = moved[b]
    assert len(st.codebooks) <= 256
    return st


def long_only(setup, k):
    """only the residues of the long modes are scaled: short packets stay finite next to long ones that do not"""
    res = sorted({r for md in setup.modes if md.blockflag for r in setup.mappings[md.mapping].submap_residue})
    shorts = {r for md in setup.modes if not md.blockflag for r in setup.mappings[md.mapping].submap_residue}
    assert res and not shorts & set(res)
    st = setup
    for r in res:
        st = scale_vq_books(st, k, only=r)
    return st


def short_only(setup, k):
    """only the residues of the short modes are scaled: a long block behind a short one is finite behind a NaN overlap"""
    res = sorted({r for md in setup.modes if not md.blockflag for r in setup.mappings[md.mapping].submap_residue})
    longs = {r for md in setup.modes if md.blockflag for r in setup.mappings[md.mapping].submap_residue}
    assert res and not longs & set(res)
    st = setup
    for r in res:
        st = scale_vq_books(st, k, only=r)
    return st


def one_submap(setup, k, submap=0):
    """only the residues of one submap (of every mode) are scaled: whole channels stay finite beside the others"""
    assert all(len(m.submap_residue) > submap and len(m.submap_residue) >= 2 for m in setup.mappings)
    st = setup
    for r in sorted({m.submap_residue[submap] for m in setup.mappings}):
        st = scale_vq_books(st, k, only=r)
    return st


def one_class(setup, k, cl=3):
    """only the books of classification `cl` (of every residue) are scaled.  With residue types 0 / 1 every channel has its own
    class words, so a packet writer that keeps the class out of one channel (ANGLE_ONLY, MAGNITUDE_ONLY) makes the non-finite
    values meet finite ones in the inverse coupling (audio.rs:763-777): its comparisons are false for a NaN, so a NaN angle
    gives (m +- a, m) -- a NaN magnitude channel and a FINITE angle channel -- and a NaN magnitude gives NaN in both."""
    st = setup
    for r in range(len(setup.residues)):
        st = scale_vq_books(st, k, only=r, classes=(cl,))
    return st


ANGLE_ONLY = dict(class_probs_by_channel=((0.45, 0.35, 0.2, 0.0), (0.3, 0.25, 0.15, 0.3)))
MAGNITUDE_ONLY = dict(class_probs_by_channel=((0.3, 0.25, 0.15, 0.3), (0.45, 0.35, 0.2, 0.0)))


def uncoupled_two_submaps(bs0=8, bs1=11):
    """stereo without coupling, channel 1 in a submap of its own with its own (type 1) residues"""
    st = sg.stereo_setup(44100, bs0, bs1)
    for flag, m in enumerate(st.mappings):
        m.coupling = []
        m.mux = [0, 1]
        own = copy.deepcopy(st.residues[m.submap_residue[0]])
        own.type, own.end = 1, own.end // 2
        st.residues.append(own)
        m.submap_floor = [m.submap_floor[0]] * 2
        m.submap_residue = [m.submap_residue[0], len(st.residues) - 1]
    return st


# ---- the oracle's view of a corpus ---------------------------------------------------------------------------------------------
class Corpus:
    """streams of one setup decoded by the oracle once: want[(s, t)] = (status, f32 [ch][m] or None), want_i16[(s, t)] = planar
    i16 of the packets that decode, state[s] = the stream's final PreviousWindowRight [ch][len] (or None)"""

    def __init__(self, setup, streams):
        self.setup, self.streams = setup, streams
        o_id, o_st = oracle_headers(setup)
        self.want, self.want_i16, self.state = {}, {}, []
        for s, pk in enumerate(streams):
            opw, opw16 = po.Pwr(), po.Pwr()
            for t, p in enumerate(pk):
                try:
                    self.want[(s, t)] = (0, po.read_audio_packet(o_id, o_st, p, opw, "f32"))
                    self.want_i16[(s, t)] = po.read_audio_packet(o_id, o_st, p, opw16, "i16")
                except po.OracleError as e:
                    self.want[(s, t)] = (e.code, None)
            self.state.append(opw.data(setup.channels))

    def blocks(self):
        return [w for rc, w in self.want.values() if rc == 0 and w.size]

    def samples(self):
        return np.concatenate([w.reshape(-1) for w in self.blocks()])


def to_i16(x):
    """samples.rs:92-103 on an f32 array: x * 32768 in f32, clamped to 32767 / -32768, NaN -> 0 (`as i16`), else truncated"""
    with np.errstate(over="ignore", invalid="ignore"):
        y = np.asarray(x, np.float32) * np.float32(32768.0)
        out = np.where(y > 32767, 32767, np.where(y < -32768, -32768, np.where(np.isnan(y), 0, np.trunc(y))))
    return out.astype(np.int16)


def _scaled(x):
    with np.errstate(over="ignore", invalid="ignore"):
        return np.abs(np.asarray(x, np.float32) * np.float32(32768.0))


def _subnormal(x):
    return (x != 0) & (np.abs(x) < np.finfo(np.float32).tiny)


def is_quiet(c):                                   # 31 741 subnormal, 3 zero
    x = c.samples()
    return 2 * np.count_nonzero(_subnormal(x)) >= x.size


def is_vanishing(c):                               # 29 335 subnormal, 2 409 zero
    x = c.samples()
    return 100 * np.count_nonzero(_subnormal(x)) >= x.size and 100 * np.count_nonzero(x == 0) >= x.size


def is_loud(c):                                    # 31 741 clip, 7 347 of them with |x * 32768| >= 2^31
    x = c.samples()
    y = _scaled(x)
    return bool(np.all(np.isfinite(y)) and 10 * np.count_nonzero(y >= TWO31) >= x.size
                and 10 * np.count_nonzero((y > 32768) & (y < TWO31)) >= x.size)


def is_huge(c):                                    # x finite everywhere; x * 32768 = +-inf for 22 592, finite and >= 2^31 for 9 152
    x = c.samples()
    y = _scaled(x)
    return bool(np.all(np.isfinite(x)) and 10 * np.count_nonzero(np.isinf(y)) >= x.size
                and 10 * np.count_nonzero(np.isfinite(y) & (y >= TWO31)) >= x.size)


def is_nonfinite(c):                               # every sample-bearing packet all NaN
    b = c.blocks()
    return bool(b) and all(bool(np.all(np.isnan(w))) for w in b)


def is_overflow(c):                                # stereo: 17 408 NaN, 14 336 finite (13 791 of them with x * 32768 = +-inf)
    x = c.samples()
    return 100 * np.count_nonzero(np.isnan(x)) >= x.size and 100 * np.count_nonzero(np.isfinite(x) & (x != 0)) >= x.size


def _share(c, pred):
    b = c.blocks()
    return bool(b) and 2 * sum(bool(pred(w)) for w in b) >= len(b)


def is_angle_nan(c):
    """one_class at 2^130 (every value of the class is NaN) kept out of the magnitude channel: in at least half of the packets
    the magnitude channel is NaN throughout and the angle channel finite and non-zero throughout (stereo 8/11: in all 26)"""
    return _share(c, lambda w: np.isnan(w[0]).all() and (np.isfinite(w[1]) & (w[1] != 0)).all())


def is_magnitude_nan(c):
    """the same class kept out of the angle channel: both channels NaN throughout in at least half of the packets"""
    return _share(c, lambda w: np.isnan(w).all())


def has_channels_beside(c):
    """one_submap: packets in which a whole channel is finite and non-zero beside a whole channel of NaN"""
    return any(bool(np.isnan(w).all(axis=1).any() and (np.isfinite(w) & (w != 0)).all(axis=1).any()) for w in c.blocks())


def has_finite_after_nan(c):
    """long_only: in one stream, a packet that is NaN throughout directly before one that is finite and non-zero throughout"""
    for (s, t), (rc, w) in c.want.items():
        nxt = c.want.get((s, t + 1))
        if rc == 0 and w.size and np.isnan(w).all() and nxt and nxt[0] == 0 and nxt[1].size and \
                (np.isfinite(nxt[1]) & (nxt[1] != 0)).all():
            return True
    return False


def has_nan_overlap_before_finite_flat(c):
    """short_only: a packet of a long block one channel of which is NaN in exactly the n0/2 samples of the overlap with the short
    block before it, and finite and non-zero in every sample behind them (the block's own flat part)"""
    ov, long_m = (1 << c.setup.bs0) // 2, (1 << c.setup.bs0) // 4 + (1 << c.setup.bs1) // 4
    for rc, w in c.want.values():
        if rc == 0 and w.shape[1] >= long_m > ov:
            for x in w:
                if np.isnan(x[:ov]).all() and (np.isfinite(x[ov:]) & (x[ov:] != 0)).all():
                    return True
    return False


# class -> (scales, condition); a class with two scales is two setups, each decoded and checked (nonfinite: at 2^126 `delta` is
# finite and `minimum` of the wider books is not; at 2^130 `delta` itself unpacks to inf and the VQ table holds NaN)
CLASSES = {
    "quiet": ((-130,), is_quiet),
    "vanishing": ((-140,), is_vanishing),
    "loud": ((20,), is_loud),
    "huge": ((120,), is_huge),
    "nonfinite": ((126, 130), is_nonfinite),
    "overflow": ((124,), is_overflow),
    # 2^126 on the books of some residues only (derived constructions above)
    "long_only": ((126,), has_finite_after_nan),
    "short_only": ((126,), has_nan_overlap_before_finite_flat),
    "one_submap0": ((126,), has_channels_beside),
    "one_submap1": ((126,), has_channels_beside),
    # the books of one classification, which the packets keep out of one channel of the coupled pair (one_class): NaN angles /
    # angles of +-2^127 (finite: the transform overflows later) beside finite magnitudes, and NaN magnitudes beside finite angles
    "angle_nan": ((130,), is_angle_nan),
    "angle_huge": ((126,), has_channels_beside),
    "magnitude_nan": ((130,), is_magnitude_nan),
}
ANGLE = ("angle_nan", "angle_huge")


def scaled_setup(setup, cls, k):
    if cls == "long_only":
        return long_only(setup, k)
    if cls == "short_only":
        return short_only(setup, k)
    if cls.startswith("one_submap"):
        return one_submap(setup, k, int(cls[-1]))
    if cls in ("angle_nan", "angle_huge", "magnitude_nan"):
        return one_class(setup, k)
    return scale_vq_books(setup, k)


def make_streams(setup, pattern, count, n, seed, **kw):
    return [sg.make_stream(setup, pattern, count, seed=seed + 31 * s, **kw) for s in range(n)]


# ---- the cases: kernel family x stream shape x value classes ---------------------------------------------------------------------
# Shapes, stream counts and expected kernels are those of tests/test_gpu_f32_interleaved.py.  A launch of `n` streams holds
# at most DISTINCT different ones, 4 in the 512-stream launches (stream s = distinct stream s % d): the launch keeps the shape that
# reaches the kernel, the oracle decodes eight streams or four.  tests/test_extreme_values.py asserts every case's class condition on the CPU, the GPU test again.
DISTINCT = 8


def distinct(n):
    return min(n, DISTINCT if n <= 64 else 4)
BASE = ("quiet", "loud", "huge", "nonfinite")
WIDE = BASE + ("vanishing", "overflow")


def _uncoupled():
    st = sg.stereo_setup(44100, 8, 11)
    for m in st.mappings:
        m.coupling = []
    return st


def _floor_posts_beyond_the_block():
    st = sg.stereo_setup(44100, 8, 11)
    f = st.floors[1]
    f.rangebits = 15
    f.x_rest = list(f.x_rest[:-4]) + [5000, 20000, 31880, 131]
    return st


def _surround51_8_10():
    st = sg.surround51_setup(48000, 8, 10)
    st.floors[3].x_rest = [64, 16, 256, 128, 32, 384]
    return st


def _libvorbis_51():
    from lewton_amd.workloads import surround51_libvorbis_coupling
    return surround51_libvorbis_coupling()


def _case(mk, pattern, count, n, seed, expect, classes, **kw):
    """expect: the kernel the case is for, by its exact name in Batch.last_kernels (a comma-separated list), or several (all must
    run).  EDGE: a long block next to a short one in its kernel's EDGE form -- there is no name for the form; without it these
    blocks go through the generic kernels, so EDGE cases also assert that none of those ran."""
    expect = (expect,) if isinstance(expect, str) else tuple(expect or ())
    return dict(mk=mk, pattern=pattern, count=count, n=n, seed=seed, expect=expect, classes=tuple(classes), kw=kw)


GENERIC_KERNELS = ("k_decouple", "k_imdct_generic", "k_ola_generic")
EDGE_CASES = ("k_long_edge_dense", "k_long12_edge")


CASES = {
    # k_long (n = 2048): coupled (decouple4), uncoupled, 5.1 with two submaps, libvorbis' 5.1 coupling (PRE), k_prep, k_mix
    "k_long_coupled": _case(lambda: sg.stereo_setup(), "L", 16, 64, 5, "k_long", WIDE, p_floor_unused=0.05),
    "k_long_uncoupled": _case(_uncoupled, "L", 16, 64, 5, "k_long", BASE, p_floor_unused=0.05),
    "k_long_two_submaps": _case(uncoupled_two_submaps, "L", 16, 64, 5, "k_long", ("one_submap0", "one_submap1"), p_floor_unused=0.05),
    "k_long_51": _case(lambda: sg.surround51_setup(), "L", 16, 24, 5, "k_long", BASE + ("one_submap0", "one_submap1"),
                       p_floor_unused=0.05),
    "k_long_pre": _case(_libvorbis_51, "L", 16, 24, 5, "k_long", BASE, p_floor_unused=0.05),
    "k_prep": _case(_floor_posts_beyond_the_block, "L", 16, 24, 5, "k_prep", BASE, p_floor_unused=0.05),
    "k_mix": _case(lambda: sg.stereo_setup(), "LSSL", 16, 2, 5, "k_mix", BASE + ("long_only", "short_only"), p_floor_unused=0.05),
    "k_long_edge_dense": _case(lambda: sg.stereo_setup(), "LLSSL", 16, 512, 5, ("k_long", "k_short"),
                               BASE + ("long_only", "short_only"), p_floor_unused=0.05),
    # k_long10 (n = 1024), k_mix10
    "k_long10": _case(lambda: sg.stereo_setup(22050, 9, 10), "L", 16, 48, 7, "k_long10", WIDE),
    # (nonfinite at 2^126 is not met here: the four residue partitions of the LFE's 1024-point block are all silent in some
    # packets, and that channel is then finite)
    "k_long10_51": _case(_surround51_8_10, "L", 16, 16, 7, "k_long10", ("quiet", "loud", "huge", "one_submap0", "one_submap1")),
    "k_mix10": _case(lambda: sg.stereo_setup(22050, 8, 10, residue_type=1), "LSSL", 16, 2, 7, "k_mix10",
                     BASE + ("long_only", "short_only")),
    # k_long12 (n = 4096) and its EDGE form 512 / 4096
    "k_long12": _case(lambda: sg.stereo_setup(44100, 9, 12), "L", 12, 32, 9, "k_long12", WIDE),
    "k_long12_edge": _case(lambda: sg.stereo_setup(44100, 9, 12), "LLSSL", 12, 32, 9, ("k_long12", "k_short"),
                          BASE + ("long_only", "short_only")),
    "k_long12_51": _case(lambda: sg.surround51_setup(48000, 9, 12), "L", 12, 8, 9, "k_long12",
                        BASE + ("one_submap0", "one_submap1")),
    # k_short<8 / 16 / 32>
    "k_short_256": _case(lambda: sg.stereo_setup(44100, 8, 11), "SSSL", 16, 512, 11, "k_short", BASE),
    "k_short_512": _case(lambda: sg.stereo_setup(44100, 9, 12), "SSSL", 16, 24, 11, "k_short", BASE),
    "k_short_1024": _case(lambda: sg.stereo_setup(44100, 10, 12), "SSSL", 16, 24, 11, "k_short", BASE),
    # k_big<13>
    "k_big": _case(lambda: sg.stereo_setup(44100, 6, 13), "LLSL", 8, 8, 13, "k_big", BASE),
    # the generic kernels: 128-point blocks (loud and nonfinite at 2^126 do not meet their conditions there: the blocks are
    # too short to sum that far), and the 5.1 setup forced onto them
    "generic_7_7": _case(lambda: sg.stereo_setup(bs0=7, bs1=7), "SLLS", 16, 8, 15, "k_ola_generic", ("quiet", "vanishing", "huge", "overflow")),
    "generic_forced_51": _case(lambda: sg.surround51_setup(), "LLSSL", 12, 6, 17, "k_ola_generic",
                               WIDE + ("long_only", "short_only", "one_submap0", "one_submap1"), force_generic=True),
    # the entropy stage on the device (its VQ accumulation)
    "k_entropy": _case(lambda: sg.stereo_setup(), "LLSL", 16, 32, 19, "k_entropy", BASE, device_entropy=True),
    "k_entropy_51": _case(lambda: sg.surround51_setup(), "LLSL", 12, 8, 19, "k_entropy",
                          ("quiet", "loud", "huge", "one_submap1"), device_entropy=True),   # residue types 0, 1 and 2 (nonfinite
    # at 2^126 is not met: the LFE's four partitions are all silent in some packets)
    # the inverse coupling on NaN / huge angles beside finite magnitudes and the other way round (residue type 1; one_class)
    "k_long_angle": _case(lambda: sg.stereo_setup(44100, 8, 11, residue_type=1), "L", 16, 64, 5, "k_long", ANGLE, **ANGLE_ONLY),
    "k_long_magnitude": _case(lambda: sg.stereo_setup(44100, 8, 11, residue_type=1), "L", 16, 64, 5, "k_long", ("magnitude_nan",),
                              **MAGNITUDE_ONLY),
    "k_mix_angle": _case(lambda: sg.stereo_setup(44100, 8, 11, residue_type=1), "LSSL", 16, 2, 5, "k_mix", ANGLE, **ANGLE_ONLY),
    "k_long10_angle": _case(lambda: sg.stereo_setup(22050, 9, 10, residue_type=1), "L", 16, 48, 7, "k_long10", ANGLE, **ANGLE_ONLY),
    "k_long12_angle": _case(lambda: sg.stereo_setup(44100, 9, 12, residue_type=1), "LLSSL", 12, 32, 9, "k_long12", ANGLE, **ANGLE_ONLY),
    "k_short_angle": _case(lambda: sg.stereo_setup(44100, 8, 11, residue_type=1), "SSSL", 16, 512, 11, "k_short", ANGLE, **ANGLE_ONLY),
    "k_short_512_angle": _case(lambda: sg.stereo_setup(44100, 9, 12, residue_type=1), "SSSL", 16, 24, 11, "k_short", ANGLE, **ANGLE_ONLY),
    "k_short_1024_angle": _case(lambda: sg.stereo_setup(44100, 10, 12, residue_type=1), "SSSL", 16, 24, 11, "k_short", ANGLE, **ANGLE_ONLY),
    "k_big_angle": _case(lambda: sg.stereo_setup(44100, 6, 13, residue_type=1), "LLSL", 8, 8, 13, "k_big", ANGLE, **ANGLE_ONLY),
    "generic_angle": _case(lambda: sg.stereo_setup(44100, 7, 7, residue_type=1), "SLLS", 16, 8, 15, "k_ola_generic", ANGLE, **ANGLE_ONLY),
    "generic_magnitude": _case(lambda: sg.stereo_setup(44100, 7, 7, residue_type=1), "SLLS", 16, 8, 15, "k_ola_generic",
                               ("magnitude_nan",), **MAGNITUDE_ONLY),
    "k_entropy_angle": _case(lambda: sg.stereo_setup(44100, 8, 11, residue_type=1), "LLSL", 16, 32, 19, "k_entropy", ANGLE,
                             device_entropy=True, **ANGLE_ONLY),
    # the window state through the HBM state pool: five launches
    "launches_stereo": _case(lambda: sg.stereo_setup(), "LLSLSSL", 21, 12, 21, None, BASE + ("overflow", "long_only", "short_only"), launches=5),
    "launches_51": _case(lambda: sg.surround51_setup(), "LLSLSSL", 21, 12, 21, None, ("quiet", "huge", "one_submap0"), launches=5),
    # (5.1: its NaN state crosses the launches under one_submap0; nonfinite is not met, the LFE is silent in some packets)
    "launches_9_12": _case(lambda: sg.stereo_setup(44100, 9, 12), "LLSLSSL", 21, 12, 21, None, ("huge", "overflow", "long_only", "short_only"),
                           launches=5),
}

FORMATS = (("i16", "f32_interleaved"), ("i16_interleaved", "f32"))


def case_ids():
    """(case, class, scale, (an i16 format, an f32 format)): the formats alternate so that all four meet every class"""
    out = []
    for ci, (name, c) in enumerate(CASES.items()):
        for ki, cls in enumerate(c["classes"]):
            for k in CLASSES[cls][0]:
                out.append((name, cls, k, FORMATS[(ci + ki + (k == 130)) % 2]))
    return out


WRITER_KW = ("p_floor_unused", "class_probs_by_channel")      # of a case's kw: the packet writer's; the others are the decode's
_bases, _corpora = {}, {}


def corpus(name, cls, k):
    """the case's scaled setup and its DISTINCT streams decoded by the oracle (kept: CPU and GPU tests share them; the packets
    are written once per case, for the unscaled setup)"""
    if name not in _bases:
        c = CASES[name]
        base = c["mk"]()
        gen = {a: b for a, b in c["kw"].items() if a in WRITER_KW}
        _bases[name] = (base, make_streams(base, c["pattern"], c["count"], distinct(c["n"]), c["seed"], **gen))
    key = (name, cls, k)
    if key not in _corpora:
        base, streams = _bases[name]
        _corpora[key] = Corpus(scaled_setup(base, cls, k), streams)
    return _corpora[key]
