"""CPU half of the extreme-value tests (tests/extreme_cases.py; the GPU half is tests/test_gpu_extreme_values.py).

  * the scaling itself: exact, deep-copying, and what a scaled header unpacks to;
  * every GPU case's class condition on the oracle's samples (the GPU test asserts it again before comparing);
  * the oracle's own handling of such values, against lewton's definitions: `as i16` of samples.rs:92-103 restated in numpy
    over every corpus, and on hand-made values;
  * the same corpora through the lane / thread models of the kernels (fast_model: k_long, short_model: k_short<L>,
    long12_model: k_long12, big_model: k_big), spectrum in, block and overlap-added samples out, against the oracle's taps --
    so whoever sees a GPU mismatch knows whether the kernel left its model or the model left lewton."""
import numpy as np
import pytest

import big_model as bm
import extreme_cases as X
import fast_model as fm
import long12_model as lm
import short_model as sm
from common import f32_identical, oracle_headers, po, sg


def fast_image(setup):          # the image builders need the product's library: imported by the model tests only, so that the
    from test_fast_model import _image      # oracle-side checks above them collect and run without it
    return _image(setup)


def long12_image(setup):
    from test_long12_model import _image
    return _image(setup)


def short_image(setup, blockflag):
    from test_short_model import _image
    return _image(setup, blockflag)


# ---- the scaling ---------------------------------------------------------------------------------------------------------------
def _unpack(x):
    return float(po.lib().lwo_float32_unpack(sg.float32_pack(x)))


@pytest.mark.parametrize("k", [-140, -130, 20, 120, 124, 126])
def test_scaling_is_exact_and_unpacks_to_f32(k):
    base = sg.stereo_setup()
    st = X.scale_vq_books(base, k)
    n = 0
    with np.errstate(over="ignore"):
        for a, b in zip(base.codebooks, st.codebooks):
            if not a.lookup_type:
                assert (a.minimum, a.delta, a.lengths) == (b.minimum, b.delta, b.lengths)
                continue
            for u, v in ((a.minimum, b.minimum), (a.delta, b.delta)):
                assert v == u * 2.0 ** k                                      # exact in f64
                want = np.float32(np.float32(u) * np.float32(2.0) ** np.float32(k)) if abs(k) < 127 else None
                assert want is None or _unpack(v) == float(want) or (np.isinf(want) and np.isinf(_unpack(v)))
            n += 1
    assert n == 4
    assert base.codebooks[4].minimum == -8.0 and base.codebooks[4].delta == 1.0   # the argument is left alone


def test_delta_unpacks_to_inf_at_2_130_and_minimum_at_2_126():
    st = X.scale_vq_books(sg.stereo_setup(), 130)
    assert all(np.isinf(_unpack(cb.delta)) for cb in st.codebooks if cb.lookup_type)
    st = X.scale_vq_books(sg.stereo_setup(), 126)
    assert all(np.isfinite(_unpack(cb.delta)) for cb in st.codebooks if cb.lookup_type)
    assert np.isneginf(_unpack(st.codebooks[4].minimum))                          # -8 * 2^126


def test_scaled_residue_is_the_unscaled_one_times_the_scale():
    """the packets written for the unscaled setup decode for the scaled one: the same symbols, every residue value times 2^20"""
    base = sg.stereo_setup()
    pk = sg.make_stream(base, "LLSSL", 5, seed=3)
    taps = []
    for st in (base, X.scale_vq_books(base, 20)):
        o_id, o_st = oracle_headers(st)
        pw = po.Pwr()
        taps.append([po.read_audio_packet(o_id, o_st, p, pw, "f32", taps=True)[1]["residue_pre_inverse"] for p in pk])
    for a, b in zip(*taps):
        assert np.any(a != 0) and np.array_equal(a * np.float32(2.0 ** 20), b)


def test_only_copies_the_books_a_residue_names():
    base = sg.surround51_setup()
    st = X.scale_vq_books(base, 126, only=1)
    assert len(st.codebooks) == len(base.codebooks) + 4 and st.residues[0].books == base.residues[0].books
    for row0, row1 in zip(base.residues[1].books, st.residues[1].books):
        for b0, b1 in zip(row0, row1):
            assert (b0 < 0) == (b1 < 0)
            if b0 >= 0:
                assert b1 >= len(base.codebooks) and st.codebooks[b1].delta == base.codebooks[b0].delta * 2.0 ** 126
                assert st.codebooks[b0].delta == base.codebooks[b0].delta and st.codebooks[b1].lengths == base.codebooks[b0].lengths
    lo = X.long_only(sg.stereo_setup(), 126)
    assert lo.residues[0].books == sg.stereo_setup().residues[0].books and lo.residues[1].books != sg.stereo_setup().residues[1].books
    sub = X.one_submap(base, 126, 1)
    assert [r.books == b.books for r, b in zip(sub.residues, base.residues)] == [True, True, False, False]


# ---- the classes on the oracle's output ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,cls,k,fmts", X.case_ids(), ids=["%s-%s-%d" % c[:3] for c in X.case_ids()])
def test_oracle_output_is_of_the_class_and_its_i16_is_as_i16(name, cls, k, fmts):
    cor = X.corpus(name, cls, k)
    assert all(rc == 0 for rc, _ in cor.want.values())
    assert X.CLASSES[cls][1](cor)
    for key, (rc, w) in cor.want.items():                                         # samples.rs:92-103 in numpy
        assert np.array_equal(cor.want_i16[key], X.to_i16(w)), key


def test_every_family_sees_the_base_classes_in_every_format():
    seen = {}
    for name, cls, k, fmts in X.case_ids():
        seen.setdefault(cls, set()).update(fmts)
        assert fmts[0].startswith("i16") and fmts[1].startswith("f32")
    assert all(len(seen[c]) == 4 for c in X.BASE), seen
    by_kernel = lambda kern: {cls for c in X.CASES.values() if kern in c["expect"] for cls in c["classes"]}
    for kern in ("k_long", "k_prep", "k_mix", "k_long10", "k_mix10", "k_long12", "k_short", "k_big", "k_entropy"):
        assert set(X.BASE) <= by_kernel(kern), kern
    assert set(X.BASE) <= set(X.CASES["generic_forced_51"]["classes"]) and "force_generic" in X.CASES["generic_forced_51"]["kw"]
    # the families of long-block kernels and the generic path also see the partial scalings, vanishing and overflow
    wide = {"long_only", "short_only", "one_submap0", "one_submap1", "vanishing", "overflow"}
    assert wide <= by_kernel("k_long") | by_kernel("k_mix")
    assert wide <= by_kernel("k_long10") | by_kernel("k_mix10")
    assert wide <= by_kernel("k_long12")
    assert wide <= by_kernel("k_ola_generic")
    # a NaN overlap before a finite flat part through every kernel that takes a short-to-long edge, and across launches
    for name in ("k_mix", "k_long_edge_dense", "k_mix10", "k_long12_edge", "generic_forced_51", "launches_stereo", "launches_9_12"):
        assert "short_only" in X.CASES[name]["classes"], name
    # and every kernel that undoes a coupling meets the non-finite angle beside a finite magnitude
    for kern in ("k_long", "k_mix", "k_long10", "k_long12", "k_short", "k_big", "k_ola_generic", "k_entropy"):
        assert set(X.ANGLE) <= by_kernel(kern), kern


@pytest.mark.parametrize("k", range(121, 126))
def test_no_scale_gives_an_infinite_sample(k):
    """the scan the `brink` class was to be chosen from (extreme_cases.py): an inf does not survive the transform"""
    base = sg.stereo_setup()
    streams = X.make_streams(base, "LLSSLSL", 14, 2, 5, p_floor_unused=0.05)
    x = X.Corpus(X.scale_vq_books(base, k), streams).samples()
    assert not np.isinf(x).any()
    assert np.isnan(x).any() == (k >= 124) and np.isfinite(x).any() == (k <= 124)


def test_oracle_sample_i16_on_hand_made_values():
    """`fl * 32768.0` in f32, > 32767 -> 32767, < -32768 -> -32768, else `as i16` (NaN -> 0, truncation toward zero)"""
    f = np.float32
    cases = [(np.nan, 0), (-np.nan, 0), (np.inf, 32767), (-np.inf, -32768), (2.0 ** 16, 32767), (-2.0 ** 16, -32768),
             (2.0 ** 113, 32767), (-2.0 ** 113, -32768),           # x finite, x * 32768 = +-inf
             (65536.0 - 2.0 ** -8, 32767), (-65536.0, -32768),     # x * 32768 = 2^31 - 128: the last f32 below 2^31; -2^31
             (2.0 ** -149, 0), (-2.0 ** -149, 0), (2.0 ** -127, 0), (-0.0, 0), (0.99999, 32767), (-1.0, -32768),
             (1.0 - 2.0 ** -15, 32767), (-1.0 + 2.0 ** -16, -32767), (2.0 ** -15, 1), (-(2.0 ** -15), -1), (1.9 * 2.0 ** -15, 1)]
    for x, want in cases:
        assert po.lib().lwo_sample_i16(f(x)) == want == int(X.to_i16(np.array([x], f))[0]), x


# ---- the corpora through the kernels' models ------------------------------------------------------------------------------------
MODEL_CLASSES = [(c, k) for c in X.BASE for k in X.CLASSES[c][0]]


def _taps(name, cls, k, count):
    """oracle taps of the first `count` packets of stream 0 of a GPU case's corpus (whose class condition is asserted): per packet
    (n, samples [ch][m], pre_mdct [ch][n/2], post_mdct [ch][n])"""
    cor = X.corpus(name, cls, k)
    assert X.CLASSES[cls][1](cor)
    o_id, o_st = oracle_headers(cor.setup)
    pw = po.Pwr()
    out = []
    for p in cor.streams[0][:count]:
        smp, t = po.read_audio_packet(o_id, o_st, p, pw, "f32", taps=True)
        out.append((t["n"], smp, t["pre_mdct"], t["post_mdct"]))
    return out


@pytest.mark.parametrize("cls,k", MODEL_CLASSES)
def test_fast_model_k_long(cls, k):
    blob, offs, _, _ = fast_image(X.CASES["k_long_coupled"]["mk"]())
    img = fm.Image(blob, offs)
    W = po.tables(11)[3]
    pk = _taps("k_long_coupled", cls, k, 3)
    with np.errstate(all="ignore"):
        for (_, _, _, prev), (_, smp, spec, td) in zip(pk[:-1], pk[1:]):
            for c in range(2):
                got, ola = fm.imdct_wave_pk(spec[c], img, prev_pb=prev[c][1024:1536], window=W)
                assert f32_identical(got, td[c]) and f32_identical(ola, smp[c]), (cls, c)


@pytest.mark.parametrize("cls,k", MODEL_CLASSES)
@pytest.mark.parametrize("case,L", [("k_short_256", 8), ("k_short_512", 16), ("k_short_1024", 32)])
def test_short_model_k_short(case, L, cls, k):
    img = sm.Image(short_image(X.CASES[case]["mk"](), 0)[0], L)
    S, n2, n4 = 64 // L, 16 * L, 8 * L
    pk = _taps(case, cls, k, 16)
    # the S blocks of one wave: short blocks behind a short block ("SSSL": packets 1, 2, 5, 6, ...), both channels
    pairs = [(a, b) for a, b in zip(pk[:-1], pk[1:]) if a[0] == b[0] == 2 * n2][:max(1, S // 2)]
    blk = [(a, b, c) for a, b in pairs for c in range(2)][:S]
    assert len(blk) == S
    spec = np.stack([b[2][c] for a, b, c in blk])
    prev = np.stack([a[3][c][n2:n2 + n4] for a, b, c in blk])
    with np.errstate(all="ignore"):
        blocks, ola, pb = sm.imdct_wave(spec, img, prev)
    for g, (a, b, c) in enumerate(blk):
        assert f32_identical(blocks[g], b[3][c]) and f32_identical(ola[g], b[1][c]) and f32_identical(pb[g], b[3][c][n2:n2 + n4]), (g, cls)


@pytest.mark.parametrize("cls,k", MODEL_CLASSES)
def test_long12_model_k_long12(cls, k):
    img = lm.Image(long12_image(X.CASES["k_long12"]["mk"]())[0])
    A = po.tables(12)[0]
    (_, _, _, prev), (_, smp, spec, td) = _taps("k_long12", cls, k, 2)
    with np.errstate(all="ignore"):
        for c in range(2):
            got, ola, pb = lm.imdct_wave(spec[c], img, A, prev[c][lm.N2:lm.N2 + lm.N4].copy())
            assert f32_identical(got, td[c]) and f32_identical(ola, smp[c]) and f32_identical(pb, td[c][lm.N2:lm.N2 + lm.N4]), (cls, c)


@pytest.mark.parametrize("cls,k", MODEL_CLASSES)
def test_big_model_k_big(cls, k):
    n2, n4 = 4096, 2048
    tabs = po.tables(13)
    (_, _, _, prev), (_, smp, spec, td) = _taps("k_big", cls, k, 2)      # "LLSL": two long blocks; the second returns the overlap and, before the short block, part of its flat right half
    with np.errstate(all="ignore"):
        got, ola, pb = bm.block(spec[0], 13, tabs, prev[0][n2:n2 + n4][::-1].copy())
    assert f32_identical(got, td[0]) and f32_identical(ola, smp[0][:n2]) and f32_identical(pb, td[0][n2:n2 + n4][::-1])
