"""The synthesis kernels on subnormal, saturating and non-finite samples (-m gpu).

Every other GPU test decodes what streamgen's packet writers produce: |x| < 1000, no subnormal, no inf, no NaN.  Here the same
packets are decoded for setups whose VQ books are scaled by a power of two (tests/extreme_cases.py), so that the residue, the
spectrum, the transform's sums, the window state and the samples are subnormal (quiet, vanishing), beyond the i16 and the i32
range (loud), beyond f32 once multiplied by 32768 (huge), NaN made by the transform (overflow), NaN / inf from the VQ table on
(nonfinite), or all of that next to finite blocks and channels (long_only, short_only, one_submap), or meet finite values in the inverse
coupling, whose comparisons a NaN answers differently (angle_nan, angle_huge, magnitude_nan).  Each case names the kernel it is meant for
(Batch.last_kernels) and asserts its class condition on the ORACLE's samples before anything is compared.

f32: bit-identical to the oracle, signs of zeros and infinities included; a NaN equals a NaN (common.f32_identical).  i16: exactly
the oracle's, i.e. `as i16` of samples.rs:92-103 -- NaN gives 0, x * 32768 = +-inf and everything beyond +-2^31 full scale.
Statuses equal the oracle's, and so does every stream's final PreviousWindowRight.

test_imdct_hand_made_spectra: single non-finite bins, FLT_MAX everywhere, the smallest subnormal everywhere, -0.0 everywhere and a
subnormal bin in a normal spectrum through lw_debug_imdct against the oracle's transform."""
import numpy as np
import pytest

import extreme_cases as X
from common import SETUPS, f32_identical, po

pytestmark = pytest.mark.gpu


def _product(setup):
    from lewton_amd import audio, header
    idp, _, stp = setup.headers()
    ident = header.read_header_ident(idp)
    st = header.read_header_setup(stp, ident.audio_channels, (ident.blocksize_0, ident.blocksize_1))
    return audio, ident, st


def _decode(setup, streams, fmt, launches=1, force_generic=False, device_entropy=False):
    """all streams' packets, stream-interleaved, in `launches` batches (the window state crosses them); returns
    ({(s, t): (status, samples)}, kernels of every launch, every stream's final window state)"""
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
        assert bt.device_status() == 0
        kernels.append(bt.last_kernels)
        for (s, t), r, blk in zip(items, res, bt.split(flat, ident.audio_channels)):
            out[(s, t)] = (r[0], blk)
    states = [pw.data() for pw in pws[:X.DISTINCT]]
    bt.close()
    return out, kernels, states


@pytest.mark.parametrize("name,cls,k,fmts", X.case_ids(), ids=["%s-%s-%d" % c[:3] for c in X.case_ids()])
def test_extreme_values(name, cls, k, fmts):
    case = X.CASES[name]
    cor = X.corpus(name, cls, k)
    assert X.CLASSES[cls][1](cor), "the oracle's samples are not of class " + cls
    if cls == "nonfinite" and k == 130:
        assert any(np.isinf(po.lib().lwo_float32_unpack(X.sg.float32_pack(cb.delta))) for cb in cor.setup.codebooks if cb.lookup_type)
    d = len(cor.streams)
    streams = [cor.streams[s % d] for s in range(case["n"])]
    run = {a: b for a, b in case["kw"].items() if a not in X.WRITER_KW}
    ch = cor.setup.channels
    seen = None
    for fmt in fmts:
        got, kernels, states = _decode(cor.setup, streams, fmt, **run)
        ran = {kk for launch in kernels for kk in launch.split(",")}
        assert set(case["expect"]) <= ran, (case["expect"], kernels)               # exact names: "k_long" is not "k_long12"
        if name in X.EDGE_CASES:
            assert not ran & set(X.GENERIC_KERNELS), kernels                      # the transitions ran in the EDGE form
        assert seen is None or seen == kernels, (seen, kernels)            # both formats through the same kernels
        seen = kernels
        checked = 0
        for (s, t), (g_rc, g) in got.items():
            rc, w = cor.want[(s % d, t)]
            assert g_rc == rc, (s, t, g_rc, rc)
            if rc:
                continue
            if fmt.startswith("i16"):
                w = cor.want_i16[(s % d, t)]
                w = np.ascontiguousarray(w.T).reshape(-1) if fmt.endswith("interleaved") else w
                assert g.dtype == np.int16 and g.shape == w.shape and np.array_equal(g, w), (fmt, s, t)
            else:
                w = np.ascontiguousarray(w.T).reshape(-1) if fmt.endswith("interleaved") else w
                assert g.dtype == np.float32 and g.shape == w.shape and f32_identical(g, w), (fmt, s, t)
            checked += 1
        assert checked > 0
        for s, g in enumerate(states):                                     # the right half each stream leaves in the state pool
            w = cor.state[s % d]
            assert (g is None) == (w is None) and (g is None or (g.shape == w.shape and f32_identical(g, w))), (fmt, s)


def _spectra(n2):
    rng = np.random.default_rng(n2)
    f = np.float32
    sub = f(2.0 ** -149)
    one_inf = (rng.standard_normal(n2) * 0.2).astype(f)
    one_inf[n2 // 3] = np.inf
    one_nan = (rng.standard_normal(n2) * 0.2).astype(f)
    one_nan[2 * n2 // 3 + 1] = np.nan
    alt = np.full(n2, np.finfo(f).max, f)
    alt[1::2] *= f(-1)
    one_sub = (rng.standard_normal(n2) * 0.2).astype(f)
    one_sub[n2 // 5] = -sub
    return {"one_inf": one_inf, "one_nan": one_nan, "flt_max_alternating": alt, "smallest_subnormal": np.full(n2, sub, f),
            "minus_zero": np.full(n2, -0.0, f), "one_subnormal_bin": one_sub}


@pytest.mark.parametrize("name", ["stereo", "stereo_9_12", "stereo_6_13"])
def test_imdct_hand_made_spectra(name):
    from lewton_amd import _native as N
    setup = SETUPS[name]()
    audio, ident, st = _product(setup)
    dec = audio.decoder_for(ident, st)
    for flag, bs in ((0, setup.bs0), (1, setup.bs1)):
        n = 1 << bs
        for what, x in _spectra(n // 2).items():
            want = po.inverse_mdct(x, bs)
            if what == "one_inf" or what == "one_nan":
                assert np.isnan(want).any()
            elif what == "smallest_subnormal":
                assert np.any((want != 0) & (np.abs(want) < np.finfo(np.float32).tiny))
            elif what == "minus_zero":
                assert np.all(want == 0)
            out = np.zeros(n, np.float32)
            assert N.lw_debug_imdct(dec._h, flag, x.ctypes.data_as(N.f32p), out.ctypes.data_as(N.f32p)) == 0, N.device_error()
            assert f32_identical(out, want), (name, bs, what)
