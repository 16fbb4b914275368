"""The window-state contract (include/lewton_amd.h "PreviousWindowRight") on the GPU, once per synthesis kernel
family (-m gpu): a launch writes the OTHER parity buffer of a stream's slot, so an uploaded batch can be launched again and a
launched batch can be dropped (lw_pwr_get_state / lw_pwr_set_state); lw_pwr_clone forks a stream; lw_pwr_reset empties it;
lw_pwr_free hands the slot to the next lw_pwr_new; the pool keeps every live state when it moves.

Decoding forwards cannot see any of this -- a family that ignored LW_RF_PARITY_IN / LW_RF_PARITY_OUT would be self-consistent from
batch to batch -- so every family goes through the same scenario (phases A-F of _scenario) and names its kernel in
lw_batch_last_kernels.  Every sample of every packet is compared with oracle.pyoracle for equality (f32 through uint32 views), every
stored right part is pwr.data() against Pwr.data(ch) bit for bit, and clone / reset are checked against the oracle's own
Pwr.clone() / Pwr.reset().  Every test makes a fresh setup, hence a fresh decoder and an empty pool."""
import ctypes as C

import numpy as np
import pytest

from common import FLOOR0_SETUPS, SETUPS, oracle_headers, po, sg
from test_gpu_long10 import _decoder, _same

pytestmark = pytest.mark.gpu

GENERIC = {"k_decouple", "k_imdct_generic", "k_ola_generic"}


def _floor_of_65_posts():
    from test_gpu_prep import CASES
    return CASES["floor_of_65_posts"][0]()   # (its plan names k_prep: test_plan_sends_the_shape_through_k_prep_not_the_generic_kernels)


def fam(setup, pattern, want, hooks=(), never=(), only=None, streams=6, cut=(18, 30), tail=5, distinct=0, writer=sg.PacketWriter,
        no_generic_in=()):
    """setup: a name of SETUPS / FLOOR0_SETUPS or a callable; hooks: (Batch method, argument) pairs; want: kernels that phases A and C
    must both name; never: kernels they must not name; only: the set all their kernels must come from; cut: the range the cuts
    c_s are chosen from; tail: packets per stream of phase C; distinct: > 0 = streams are drawn from a pool of that many packets;
    writer: the packet writer (a setup with a random floor needs the one that draws among the entries its books use); no_generic_in:
    phases whose launches must not name a generic kernel"""
    return dict(setup=setup, pattern=pattern, want=set(want), hooks=tuple(hooks), never=set(never), only=only, streams=streams,
                cut=cut, tail=tail, distinct=distinct, writer=writer, no_generic_in=tuple(no_generic_in))


FAMILIES = {
    "k_long_stereo": fam("stereo", "L", {"k_long"}),
    "k_long_surround51": fam("surround51", "L", {"k_long"}),
    # chunk starts inside a stream.  A forced round count keeps the predecessors in the pre-pass launch whatever the halo hook says
    # (lw_batch.cpp: inline_halo = halo_mode != 0 && !forced_rounds), so both hooks of the first two name k_long<halo>; the items inside
    # the launch need the planner's own shape and a stream long enough for chunks of four packets and more: 1024 packets per launch
    "k_long_chunks_halo_pre_pass": fam("stereo", "L", {"k_long", "k_long<halo>"}, [("debug_set_rounds", 1), ("debug_set_halo", 0)],
                                       streams=1, cut=(48, 48), tail=40),
    "k_long_chunks_halo_default": fam("stereo", "L", {"k_long", "k_long<halo>"}, [("debug_set_rounds", 1), ("debug_set_halo", -1)],
                                      streams=1, cut=(48, 48), tail=40),
    "k_long_chunks_halo_items": fam("stereo", "L", {"k_long"}, [("debug_set_halo", -1)], never={"k_long<halo>"},
                                    streams=1, cut=(1024, 1024), tail=1024, distinct=64),
    "k_mix": fam("stereo", "LLSSSSLLSL", {"k_mix"}, [("debug_set_mix", -1)]),
    "k_long_edge_k_short8": fam("stereo", "LLSSSSLLSL", {"k_long", "k_short"}, [("debug_set_mix", 0)], never={"k_mix"}),
    "k_long10": fam("stereo_9_10", "L", {"k_long10"}, never={"k_short"}),
    "k_mix10_9_10": fam("stereo_9_10", "LLLSSSLLLL", {"k_mix10"}),
    "k_mix10_8_10": fam("stereo_8_10", "LLLSSSLLLL", {"k_mix10"}),
    "k_long10_edge_k_short16": fam("stereo_9_10", "LLLSSSLLLL", {"k_long10", "k_short"}, [("debug_set_mix", 0)], never={"k_mix10"}),
    "k_long10_edge_k_short8": fam("stereo_8_10", "LLLSSSLLLL", {"k_long10", "k_short"}, [("debug_set_mix", 0)], never={"k_mix10"}),
    "k_short16_long_role": fam("stereo_8_9", "LLLSSL", {"k_short"}),
    "k_short32_long_role": fam("stereo_9_10", "L", {"k_short"}, [("debug_set_long10", 0)], never={"k_long10"}),
    "k_long12": fam("stereo_9_12", "L", {"k_long12"}, never={"k_big"}),
    # (the EDGE form: long blocks with a short slope stay off the generic kernels.  Behind a failing packet the stored right part
    # does not fit the next block's slope and that block goes to the generic kernels: phases A, C and D; E and F have no such packet)
    "k_long12_edge": fam("stereo_9_12", "LLSSL", {"k_long12", "k_short"}, no_generic_in=("E", "F")),
    "k_long12_tdonly_k_ola_generic": fam("stereo_10_12", "LSSSSL", {"k_long12", "k_ola_generic"}),
    "k_big12": fam("stereo_9_12", "LLSSL", {"k_big"}, [("debug_set_long10", 0)], never={"k_long12"}),
    # (the issue's "LSSL" has no long block between two long ones, the only window k_big takes: lw_batch.cpp plans every long block of
    # that pattern on the generic kernels.  "LLLSSL" keeps the L-S-S-L run next to 64-point blocks and gives k_big its blocks.)
    "k_big13": fam("stereo_6_13", "LLLSSL", {"k_big"}),
    "generic_7_7": fam("stereo_7_7", "LSLL", {"k_imdct_generic", "k_ola_generic"}, only=GENERIC),
    "generic_forced": fam("stereo", "LLSSL", {"k_imdct_generic", "k_ola_generic"}, [("set_force_generic", True)], only=GENERIC),
    "k_prep": fam(_floor_of_65_posts, "LLSSL", {"k_prep"}, writer=sg.RandomPacketWriter),
    "floor0": fam("floor0_mixed", "LSLLS", {"k_prep", "k_long10"}),          # (the long blocks' floor-0 curves reach k_long10 through k_prep)
    "k_entropy": fam("stereo", "LLSSL", {"k_entropy"}, [("set_entropy_on_device", True)]),
}

CLASSES = ("long_between_long", "long_short_right", "inside_short_run", "last_short_before_long", "after_failed", "after_unused_floor")


def _setup_of(f):
    s = f["setup"]
    return s() if callable(s) else dict(SETUPS, **FLOOR0_SETUPS)[s]()


def _head(setup, pkt):
    """(block flag, previous window flag, next window flag, channel 0's floor unused) from a packet's first bits: bit 0 the packet
    type, ilog(modes - 1) mode bits, the two window flags of a long block, then channel 0's floor -- one flag bit of a floor 1, the
    amplitude of a floor 0 (audio.rs:921-938, :109-121, :226-229)"""
    bits = int.from_bytes(pkt[:8], "little")
    pos = 1
    mb = sg.ilog(len(setup.modes) - 1)
    mode = bits >> pos & ((1 << mb) - 1)
    pos += mb
    md = setup.modes[mode]
    pf = nf = 0
    if md.blockflag:
        pf, nf = bits >> pos & 1, bits >> pos + 1 & 1
        pos += 2
    mp = setup.mappings[md.mapping]
    fl = setup.floors[mp.submap_floor[mp.mux[0]]]
    width = fl.amplitude_bits if isinstance(fl, sg.Floor0) else 1
    return md.blockflag, pf, nf, (bits >> pos & ((1 << width) - 1)) == 0


def _is_class(setup, pk, c, cls):
    """is the right part stored after packet c - 1 of `pk` what `cls` says (read from the packets' mode and window bits)"""
    if cls == "after_failed":
        return True                          # (any cut: packet c - 1 is then replaced by the failing one)
    bf, _pf, nf, unused = _head(setup, pk[c - 1])
    if cls == "long_between_long":
        return bool(bf and _head(setup, pk[c - 1])[1] and nf)
    if cls == "long_short_right":
        return bool(bf and not nf)
    if cls == "inside_short_run":
        return not bf and not _head(setup, pk[c])[0]
    if cls == "last_short_before_long":
        return not bf and bool(_head(setup, pk[c])[0])
    return bool(unused)


def _choose_cuts(setup, streams, lo, hi):
    """one (cut, class) per stream: every class that some stream has in [lo, hi] is taken by a stream of its own (a matching, six by
    six at most), the streams left over take the first class they have.  Returns (cuts, classes, classes some stream has)."""
    n = len(streams)
    has = [{cls: [c for c in range(lo, hi + 1) if _is_class(setup, streams[s], c, cls)] for cls in CLASSES} for s in range(n)]
    cuts, classes = [None] * n, [None] * n
    avail = [cls for cls in CLASSES if any(h[cls] for h in has)]

    def match(k, taken):                     # the first assignment of a stream of its own to each of avail[k:], or None
        if k == len(avail):
            return []
        for s in range(n):
            if s not in taken and has[s][avail[k]]:
                rest = match(k + 1, taken | {s})
                if rest is not None:
                    return [s] + rest
        return None

    for cls, s in zip(avail, (match(0, frozenset()) if n >= len(avail) else None) or []):
        cuts[s], classes[s] = has[s][cls][0], cls
    for s in range(n):                       # streams left over (or fewer streams than classes): the first class they have
        if cuts[s] is None:
            cls = next(c for c in CLASSES if has[s][c])
            cuts[s], classes[s] = has[s][cls][0], cls
    return cuts, classes, set(avail)


def _packets(f, setup, count, seed):
    """make_stream with the family's writer: mode 0 the short blocks, mode 1 the long ones"""
    pw = f["writer"](setup, seed, p_floor_unused=0.1)
    return [pw.packet(1 if bf else 0, pf, nf) for bf, pf, nf in sg.block_sequence(f["pattern"], count)]


_MATERIAL = {}


def _material(name):
    """the setup and the streams of one family's scenario, their cuts, the cuts' classes and the index of each stream's failing
    packet; made once per family and left unchanged (a fresh setup, hence a fresh decoder, per call)"""
    f = FAMILIES[name]
    setup = _setup_of(f)
    if name not in _MATERIAL:
        _MATERIAL[name] = _make_material(f, setup)
        _check_cuts(name, f, setup, *_MATERIAL[name])
    return (setup,) + _MATERIAL[name]


def _make_material(f, setup):
    lo, hi = f["cut"]
    n, length = f["streams"], hi + f["tail"] + 20
    if f["distinct"]:                        # an all-long pattern: every order of its packets is a stream
        pool = _packets(f, setup, f["distinct"], 6100)
        rng = np.random.default_rng(61)
        streams = [[pool[int(i)] for i in rng.integers(0, len(pool), length)] for _ in range(n)]
    else:
        streams = [_packets(f, setup, length, 6100 + 13 * s) for s in range(n)]
    cuts, classes, avail = _choose_cuts(setup, streams, lo, hi)
    fails = []
    for s in range(n):
        # the failing packet: an empty one, EndOfPacket at its first bit (audio.rs:921-922; a packet cut anywhere behind its mode bits
        # decodes: the end of the packet inside a floor or a residue is no error, audio.rs:99, :701).  In front of the cut, right at it,
        # or inside the tails of phases C and D
        at = cuts[s] - 1 if classes[s] == "after_failed" else (cuts[s] + 2 if s % 2 else cuts[s] - 4)
        streams[s][at] = b""
        fails.append(at)
    return streams, cuts, classes, avail, fails


def _check_cuts(name, f, setup, streams, cuts, classes, avail, fails):
    """the chosen cuts read back from the packets' own mode and window bits, and six streams cover every class their pattern has"""
    pat = 3 * f["pattern"]
    expect = {"after_failed"} | ({"long_between_long"} if "LLL" in pat else set()) | ({"inside_short_run"} if "SS" in pat else set()) | \
        ({"long_short_right", "last_short_before_long"} if "S" in pat else set())
    assert expect <= avail, (name, expect, avail)
    if f["streams"] >= len(CLASSES):
        assert set(classes) == avail, (name, classes, avail)
    for s, (c, cls) in enumerate(zip(cuts, classes)):
        pk = streams[s]
        assert f["cut"][0] <= c <= f["cut"][1] and sum(p == b"" for p in pk) == 1 and pk[fails[s]] == b"", (name, s)
        if cls == "after_failed":
            assert pk[c - 1] == b"", (name, s)
            continue
        bf, pf, nf, unused = _head(setup, pk[c - 1])
        nxt = _head(setup, pk[c])[0]
        assert {"long_between_long": bf and pf and nf, "long_short_right": bf and not nf, "inside_short_run": not bf and not nxt,
                "last_short_before_long": not bf and nxt, "after_unused_floor": unused}[cls], (name, s, cls)


def test_the_cuts_are_what_they_claim_to_be():
    """no GPU work of its own: every family's material is made here (and checked as it is made, _check_cuts), once for all the tests
    below"""
    for name in FAMILIES:
        _material(name)


class _Run:
    """one decoder, one Batch with the family's hooks, the product's and the oracle's streams side by side"""

    def __init__(self, f, setup, fmt, cap):
        from lewton_amd import _native as N
        from lewton_amd.batch import Batch
        self.N, self.fmt, self.setup, self.ch = N, fmt, setup, setup.channels
        self.audio, self.dec = _decoder(setup)
        self.o_id, self.o_st = oracle_headers(setup)
        self.bt = Batch(self.dec, cap, fmt)
        for hook, arg in f["hooks"]:
            assert getattr(self.bt, hook)(arg) in (None, True), hook
        self.kernels = {}

    def launch(self, phase, items, opws):
        """items: (packet, product stream, key of the oracle stream in opws); plans, uploads and launches them and compares status
        and samples of every packet with the oracle's, which decodes into opws.  Returns the launch's bytes and the results."""
        res = self.bt.entropy([(p, pw) for p, pw, _ in items], n_threads=2)
        self.bt.upload()
        flat = self.bt.synth_to_host().copy()
        self.kernels.setdefault(phase, set()).update(self.bt.last_kernels.split(","))
        got = self.bt.split(flat, self.ch)
        for i, (p, _pw, key) in enumerate(items):
            try:
                want, rc = np.asarray(po.read_audio_packet(self.o_id, self.o_st, p, opws[key], self.fmt)), 0
            except po.OracleError as e:
                want, rc = None, e.code
            assert res[i][0] == rc, (phase, i, key, res[i][0], rc)
            assert _same(got[i], want, self.fmt), (phase, i, key, self.bt.last_kernels)
            if rc == 0:
                assert res[i][1] * self.ch == want.size, (phase, i, key)
        return flat, res

    def relaunch(self, phase, flat):
        again = self.bt.synth_to_host()
        assert again.size == flat.size and np.array_equal(again.view(np.uint8), flat.view(np.uint8)), phase

    def same_state(self, pw, opw, tag):
        got, want = pw.data(), opw.data(self.ch)
        assert (got is None) == (want is None), tag
        if want is not None:
            assert got.shape == want.shape and np.array_equal(got.view(np.uint32), want.view(np.uint32)), tag

    def slot(self, pw):
        return self.N.lw_debug_pwr_slot(pw._h)

    def free(self, pw):
        self.N.lw_pwr_free(pw._h)
        pw._h = None


def _bits_of(state):
    return None if state is None else state.view(np.uint32).copy()


def _scenario(name, fmt):
    f = FAMILIES[name]
    setup, streams, cuts, classes, _avail, _fails = _material(name)
    n, tail = len(streams), f["tail"]
    R = _Run(f, setup, fmt, max(sum(cuts), n * tail, 2 * n * 8))
    pws = [R.audio.PreviousWindowRight() for _ in range(n)]
    opws = {s: po.Pwr() for s in range(n)}

    # A. forward: packets [0, c_s) of every stream, stream-major, from empty streams
    flat, res = R.launch("A", [(streams[s][t], pws[s], s) for s in range(n) for t in range(cuts[s])], opws)
    for s in range(n):
        R.same_state(pws[s], opws[s], ("A", s))
        # the packet in front of the cut decoded (its right part is the stored one), or is the failing one
        assert (res[sum(cuts[:s + 1]) - 1][0] != 0) == (classes[s] == "after_failed"), (s, classes[s])
    after_a = [_bits_of(pws[s].data()) for s in range(n)]
    assert any(a is not None for a in after_a)
    # B. the uploaded batch once more: the same bytes, the same stored right parts
    R.relaunch("B", flat)
    for s in range(n):
        R.same_state(pws[s], opws[s], ("B", s))

    # C. roll-back: a batch whose streams start from the pool, launched twice and dropped
    saved = [R.N.PwrState() for _ in range(n)]
    for s in range(n):
        R.N.lw_pwr_get_state(pws[s]._h, C.byref(saved[s]))
    oclones = {s: opws[s].clone() for s in range(n)}
    flat, _ = R.launch("C", [(streams[s][cuts[s] + t], pws[s], s) for s in range(n) for t in range(tail)], oclones)
    for s in range(n):
        R.same_state(pws[s], oclones[s], ("C", s))
    R.relaunch("C again", flat)
    for s in range(n):
        R.same_state(pws[s], oclones[s], ("C again", s))
        R.N.lw_pwr_set_state(pws[s]._h, C.byref(saved[s]))
        got = _bits_of(pws[s].data())
        assert (got is None) == (after_a[s] is None) and (got is None or np.array_equal(got, after_a[s])), ("C rolled back", s)

    # D. clone: every original goes on with its own tail, every twin with the tail of the next stream
    twins = [pw.clone() for pw in pws]
    for s in range(n):
        opws[("twin", s)] = opws[s].clone()
        assert R.slot(twins[s]) != R.slot(pws[s]) and R.slot(twins[s]) >= 0, s
    assert len({R.slot(p) for p in pws + twins}) == 2 * n
    nxt = [(s + 1) % n for s in range(n)]
    items = []
    for t in range(8):
        for s in range(n):
            items.append((streams[s][cuts[s] + t], pws[s], s))
            items.append((streams[nxt[s]][cuts[nxt[s]] + t], twins[s], ("twin", s)))
    R.launch("D", items, opws)
    for s in range(n):
        R.same_state(pws[s], opws[s], ("D", s))
        R.same_state(twins[s], opws[("twin", s)], ("D twin", s))

    # E. reset streams 0, 2 and 4; three more packets of every stream
    for s in range(0, min(n, 6), 2):
        pws[s].reset()
        opws[s].reset()
        assert pws[s].is_empty() and opws[s].is_empty()
    items = [(streams[s][cuts[s] + 8 + t], pws[s], s) for s in range(n) for t in range(3)]
    items += [(streams[nxt[s]][cuts[nxt[s]] + 8 + t], twins[s], ("twin", s)) for s in range(n) for t in range(3)]
    _, res = R.launch("E", items, opws)
    for s in range(0, min(n, 6), 2):
        assert res[3 * s][:2] == (0, 0), (s, res[3 * s])       # a stream's first packet after a reset: no samples (audio.rs:1140-1152)
    for s in range(n):
        R.same_state(pws[s], opws[s], ("E", s))
        R.same_state(twins[s], opws[("twin", s)], ("E twin", s))

    # F. free the twins; the next streams take exactly their slots, most recently freed first
    freed = [R.slot(tw) for tw in twins]
    stored = [_head(setup, streams[nxt[s]][cuts[nxt[s]] + 10])[0] for s in range(n)]   # block class of the last packet a twin stored
    for tw in twins:
        R.free(tw)
    fresh = [R.audio.PreviousWindowRight() for _ in range(n)]
    for pw in fresh:
        pw._bind(R.dec)
    assert [R.slot(pw) for pw in fresh] == freed[::-1], ([R.slot(pw) for pw in fresh], freed)
    items = []
    for j in range(n):
        was = stored[n - 1 - j]
        pk = streams[j]
        # where the pattern has both block classes: start with a block of the other class than the one the slot last stored
        first = next((i for i in range(len(pk) - 6) if pk[i] != b"" and bool(_head(setup, pk[i])[0]) != bool(was)), 0)
        assert set(f["pattern"]) != {"L", "S"} or bool(_head(setup, pk[first])[0]) != bool(was), j
        opws[("fresh", j)] = po.Pwr()
        items += [(pk[first + t], fresh[j], ("fresh", j)) for t in range(6)]
    items += [(streams[s][cuts[s] + 11 + t], pws[s], s) for s in range(n) for t in range(3)]
    R.launch("F", items, opws)
    for s in range(n):
        R.same_state(pws[s], opws[s], ("F", s))
        R.same_state(fresh[s], opws[("fresh", s)], ("F fresh", s))

    # the family's kernels, in the launches that read and wrote the pool
    print("\n[%s %s] kernels: %s" % (name, fmt, {k: sorted(v) for k, v in R.kernels.items()}))
    for phase in ("A", "C"):
        seen = R.kernels[phase]
        assert f["want"] <= seen and not (f["never"] & seen), (phase, seen)
        assert f["only"] is None or seen <= f["only"], (phase, seen)
    for phase in f["no_generic_in"]:
        assert not (GENERIC & R.kernels[phase]), (phase, R.kernels[phase])
    R.bt.close()


@pytest.mark.parametrize("fmt", ["i16", "f32"])
@pytest.mark.parametrize("name", sorted(FAMILIES))
def test_stream_state_contract(name, fmt):
    _scenario(name, fmt)


# ---- the pool moves while streams hold live state ------------------------------------------------------------------------------

GROWTH = {"k_long": ("stereo", "L", {"k_long"}), "k_mix": ("stereo", "LLSSSSLLSL", {"k_mix"}), "k_long12_edge": ("stereo_9_12", "LLSSL", {"k_long12"})}


class _Crowd:
    """many streams of one decoder, each a window into one of twelve packet sequences (neighbouring slots hold different states)"""

    def __init__(self, key):
        name, pattern, self.want = GROWTH[key]
        setup = SETUPS[name]()
        self.R = _Run(fam(name, pattern, self.want), setup, "i16", 300)
        self.seqs = [sg.make_stream(setup, pattern, 16, seed=6400 + q, p_floor_unused=0.1) for q in range(12)]
        self.pws, self.opws, self.done = [], {}, []

    def open(self, count, first_slot):
        for _ in range(count):
            s = len(self.pws)
            pw = self.R.audio.PreviousWindowRight()
            pw._bind(self.R.dec)
            assert self.R.slot(pw) == s and s >= first_slot, (s, self.R.slot(pw), first_slot)
            self.pws.append(pw)
            self.opws[s] = po.Pwr()
            self.done.append(0)

    def decode(self, phase, per):
        items = []
        for s, pw in enumerate(self.pws):
            q, at = s % 12, (s // 12) % 4 + self.done[s]
            items += [(self.seqs[q][at + t], pw, s) for t in range(per if self.done[s] else 2)]
            self.done[s] += per if self.done[s] else 2
        self.R.launch(phase, items, self.opws)
        for s, pw in enumerate(self.pws):
            self.R.same_state(pw, self.opws[s], (phase, s))


@pytest.mark.parametrize("key", sorted(GROWTH))
def test_pool_growth_keeps_live_state(key):
    """the pool starts at 64 slots and doubles (grow_state_to: synchronise, allocate, copy state_cap slots, free).  Every slot of the
    old pool holds live state when it moves -- the last one included: 64 streams, not 60 -- so a copy that is one slot short, or
    that copies one parity buffer, loses a stream.  Then the same through lw_decoder_reserve_streams, the exact-size path."""
    cr = _Crowd(key)
    cr.open(64, 0)
    cr.decode("64", 1)                       # two packets each: live state in slots 0 .. 63
    cr.open(10, 64)                          # the 65th stream moves the pool
    cr.decode("74", 1)
    cr.open(54, 74)
    cr.decode("128", 1)                      # live state in slots 0 .. 127
    cr.open(10, 128)                         # the 129th stream moves it again
    cr.decode("138", 1)
    cr.decode("138 again", 1)
    seen = set().union(*cr.R.kernels.values())
    assert cr.want <= seen, seen
    cr.R.bt.close()
    cr = _Crowd(key)
    cr.open(64, 0)
    cr.decode("64", 1)
    assert cr.R.dec.reserve_streams(100) == 0
    cr.open(36, 64)                          # exactly 100 slots: 64 .. 99 and no more
    cr.decode("100", 1)
    assert cr.R.dec.reserve_streams(101) == 0     # slot 99 holds live state while the pool moves
    cr.open(1, 100)
    cr.decode("101", 1)
    assert cr.R.dec.reserve_streams(64) == 0      # below the capacity: nothing moves
    cr.decode("101 again", 1)
    assert cr.want <= set().union(*cr.R.kernels.values())
    cr.R.bt.close()


# ---- a freed slot's next stream behind a launch that is still in flight ------------------------------------------------------------

def test_ring_freed_slots_reused_behind_a_launch_in_flight():
    """lw_ring_launch orders a launch behind the previous one.  Streams A are freed straight after the submit of their last packets,
    streams B take their slots and are submitted twice before anything is collected: B's first batch writes the slots that A's
    batch, still in flight, reads and writes.  In launch order B's second batch finds B's right parts, not A's.  (The pool's memory
    stays valid throughout: nothing here can fault.)"""
    from lewton_amd import _native as N
    from lewton_amd.ring import Ring
    setup = SETUPS["stereo"]()
    audio, dec = _decoder(setup)
    o_id, o_st = oracle_headers(setup)
    n, per = 12, 10
    ring = Ring(dec, 3, n * per, "i16")
    sa = [sg.make_stream(setup, "LLSSSSLLSL", 2 * per, seed=6700 + s, p_floor_unused=0.1) for s in range(n)]
    sb = [sg.make_stream(setup, "SLLSSLLLSS", 2 * per, seed=6800 + s, p_floor_unused=0.1) for s in range(n)]
    pa = [audio.PreviousWindowRight() for _ in range(n)]
    oa, ob = [po.Pwr() for _ in range(n)], [po.Pwr() for _ in range(n)]

    def check(streams, opws, lo, res, pcm):
        k = 0
        for s in range(n):
            for t in range(lo, lo + per):
                want = np.asarray(po.read_audio_packet(o_id, o_st, streams[s][t], opws[s], "i16")).reshape(-1)
                status, m, off = res[k]
                assert status == 0 and 2 * m == want.size and np.array_equal(pcm[off:off + 2 * m], want), (s, t)
                k += 1

    ring.submit(ring.marshal([(sa[s][t], pa[s]) for s in range(n) for t in range(per)]), n_threads=2)
    res, pcm = ring.collect()
    ring.release()
    check(sa, oa, 0, res, pcm)                                     # A's streams hold live state
    ring.submit(ring.marshal([(sa[s][per + t], pa[s]) for s in range(n) for t in range(per)]), n_threads=2)
    slots_a = [N.lw_debug_pwr_slot(p._h) for p in pa]
    for p in pa:                                                   # freed while their last batch is in flight
        N.lw_pwr_free(p._h)
        p._h = None
    pb = [audio.PreviousWindowRight() for _ in range(n)]
    for p in pb:
        p._bind(dec)
    assert [N.lw_debug_pwr_slot(p._h) for p in pb] == slots_a[::-1]
    ring.submit(ring.marshal([(sb[s][t], pb[s]) for s in range(n) for t in range(per)]), n_threads=2)
    ring.submit(ring.marshal([(sb[s][per + t], pb[s]) for s in range(n) for t in range(per)]), n_threads=2)
    assert ring.in_flight == 3
    for streams, opws, lo in ((sa, oa, per), (sb, ob, 0), (sb, ob, per)):
        res, pcm = ring.collect()
        ring.release()
        check(streams, opws, lo, res, pcm)
    for s in range(n):
        assert np.array_equal(pb[s].data().view(np.uint32), ob[s].data(2).view(np.uint32)), s
    ring.close()
