#!/usr/bin/env python3
"""Cost of stream-major rows (lw_rows_synth = lw_batch_synth + k_rows) next to the packet-major launch it wraps.

Shape: BASELINE configs[1] (256 coupled stereo streams x packets / 256 consecutive long packets, every timed packet yields 1024
samples per channel), rows [256][2][samples of the batch].  Per format, alternated in the same process, HIP events around
--steps steps each, batches rotated over >= 0.5 GiB (tools/bench_configs.py::rotation_batches; every rotated batch has its own
PCM buffer, its own rows tensor and its own lw_rows object, so that neither the staging buffer nor the rows stay in the
Infinity Cache):
  (a) synth      lw_batch_synth alone (packet-major, what exists without this feature)
  (b) rows       lw_rows_synth, co-aligned (every piece's source and destination congruent mod 16 bytes)
  (b5) rows_skip5  the same with skip = 5 on the first packet of every row: every later piece is shifted
  (c) copy       the yardstick: dst.copy_(src) of as many elements between two contiguous torch tensors
Plain launches, no hipGraph (lw_rows_synth rotates pinned descriptor arrays under events): at 4096 packets per step a step
is short enough for the host's enqueue rate to show in (a) and (b); the kernel's own time comes from
    rocprofv3 --kernel-trace --stats -- python tools/bench_rows.py --kernel-only rows
which runs (b) alone (rows_skip5: (b5)).  --e2e adds decode_streams end to end (device entropy stage, PCM staying on the GPU) next to the staging
ring of lewton_amd/e2e.py in the same process.
    python tools/bench_rows.py [--packets 4096,16384] [--formats i16,f32] [--steps 200] [--rounds 3] [--e2e]"""
import argparse
import ctypes as C
import dataclasses
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from bench_configs import rotation_batches  # noqa: E402
from lewton_amd import audio, header, rows as R, streamgen as sg, workloads as wl  # noqa: E402
from lewton_amd.batch import Batch  # noqa: E402


def build(packets, fmt):
    w = dataclasses.replace(wl.by_key("9", packets // 2), key="1")
    setup = w.setup()
    idp, _, stp = setup.headers()
    ident = header.read_header_ident(idp)
    st = header.read_header_setup(stp, ident.audio_channels, (ident.blocksize_0, ident.blocksize_1))
    dec = audio.decoder_for(ident, st, torch.cuda.current_device())
    NP, ch = w.n_streams * w.per_stream, ident.audio_channels
    seqs0 = wl.stream_material(w, setup, batch=0)
    dt = torch.float32 if fmt.startswith("f32") else torch.int16
    slots, nb, b = [], None, 0
    while nb is None or b < nb:
        pw = [audio.PreviousWindowRight() for _ in range(w.n_streams)]
        seqs = seqs0[b % len(seqs0):] + seqs0[:b % len(seqs0)]
        prime_items, items = wl.items_of(w, seqs, pw)
        prime = Batch(dec, w.n_streams, fmt)
        prime.entropy(prime_items)
        prime.upload(None)
        prime.synth_to_host(None)
        prime.close()
        bt = Batch(dec, NP, fmt)
        res = bt.entropy(items)
        bt.upload(None)
        if nb is None:
            nb = rotation_batches(bt.algorithmic_bytes)
        assert all(s == 0 for s, m, o in res)
        m = np.array([r[1] for r in res], np.int64).reshape(w.n_streams, w.per_stream)
        t0 = np.cumsum(m, 1) - m
        T = int(m.sum(1).max())
        places = np.zeros(NP, R.PLACE_DTYPE)
        places["row"] = np.repeat(np.arange(w.n_streams), w.per_stream)
        places["keep"] = R.ALL
        places["t0"] = t0.reshape(-1)
        shifted = places.copy()
        first = np.arange(w.n_streams) * w.per_stream
        shifted["skip"][first] = 5
        shifted["t0"] = np.maximum(places["t0"].astype(np.int64) - 5, 0)
        slots.append(dict(bt=bt, pw=pw, rows=R.Rows(dec, NP, fmt), places=places, shifted=shifted,
                          out=torch.empty(bt.out_elems, dtype=dt, device="cuda"), copy=torch.empty(bt.out_elems, dtype=dt, device="cuda"),
                          tensor=torch.zeros((w.n_streams, ch, T), dtype=dt, device="cuda")))
        b += 1
    torch.cuda.synchronize()
    return w, slots


def timed(fn, nb, steps):
    for k in range(2 * nb):
        fn(k)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t = time.perf_counter()
    e0.record()
    for k in range(steps):
        fn(k)
    e1.record()
    enq = (time.perf_counter() - t) * 1e6 / steps
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / steps, enq


def variants(slots):
    nb = len(slots)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def a(k):
        s = slots[k % nb]
        s["bt"].synth(C.c_void_p(s["out"].data_ptr()), s["out"].numel(), st)

    def b(k):
        s = slots[k % nb]
        s["rows"].synth(s["bt"], s["places"], s["tensor"])

    def b5(k):
        s = slots[k % nb]
        s["rows"].synth(s["bt"], s["shifted"], s["tensor"])

    def c(k):
        s = slots[k % nb]
        s["copy"].copy_(s["out"])

    return {"synth": a, "rows": b, "rows_skip5": b5, "copy": c}


def bench(packets, fmt, steps, rounds):
    w, slots = build(packets, fmt)
    nb, v = len(slots), variants(slots)
    es = 4 if fmt.startswith("f32") else 2
    elems = slots[0]["bt"].out_elems
    acc = {k: [] for k in v}
    for _ in range(rounds):
        for name, fn in v.items():
            acc[name].append(timed(fn, nb, steps))
    us = {k: float(np.median([x[0] for x in r])) for k, r in acc.items()}
    line = {"packets_per_step": packets, "format": fmt, "steps": steps, "rounds": rounds, "batches_rotated": nb,
            "pcm_bytes_per_step": elems * es, "pieces_per_step": slots[0]["rows"].last_segments,
            "us_per_step": {k: round(x, 2) for k, x in us.items()},
            "us_per_step_all_rounds": {k: [round(x[0], 2) for x in r] for k, r in acc.items()},
            "host_enqueue_us_per_step": {k: round(float(np.median([x[1] for x in r])), 2) for k, r in acc.items()},
            "rows_minus_synth_us": round(us["rows"] - us["synth"], 2), "rows_skip5_minus_synth_us": round(us["rows_skip5"] - us["synth"], 2),
            "rows_minus_synth_over_copy": round((us["rows"] - us["synth"]) / us["copy"], 3),
            "copy_rate_GBps_of_the_yardstick": round(2 * elems * es / us["copy"] / 1e3, 1),
            "kernels": slots[0]["bt"].last_kernels}
    for s in slots:
        s["rows"].close()
        s["bt"].close()
    return line


def kernel_only(packets, fmt, steps, name):
    """(b) or (b5) alone, for a rocprofv3 --kernel-trace --stats run: k_rows<2> is the i16 kernel, k_rows<4> the f32 one"""
    w, slots = build(packets, fmt)
    timed(variants(slots)[name], len(slots), steps)
    for s in slots:
        s["rows"].close()
        s["bt"].close()


def e2e(batches):
    from lewton_amd import e2e as E
    setup = sg.stereo_setup(44100, 8, 11)
    idp, _, stp = setup.headers()
    ident = header.read_header_ident(idp)
    st = header.read_header_setup(stp, 2, (8, 11))
    dec = audio.decoder_for(ident, st, 0)
    pool = sg.make_stream(setup, "L", 512, seed=9)
    rng = np.random.default_rng(1)
    per = 16 * batches
    streams = [[pool[int(i)] for i in rng.integers(0, len(pool), per + 1)] for _ in range(256)]
    out = {}
    for fmt in ("i16", "f32"):
        R.decode_streams(ident, st, [s[:17] for s in streams], fmt, max_packets=4096, entropy_on_device=True)   # warm
        t = time.perf_counter()
        pcm, lengths, errors = R.decode_streams(ident, st, streams, fmt, max_packets=4096, run=16, entropy_on_device=True)
        dt = time.perf_counter() - t
        assert not errors and int(lengths.min()) == per * 1024
        out["decode_streams_" + fmt] = {"packets": 256 * (per + 1), "seconds": round(dt, 4), "M_packets_per_s": round(256 * (per + 1) / dt / 1e6, 3),
                                        "pcm_shape": list(pcm.shape)}
        del pcm
        r = E.measure(dec, pool, batches, 4096, 256, samples=fmt, device_entropy=True)
        out["ring_" + fmt] = {"packets": r["packets"], "seconds": round(r["seconds"], 4), "M_packets_per_s": round(r["value"] / 1e6, 3),
                              "d2h_GBps": round(r["d2h_GBps"], 2)}
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--packets", default="4096,16384")
    ap.add_argument("--formats", default="i16,f32")
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--kernel-only", default="", help="rows or rows_skip5: run that variant alone (under rocprofv3)")
    ap.add_argument("--e2e", action="store_true")
    ap.add_argument("--e2e-batches", type=int, default=8)
    args = ap.parse_args()
    for p in [int(x) for x in args.packets.split(",")]:
        for fmt in args.formats.split(","):
            if args.kernel_only:
                kernel_only(p, fmt, args.steps, args.kernel_only)
            else:
                print(json.dumps(bench(p, fmt, args.steps, args.rounds)), flush=True)
    if args.e2e:
        print(json.dumps(e2e(args.e2e_batches)), flush=True)
