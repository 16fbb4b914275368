#!/usr/bin/env python3
"""Cost of the channel matrix in the row assembler (lw_rows_synth_mix, k_rows_mix) next to k_rows on the same batches.

Shape and rotation: tools/bench_rows.py (256 coupled stereo streams of long packets, 1024 samples per channel and packet, batches
rotated over >= 0.5 GiB so that neither the staging buffer nor the rows stay in the Infinity Cache).  Variants, per format:
  rows      lw_rows_synth: k_rows, the yardstick (rows [256][2][T])
  mono      lw_rows_synth_mix with [[0.5, 0.5]]: reads the same bytes, writes half (rows [256][1][T])
  identity  lw_rows_synth_mix with [[1, 0], [0, 1]]: the same bytes as k_rows through the mix kernel
The kernel's own time comes from a run of its own per variant,
    rocprofv3 --kernel-trace --stats -- python tools/bench_rows_mix.py --kernel-only mono --packets 4096 --formats f32,f32_interleaved
(mono and identity run the same instantiation, k_rows_mix<ES, ITL, 2>, so they cannot share a process under --stats).  Without
--kernel-only: HIP events around --steps steps of each variant, alternated in one process; a step is lw_batch_synth plus the
assembler, and at 4096 packets the host's enqueue rate shows in it (tools/bench_rows.py says why).
    python tools/bench_rows_mix.py [--packets 4096,16384] [--formats f32,f32_interleaved] [--steps 200] [--rounds 3]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import bench_rows as BR  # noqa: E402

MATRICES = {"mono": np.array([[0.5, 0.5]], np.float32), "identity": np.array([[1, 0], [0, 1]], np.float32)}


def variants(slots, fmt):
    nb = len(slots)
    itl = fmt.endswith("interleaved")
    for s in slots:
        B, ch, T = s["tensor"].shape
        for name, m in MATRICES.items():
            shape = (B, T, len(m)) if itl else (B, len(m), T)
            s[name] = torch.zeros(shape, dtype=s["tensor"].dtype, device="cuda")
        if itl:
            s["tensor"] = s["tensor"].view(B, T, ch)

    def rows(k):
        s = slots[k % nb]
        s["rows"].synth(s["bt"], s["places"], s["tensor"])

    def mix(name):
        def fn(k):
            s = slots[k % nb]
            s["rows"].synth(s["bt"], s["places"], s[name], mix=MATRICES[name])
        return fn

    return {"rows": rows, "mono": mix("mono"), "identity": mix("identity")}


def close(slots):
    for s in slots:
        s["rows"].close()
        s["bt"].close()


def bench(packets, fmt, steps, rounds):
    w, slots = BR.build(packets, fmt)
    nb, v = len(slots), variants(slots, fmt)
    acc = {k: [] for k in v}
    pieces = {}
    for _ in range(rounds):
        for name, fn in v.items():
            acc[name].append(BR.timed(fn, nb, steps))
            pieces[name] = slots[0]["rows"].last_segments
    line = {"packets_per_step": packets, "format": fmt, "steps": steps, "rounds": rounds, "batches_rotated": nb,
            "pcm_bytes_per_step": slots[0]["bt"].out_elems * 4, "pieces_per_step": pieces,
            "us_per_step": {k: round(float(np.median([x[0] for x in r])), 2) for k, r in acc.items()},
            "us_per_step_all_rounds": {k: [round(x[0], 2) for x in r] for k, r in acc.items()},
            "host_enqueue_us_per_step": {k: round(float(np.median([x[1] for x in r])), 2) for k, r in acc.items()}}
    close(slots)
    return line


def kernel_only(packets, fmt, steps, name):
    w, slots = BR.build(packets, fmt)
    BR.timed(variants(slots, fmt)[name], len(slots), steps)
    close(slots)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--packets", default="4096,16384")
    ap.add_argument("--formats", default="f32,f32_interleaved")
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--kernel-only", default="", help="rows, mono or identity: run that variant alone (under rocprofv3)")
    args = ap.parse_args()
    for p in [int(x) for x in args.packets.split(",")]:
        for fmt in args.formats.split(","):
            if args.kernel_only:
                kernel_only(p, fmt, args.steps, args.kernel_only)
            else:
                print(json.dumps(bench(p, fmt, args.steps, args.rounds)), flush=True)
