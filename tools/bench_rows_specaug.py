#!/usr/bin/env python3
"""Cost of SpecAugment's masks (lw_specaug_rows: k_specaug out of place, k_specaug_inplace in place) next to a plain copy of the
bytes the pass out of place must move and to the same masking in torch ops.

Shape: [64][1][80][3000] feature rows, every line full (64 utterances of 30 s), under the WeNet preset (two time masks of 1 .. 50
frames, two frequency masks of 1 .. 10 bins), ids 0 .. 63: out of place and in place (which writes the masked elements alone and
reads nothing), each at tiles of 2048 frames (the default) and of 1024.  The tensors are rotated over >= 0.5 GiB so that none stays in
the Infinity Cache.  Yardsticks from the same session: a flat dst.copy_(src) of the same tensor -- the pass out of place reads and
writes every element once, as the copy does: its floor -- and the masking in torch ops: the spans drawn on the host with numpy,
sent to the device, two comparisons against arange per kind, and one masked_fill_ in place, by HIP events.

Every variant runs in a process of its own under
    rocprofv3 --kernel-trace --stats -- python tools/bench_rows_specaug.py --kernel-only NAME
with nothing else traced and no counters; the kernel's own time is the k_specaug row of that run's kernel statistics, and the child
also times its calls with HIP events (the host side of a call shows in those).  Ratios are quoted like for like: kernel over
kernel, events over events.  Without --kernel-only this script starts those runs one after the other, stops at the first that
fails, and prints one JSON line per variant and a table:
    python tools/bench_rows_specaug.py [--steps 50] [--write profiles/rows_specaug_bench.txt]"""
import argparse
import json
import os
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_rows_spec import kernel_stats, timed  # noqa: E402

ROWS, LINES, FRAMES = 64, 80, 3000
# name -> (in place, tile)
PASSES = {"out_of_place": (False, 2048), "out_of_place_1024": (False, 1024), "in_place": (True, 2048), "in_place_1024": (True, 1024)}
VARIANTS = ["copy"] + list(PASSES) + ["torch"]
ROTATE_BYTES = 1 << 29
WARMUP = 10


def child(name, steps):
    import numpy as np
    import torch
    nbytes = ROWS * LINES * FRAMES * 4
    line = {"variant": name, "steps": steps, "src": [ROWS, 1, LINES, FRAMES], "bytes": 2 * nbytes}
    nb = -(-ROTATE_BYTES // nbytes)
    gen = torch.Generator(device="cuda").manual_seed(1)
    srcs = [torch.randn((ROWS, 1, LINES, FRAMES), device="cuda", generator=gen) for _ in range(nb)]
    obj = None
    if name == "copy":
        dsts = [torch.empty_like(t) for t in srcs]
        fn = lambda k: dsts[k % nb].copy_(srcs[k % nb])                                        # noqa: E731
    elif name == "torch":
        rng = np.random.default_rng(1)
        t, f = torch.arange(FRAMES, device="cuda"), torch.arange(LINES, device="cuda")

        def spans(n, lo, hi):
            w = rng.integers(lo, hi + 1, (ROWS, 2))
            s = (rng.random((ROWS, 2)) * (n - w + 1)).astype(np.int64)
            return torch.from_numpy(np.stack([s, s + w])).cuda()

        def fn(k):
            ts, fs = spans(FRAMES, 1, 50), spans(LINES, 1, 10)
            tm = ((t >= ts[0][:, :, None]) & (t < ts[1][:, :, None])).any(1)
            fm = ((f >= fs[0][:, :, None]) & (f < fs[1][:, :, None])).any(1)
            return srcs[k % nb].masked_fill_(tm[:, None, None, :] | fm[:, None, :, None], 0.0)
    else:
        from lewton_amd.rows import SpecAugment
        in_place, tile = PASSES[name]
        obj = SpecAugment.wenet(seed=2024)
        obj.set_tile_frames(tile)
        n, ids = [FRAMES] * ROWS, list(range(ROWS))
        line["bytes"] = 2 * nbytes if not in_place else None                                   # in place: what is written depends on the draw
        dsts = srcs if in_place else [torch.empty_like(t) for t in srcs]
        fn = lambda k: obj.run(srcs[k % nb], n, ids=ids, out=None if in_place else dsts[k % nb])   # noqa: E731
    line["buffers_rotated"] = nb
    line["events_us"] = round(timed(fn, steps, WARMUP), 2)
    if obj is not None:
        line["launches"], line["tile_frames"] = obj.last_launches(), obj.tile_frames
        if PASSES[name][0]:
            torch.cuda.synchronize()
            line["masked_share"] = round(float((srcs[0] == 0).float().mean()), 4)
        obj.close()
    print("RESULT " + json.dumps(line), flush=True)


def parent(steps, write):
    prof = shutil.which("rocprofv3")
    lines = []
    for name in VARIANTS:
        tmp = tempfile.mkdtemp(prefix="rows_specaug_")
        cmd = [sys.executable, os.path.abspath(__file__), "--kernel-only", name, "--steps", str(steps)]
        if prof:
            cmd = [prof, "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp, "-o", name, "--"] + cmd
        r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=240)
        res = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
        if r.returncode or not res:
            sys.stderr.write(r.stdout[-2000:] + r.stderr[-2000:])
            raise SystemExit("variant %s failed (%d): nothing more is started" % (name, r.returncode))
        line = json.loads(res[-1][7:])
        stats = kernel_stats(tmp)
        shutil.rmtree(tmp, ignore_errors=True)
        mine = {k.split("(")[0][:40]: v[1] / 1e3 for k, v in stats.items() if "k_specaug" in k}
        if mine:
            line["kernel_us"] = round(sum(mine.values()), 2)
            line["kernels"] = {k: round(v, 2) for k, v in mine.items()}
            if line["bytes"]:
                line["kernel_TB_per_s"] = round(line["bytes"] / (line["kernel_us"] * 1e-6) / 1e12, 3)
        elif stats:  # the yardstick's own kernels: those that ran in every call, and not once per rotated buffer
            per_call = {k: v for k, v in stats.items() if v[0] % (steps + WARMUP) == 0}
            if per_call:
                line["kernel_us"] = round(sum(v[0] * v[1] for v in per_call.values()) / (steps + WARMUP) / 1e3, 2)
                line["kernels"] = len(per_call)
        lines.append(line)
        print(json.dumps(line), flush=True)
    by = {l["variant"]: l for l in lines}
    cp, t = by["copy"], by["torch"]
    table = ["pass | launches | kernel (trace) | copy_ of the same tensor (trace) | pass / copy, kernels | call (events) | copy_ (events) | call / copy, events | torch ops (events) | torch ops / call, events",
             "---|---|---|---|---|---|---|---|---|---"]
    us = lambda v: "%.2f us" % v if v else "n/a"                                               # noqa: E731
    for p in PASSES:
        l = by[p]
        k, ck = l.get("kernel_us"), cp.get("kernel_us")
        table.append("%s | %d | %s | %s | %s | %.2f us | %.2f us | %.2f | %.2f us | %.2f" % (
            p, l["launches"], us(k), us(ck), "%.2f" % (k / ck) if k and ck else "n/a", l["events_us"], cp["events_us"], l["events_us"] / cp["events_us"],
            t["events_us"], t["events_us"] / l["events_us"]))
    print("\n".join(table))
    if write:
        with open(write, "w") as f:
            f.write("# tools/bench_rows_specaug.py --steps %d: one process per variant under rocprofv3 --kernel-trace --stats\n" % steps)
            f.write("\n".join(json.dumps(l) for l in lines) + "\n\n" + "\n".join(table) + "\n")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--kernel-only", default="", help="one of %s: run that variant alone (under rocprofv3)" % ", ".join(VARIANTS))
    ap.add_argument("--write", default="", help="also write the lines and the table to this file")
    args = ap.parse_args()
    if args.kernel_only:
        child(args.kernel_only, args.steps)
    else:
        parent(args.steps, args.write)
