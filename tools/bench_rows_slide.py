#!/usr/bin/env python3
"""Cost of the sliding-window normalisation (lw_slide_rows: k_slide) and of frame selection (lw_select_rows: k_select_count, k_select)
next to a plain copy of the bytes each pass must move and to torch's own chain for the same result.

Shape: [64][1][80][3000] feature rows, every line full (64 utterances of 30 s).  k_slide at (300, 100, center) and at (600, 100, not
centred), each with and without norm_vars; k_select with half the frames kept at random.  Source and destination tensors are
rotated over >= 0.5 GiB each so that neither stays in the Infinity Cache.  Yardsticks from the same session: a flat dst.copy_(src)
of HALF the bytes the pass reads and writes (a copy reads and writes each of its bytes once, so it moves the same total: the pass's
floor), and torch's chain -- float64 cumulative sums of the lines and of their squares, gathered at the windows' ends, for the
window; boolean indexing of the frame-major view for the selection -- both by HIP events.

Every variant runs in a process of its own under
    rocprofv3 --kernel-trace --stats -- python tools/bench_rows_slide.py --kernel-only NAME
with nothing else traced and no counters; the kernel's own time is the sum of the k_slide / k_select rows of that run's kernel
statistics, and the child also times its calls with HIP events (the host side of a call and the gaps between launches show in
those).  Ratios are quoted like for like: kernel over kernel, events over events.  Without --kernel-only this script starts those
runs one after the other, stops at the first that fails, and prints one JSON line per variant and a table:
    python tools/bench_rows_slide.py [--steps 50] [--write profiles/rows_slide_bench.txt]"""
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
# name -> (cmn_window, min_cmn_window, center, norm_vars)
SLIDES = {"300c": (300, 100, True, False), "300c_nv": (300, 100, True, True), "600": (600, 100, False, False), "600_nv": (600, 100, False, True)}
PASSES = ["slide_" + s for s in SLIDES] + ["select_half"]
VARIANTS = ["copy"] + [k + p for p in PASSES for k in ("", "torch_")]
ROTATE_BYTES = 1 << 29
WARMUP = 10


def child(name, steps):
    import numpy as np
    import torch
    bytes_line = ROWS * LINES * FRAMES * 4
    line = {"variant": name, "steps": steps, "src": [ROWS, 1, LINES, FRAMES], "bytes": 2 * bytes_line}
    gen = torch.Generator(device="cuda").manual_seed(1)
    nb = -(-ROTATE_BYTES // bytes_line)
    srcs = [torch.randn((ROWS, 1, LINES, FRAMES), device="cuda", generator=gen).mul_(3.0).sub_(12.0) for _ in range(nb)]
    obj = None
    n = [FRAMES] * ROWS
    if name == "copy":
        dsts = [torch.empty_like(t) for t in srcs]
        fn = lambda k: dsts[k % nb].copy_(srcs[k % nb])                                        # noqa: E731
    elif name.endswith("select_half"):
        mask = torch.rand((ROWS, 1, FRAMES), device="cuda", generator=gen) < 0.5
        line["bytes"] += ROWS * FRAMES
        if name.startswith("torch_"):
            fn = lambda k: srcs[k % nb].permute(0, 1, 3, 2)[mask]                              # noqa: E731  ([kept frames][80], the counts apart)
        else:
            from lewton_amd.rows import SelectFrames
            obj = SelectFrames()
            dsts = [torch.empty_like(t) for t in srcs]
            fn = lambda k: obj.run(srcs[k % nb], n, mask, out=dsts[k % nb])                   # noqa: E731
    else:
        W, mn, center, nv = SLIDES[name.split("slide_")[1]]
        from lewton_amd.rows import SlidingCMVN
        obj = SlidingCMVN(W, mn, center, nv)
        if name.startswith("torch_"):
            wins = [obj.window(t, FRAMES) for t in range(FRAMES)]
            s = torch.tensor([w[0] for w in wins], device="cuda")
            e = torch.tensor([w[1] for w in wins], device="cuda")
            cnt = (e - s).double()
            obj.close()
            obj = None

            def fn(k):
                d = srcs[k % nb].double()
                c1 = torch.nn.functional.pad(torch.cumsum(d, dim=3), (1, 0))
                mu = (c1[..., e] - c1[..., s]) / cnt
                z = d - mu
                if nv:
                    c2 = torch.nn.functional.pad(torch.cumsum(d * d, dim=3), (1, 0))
                    z = z / torch.sqrt(torch.clamp((c2[..., e] - c2[..., s]) / cnt - mu * mu, min=1e-10))
                return z.float()
        else:
            dsts = [torch.empty_like(t) for t in srcs]
            fn = lambda k: obj.run(srcs[k % nb], n, out=dsts[k % nb])                         # noqa: E731
    line["buffers_rotated"] = nb
    line["events_us"] = round(timed(fn, steps, WARMUP), 2)
    if obj is not None:
        line["launches"], line["tile_frames"] = obj.last_launches(), obj.tile_frames
        obj.close()
    print("RESULT " + json.dumps(line), flush=True)


def parent(steps, write):
    prof = shutil.which("rocprofv3")
    lines = []
    for name in VARIANTS:
        tmp = tempfile.mkdtemp(prefix="rows_slide_")
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
        mine = {k.split("(")[0][:40]: v[1] / 1e3 for k, v in stats.items() if "k_slide" in k or "k_select" in k}
        if mine:
            line["kernel_us"] = round(sum(mine.values()), 2)
            line["kernels"] = {k: round(v, 2) for k, v in mine.items()}
            line["kernel_TB_per_s"] = round(line["bytes"] / (line["kernel_us"] * 1e-6) / 1e12, 3)
        elif stats and (name == "copy" or name.startswith("torch_")):  # the yardstick's own kernels: those that ran in every call
            per_call = {k: v for k, v in stats.items() if v[0] >= steps}
            if per_call:
                line["kernel_us"] = round(sum(v[0] * v[1] for v in per_call.values()) / (steps + WARMUP) / 1e3, 2)
                line["kernels"] = len(per_call)
        lines.append(line)
        print(json.dumps(line), flush=True)
    by = {l["variant"]: l for l in lines}
    cp = by["copy"]
    table = ["pass | kernels (trace) | copy_ of the same bytes (trace) | pass / copy, kernels | call (events) | copy_ (events) | call / copy, events | torch's chain (events) | torch's chain / call, events",
             "---|---|---|---|---|---|---|---|---"]
    us = lambda v: "%.2f us" % v if v else "n/a"                                               # noqa: E731
    for p in PASSES:
        l, t = by[p], by["torch_" + p]
        k, ck = l.get("kernel_us"), cp.get("kernel_us")
        table.append("%s | %s | %s | %s | %.2f us | %.2f us | %.2f | %.2f us | %.2f" % (
            p, us(k), us(ck), "%.2f" % (k / ck) if k and ck else "n/a", l["events_us"], cp["events_us"], l["events_us"] / cp["events_us"],
            t["events_us"], t["events_us"] / l["events_us"]))
    print("\n".join(table))
    if write:
        with open(write, "w") as f:
            f.write("# tools/bench_rows_slide.py --steps %d: one process per variant under rocprofv3 --kernel-trace --stats\n" % steps)
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
