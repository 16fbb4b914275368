#!/usr/bin/env python3
"""Cost of the energy VAD (lw_vad_rows: k_vad, or k_vad_sum + k_vad_fold + k_vad_decide) next to a plain copy of the bytes the pass
must move and to the same decision in torch ops.

Shape: [64][1][81][3000] feature rows with the log energy in line 0, every line full (64 utterances of 30 s), under the SRE recipes'
(5.5, 0.5, 2, 0.12): the fused form (one launch), the split form forced on the same input (three), and energy_mean_scale = 0 (the
decide launch alone); [16][1][81][16384], the longest rows the fused form takes, through both forms; then ONE row of 360000 frames (an
hour), which takes the split form by itself.  The sources are rotated over >= 0.5 GiB so that none stays in the Infinity Cache.  Yardsticks from the same session: a flat dst.copy_(src) of HALF the bytes
the pass must move -- one line in, one byte per frame out; a copy reads and writes each of its bytes once, so it moves the same
total: the pass's floor -- and the same decision in torch ops: a mean of the line, a comparison, a conv1d of ones for the context
and a second comparison, by HIP events.

Every variant runs in a process of its own under
    rocprofv3 --kernel-trace --stats -- python tools/bench_rows_vad.py --kernel-only NAME
with nothing else traced and no counters; the kernels' own time is the sum of the k_vad* rows of that run's kernel statistics, and
the child also times its calls with HIP events (the host side of a call and the gaps between launches show in those).  Ratios are
quoted like for like: kernel over kernel, events over events.  Without --kernel-only this script starts those runs one after the
other, stops at the first that fails, and prints one JSON line per variant and a table:
    python tools/bench_rows_vad.py [--steps 50] [--write profiles/rows_vad_bench.txt]"""
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

LINES = 81
SHAPES = {"batch": (64, 3000), "edge": (16, 16384), "hour": (1, 360000)}   # rows, frames; edge: the fused form's longest rows
CFG = (5.5, 0.5, 2, 0.12)
# name -> (shape, route, energy_mean_scale)
PASSES = {"fused": ("batch", "fused", 0.5), "split": ("batch", "split", 0.5), "scale0": ("batch", "auto", 0.0),
          "edge_fused": ("edge", "fused", 0.5), "edge_split": ("edge", "split", 0.5), "hour": ("hour", "auto", 0.5)}
VARIANTS = ["copy_" + s for s in SHAPES] + list(PASSES) + ["torch_" + s for s in SHAPES]
ROTATE_BYTES = 1 << 29
WARMUP = 10


def child(name, steps):
    import torch
    shape = PASSES[name][0] if name in PASSES else name.split("_")[1]
    rows, frames = SHAPES[shape]
    moved = rows * frames * 5                                         # one f32 line in, one byte per frame out
    line = {"variant": name, "steps": steps, "src": [rows, 1, LINES, frames], "bytes": moved}
    obj = None
    if name.startswith("copy_"):
        nb = -(-ROTATE_BYTES // (moved // 2))
        srcs = [torch.zeros(moved // 2, dtype=torch.uint8, device="cuda") for _ in range(nb)]
        dsts = [torch.empty_like(t) for t in srcs]
        fn = lambda k: dsts[k % nb].copy_(srcs[k % nb])                                        # noqa: E731
    else:
        gen = torch.Generator(device="cuda").manual_seed(1)
        nb = -(-ROTATE_BYTES // (rows * LINES * frames * 4))
        srcs = [torch.randn((rows, 1, LINES, frames), device="cuda", generator=gen).mul_(3.0).add_(12.0) for _ in range(nb)]
        n = [frames] * rows
        if name.startswith("torch_"):
            thr0, scale, ctx, prop = CFG
            ones = torch.ones((1, 1, 2 * ctx + 1), device="cuda")
            t = torch.arange(frames, device="cuda")
            den = (torch.clamp(t + ctx + 1, max=frames) - torch.clamp(t - ctx, min=0)).float() * prop

            def fn(k):
                e = srcs[k % nb][:, :, 0, :]
                thr = thr0 + scale * e.mean(dim=2, keepdim=True)
                num = torch.nn.functional.conv1d((e > thr).float(), ones, padding=ctx)
                return num >= den
        else:
            from lewton_amd.rows import EnergyVad
            _, route, scale = PASSES[name]
            obj = EnergyVad(CFG[0], scale, CFG[2], CFG[3])
            obj.set_route(route)
            dsts = [torch.empty((rows, 1, frames), dtype=torch.uint8, device="cuda") for _ in range(nb)]
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
        tmp = tempfile.mkdtemp(prefix="rows_vad_")
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
        mine = {k.split("(")[0][:40]: v[1] / 1e3 for k, v in stats.items() if "k_vad" in k}
        if mine:
            line["kernel_us"] = round(sum(mine.values()), 2)
            line["kernels"] = {k: round(v, 2) for k, v in mine.items()}
            line["kernel_TB_per_s"] = round(line["bytes"] / (line["kernel_us"] * 1e-6) / 1e12, 3)
        elif stats:  # the yardstick's own kernels: those that ran in every call, and not once per rotated buffer
            per_call = {k: v for k, v in stats.items() if v[0] % (steps + WARMUP) == 0}
            if per_call:
                line["kernel_us"] = round(sum(v[0] * v[1] for v in per_call.values()) / (steps + WARMUP) / 1e3, 2)
                line["kernels"] = len(per_call)
        lines.append(line)
        print(json.dumps(line), flush=True)
    by = {l["variant"]: l for l in lines}
    table = ["pass | launches | kernels (trace) | copy_ of the same bytes (trace) | pass / copy, kernels | call (events) | copy_ (events) | call / copy, events | torch ops (events) | torch ops / call, events",
             "---|---|---|---|---|---|---|---|---|---"]
    us = lambda v: "%.2f us" % v if v else "n/a"                                               # noqa: E731
    for p, (shape, _, _) in PASSES.items():
        l, cp, t = by[p], by["copy_" + shape], by["torch_" + shape]
        k, ck = l.get("kernel_us"), cp.get("kernel_us")
        table.append("%s | %d | %s | %s | %s | %.2f us | %.2f us | %.2f | %.2f us | %.2f" % (
            p, l["launches"], us(k), us(ck), "%.2f" % (k / ck) if k and ck else "n/a", l["events_us"], cp["events_us"], l["events_us"] / cp["events_us"],
            t["events_us"], t["events_us"] / l["events_us"]))
    print("\n".join(table))
    if write:
        with open(write, "w") as f:
            f.write("# tools/bench_rows_vad.py --steps %d: one process per variant under rocprofv3 --kernel-trace --stats\n" % steps)
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
