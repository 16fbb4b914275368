#!/usr/bin/env python3
"""Cost of the segment pass (lw_segment_rows: k_segment_count + k_segment) and of the cut (lw_cut_rows: k_cut) next to a plain copy of
the bytes each must move, and the segments next to the same result from torch ops plus a host loop.

Segments: [64][1][3000] masks of bursts (64 utterances of 30 s at a 10 ms shift) under (pad_onset, pad_offset, min_off, min_on) =
(10, 30, 50, 25), spans and counts alone and with the smoothed mask.  Yardsticks from the same session: a flat dst.copy_(src) of
HALF the bytes the pass must move (the mask in, and the smoothed mask out where it is wanted; a copy reads and writes each of its
bytes once, so it moves the same total), and the same spans from torch ops -- max_pool1d for the pad, a closing and an opening for
the fill and the drop, a diff and nonzero for the edges -- with the host loop that turns the edges into per-row lists, which the
child holds against the pass's own result before it times anything.
Cut: [64][1][480000] rows (64 utterances of 30 s at 16 kHz) cut into 256 segments of 1 s .. 15 s at odd starts, float32 and int16,
next to a flat copy_ of the bytes written.  The sources are rotated over >= 0.5 GiB so that none stays in the Infinity Cache.

Every variant runs in a process of its own under
    rocprofv3 --kernel-trace --stats -- python tools/bench_rows_segment.py --kernel-only NAME
with nothing else traced and no counters; the kernels' own time is the sum of the k_segment* or k_cut rows of that run's kernel
statistics, and the child also times its calls with HIP events.  Ratios are quoted like for like: kernel over kernel, events over
events.  Without --kernel-only this script starts those runs one after the other, each under a time limit of its own, stops at
the first that fails, and prints one JSON line per variant and a table:
    python tools/bench_rows_segment.py [--steps 50] [--write profiles/rows_segment_bench.txt]"""
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

ROWS, FRAMES, SAMPLES, JOBS = 64, 3000, 480000, 256
PARAMS = (10, 30, 50, 25)
SEG_CAP = 64
VARIANTS = ["copy_segment", "segment", "torch_segment", "copy_smooth", "segment_smooth", "copy_cut_f32", "cut_f32", "copy_cut_i16", "cut_i16"]
COPY_OF = {"segment": "copy_segment", "segment_smooth": "copy_smooth", "cut_f32": "copy_cut_f32", "cut_i16": "copy_cut_i16"}
ROTATE_BYTES = 1 << 29
WARMUP = 10
STEP_TIMEOUT = 240


def masks(nb):
    """nb masks uint8 [64][1][3000] of bursts: runs around 40 frames, gaps around 15 with one in five a pause around 150"""
    import numpy as np
    import torch
    rng = np.random.default_rng(1)
    out = []
    for _ in range(nb):
        m = np.zeros((ROWS, 1, FRAMES), np.uint8)
        for r in range(ROWS):
            t, on = 0, False
            while t < FRAMES:
                k = int(rng.geometric(1 / 40.0)) if on else int(rng.geometric(1 / (150.0 if rng.random() < 0.2 else 15.0)))
                m[r, 0, t:t + k] = on
                t, on = t + k, not on
        out.append(torch.from_numpy(m).to("cuda"))
    return out


def cut_jobs():
    """256 jobs (row, start, end): odd starts in the first 200 000 samples, 16 000 .. 240 000 samples each"""
    jobs = []
    for i in range(JOBS):
        start = 2 * ((i * 7919) % 100000) + 1
        jobs.append((i % ROWS, start, start + 16000 + (i * 104729) % 224000 + i % 3))
    return jobs


def torch_segments(m, pad_onset, pad_offset, min_off, min_on):
    """the spans of a mask [rows][1][T] by torch ops and a host loop: {row: [(a, b), ...]}"""
    import torch
    import torch.nn.functional as F
    x = (m != 0).float()
    P = F.max_pool1d(F.pad(x, (pad_offset, pad_onset)), pad_onset + pad_offset + 1, 1)
    g = max(min_off - 1, 0)
    D = F.max_pool1d(F.pad(P, (g, 0)), g + 1, 1)                                         # any set frame in [t - g, t]
    E = -F.max_pool1d(F.pad(-D, (0, g), value=-1.0), g + 1, 1)                           # ... for every frame of [t, t + g]
    between = (torch.cummax(P, 2)[0] > 0) & (torch.cummax(P.flip(2), 2)[0].flip(2) > 0)
    C = torch.maximum(P, E * between)
    k = max(min_on, 1)
    R = -F.max_pool1d(F.pad(-C, (0, k - 1), value=0.0), k, 1)                            # a run of k frames starts at t
    O = F.max_pool1d(F.pad(R, (k - 1, 0)), k, 1)
    d = torch.diff(F.pad(O, (1, 1)), dim=2)
    starts, ends = torch.nonzero(d[:, 0] > 0).cpu().tolist(), torch.nonzero(d[:, 0] < 0).cpu().tolist()     # the synchronisation
    out = {}
    for (r, a), (_, b) in zip(starts, ends):
        out.setdefault(r, []).append((a, b))
    return out


def child(name, steps):
    import numpy as np
    import torch
    line = {"variant": name, "steps": steps}
    obj = None
    if name in ("copy_segment", "copy_smooth", "segment", "segment_smooth", "torch_segment"):
        smooth = name.endswith("smooth")
        moved = ROWS * FRAMES * (2 if smooth else 1)
        line["bytes"], line["src"] = moved, [ROWS, 1, FRAMES]
        nb = -(-ROTATE_BYTES // (ROWS * FRAMES))
        if name.startswith("copy_"):
            srcs = [torch.zeros(max(moved // 2, 1), dtype=torch.uint8, device="cuda") for _ in range(nb)]
            dsts = [torch.empty_like(t) for t in srcs]
            fn = lambda k: dsts[k % nb].copy_(srcs[k % nb])                                    # noqa: E731
        else:
            from lewton_amd.rows import Segments
            nb = min(nb, 256)                                                                # (the masks are made on the host)
            srcs = masks(nb)
            n = [FRAMES] * ROWS
            obj = Segments(*PARAMS)
            spans, counts = obj.run(srcs[0], n, seg_capacity=SEG_CAP)
            k0 = counts.cpu().numpy()[:, 0]
            want = {r: [tuple(s) for s in spans[r, 0, :k0[r]].cpu().tolist()] for r in range(ROWS) if k0[r]}
            assert torch_segments(srcs[0], *PARAMS) == want and int(k0.max()) <= SEG_CAP, "the torch restatement differs from the pass"
            line["segments"] = int(k0.sum())
            if name == "torch_segment":
                fn = lambda k: torch_segments(srcs[k % nb], *PARAMS)                           # noqa: E731
            else:
                outs = [torch.empty((ROWS, 1, FRAMES), dtype=torch.uint8, device="cuda") for _ in range(nb)] if smooth else None
                fn = lambda k: obj.run(srcs[k % nb], n, seg_capacity=SEG_CAP, out_mask=outs[k % nb] if smooth else None)   # noqa: E731
    else:
        elem, dtype = (4, torch.float32) if name.endswith("f32") else (2, torch.int16)
        jobs = cut_jobs()
        written = sum(b - a for _, a, b in jobs) * elem
        line["bytes"], line["src"], line["jobs"] = 2 * written, [ROWS, 1, SAMPLES], len(jobs)
        if name.startswith("copy_"):
            nb = -(-ROTATE_BYTES // written)
            srcs = [torch.zeros(written, dtype=torch.uint8, device="cuda") for _ in range(nb)]
            dst = torch.empty_like(srcs[0])
            fn = lambda k: dst.copy_(srcs[k % nb])                                            # noqa: E731
        else:
            from lewton_amd.rows import CutRows
            nb = -(-ROTATE_BYTES // (ROWS * SAMPLES * elem))
            srcs = [torch.zeros((ROWS, 1, SAMPLES), dtype=dtype, device="cuda") for _ in range(nb)]
            cap = -(-max(b - a for _, a, b in jobs) // 8) * 8
            dst = torch.empty((len(jobs), 1, cap), dtype=dtype, device="cuda")
            jb = np.asarray(jobs, np.uint64)
            obj = CutRows()
            fn = lambda k: obj.run(srcs[k % nb], [SAMPLES] * ROWS, jb, out=dst, samples="f32" if elem == 4 else "i16")   # noqa: E731
    line["buffers_rotated"] = nb
    line["events_us"] = round(timed(fn, steps, WARMUP), 2)
    if obj is not None:
        line["launches"] = obj.last_launches()
        obj.close()
    print("RESULT " + json.dumps(line), flush=True)


def parent(steps, write):
    prof = shutil.which("rocprofv3")
    lines = []
    for name in VARIANTS:
        tmp = tempfile.mkdtemp(prefix="rows_segment_")
        cmd = [sys.executable, os.path.abspath(__file__), "--kernel-only", name, "--steps", str(steps)]
        if prof:
            cmd = [prof, "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp, "-o", name, "--"] + cmd
        cmd = ["timeout", "-k", "10", str(STEP_TIMEOUT)] + cmd
        r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True)
        res = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
        if r.returncode or not res:
            sys.stderr.write(r.stdout[-2000:] + r.stderr[-2000:])
            raise SystemExit("variant %s failed (%d): nothing more is started" % (name, r.returncode))
        line = json.loads(res[-1][7:])
        stats = kernel_stats(tmp)
        shutil.rmtree(tmp, ignore_errors=True)
        mine = {k.split("(")[0][:40]: v[1] / 1e3 for k, v in stats.items() if "k_segment" in k or "k_cut" in k}
        if mine and not name.startswith(("copy_", "torch_")):
            line["kernel_us"] = round(sum(mine.values()), 2)
            line["kernels"] = {k: round(v, 2) for k, v in mine.items()}
            line["kernel_TB_per_s"] = round(line["bytes"] / (line["kernel_us"] * 1e-6) / 1e12, 3)
        elif stats and name.startswith("copy_"):  # the yardstick's own kernels: those that ran in every call
            per_call = {k: v for k, v in stats.items() if v[0] % (steps + WARMUP) == 0}
            if per_call:
                line["kernel_us"] = round(sum(v[0] * v[1] for v in per_call.values()) / (steps + WARMUP) / 1e3, 2)
                line["kernels"] = len(per_call)
        lines.append(line)
        print(json.dumps(line), flush=True)
    by = {l["variant"]: l for l in lines}
    table = ["pass | launches | kernels (trace) | copy_ of the same bytes (trace) | pass / copy, kernels | call (events) | copy_ (events) | call / copy, events",
             "---|---|---|---|---|---|---|---"]
    us = lambda v: "%.2f us" % v if v else "n/a"                                               # noqa: E731
    for p, c in COPY_OF.items():
        l, cp = by[p], by[c]
        k, ck = l.get("kernel_us"), cp.get("kernel_us")
        table.append("%s | %d | %s | %s | %s | %.2f us | %.2f us | %.2f" % (
            p, l["launches"], us(k), us(ck), "%.2f" % (k / ck) if k and ck else "n/a", l["events_us"], cp["events_us"], l["events_us"] / cp["events_us"]))
    t, s = by["torch_segment"], by["segment"]
    table.append("")
    table.append("torch ops and a host loop, per call with its synchronisation (events): %.2f us = %.2f x the pass's call (%.2f us, no synchronisation)" % (
        t["events_us"], t["events_us"] / s["events_us"], s["events_us"]))
    print("\n".join(table))
    if write:
        with open(write, "w") as f:
            f.write("# tools/bench_rows_segment.py --steps %d: one process per variant under rocprofv3 --kernel-trace --stats\n" % steps)
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
