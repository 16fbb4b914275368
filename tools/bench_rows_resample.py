#!/usr/bin/env python3
"""Cost of the row resampler (lw_resample_rows, k_resample) next to a plain copy of its input.

Shapes: rows [256][2][16384] f32 planar at 44100 -> 16000 and 48000 -> 16000, each with hann / 6 and kaiser / 16, and
[256][1][16384] at 16000 -> 44100 (hann / 6).  Source and destination tensors are rotated over >= 0.5 GiB of input so that neither
stays in the Infinity Cache.  Yardstick: dst.copy_(src) of the input tensor's bytes, HIP events, in the same session (DESIGN.md
section 3.14 (c)).

Every variant runs in a process of its own under
    rocprofv3 --kernel-trace --stats -- python tools/bench_rows_resample.py --kernel-only NAME
with nothing else traced; the kernel's own time is the k_resample row of that run's kernel statistics, and the child also times
its steps with HIP events (Resampler.run as a whole: the host side of the call shows in it).  Without --kernel-only this script
starts those runs one after the other, stops at the first that fails, and prints one JSON line per variant and a table:
    python tools/bench_rows_resample.py [--steps 200] [--write profiles/rows_resample_bench.txt]"""
import argparse
import csv
import glob
import json
import os
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HANN, KAISER = {}, {"window": "kaiser", "zeros": 16}
VARIANTS = {  # name -> (in_rate, out_rate, filter, channels)
    "441_160_hann": (44100, 16000, HANN, 2), "441_160_kaiser": (44100, 16000, KAISER, 2),
    "3_1_hann": (48000, 16000, HANN, 2), "3_1_kaiser": (48000, 16000, KAISER, 2),
    "160_441_hann": (16000, 44100, HANN, 1),
}
COPIES = {"copy_stereo": 2, "copy_mono": 1}
ROWS, SAMPLES = 256, 16384
ROTATE_BYTES = 1 << 29


def timed(fn, steps, warmup=20):
    import torch
    for k in range(warmup):
        fn(k)
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for k in range(steps):
        fn(k)
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / steps


def child(name, steps):
    import torch
    ch = COPIES[name] if name in COPIES else VARIANTS[name][3]
    in_bytes = ROWS * ch * SAMPLES * 4
    nb = -(-ROTATE_BYTES // in_bytes)
    gen = torch.Generator(device="cuda").manual_seed(1)
    srcs = [torch.randn((ROWS, ch, SAMPLES), device="cuda", generator=gen) for _ in range(nb)]
    line = {"variant": name, "rows": [ROWS, ch, SAMPLES], "in_bytes": in_bytes, "buffers_rotated": nb, "steps": steps}
    if name in COPIES:
        dsts = [torch.empty_like(s) for s in srcs]
        line["events_us"] = round(timed(lambda k: dsts[k % nb].copy_(srcs[k % nb]), steps), 2)
    else:
        from lewton_amd.rows import Resampler
        in_rate, out_rate, filt, _ = VARIANTS[name]
        rs = Resampler(in_rate, out_rate, **filt)
        T = rs.out_len(SAMPLES)
        dsts = [torch.zeros((ROWS, ch, T), device="cuda") for _ in range(nb)]
        lengths = [SAMPLES] * ROWS
        line["events_us"] = round(timed(lambda k: rs.run(srcs[k % nb], lengths, out=dsts[k % nb]), steps), 2)
        line.update(out_bytes=ROWS * ch * T * 4, taps_per_phase=rs.taps_per_phase, phases=rs.new, route=rs.last_route,
                    tap_multiplies=ROWS * ch * T * rs.taps_per_phase)
        rs.close()
    print("RESULT " + json.dumps(line), flush=True)


def kernel_stats(directory):
    """{kernel name: (calls, average ns)} from the run's *kernel_stats.csv"""
    out = {}
    for path in glob.glob(os.path.join(directory, "**", "*kernel_stats.csv"), recursive=True):
        with open(path, newline="") as f:
            for row in csv.DictReader(f):
                try:
                    out[row["Name"]] = (int(row["Calls"]), float(row["AverageNs"]))
                except (KeyError, ValueError):
                    continue
    return out


def parent(steps, write):
    prof = shutil.which("rocprofv3")
    lines = []
    for name in list(COPIES) + list(VARIANTS):
        tmp = tempfile.mkdtemp(prefix="rows_resample_")
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
        mine = {k: v for k, v in stats.items() if "k_resample" in k}
        if mine:
            (kname, (calls, avg)), = list(mine.items())[:1]
            line.update(kernel=kname.split("(")[0], kernel_calls=calls, kernel_us=round(avg / 1e3, 2))
        elif name in COPIES and stats:
            line["kernels_seen"] = {k.split("(")[0][:60]: round(v[1] / 1e3, 2) for k, v in stats.items()}
        lines.append(line)
        print(json.dumps(line), flush=True)
    yard = {l["rows"][1]: l["events_us"] for l in lines if l["variant"] in COPIES}
    table = ["variant | K x phases | route | k_resample (rocprofv3) | Resampler.run (events) | copy_(src) (events) | kernel / copy | tap multiplies / s",
             "---|---|---|---|---|---|---|---"]
    for l in lines:
        if l["variant"] in COPIES:
            continue
        c, k = yard[l["rows"][1]], l.get("kernel_us")
        table.append("%s | %d x %d | %d | %s us | %.2f us | %.2f us | %s | %s" % (
            l["variant"], l["taps_per_phase"], l["phases"], l["route"], "%.2f" % k if k else "n/a", l["events_us"], c,
            "%.2f" % (k / c) if k else "n/a", "%.2f T" % (l["tap_multiplies"] / (k * 1e-6) / 1e12) if k else "n/a"))
    print("\n".join(table))
    if write:
        with open(write, "w") as f:
            f.write("# tools/bench_rows_resample.py --steps %d: one process per variant under rocprofv3 --kernel-trace --stats\n" % steps)
            f.write("\n".join(json.dumps(l) for l in lines) + "\n\n" + "\n".join(table) + "\n")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--kernel-only", default="", help="one of %s: run that variant alone (under rocprofv3)" % ", ".join(list(COPIES) + list(VARIANTS)))
    ap.add_argument("--write", default="", help="also write the lines and the table to this file")
    args = ap.parse_args()
    if args.kernel_only:
        child(args.kernel_only, args.steps)
    else:
        parent(args.steps, args.write)
