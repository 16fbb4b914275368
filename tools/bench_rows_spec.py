#!/usr/bin/env python3
"""Cost of the spectral frames of rows (lw_spec_rows, k_spec) next to a plain copy of its input.

Shape: rows [256][1][16384] f32 at 16 kHz, 26 368 frames.  Variants: (n_fft 400, hop 160, 80 mel bands), (400, 160, power
spectrum only) and (512, 160, 80 mel bands), each on route 0 (the matrix cores) and on route 1 (per-lane fmaf chains).  Source and
destination tensors are rotated over >= 0.5 GiB of input so that neither stays in the Infinity Cache.  Yardstick: dst.copy_(src) of
the input tensor's bytes, HIP events, in the same session.  Where the installed torch can run it, torch.stft + matmul on the same
shape is timed too: a comparison, not a target (its FFT has another summation order and another cost).

Every variant runs in a process of its own under
    rocprofv3 --kernel-trace --stats -- python tools/bench_rows_spec.py --kernel-only NAME
with nothing else traced and no counters; the kernel's own time is the k_spec row of that run's kernel statistics, and the child
also times its steps with HIP events (Spectrogram.run as a whole: the host side of the call shows in it).  Without --kernel-only
this script starts those runs one after the other, stops at the first that fails, and prints one JSON line per variant and a table:
    python tools/bench_rows_spec.py [--steps 100] [--write profiles/rows_spec_bench.txt]
FLOP are counted as the contract's: 2 * win_length * 2 B per frame for the DFT fold, 3 B for P, 2 * n_mels * B for the mel fold;
the fraction is of the 157 TFLOP/s f32 matrix peak."""
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

SHAPES = {"400_160_mel80": (400, 160, 80), "400_160_power": (400, 160, 0), "512_160_mel80": (512, 160, 80)}   # n_fft, hop, n_mels
VARIANTS = {"%s_route%d" % (k, r): v + (r,) for k, v in SHAPES.items() for r in (0, 1)}
OTHERS = ["copy", "torch_stft_400_160_mel80"]
ROWS, SAMPLES, RATE = 256, 16384, 16000
ROTATE_BYTES = 1 << 29
F32_MATRIX_PEAK = 157e12


def timed(fn, steps, warmup=10):
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
    in_bytes = ROWS * SAMPLES * 4
    nb = -(-ROTATE_BYTES // in_bytes)
    gen = torch.Generator(device="cuda").manual_seed(1)
    srcs = [torch.randn((ROWS, 1, SAMPLES), device="cuda", generator=gen) for _ in range(nb)]
    line = {"variant": name, "rows": [ROWS, 1, SAMPLES], "in_bytes": in_bytes, "buffers_rotated": nb, "steps": steps}
    if name == "copy":
        dsts = [torch.empty_like(s) for s in srcs]
        line["events_us"] = round(timed(lambda k: dsts[k % nb].copy_(srcs[k % nb]), steps), 2)
    elif name.startswith("torch_stft"):
        from lewton_amd.rows import mel_filterbank
        fb = torch.from_numpy(mel_filterbank(RATE, 400, 80)).cuda()
        win = torch.hann_window(400, periodic=True, device="cuda")

        def step(k):
            s = torch.stft(srcs[k % nb][:, 0], 400, hop_length=160, window=win, center=True, pad_mode="constant", return_complex=True)
            return torch.matmul(fb, s.real * s.real + s.imag * s.imag)
        try:
            line["events_us"] = round(timed(step, steps), 2)
        except Exception as e:  # an installed torch without this path: recorded, not fatal
            line["unavailable"] = "%s: %s" % (type(e).__name__, str(e)[:200])
    else:
        from lewton_amd.rows import Spectrogram, mel_filterbank
        n_fft, hop, n_mels, route = VARIANTS[name]
        sp = Spectrogram(n_fft, hop, mel=mel_filterbank(RATE, n_fft, n_mels) if n_mels else None)
        sp.set_route(route)
        T = sp.frames(SAMPLES)
        dsts = [torch.zeros((ROWS, 1, sp.features, T), device="cuda") for _ in range(nb)]
        lengths = [SAMPLES] * ROWS
        line["events_us"] = round(timed(lambda k: sp.run(srcs[k % nb], lengths, out=dsts[k % nb]), steps), 2)
        B = sp.bins
        line.update(out_bytes=ROWS * sp.features * T * 4, frames=ROWS * T, route=sp.last_route(),
                    flop=ROWS * T * (2 * sp.win_length * 2 * B + 3 * B + 2 * n_mels * B))
        sp.close()
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
    for name in OTHERS + list(VARIANTS):
        tmp = tempfile.mkdtemp(prefix="rows_spec_")
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
        mine = {k: v for k, v in stats.items() if "k_spec" in k}
        if mine:
            (kname, (calls, avg)), = list(mine.items())[:1]
            line.update(kernel=kname.split("(")[0], kernel_calls=calls, kernel_us=round(avg / 1e3, 2))
        elif stats:
            line["kernels_seen"] = {k.split("(")[0][:60]: round(v[1] / 1e3, 2) for k, v in stats.items()}
        lines.append(line)
        print(json.dumps(line), flush=True)
    by = {l["variant"]: l for l in lines}
    copy = by["copy"]["events_us"]
    table = ["variant | route | k_spec (rocprofv3) | Spectrogram.run (events) | copy_(src) (events) | kernel / copy | FLOP/s | of the f32 matrix peak | route 0 / route 1",
             "---|---|---|---|---|---|---|---|---"]
    for l in lines:
        if l["variant"] not in VARIANTS:
            continue
        k = l.get("kernel_us")
        other = by.get(l["variant"][:-1] + "1", {}).get("kernel_us") if l["route"] == 0 else None
        table.append("%s | %d | %s us | %.2f us | %.2f us | %s | %s | %s | %s" % (
            l["variant"], l["route"], "%.2f" % k if k else "n/a", l["events_us"], copy, "%.2f" % (k / copy) if k else "n/a",
            "%.1f T" % (l["flop"] / (k * 1e-6) / 1e12) if k else "n/a", "%.1f %%" % (100 * l["flop"] / (k * 1e-6) / F32_MATRIX_PEAK) if k else "n/a",
            "%.2f" % (k / other) if k and other else ""))
    t = by["torch_stft_400_160_mel80"]
    table.append("torch.stft + matmul (400, 160, 80 mel bands), events: %s" % ("%.2f us" % t["events_us"] if "events_us" in t else t.get("unavailable")))
    print("\n".join(table))
    if write:
        with open(write, "w") as f:
            f.write("# tools/bench_rows_spec.py --steps %d: one process per variant under rocprofv3 --kernel-trace --stats\n" % steps)
            f.write("\n".join(json.dumps(l) for l in lines) + "\n\n" + "\n".join(table) + "\n")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--kernel-only", default="", help="one of %s: run that variant alone (under rocprofv3)" % ", ".join(OTHERS + list(VARIANTS)))
    ap.add_argument("--write", default="", help="also write the lines and the table to this file")
    args = ap.parse_args()
    if args.kernel_only:
        child(args.kernel_only, args.steps)
    else:
        parent(args.steps, args.write)
