#!/usr/bin/env python3
"""Cost of the complex spectral frames (k_spec_complex) and of the inverse (lw_istft_rows, k_istft) on what [256][1][16384] rows
at 16 kHz give: 25 ms hann windows every 10 ms in a 400- and in a 512-point transform.

Variants, each in a process of its own, per shape (400 = (400, 400, 160), 512 = (512, 400, 160)):
    spec_power    Spectrogram(n_fft, 160, 400, pad_mode="reflect"): k_spec, the power spectrum.  With --tree PATH the package is
                  imported from another checkout (the parent commit), so that the two can be timed in one session, alternating
    spec_complex  the same object with output="complex": k_spec_complex, 2 B lines in place of B
    istft         InverseSpectrogram over the [256][1][2 B][frames] tensor, lengths 16384: k_istft
    copy          a flat device copy that moves as many bytes as k_istft must (its source read once, its rows written once)
    torch_istft   torch.istft over the same values as a complex tensor; it has no bit contract and is timed by events only
Source tensors are rotated over >= 0.5 GiB so that none stays in the Infinity Cache.  Under
    rocprofv3 --kernel-trace --stats -- python tools/bench_rows_istft.py --kernel-only NAME --shape 512
the kernels' own times are the k_spec / k_istft rows of that run's kernel statistics (averages over warm-up and steps: 60 calls);
the child also times its calls with HIP events.  Without --kernel-only this script starts those runs one after the other, stops at
the first that fails, and prints one JSON line per run and a table:
    python tools/bench_rows_istft.py [--steps 50] [--parent-tree PATH] [--write profiles/rows_istft_bench.txt]"""
import argparse
import json
import os
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

ROWS, SAMPLES = 256, 16384
SHAPES = {"400": (400, 400, 160), "512": (512, 400, 160)}
ROTATE_BYTES = 1 << 29
VARIANTS = ["spec_power", "spec_complex", "istft", "copy", "torch_istft"]
WARMUP = 10


def child(name, shape, steps, tree):
    sys.path.insert(0, tree or ROOT)
    import torch
    from lewton_amd import rows as R        # (first: bench_rows_spec puts its own checkout in front of the path)
    from bench_rows_spec import timed
    n_fft, win, hop = SHAPES[shape]
    B, T = n_fft // 2 + 1, 1 + SAMPLES // hop
    gen = torch.Generator(device="cuda").manual_seed(1)
    line = {"variant": name, "shape": [n_fft, win, hop], "rows": [ROWS, 1, SAMPLES], "frames": T, "steps": steps}
    lengths = [SAMPLES] * ROWS
    if name.startswith("spec"):
        nb = -(-ROTATE_BYTES // (ROWS * SAMPLES * 4))
        srcs = [torch.randn((ROWS, 1, SAMPLES), device="cuda", generator=gen).mul_(0.1) for _ in range(nb)]
        kw = dict(output="complex") if name == "spec_complex" else {}
        sp = R.Spectrogram(n_fft, hop, win, pad_mode="reflect", **kw)
        dsts = [torch.empty((ROWS, 1, sp.features, T), device="cuda") for _ in range(2)]
        line["events_us"] = round(timed(lambda k: sp.run(srcs[k % nb], lengths, out=dsts[k & 1]), steps, WARMUP), 2)
        line["features"], line["route"], line["out_bytes"] = sp.features, sp.last_route(), ROWS * sp.features * T * 4
        sp.close()
    else:
        in_bytes, out_bytes = ROWS * 2 * B * T * 4, ROWS * SAMPLES * 4
        nb = -(-ROTATE_BYTES // in_bytes)
        line["in_bytes"], line["out_bytes"] = in_bytes, out_bytes
        if name == "copy":
            n = (in_bytes + out_bytes) // 8                                  # floats: read n, write n
            srcs = [torch.randn(n, device="cuda", generator=gen) for _ in range(-(-ROTATE_BYTES // (4 * n)))]
            dsts = [torch.empty(n, device="cuda") for _ in range(2)]
            line["events_us"] = round(timed(lambda k: dsts[k & 1].copy_(srcs[k % len(srcs)]), steps, WARMUP), 2)
        else:
            specs = [torch.randn((ROWS, 1, 2 * B, T), device="cuda", generator=gen).mul_(0.1) for _ in range(nb)]
            frames = [T] * ROWS
            if name == "istft":
                inv = R.InverseSpectrogram(n_fft, hop, win)
                dsts = [torch.empty((ROWS, 1, SAMPLES), device="cuda") for _ in range(2)]
                line["events_us"] = round(timed(lambda k: inv.run(specs[k % nb], frames, lengths=lengths, out=dsts[k & 1]), steps, WARMUP), 2)
                line["route"], line["tile_frames"] = inv.last_route(), inv.tile_frames
                inv.close()
            else:
                zs = [torch.complex(s[:, 0, :B].contiguous(), s[:, 0, B:].contiguous()) for s in specs]
                window = torch.hann_window(win, device="cuda")
                line["events_us"] = round(timed(lambda k: torch.istft(zs[k % nb], n_fft, hop, win, window, center=True, length=SAMPLES), steps, WARMUP), 2)
    print("RESULT " + json.dumps(line), flush=True)


def parent(steps, write, parent_tree):
    from bench_rows_spec import kernel_stats
    prof = shutil.which("rocprofv3")
    runs = []
    for shape in SHAPES:
        runs += [("spec_power", shape, ""), ("spec_complex", shape, "")]
        if parent_tree:
            runs += [("spec_power", shape, parent_tree), ("spec_power", shape, ""), ("spec_power", shape, parent_tree)]
        else:
            runs += [("spec_power", shape, "")]
        runs += [("istft", shape, ""), ("istft", shape, ""), ("copy", shape, ""), ("torch_istft", shape, "")]
    lines = []
    for name, shape, tree in runs:
        tmp = tempfile.mkdtemp(prefix="rows_istft_")
        cmd = [sys.executable, os.path.abspath(__file__), "--kernel-only", name, "--shape", shape, "--steps", str(steps)] + (["--tree", tree] if tree else [])
        if prof and name not in ("torch_istft", "copy"):
            cmd = [prof, "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp, "-o", name, "--"] + cmd
        r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=240)
        res = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
        if r.returncode or not res:
            sys.stderr.write(r.stdout[-2000:] + r.stderr[-2000:])
            raise SystemExit("variant %s failed (%d): nothing more is started" % (name, r.returncode))
        line = json.loads(res[-1][7:])
        line["tree"] = "parent" if tree else "this"
        stats = kernel_stats(tmp)
        shutil.rmtree(tmp, ignore_errors=True)
        for kern in ("k_spec", "k_istft"):
            mine = [v[1] / 1e3 for k, v in stats.items() if kern in k]
            if mine:
                line["kernel"], line["kernel_us"] = kern, round(sum(mine), 2)
        lines.append(line)
        print(json.dumps(line), flush=True)
    table = ["shape | variant | tree | kernel (trace) | call (events)", "---|---|---|---|---"]
    us = lambda v: "%.2f us" % v if v else "n/a"                                               # noqa: E731
    for l in lines:
        table.append("%s | %s | %s | %s | %s" % (tuple(l["shape"]), l["variant"], l["tree"], us(l.get("kernel_us")), us(l["events_us"])))
    print("\n".join(table))
    if write:
        with open(write, "w") as f:
            f.write("# tools/bench_rows_istft.py --steps %d: one process per run, under rocprofv3 --kernel-trace --stats but for copy and torch_istft\n" % steps)
            f.write("\n".join(json.dumps(l) for l in lines) + "\n\n" + "\n".join(table) + "\n")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--kernel-only", default="", help="one of %s: run that variant alone (under rocprofv3)" % ", ".join(VARIANTS))
    ap.add_argument("--shape", default="512", choices=sorted(SHAPES))
    ap.add_argument("--tree", default="", help="import the package from this checkout instead (spec_power only)")
    ap.add_argument("--parent-tree", default="", help="a built checkout of the parent commit: spec_power is timed on both, alternating")
    ap.add_argument("--write", default="", help="also write the lines and the table to this file")
    args = ap.parse_args()
    if args.kernel_only:
        child(args.kernel_only, args.shape, args.steps, args.tree)
    else:
        parent(args.steps, args.write, args.parent_tree)
