#!/usr/bin/env python3
"""Cost of the Kaldi-compatible filterbank front end (lw_spec_create_ex: k_spec with its per-frame prologue, then k_feat) on
[256][1][16384] rows at 16 kHz, 25 ms povey windows every 10 ms in a 512-point transform, 80 Kaldi mel bands, pre-emphasis 0.97.

Variants, each in a process of its own:
    fbank        Spectrogram(framing="kaldi", remove_dc=True, energy=True) + LogCompress("ln", FLT_EPSILON): k_spec<.., .., 1> + k_feat
    fbank_plain  the same object with remove_dc=False and energy=False: k_spec<.., .., 0> + k_feat.  fbank - fbank_plain is the
                 price of the prologue (the 64 chains of 400 dependent f64 additions per tile, and the staged span)
    stft         Spectrogram(512, 160, 400, center=False, mel=mel_filterbank(16000, 512, 80)): what an object made before
                 lw_spec_create_ex existed runs.  With --tree PATH the package is imported from another checkout (the parent
                 commit), so the two can be timed in one session; run it more than once per tree for the run-to-run spread
    torch        the same front end written with torch ops (unfold, mean, pre-emphasis, window, rfft, matmul, log); it has no
                 bit contract and is timed by events only
Source tensors are rotated over >= 0.5 GiB so that none stays in the Infinity Cache.  Under
    rocprofv3 --kernel-trace --stats -- python tools/bench_rows_fbank.py --kernel-only NAME
the kernels' own times are the k_spec and k_feat rows of that run's kernel statistics; the child also times its calls with HIP
events.  Without --kernel-only this script starts those runs one after the other, stops at the first that fails, and prints one
JSON line per run and a table:
    python tools/bench_rows_fbank.py [--steps 50] [--parent-tree PATH] [--write profiles/rows_fbank_bench.txt]"""
import argparse
import json
import os
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

ROWS, SAMPLES, RATE = 256, 16384, 16000
N_FFT, WIN, HOP, BANDS = 512, 400, 160, 80
ROTATE_BYTES = 1 << 29
VARIANTS = ["fbank", "fbank_plain", "stft", "torch"]
WARMUP = 10


def child(name, steps, tree):
    sys.path.insert(0, tree or ROOT)
    import numpy as np
    import torch
    from lewton_amd import rows as R        # (first: bench_rows_spec puts its own checkout in front of the path)
    from bench_rows_spec import timed
    in_bytes = ROWS * SAMPLES * 4
    nb = -(-ROTATE_BYTES // in_bytes)
    gen = torch.Generator(device="cuda").manual_seed(1)
    srcs = [torch.randn((ROWS, 1, SAMPLES), device="cuda", generator=gen).mul_(0.1) for _ in range(nb)]
    lengths = [SAMPLES] * ROWS
    line = {"variant": name, "tree": os.path.abspath(tree or ROOT), "rows": [ROWS, 1, SAMPLES], "buffers_rotated": nb, "steps": steps}
    if name == "torch":
        fb = torch.from_numpy(R.kaldi_mel_banks(RATE, N_FFT, BANDS)).cuda()
        a = 2 * np.pi * np.arange(WIN) / (WIN - 1)
        win = torch.from_numpy(((0.5 - 0.5 * np.cos(a)) ** 0.85).astype(np.float32)).cuda()
        eps = float(np.finfo(np.float32).eps)

        def fn(k):
            f = srcs[k % nb][:, 0].unfold(1, WIN, HOP)
            f = f - f.mean(dim=2, keepdim=True)
            e = (f * f).sum(dim=2)
            f = torch.cat([f[:, :, :1] * (1 - 0.97), f[:, :, 1:] - 0.97 * f[:, :, :-1]], dim=2) * win
            p = torch.fft.rfft(f, n=N_FFT).abs().pow(2)
            m = torch.matmul(p, fb.T)
            return torch.log(torch.clamp(torch.cat([e[:, :, None], m], dim=2), min=eps))
        line["events_us"] = round(timed(fn, steps, WARMUP), 2)
    else:
        if name == "stft":
            sp = R.Spectrogram(N_FFT, HOP, WIN, center=False, mel=R.mel_filterbank(RATE, N_FFT, BANDS))
        else:
            on = name == "fbank"
            sp = R.Spectrogram(N_FFT, HOP, WIN, "povey", center=False, mel=R.kaldi_mel_banks(RATE, N_FFT, BANDS), framing="kaldi",
                               preemphasis=0.97, remove_dc=on, energy=on)
        lg = R.LogCompress("ln", floor=float(np.finfo(np.float32).eps), top=float("inf"), add=0.0, mul=1.0)
        T = sp.frames(SAMPLES)
        dsts = [torch.empty((ROWS, 1, sp.features, T), device="cuda") for _ in range(2)]
        frames = [T] * ROWS

        def fn(k):
            sp.run(srcs[k % nb], lengths, out=dsts[k & 1])
            lg.run(dsts[k & 1], frames)
        line["events_us"] = round(timed(fn, steps, WARMUP), 2)
        line["frames"], line["features"], line["route"] = T, sp.features, sp.last_route()
        sp.close()
        lg.close()
    print("RESULT " + json.dumps(line), flush=True)


def parent(steps, write, parent_tree):
    from bench_rows_spec import kernel_stats
    prof = shutil.which("rocprofv3")
    runs = [("fbank", ""), ("fbank_plain", ""), ("stft", ""), ("torch", "")]
    if parent_tree:
        runs += [("stft", parent_tree), ("stft", ""), ("stft", parent_tree)]
    else:
        runs += [("stft", "")]
    lines = []
    for name, tree in runs:
        tmp = tempfile.mkdtemp(prefix="rows_fbank_")
        cmd = [sys.executable, os.path.abspath(__file__), "--kernel-only", name, "--steps", str(steps)] + (["--tree", tree] if tree else [])
        if prof and name != "torch":
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
        for kern in ("k_spec", "k_feat"):
            mine = [v[1] / 1e3 for k, v in stats.items() if kern in k]
            if mine:
                line[kern + "_us"] = round(sum(mine), 2)
        lines.append(line)
        print(json.dumps(line), flush=True)
    table = ["variant | tree | k_spec (trace) | k_feat (trace) | call (events)", "---|---|---|---|---"]
    us = lambda v: "%.2f us" % v if v else "n/a"                                               # noqa: E731
    for l in lines:
        table.append("%s | %s | %s | %s | %s" % (l["variant"], l["tree"], us(l.get("k_spec_us")), us(l.get("k_feat_us")), us(l["events_us"])))
    a, b = lines[0].get("k_spec_us"), lines[1].get("k_spec_us")
    if a and b:
        table.append("")
        table.append("the prologue (DC removal and energy): k_spec %.2f us - %.2f us = %.2f us, %.1f %% of the kernel without it" % (a, b, a - b, 100 * (a - b) / b))
    print("\n".join(table))
    if write:
        with open(write, "w") as f:
            f.write("# tools/bench_rows_fbank.py --steps %d: one process per run, under rocprofv3 --kernel-trace --stats but for torch\n" % steps)
            f.write("\n".join(json.dumps(l) for l in lines) + "\n\n" + "\n".join(table) + "\n")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--kernel-only", default="", help="one of %s: run that variant alone (under rocprofv3)" % ", ".join(VARIANTS))
    ap.add_argument("--tree", default="", help="import the package from this checkout instead (stft only)")
    ap.add_argument("--parent-tree", default="", help="a built checkout of the parent commit: stft is timed on both, twice each, alternating")
    ap.add_argument("--write", default="", help="also write the lines and the table to this file")
    args = ap.parse_args()
    if args.kernel_only:
        child(args.kernel_only, args.steps, args.tree)
    else:
        parent(args.steps, args.write, args.parent_tree)
