#!/usr/bin/env python3
"""Cost of finishing feature rows (lw_feat_rows: k_feat_log + k_feat_fin) next to a plain copy of the same bytes and to torch's own
chain, and of reflect against zero padding in k_spec.

Shapes: features [256][1][80][103] f32 (what Spectrogram(400, 160, 80 mel bands) makes of 256 rows of 16 384 samples) and
[64][1][80][3000] (Whisper's 30 s windows).  Variants per shape: LogCompress.whisper() (top = 8: two launches) and the same with
top = inf (one launch), out of place, every line full.  Source and destination tensors are rotated over >= 0.5 GiB each so that
neither stays in the Infinity Cache.  Yardsticks from the same session: dst.copy_(src) of the same bytes, and torch's chain
(clamp, log10, amax over the row, maximum, add, mul), both by HIP events.  The kernels read and write every element once per
launch, so two launches cannot beat twice the copy.  On the shape of tools/bench_rows_spec.py ([256][1][16384], 400 / 160 / 80 mel
bands, route 0) k_spec is timed with zero and with reflect padding.

Every variant runs in a process of its own under
    rocprofv3 --kernel-trace --stats -- python tools/bench_rows_feat.py --kernel-only NAME
with nothing else traced and no counters; the kernels' own times are the k_feat_log / k_feat_fin / k_spec rows of that run's
kernel statistics, and the child also times its steps with HIP events (the host side of a call shows in those).  Without
--kernel-only this script starts those runs one after the other, stops at the first that fails, and prints one JSON line per
variant and a table:
    python tools/bench_rows_feat.py [--steps 100] [--write profiles/rows_feat_bench.txt]"""
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

SHAPES = {"256x80x103": (256, 1, 80, 103), "64x80x3000": (64, 1, 80, 3000)}
KINDS = ["copy", "torch_chain", "feat_top8", "feat_topinf"]
SPEC = ["spec_zero", "spec_reflect"]
VARIANTS = ["%s_%s" % (k, s) for s in SHAPES for k in KINDS] + SPEC
ROTATE_BYTES = 1 << 29


def child(name, steps):
    import torch
    line = {"variant": name, "steps": steps}
    if name in SPEC:
        from lewton_amd.rows import Spectrogram, mel_filterbank
        rows, samples = 256, 16384
        nb = -(-ROTATE_BYTES // (rows * samples * 4))
        gen = torch.Generator(device="cuda").manual_seed(1)
        srcs = [torch.randn((rows, 1, samples), device="cuda", generator=gen) for _ in range(nb)]
        sp = Spectrogram(400, 160, mel=mel_filterbank(16000, 400, 80), pad_mode=name[5:])
        dsts = [torch.zeros((rows, 1, 80, sp.frames(samples)), device="cuda") for _ in range(nb)]
        lengths = [samples] * rows
        line.update(shape=[rows, 1, samples], buffers_rotated=nb,
                    events_us=round(timed(lambda k: sp.run(srcs[k % nb], lengths, out=dsts[k % nb]), steps), 2))
        sp.close()
    else:
        kind, shape = name.rsplit("_", 1)
        shape = SHAPES[shape]
        nbytes = shape[0] * shape[1] * shape[2] * shape[3] * 4
        nb = -(-ROTATE_BYTES // nbytes)
        gen = torch.Generator(device="cuda").manual_seed(1)
        srcs = [torch.randn(shape, device="cuda", generator=gen).square_() for _ in range(nb)]      # a power: non-negative
        dsts = [torch.empty_like(s) for s in srcs]
        line.update(shape=list(shape), bytes=nbytes, buffers_rotated=nb)
        if kind == "copy":
            fn = lambda k: dsts[k % nb].copy_(srcs[k % nb])                                         # noqa: E731
        elif kind == "torch_chain":
            def fn(k):
                x = torch.clamp(srcs[k % nb], min=1e-10).log10()
                x = torch.maximum(x, x.amax(dim=(1, 2, 3), keepdim=True) - 8.0)
                torch.mul(x + 4.0, 0.25, out=dsts[k % nb])
        else:
            from lewton_amd.rows import LogCompress
            lc = LogCompress(top=8.0 if kind == "feat_top8" else float("inf"))
            frames = [shape[3]] * shape[0]
            fn = lambda k: lc.run(srcs[k % nb], frames, out=dsts[k % nb])                           # noqa: E731
        line["events_us"] = round(timed(fn, steps), 2)
        if kind.startswith("feat"):
            line["launches"] = lc.last_launches()
            lc.close()
    print("RESULT " + json.dumps(line), flush=True)


def parent(steps, write):
    prof = shutil.which("rocprofv3")
    lines = []
    for name in VARIANTS:
        tmp = tempfile.mkdtemp(prefix="rows_feat_")
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
        mine = {k.split("(")[0].replace("void ", ""): round(v[1] / 1e3, 2) for k, v in stats.items() if "k_feat" in k or "k_spec" in k}
        if mine:
            line.update(kernels_us=mine, kernel_us=round(sum(mine.values()), 2))
        elif stats:
            line["kernels_seen"] = {k.split("(")[0][:60]: round(v[1] / 1e3, 2) for k, v in stats.items()}
        lines.append(line)
        print(json.dumps(line), flush=True)
    by = {l["variant"]: l for l in lines}
    table = ["shape | variant | kernels (rocprofv3) | call (events) | copy_(src) (events) | kernels / copy | GB/s moved by the kernels | torch's chain (events)",
             "---|---|---|---|---|---|---|---"]
    for s in SHAPES:
        copy, chain = by["copy_" + s]["events_us"], by["torch_chain_" + s]["events_us"]
        for kind in ("feat_top8", "feat_topinf"):
            l = by["%s_%s" % (kind, s)]
            k = l.get("kernel_us")
            moved = 2 * l["bytes"] * l["launches"]                      # every launch reads and writes every element
            table.append("%s | %s (%d launch%s) | %s | %.2f us | %.2f us | %s | %s | %.2f us" % (
                s, kind, l["launches"], "es" if l["launches"] > 1 else "", "%.2f us" % k if k else "n/a", l["events_us"], copy,
                "%.2f" % (k / copy) if k else "n/a", "%.0f" % (moved / (k * 1e-6) / 1e9) if k else "n/a", chain))
    z, r = by["spec_zero"], by["spec_reflect"]
    table.append("k_spec [256][1][16384], 400 / 160 / 80 mel bands, route 0: zero %s us, reflect %s us (rocprofv3); calls %.2f / %.2f us (events)" % (
        z.get("kernel_us", "n/a"), r.get("kernel_us", "n/a"), z["events_us"], r["events_us"]))
    print("\n".join(table))
    if write:
        with open(write, "w") as f:
            f.write("# tools/bench_rows_feat.py --steps %d: one process per variant under rocprofv3 --kernel-trace --stats\n" % steps)
            f.write("\n".join(json.dumps(l) for l in lines) + "\n\n" + "\n".join(table) + "\n")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--kernel-only", default="", help="one of %s: run that variant alone (under rocprofv3)" % ", ".join(VARIANTS))
    ap.add_argument("--write", default="", help="also write the lines and the table to this file")
    args = ap.parse_args()
    if args.kernel_only:
        child(args.kernel_only, args.steps)
    else:
        parent(args.steps, args.write)
