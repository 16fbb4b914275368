#!/usr/bin/env python3
"""Cost of normalising rows (lw_norm_rows: k_norm_sum + k_norm_fold + k_norm_apply) next to a plain copy of the same bytes and to
torch's masked chain for the same result.

Shapes: [64][1][1][480000] f32 under Normalize.wav2vec2() (64 utterances of 30 s at 16 kHz) and [256][1][80][3000] under
Normalize.cmvn() (20 480 scopes of a dozen chunks), out of place, every line full.  Source and destination tensors are rotated
over >= 0.5 GiB each so that neither stays in the Infinity Cache.  Yardsticks from the same session: dst.copy_(src) of the same
bytes, and torch's chain (mask, masked mean, masked centred variance, scale, mask), both by HIP events.  The pass reads every
element twice and writes it once, so 1.5 times the copy, which reads once and writes once, is its floor.

Every variant runs in a process of its own under
    rocprofv3 --kernel-trace --stats -- python tools/bench_rows_norm.py --kernel-only NAME
with nothing else traced and no counters; the kernels' own times are the k_norm_* rows of that run's kernel statistics, and the
child also times its calls with HIP events (the host side of a call shows in those).  Without --kernel-only this script starts
those runs one after the other, stops at the first that fails, and prints one JSON line per variant and a table:
    python tools/bench_rows_norm.py [--steps 50] [--write profiles/rows_norm_bench.txt]"""
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

SHAPES = {"64x480000": ((64, 1, 1, 480000), "wav2vec2"), "256x80x3000": ((256, 1, 80, 3000), "cmvn")}
KINDS = ["copy", "torch_chain", "norm"]
VARIANTS = ["%s_%s" % (k, s) for s in SHAPES for k in KINDS]
ROTATE_BYTES = 1 << 29


def child(name, steps):
    import torch
    kind, shape = name.rsplit("_", 1)
    shape, preset = SHAPES[shape]
    nbytes = shape[0] * shape[1] * shape[2] * shape[3] * 4
    nb = -(-ROTATE_BYTES // nbytes)
    gen = torch.Generator(device="cuda").manual_seed(1)
    srcs = [torch.randn(shape, device="cuda", generator=gen).mul_(0.1).add_(0.01) for _ in range(nb)]
    dsts = [torch.empty_like(s) for s in srcs]
    line = {"variant": name, "steps": steps, "shape": list(shape), "bytes": nbytes, "buffers_rotated": nb}
    nm = None
    if kind == "copy":
        fn = lambda k: dsts[k % nb].copy_(srcs[k % nb])                                         # noqa: E731
    elif kind == "torch_chain":
        lengths = torch.full((shape[0], 1, 1, 1), shape[3], device="cuda")
        dims, eps = ((2, 3), 1e-7) if preset == "wav2vec2" else ((3,), 1e-20)
        count = float(shape[3] * (shape[2] if preset == "wav2vec2" else 1))

        def fn(k):
            x = srcs[k % nb]
            mask = torch.arange(shape[3], device="cuda") < lengths
            mean = (x * mask).sum(dim=dims, keepdim=True) / count
            c = (x - mean) * mask
            var = (c * c).sum(dim=dims, keepdim=True) / count
            torch.mul(c, torch.rsqrt(var + eps), out=dsts[k % nb])
    else:
        from lewton_amd.rows import Normalize
        nm = Normalize.wav2vec2() if preset == "wav2vec2" else Normalize.cmvn()
        n = [shape[3]] * shape[0]
        fn = lambda k: nm.run(srcs[k % nb], n, out=dsts[k % nb])                                # noqa: E731
    line["events_us"] = round(timed(fn, steps), 2)
    if nm is not None:
        line["launches"] = nm.last_launches()
        nm.close()
    print("RESULT " + json.dumps(line), flush=True)


def parent(steps, write):
    prof = shutil.which("rocprofv3")
    lines = []
    for name in VARIANTS:
        tmp = tempfile.mkdtemp(prefix="rows_norm_")
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
        mine = {k.split("(")[0].replace("void ", ""): round(v[1] / 1e3, 2) for k, v in stats.items() if "k_norm" in k}
        if mine:
            line.update(kernels_us=mine, kernel_us=round(sum(mine.values()), 2))
        elif stats and name.startswith("norm"):
            line["kernels_seen"] = {k.split("(")[0][:60]: round(v[1] / 1e3, 2) for k, v in stats.items()}
        lines.append(line)
        print(json.dumps(line), flush=True)
    by = {l["variant"]: l for l in lines}
    table = ["shape | k_norm_sum | k_norm_fold | k_norm_apply | kernels together | call (events) | copy_(src) (events) | kernels / (1.5 x copy) | torch's chain (events)",
             "---|---|---|---|---|---|---|---|---"]
    for s in SHAPES:
        copy, chain, l = by["copy_" + s]["events_us"], by["torch_chain_" + s]["events_us"], by["norm_" + s]
        ks, k = l.get("kernels_us", {}), l.get("kernel_us")
        table.append("%s (%s) | %s | %s | %s | %s | %.2f us | %.2f us | %s | %.2f us" % (
            s, SHAPES[s][1], ks.get("k_norm_sum", "n/a"), ks.get("k_norm_fold", "n/a"), ks.get("k_norm_apply", "n/a"),
            "%.2f us" % k if k else "n/a", l["events_us"], copy, "%.2f" % (k / (1.5 * copy)) if k else "n/a", chain))
    print("\n".join(table))
    if write:
        with open(write, "w") as f:
            f.write("# tools/bench_rows_norm.py --steps %d: one process per variant under rocprofv3 --kernel-trace --stats\n" % steps)
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
