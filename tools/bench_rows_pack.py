#!/usr/bin/env python3
"""Cost of the frame-major model input (lw_pack_rows: k_pack) next to a plain copy of the bytes the pass must move and to torch's
chain for the same tensor.

Shapes, every row full, the mask asked for: [64][1][80][3000] log-mel rows -> the plain transpose in f32, the same -> bf16, LFR 7/6
with shift and scale -> bf16 (the FunASR input), and splice +-5 at stride 1 -> f32 (write-dominated: 11 x the source).  Source and
destination tensors are rotated over >= 0.5 GiB each so that neither stays in the Infinity Cache.  Yardsticks from the same
session: a flat dst.copy_(src) of HALF the bytes the pass reads and writes (a copy reads and writes each of its bytes once, so it
moves the same total: the pass's floor), and torch's chain (transpose().contiguous() or a clamped index_select, permute and
reshape; subtract, multiply, .to(dtype), the arange < lengths mask), both by HIP events.

Every variant runs in a process of its own under
    rocprofv3 --kernel-trace --stats -- python tools/bench_rows_pack.py --kernel-only NAME
with nothing else traced and no counters; the kernel's own time is the k_pack row of that run's kernel statistics (for the copy and
torch's chain: the kernels of their trace that ran in every call), and the child also times its calls with HIP events (the host
side of a call shows in those).  Ratios are quoted like for like: kernel over kernel, events over events.  Without --kernel-only
this script starts those runs one after the other, stops at the first that fails, and prints one JSON line per variant and a table:
    python tools/bench_rows_pack.py [--steps 50] [--write profiles/rows_pack_bench.txt]"""
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

# name -> (rows, F, frames, left, right, stride, dtype, shift and scale)
SHAPES = {"transposeF32": (64, 80, 3000, 0, 0, 1, "f32", False), "transposeBf16": (64, 80, 3000, 0, 0, 1, "bf16", False),
          "lfr76Bf16": (64, 80, 3000, 3, 3, 6, "bf16", True), "splice5F32": (64, 80, 3000, 5, 5, 1, "f32", False)}
KINDS = ["copy", "torch_chain", "pack"]
VARIANTS = ["%s_%s" % (k, s) for s in SHAPES for k in KINDS]
ROTATE_BYTES = 1 << 29
WARMUP = 10


def child(name, steps):
    import numpy as np
    import torch
    kind, shape = name.rsplit("_", 1)
    rows, F, frames, left, right, stride, dtype, affine = SHAPES[shape]
    W = left + right + 1
    D, t_out, es = W * F, -(-frames // stride), 4 if dtype == "f32" else 2
    tdtype = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}[dtype]
    src_bytes, dst_bytes = rows * F * frames * 4, rows * t_out * D * es + rows * t_out
    line = {"variant": name, "steps": steps, "src": [rows, 1, F, frames], "dst": [rows, 1, t_out, D], "dtype": dtype, "bytes": src_bytes + dst_bytes}
    gen = torch.Generator(device="cuda").manual_seed(1)
    pk = None
    if kind == "copy":
        half = (src_bytes + dst_bytes) // 8                                                   # floats: half the bytes moved
        nb = -(-ROTATE_BYTES // (half * 4))
        a = [torch.randn(half, device="cuda", generator=gen) for _ in range(nb)]
        b = [torch.empty_like(t) for t in a]
        fn = lambda k: b[k % nb].copy_(a[k % nb])                                             # noqa: E731
    else:
        nb = -(-ROTATE_BYTES // min(src_bytes, dst_bytes))
        srcs = [torch.randn((rows, 1, F, frames), device="cuda", generator=gen).mul_(20.0).sub_(40.0) for _ in range(nb)]
        rng = np.random.default_rng(1)
        shift = rng.standard_normal(D).astype(np.float32) if affine else None
        scale = (1.0 + 0.1 * rng.standard_normal(D)).astype(np.float32) if affine else None
        if kind == "torch_chain":
            sh, sc = (torch.from_numpy(v).cuda() for v in (shift, scale)) if affine else (None, None)
            idx = torch.clamp(torch.arange(t_out, device="cuda")[:, None] * stride - left + torch.arange(W, device="cuda")[None, :], 0, frames - 1).reshape(-1)
            lengths = torch.full((rows,), t_out, device="cuda")

            def fn(k):
                x = srcs[k % nb]
                if W == 1 and stride == 1:
                    y = x.transpose(2, 3).contiguous()
                else:
                    y = x.index_select(3, idx).reshape(rows, 1, F, t_out, W).permute(0, 1, 3, 4, 2).reshape(rows, 1, t_out, D)
                if sh is not None:
                    y = (y + sh) * sc
                return y.to(tdtype), torch.arange(t_out, device="cuda")[None, :] < lengths[:, None]
        else:
            from lewton_amd.rows import FramePack
            dsts = [torch.empty((rows, 1, t_out, D), dtype=tdtype, device="cuda") for _ in range(nb)]
            masks = [torch.empty((rows, t_out), dtype=torch.uint8, device="cuda") for _ in range(nb)]
            pk = FramePack(F, left, right, stride, "replicate", dtype, shift=shift, scale=scale)
            n = [frames] * rows
            fn = lambda k: pk.run(srcs[k % nb], n, out=dsts[k % nb], want_mask=masks[k % nb])  # noqa: E731
    line["buffers_rotated"] = nb
    line["events_us"] = round(timed(fn, steps, WARMUP), 2)
    if pk is not None:
        line["launches"], line["tile_frames"] = pk.last_launches(), pk.tile_frames
        pk.close()
    print("RESULT " + json.dumps(line), flush=True)


def parent(steps, write):
    prof = shutil.which("rocprofv3")
    lines = []
    for name in VARIANTS:
        tmp = tempfile.mkdtemp(prefix="rows_pack_")
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
        mine = [v[1] / 1e3 for k, v in stats.items() if "k_pack" in k]
        if mine:
            line["kernel_us"] = round(sum(mine), 2)
            line["kernel_TB_per_s"] = round(line["bytes"] / (line["kernel_us"] * 1e-6) / 1e12, 3)
        elif stats and not name.startswith("pack"):  # the yardstick's own kernels: those that ran in every call (not the set-up's)
            per_call = {k: v for k, v in stats.items() if v[0] >= steps}
            if per_call:
                line["kernel_us"] = round(sum(v[0] * v[1] for v in per_call.values()) / (steps + WARMUP) / 1e3, 2)
                line["kernels"] = len(per_call)
        elif stats:
            line["kernels_seen"] = {k.split("(")[0][:60]: round(v[1] / 1e3, 2) for k, v in stats.items()}
        lines.append(line)
        print(json.dumps(line), flush=True)
    by = {l["variant"]: l for l in lines}
    table = ["shape | k_pack (trace) | copy_ of the same bytes (trace) | k_pack / copy, kernels | torch's chain (trace) | torch's chain / k_pack, kernels | call (events) | copy_ (events) | call / copy, events | torch's chain (events)",
             "---|---|---|---|---|---|---|---|---|---"]
    us = lambda v: "%.2f us" % v if v else "n/a"                                               # noqa: E731
    for s in SHAPES:
        cp, ch, l = by["copy_" + s], by["torch_chain_" + s], by["pack_" + s]
        k, ck, tk = l.get("kernel_us"), cp.get("kernel_us"), ch.get("kernel_us")
        table.append("%s | %s | %s | %s | %s | %s | %.2f us | %.2f us | %.2f | %.2f us" % (
            s, us(k), us(ck), "%.2f" % (k / ck) if k and ck else "n/a", us(tk), "%.2f" % (tk / k) if k and tk else "n/a", l["events_us"],
            cp["events_us"], l["events_us"] / cp["events_us"], ch["events_us"]))
    print("\n".join(table))
    if write:
        with open(write, "w") as f:
            f.write("# tools/bench_rows_pack.py --steps %d: one process per variant under rocprofv3 --kernel-trace --stats\n" % steps)
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
