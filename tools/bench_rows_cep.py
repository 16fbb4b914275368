#!/usr/bin/env python3
"""Cost of cepstra and deltas of feature rows (lw_cep_rows: k_cep) next to a plain copy of the bytes the pass must move and to
torch's chain for the same features.

Shapes, every line full, delta-deltas of width 2: [64][1][80][3000] log-mel rows -> 13 cepstra + deltas + delta-deltas (the
headline: 64 utterances of 30 s), the same rows -> the 80 lines themselves + deltas + delta-deltas (the identity), and
[64][1][256][3000] -> 256 + deltas + delta-deltas through a dense matrix (the one compute-bound shape).  Source and destination
tensors are rotated over >= 0.5 GiB each so that neither stays in the Infinity Cache.  Yardsticks from the same session: a flat
dst.copy_(src) of HALF the bytes the pass reads and writes (a copy reads and writes each of its bytes once, so it moves the same
total: the pass's floor), and torch's chain (matmul, conv1d over replicate-padded lines twice, cat), both by HIP events.

Every variant runs in a process of its own under
    rocprofv3 --kernel-trace --stats -- python tools/bench_rows_cep.py --kernel-only NAME
with nothing else traced and no counters; the kernel's own time is the k_cep row of that run's kernel statistics (for the copy
and torch's chain: the kernels of their trace that ran in every call -- for the chain that sum also holds the kernels the library
tries while it chooses an algorithm during the warm-up, so it is far above the chain's event time and is not a figure to quote;
the chain is compared by events), and the child also times its calls with HIP events (the host side of a call and the gaps between
launches show in those).  Ratios are quoted like for like: kernel over kernel, events over events.  Without --kernel-only this script starts those
runs one after the other, stops at the first that fails, and prints one JSON line per variant and a table:
    python tools/bench_rows_cep.py [--steps 50] [--write profiles/rows_cep_bench.txt]"""
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

# name -> (rows, n_in, n_out, frames, identity)
SHAPES = {"80to13": (64, 80, 13, 3000, False), "80identity": (64, 80, 80, 3000, True), "256to256": (64, 256, 256, 3000, False)}
KINDS = ["copy", "torch_chain", "cep"]
VARIANTS = ["%s_%s" % (k, s) for s in SHAPES for k in KINDS]
ROTATE_BYTES = 1 << 29
ORDER, WIDTH = 2, 2
WARMUP = 10


def child(name, steps):
    import numpy as np
    import torch
    kind, shape = name.rsplit("_", 1)
    rows, n_in, n_out, frames, identity = SHAPES[shape]
    src_bytes, dst_bytes = rows * n_in * frames * 4, rows * n_out * (1 + ORDER) * frames * 4
    flops = rows * frames * ((0 if identity else 2 * n_in * n_out) + ORDER * n_out * 3 * WIDTH)
    line = {"variant": name, "steps": steps, "src": [rows, 1, n_in, frames], "dst": [rows, 1, n_out * (1 + ORDER), frames],
            "bytes": src_bytes + dst_bytes, "flops": flops}
    gen = torch.Generator(device="cuda").manual_seed(1)
    cp = None
    if kind == "copy":
        half = (src_bytes + dst_bytes) // 8                                                   # floats: half the bytes moved
        nb = -(-ROTATE_BYTES // (half * 4))
        a = [torch.randn(half, device="cuda", generator=gen) for _ in range(nb)]
        b = [torch.empty_like(t) for t in a]
        fn = lambda k: b[k % nb].copy_(a[k % nb])                                             # noqa: E731
    else:
        nb = -(-ROTATE_BYTES // min(src_bytes, dst_bytes))
        srcs = [torch.randn((rows, 1, n_in, frames), device="cuda", generator=gen).mul_(20.0).sub_(40.0) for _ in range(nb)]
        from lewton_amd.rows import Cepstrum, dct_matrix
        m = None if identity else dct_matrix(n_out, n_in)
        if kind == "torch_chain":
            mt = None if m is None else torch.from_numpy(m).cuda()
            probe = Cepstrum.deltas(4, ORDER, WIDTH)
            w = probe.delta_weights()
            probe.close()
            k1 = np.zeros(2 * WIDTH + 1, np.float32)
            for n in range(1, WIDTH + 1):
                k1[WIDTH + n], k1[WIDTH - n] = w[n - 1], -w[n - 1]
            kern = torch.from_numpy(k1).cuda()[None, None, :]

            def delta(s):
                p = torch.nn.functional.pad(s.reshape(rows * n_out, 1, frames), (WIDTH, WIDTH), mode="replicate")
                return torch.nn.functional.conv1d(p, kern).reshape(rows, 1, n_out, frames)

            def fn(k):
                x = srcs[k % nb]
                s = x if mt is None else torch.matmul(mt, x)
                d = delta(s)
                return torch.cat([s, d, delta(d)], dim=2)
        else:
            dsts = [torch.empty((rows, 1, n_out * (1 + ORDER), frames), device="cuda") for _ in range(nb)]
            cp = Cepstrum(n_in, m, ORDER, WIDTH)
            n = [frames] * rows
            fn = lambda k: cp.run(srcs[k % nb], n, out=dsts[k % nb])                          # noqa: E731
    line["buffers_rotated"] = nb
    line["events_us"] = round(timed(fn, steps, WARMUP), 2)
    if cp is not None:
        line["launches"], line["tile_frames"] = cp.last_launches(), cp.tile_frames
        cp.close()
    print("RESULT " + json.dumps(line), flush=True)


def parent(steps, write):
    prof = shutil.which("rocprofv3")
    lines = []
    for name in VARIANTS:
        tmp = tempfile.mkdtemp(prefix="rows_cep_")
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
        mine = [v[1] / 1e3 for k, v in stats.items() if "k_cep" in k]
        if mine:
            line["kernel_us"] = round(sum(mine), 2)
            line["kernel_TB_per_s"] = round(line["bytes"] / (line["kernel_us"] * 1e-6) / 1e12, 3)
            line["kernel_TFLOP_per_s"] = round(line["flops"] / (line["kernel_us"] * 1e-6) / 1e12, 2)
        elif stats and not name.startswith("cep"):  # the yardstick's own kernels: those that ran in every call (not the set-up's)
            per_call = {k: v for k, v in stats.items() if v[0] >= steps}
            if per_call:
                line["kernel_us"] = round(sum(v[0] * v[1] for v in per_call.values()) / (steps + WARMUP) / 1e3, 2)
                line["kernels"] = len(per_call)
        elif stats:
            line["kernels_seen"] = {k.split("(")[0][:60]: round(v[1] / 1e3, 2) for k, v in stats.items()}
        lines.append(line)
        print(json.dumps(line), flush=True)
    by = {l["variant"]: l for l in lines}
    table = ["shape | k_cep (trace) | copy_ of the same bytes (trace) | k_cep / copy, kernels | torch's chain (trace) | torch's chain / k_cep, kernels | call (events) | copy_ (events) | call / copy, events | torch's chain (events)",
             "---|---|---|---|---|---|---|---|---|---"]
    us = lambda v: "%.2f us" % v if v else "n/a"                                               # noqa: E731
    for s in SHAPES:
        cp, ch, l = by["copy_" + s], by["torch_chain_" + s], by["cep_" + s]
        k, ck, tk = l.get("kernel_us"), cp.get("kernel_us"), ch.get("kernel_us")
        table.append("%s | %s | %s | %s | %s | %s | %.2f us | %.2f us | %.2f | %.2f us" % (
            s, us(k), us(ck), "%.2f" % (k / ck) if k and ck else "n/a", us(tk), "%.2f" % (tk / k) if k and tk else "n/a", l["events_us"],
            cp["events_us"], l["events_us"] / cp["events_us"], ch["events_us"]))
    print("\n".join(table))
    if write:
        with open(write, "w") as f:
            f.write("# tools/bench_rows_cep.py --steps %d: one process per variant under rocprofv3 --kernel-trace --stats\n" % steps)
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
