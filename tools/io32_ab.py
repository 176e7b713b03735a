#!/usr/bin/env python3
"""float64 vs float32 / complex64 I/O of the batched detector pipeline, on one box.

  1. interleaved A/B of DetectorSweep.run(io="f64") against io="f32": 4x8, N = 128, N_res = 512, fp16 predict and
     fit, default chunk, Eb/No 6 / 12 / 18 dB -- bench.py's `sweep` record, both widths in alternating order;
  2. per step at the headline shape (one default chunk of blocks): gen + train + predict + detect, CUDA events;
  3. unless --no-trace: the same steps again in a child process under `rocprofv3 --kernel-trace --stats`, and the
     kernel time of gen_frames_kernel, the predict kernel and detect_count_kernel in both widths.

    python tools/io32_ab.py [--rounds 3] [--steps 10] [--no-trace | --trace-only] [--out profiles/io32_ab.txt]
"""
import argparse
import csv
import glob
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)


def make_sweep(io):
    from esn_ofdm_mimo_amd.montecarlo import DetectorSweep, LinkParams
    return DetectorSweep(LinkParams(), n_reservoir=512, noise=0.001, seed=1234, precision="f16", fit_precision="f16",
                         io=io)


def sweep_ab(torch, rounds, log):
    sw = {io: make_sweep(io) for io in ("f64", "f32")}
    F = sw["f64"].p.coherence_symbols
    chunk = sw["f64"].default_chunk_blocks(F)
    blocks = 3 * chunk
    points = [6.0, 12.0, 18.0]
    for s in sw.values():                                        # warm-up: allocator, packed images, code objects
        s.run([points[0]], chunk, frames_per_block=F)
    rate = {"f64": [], "f32": []}
    counts = {}
    for r in range(rounds):
        for io in (("f64", "f32") if r % 2 == 0 else ("f32", "f64")):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            _, c = sw[io].run(points, blocks, frames_per_block=F)
            torch.cuda.synchronize()
            rate[io].append(len(points) * blocks * F / (time.perf_counter() - t0))
            counts.setdefault(io, c)
    same = bool((counts["f64"] == counts["f32"]).all())
    log(f"[sweep] 4x8 N=128 N_res=512 fp16, {len(points)} points x {blocks} blocks x {F} frames (chunk {chunk}), "
        f"{rounds} interleaved rounds")
    for io in ("f64", "f32"):
        log(f"[sweep] io={io}: median {statistics.median(rate[io]) / 1e6:.3f} M symbols/s  "
            f"(runs {', '.join(f'{x / 1e6:.3f}' for x in rate[io])})")
    log(f"[sweep] f32 / f64 = {statistics.median(rate['f32']) / statistics.median(rate['f64']):.3f}; "
        f"counters identical: {same}")


def one_step(torch, sw, G, F):
    """What DetectorSweep.run launches for blocks 0 .. G - 1 at 12 dB, without the counter sums."""
    data = sw.src.blocks_fast(12.0, 0, 0, G, F, io="c64" if sw.io == "f32" else "c128")
    sw.set_snr(12.0, G)
    sw.train(data["pilot_y"], data["pilot_x"], seed=sw.stream_seed(0, 0))
    err, bits = (torch.zeros(G, dtype=torch.int64, device=sw.device) for _ in range(2))
    sw.detect(data["data_y"], data["data_bits"], F, err, bits, seed=sw.stream_seed(0, 1))


def step_times(torch, steps, log, tag="[step]"):
    """gen + train + predict + detect of one default chunk of blocks, per width, interleaved step by step."""
    sw = {io: make_sweep(io) for io in ("f64", "f32")}
    F = sw["f64"].p.coherence_symbols
    G = sw["f64"].default_chunk_blocks(F)
    ms = {"f64": [], "f32": []}
    for i in range(steps + 2):
        for io in ("f64", "f32"):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            one_step(torch, sw[io], G, F)
            b.record()
            torch.cuda.synchronize()
            if i >= 2:
                ms[io].append(a.elapsed_time(b))
    log(f"{tag} one step = {G} blocks x {F} frames ({G * F} data frames): gen + train + predict + detect")
    for io in ("f64", "f32"):
        log(f"{tag} io={io}: median {statistics.median(ms[io]):.2f} ms  (min {min(ms[io]):.2f}, max {max(ms[io]):.2f})")
    log(f"{tag} f64 / f32 = {statistics.median(ms['f64']) / statistics.median(ms['f32']):.3f}")


KERNELS = ("gen_frames_kernel", "recur_skew16_kernel", "detect_count_kernel")


def kernel_trace(log, steps):
    if not glob.glob("/opt/rocm*/bin/rocprofv3"):
        log("[trace] rocprofv3 not found: skipped")
        return
    with tempfile.TemporaryDirectory() as d:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "io32", "--",
               sys.executable, os.path.abspath(__file__), "--child-steps", str(steps)]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
        if r.returncode != 0:
            log(f"[trace] rocprofv3 exited with {r.returncode}: {r.stderr[-400:]}")
            return
        stats = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
        if not stats:
            log("[trace] no kernel_stats.csv written")
            return
        log(f"[trace] rocprofv3 --kernel-trace --stats, {steps} steps per width (template argument: true = float32 I/O)")
        with open(stats[0]) as f:
            for row in csv.DictReader(f):
                name = row.get("Name", "")
                if any(k in name for k in KERNELS):
                    short = name.split("(")[0].replace("void ", "")
                    log(f"[trace] {short:60s} calls {int(row['Calls']):5d}  avg {float(row['AverageNs']) / 1e6:8.3f} ms")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--no-trace", action="store_true")
    ap.add_argument("--trace-only", action="store_true", help="part 3 alone")
    ap.add_argument("--out", default=None)
    ap.add_argument("--child-steps", type=int, default=0, help=argparse.SUPPRESS)
    args = ap.parse_args()
    import torch
    lines = []

    def log(s):
        print(s, flush=True)
        lines.append(s)
    if args.child_steps:                 # the traced child: the per-step loop only
        step_times(torch, args.child_steps, log, tag="[child]")
        return
    if not args.trace_only:
        sweep_ab(torch, args.rounds, log)
        step_times(torch, args.steps, log)
    if not args.no_trace:
        kernel_trace(log, 5)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
