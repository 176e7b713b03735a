#!/usr/bin/env python3
"""What a reservoir costs on the device and on the host, and what `reservoirs="fresh"` costs a sweep.

For every N_res (default 100 300 512 2048):
    device   generate + spectral radius (24 squarings) + scale through reservoirs.generate, per reservoir, for a batch
             of 1 and for a full chunk (the memory-bounded default of DetectorSweep(reservoirs="fresh"), at most
             --max-chunk); device events, warmed, median of the repeats
    host     montecarlo.draw_reservoir (np.linalg.eigvals) on the CPUs this process is given, median
    error    |device radius - max|eigvals|| / max|eigvals| on the matrix the device drew (copied to the host)
Then DetectorSweep.run symbols/s and BER at 6, 12 and 21 dB for "shared", "per_block" (pool of 8) and "fresh" at the
headline configuration (4x8 link, N_res = 512, fp16 fit and predict).

--split adds the split-operand radius ("f16x2": csrc/esn_specrad_split.hip) beside the float64 one:
    radius   esn_spectral_radius_batch against esn_spectral_radius_split_batch alone (no draw, no scale) on a full
             chunk, each at K = 24 and 16, the four candidates interleaved inside every repeat of one process
    sweep    "fresh" with the float64 radius and with f16x2, K = 16, each with the radius cache of DetectorSweep off
             and on ("+cache"), beside "shared"; without --split the "fresh" row runs with the cache off, as the
             figures recorded before the cache existed did

    python tools/time_reservoir_gen.py [--out profiles/reservoir_gen_time.txt] [--skip-sweep] [--host-2048]
    python tools/time_reservoir_gen.py --split --skip-gen --n-res 512 2048 --out profiles/reservoir_split_time.txt
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from esn_ofdm_mimo_amd import _lib, reservoirs  # noqa: E402
from esn_ofdm_mimo_amd.montecarlo import DetectorSweep, LinkParams, draw_reservoir  # noqa: E402


def device_ms(n_res, n_sets, repeats, warmup=2):
    """sorted ms of generate(n_sets) (draw + radius + scale; check_status=False: no host read inside the events)"""
    def call():
        return reservoirs.generate(16, 8, n_res, 0.9, 0.1, 5, first_set=0, n_sets=n_sets, check_status=False)
    for _ in range(warmup):
        call()
    torch.cuda.synchronize()
    ms = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        call()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return sorted(ms)


def radius_ms(n_res, n_sets, repeats, warmup=2):
    """{(precision, K): sorted ms} of the radius alone on n_sets drawn matrices, the candidates interleaved in every
    repeat; and the worst relative difference of f16x2 from f64 at the same K"""
    W = reservoirs.generate(16, 8, n_res, 0.9, 0.1, 5, first_set=0, n_sets=n_sets, check_status=False)[0]
    W = W * (1.0 / 0.9)                                                      # (any scale: the radius follows it)
    cands = [("f64", 24), ("f16x2", 24), ("f64", 16), ("f16x2", 16)]
    got = {}
    for _ in range(warmup):
        for prec, k in cands:
            got[(prec, k)] = reservoirs.spectral_radius(W, n_squarings=k, precision=prec)
    torch.cuda.synchronize()
    ms = {c: [] for c in cands}
    for _ in range(repeats):
        for prec, k in cands:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            reservoirs.spectral_radius(W, n_squarings=k, precision=prec)
            b.record()
            torch.cuda.synchronize()
            ms[(prec, k)].append(a.elapsed_time(b))
    diff = {k: float(((got[("f16x2", k)] - got[("f64", k)]).abs() / got[("f64", k)]).max().cpu()) for k in (24, 16)}
    return {c: sorted(v) for c, v in ms.items()}, diff


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n-res", type=int, nargs="+", default=[100, 300, 512, 2048])
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--max-chunk", type=int, default=256)
    ap.add_argument("--host-repeats", type=int, default=3)
    ap.add_argument("--host-2048", action="store_true", help="time the host draw at N_res >= 2048 too (8.8 s each)")
    ap.add_argument("--skip-sweep", action="store_true")
    ap.add_argument("--sweep-repeats", type=int, default=3, help="timed runs of every sweep row (median [min .. max])")
    ap.add_argument("--skip-gen", action="store_true", help="leave the generate / host draw table out")
    ap.add_argument("--split", action="store_true", help="time the f16x2 radius beside the float64 one")
    ap.add_argument("--blocks", type=int, default=0, help="blocks per Eb/No point of the sweeps (0: two default chunks)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"device {_lib.device_info()['arch']}  CPUs {len(os.sched_getaffinity(0))} (BLAS threads: OMP_NUM_THREADS={os.environ.get('OMP_NUM_THREADS', 'unset')})  repeats {a.repeats} (median [min .. max])")
    if not a.skip_gen:
        say("N_res  batch   device ms/reservoir                host draw_reservoir s   radius rel. error vs eigvals")
    for n in ([] if a.skip_gen else a.n_res):
        budget = DetectorSweep.FRESH_BUDGET_BYTES // (DetectorSweep.FRESH_BYTES_PER_BLOCK_N2 * n * n)
        full = max(1, min(a.max_chunk, budget))
        host = None
        if n < 2048 or a.host_2048:
            ts = []
            for r in range(a.host_repeats):
                t0 = time.perf_counter()
                draw_reservoir(16, 8, n, 0.9, 0.1, 100 + r)
                ts.append(time.perf_counter() - t0)
            host = sorted(ts)[len(ts) // 2]
        err = None
        if n < 2048 or a.host_2048:
            W, _, _, radius, status = reservoirs.generate(16, 8, n, 0.9, 0.1, 5, first_set=0, n_sets=1)
            w = W[0].cpu().numpy() * (float(radius[0].cpu()) / 0.9)              # the unscaled draw
            eig = float(np.max(np.abs(np.linalg.eigvals(w))))
            err = abs(float(radius[0].cpu()) - eig) / eig
        for s in sorted({1, full}):
            ms = device_ms(n, s, a.repeats)
            med = ms[len(ms) // 2]
            say(f"{n:5d}  {s:5d}   {med / s:9.4f} [{ms[0] / s:9.4f} .. {ms[-1] / s:9.4f}]   "
                f"{'-' if host is None else f'{host:8.3f}':>12s}            {'-' if err is None else f'{err:.2e}'}")
    if a.split:
        say("radius alone on a full chunk, ms per chunk, median [min .. max]; f16x2 against f64 at the same K")
        say("N_res  chunk   K   f64 ms                         f16x2 ms                       speed-up   worst rel. diff")
        for n in a.n_res:
            budget = DetectorSweep.FRESH_BUDGET_BYTES // (DetectorSweep.FRESH_BYTES_PER_BLOCK_N2 * n * n)
            full = max(1, min(a.max_chunk, budget))
            ms, diff = radius_ms(n, full, a.repeats)
            for k in (24, 16):
                d, h = ms[("f64", k)], ms[("f16x2", k)]
                say(f"{n:5d}  {full:5d}  {k:2d}   {d[len(d) // 2]:8.3f} [{d[0]:8.3f} .. {d[-1]:8.3f}]   "
                    f"{h[len(h) // 2]:8.3f} [{h[0]:8.3f} .. {h[-1]:8.3f}]   {d[len(d) // 2] / h[len(h) // 2]:6.2f} x   "
                    f"{diff[k]:.2e}")
    if not a.skip_sweep:
        ebno = [6, 12, 21]
        prm = LinkParams()
        F = prm.coherence_symbols
        say(f"DetectorSweep.run at the headline configuration: N_res 512, fp16 fit and predict, {F} frames per block, "
            f"Eb/No {ebno} dB")
        split = dict(reservoirs="fresh", radius_precision="f16x2", radius_squarings=16)
        rows = [("shared", dict(reservoirs="shared")), ("per_block", dict(reservoirs="per_block", pool=8)),
                ("fresh", dict(reservoirs="fresh", fresh_radius_cache=False))]
        if a.split:
            rows = [rows[0], rows[2], ("fresh+cache", dict(reservoirs="fresh")),
                    ("f16x2/16", dict(fresh_radius_cache=False, **split)), ("f16x2/16+cache", split)]
        for name, kw in rows:
            t0 = time.perf_counter()
            sw = DetectorSweep(prm, n_reservoir=512, noise=0.001, seed=1234, precision="f16", fit_precision="f16", **kw)
            t_init = time.perf_counter() - t0
            chunk = sw.default_chunk_blocks(F)
            blocks = a.blocks or 2 * chunk
            sw.run(ebno[:1], min(blocks, chunk))                                  # warm-up: allocations, first launches
            torch.cuda.synchronize()
            dts = []
            for _ in range(a.sweep_repeats):
                t0 = time.perf_counter()
                ber, cnt = sw.run(ebno, blocks)
                torch.cuda.synchronize()
                dts.append(time.perf_counter() - t0)
            dts.sort()
            sym = len(ebno) * blocks * F
            say(f"  {name:14s} constructor {t_init:7.2f} s   chunk {chunk:5d}   blocks/point {blocks:6d}   "
                f"{sym / dts[len(dts) // 2] / 1e6:8.3f} [{sym / dts[-1] / 1e6:8.3f} .. {sym / dts[0] / 1e6:8.3f}] M symbols/s   "
                "BER " + "  ".join(f"{e} dB {b:.4e}" for e, b in zip(ebno, ber)))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
