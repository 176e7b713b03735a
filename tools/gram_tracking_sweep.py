#!/usr/bin/env python3
"""Tracking from a multi-pilot start: DetectorSweep(solve_method="gram") on the two configurations of
tools/tracking_sweep.py, one Eb/No.  For every number of pilots P, on the same data frames:

    static      the read-out fitted once on the P pilots (P = 1: one run per lambda of the grid; P >= 2: the lambda chosen
                per block on the held-out last pilot)
    decisions   then re-fitted after every data symbol on the detector's own decisions, for every forgetting factor gamma
    genie       the same on the true transmit signal: the bound, not a receiver

(P = 1 tracks at the grid's middle lambda), per-symbol and block-mean BER of each; beside them the LS-MMSE baseline's
static / decisions / genie figures on the same frames (baseline_tracking_point, window 1), and the wall time of a tracked
chunk in this mode beside the shipped window-2 chunk (solve_method="auto", track_window=2, ridge at the grid's middle).
The JSON is rewritten after every run, so a run that is cut short leaves what it measured.

    python tools/gram_tracking_sweep.py [--preset 4x8|2x2] [--ebno 21] [--blocks 64] [--chunk 64] [--pilots 1 2 4]
                                        [--gammas 0 0.5 0.8 1] [--grid 1e-4 1e-3 1e-2] [--commit C] [--out file.json]

Writes profiles/gram_tracking_<preset>_<ebno>dB.json unless --out is given.  Needs an MI355X."""
import argparse
import dataclasses
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from tracking_sweep import PRESETS  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--preset", choices=sorted(PRESETS), default="4x8")
    ap.add_argument("--ebno", type=float, default=21.0)
    ap.add_argument("--blocks", type=int, default=64)
    ap.add_argument("--chunk", type=int, default=64)
    ap.add_argument("--pilots", type=int, nargs="+", default=[1, 2, 4])
    ap.add_argument("--gammas", type=float, nargs="+", default=[0.0, 0.5, 0.8, 1.0])
    ap.add_argument("--grid", type=float, nargs="+", default=[1e-4, 1e-3, 1e-2])
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--commit", default=None, help="recorded in the JSON")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from esn_ofdm_mimo_amd import _lib
    from esn_ofdm_mimo_amd.montecarlo import DetectorSweep, LinkParams, baseline_tracking_point
    o = PRESETS[a.preset]
    base = LinkParams() if a.preset == "4x8" else dataclasses.replace(LinkParams.block_fading(2, 2, n_sub=64), m=2)
    F = o["frames"] or base.coherence_symbols
    params = dataclasses.replace(base, coherence_fixed=F, fading="jakes", f_d=o["fd"])
    out = a.out or os.path.join(ROOT, "profiles", f"gram_tracking_{a.preset}_{a.ebno:g}dB.json")
    mid = a.grid[len(a.grid) // 2]
    n_chunks = (a.blocks + a.chunk - 1) // a.chunk
    result = {"config": dict(preset=a.preset, n_t=params.n_t, n_r=params.n_r, n_sub=params.n_sub, bits_per_symbol=params.m,
                             channel=params.channel, ebno_db=a.ebno, f_d_hz=params.f_d, fd_tsym=params.fd_tsym,
                             n_reservoir=o["n_res"], state_noise=o["noise"], precision=o["precision"],
                             fit_precision=o["fit_precision"], grid=a.grid, gammas=a.gammas, pilots=a.pilots,
                             blocks=a.blocks, frames_per_block=F, chunk_blocks=a.chunk, seed=a.seed,
                             device=_lib.device_info()["arch"], commit=a.commit),
              "symbol": list(range(1, F + 1)), "runs": []}

    def save():
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            json.dump(result, f, indent=1)

    def run(label, timed=False, **kw):
        sw = DetectorSweep(params, n_reservoir=o["n_res"], noise=o["noise"], seed=a.seed, precision=o["precision"],
                           fit_precision=o["fit_precision"], symbol_counts=True, **kw)
        if timed:
            sw.run([a.ebno], min(a.chunk, a.blocks), chunk_blocks=a.chunk)      # warm-up: one chunk
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ber, counters = sw.run([a.ebno], a.blocks, chunk_blocks=a.chunk)
        torch.cuda.synchronize()
        seconds = time.perf_counter() - t0
        sc = sw.symbol_error_counts[a.ebno]
        rec = dict(label=label, ber=float(ber[0]), errors=int(counters[0, 0]), bits=int(counters[0, 1]),
                   flagged=int(sw.fits_repaired), ms_per_chunk=1e3 * seconds / n_chunks if timed else None,
                   ber_per_symbol=(sc[:, 0] / sc[:, 1]).tolist(),
                   **{k: (list(v) if isinstance(v, (list, tuple)) else v) for k, v in kw.items()})
        if sw.ridge_grid is not None:
            rec["choice_counts"] = sw.ridge_choice_counts[a.ebno].tolist()
        result["runs"].append(rec)
        save()
        print(f"{label:44s} BER {rec['ber']:.4e}  first {rec['ber_per_symbol'][0]:.3e}  last {rec['ber_per_symbol'][-1]:.3e}"
              + (f"  {rec['ms_per_chunk']:9.2f} ms per chunk" if timed else ""), flush=True)
        return sw

    sw = None
    for P in a.pilots:
        fit = dict(ridge_grid=a.grid) if P >= 2 else dict(ridge=mid)
        if P == 1:
            for lam in a.grid:
                sw = run(f"P=1 static lambda={lam:g}", solve_method="gram", n_pilots=1, ridge=lam)
        else:
            sw = run(f"P={P} static grid", solve_method="gram", n_pilots=P, **fit)
        for track in ("decisions", "genie"):
            for gamma in a.gammas:
                sw = run(f"P={P} {track} gamma={gamma:g}", timed=(gamma == a.gammas[-1]), solve_method="gram", n_pilots=P,
                         track=track, track_forget=gamma, **fit)
    # the shipped tracked chunk (one pilot, window 2) on the same frames, for the time and the BER it gave
    for track in ("decisions", "genie"):
        run(f"shipped window-2 {track} ridge={mid:g}", timed=True, solve_method="auto", track=track, track_window=2, ridge=mid)
    # the LS-MMSE baseline on the same frames
    for label, track in (("static", None), ("decisions", "decisions"), ("genie", "genie")):
        mm = baseline_tracking_point(sw.src, a.ebno, 0, a.blocks, F, track=track, window=1, chunk_blocks=a.chunk)
        result["runs"].append(dict(label="mmse " + label, detector="mmse", track=track, ber=mm["ber"],
                                   errors=int(mm["errors"].sum()), bits=int(mm["bits"].sum()),
                                   ber_per_symbol=(mm["errors"] / mm["bits"]).tolist()))
        save()
        print(f"{'mmse ' + label:44s} BER {mm['ber']:.4e}", flush=True)
    # the spread over blocks the statistical test needs is not kept here: it runs its own two sweeps
    print("wrote", out)


if __name__ == "__main__":
    main()
