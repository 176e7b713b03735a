#!/usr/bin/env python3
"""Does re-fitting the read-out inside a coherence block help under Doppler?  For one configuration and one Eb/No, the
bit error rate of data symbol 1 .. F of a block (LinkParams.fading = "jakes") for three receivers on the same frames:

    static      the read-out fitted once, on the pilot (DetectorSweep(track=None): what every sweep did so far)
    decisions   re-fitted after every data symbol on the detector's own re-modulated decisions (track="decisions")
    genie       re-fitted on the true transmit signal (track="genie"): the bound, not a receiver

with the window (training sets per re-fit) given, and beside each the LS-MMSE baseline on the same frames treated the same
way (baseline_tracking_point: "mmse static" counts every symbol against the pilot estimate, "mmse decisions" / "mmse genie"
re-estimate the channel after every data symbol from the last --mmse-window symbols, esn_channel_track) -- six curves, so
a tracked ESN is never set against an untracked baseline.  Beside the curves: the wall time of a chunk of each mode (one warm-up
chunk, then the whole run timed with a device synchronisation at the end), so the price of tracking is on record.

    python tools/tracking_sweep.py [--preset 4x8|2x2] [--ebno 21] [--fd HZ] [--frames F] [--blocks 64] [--window 2] [--mmse-window 1]
                                   [--n-res N] [--precision P] [--fit-precision P] [--noise X] [--ridge LAMBDA]
                                   [--chunk 64] [--out file.json]

Presets (each option overrides its part): 4x8 = LinkParams() (TDL-B, N = 128, 16-QAM), N_res 512, f16 / f16, state noise
0.001, 25 Hz, F from the coherence rule at 100 Hz; 2x2 = exponential PDP, N = 64, QPSK, N_res 32, f32 predict and f64
fit, no state noise, 576.9 Hz (fd_tsym 0.02), F = 24.  Writes profiles/tracking_sweep_<preset>_<ebno>dB[_ridge<l>].json
unless --out is given.  Needs an MI355X."""
import argparse
import dataclasses
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PRESETS = {"4x8": dict(n_res=512, precision="f16", fit_precision="f16", noise=0.001, fd=25.0, frames=0),
           "2x2": dict(n_res=32, precision="f32", fit_precision="f64", noise=0.0, fd=576.9, frames=24)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--preset", choices=sorted(PRESETS), default="4x8")
    ap.add_argument("--ebno", type=float, default=21.0)
    ap.add_argument("--fd", type=float, default=None, help="Doppler frequency in Hz")
    ap.add_argument("--frames", type=int, default=None, help="data symbols per block (0: the coherence rule at 100 Hz)")
    ap.add_argument("--blocks", type=int, default=64)
    ap.add_argument("--window", type=int, default=2, help="training sets per re-fit (track_window)")
    ap.add_argument("--mmse-window", type=int, default=1, help="data symbols per channel re-estimate of the MMSE baseline")
    ap.add_argument("--n-res", type=int, default=None)
    ap.add_argument("--precision", default=None)
    ap.add_argument("--fit-precision", default=None)
    ap.add_argument("--noise", type=float, default=None)
    ap.add_argument("--ridge", type=float, default=None, help="lambda of every fit (default: pinv)")
    ap.add_argument("--chunk", type=int, default=64, help="blocks per launch group")
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--commit", default=None, help="recorded in the JSON")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from esn_ofdm_mimo_amd import _lib
    from esn_ofdm_mimo_amd.montecarlo import DetectorSweep, LinkParams, baseline_tracking_point
    o = dict(PRESETS[a.preset])
    for k in o:
        if getattr(a, k) is not None:
            o[k] = getattr(a, k)
    if a.preset == "4x8":
        base = LinkParams()
    else:
        base = dataclasses.replace(LinkParams.block_fading(2, 2, n_sub=64), m=2)
    F = o["frames"] or base.coherence_symbols
    params = dataclasses.replace(base, coherence_fixed=F, fading="jakes", f_d=o["fd"])
    tag = "" if a.ridge is None else f"_ridge{a.ridge:g}"
    out = a.out or os.path.join(ROOT, "profiles", f"tracking_sweep_{a.preset}_{a.ebno:g}dB{tag}.json")
    result = {"config": dict(preset=a.preset, n_t=params.n_t, n_r=params.n_r, n_sub=params.n_sub, bits_per_symbol=params.m,
                             channel=params.channel, ebno_db=a.ebno, f_d_hz=params.f_d, fd_tsym=params.fd_tsym,
                             n_reservoir=o["n_res"], state_noise=o["noise"], precision=o["precision"],
                             fit_precision=o["fit_precision"], ridge=a.ridge, track_window=a.window, blocks=a.blocks,
                             frames_per_block=F, chunk_blocks=a.chunk, seed=a.seed, device=_lib.device_info()["arch"],
                             commit=a.commit),
              "symbol": list(range(1, F + 1)), "curves": []}
    n_chunks = (a.blocks + a.chunk - 1) // a.chunk
    for label, track in (("static", None), ("decisions", "decisions"), ("genie", "genie")):
        sw = DetectorSweep(params, n_reservoir=o["n_res"], noise=o["noise"], seed=a.seed, precision=o["precision"],
                           fit_precision=o["fit_precision"], ridge=a.ridge, symbol_counts=True, track=track,
                           track_window=a.window)
        sw.run([a.ebno], min(a.chunk, a.blocks), chunk_blocks=a.chunk)          # warm-up: one chunk
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ber, counters = sw.run([a.ebno], a.blocks, chunk_blocks=a.chunk)
        torch.cuda.synchronize()
        seconds = time.perf_counter() - t0
        sc = sw.symbol_error_counts[a.ebno]
        curve = dict(label=label, track=track, ber=float(ber[0]), errors=int(counters[0, 0]), bits=int(counters[0, 1]),
                     fits_repaired=int(sw.fits_repaired), ms_per_chunk=1e3 * seconds / n_chunks,
                     ber_per_symbol=(sc[:, 0] / sc[:, 1]).tolist())
        result["curves"].append(curve)
        pick = sorted({0, F // 4, F // 2, F - 1})
        print(f"{label:10s} BER {curve['ber']:.4e}  {curve['ms_per_chunk']:9.2f} ms per chunk of {min(a.chunk, a.blocks)} "
              f"blocks   per symbol " + "  ".join(f"s={s + 1}: {curve['ber_per_symbol'][s]:.3e}" for s in pick))
        # the LS-MMSE baseline over the same frames (the sweep's FrameSource, Eb/No index 0, blocks 0 ..), tracked the
        # same way: its channel estimate re-made after every data symbol from the last --mmse-window symbols
        kw = dict(track=track, window=a.mmse_window, chunk_blocks=a.chunk)
        baseline_tracking_point(sw.src, a.ebno, 0, min(a.chunk, a.blocks), F, **kw)              # warm-up: one chunk
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        mm = baseline_tracking_point(sw.src, a.ebno, 0, a.blocks, F, **kw)
        torch.cuda.synchronize()
        seconds = time.perf_counter() - t0
        curve = dict(label="mmse " + label, track=track, detector="mmse", window=a.mmse_window, ber=mm["ber"],
                     errors=int(mm["errors"].sum()), bits=int(mm["bits"].sum()), estimates_flagged=mm["failed"],
                     ms_per_chunk=1e3 * seconds / n_chunks, ber_per_symbol=(mm["errors"] / mm["bits"]).tolist())
        result["curves"].append(curve)
        print(f"{curve['label']:15s} BER {curve['ber']:.4e}  {curve['ms_per_chunk']:9.2f} ms per chunk   per symbol "
              + "  ".join(f"s={s + 1}: {curve['ber_per_symbol'][s]:.3e}" for s in pick))
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(result, f, indent=1)
    print("wrote", out)


if __name__ == "__main__":
    main()
