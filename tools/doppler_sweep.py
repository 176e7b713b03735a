#!/usr/bin/env python3
"""BER against the age of the pilot: for one preset and one Eb/No, the bit error rate of data symbol 1 .. F of a
coherence block for the ESN detector and for the LS-MMSE baseline, with the channel moving inside the block
(LinkParams.fading = "jakes", esn_gen_taps_doppler) at several Doppler frequencies -- 0 Hz included -- and the
block-fading curve (one tap set per block, the reference's assumption) beside them.

The ESN curve is DetectorSweep(symbol_counts=True).symbol_error_counts; the MMSE curve counts every data frame against
the block's pilot estimate H (esn_channel_estimate on the sparse LS pilot of symbol 0) expanded to one H per frame, in
chunks.  Frames are the same for both detectors (same seed, same counters).

    python tools/doppler_sweep.py [--preset 4x8|2x2] [--ebno 21] [--fd 0,25,50,100,200] [--blocks 256] [--frames 0]
                                  [--n-res 512] [--precision f16] [--fit-precision f16] [--chunk 64] [--out file.json]

Writes profiles/doppler_sweep_<preset>_<ebno>dB.json unless --out is given.  Needs an MI355X: no figure of this tool
exists until it has run on one."""
import argparse
import dataclasses
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--preset", choices=("4x8", "2x2"), default="4x8",
                    help="4x8: TDL-B, N = 128 (LinkParams()); 2x2: exponential PDP, N = 512 (LinkParams.block_fading)")
    ap.add_argument("--ebno", type=float, default=21.0)
    ap.add_argument("--fd", default="0,25,50,100,200", help="Doppler frequencies in Hz")
    ap.add_argument("--blocks", type=int, default=256)
    ap.add_argument("--frames", type=int, default=0, help="data symbols per block (0: the preset's coherence rule at 100 Hz)")
    ap.add_argument("--n-res", type=int, default=512)
    ap.add_argument("--precision", default="f16")
    ap.add_argument("--fit-precision", default="f16")
    ap.add_argument("--noise", type=float, default=0.001)
    ap.add_argument("--chunk", type=int, default=64, help="blocks per launch")
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--commit", default=None, help="recorded in the JSON")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    import torch
    from scipy.special import j0
    from esn_ofdm_mimo_amd import _lib
    from esn_ofdm_mimo_amd.montecarlo import DetectorSweep, LinkParams
    base = LinkParams() if a.preset == "4x8" else LinkParams.block_fading(2, 2)
    F = a.frames or base.coherence_symbols
    base = dataclasses.replace(base, coherence_fixed=F)
    fds = [float(x) for x in a.fd.split(",")]
    out = a.out or os.path.join(ROOT, "profiles", f"doppler_sweep_{a.preset}_{a.ebno:g}dB.json")
    result = {"config": dict(preset=a.preset, n_t=base.n_t, n_r=base.n_r, n_sub=base.n_sub, bits_per_symbol=base.m,
                             channel=base.channel, ebno_db=a.ebno, n_reservoir=a.n_res, state_noise=a.noise,
                             precision=a.precision, fit_precision=a.fit_precision, blocks=a.blocks, frames_per_block=F,
                             seed=a.seed, device=_lib.device_info()["arch"], commit=a.commit),
              "symbol": list(range(1, F + 1)), "curves": []}
    t0 = time.perf_counter()
    for label, params in [("block", base)] + [(f"jakes {fd:g} Hz", dataclasses.replace(base, fading="jakes", f_d=fd))
                                              for fd in fds]:
        sw = DetectorSweep(params, n_reservoir=a.n_res, noise=a.noise, seed=a.seed, precision=a.precision,
                           fit_precision=a.fit_precision, symbol_counts=True)
        ber, counters = sw.run([a.ebno], a.blocks, chunk_blocks=a.chunk)
        esn = sw.symbol_error_counts[a.ebno]
        src, dev = sw.src, sw.device
        mm = torch.zeros((F, 2), dtype=torch.int64, device=dev)
        for b0 in range(0, a.blocks, a.chunk):
            g = min(a.chunk, a.blocks - b0)
            d = src.blocks_fast(a.ebno, 0, b0, g, F, with_ls_pilot=True)
            H = src.estimate_channel(d["pilot_bits"], d["pilot_y_ls"], a.ebno)
            e, nb = src.mmse_detect_count(H.repeat_interleave(F, dim=0), d["data_y"], d["data_bits"], 1, a.ebno)
            mm += torch.stack([e.view(g, F).sum(dim=0), nb.view(g, F).sum(dim=0)], dim=1)
        mm = mm.cpu().numpy()
        curve = dict(label=label, fading=params.fading, f_d_hz=params.f_d if params.fading == "jakes" else None,
                     fd_tsym=params.fd_tsym if params.fading == "jakes" else None,
                     esn_ber=float(ber[0]), mmse_ber=float(mm[:, 0].sum() / mm[:, 1].sum()),
                     fits_repaired=int(sw.fits_repaired), bits_per_symbol_index=int(esn[0, 1]),
                     esn_ber_per_symbol=(esn[:, 0] / esn[:, 1]).tolist(), mmse_ber_per_symbol=(mm[:, 0] / mm[:, 1]).tolist())
        if params.fading == "jakes":      # what the model promises for the channel: J0(2 pi fd_tsym s) at data symbol s
            curve["j0_per_symbol"] = j0(2 * np.pi * params.fd_tsym * np.arange(1, F + 1)).tolist()
        result["curves"].append(curve)
        pick = sorted({0, F // 4, F // 2, F - 1})
        print(f"{label:14s} ESN {curve['esn_ber']:.4e}  MMSE {curve['mmse_ber']:.4e}   per symbol "
              + "  ".join(f"s={s + 1}: {curve['esn_ber_per_symbol'][s]:.3e} / {curve['mmse_ber_per_symbol'][s]:.3e}"
                          for s in pick))
    result["seconds"] = time.perf_counter() - t0
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(result, f, indent=1)
    print("wrote", out)


if __name__ == "__main__":
    main()
