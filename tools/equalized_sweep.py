#!/usr/bin/env python3
"""BER against Eb/No of a small ESN behind the LS-MMSE equaliser (points.equalized_esn_point: the equalised signal back
in the time domain is the reservoir's input) beside the ESN that reads the received signal and the equaliser itself, all
on the same frames (one FrameSource seed):

    esn 512 ridge 0.001           DetectorSweep (fp16 kernels, state noise 0.001): the one-pilot ESN of the README
    ls-mmse                       esn_mmse_detect_count on the pilot's channel estimate (the point's want_mmse counters)
    eq-esn N [ridge 1e-05]        equalized_esn_point at N_res = 2 / 8 / 32 / 128, pinv and ridge 1e-5, float64
    ... clip 0                    ls-mmse and the eq-esn rows again with the amplifier driven harder (clip_db = 0)

    python tools/equalized_sweep.py [--preset 4x8|2x2] [--blocks 256] [--ebno 0:30:3] [--n-res 2,8,32,128]
                                    [--ridge 1e-5] [--out file.json]

--preset 4x8: TDL-B, N = 128, 16-QAM (LinkParams()); 2x2: the block-fading drivers' exponential-PDP link, N = 512
(LinkParams.block_fading()).  Writes profiles/equalized_sweep_<preset>.json unless --out is given.  Needs an MI355X."""
import argparse
import dataclasses
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--preset", choices=("4x8", "2x2"), default="4x8")
    ap.add_argument("--blocks", type=int, default=256)
    ap.add_argument("--ebno", default="0:30:3", help="first:last:step in dB")
    ap.add_argument("--n-res", default="2,8,32,128", help="reservoir sizes behind the equaliser, comma separated")
    ap.add_argument("--ridge", type=float, default=1e-5)
    ap.add_argument("--esn-units", type=int, default=512, help="the units of the ESN beside the equaliser")
    ap.add_argument("--esn-ridge", type=float, default=1e-3)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--commit", default=None, help="recorded in the JSON")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from esn_ofdm_mimo_amd import _lib
    from esn_ofdm_mimo_amd.montecarlo import DetectorSweep, FrameSource, LinkParams, equalized_esn_point
    lo, hi, step = (float(v) for v in a.ebno.split(":"))
    points = [lo + i * step for i in range(int(round((hi - lo) / step)) + 1)]
    sizes = [int(v) for v in a.n_res.split(",")]
    base = LinkParams() if a.preset == "4x8" else LinkParams.block_fading()
    F = base.coherence_symbols
    curves = []

    def add(label, ber, **more):
        curves.append(dict(label=label, ber=[float(v) for v in ber], **more))
        print(f"{label:30s} " + " ".join(f"{v:.4f}" for v in ber), flush=True)

    sw = DetectorSweep(base, n_reservoir=a.esn_units, noise=0.001, seed=a.seed, precision="f16", fit_precision="f16",
                       ridge=a.esn_ridge)
    ber, _ = sw.run(points, a.blocks, frames_per_block=F)
    add(f"esn {a.esn_units} ridge {a.esn_ridge:g}", ber, clip_db=base.clip_db, ridge=a.esn_ridge, n_reservoir=a.esn_units,
        fits_repaired=int(sw.fits_repaired))
    for clip in (base.clip_db, 0.0):
        params = dataclasses.replace(base, clip_db=clip)
        src = sw.src if clip == base.clip_db else FrameSource(params, seed=a.seed)
        tag = "" if clip == base.clip_db else " clip 0"
        first = True                                          # the first row of a clip level brings the MMSE counters
        for n in sizes:
            for ridge in (None, a.ridge):
                ber, mmse = [], []
                for si, eb in enumerate(points):
                    out = equalized_esn_point(src, eb, si, a.blocks, n_reservoir=n, ridge=ridge, frames_per_block=F,
                                              want_mmse=first)
                    ber.append(float(out[0].sum()) / float(out[1].sum()))
                    if first:
                        mmse.append(float(out[2].sum()) / float(out[3].sum()))
                if first:
                    add("ls-mmse" + tag, mmse, clip_db=clip)
                    first = False
                add(f"eq-esn {n}" + ("" if ridge is None else f" ridge {ridge:g}") + tag, ber, clip_db=clip, ridge=ridge,
                    n_reservoir=n)
    result = {"config": dict(preset=a.preset, n_t=base.n_t, n_r=base.n_r, n_sub=base.n_sub, bits_per_symbol=base.m,
                             channel=base.channel, blocks=a.blocks, frames_per_block=F, seed=a.seed,
                             kernels="eq-esn: float64 throughout; esn: fp16 predict, fp16 harvest + float64 solve",
                             state_noise=0.001, delay_behind_equaliser=0, device=_lib.device_info()["arch"],
                             commit=a.commit),
              "ebno_db": points, "curves": curves}
    out = a.out or os.path.join(ROOT, "profiles", f"equalized_sweep_{a.preset}.json")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(result, f, indent=1)
    print("wrote", out)


if __name__ == "__main__":
    main()
