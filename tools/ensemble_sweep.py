#!/usr/bin/env python3
"""BER against Eb/No of reservoir ensembles (points.ensemble_point: K small ESNs per block, each fitted on the block's one
pilot, outputs averaged before the FFT) beside one ESN, the windowed ELM and the LS-MMSE baseline, all on the same frames
(one FrameSource seed), for every output delay of --delay:

    esn [ridge l]             DetectorSweep (--n-res units, fp16 kernels, state noise 0.001), pinv and --ridge
    ens KxN [ridge l]         ensemble_point for every pair of --pairs, pinv and --ridge, fp16 kernels
    ens KxN member k          with --member-counts: each member's own BER at --ridge, from the same launches
    elm g=0.05 ridge l        points.elm_point (512 hidden units, window 8), the best learned comparator at one pilot
    ls-mmse                   baseline_tracking_point(track=None)

    python tools/ensemble_sweep.py [--blocks 256] [--ebno 0:30:3] [--pairs 2x256,4x256,8x256] [--n-res 512]
                                   [--ridge 1e-3] [--delay -1,1] [--member-counts] [--out file.json]

--delay d sets LinkParams.delay_fixed (-1: the reference's (min + max) // 2 = 3); several values give several sets of
curves in the one file.  4x8, TDL-B, N = 128, 16-QAM.  Writes profiles/ensemble_sweep_4x8.json unless --out is given.
Needs an MI355X."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=256)
    ap.add_argument("--ebno", default="0:30:3", help="first:last:step in dB")
    ap.add_argument("--pairs", default="2x256,4x256,8x256", help="K x N_res, comma separated")
    ap.add_argument("--n-res", type=int, default=512, help="the single ESN's units")
    ap.add_argument("--ridge", type=float, default=1e-3)
    ap.add_argument("--delay", default="-1", help="delay_fixed values, comma separated; -1 = the reference's")
    ap.add_argument("--member-counts", action="store_true")
    ap.add_argument("--no-elm", action="store_true")
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--commit", default=None, help="recorded in the JSON")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from esn_ofdm_mimo_amd import _lib
    from esn_ofdm_mimo_amd.montecarlo import (DetectorSweep, LinkParams, baseline_tracking_point, elm_point,
                                              ensemble_point)
    lo, hi, step = (float(v) for v in a.ebno.split(":"))
    points = [lo + i * step for i in range(int(round((hi - lo) / step)) + 1)]
    pairs = [tuple(int(v) for v in pr.split("x")) for pr in a.pairs.split(",")]
    curves = []
    params = None
    for delay in (int(v) for v in a.delay.split(",")):
        params = LinkParams(delay_fixed=delay)
        F = params.coherence_symbols

        def add(label, ber, **more):
            curves.append(dict(label=label, delay=params.delay, ber=[float(v) for v in ber], **more))
            print(f"d={params.delay} {label:26s} " + " ".join(f"{v:.4f}" for v in ber), flush=True)

        src = None
        for ridge in (None, a.ridge):
            sw = DetectorSweep(params, n_reservoir=a.n_res, noise=0.001, seed=a.seed, precision="f16", fit_precision="f16",
                               ridge=ridge)
            ber, _ = sw.run(points, a.blocks, frames_per_block=F)
            add(f"esn {a.n_res}" + ("" if ridge is None else f" ridge {ridge:g}"), ber, ridge=ridge, n_members=1,
                n_reservoir=a.n_res, fits_repaired=int(sw.fits_repaired))
            src = sw.src
        for K, n in pairs:
            for ridge in (None, a.ridge):
                want_members = a.member_counts and ridge is not None
                ber, mber = [], []
                for si, eb in enumerate(points):
                    out = ensemble_point(src, eb, si, a.blocks, n_members=K, n_reservoir=n, precision="f16",
                                         fit_precision="f16", ridge=ridge, frames_per_block=F, member_counts=want_members)
                    ber.append(float(out[0].sum()) / float(out[1].sum()))
                    if want_members:
                        mber.append((out[2].sum(dim=0).double() / float(out[1].sum())).tolist())
                label = f"ens {K}x{n}" + ("" if ridge is None else f" ridge {ridge:g}")
                add(label, ber, ridge=ridge, n_members=K, n_reservoir=n)
                for k in range(K if want_members else 0):
                    add(f"ens {K}x{n} member {k}", [row[k] for row in mber], ridge=ridge, n_members=K, n_reservoir=n,
                        member=k)
        if not a.no_elm:
            ber = []
            for si, eb in enumerate(points):
                e, nb = elm_point(src, eb, si, a.blocks, n_hidden=512, window=8, gain=0.05, ridge=a.ridge, seed=a.seed,
                                  frames_per_block=F)
                ber.append(float(e.sum()) / float(nb.sum()))
            add(f"elm g=0.05 ridge {a.ridge:g}", ber, ridge=a.ridge)
        add("ls-mmse", [baseline_tracking_point(src, eb, si, a.blocks, F)["ber"] for si, eb in enumerate(points)])
    result = {"config": dict(n_t=params.n_t, n_r=params.n_r, n_sub=params.n_sub, bits_per_symbol=params.m,
                             channel=params.channel, blocks=a.blocks, frames_per_block=params.coherence_symbols,
                             seed=a.seed, kernels="fp16 predict, fp16 harvest + float64 solve", state_noise=0.001,
                             device=_lib.device_info()["arch"], commit=a.commit),
              "ebno_db": points, "curves": curves}
    out = a.out or os.path.join(ROOT, "profiles", "ensemble_sweep_4x8.json")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(result, f, indent=1)
    print("wrote", out)


if __name__ == "__main__":
    main()
