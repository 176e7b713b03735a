#!/usr/bin/env python3
"""BER against Eb/No of the amplifier-aware LS-MMSE baseline (points.dcc_point: decision-aided cancellation of the
transmit amplifier's distortion) beside the equaliser it extends and the small ESN behind that equaliser, all on the same
frames (one FrameSource seed), with the amplifier at the recipe's clip level and driven harder:

    ls-mmse                       esn_mmse_detect_count on the pilot's channel estimate (pass 0 of dcc_point)
    dcc 1 / 2 / 3                 the bit errors after 1, 2 and 3 cancellation passes (one dcc_point at n_iter = 3: pass it
                                  of a longer run is the last pass of a shorter one)
    eq-esn 2 / 8                  equalized_esn_point at N_res = 2 and 8, ridge 1e-5, float64
    ... clip 0                    the same rows with clip_db = 0
    dcc 2 a_clip +1 dB / -1 dB    two passes with the detector told a clip level 1 dB off (clip_db of the recipe)

    python tools/dcc_sweep.py [--blocks 256] [--ebno 0:30:3] [--n-res 2,8] [--ridge 1e-5] [--out file.json]

4x8, TDL-B, N = 128, 16-QAM (LinkParams()), 75 frames per block.  Writes profiles/dcc_sweep_4x8.json unless --out is
given.  Needs an MI355X."""
import argparse
import dataclasses
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=256)
    ap.add_argument("--ebno", default="0:30:3", help="first:last:step in dB")
    ap.add_argument("--n-res", default="2,8", help="reservoir sizes behind the equaliser, comma separated")
    ap.add_argument("--ridge", type=float, default=1e-5)
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--commit", default=None, help="recorded in the JSON")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from esn_ofdm_mimo_amd import _lib
    from esn_ofdm_mimo_amd.montecarlo import FrameSource, LinkParams, dcc_point, equalized_esn_point
    lo, hi, step = (float(v) for v in a.ebno.split(":"))
    points = [lo + i * step for i in range(int(round((hi - lo) / step)) + 1)]
    sizes = [int(v) for v in a.n_res.split(",")]
    base = LinkParams()
    F = base.coherence_symbols
    curves = []

    def add(label, ber, **more):
        curves.append(dict(label=label, ber=[float(v) for v in ber], **more))
        print(f"{label:30s} " + " ".join(f"{v:.5f}" for v in ber), flush=True)

    for clip in (base.clip_db, 0.0):
        src = FrameSource(dataclasses.replace(base, clip_db=clip), seed=a.seed)
        tag = "" if clip == base.clip_db else " clip 0"
        rows = [[] for _ in range(a.passes + 1)]
        for si, eb in enumerate(points):
            _, nb, it = dcc_point(src, eb, si, a.blocks, n_iter=a.passes, frames_per_block=F)
            for k, e in enumerate(it.tolist()):
                rows[k].append(e / float(nb.sum()))
        add("ls-mmse" + tag, rows[0], clip_db=clip)
        for k in range(1, a.passes + 1):
            add(f"dcc {k}" + tag, rows[k], clip_db=clip, n_iter=k)
        for n in sizes:
            ber = []
            for si, eb in enumerate(points):
                e, nb = equalized_esn_point(src, eb, si, a.blocks, n_reservoir=n, ridge=a.ridge, frames_per_block=F)
                ber.append(float(e.sum()) / float(nb.sum()))
            add(f"eq-esn {n}" + tag, ber, clip_db=clip, ridge=a.ridge, n_reservoir=n)
        if clip == base.clip_db:
            for off in (1.0, -1.0):
                ber = []
                for si, eb in enumerate(points):
                    e, nb, _ = dcc_point(src, eb, si, a.blocks, n_iter=2, a_clip_db_error=off, frames_per_block=F)
                    ber.append(float(e.sum()) / float(nb.sum()))
                add(f"dcc 2 a_clip {off:+g} dB", ber, clip_db=clip, n_iter=2, a_clip_db_error=off)
    result = {"config": dict(preset="4x8", n_t=base.n_t, n_r=base.n_r, n_sub=base.n_sub, bits_per_symbol=base.m,
                             channel=base.channel, blocks=a.blocks, frames_per_block=F, seed=a.seed,
                             kernels="float64 throughout", state_noise=0.001, device=_lib.device_info()["arch"],
                             commit=a.commit),
              "ebno_db": points, "curves": curves}
    out = a.out or os.path.join(ROOT, "profiles", "dcc_sweep_4x8.json")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(result, f, indent=1)
    print("wrote", out)


if __name__ == "__main__":
    main()
