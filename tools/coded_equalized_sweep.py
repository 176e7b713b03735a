#!/usr/bin/env python3
"""Uncoded and coded BER against Eb/No of the LS-MMSE detector and of a small ESN behind the LS-MMSE equaliser
(points.coded_equalized_point), each with the reference's flat LLRs (one decision-directed sigma^2 per frame) and with
LLRs weighted by the equaliser's SINR per subcarrier and stream, beside the coded comparison of the ESN that reads the
received signal (points.coded_ber_point), all on the same payloads and frames (one FrameSource seed, one code):

    ls-mmse flat | sinr            the MMSE leg of coded_equalized_point (flat: coded_ber_point's, bit for bit)
    eq-esn N flat | sinr           its ESN leg at N_res = 2 and 8, ridge 1e-5, float64, state noise 0.001
    esn 512                        coded_ber_point: DetectorSweep (fp16 kernels, state noise 0.001), flat LLRs

    python tools/coded_equalized_sweep.py [--blocks 256] [--ebno 0:30:3] [--extra 10.5,13.5] [--n-res 2,8]
                                          [--out file.json]

4x8, TDL-B, N = 128, 16-QAM (LinkParams()), 75 frames per block, code (512, .) of LdpcCode(512, 4, 8, seed=11);
calibration on the first 30 % of the blocks, decoding on the rest.  Writes profiles/coded_equalized_4x8.json unless
--out is given.  Needs an MI355X."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=256)
    ap.add_argument("--ebno", default="0:30:3", help="first:last:step in dB")
    ap.add_argument("--extra", default="10.5,13.5", help="further Eb/No points in dB, comma separated")
    ap.add_argument("--n-res", default="2,8", help="reservoir sizes behind the equaliser, comma separated")
    ap.add_argument("--ridge", type=float, default=1e-5)
    ap.add_argument("--esn-units", type=int, default=512, help="the units of the ESN beside the equaliser (0: leave it out)")
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--payload-seed", type=int, default=3)
    ap.add_argument("--commit", default=None, help="recorded in the JSON")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from esn_ofdm_mimo_amd import _lib
    from esn_ofdm_mimo_amd.coded import LdpcCode
    from esn_ofdm_mimo_amd.montecarlo import (DetectorSweep, FrameSource, LinkParams, coded_ber_point,
                                              coded_equalized_point)
    lo, hi, step = (float(v) for v in a.ebno.split(":"))
    points = [lo + i * step for i in range(int(round((hi - lo) / step)) + 1)]
    points = sorted(set(points + [float(v) for v in a.extra.split(",") if v]))
    sizes = [int(v) for v in a.n_res.split(",")]
    prm = LinkParams()
    F = prm.coherence_symbols
    src = FrameSource(prm, seed=a.seed)
    code = LdpcCode(prm.n_sub * prm.m, 4, 8, seed=11)
    rows = {}                                                 # label -> dict(uncoded=[...], coded=[...], ...)

    def put(label, si, uncoded, coded, **more):
        r = rows.setdefault(label, dict(label=label, uncoded=[None] * len(points), coded=[None] * len(points), **more))
        r["uncoded"][si], r["coded"][si] = float(uncoded), float(coded)

    out = a.out or os.path.join(ROOT, "profiles", "coded_equalized_4x8.json")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)

    def dump(done):
        """The file as it stands after `done` Eb/No points (the rest null): a run cut short leaves what it measured."""
        n_cal = max(1, int(round(0.3 * a.blocks)))
        result = {"config": dict(n_t=prm.n_t, n_r=prm.n_r, n_sub=prm.n_sub, bits_per_symbol=prm.m, channel=prm.channel,
                                 blocks=a.blocks, frames_per_block=F, calibration_blocks=n_cal,
                                 decoded_blocks=a.blocks - n_cal, code=dict(n=code.n, k=code.k, d_v=4, d_c=8, seed=11),
                                 seed=a.seed, payload_seed=a.payload_seed, state_noise=0.001, delay_behind_equaliser=0,
                                 kernels="eq-esn: float64 throughout; esn: fp16 predict, fp16 harvest + float64 solve",
                                 device=_lib.device_info()["arch"], commit=a.commit, points_done=done),
                  "ebno_db": points, "curves": list(rows.values())}
        with open(out, "w") as f:
            json.dump(result, f, indent=1)

    sw = DetectorSweep(prm, n_reservoir=a.esn_units, noise=0.001, seed=a.seed, precision="f16", fit_precision="f16") \
        if a.esn_units else None
    t0 = time.time()
    for si, eb in enumerate(points):
        for n in sizes:
            for mode in ("flat", "sinr"):
                r = coded_equalized_point(src, code, eb, si, a.blocks, llr=mode, n_reservoir=n, ridge=a.ridge,
                                          frames_per_block=F, seed=a.payload_seed)
                put(f"eq-esn {n} {mode}", si, r["ESN_uncoded"], r["ESN_coded"], llr=mode, n_reservoir=n, ridge=a.ridge)
                if n == sizes[0]:
                    put(f"ls-mmse {mode}", si, r["MMSE_uncoded"], r["MMSE_coded"], llr=mode)
        if sw is not None:
            r = coded_ber_point(sw, code, eb, si, a.blocks, frames_per_block=F, seed=a.payload_seed)
            put(f"esn {a.esn_units}", si, r["ESN_uncoded"], r["ESN_coded"], llr="flat", n_reservoir=a.esn_units)
        print(f"Eb/No {eb:5.1f} dB ({time.time() - t0:6.0f} s): " + "  ".join(
            f"{k} {v['uncoded'][si]:.4f}/{v['coded'][si]:.5f}" for k, v in rows.items()), flush=True)
        dump(si + 1)
    print("wrote", out)


if __name__ == "__main__":
    main()
