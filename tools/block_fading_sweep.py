#!/usr/bin/env python3
"""The block-fading drivers' sweep on the GPU (OFDM_{SISO,SIMO_1-2,MIMO_2-2}_NBF_LDPC.py,
Demo_MIMO_4x8_ChannelRank_TrainSNR_LDPC_fast.py): per Eb/No the five uncoded and five coded BER holders (ESN matched, ESN
trained at a fixed Eb/No, LS-ZF, MMSE, Perfect-ZF) and the drivers' second output, the channel record from the
per-subcarrier SVD of the true channel (OFDM_MIMO_2-2_NBF_LDPC.py:369-385,515-521), in the shape the drivers pickle
(:526-532).  Writes one JSON:

    {"config": {...}, "EBN0": [...], "BER_ESN_matched": [...], ..., "BERC_PerfectZF": [...],
     "channel": {"EBN0": [...], "capacity_bits_per_sc": [...], "frac_rank_ge_full": [...],
                 "cond_number": {"p50": [...], "p90": [...]}}}

    python tools/block_fading_sweep.py --nt 2 --nr 2 --n-sub 512 --blocks 512 --ebno 0,6,12,18,24 --out sweep.json
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DETECTORS = ("ESN_matched", "ESN_trainFixed", "LS_ZF", "MMSE", "PerfectZF")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--nt", type=int, default=2)
    ap.add_argument("--nr", type=int, default=2)
    ap.add_argument("--n-sub", type=int, default=512)
    ap.add_argument("--n-res", type=int, default=100)
    ap.add_argument("--blocks", type=int, default=256, help="coherence blocks per Eb/No point")
    ap.add_argument("--ebno", default="0,3,6,9,12,15,18,21,24", help="comma-separated Eb/No list in dB")
    ap.add_argument("--precision", default="f16", choices=["f64", "f32", "f16", "bf16"])
    ap.add_argument("--train-ebno", type=float, default=12.0, help="Eb/No of the fixed-SNR ESN (TRAIN_EBNO_FIXED_DB)")
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    ebno = [float(x) for x in a.ebno.split(",") if x.strip()]
    from esn_ofdm_mimo_amd.coded import LdpcCode
    from esn_ofdm_mimo_amd.montecarlo import DetectorSweep, LinkParams, block_fading_point
    prm = LinkParams.block_fading(a.nt, a.nr, a.n_sub)
    fitp = a.precision if a.precision in ("f16", "bf16") else "f32"
    kw = dict(n_reservoir=a.n_res, noise=0.001, seed=a.seed, precision=a.precision, fit_precision=fitp)
    sw = DetectorSweep(prm, **kw)
    sw_fixed = DetectorSweep(prm, train_ebno=a.train_ebno, **kw)
    code = LdpcCode(prm.n_sub * prm.m, 4, 8, seed=11)
    out = {"config": dict(n_t=a.nt, n_r=a.nr, n_sub=a.n_sub, n_res=a.n_res, blocks=a.blocks, precision=a.precision,
                          train_ebno=a.train_ebno, seed=a.seed, symbols_per_block=prm.coherence_symbols),
           "EBN0": ebno}
    for d in DETECTORS:
        out["BER_" + d], out["BERC_" + d] = [], []
    chan = {"EBN0": ebno, "capacity_bits_per_sc": [], "frac_rank_ge_full": [], "cond_number": {"p50": [], "p90": []}}
    t0 = time.perf_counter()
    for si, eb in enumerate(ebno):
        r = block_fading_point(sw, code, eb, si, a.blocks, fixed_sweep=sw_fixed, seed=a.seed, channel_metrics=True)
        for d in DETECTORS:
            out["BER_" + d].append(r["BER_" + d])
            out["BERC_" + d].append(r["BERC_" + d])
        chan["capacity_bits_per_sc"].append(r["capacity_bits_per_sc"])
        chan["frac_rank_ge_full"].append(r["frac_rank_ge_full"])
        chan["cond_number"]["p50"].append(r["cond_p50"])
        chan["cond_number"]["p90"].append(r["cond_p90"])
        print(f"Eb/No {eb:5.1f} dB  " + "  ".join(f"{d} {r['BER_' + d]:.5f}/{r['BERC_' + d]:.5f}" for d in DETECTORS) +
              f"   cap {r['capacity_bits_per_sc']:.3f} b/sc  full rank {r['frac_rank_ge_full']:.3f}  cond p50 "
              f"{r['cond_p50']:.2f} p90 {r['cond_p90']:.2f}", flush=True)
    out["channel"] = chan
    print(f"{len(ebno)} points x {a.blocks} blocks in {time.perf_counter() - t0:.1f} s")
    text = json.dumps(out, indent=1)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    else:
        print(text)


if __name__ == "__main__":
    main()
