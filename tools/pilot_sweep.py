#!/usr/bin/env python3
"""BER against the number of pilot symbols per coherence block, P in {1, 2, 3, 4}: 4x8 TDL-B, N = 128,
16-QAM (LinkParams()), one reservoir size, a few Eb/No points, the same data frames for every cell.

Fit columns: pinv, each fixed lambda of --lambdas, and ridge_grid over those lambdas (P = 1: the leave-one-out choice on
the one pilot; P >= 2: the hold-out choice on the last pilot, ReservoirBank.fit_pilots), with the histogram of the chosen
candidates.  One LS-MMSE column whose channel is the mean of the P per-pilot estimates (FrameSource.estimate_channel on
each pilot's sparse pattern), so the baseline gets the same pilots.  Every cell carries its standard error over blocks
(the blocks are the independent units).

    python tools/pilot_sweep.py [--ebno 12,21] [--lambdas 1e-4,1e-3,1e-2] [--blocks 256] [--n-res 512] [--pilots 1,2,3,4]
                                [--precision f16] [--fit-precision f16] [--out profiles/pilot_sweep_4x8.json]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ebno", default="12,21")
    ap.add_argument("--lambdas", default="1e-4,1e-3,1e-2")
    ap.add_argument("--pilots", default="1,2,3,4")
    ap.add_argument("--blocks", type=int, default=256)
    ap.add_argument("--n-res", type=int, default=512)
    ap.add_argument("--precision", default="f16")
    ap.add_argument("--fit-precision", default="f16")
    ap.add_argument("--frames", type=int, default=12, help="data frames per block")
    ap.add_argument("--chunk", type=int, default=256, help="blocks per launch")
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--commit", default=None, help="recorded in the JSON")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pilot_sweep_4x8.json"))
    a = ap.parse_args()
    import torch
    from esn_ofdm_mimo_amd import _lib
    from esn_ofdm_mimo_amd.frames import complex_as_io
    from esn_ofdm_mimo_amd.montecarlo import DetectorSweep, LinkParams
    ebnos = [float(x) for x in a.ebno.split(",")]
    lams = [float(x) for x in a.lambdas.split(",")]
    pilots = [int(x) for x in a.pilots.split(",")]
    prm, F, Pmax = LinkParams(), a.frames, max(max(pilots), 2)          # (the `pilots_*` keys come with P >= 2)
    sw = DetectorSweep(prm, n_reservoir=a.n_res, noise=0.001, seed=a.seed, precision=a.precision,
                       fit_precision=a.fit_precision)
    bank, dev, src, d = sw.bank, sw.device, sw.src, prm.delay
    fits = [("pinv", {})] + [(f"{lam:g}", dict(ridge=lam)) for lam in lams] + [("ridge_grid", dict(ridge_grid=lams))]
    cols = [name for name, _ in fits] + ["ls_mmse"]
    t0 = time.perf_counter()
    result = {"config": dict(n_t=prm.n_t, n_r=prm.n_r, n_sub=prm.n_sub, bits_per_symbol=prm.m, channel=prm.channel,
                             n_reservoir=a.n_res, state_noise=0.001, precision=a.precision, fit_precision=a.fit_precision,
                             blocks=a.blocks, frames_per_block=F, seed=a.seed, reservoirs="shared",
                             device=_lib.device_info()["arch"], commit=a.commit),
              "lambdas": lams, "ebno_db": ebnos, "pilots": pilots, "ber": {}, "stderr_over_blocks": {},
              "choice_counts": {}, "fits_repaired": {}}
    for si, ebno in enumerate(ebnos):
        per_block = {(P, c): [] for P in pilots for c in cols}          # error counts per block, chunk by chunk
        picks = {P: torch.zeros(len(lams), dtype=torch.int64, device=dev) for P in pilots}
        repaired, bits_per_block = 0, F * prm.n_sub * prm.m * prm.n_t
        for b0 in range(0, a.blocks, a.chunk):
            g = min(a.chunk, a.blocks - b0)
            data = src.blocks_fast(ebno, si, b0, g, F, with_ls_pilot=True, n_pilots=Pmax)
            py, px, pb, pls = (data[k] for k in ("pilots_y", "pilots_x", "pilots_bits", "pilots_y_ls"))
            sw.set_snr(ebno, g)
            T = py.shape[2]
            U = torch.zeros((g, Pmax, T + d, sw.n_in), dtype=torch.float64, device=dev)
            D = torch.zeros((g, Pmax, T + d, sw.n_out), dtype=torch.float64, device=dev)
            U[:, :, :T] = complex_as_io(py)
            D[:, :, d:] = complex_as_io(px)
            seeds = [sw.stream_seed(si, 0)] + [sw.stream_seed(si, sw.PILOT_LEG0 + q) for q in range(1, Pmax)]
            H_p = [src.estimate_channel(pb[:, q].contiguous(), pls[:, q].contiguous(), ebno) for q in range(Pmax)]
            for P in pilots:
                rows = P * (T + d - prm.forget)
                chol = bank.chol_fits(rows, bank.n_reservoir + sw.n_in)
                e_dtype = "f32" if chol and a.fit_precision in ("f16", "bf16") else "f64"
                for name, kw in fits:
                    E = bank.fit_pilots(U[:, :P], D[:, :P], transient=prm.forget, precision=a.fit_precision,
                                        noise_mode="counter", seed=seeds[:P], method="auto", e_dtype=e_dtype,
                                        group_offset=b0, **kw)
                    if name == "ridge_grid":            # (before a repair: a block without a choice is in no bin)
                        ch = bank.last_ridge_choice
                        picks[P] += torch.bincount(ch.clamp(min=0).long(), weights=ch.ge(0).double(),
                                                   minlength=len(lams)).to(torch.int64)
                    n_bad = bank.resolve_failed(E, bank.fit_rows[1], 0, bank.W_out, bank.fit_status,
                                                ridge=kw.get("ridge"), ridge_grid=kw.get("ridge_grid"))
                    if n_bad:
                        repaired += n_bad
                        bank.set_readout(bank.W_out)
                    e = torch.zeros(g, dtype=torch.int64, device=dev)
                    n = torch.zeros(g, dtype=torch.int64, device=dev)
                    sw.detect(data["data_y"], data["data_bits"], F, e, n, seed=sw.stream_seed(si, 1), group_offset=b0)
                    per_block[P, name].append(e)
                H = torch.stack(H_p[:P]).mean(dim=0)
                e, _ = src.mmse_detect_count(H, data["data_y"], data["data_bits"], F, ebno)
                per_block[P, "ls_mmse"].append(e)
        key = f"{ebno:g}"
        result["ber"][key], result["stderr_over_blocks"][key], result["choice_counts"][key] = {}, {}, {}
        result["fits_repaired"][key] = repaired
        for P in pilots:
            ber, sem = {}, {}
            for c in cols:
                r = torch.cat(per_block[P, c]).double() / bits_per_block
                ber[c] = float(r.mean())
                sem[c] = float(r.std(unbiased=True) / len(r) ** 0.5) if len(r) > 1 else 0.0
            result["ber"][key][str(P)], result["stderr_over_blocks"][key][str(P)] = ber, sem
            result["choice_counts"][key][str(P)] = {f"{lam:g}": c for lam, c in zip(lams, picks[P].cpu().tolist())}
            print(f"Eb/No {ebno:5.1f} dB  P = {P}  " + "  ".join(f"{c}: {ber[c]:.5f} +- {sem[c]:.5f}" for c in cols) +
                  "   picks " + " ".join(f"{k}:{v}" for k, v in result["choice_counts"][key][str(P)].items()), flush=True)
    result["seconds"] = round(time.perf_counter() - t0, 1)
    with open(a.out, "w") as f:
        f.write(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
