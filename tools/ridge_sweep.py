#!/usr/bin/env python3
"""BER against the ridge parameter lambda of the read-out fit (ReservoirBank.solve(ridge=)), so that a user can choose
lambda for one configuration: 4x8 TDL-B, N = 128, 16-QAM (LinkParams()), one reservoir size, a few Eb/No points.

Per chunk of coherence blocks the frames are generated once and the pilots harvested once; all lambdas are solved in
ONE launch ([G, L] ridge); then per lambda set_readout -> predict -> detect on the same data frames.  The pinv column
is today's fit (the existing entry points) on the same harvest.  pinv stays the default and the reference-parity
mode; ridge is an extension the reference does not have.

    python tools/ridge_sweep.py [--ebno 6,12,21] [--lambdas 0,1e-4,3e-4,1e-3,3e-3,1e-2] [--blocks 256] [--n-res 512]
                                [--precision f16] [--fit-precision f16] [--out file.json] [--loo]

--loo adds the column "LOO choice": per block the lambda (among the positive --lambdas) with the smallest leave-one-out
score of the block's own pilot (ReservoirBank.solve(ridge_grid=)), detected on the same frames as the fixed-lambda
columns, and the histogram of the choices.  Without --out it then writes profiles/ridge_sweep_nres<N>_loo.json.
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
    ap.add_argument("--ebno", default="6,12,21")
    ap.add_argument("--lambdas", default="0,1e-4,3e-4,1e-3,3e-3,1e-2")
    ap.add_argument("--blocks", type=int, default=256)
    ap.add_argument("--n-res", type=int, default=512)
    ap.add_argument("--precision", default="f16")
    ap.add_argument("--fit-precision", default="f16")
    ap.add_argument("--frames", type=int, default=0, help="data frames per block (0: the coherence time)")
    ap.add_argument("--chunk", type=int, default=256, help="blocks per launch")
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--commit", default=None, help="recorded in the JSON")
    ap.add_argument("--out", default=None)
    ap.add_argument("--loo", action="store_true", help="add the leave-one-out choice column and its histogram")
    a = ap.parse_args()
    import torch
    from esn_ofdm_mimo_amd import _lib
    from esn_ofdm_mimo_amd.montecarlo import DetectorSweep, LinkParams
    ebnos = [float(x) for x in a.ebno.split(",")]
    lams = [float(x) for x in a.lambdas.split(",")]
    grid = [lam for lam in lams if lam > 0.0]                   # (lambda = 0 is the pinv fit: no LOO score at n <= c)
    if a.loo and not a.out:
        a.out = os.path.join(ROOT, "profiles", f"ridge_sweep_nres{a.n_res}_loo.json")
    prm = LinkParams()
    F = a.frames or prm.coherence_symbols
    sw = DetectorSweep(prm, n_reservoir=a.n_res, noise=0.001, seed=a.seed, precision=a.precision,
                       fit_precision=a.fit_precision)
    bank, dev = sw.bank, sw.device
    t0 = time.perf_counter()
    result = {"config": dict(n_t=prm.n_t, n_r=prm.n_r, n_sub=prm.n_sub, bits_per_symbol=prm.m, channel=prm.channel,
                             n_reservoir=a.n_res, state_noise=0.001, precision=a.precision,
                             fit_precision=a.fit_precision, blocks=a.blocks, frames_per_block=F, seed=a.seed,
                             reservoirs="shared", device=_lib.device_info()["arch"], commit=a.commit),
              "lambdas": lams, "ebno_db": ebnos, "ber": {}, "ber_pinv": {}, "fits_repaired": {}, "bits": {}}
    if a.loo:
        result.update(loo_grid=grid, ber_loo={}, loo_choice_counts={})
    for si, ebno in enumerate(ebnos):
        ncol = len(lams) + 1 + int(a.loo)
        err = torch.zeros(ncol, dtype=torch.int64, device=dev)          # [pinv, lambda 0, lambda 1, ..., LOO choice]
        nbits = torch.zeros(ncol, dtype=torch.int64, device=dev)
        picks = torch.zeros(len(grid), dtype=torch.int64, device=dev)
        repaired = 0
        for b0 in range(0, a.blocks, a.chunk):
            g = min(a.chunk, a.blocks - b0)
            data = sw.src.blocks_fast(ebno, si, b0, g, F)
            sw.set_snr(ebno, g)
            E = sw.train(data["pilot_y"], data["pilot_x"], seed=sw.stream_seed(si, 0), group_offset=b0)   # pinv fit
            repaired += sw.repair_fit(E)
            readouts = [bank.W_out]
            U, D, tr = sw.fit_io
            ridge = torch.tensor(lams, dtype=torch.float64, device=dev).expand(g, len(lams)).contiguous()
            W, st = bank.solve(E, D, tr, method=sw.solve_method, ridge=ridge)    # every lambda, one launch
            repaired += bank.resolve_failed(E, D, tr, W, st, ridge=ridge)
            if int(st.ne(0).sum().item()):
                raise RuntimeError(f"ridge solve left status {st.unique().tolist()} at Eb/No {ebno}")
            readouts += [W[:, l] for l in range(len(lams))]
            if a.loo:
                Wl, stl = bank.solve(E, D, tr, ridge_grid=grid)
                ch = bank.last_ridge_choice
                picks += torch.bincount(ch.clamp(min=0).long(), weights=ch.ge(0).double(),
                                        minlength=len(grid)).to(torch.int64)
                repaired += bank.resolve_failed(E, D, tr, Wl, stl, ridge_grid=grid)
                readouts.append(Wl)
            for k, w in enumerate(readouts):
                bank.set_readout(w)
                e = torch.zeros(g, dtype=torch.int64, device=dev)
                n = torch.zeros(g, dtype=torch.int64, device=dev)
                sw.detect(data["data_y"], data["data_bits"], F, e, n, seed=sw.stream_seed(si, 1), group_offset=b0)
                err[k] += e.sum()
                nbits[k] += n.sum()
        ber = (err.double() / nbits.double()).cpu().tolist()
        key = f"{ebno:g}"
        result["ber_pinv"][key] = ber[0]
        result["ber"][key] = {f"{lam:g}": ber[1 + l] for l, lam in enumerate(lams)}
        result["fits_repaired"][key] = repaired
        result["bits"][key] = int(nbits[0].item())
        line = f"Eb/No {ebno:5.1f} dB  pinv {ber[0]:.5f}   " + \
            "  ".join(f"{lam:g}: {ber[1 + l]:.5f}" for l, lam in enumerate(lams))
        if a.loo:
            counts = picks.cpu().tolist()
            result["ber_loo"][key] = ber[-1]
            result["loo_choice_counts"][key] = {f"{lam:g}": c for lam, c in zip(grid, counts)}
            line += f"   LOO choice: {ber[-1]:.5f}  picks " + " ".join(f"{lam:g}:{c}" for lam, c in zip(grid, counts))
        print(line, flush=True)
    result["seconds"] = round(time.perf_counter() - t0, 1)
    text = json.dumps(result, indent=1)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    else:
        print(text)


if __name__ == "__main__":
    main()
