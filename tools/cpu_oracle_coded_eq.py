#!/usr/bin/env python3
"""The coded leg behind the LS-MMSE equaliser on the NumPy oracle: info-bit BER after LDPC decoding of the LS-MMSE
detector and of a small ESN behind the equaliser, each with flat LLRs (one decision-directed sigma^2 per frame) and with
LLRs weighted by the equaliser's SINR per subcarrier and stream over the block's mean (tests/soft_ref.py) -- the CPU-side
record the device's coded_equalized_point is set beside.  A record, not a test: about a minute per Eb/No point and process.

    python tools/cpu_oracle_coded_eq.py [--ebno 9 10.5 12 13.5] [--blocks 16] [--frames 8] [--procs 8] [--out file.json]

4x8 / TDL-B / N = 128 / 16-QAM, N_res = 8, ridge 1e-5, state noise 1e-3; frames and estimator of oracle/, the chain of
tests/equalize_ref.py, code and BP decoder of oracle/ldpc_oracle.py ((512, .) from RandomState(5), 50 iterations).  Seeds
as equalize_ref.block_errors: frames RandomState(7000 + block), taps 1234 + int(ebno) + 75 block + 1, reservoir
RandomState(9000 + block); the bits drawn for a frame give the payload (their first k rows per stream), the code words
take their place on the air.  Calibration (fit_logreg_1d per bit position) on the first 5/16 of the blocks, decoding on
the rest.  Writes profiles/coded_equalized_oracle.json unless --out is given."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

LLR_CLIP, SNR_FOR_LDPC, MAXITER = 20.0, 1.0, 50


def one_thread():
    """Pool initialiser: one BLAS / OpenMP thread per worker, set before the worker first imports numpy."""
    for var in ("OMP_NUM_THREADS", "OPENBLAS_NUM_THREADS", "MKL_NUM_THREADS"):
        os.environ[var] = "1"


def make_code(n):
    import numpy as np
    from oracle import ldpc_oracle as lo
    H_sys, P, k, _ = lo.systematic_code(lo.gallager_parity_check(n, 4, 8, np.random.RandomState(5)))
    return H_sys, P, k


def one_block(job):
    """One coherence block: (u [F, n_t, k], bits [F, N m, n_t], X_mmse, X_esn [F, N, n_t], w, mu [N, n_t])."""
    ebno, block, frames, n_res, ridge = job
    import numpy as np
    import equalize_ref as qr
    import soft_ref as sr
    from oracle import baselines as bl
    from oracle import ldpc_oracle as lo
    from oracle.ofdm_frames import LinkConfig, channel, modulate, random_bits, tdlb_mimo_taps
    cfg = LinkConfig()
    _, P, k = make_code(cfg.n_sub * cfg.m)
    rs = np.random.RandomState(7000 + block)
    taps = tdlb_mimo_taps(cfg, 1234 + int(ebno) + block * 75 + 1)
    p_i = cfg.p_i(ebno)
    pilot = bl.pilot_frames(cfg, ebno, taps, rs)
    H = bl.estimate_channel(cfg, ebno, pilot["X_LS"], pilot["y_ls_cp"])
    esn = qr.make_esn(cfg.n_t, n_res, cfg.input_scaling(ebno), cfg.teacher_scale, ridge, noise=0.001,
                      random_state=np.random.RandomState(9000 + block))
    _, pilot_rows = qr.equalize_frame(pilot["y_cp"], H, p_i, cfg.no, cfg.cp, 0)
    us, bits, x_mm, rows = [], [], [], []
    for _ in range(frames):
        u = random_bits(cfg, rs)[:k].T.astype(np.uint8)                     # [n_t, k]
        cw = lo.encode(P, u).T.astype(np.int32)                             # [N m, n_t]
        _, _, x_pa = modulate(cw, cfg, ebno)
        X, r = qr.equalize_frame(channel(x_pa, taps, cfg, rs), H, p_i, cfg.no, cfg.cp, 0)
        us.append(u); bits.append(cw); x_mm.append(X); rows.append(r)
    x_esn, _ = qr.chain_block(esn, pilot_rows, pilot["x_cp"], rows, cfg.n_sub, cfg.cp, 0, p_i, cfg.m)
    w, mu, _ = sr.sinr_weights(H[None], np.array([p_i]), cfg.no)
    return np.stack(us), np.stack(bits), np.stack(x_mm), x_esn, w[0], mu[0]


def decode_leg(job):
    """Info-bit errors of one detector's LLRs [B, n_t, N m]: calibration on the first n_cal frames, BP on the rest."""
    llr, bits, u, n_cal, m = job
    import numpy as np
    from oracle import ldpc_oracle as lo
    H_sys, _, k = make_code(llr.shape[2])
    B, n_t, n = llr.shape
    per_bit = llr.reshape(B, n_t, -1, m)
    truth = bits.transpose(0, 2, 1).reshape(B, n_t, -1, m)
    ab = [lo.fit_logreg_1d(per_bit[:n_cal, :, :, b].reshape(-1), truth[:n_cal, :, :, b].reshape(-1).astype(float))
          for b in range(m)]
    a, b = np.array([v[0] for v in ab]), np.array([v[1] for v in ab])
    cal = -(a * per_bit[n_cal:] + b)
    yobs = 0.5 * np.clip(cal, -LLR_CLIP, LLR_CLIP).reshape(-1, n)
    x = lo.decode_bp(H_sys, yobs, SNR_FOR_LDPC, MAXITER)
    errs = int(np.sum(x[:, :k] != u[n_cal:].reshape(-1, k)))
    return errs, int(yobs.shape[0] * k), a.tolist(), b.tolist()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ebno", type=float, nargs="+", default=[9.0, 10.5, 12.0, 13.5])
    ap.add_argument("--blocks", type=int, default=16)
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--n-res", type=int, default=8)
    ap.add_argument("--ridge", type=float, default=1e-5)
    ap.add_argument("--procs", type=int, default=8)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import multiprocessing as mp
    import numpy as np
    import soft_ref as sr
    from oracle import esn_oracle as eo
    from oracle.ofdm_frames import LinkConfig
    cfg = LinkConfig()
    m, F = cfg.m, a.frames
    n_cal = max(1, int(round(5.0 / 16.0 * a.blocks))) * F
    const = eo.unit_qam(m)
    records = []
    out = a.out or os.path.join(ROOT, "profiles", "coded_equalized_oracle.json")
    with mp.get_context("spawn").Pool(a.procs, initializer=one_thread) as pool:
        for ebno in a.ebno:
            t0 = time.time()
            res = pool.map(one_block, [(ebno, b, F, a.n_res, a.ridge) for b in range(a.blocks)])
            u, bits, x_mm, x_esn = (np.concatenate([r[i] for r in res]) for i in range(4))
            w, mu = (np.stack([r[i] for r in res]) for i in (4, 5))
            ones = np.ones_like(w)
            rec = dict(ebno_db=ebno)
            jobs, names = [], []
            for det, X in (("mmse", x_mm), ("eq_esn", x_esn)):
                hard = np.stack([eo.hard_bits(X[f], const, m) for f in range(X.shape[0])])
                rec[det + "_uncoded"] = float(np.mean(hard != bits))
                for mode, (ww, mm) in (("flat", (ones, ones)), ("weighted", (w, mu))):
                    llr, _ = sr.llr_weighted(X, ww, mm, m, F)
                    jobs.append((llr, bits, u, n_cal, m))
                    names.append(f"{det}_coded_{mode}")
            for name, (errs, nb, ca, cb) in zip(names, pool.map(decode_leg, jobs, chunksize=1)):
                rec[name], rec[name + "_errors"], rec[name + "_bits"], rec[name + "_a"] = errs / nb, errs, nb, ca
            rec["seconds"] = time.time() - t0
            print(json.dumps(rec), flush=True)
            records.append(rec)
            with open(out, "w") as f:
                json.dump({"config": dict(n_t=cfg.n_t, n_r=cfg.n_r, n_sub=cfg.n_sub, bits_per_symbol=m, blocks=a.blocks,
                                          frames_per_block=F, calibration_frames=n_cal, n_reservoir=a.n_res, ridge=a.ridge,
                                          state_noise=0.001, code=dict(n=cfg.n_sub * m, d_v=4, d_c=8, seed=5),
                                          bp_iterations=MAXITER, where="NumPy oracle, CPU"),
                           "points": records}, f, indent=1)
    print("wrote", out)


if __name__ == "__main__":
    main()
