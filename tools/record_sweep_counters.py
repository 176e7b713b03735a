"""Records what small DetectorSweep runs, the two coded comparison points and the seven uncoded comparison points produce
-- the int64 counters, fits_repaired, the SHA-256 of the bank's W_out after the run and, where a case has them,
ridge_choice_counts, symbol_error_counts and fresh_radius_hits; of an uncoded point its counters per block -- into
tests/golden/sweep_parent_counters.json for tests/test_gpu_sweep_counters.py: a rewrite of the Monte-Carlo harness that
is meant to keep its results keeps every one of these entries.  Needs a GPU.

Run it from the tree of the commit whose results are to be pinned (the package next to this tool is the one loaded):

    python tools/record_sweep_counters.py --commit <hash>

Every case runs twice and the file is written only if the two runs agree: a case that is not deterministic on the
recorded commit pins nothing.  One case per constructor arm and per branch of a chunk (CASES); unless a case says
otherwise: LinkParams.block_fading(n_t=2, n_r=2, n_sub=64) with three data symbols per pilot, n_reservoir 64, seed 7,
run([6, 18] dB, 6 blocks per point, chunks of 4), so every point has one full and one short chunk and no cluster kernel
or workspace path is involved.  The coded points use LdpcCode(64 * 4 = 256, 4, 8, seed=11).  The uncoded points
(POINT_CASES) run at 18 dB on FrameSource(small_link(), seed 7): 6 blocks from block 2 on in chunks of 4, three data
frames per block -- again one full and one short chunk, and a first block that is not 0.

The reservoirs of most cases are drawn on the host through np.linalg.eigvals, which follows the host's LAPACK; for these
the file also holds the SHA-256 of the drawn W (host_draw_digest, computed here without the package), so that a
machine whose LAPACK rounds differently is told apart from a harness that computes something else."""
import argparse
import dataclasses
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

GOLDEN = os.path.join(ROOT, "tests", "golden", "sweep_parent_counters.json")
SEED, N_RES = 7, 64
EBNO, BLOCKS, CHUNK = [6.0, 18.0], 6, 4
CODED_EBNO, CODED_SNR_IDX, CODED_BLOCKS, CODED_SEED = 18.0, 1, 8, 3


def ridge_by_ebno(ebno_db):
    return 1e-3 if ebno_db > 12 else 1.0


def small_link(**changes):
    from esn_ofdm_mimo_amd.montecarlo import LinkParams
    return dataclasses.replace(LinkParams.block_fading(n_t=2, n_r=2, n_sub=64), coherence_fixed=3, **changes)


def siso_link():
    from esn_ofdm_mimo_amd.montecarlo import LinkParams
    return LinkParams.siso_awgn(n_sub=64, symbols_per_pilot=3)


def bench_link():
    from esn_ofdm_mimo_amd.montecarlo import LinkParams
    return LinkParams()


# name: (link, DetectorSweep keywords beyond seed, run keywords beyond chunk_blocks)
CASES = {
    "defaults": (small_link, {}, {}),
    "per_block_f16_io32": (small_link, dict(reservoirs="per_block", pool=3, precision="f16", fit_precision="f16",
                                            io="f32"), {}),
    "fresh_cache": (small_link, dict(reservoirs="fresh", fresh_radius_cache=True), {}),
    "fresh_no_cache": (small_link, dict(reservoirs="fresh", fresh_radius_cache=False), {}),
    "fresh_f16x2": (small_link, dict(reservoirs="fresh", radius_precision="f16x2"), {}),
    "device_radius_per_block": (small_link, dict(radius="device", reservoirs="per_block", pool=2), {}),
    "ridge_float": (small_link, dict(ridge=1e-3), {}),
    "ridge_callable": (small_link, dict(ridge=ridge_by_ebno), {}),
    "ridge_grid": (small_link, dict(ridge_grid=[1e-6, 1e-3, 1e-1]), {}),
    "symbol_counts_jakes": (lambda: small_link(fading="jakes", f_d=1000.0), dict(symbol_counts=True), {}),
    "train_ebno": (small_link, dict(train_ebno=12.0), {}),
    "siso_continuation": (siso_link, dict(n_reservoir=32), {}),
    "rank_1_of_2": (small_link, dict(rank=1, world_size=2), {}),
    "bench_link": (bench_link, dict(), dict(frames_per_block=2)),
    "track_decisions": (small_link, dict(track="decisions", track_window=2, symbol_counts=True), {}),
    "track_genie": (small_link, dict(track="genie", ridge=1e-3, symbol_counts=True), {}),
    "pilots3_grid": (small_link, dict(n_pilots=3, ridge_grid=[1e-6, 1e-3, 1e-1]), {}),
    "gram_track": (small_link, dict(solve_method="gram", ridge=1e-3, n_pilots=2, track="decisions", track_forget=0.9,
                                    symbol_counts=True), {}),
    "chol_f16": (small_link, dict(solve_method="chol", fit_precision="f16", precision="f16"), {}),
}
DEVICE_DRAWN = ("fresh_cache", "fresh_no_cache", "fresh_f16x2", "device_radius_per_block")
POINTS_CASE = "coded_points"
POINTS_POOL = 3
POINT_EBNO, POINT_SNR_IDX = 18.0, 1
POINT_BLOCKS = dict(n_blocks=6, first_block=2, chunk_blocks=4, frames_per_block=3)
# name: (function of esn_ofdm_mimo_amd.montecarlo, its keywords beyond POINT_BLOCKS)
POINT_CASES = {
    "baseline_tracking_point": ("baseline_tracking_point", dict(track="decisions", window=2)),
    "elm_point": ("elm_point", dict(n_hidden=16, window=4, weights="per_block", ridge=1e-3)),
    "fnn_point": ("fnn_point", dict(n_hidden=16, window=4, epochs=3, weights="per_block")),
    "cnn_point": ("cnn_point", dict(channels=(4, 8), kernel=3, epochs=3)),
    "lstm_point": ("lstm_point", dict(n_hidden=8, epochs=3, slice="reference")),
    "ensemble_point_shared": ("ensemble_point", dict(n_members=2, n_reservoir=32, reservoirs="shared",
                                                     member_counts=True)),
    "ensemble_point_fresh_f16_io32": ("ensemble_point", dict(n_members=2, n_reservoir=32, reservoirs="fresh",
                                                             precision="f16", fit_precision="f16", io="f32")),
    "equalized_esn_point": ("equalized_esn_point", dict(n_reservoir=8, reservoirs="per_block", pool=2, want_mmse=True)),
}
# the host draws of the points that have one: name -> (n_reservoir, seeds beyond SEED * 7919 + 17)
POINT_HOST_DRAWS = {"ensemble_point_shared": (32, (0, 104729)), "equalized_esn_point": (8, (0, 1))}
HOST_DRAWN = tuple(k for k in CASES if k not in DEVICE_DRAWN) + (POINTS_CASE,) + tuple(POINT_HOST_DRAWS)


def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def host_draw_digest(name):
    """SHA-256 of the W matrices the case's constructor draws on the host, stacked: the reference's recipe (uniform - 0.5,
    sparsify, scale by max |eigvals|) with the sweep's seeds, written out here so that it does not pass through the
    package under test.  No GPU."""
    if name in POINT_HOST_DRAWS:
        n_res, offsets = POINT_HOST_DRAWS[name]
    elif name == POINTS_CASE:
        n_res, offsets = N_RES, range(POINTS_POOL)
    else:
        _, kw, _ = CASES[name]
        n_res = kw.get("n_reservoir", N_RES)
        offsets = range(kw.get("pool", 8) if kw.get("reservoirs", "shared") == "per_block" else 1)
    ws = []
    for i in offsets:
        rs = np.random.RandomState(SEED * 7919 + 17 + i)
        w = rs.rand(n_res, n_res) - 0.5
        w[rs.rand(n_res, n_res) < 0.1] = 0
        ws.append(w * (0.9 / np.max(np.abs(np.linalg.eigvals(w)))))
    return _sha(np.stack(ws))


def make_sweep(name):
    from esn_ofdm_mimo_amd.montecarlo import DetectorSweep
    link, kw, _ = CASES[name]
    return DetectorSweep(link(), **{"n_reservoir": N_RES, "seed": SEED, **kw})


def sweep_record(name):
    """One run of the case's sweep, as the JSON-ready record."""
    sw = make_sweep(name)
    _, counters = sw.run(EBNO, BLOCKS, chunk_blocks=CHUNK, **CASES[name][2])
    rec = {"counters": np.asarray(counters).tolist(), "fits_repaired": int(sw.fits_repaired),
           "w_out_sha256": _sha(sw.bank.W_out.cpu().numpy())}
    if sw.ridge_choice_counts:
        rec["ridge_choice_counts"] = {f"{e:g}": np.asarray(v).tolist() for e, v in sw.ridge_choice_counts.items()}
    if sw.symbol_error_counts:
        rec["symbol_error_counts"] = {f"{e:g}": np.asarray(v).tolist() for e, v in sw.symbol_error_counts.items()}
    if sw.reservoirs == "fresh":
        rec["fresh_radius_hits"] = int(sw.fresh_radius_hits)
    return rec


def _plain(d):
    """Floats as float.hex, arrays as lists of float.hex, ints as they are."""
    out = {}
    for k, v in d.items():
        if isinstance(v, np.ndarray):
            out[k] = [float(x).hex() for x in v.reshape(-1)]
        elif isinstance(v, (int, np.integer)):
            out[k] = int(v)
        else:
            out[k] = float(v).hex()
    return out


def points_record():
    """coded_ber_point and block_fading_point (with a train_ebno=12 sweep and the channel record) on per_block sweeps."""
    from esn_ofdm_mimo_amd.coded import LdpcCode
    from esn_ofdm_mimo_amd.montecarlo import DetectorSweep, block_fading_point, coded_ber_point
    prm = small_link()
    kw = dict(n_reservoir=N_RES, seed=SEED, reservoirs="per_block", pool=POINTS_POOL)
    sweep, fixed = DetectorSweep(prm, **kw), DetectorSweep(prm, train_ebno=12.0, **kw)
    code = LdpcCode(prm.n_sub * prm.m, 4, 8, seed=11)
    coded = coded_ber_point(sweep, code, CODED_EBNO, CODED_SNR_IDX, n_blocks=CODED_BLOCKS, frames_per_block=2,
                            seed=CODED_SEED)
    w_coded = _sha(sweep.bank.W_out.cpu().numpy())
    fading = block_fading_point(sweep, code, CODED_EBNO, CODED_SNR_IDX, n_blocks=CODED_BLOCKS, fixed_sweep=fixed,
                                channel_metrics=True, seed=CODED_SEED)
    return {"coded_ber_point": _plain(coded), "block_fading_point": _plain(fading),
            "w_out_sha256": {"after_coded_ber_point": w_coded, "matched": _sha(sweep.bank.W_out.cpu().numpy()),
                             "train_fixed": _sha(fixed.bank.W_out.cpu().numpy())}}


def point_record(name):
    """One uncoded comparison point: what it returns, as lists (of the baseline's dict: errors, bits and failed)."""
    from esn_ofdm_mimo_amd import montecarlo as mc
    fn, kw = POINT_CASES[name]
    out = getattr(mc, fn)(mc.FrameSource(small_link(), seed=SEED), POINT_EBNO, POINT_SNR_IDX, **POINT_BLOCKS, **kw)
    if isinstance(out, dict):
        return {"errors": out["errors"].tolist(), "bits": out["bits"].tolist(), "failed": int(out["failed"])}
    return {"outputs": [t.cpu().numpy().tolist() for t in out]}


def record(name):
    if name in POINT_CASES:
        return point_record(name)
    return points_record() if name == POINTS_CASE else sweep_record(name)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--commit", required=True, help="hash of the commit this tree is")
    ap.add_argument("--out", default=GOLDEN)
    args = ap.parse_args()
    import torch
    cases = {}
    for name in list(CASES) + [POINTS_CASE] + list(POINT_CASES):
        first, second = record(name), record(name)
        if first != second:
            sys.exit(f"{name}: two runs of this tree differ, nothing written\n{first}\n{second}")
        cases[name] = first
        print(f"{name}: {first.get('counters', first.get('outputs', ''))}", flush=True)
    doc = {"commit": args.commit, "numpy": np.__version__, "torch": torch.__version__,
           "device": torch.cuda.get_device_name(0), "seed": SEED,
           "host_draw_sha256": {name: host_draw_digest(name) for name in HOST_DRAWN}, "cases": cases}
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=0, sort_keys=True)
        f.write("\n")
    print(f"{args.out}: {len(cases)} cases")


if __name__ == "__main__":
    main()
