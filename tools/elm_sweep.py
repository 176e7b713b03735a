#!/usr/bin/env python3
"""BER against Eb/No of the windowed ELM beside the ESN and the LS-MMSE baseline, all on the same frames (one FrameSource
seed; the ELM and the baseline read the blocks the sweep detects):

    esn [ridge l]        DetectorSweep (N_res, fp16 kernels, state noise 0.001), pinv and, with --ridge, that lambda
    elm g=G [ridge l]    points.elm_point, slice "aligned", for every --gain and for pinv and --ridge
    elm reference slice  the first --gain, pinv, rows [0, N) of the un-cut output: the slice the reference's ELM / FNN
                         branches take (system_model_2_all_comparision.py:151-152, :570-571)
    ls-mmse              baseline_tracking_point(track=None)
    fnn, fnn reference slice   with --fnn: points.fnn_point (--fnn-hidden units, 50 Adam epochs per pilot), slices
                         "aligned" and "reference"
    cnn, cnn reference slice   with --cnn: points.cnn_point (channels 32 and 64, kernel 5, 50 Adam epochs per pilot,
                         float64), slices "aligned" and "reference"
    lstm, lstm reference slice   with --lstm: points.lstm_point (--lstm-hidden units, 50 Adam epochs per pilot, float64),
                         slices "aligned" and "reference" -- the reference's RNN curve

    python tools/elm_sweep.py [--preset 4x8|2x2] [--blocks 256] [--ebno 0:30:3] [--hidden H] [--window 8]
                              [--gain 0.05,0.02] [--ridge 1e-3] [--n-res 512] [--precision f64|f16] [--out file.json]
                              [--fnn [--fnn-hidden 100]] [--cnn] [--lstm [--lstm-hidden 100]]

Presets: 4x8 = LinkParams() (TDL-B, N = 128, 16-QAM), 512 hidden units against N_res 512; 2x2 = the block-fading 2x2
configuration at N = 512 (exponential PDP, 16-QAM), 100 hidden units as the reference's ELM(4 * window), N_res 100.
Writes profiles/elm_sweep_<preset>.json (with --fnn: profiles/fnn_sweep_<preset>.json; with --cnn: profiles/cnn_sweep_<preset>.json;
with --lstm: profiles/lstm_sweep_<preset>.json) unless --out is given.  Needs an MI355X."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PRESETS = {"4x8": dict(hidden=512, n_res=512), "2x2": dict(hidden=100, n_res=100)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--preset", choices=sorted(PRESETS), default="4x8")
    ap.add_argument("--blocks", type=int, default=256)
    ap.add_argument("--ebno", default="0:30:3", help="first:last:step in dB")
    ap.add_argument("--hidden", type=int, default=None)
    ap.add_argument("--n-res", type=int, default=None)
    ap.add_argument("--window", type=int, default=8)
    ap.add_argument("--gain", default="0.05,0.02")
    ap.add_argument("--ridge", type=float, default=1e-3)
    ap.add_argument("--precision", default="f64")
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--commit", default=None, help="recorded in the JSON")
    ap.add_argument("--out", default=None)
    ap.add_argument("--fnn", action="store_true", help="add the windowed FNN's curves")
    ap.add_argument("--fnn-hidden", type=int, default=100)
    ap.add_argument("--cnn", action="store_true", help="add the windowed CNN's curves")
    ap.add_argument("--lstm", action="store_true", help="add the LSTM's curves (the reference's RNN)")
    ap.add_argument("--lstm-hidden", type=int, default=100)
    a = ap.parse_args()
    from esn_ofdm_mimo_amd import _lib
    from esn_ofdm_mimo_amd.montecarlo import DetectorSweep, LinkParams, baseline_tracking_point, elm_point
    o = {k: getattr(a, k) if getattr(a, k) is not None else v for k, v in PRESETS[a.preset].items()}
    params = LinkParams() if a.preset == "4x8" else LinkParams.block_fading(2, 2, n_sub=512)
    lo, hi, step = (float(v) for v in a.ebno.split(":"))
    points = [lo + i * step for i in range(int(round((hi - lo) / step)) + 1)]
    gains = [float(g) for g in a.gain.split(",")]
    F = params.coherence_symbols
    curves = []

    def add(label, ber, **more):
        curves.append(dict(label=label, ber=[float(v) for v in ber], **more))
        print(f"{label:28s} " + " ".join(f"{v:.4f}" for v in ber), flush=True)

    src = None
    for ridge in (None, a.ridge):
        sw = DetectorSweep(params, n_reservoir=o["n_res"], noise=0.001, seed=a.seed, precision="f16", fit_precision="f16",
                           ridge=ridge)
        ber, _ = sw.run(points, a.blocks, frames_per_block=F)
        add("esn" + ("" if ridge is None else f" ridge {ridge:g}"), ber, ridge=ridge, fits_repaired=int(sw.fits_repaired))
        src = sw.src

    def elm(gain, ridge, sl):
        out = []
        for si, eb in enumerate(points):
            e, n = elm_point(src, eb, si, a.blocks, n_hidden=o["hidden"], window=a.window, gain=gain, ridge=ridge,
                             precision=a.precision, slice=sl, seed=a.seed, frames_per_block=F)
            out.append(float(e.sum()) / float(n.sum()))
        return out

    for gain in gains:
        for ridge in (None, a.ridge):
            add(f"elm g={gain:g}" + ("" if ridge is None else f" ridge {ridge:g}"), elm(gain, ridge, "aligned"),
                gain=gain, ridge=ridge, slice="aligned")
    add(f"elm g={gains[0]:g} reference slice", elm(gains[0], None, "reference"), gain=gains[0], ridge=None,
        slice="reference")
    add("ls-mmse", [baseline_tracking_point(src, eb, si, a.blocks, F)["ber"] for si, eb in enumerate(points)])
    if a.fnn:
        from esn_ofdm_mimo_amd.montecarlo import fnn_point
        for sl in ("aligned", "reference"):
            ber = []
            for si, eb in enumerate(points):
                e, n = fnn_point(src, eb, si, a.blocks, n_hidden=a.fnn_hidden, window=a.window, precision=a.precision,
                                 slice=sl, seed=a.seed, frames_per_block=F)
                ber.append(float(e.sum()) / float(n.sum()))
            add("fnn" + ("" if sl == "aligned" else " reference slice"), ber, n_hidden=a.fnn_hidden, epochs=50, lr=0.01,
                slice=sl)
    if a.cnn:
        from esn_ofdm_mimo_amd.montecarlo import cnn_point
        for sl in ("aligned", "reference"):
            ber = []
            for si, eb in enumerate(points):
                e, n = cnn_point(src, eb, si, a.blocks, slice=sl, seed=a.seed, frames_per_block=F)
                ber.append(float(e.sum()) / float(n.sum()))
            add("cnn" + ("" if sl == "aligned" else " reference slice"), ber, channels=[32, 64], kernel=5, epochs=50,
                lr=0.01, slice=sl)
    if a.lstm:
        from esn_ofdm_mimo_amd.montecarlo import lstm_point
        for sl in ("aligned", "reference"):
            ber = []
            for si, eb in enumerate(points):
                e, n = lstm_point(src, eb, si, a.blocks, n_hidden=a.lstm_hidden, slice=sl, seed=a.seed, frames_per_block=F)
                ber.append(float(e.sum()) / float(n.sum()))
            add("lstm" + ("" if sl == "aligned" else " reference slice"), ber, n_hidden=a.lstm_hidden, epochs=50, lr=0.01,
                slice=sl)
    result = {"config": dict(preset=a.preset, n_t=params.n_t, n_r=params.n_r, n_sub=params.n_sub, bits_per_symbol=params.m,
                             channel=params.channel, blocks=a.blocks, frames_per_block=F, n_hidden=o["hidden"],
                             window=a.window, n_reservoir=o["n_res"], elm_precision=a.precision, seed=a.seed,
                             device=_lib.device_info()["arch"], commit=a.commit),
              "ebno_db": points, "curves": curves}
    kind = "lstm" if a.lstm else "cnn" if a.cnn else "fnn" if a.fnn else "elm"
    out = a.out or os.path.join(ROOT, "profiles", f"{kind}_sweep_{a.preset}.json")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(result, f, indent=1)
    print("wrote", out)


if __name__ == "__main__":
    main()
