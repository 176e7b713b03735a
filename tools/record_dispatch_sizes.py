"""Records what the size queries answer over a grid of shapes and dispatch knobs into
tests/golden/dispatch_sizes.json, for tests/test_dispatch_cpu.py to replay.  Needs the built library, no GPU.

Run it on the commit whose answers are to be pinned (ESN_HIP_LIB selects another build of the library):

    python tools/record_dispatch_sizes.py --commit $(git rev-parse HEAD)

Layout of the file: the grid axes; per shape the knob-independent values [tile_frames, packed_weights_bytes,
packed_readout_bytes]; per shape and (n_frames, F) the default-knob [predict_workspace_bytes,
harvest_workspace_bytes]; per knob setting the full rows [tile, weights, readout, predict_ws, harvest_ws] that differ
from the default row of the same shape.  A combination absent from a knob's list equals its default row."""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PRECISIONS = ("f64", "f32", "f16", "bf16")
N_RES = (64, 128, 129, 256, 257, 300, 512, 513, 1024, 1025, 1500, 2048, 2049)
IO = ((2, 2), (3, 2), (4, 4), (16, 8), (16, 16))
N_WSETS = (1, 3)
FRAMES = ((1, 1), (8, 1), (9, 4), (150, 75), (4096, 64))            # (n_frames, frames_per_group)
DEFAULTS = {"cluster": "1", "big_gemm": "1", "hcluster": "1", "f64_mfma": "1", "s16": "1", "skew": "1"}
MOVED = (("cluster", "0"), ("big_gemm", "0"), ("hcluster", "0"), ("f64_mfma", "0"), ("s16", "0"), ("skew", "0"))


def shapes():
    for prec in PRECISIONS:
        for n_res in N_RES:
            for n_in, n_out in IO:
                for nw in N_WSETS:
                    yield prec, n_res, n_in, n_out, nw


def shape_key(prec, n_res, n_in, n_out, nw):
    return f"{prec}|{n_res}|{n_in}|{n_out}|{nw}"


def walk(lib, _lib):
    """{(shape key, frames index): [tile, weights, readout, predict_ws, harvest_ws]} under the knobs as they stand"""
    rows = {}
    for prec, n_res, n_in, n_out, nw in shapes():
        p, sh = _lib.PRECISIONS[prec], _lib.Shape(n_res, n_in, n_out, 1, nw, 1.0)
        fixed = [lib.esn_tile_frames(p, C.byref(sh)), lib.esn_packed_weights_bytes(p, C.byref(sh)),
                 lib.esn_packed_readout_bytes(p, C.byref(sh))]
        for i, (nf, f) in enumerate(FRAMES):
            rows[shape_key(prec, n_res, n_in, n_out, nw), i] = fixed + [
                lib.esn_predict_workspace_bytes(p, C.byref(sh), nf, f),
                lib.esn_harvest_workspace_bytes(p, C.byref(sh), nf)]
    return rows


def record(lib, _lib):
    for k, v in DEFAULTS.items():
        _lib.debug_set(k, v)
    base = walk(lib, _lib)
    fixed, sizes = {}, {}
    for (key, i), row in base.items():
        assert fixed.setdefault(key, row[:3]) == row[:3]
        sizes.setdefault(key, []).append(row[3:])
    diffs = {}
    for k, v in MOVED:
        _lib.debug_set(k, v)
        try:
            moved = walk(lib, _lib)
        finally:
            _lib.debug_set(k, DEFAULTS[k])
        diffs[f"{k}={v}"] = {f"{key}|{i}": row for (key, i), row in moved.items() if row != base[key, i]}
    return fixed, sizes, diffs


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--commit", required=True, help="hash of the commit the loaded library was built from")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "dispatch_sizes.json"))
    args = ap.parse_args()
    from esn_ofdm_mimo_amd import _lib
    fixed, sizes, diffs = record(_lib.load(), _lib)
    doc = {"commit": args.commit,
           "grid": {"precisions": PRECISIONS, "n_res": N_RES, "io": IO, "n_wsets": N_WSETS, "frames": FRAMES,
                    "defaults": DEFAULTS, "moved": MOVED},
           "shape": fixed, "sizes": sizes, "diffs": diffs}
    with open(args.out, "w") as f:
        json.dump(doc, f, separators=(",", ":"), sort_keys=True)
        f.write("\n")
    n = len(fixed) * len(FRAMES)
    print(f"{args.out}: {n} default rows, {n * len(MOVED)} knob rows of which "
          f"{sum(len(d) for d in diffs.values())} differ ({ {k: len(d) for k, d in diffs.items() if d} })")


if __name__ == "__main__":
    main()
