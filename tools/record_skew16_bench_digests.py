"""Records SHA-256 digests of what the 16x16x32 skewed predict kernel (esn_recur_skew16_impl.h) writes at the bench's own
launch shape, cut down, into tests/golden/skew16_bench_shape_digests.json, for tests/test_gpu_skew16_bench_shape.py.
Needs a GPU.

tools/record_skew16_digests.py pins a covering sample of small launches (at most 11 groups, 24 steps).  This one pins the
shape bench.py runs -- N_res 512, 16 inputs, 8 outputs, 75 frames per group, 138 steps, transient 10, counter noise -- at
40 groups: 25 workgroups of 128 slots, groups of 80 slots (five of padding) that straddle workgroup boundaries.  f16 and
bf16, float64 and float32 I/O, with and without an initial state, and one case whose inputs end before the steps do.

Run it with the library of the commit whose results are to be pinned (ESN_HIP_LIB selects another build):

    ESN_HIP_LIB=<that tree>/esn_ofdm_mimo_amd/libesn_hip.so python tools/record_skew16_bench_digests.py --commit <hash>
"""
import argparse
import hashlib
import itertools
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

GOLDEN = os.path.join(ROOT, "tests", "golden", "skew16_bench_shape_digests.json")
SEED = 20261016
SHAPE = {"n_res": 512, "n_in": 16, "n_out": 8, "F": 75, "G": 40, "T": 138, "transient": 10, "noise_mode": "counter"}
AXES = {"precision": ("f16", "bf16"), "io": ("f64", "f32"), "init": (False, True)}
T_IN_SHORT = 131          # the one case with T_in < T: the last seven steps read zeros


def cases():
    out = [dict(zip(AXES, v), t_in=SHAPE["T"]) for v in itertools.product(*AXES.values())]
    out.append(dict(precision="f16", io="f64", init=False, t_in=T_IN_SHORT))
    for c in out:
        c["id"] = "-".join(f"{k}={int(c[k]) if isinstance(c[k], bool) else c[k]}" for k in (*AXES, "t_in"))
    return out


def arrays(i, c):
    """Weights, read-out, scalings, inputs and initial state of case i."""
    rng = np.random.default_rng([SEED, i])
    n, n_in, n_out, G = SHAPE["n_res"], SHAPE["n_in"], SHAPE["n_out"], SHAPE["G"]
    B = G * SHAPE["F"]
    return dict(
        w=(rng.random((1, n, n)) < 0.1) * rng.standard_normal((1, n, n)) * (0.9 / np.sqrt(0.1 * n)),
        w_in=rng.uniform(-1, 1, (1, n, n_in)), w_fb=rng.uniform(-1, 1, (1, n, n_out)),
        w_out=rng.standard_normal((G, n_out, n + n_in)) * 0.004,       # weak feedback
        in_scale=rng.random((G, n_in)) * 0.2 + 0.1, in_shift=rng.standard_normal((G, n_in)) * 0.05,
        t_scale=rng.random((G, n_out)) + 0.5, t_shift=rng.standard_normal((G, n_out)) * 0.1,
        u=rng.standard_normal((B, c["t_in"], n_in)),
        x0=rng.standard_normal((G, n)) * 0.1 if c["init"] else None,
        y0=rng.standard_normal((G, n_out)) * 0.1 if c["init"] else None)


def digest(i, c):
    """SHA-256 of the raw bytes of Y of case i, from the library that esn_ofdm_mimo_amd._lib has loaded."""
    from esn_ofdm_mimo_amd import _lib, batched
    a = arrays(i, c)
    bank = batched.ReservoirBank(SHAPE["n_in"], SHAPE["n_out"], SHAPE["n_res"], a["w"], a["w_in"], a["w_fb"], noise=1e-3)
    bank.set_scaling(a["in_scale"], a["in_shift"], a["t_scale"], a["t_shift"])
    bank.set_readout(a["w_out"])
    path = _lib.recur_path(False, c["precision"], bank.shape, a["u"].shape[0], SHAPE["F"])
    assert path == "skew16", (c["id"], path)
    u = a["u"].astype(np.float32) if c["io"] == "f32" else a["u"]
    y = bank.predict(u, SHAPE["F"], T=SHAPE["T"], transient=SHAPE["transient"], precision=c["precision"], x0=a["x0"],
                     y0=a["y0"], noise_mode=SHAPE["noise_mode"], seed=11 + i, io=c["io"])
    y = y.cpu().numpy()
    assert y.shape == (a["u"].shape[0], SHAPE["T"] - SHAPE["transient"], SHAPE["n_out"]) and np.isfinite(y).all(), c["id"]
    assert y.dtype == (np.float32 if c["io"] == "f32" else np.float64)
    return hashlib.sha256(np.ascontiguousarray(y).tobytes()).hexdigest()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--commit", required=True, help="hash of the commit the loaded library was built from")
    ap.add_argument("--out", default=GOLDEN)
    args = ap.parse_args()
    from esn_ofdm_mimo_amd import _lib
    cs = cases()
    doc = {"commit": args.commit, "seed": SEED, "shape": SHAPE, "t_in_short": T_IN_SHORT,
           "axes": {k: [int(x) if isinstance(x, bool) else x for x in v] for k, v in AXES.items()},
           "digests": [[c["id"], digest(i, c)] for i, c in enumerate(cs)]}
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=0, sort_keys=True)
        f.write("\n")
    print(f"{args.out}: {len(cs)} digests from {_lib.LIB_PATH}")


if __name__ == "__main__":
    main()
