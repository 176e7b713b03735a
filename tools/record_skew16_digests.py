"""Records SHA-256 digests of what the 16x16x32 skewed predict kernel (esn_recur_skew16_impl.h) writes over a
covering sample of its shapes into tests/golden/skew16_parent_digests.json, for tests/test_gpu_skew16_sets.py to
compare against: a rewrite of the kernel that is meant to keep its results keeps every output byte.  Needs a GPU.

Run it with the library of the commit whose results are to be pinned (ESN_HIP_LIB selects another build):

    ESN_HIP_LIB=<that tree>/esn_ofdm_mimo_amd/libesn_hip.so python tools/record_skew16_digests.py --commit <hash>

The sample: every value of every axis below occurs, and so does every (precision, noise mode, I/O type) triple --
the twelve instances of the kernel -- with N_CASES / 12 cases each; the other axes are drawn per case from a seeded
generator (the full product would be 14 000 launches).  Inputs come from seeded NumPy generators, so this tool and
the test build the same arrays."""
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

GOLDEN = os.path.join(ROOT, "tests", "golden", "skew16_parent_digests.json")
SEED = 20260716
N_CASES = 96
AXES = {
    "precision": ("f16", "bf16"),
    "noise_mode": ("none", "counter", "tensor"),
    "io": ("f64", "f32"),
    "n_in": (2, 4, 8, 16),
    "n_out": (1, 4, 5, 8),
    "n_res": (300, 512),
    "F": (75, 16, 7),                 # frames per group
    "G": (1, 3, 11),                  # groups
    "n_wsets": (1, 2),
    "transient": (0, 10),
    "init": (True, False),            # with / without x0 and y0
    "ragged": (0, 3),                 # frames missing from the last group
    "t_pad": (0, 4),                  # T - T_in: steps past the end of the inputs read zeros
}
T_IN = 20
TRIPLE = ("precision", "noise_mode", "io")


def cases():
    """The sample, a list of dicts over AXES (deterministic: SEED)."""
    rng = np.random.default_rng(SEED)
    triples = list(itertools.product(*(AXES[k] for k in TRIPLE)))
    rest = [k for k in AXES if k not in TRIPLE]
    out = []
    for i in range(N_CASES):
        c = dict(zip(TRIPLE, triples[i % len(triples)]))
        for k in rest:
            c[k] = AXES[k][int(rng.integers(len(AXES[k])))]
        if c["G"] * c["F"] <= c["ragged"]:
            c["ragged"] = 0
        c["id"] = "-".join(f"{k}={int(c[k]) if isinstance(c[k], bool) else c[k]}" for k in AXES)
        out.append(c)
    for k, vals in AXES.items():
        seen = {c[k] for c in out}
        assert seen == set(vals), (k, seen)
    assert {tuple(c[k] for k in TRIPLE) for c in out} == set(triples)
    assert len({c["id"] for c in out}) > N_CASES * 3 // 4       # (a repeated draw is harmless, a degenerate sample is not)
    return out


def arrays(i, c):
    """Weights, read-out, scalings, inputs and initial state of case i."""
    rng = np.random.default_rng([SEED, i])
    n, n_in, n_out, nw, G = c["n_res"], c["n_in"], c["n_out"], c["n_wsets"], c["G"]
    B, T = G * c["F"] - c["ragged"], T_IN + c["t_pad"]
    w = (rng.random((nw, n, n)) < 0.1) * rng.standard_normal((nw, n, n)) * (0.9 / np.sqrt(0.1 * n))
    a = dict(
        w=w, w_in=rng.uniform(-1, 1, (nw, n, n_in)), w_fb=rng.uniform(-1, 1, (nw, n, n_out)),
        w_out=rng.standard_normal((G, n_out, n + n_in)) * 0.004,       # weak feedback
        in_scale=rng.random((G, n_in)) * 0.2 + 0.1, in_shift=rng.standard_normal((G, n_in)) * 0.05,
        t_scale=rng.random((G, n_out)) + 0.5, t_shift=rng.standard_normal((G, n_out)) * 0.1,
        u=rng.standard_normal((B, T_IN, n_in)),
        x0=rng.standard_normal((G, n)) * 0.1 if c["init"] else None,
        y0=rng.standard_normal((G, n_out)) * 0.1 if c["init"] else None,
        noise_u=rng.random((B, T, n)) if c["noise_mode"] == "tensor" else None)
    return a, T


def digest(i, c):
    """SHA-256 of the raw bytes of Y of case i, from the library that esn_ofdm_mimo_amd._lib has loaded."""
    from esn_ofdm_mimo_amd import _lib, batched
    a, T = arrays(i, c)
    bank = batched.ReservoirBank(c["n_in"], c["n_out"], c["n_res"], a["w"], a["w_in"], a["w_fb"],
                                 noise=0.0 if c["noise_mode"] == "none" else 1e-3)
    bank.set_scaling(a["in_scale"], a["in_shift"], a["t_scale"], a["t_shift"])
    bank.set_readout(a["w_out"])
    path = _lib.recur_path(False, c["precision"], bank.shape, a["u"].shape[0], c["F"])
    assert path == "skew16", (c["id"], path)
    u = a["u"].astype(np.float32) if c["io"] == "f32" else a["u"]
    y = bank.predict(u, c["F"], T=T, transient=c["transient"], precision=c["precision"], x0=a["x0"], y0=a["y0"],
                     noise_mode=c["noise_mode"], noise_u=a["noise_u"], seed=5 + i, io=c["io"])
    y = y.cpu().numpy()
    assert y.shape == (a["u"].shape[0], T - c["transient"], c["n_out"]) and np.isfinite(y).all(), c["id"]
    assert y.dtype == (np.float32 if c["io"] == "f32" else np.float64)
    return hashlib.sha256(np.ascontiguousarray(y).tobytes()).hexdigest()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--commit", required=True, help="hash of the commit the loaded library was built from")
    ap.add_argument("--out", default=GOLDEN)
    args = ap.parse_args()
    from esn_ofdm_mimo_amd import _lib
    cs = cases()
    doc = {"commit": args.commit, "seed": SEED, "axes": {k: list(v) for k, v in AXES.items()},
           "digests": [[c["id"], digest(i, c)] for i, c in enumerate(cs)]}
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=0, sort_keys=True)
        f.write("\n")
    print(f"{args.out}: {len(cs)} digests from {_lib.LIB_PATH}")


if __name__ == "__main__":
    main()
