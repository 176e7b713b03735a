"""Records SHA-256 digests of what the MFMA recurrence kernel (esn::recur_mfma_kernel, esn_recur_mfma_impl.h: the skewed
32x32x16 predict schedule, the in-step predict schedule and the in-step harvest) writes over a covering sample of its
shapes into tests/golden/mfma_parent_digests.json, for tests/test_gpu_mfma_digests.py to compare against: a rewrite of
the kernel that is meant to keep its results keeps every output byte.  Needs a GPU.

Run it with the library of the commit whose results are to be pinned (ESN_HIP_LIB selects another build):

    ESN_HIP_LIB=<that tree>/esn_ofdm_mimo_amd/libesn_hip.so python tools/record_mfma_digests.py --commit <hash>

The sample: every value of every axis below occurs, and so does every (kind, precision, noise mode, output type)
combination -- predict digests Y (float64 / float32 I/O), harvest digests E of ReservoirBank.harvest (e_dtype) -- with
N_CASES / 36 cases each; the other axes are drawn per case from a seeded generator.  Inputs come from seeded NumPy
generators, so this tool and the test build the same arrays.

The knobs of a case (knobs_of below, restored afterwards) keep the call on this kernel: s16=0 (257..512 units stay off the
16x16x32 kernel), hcluster=0 (no clustered harvest), big_gemm=0 (no launch-per-step GEMM beyond 1024 units), and skew
per case (the `schedule` axis: half-precision predict on the skewed or on the in-step schedule)."""
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

GOLDEN = os.path.join(ROOT, "tests", "golden", "mfma_parent_digests.json")
SEED = 20261021          # (a seed under which each of the three skewed tilings occurs: cases() asserts it)
N_CASES = 144
AXES = {
    "kind": ("predict", "harvest"),
    "precision": ("f32", "f16", "bf16"),
    "noise_mode": ("none", "counter", "tensor"),
    "out": ("f64", "f32"),            # predict: I/O type of U and Y; harvest: e_dtype
    # the smallest sizes of each row of mfma_geometry's table: (4,1,2); (4,2,2) / (8,1,4); (8,2,2) / (8,2,4) /
    # harvest (8,2,1); (8,4,1) / (8,4,2); (16,4,1) (half precision only: float32 redraws it)
    "n_res": (48, 200, 300, 600, 1100),
    "schedule": ("default", "skew0"),
    "n_in": (2, 3, 6, 16),            # 3: register staging, no LDS-DMA; 6: DMA, no skew; 2, 16: skew-eligible
    "n_out": (1, 5, 8, 12),           # 12: two read-out images without the fold in half precision
    "F": (75, 16, 7),                 # frames per group
    "G": (1, 3, 11),                  # groups
    "n_wsets": (1, 2),
    "transient": (0, 10),
    "init": (True, False),            # with / without x0 and y0
    "ragged": (0, 3),                 # frames missing from the last group
    "t_pad": (0, 4),                  # T - T_in: steps past the end of the inputs read zeros
    "gain": (0.1, 5.0),               # on in_scale: float32 tiles on both sides of the TANH32_SERIES_MAX vote
}
T_IN = 20
COMBO = ("kind", "precision", "noise_mode", "out")
HARVEST_F_MAX = 16                    # a harvest has one pilot per group: G * min(F, 16) - ragged pilots


def cases():
    """The sample, a list of dicts over AXES (deterministic: SEED)."""
    rng = np.random.default_rng(SEED)
    combos = list(itertools.product(*(AXES[k] for k in COMBO)))
    rest = [k for k in AXES if k not in COMBO]
    out = []
    for i in range(N_CASES):
        c = dict(zip(COMBO, combos[i % len(combos)]))
        for k in rest:
            c[k] = AXES[k][int(rng.integers(len(AXES[k])))]
        while c["precision"] == "f32" and c["n_res"] > 1024:
            c["n_res"] = AXES["n_res"][int(rng.integers(len(AXES["n_res"])))]
        if c["G"] * min(c["F"], HARVEST_F_MAX) <= c["ragged"]:
            c["ragged"] = 0
        c["id"] = "-".join(f"{k}={int(c[k]) if isinstance(c[k], bool) else c[k]}" for k in AXES)
        out.append(c)
    for k, vals in AXES.items():
        seen = {c[k] for c in out}
        assert seen == set(vals), (k, seen)
    assert {tuple(c[k] for k in COMBO) for c in out} == set(combos)
    assert len({c["id"] for c in out}) == N_CASES
    assert {c["n_res"] for c in out if skew_eligible(c) and c["schedule"] == "default"} == {200, 300, 600}
    return out


def knobs_of(c):
    return {"s16": 0, "hcluster": 0, "big_gemm": 0, "skew": 0 if c["schedule"] == "skew0" else 1}


class knobs:
    """with knobs(c): the case's knobs, back to their defaults afterwards"""

    def __init__(self, c):
        self.k = knobs_of(c)

    def __enter__(self):
        from esn_ofdm_mimo_amd import _lib
        for key, v in self.k.items():
            _lib.debug_set(key, v)

    def __exit__(self, *exc):
        from esn_ofdm_mimo_amd import _lib
        for key in self.k:
            _lib.debug_set(key, None)


def n_sequences(c):
    return c["G"] * (min(c["F"], HARVEST_F_MAX) if c["kind"] == "harvest" else c["F"]) - c["ragged"]


def shape_of(c):
    from esn_ofdm_mimo_amd import _lib
    return _lib.Shape(c["n_res"], c["n_in"], c["n_out"], 1, c["n_wsets"], 0.0)


def paths(c):
    """(no GPU) the kernel the library picks for the case under its knobs, with and without a workspace lent"""
    from esn_ofdm_mimo_amd import _lib
    harvest = c["kind"] == "harvest"
    with knobs(c):
        return tuple(_lib.recur_path(harvest, c["precision"], shape_of(c), n_sequences(c), 1 if harvest else c["F"], ws)
                     for ws in (True, False))


def skew_eligible(c):
    return (c["kind"] == "predict" and c["precision"] != "f32" and c["n_in"] in (2, 16) and c["n_out"] <= 8 and
            c["n_res"] in (200, 300, 600))


def arrays(i, c):
    """Weights, read-out, scalings, inputs, teacher and initial state of case i."""
    rng = np.random.default_rng([SEED, i])
    n, n_in, n_out, nw = c["n_res"], c["n_in"], c["n_out"], c["n_wsets"]
    harvest = c["kind"] == "harvest"
    B, T = n_sequences(c), T_IN + c["t_pad"]
    G = B if harvest else c["G"]                      # groups: one pilot each when harvesting
    t_u = T if harvest else T_IN
    w = (rng.random((nw, n, n)) < 0.1) * rng.standard_normal((nw, n, n)) * (0.9 / np.sqrt(0.1 * n))
    a = dict(
        w=w, w_in=rng.uniform(-1, 1, (nw, n, n_in)), w_fb=rng.uniform(-1, 1, (nw, n, n_out)),
        w_out=rng.standard_normal((G, n_out, n + n_in)) * 0.004,       # weak feedback
        in_scale=(rng.random((G, n_in)) * 0.2 + 0.1) * c["gain"], in_shift=rng.standard_normal((G, n_in)) * 0.05,
        t_scale=rng.random((G, n_out)) + 0.5, t_shift=rng.standard_normal((G, n_out)) * 0.1,
        u=rng.standard_normal((B, t_u, n_in)),
        d=rng.standard_normal((B, T, n_out)) * 0.3 if harvest else None,
        x0=rng.standard_normal((G, n)) * 0.1 if c["init"] else None,
        y0=rng.standard_normal((G, n_out)) * 0.1 if c["init"] else None,
        noise_u=rng.random((B, T - 1 if harvest else T, n)) if c["noise_mode"] == "tensor" else None)
    return a, T


def digest(i, c, knob_values=None):
    """SHA-256 of the raw bytes of Y (predict) or E (harvest) of case i, from the library that
    esn_ofdm_mimo_amd._lib has loaded."""
    from esn_ofdm_mimo_amd import batched
    a, T = arrays(i, c)
    assert paths(c) == ("mfma", "mfma"), (c["id"], paths(c))
    f32 = c["out"] == "f32"
    with knobs(c if knob_values is None else dict(c, **knob_values)):
        bank = batched.ReservoirBank(c["n_in"], c["n_out"], c["n_res"], a["w"], a["w_in"], a["w_fb"],
                                     noise=0.0 if c["noise_mode"] == "none" else 1e-3)
        bank.set_scaling(a["in_scale"], a["in_shift"], a["t_scale"], a["t_shift"])
        if c["kind"] == "harvest":
            y = bank.harvest(a["u"], a["d"], precision=c["precision"], noise_mode=c["noise_mode"], noise_u=a["noise_u"],
                             seed=5 + i, e_dtype=c["out"])
            want = (a["u"].shape[0], T, c["n_res"] + c["n_in"])
        else:
            bank.set_readout(a["w_out"])
            u = a["u"].astype(np.float32) if f32 else a["u"]
            y = bank.predict(u, c["F"], T=T, transient=c["transient"], precision=c["precision"], x0=a["x0"], y0=a["y0"],
                             noise_mode=c["noise_mode"], noise_u=a["noise_u"], seed=5 + i, io=c["out"])
            want = (a["u"].shape[0], T - c["transient"], c["n_out"])
        y = y.cpu().numpy()
    assert y.shape == want and np.isfinite(y).all(), c["id"]
    assert y.dtype == (np.float32 if f32 else np.float64)
    return hashlib.sha256(np.ascontiguousarray(y).tobytes()).hexdigest()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--commit", required=True, help="hash of the commit the loaded library was built from")
    ap.add_argument("--out", default=GOLDEN)
    args = ap.parse_args()
    from esn_ofdm_mimo_amd import _lib
    cs = cases()
    # the schedule knob takes effect: the skewed schedule adds the counter noise of fp16 in packed halves, the in-step
    # schedule in float32, so the two digests of one skew-eligible case differ
    i = next(i for i, c in enumerate(cs) if skew_eligible(c) and c["precision"] == "f16" and c["noise_mode"] == "counter")
    pair = [digest(i, cs[i], {"schedule": s}) for s in AXES["schedule"]]
    assert pair[0] != pair[1], (cs[i]["id"], "skew=0 and skew=1 gave the same bytes")
    doc = {"commit": args.commit, "seed": SEED, "axes": {k: list(v) for k, v in AXES.items()},
           "digests": [[c["id"], digest(i, c)] for i, c in enumerate(cs)]}
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=0, sort_keys=True)
        f.write("\n")
    print(f"{args.out}: {len(cs)} digests from {_lib.LIB_PATH}")


if __name__ == "__main__":
    main()
