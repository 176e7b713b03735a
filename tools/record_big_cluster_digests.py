"""Records SHA-256 digests of what the launch-per-step GEMM kernels (big_step_kernel of esn_big_predict.hip,
bigh_step_kernel of esn_big_harvest.hip) and the harvest cluster kernel (esn_harvest_cluster.hip) write at a few small
shapes into tests/golden/big_cluster_parent_digests.json, for tests/test_gpu_big_cluster_digests.py to compare against: a
clean-up of these kernels that is meant to keep their results keeps every output byte.  Needs a GPU.

Run it with the library of the commit whose results are to be pinned (ESN_HIP_LIB selects another build):

    ESN_HIP_LIB=<that tree>/esn_ofdm_mimo_amd/libesn_hip.so python tools/record_big_cluster_digests.py --commit <hash>

The cases (SHAPES below, each with f16 and bf16 and with noise `none` and `counter`, then each once more with noise
`tensor`, every knob at its default):
  big predict      1100 units, 2 groups of 20 frames with the last group short (one 256-slot tile, 5 row tiles)
  big harvest      1100 units, 65 pilots (a second, nearly empty pilot tile), float64 and float32 extended states
  cluster harvest  512 units with 17 pilots (a partial second cluster), 300 units with a lone pilot, and 3 weight sets
                   with 10 pilots at group_offset 5
The weights are a seeded uniform draw scaled to a spectral radius near 0.9 (no eigenvalue computation), the inputs come
from seeded NumPy generators, so this tool and the test build the same arrays."""
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

GOLDEN = os.path.join(ROOT, "tests", "golden", "big_cluster_parent_digests.json")
SEED = 20261020
# kind, the kernel it must reach (esn_ofdm_mimo_amd._lib.PATHS), n_res, n_in, n_out, sequences, T, then per kind:
# predict: frames per group F, transient; harvest: e_dtype, n_wsets, group_offset
SHAPES = (
    dict(kind="predict", path="big_predict", n_res=1100, n_in=2, n_out=2, B=2 * 20 - 3, T=12, F=20, transient=2),
    dict(kind="harvest", path="big_harvest", n_res=1100, n_in=2, n_out=2, B=65, T=10, e_dtype="f64"),
    dict(kind="harvest", path="big_harvest", n_res=1100, n_in=2, n_out=2, B=65, T=10, e_dtype="f32"),
    dict(kind="harvest", path="harvest_cluster", n_res=512, n_in=16, n_out=8, B=17, T=10),
    dict(kind="harvest", path="harvest_cluster", n_res=300, n_in=16, n_out=8, B=1, T=10),
    dict(kind="harvest", path="harvest_cluster", n_res=512, n_in=16, n_out=8, B=10, T=10, n_wsets=3, group_offset=5),
)
PRECISIONS = ("f16", "bf16")
NOISE_MODES = ("none", "counter")
# appended behind the product of the modes above: the case index seeds the arrays and the kernel, so a mode added to
# NOISE_MODES would move every digest recorded before it
LATER_NOISE_MODES = ("tensor",)


def cases():
    out = []
    for s, precision, noise_mode in itertools.chain(itertools.product(SHAPES, PRECISIONS, NOISE_MODES),
                                                    itertools.product(SHAPES, PRECISIONS, LATER_NOISE_MODES)):
        c = dict(dict(e_dtype="f64", n_wsets=1, group_offset=0), **s, precision=precision, noise_mode=noise_mode)
        c["id"] = "{path}-n{n_res}-b{B}-e{e_dtype}-w{n_wsets}-{precision}-{noise_mode}".format(**c)
        out.append(c)
    assert len({c["id"] for c in out}) == len(out)
    return out


def shape_of(c):
    from esn_ofdm_mimo_amd import _lib
    return _lib.Shape(c["n_res"], c["n_in"], c["n_out"], 1, c["n_wsets"], 0.0)


def path(c):
    """(no GPU) the kernel the library picks for the case when a workspace is lent"""
    from esn_ofdm_mimo_amd import _lib
    harvest = c["kind"] == "harvest"
    return _lib.recur_path(harvest, c["precision"], shape_of(c), c["B"], 1 if harvest else c["F"], True)


def arrays(i, c):
    rng = np.random.default_rng([SEED, i])
    n, n_in, n_out, nw, B, T = c["n_res"], c["n_in"], c["n_out"], c["n_wsets"], c["B"], c["T"]
    G = B if c["kind"] == "harvest" else -(-B // c["F"])
    return dict(
        w=rng.uniform(-1, 1, (nw, n, n)) * (0.9 / np.sqrt(n / 3.0)),       # radius of a uniform matrix: sqrt(n / 3)
        w_in=rng.uniform(-1, 1, (nw, n, n_in)), w_fb=rng.uniform(-1, 1, (nw, n, n_out)),
        w_out=rng.standard_normal((G, n_out, n + n_in)) * 0.004,            # weak feedback
        in_scale=rng.random((G, n_in)) * 0.2 + 0.1, in_shift=rng.standard_normal((G, n_in)) * 0.05,
        t_scale=rng.random((G, n_out)) + 0.5, t_shift=rng.standard_normal((G, n_out)) * 0.1,
        u=rng.standard_normal((B, T, n_in)), d=np.tanh(rng.standard_normal((B, T, n_out))),
        x0=rng.standard_normal((G, n)) * 0.1, y0=rng.standard_normal((G, n_out)) * 0.1,
        noise_u=rng.random((B, T - 1, n) if c["kind"] == "harvest" else (B, T, n)))       # drawn last, read in tensor mode


def digest(i, c):
    """SHA-256 of the raw bytes of Y (predict) or E (harvest) of case i, from the library that
    esn_ofdm_mimo_amd._lib has loaded."""
    from esn_ofdm_mimo_amd import batched
    a = arrays(i, c)
    assert path(c) == c["path"], (c["id"], path(c))
    bank = batched.ReservoirBank(c["n_in"], c["n_out"], c["n_res"], a["w"], a["w_in"], a["w_fb"],
                                 noise=0.0 if c["noise_mode"] == "none" else 1e-3)
    bank.set_scaling(a["in_scale"], a["in_shift"], a["t_scale"], a["t_shift"])
    noise_u = a["noise_u"] if c["noise_mode"] == "tensor" else None
    if c["kind"] == "harvest":
        y = bank.harvest(a["u"], a["d"], precision=c["precision"], noise_mode=c["noise_mode"], noise_u=noise_u,
                         seed=5 + i, e_dtype=c["e_dtype"], group_offset=c["group_offset"])
        if c["path"] == "harvest_cluster":
            bank.raise_if_harvest_timed_out()
        want, dtype = (c["B"], c["T"], c["n_res"] + c["n_in"]), (np.float32 if c["e_dtype"] == "f32" else np.float64)
    else:
        bank.set_readout(a["w_out"])
        y = bank.predict(a["u"], c["F"], T=c["T"], transient=c["transient"], precision=c["precision"], x0=a["x0"],
                         y0=a["y0"], noise_mode=c["noise_mode"], noise_u=noise_u, seed=5 + i)
        want, dtype = (c["B"], c["T"] - c["transient"], c["n_out"]), np.float64
    y = y.cpu().numpy()
    assert y.shape == want and y.dtype == dtype and np.isfinite(y).all(), c["id"]
    return hashlib.sha256(np.ascontiguousarray(y).tobytes()).hexdigest()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--commit", required=True, help="hash of the commit the loaded library was built from")
    ap.add_argument("--out", default=GOLDEN)
    args = ap.parse_args()
    from esn_ofdm_mimo_amd import _lib
    cs = cases()
    doc = {"commit": args.commit, "seed": SEED, "digests": [[c["id"], digest(i, c)] for i, c in enumerate(cs)]}
    # the noise and the precision reach the bytes: no two cases of one shape share a digest
    assert len({d for _, d in doc["digests"]}) == len(cs), "two cases gave the same bytes"
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=0, sort_keys=True)
        f.write("\n")
    print(f"{args.out}: {len(cs)} digests from {_lib.LIB_PATH}")


if __name__ == "__main__":
    main()
