"""Records SHA-256 digests of the two W_out that ReservoirBank.solve(method="chol") writes for one set of extended states
given as float32 and as the same values widened to float64, with the relative difference between the two, into
tests/golden/readout_path_parent_digests.json for tests/test_gpu_readout_path.py: both storage types go through one
call path, and a rewrite of that path that is meant to keep the results keeps every byte of both.  Needs a GPU.

Run it from the tree of the commit whose results are to be pinned (the package next to this tool is the one loaded):

    python tools/record_readout_path_digests.py --commit <hash>

The shape is the small one of that test: G 3, n_reservoir 20, n_inputs 4 (24 columns), n_outputs 2, T 45, transient 5,
per-group teacher scale and shift; inputs from a seeded NumPy generator, so this tool and the test build the same arrays."""
import argparse
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

GOLDEN = os.path.join(ROOT, "tests", "golden", "readout_path_parent_digests.json")
SEED = 20261018
G, N_RES, N_IN, N_OUT, T, TRANSIENT = 3, 20, 4, 2, 45, 5


def arrays(n_res=N_RES, t=T):
    """E [G, t, n_res + N_IN], D [G, t, N_OUT], t_scale and t_shift [G, N_OUT], all float64."""
    rng = np.random.default_rng([SEED, n_res, t])
    E = rng.standard_normal((G, t, n_res + N_IN))
    D = rng.standard_normal((G, t, N_OUT))
    return E, D, rng.random((G, N_OUT)) + 0.5, rng.standard_normal((G, N_OUT))


def bank_for(n_res=N_RES, t=T):
    """(bank with the per-group teacher scalings set, E, D); the reservoir itself is not used by solve."""
    from esn_ofdm_mimo_amd import batched
    E, D, t_scale, t_shift = arrays(n_res, t)
    bank = batched.ReservoirBank(N_IN, N_OUT, n_res, np.zeros((n_res, n_res)), np.zeros((n_res, N_IN)),
                                 np.zeros((n_res, N_OUT)))
    bank.set_scaling(None, None, t_scale, t_shift)
    return bank, E, D


def f32_f64_pair():
    """(digest of W_out from float32 E, digest of W_out from the same E widened to float64, max |difference| over
    max |W_out|), from the package next to this tool."""
    import torch
    bank, E, D = bank_for()
    E32 = torch.as_tensor(E, device="cuda").float()
    W32, st32 = bank.solve(E32, D, TRANSIENT, method="chol")
    W64, st64 = bank.solve(E32.double(), D, TRANSIENT, method="chol")
    assert st32.cpu().tolist() == st64.cpu().tolist() == [0] * G
    W32, W64 = W32.cpu().numpy(), W64.cpu().numpy()
    return (hashlib.sha256(np.ascontiguousarray(W32).tobytes()).hexdigest(),
            hashlib.sha256(np.ascontiguousarray(W64).tobytes()).hexdigest(),
            float(np.abs(W32 - W64).max() / np.abs(W64).max()))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--commit", required=True, help="hash of the commit this tree is")
    ap.add_argument("--out", default=GOLDEN)
    args = ap.parse_args()
    d32, d64, rel = f32_f64_pair()
    with open(args.out, "w") as f:
        json.dump({"commit": args.commit, "seed": SEED, "w_out_f32_states": d32, "w_out_f64_states": d64,
                   "relative_difference": rel}, f, indent=0, sort_keys=True)
        f.write("\n")
    print(f"{args.out}: float32 / float64 states differ by {rel:.3e} relative")


if __name__ == "__main__":
    main()
