"""Records SHA-256 digests of what the solve of the running normal equations (ReservoirBank.gram_solve:
gram_solve_kernel in esn_gram.hip) writes into W_out and status, into tests/golden/gram_solve_parent_digests.json, for
tests/test_gpu_gram_solve_digests.py to compare against: a rewrite of its factorisation or substitutions that is meant
to keep the results keeps every output byte.  Needs a GPU.

Run it with the library of the commit whose results are to be pinned (ESN_HIP_LIB selects another build):

    ESN_HIP_LIB=<that tree>/esn_ofdm_mimo_amd/libesn_hip.so python tools/record_gram_solve_digests.py --commit <hash>

The state is built on the host, so the accumulate kernel is not in the digest: Gm = E^T E and Cm = D^T E in float64
NumPy from a seeded E [G, rows, cols] and D [G, rows, n_out] (rounded to multiples of 2^-10, so both products are exact
whatever the host's BLAS does), G = 3, rows = 2 cols (128 rows at cols 528 and 544: a rank-deficient Gm that only lambda
makes definite).  lambda[g][l] = cols * (1e-3, 1e-1, 10)[(g + l) % 3], a different
one per group and candidate, except in the last two cases.  (cols, n_out, candidates):
  5, 1, 1      the smallest ragged tile
  16, 2, 2     one exact tile
  17, 4, 2     one column past a tile
  132, 9, 3    more right-hand sides than waves: the second trip of the substitution loop
  528, 8, 2    the ninth row slot of a lane
  544, 16, 1   the limit of both
  132, 8, 2    lambdas (0, 1e-3) and column 7 of E zero in group 1: pivot 7 is exactly 0 at lambda 0, that entry alone is
               flagged (status 1, its W_out zero)
  17, 4, 3     lambdas (1e-3, -1, NaN): status (0, 2, 2) in every group"""
import argparse
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

GOLDEN = os.path.join(ROOT, "tests", "golden", "gram_solve_parent_digests.json")
SEED = 20261020
G = 3
LAMBDA_SCALES = (1e-3, 1e-1, 10.0)
ZERO_GROUP, ZERO_COL = 1, 7


def cases():
    """The sample, a list of dicts: cols, n_out, L, special (None, "zero_pivot", "bad_lambda")."""
    out = [dict(cols=c, n_out=o, L=nl, special=None)
           for c, o, nl in ((5, 1, 1), (16, 2, 2), (17, 4, 2), (132, 9, 3), (528, 8, 2), (544, 16, 1))]
    out.append(dict(cols=132, n_out=8, L=2, special="zero_pivot"))
    out.append(dict(cols=17, n_out=4, L=3, special="bad_lambda"))
    for c in out:
        c["id"] = f"{c['cols']}-o{c['n_out']}-L{c['L']}" + (f"-{c['special']}" if c["special"] else "")
    assert len({c["id"] for c in out}) == len(out)
    return out


def arrays(i, c):
    """Gm [G, cols, cols], Cm [G, n_out, cols] and lambda [G, L] of case i, float64."""
    rng = np.random.default_rng([SEED, i])
    cols = c["cols"]
    rows = 128 if cols >= 528 else 2 * cols
    # multiples of 2^-10 below 8: every product and every partial sum of E^T E and D^T E is exact in float64, so Gm and
    # Cm do not depend on the order in which the host's BLAS adds, and Gm is symmetric bit for bit
    E = np.round(rng.standard_normal((G, rows, cols)) * 1024.0) / 1024.0
    D = np.round(rng.standard_normal((G, rows, c["n_out"])) * 1024.0) / 1024.0
    if c["special"] == "zero_pivot":
        E[ZERO_GROUP, :, ZERO_COL] = 0.0
        lam = np.tile(np.array([0.0, 1e-3]), (G, 1))
    elif c["special"] == "bad_lambda":
        lam = np.tile(np.array([1e-3, -1.0, np.nan]), (G, 1))
    else:
        lam = cols * np.array([[LAMBDA_SCALES[(g + l) % 3] for l in range(c["L"])] for g in range(G)])
    Et = E.transpose(0, 2, 1)
    return np.ascontiguousarray(Et @ E), np.ascontiguousarray(D.transpose(0, 2, 1) @ E), lam


def expected_status(c):
    st = [[0] * c["L"] for _ in range(G)]
    if c["special"] == "zero_pivot":
        st[ZERO_GROUP][0] = 1
    elif c["special"] == "bad_lambda":
        st = [[0, 2, 2] for _ in range(G)]
    return st


def digests(i, c):
    """(SHA-256 of the W_out bytes, SHA-256 of the status bytes, status as nested lists) of case i, from the library
    that esn_ofdm_mimo_amd._lib has loaded."""
    import torch
    from esn_ofdm_mimo_amd import batched
    Gm, Cm, lam = arrays(i, c)
    cols, n_out = c["cols"], c["n_out"]
    bank = batched.ReservoirBank(1, n_out, 2, np.zeros((2, 2)), np.zeros((2, 1)), np.zeros((2, n_out)))
    state = batched.GramState(torch.as_tensor(Gm, device="cuda"), torch.as_tensor(Cm, device="cuda"), None, None)
    W, status = bank.gram_solve(state, lam)
    W, status = W.cpu().numpy(), status.cpu().numpy()
    assert W.shape == (G, c["L"], n_out, cols) and W.dtype == np.float64 and status.dtype == np.int32, c["id"]
    return (hashlib.sha256(np.ascontiguousarray(W).tobytes()).hexdigest(),
            hashlib.sha256(np.ascontiguousarray(status).tobytes()).hexdigest(), status.tolist())


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--commit", required=True, help="hash of the commit the loaded library was built from")
    ap.add_argument("--out", default=GOLDEN)
    args = ap.parse_args()
    from esn_ofdm_mimo_amd import _lib
    rows = []
    for i, c in enumerate(cases()):
        w, s, st = digests(i, c)
        # a sample that flags a healthy entry (or passes the singular one) is a wrong sample
        assert st == expected_status(c), (c["id"], st)
        rows.append([c["id"], w, s])
    doc = {"commit": args.commit, "seed": SEED, "digests": rows}
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=0, sort_keys=True)
        f.write("\n")
    print(f"{args.out}: {len(rows)} cases from {_lib.LIB_PATH}")


if __name__ == "__main__":
    main()
