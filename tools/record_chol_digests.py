"""Records SHA-256 digests of what the Cholesky read-out solve (ReservoirBank.solve(..., method="chol"): the LDS
kernel readout_chol_kernel up to Gram dimension 128, readout_chol_big_kernel beyond) writes into W_out and status
over the smallest shapes at which its diagonal-block factorisation can go wrong, into
tests/golden/chol_parent_digests.json, for tests/test_gpu_chol_digests.py to compare against: a rewrite of the
factorisation that is meant to keep its results keeps every output byte.  Needs a GPU.

Run it with the library of the commit whose results are to be pinned (ESN_HIP_LIB selects another build):

    ESN_HIP_LIB=<that tree>/esn_ofdm_mimo_amd/libesn_hip.so python tools/record_chol_digests.py --commit <hash>

The sample (rows x cols is the system after the transient; E is seeded randn with three columns scaled by 1e-2):
  wide   one tile and ragged tiles, n = rows in {16, 17, 100, 127, 128} at cols 528, n_out 8, G 3; 40 x 60, n_out 3
  tall   Gram dimension = cols: 300 x 100, 140 x 37, 512 x 128, n_out 8
  tail   of the two-workgroups-per-CU residency: G 5, and G 513 at 128 x 528 float32 (one past a full round)
  drop   a rejected pivot: wide 128 x 528, G 5, row 90 of group 2 a copy of row 41; the same with an all-zero row;
         tall 300 x 100 with a duplicated column -- status 1 for group 2 only, its W_out is part of the digest
  ridge  lambda 0.0 and 1e-3 on one wide and one tall shape (the ridge instances of the kernel)
  big    readout_chol_big_kernel: wide 144 x 528 and 130 x 200, tall 600 x 144, G 2, n_out 8
  w_out  the W_out passes of the LDS kernel that cols 528 and 60 never take, wide, G 3: 40 x 61, n_out 3 (no 16-byte
         runs: scalar Gram fetch and scalar W_out loop); 20 x 600 (float32: DMA Gram, then the scalar loop, three parts
         do not fit the tile area; float64: the vector pass with one part); 20 x 800 (float32: two parts through the
         W_out ring, two rows per chunk)
  big-ridge / big-drop / big   what the three `big` shapes leave out of readout_chol_big_kernel, G 2, n_out 8: its ridge
         instance (144 x 528 and 600 x 144 at lambda 0.0 and 1e-3); a rejected pivot that is exactly 0 (G 5, group 2:
         144 x 528 with row 90 zero, 600 x 144 with column 60 zero); idle substitution waves (130 x 200, n_out 3); one
         live row in the last tile (129 x 528); all eight row slots of a lane (512 x 528)
each with float64 and float32 E, except G 513.  Inputs come from seeded NumPy generators, so this tool and the test
build the same arrays."""
import argparse
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

GOLDEN = os.path.join(ROOT, "tests", "golden", "chol_parent_digests.json")
SEED = 20261017
TRANSIENT = 3
BAD_GROUP = 2


def cases():
    """The sample, a list of dicts: kind, rows, cols, n_out, G, e32, drop (None, "row", "zero", "col", "zerocol"), ridge."""
    shapes = [("wide", n, 528, 8, 3) for n in (16, 17, 100, 127, 128)] + [("wide", 40, 60, 3, 3)]
    shapes += [("tall", 300, 100, 8, 3), ("tall", 140, 37, 8, 3), ("tall", 512, 128, 8, 3)]
    shapes += [("tail", 128, 528, 8, 5)]
    out = [dict(kind=k, rows=r, cols=c, n_out=o, G=g, e32=e32, drop=None, ridge=None)
           for k, r, c, o, g in shapes for e32 in (False, True)]
    out.append(dict(kind="tail", rows=128, cols=528, n_out=8, G=513, e32=True, drop=None, ridge=None))
    for drop, r, c in (("row", 128, 528), ("zero", 128, 528), ("col", 300, 100)):
        out += [dict(kind="drop", rows=r, cols=c, n_out=8, G=5, e32=e32, drop=drop, ridge=None) for e32 in (False, True)]
    for r, c in ((100, 528), (300, 100)):
        out += [dict(kind="ridge", rows=r, cols=c, n_out=8, G=3, e32=e32, drop=None, ridge=lam)
                for lam in (0.0, 1e-3) for e32 in (False, True)]
    for r, c in ((144, 528), (130, 200), (600, 144)):
        out += [dict(kind="big", rows=r, cols=c, n_out=8, G=2, e32=e32, drop=None, ridge=None) for e32 in (False, True)]
    # the W_out paths no shape above takes (appended: inputs are seeded by case index)
    for r, c, o in ((40, 61, 3), (20, 600, 8), (20, 800, 8)):
        out += [dict(kind="wide", rows=r, cols=c, n_out=o, G=3, e32=e32, drop=None, ridge=None) for e32 in (False, True)]
    # readout_chol_big_kernel beyond the three `big` shapes (appended)
    for r, c in ((144, 528), (600, 144)):
        out += [dict(kind="big-ridge", rows=r, cols=c, n_out=8, G=2, e32=e32, drop=None, ridge=lam)
                for lam in (0.0, 1e-3) for e32 in (False, True)]
    for drop, r, c in (("zero", 144, 528), ("zerocol", 600, 144)):
        out += [dict(kind="big-drop", rows=r, cols=c, n_out=8, G=5, e32=e32, drop=drop, ridge=None) for e32 in (False, True)]
    for r, c, o in ((130, 200, 3), (129, 528, 8), (512, 528, 8)):
        out += [dict(kind="big", rows=r, cols=c, n_out=o, G=2, e32=e32, drop=None, ridge=None) for e32 in (False, True)]
    for c in out:
        c["id"] = (f"{c['kind']}-{c['rows']}x{c['cols']}-o{c['n_out']}-G{c['G']}-{'f32' if c['e32'] else 'f64'}"
                   + (f"-drop_{c['drop']}" if c["drop"] else "") + (f"-ridge{c['ridge']:g}" if c["ridge"] is not None else ""))
    assert len({c["id"] for c in out}) == len(out)
    return out


def arrays(i, c):
    """E [G, TRANSIENT + rows, cols] (float64 or float32), D and t_scale of case i."""
    rng = np.random.default_rng([SEED, i])
    G, t = c["G"], c["rows"] + TRANSIENT
    dt = np.float32 if c["e32"] else np.float64
    E = rng.standard_normal((G, t, c["cols"]), dtype=dt)
    E[:, :, :3] *= dt(1e-2)                                   # uneven column scales
    D = rng.standard_normal((G, t, c["n_out"]))
    t_scale = rng.random((G, c["n_out"])) + 0.5
    if c["drop"] == "row":
        E[BAD_GROUP, TRANSIENT + 90] = E[BAD_GROUP, TRANSIENT + 41]
        D[BAD_GROUP, TRANSIENT + 90] = D[BAD_GROUP, TRANSIENT + 41]
    elif c["drop"] == "zero":
        E[BAD_GROUP, TRANSIENT + 90] = 0
    elif c["drop"] == "col":
        E[BAD_GROUP, :, 60] = E[BAD_GROUP, :, 17]
    elif c["drop"] == "zerocol":
        E[BAD_GROUP, :, 60] = 0
    return E, D, t_scale


def expected_status(c):
    st = [0] * c["G"]
    if c["drop"]:
        st[BAD_GROUP] = 1
    return st


def digests(i, c):
    """(SHA-256 of the W_out bytes, SHA-256 of the status bytes, status as a list) of case i, from the library that
    esn_ofdm_mimo_amd._lib has loaded."""
    import torch
    from esn_ofdm_mimo_amd import batched
    E, D, t_scale = arrays(i, c)
    cols, n_out = c["cols"], c["n_out"]
    bank = batched.ReservoirBank(cols - 2, n_out, 2, np.zeros((2, 2)), np.zeros((2, cols - 2)), np.zeros((2, n_out)))
    bank.set_scaling(None, None, t_scale, None)
    W, status = bank.solve(torch.as_tensor(E, device="cuda"), D, TRANSIENT, method="chol", ridge=c["ridge"])
    W, status = W.cpu().numpy(), status.cpu().numpy()
    assert W.shape == (c["G"], n_out, cols) and W.dtype == np.float64 and status.dtype == np.int32, c["id"]
    return (hashlib.sha256(np.ascontiguousarray(W).tobytes()).hexdigest(),
            hashlib.sha256(np.ascontiguousarray(status).tobytes()).hexdigest(), [int(s) for s in status])


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--commit", required=True, help="hash of the commit the loaded library was built from")
    ap.add_argument("--out", default=GOLDEN)
    args = ap.parse_args()
    from esn_ofdm_mimo_amd import _lib
    rows = []
    for i, c in enumerate(cases()):
        w, s, st = digests(i, c)
        # a sample whose healthy groups are flagged (or whose singular one is not) is a wrong sample
        assert st == expected_status(c), (c["id"], st)
        rows.append([c["id"], w, s])
    doc = {"commit": args.commit, "seed": SEED, "transient": TRANSIENT, "digests": rows}
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=0, sort_keys=True)
        f.write("\n")
    print(f"{args.out}: {len(rows)} cases from {_lib.LIB_PATH}")


if __name__ == "__main__":
    main()
