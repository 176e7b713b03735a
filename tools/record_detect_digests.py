"""Records SHA-256 digests of what the detector tail (ReservoirBank.detect_count: detect_count_kernel, and
detect_count_fixed_kernel where the dispatch of launch_detect_count picks it) writes into err, bits and X_hat over the
smallest cases at which the fixed-shape instance can go wrong, into tests/golden/detect_parent_digests.json, for
tests/test_gpu_detect_digests.py to compare against: the fixed instance and the generic kernel behind the shared
helpers keep every output byte of the commit the file names.  Needs a GPU.

Run it with the library of the commit whose results are to be pinned (ESN_HIP_LIB selects another build):

    ESN_HIP_LIB=<that tree>/esn_ofdm_mimo_amd/libesn_hip.so python tools/record_detect_digests.py --commit <hash>

The sample, with K = 8 the frames a workgroup of the fixed instance takes (B frames, F frames per group), at
(N = 128, n_t = 4, 16-QAM) unless named, each with float64 and float32 Y:
  one     B 1, F 1
  ragged  B K - 1, K + 1, 2 K + 3 at F 3: several groups inside a workgroup, a ragged last workgroup
  bound   B 151, F 75: a group boundary inside a workgroup, a last group of one frame
  spread  B 20, F 20: one group over three workgroups
  zero    Y identically zero; negz: Y with row 5 of every frame set to -0.0 (signed zeros through the butterflies)
  twice   two calls into the same counters
  txoff   tx_bits a view one byte into a larger buffer; yoff: Y a view 8 bytes into a larger buffer (the generic
          kernel's alignment fallback; float32 Y at 8 bytes stays on the fixed instance)
  other   N 64, n_t 2, QPSK: a shape the fixed instance does not serve
Inputs are those of tests/test_gpu_io32.py::test_detect_count_f32_matches_widened (Y = 0.7 x normal, random bits,
p_i = 0.5 + uniform per group) from seeded NumPy generators, so this tool and the tests build the same arrays."""
import argparse
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

GOLDEN = os.path.join(ROOT, "tests", "golden", "detect_parent_digests.json")
SEED = 20261018
K = 8                                    # kDetFixedFrames in esn_detect.hip


def cases():
    """The sample, a list of dicts: kind, B, F, n_sub, n_t, m, y32, ymode, twice, tx_off, y_off (bytes)."""
    rows = [("one", 1, 1), ("ragged", K - 1, 3), ("ragged", K + 1, 3), ("ragged", 2 * K + 3, 3), ("bound", 151, 75),
            ("spread", 20, 20)]
    out = []
    for y32 in (False, True):
        base = dict(n_sub=128, n_t=4, m=4, y32=y32, ymode="randn", twice=False, tx_off=0, y_off=0)
        out += [dict(base, kind=k, B=b, F=f) for k, b, f in rows]
        out.append(dict(base, kind="zero", B=K + 1, F=3, ymode="zero"))
        out.append(dict(base, kind="negz", B=K + 1, F=3, ymode="negz"))
        out.append(dict(base, kind="twice", B=K + 1, F=3, twice=True))
        out.append(dict(base, kind="txoff", B=K + 1, F=3, tx_off=1))
        out.append(dict(base, kind="yoff", B=K + 1, F=3, y_off=8))
        out.append(dict(base, kind="other", B=K + 1, F=3, n_sub=64, n_t=2, m=2))
    for c in out:
        c["id"] = f"{c['kind']}-B{c['B']}-F{c['F']}-N{c['n_sub']}x{c['n_t']}m{c['m']}-{'f32' if c['y32'] else 'f64'}"
    assert len({c["id"] for c in out}) == len(out)
    return out


def arrays(i, c):
    """Y [B, N, 2 n_t] (float64 or float32), tx bits uint8 [B, N m, n_t] and p_i [groups] of case i, as NumPy.  The
    float32 and float64 variants of a case share the random stream, as the cases are built in the same order."""
    rs = np.random.RandomState(SEED % (2 ** 31) + i % (len(cases()) // 2))
    B, F, n_sub, n_t, m = c["B"], c["F"], c["n_sub"], c["n_t"], c["m"]
    Y = (rs.randn(B, n_sub, 2 * n_t) * 0.7).astype(np.float32 if c["y32"] else np.float64)
    bits = rs.randint(0, 2, (B, n_sub * m, n_t)).astype(np.uint8)
    p_i = 0.5 + rs.rand((B + F - 1) // F)
    if c["ymode"] == "zero":
        Y[:] = 0.0
    elif c["ymode"] == "negz":
        Y[:, 5, :] = -0.0
    return Y, bits, p_i


def _offset_view(torch, a, off_bytes):
    """device tensor with the values of the NumPy array `a` that starts off_bytes into a larger allocation"""
    t = torch.as_tensor(a, device="cuda")
    if not off_bytes:
        return t
    assert off_bytes % a.itemsize == 0
    skip = off_bytes // a.itemsize
    big = torch.empty(t.numel() + skip, dtype=t.dtype, device="cuda")
    v = big[skip:].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() == big.data_ptr() + off_bytes and v.is_contiguous()
    return v


def run(i, c, want_xhat=True):
    """(err, bits, X_hat or None) device tensors of case i from the library that esn_ofdm_mimo_amd._lib has loaded,
    under whatever knobs are set"""
    import torch
    from esn_ofdm_mimo_amd import batched
    Y, tx, p_i = arrays(i, c)
    n_t = c["n_t"]
    bank = batched.ReservoirBank(2, 2 * n_t, 2, np.zeros((2, 2)), np.zeros((2, 2)), np.zeros((2, 2 * n_t)))
    Yd = _offset_view(torch, Y, c["y_off"])
    txd = _offset_view(torch, tx, c["tx_off"])
    assert (Yd.data_ptr() % 16 == 0) == (c["y_off"] == 0) and (txd.data_ptr() % 16 == 0) == (c["tx_off"] == 0)
    pd = torch.as_tensor(p_i, device="cuda")
    res = bank.detect_count(Yd, txd, pd, c["F"], c["n_sub"], n_t, c["m"], want_xhat=want_xhat)
    if c["twice"]:
        res = bank.detect_count(Yd, txd, pd, c["F"], c["n_sub"], n_t, c["m"], err=res[0], bits=res[1], want_xhat=want_xhat)
    torch.cuda.synchronize()
    return (res[0], res[1], res[2] if want_xhat else None)


def digests(i, c):
    """[SHA-256 of the err bytes, of the bits bytes, of the X_hat bytes] of case i"""
    return [hashlib.sha256(np.ascontiguousarray(t.cpu().numpy()).tobytes()).hexdigest() for t in run(i, c)]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--commit", required=True, help="hash of the commit the loaded library was built from")
    ap.add_argument("--out", default=GOLDEN)
    args = ap.parse_args()
    from esn_ofdm_mimo_amd import _lib
    rows = [[c["id"], *digests(i, c)] for i, c in enumerate(cases())]
    doc = {"commit": args.commit, "seed": SEED, "frames_per_workgroup": K, "digests": rows}
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=0, sort_keys=True)
        f.write("\n")
    print(f"{args.out}: {len(rows)} cases from {_lib.LIB_PATH}")


if __name__ == "__main__":
    main()
