#!/usr/bin/env python3
"""Diagnostic: where the LDS Cholesky read-out solve (readout_chol_kernel, wide float32 E) spends its cycles.
Loads the -DESN_STAMPS build (libesn_hip_stamps.so), solves the headline shape (2048 systems of 128 x 528) once
per arm of the `chol_dma` knob and prints, per wave of workgroup 0, the summed s_memtime cycles of
  Gram:  DMA / load wait | barrier | operand-read latency (dma arm) | MFMA issue
  W_out: DMA wait | barrier | rows (dma arm only)
the phase totals, and the factor phase split into panel + trailing-update MFMAs | its two barrier waits per 16
columns | the diagonal-tile factorisation and inversion (wave 0 only).  Shares only: every stamp waits lgkmcnt(0), which the real kernel does not.

    python tools/chol_stamps.py [--groups 2048]
"""
import argparse
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from esn_ofdm_mimo_amd import _lib, build  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--groups", type=int, default=2048)
    a = ap.parse_args()
    if "ESN_STAMPS_LIB" not in os.environ:
        build.build_library(stamps=True, verbose=False)
    _lib.LIB_PATH = os.path.join(ROOT, "esn_ofdm_mimo_amd", os.environ.get("ESN_STAMPS_LIB", "libesn_hip_stamps.so"))
    from esn_ofdm_mimo_amd import batched
    lib = _lib.load()
    lib.esn_debug_set_stamp_buffer.argtypes = [C.c_void_p]
    buf = torch.zeros(16 * 8, dtype=torch.int64, device="cuda")
    lib.esn_debug_set_stamp_buffer(buf.data_ptr())
    rs = np.random.RandomState(0)
    n_res, n_in, n_out, rows, tr = 512, 16, 8, 139, 11
    bank = batched.ReservoirBank(n_in, n_out, n_res, rs.rand(n_res, n_res) - 0.5, rs.rand(n_res, n_in), rs.rand(n_res, n_out))
    E = torch.randn(a.groups, rows, n_res + n_in, device="cuda", dtype=torch.float32) * 0.1
    D = torch.randn(a.groups, rows, n_out, device="cuda", dtype=torch.float64)
    for dma in ("0", "1"):
        _lib.debug_set("chol_dma", dma)
        bank.solve(E, D, tr, method="chol")
        torch.cuda.synchronize()
        buf.zero_()
        bank.solve(E, D, tr, method="chol")
        torch.cuda.synchronize()
        raw = buf.cpu().numpy().reshape(16, 8)
        print(f"chol_dma={dma}: cycles (s_memtime ticks) per wave of workgroup 0")
        if dma == "1":
            names = ["G wait", "G barrier", "G opread", "G mfma", "W wait", "W barrier", "W rows"]
        else:
            names = ["G ld+commit", "G barrier", "-", "G mfma", "-", "-", "-"]
        print("wave " + " ".join(f"{n:>11s}" for n in names) + " |" +
              " ".join(f"{n:>9s}" for n in ["gram", "factor", "solves", "w_out", "total"]) + " |" +
              " ".join(f"{n:>9s}" for n in ["F mfma", "F barrier", "F diag"]))
        for w in range(8):
            print(f"{w:4d} " + " ".join(f"{x:11d}" for x in raw[w, :7]) + " |" +
                  " ".join(f"{x:9d}" for x in raw[8 + w, :5]) + " |" + " ".join(f"{x:9d}" for x in raw[8 + w, 5:8]))
    _lib.debug_set("chol_dma", "1")


if __name__ == "__main__":
    main()
